"""The annotation-file readers (data_loaders/pascal.py, coco.py, inferred.py), their epoch order / sharding / resume
(data_loaders/files.py), the host JPEG decode (dataset.decode_image) and the train CLI's dataset flags -- CPU only, on
fixtures written into tmp_path."""
import itertools
import json
import os

import numpy as np
import pytest

import files_fixtures as ff

SIZES = [(48, 64), (64, 48), (40, 40), (48, 64)]


@pytest.fixture
def voc(tmp_path):
    pytest.importorskip('PIL')
    samples = ff.render(SIZES)
    root = str(tmp_path / 'voc')
    names = ff.write_voc(root, samples)
    return root, names, samples


def _same(a, b):
    assert a['image_file'] == b['image_file']
    assert a['image_size'] == b['image_size']
    np.testing.assert_array_equal(a['boxes'], b['boxes'])
    np.testing.assert_array_equal(a['class_ids'], b['class_ids'])
    assert a['boxes'].dtype == np.float32 and a['boxes'].shape[1] == 4


def test_pascal_yields_the_reference_samples(voc):
    from data_loaders.pascal import Pascal
    root, names, samples = voc
    dl = Pascal(root, 'trainval')
    assert dl.num_classes == 20 and dl.class_names[:3] == ff.VOC_NAMES
    got = list(dl)
    assert len(got) == len(samples)
    for name, g, (image, boxes, ids) in zip(names, got, samples):          # annotation order, every object kept
        assert g['image_file'] == os.path.join(root, 'JPEGImages', name + '.jpg')
        assert g['image_size'] == image.shape[:2]
        np.testing.assert_array_equal(g['boxes'], boxes)                     # [ymin, xmin, ymax, xmax], no 1-based shift
        np.testing.assert_array_equal(g['class_ids'], ids)
    assert dl.max_objects() == max(len(s[2]) for s in samples)
    assert dl.max_image_pixels() == 64 * 48


def test_coco_yields_the_reference_samples_and_matches_pascal(voc, tmp_path):
    from data_loaders.coco import COCO
    from data_loaders.pascal import Pascal
    root, names, samples = voc
    img_dir = os.path.join(root, 'JPEGImages')
    ann = ff.write_coco(str(tmp_path / 'ann.json'), img_dir, samples, names)
    dl = COCO(ann, img_dir)
    assert dl.num_classes == 3 and dl.class_names == ff.VOC_NAMES          # category ids in sorted order: 3, 7, 11
    got = list(dl)
    for g, p in zip(got, Pascal(root, 'trainval')):
        _same(g, p)
    assert len(got) == len(samples)


def test_coco_drops_crowd_and_small_boxes_and_inferred_skips_empty_images(voc, tmp_path):
    from data_loaders.coco import COCO
    from data_loaders.inferred import Inferred
    root, names, samples = voc
    img_dir = os.path.join(root, 'JPEGImages')
    extra = [{'image_id': 100, 'category_id': 7, 'iscrowd': 1, 'bbox': [1.0, 2.0, 10.0, 10.0]},     # crowd
             {'image_id': 101, 'category_id': 3, 'iscrowd': 0, 'bbox': [1.0, 2.0, 0.5, 10.0]},      # 0.5 pixel wide
             {'image_id': 999, 'category_id': 11, 'iscrowd': 0, 'bbox': [3.0, 4.0, 5.0, 0.5]}]      # its only box dropped
    ann = ff.write_coco(str(tmp_path / 'ann.json'), img_dir, samples, names, extra_annotations=extra,
                        extra_images=[{'id': 999, 'file_name': 'empty.jpg', 'height': 30, 'width': 30}])
    got = list(COCO(ann, img_dir))
    assert len(got) == len(samples) + 1 and len(got[-1]['class_ids']) == 0
    for g, (_, boxes, _) in zip(got, samples):
        assert len(g['boxes']) == len(boxes)
    dl = Inferred('coco', [ann, img_dir])
    assert dl.skipped == 1 and len(list(dl)) == len(samples)


def test_coco_bbox_conversion(tmp_path):
    from data_loaders.coco import COCO
    data = {'images': [{'id': 5, 'file_name': 'a.jpg', 'height': 20, 'width': 30}],
            'annotations': [{'id': 1, 'image_id': 5, 'category_id': 9, 'iscrowd': 0, 'bbox': [2.5, 3.0, 4.0, 6.5]}],
            'categories': [{'id': 9, 'name': 'x'}, {'id': 2, 'name': 'y'}]}
    path = str(tmp_path / 'a.json')
    with open(path, 'w') as f:
        json.dump(data, f)
    (s,) = list(COCO(path, '/img'))
    np.testing.assert_array_equal(s['boxes'], [[3.0, 2.5, 9.5, 6.5]])       # [y, x, y + h, x + w]
    assert s['class_ids'].tolist() == [1] and s['image_size'] == (20, 30) and s['image_file'] == os.path.join('/img', 'a.jpg')


def test_pascal_unknown_class_names_the_file_and_zero_width_box_is_skipped(voc, tmp_path):
    from data_loaders.inferred import Inferred
    from data_loaders.pascal import Pascal
    root, names, samples = voc
    bad = str(tmp_path / 'bad')
    ff.write_voc(bad, samples[:2], extra_objects={names[1]: '<object><name>unicorn</name><bndbox><xmin>1</xmin><ymin>1</ymin>'
                                                             '<xmax>5</xmax><ymax>5</ymax></bndbox></object>'})
    with pytest.raises(ValueError, match=names[1] + r'\.xml'):
        Pascal(bad, 'trainval')
    zero = str(tmp_path / 'zero')
    ff.write_voc(zero, samples[:2], extra_objects={names[0]: '<object><name>bird</name><bndbox><xmin>7</xmin><ymin>1</ymin>'
                                                              '<xmax>7</xmax><ymax>5</ymax></bndbox></object>'})
    dl = Inferred('pascal', [zero, 'trainval'])
    assert dl.skipped == 1
    got = list(dl)
    assert len(got) == 1 and got[0]['image_file'].endswith(names[1] + '.jpg')


def test_inferred_dispatch(voc, tmp_path):
    from data_loaders.coco import COCO
    from data_loaders.inferred import Inferred
    from data_loaders.pascal import Pascal
    from data_loaders.shapes import Shapes
    root, names, samples = voc
    assert isinstance(Inferred('pascal', [root, 'trainval']).loader, Pascal)
    ann = ff.write_coco(str(tmp_path / 'a.json'), root, samples, names)
    assert isinstance(Inferred('coco', [ann, root]).loader, COCO)
    sh = Inferred('shapes', [None, '3', '40'])
    assert isinstance(sh.loader, Shapes) and sh.num_classes == 3
    got = list(sh)
    assert len(got) == 3 and got[0]['image'].shape == (40, 40, 3)
    with pytest.raises(ValueError, match='unknown dataset type'):
        Inferred('imagenet', [])


# ---- epoch order, sharding, resume (data_loaders/files.py) on synthetic records

def _records(n, seed=0):
    from data_loaders.files import FileDataset
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 375), (333, 500), (500, 500), (480, 640), (281, 500)]

    class Fake(FileDataset):
        def __init__(self):
            super(Fake, self).__init__()
            self._class_names = ['a', 'b']
            self._keep({'image_file': 'img%d.jpg' % i, 'boxes': np.array([[1, 2, 3, 4]] * (1 + i % 3), np.float32),
                        'class_ids': np.zeros(1 + i % 3, np.int32), 'image_size': sizes[int(rng.integers(len(sizes)))]}
                       for i in range(n))
    return Fake()


def _files(it, k):
    return [s['image_file'] for s in itertools.islice(it, k)]


def test_epochs_are_permutations_and_shards_partition_them():
    n = 37
    dl = _records(n).configure(seed=3, repeat=True)
    stream = _files(iter(dl), 3 * n)
    for e in range(3):
        ep = stream[e * n:(e + 1) * n]
        assert sorted(ep) == sorted('img%d.jpg' % i for i in range(n))
    assert stream[:n] != stream[n:2 * n]                                     # a new order per epoch
    assert _files(iter(_records(n).configure(seed=3, repeat=True)), n) == stream[:n]      # deterministic per seed
    world = 3
    shards = [_files(iter(_records(n).configure(seed=3, rank=r, world=world)), n) for r in range(world)]
    assert sum(len(s) for s in shards) == n
    assert sorted(sum(shards, [])) == sorted(stream[:n])
    for r in range(world):
        assert shards[r] == stream[r:n:world]                                # sample i goes to rank i % world
    dl = _records(5)
    assert _files(iter(dl), 10) == ['img%d.jpg' % i for i in range(5)]      # unconfigured: one pass in annotation order
    assert dl.max_objects() == 3 and dl.max_image_pixels() == max(r['image_size'][0] * r['image_size'][1] for r in dl.records)


@pytest.mark.parametrize('shape_runs', [0, 4])
def test_skip_equals_dropping_samples_across_epochs(shape_runs):
    n = 23
    cfg = dict(seed=5, rank=1, world=2, repeat=True, shape_runs=shape_runs, scale=96)
    full = _files(iter(_records(n).configure(**cfg)), 40)
    for k in (0, 7, 11, 12, 30):
        dl = _records(n).configure(**cfg)
        dl.skip(k)
        assert _files(iter(dl), 40 - k) == full[k:], k


def test_shape_runs_cover_every_sample_in_runs_of_at_most_k():
    import dataset
    from data_loaders import files
    n, k = 1100, 8                                                           # three windows of up to 512 samples
    dl = _records(n).configure(seed=1, shape_runs=k, scale=96)
    order = dl.epoch_order(0)
    assert sorted(order) == list(range(n))
    assert order == _records(n).configure(seed=1, shape_runs=k, scale=96).epoch_order(0)
    assert order != _records(n).configure(seed=2, shape_runs=k, scale=96).epoch_order(0)
    plain = _records(n).configure(seed=1).epoch_order(0)
    for w0 in range(0, n, files.WINDOW):                                     # a window holds the same samples as the plain order's
        assert sorted(order[w0:w0 + files.WINDOW]) == sorted(plain[w0:w0 + files.WINDOW])
    keys = [dataset.rescale_size(dl.records[i]['image_size'], 96) for i in range(n)]
    chunks = files.shape_run_order(keys[:100], k, seed=0)
    assert sorted(sum(chunks, [])) == list(range(100))
    assert all(1 <= len(c) <= k and len({keys[i] for i in c}) == 1 for c in chunks)
    # consecutive same-size runs are long: far fewer shape changes than in the plain order
    changes = lambda o: sum(keys[a] != keys[b] for a, b in zip(o, o[1:]))
    assert changes(order) < changes(plain) // 2


# ---- host decode

def test_decode_image_equals_pillow_and_grey_has_three_equal_channels(tmp_path):
    PIL = pytest.importorskip('PIL')
    from PIL import Image
    import dataset
    rgb = ff.render([(37, 53)])[0][0]
    p = str(tmp_path / 'a.jpg')
    Image.fromarray(rgb).save(p, quality=90)
    got = dataset.decode_image(p)
    assert got.dtype == np.uint8 and got.shape == (37, 53, 3)
    np.testing.assert_array_equal(got, np.asarray(Image.open(p).convert('RGB')))
    g = str(tmp_path / 'g.jpg')
    Image.fromarray(rgb[..., 0]).save(g)
    grey = dataset.decode_image(g.encode('utf-8'))                           # the reference's samples carry bytes paths
    assert grey.shape == (37, 53, 3) and (grey[..., 0] == grey[..., 1]).all() and (grey[..., 1] == grey[..., 2]).all()
    png = str(tmp_path / 'c.png')
    Image.fromarray(rgb).save(png)
    np.testing.assert_array_equal(dataset.decode_image(png), rgb)             # PNG is accepted, lossless
    assert PIL is not None


def test_decoded_pool_keeps_order_and_decoded_size_wins(voc):
    import dataset
    from data_loaders.pascal import Pascal
    root, names, samples = voc
    dl = Pascal(root, 'trainval')
    dl.records[0]['image_size'] = (1, 1)                                     # a wrong annotation
    got = list(dataset.decoded(dl, workers=3))
    assert [g['image'].shape[:2] for g in got] == [s[0].shape[:2] for s in samples]
    assert got[0]['image_size'] == samples[0][0].shape[:2]
    for g in got:
        np.testing.assert_array_equal(g['image'], dataset.decode_image(g['image_file']))
    passthrough = [{'image': np.zeros((2, 2, 3), np.uint8), 'i': i} for i in range(5)]
    assert [s['i'] for s in dataset.decoded(passthrough)] == list(range(5))


# ---- CLI

def test_parser_accepts_the_file_dataset_flags():
    import train
    p = train.build_parser()
    a = p.parse_args(['--dataset', 'pascal', '/d/VOC2012', 'trainval', '--shape-runs', '4', '--decode-workers', '6',
                      '--eval-dataset', 'pascal', '/d/VOC2007', 'test', '--eval-images', '10'])
    assert a.dataset == ['pascal', '/d/VOC2012', 'trainval'] and a.shape_runs == 4 and a.decode_workers == 6
    assert a.eval_dataset == ['pascal', '/d/VOC2007', 'test'] and a.eval_images == 10
    a = p.parse_args(['--dataset', 'coco', 'ann.json', 'images'])
    assert a.dataset == ['coco', 'ann.json', 'images'] and a.shape_runs is None and a.steps_per_epoch is None
    a = p.parse_args(['--dataset', 'shapes', './tmp', '10', '96'])
    assert a.dataset == ['shapes', './tmp', '10', '96']
    a = p.parse_args([])
    assert a.dataset == ['shapes'] and a.eval_dataset is None and a.decode_workers == 4


def test_main_rejects_bad_dataset_arguments_before_touching_the_gpu():
    import train
    with pytest.raises(SystemExit):
        train.main(['--dataset', 'pascal', 'only_root'])
    with pytest.raises(SystemExit):
        train.main(['--dataset', 'imagenet', 'a', 'b'])
    with pytest.raises(SystemExit):                                          # a file dataset's eval needs --eval-dataset
        train.main(['--dataset', 'coco', 'a.json', 'img', '--eval-images', '4'])
