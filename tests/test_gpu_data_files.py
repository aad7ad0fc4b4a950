"""Real-image training on the MI355X: the one-pass raw-image -> [image, hflip] kernel (rn_resize_pair_u8), the ragged staging
of dataset.DeviceFeed (one captured graph set per NETWORK input shape) and train.main on a VOC tree written at test time."""
import os

import numpy as np
import pytest
import torch

from oracle import dataset_ref

pytestmark = pytest.mark.gpu

RAW_SIZES = [(37, 53), (53, 37), (1, 9), (9, 1), (375, 500), (333, 500)]


def _expected_pair(img, size):
    import augmentation
    import dataset
    slot0 = dataset.rescale_image(img, size=size, normalize=True)
    return torch.stack([slot0, augmentation._flip(slot0, 1)])


def test_resize_pair_u8_is_rescale_plus_flip_eager_and_in_one_graph():
    import dataset
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for h, w in RAW_SIZES]
    for img, (h, w) in zip(images, RAW_SIZES):
        for size in ((h, w), dataset.rescale_size((h, w), 96), (1, 1), (5, 1)):
            raw = img.reshape(-1)
            desc = torch.from_numpy(dataset.resize_desc((h, w), size)).to(dev)
            got = dataset.resize_pair_u8(raw, desc, size)
            assert torch.equal(got, _expected_pair(img, size)), ((h, w), size)
    # one capture, replayed after staging other raw sizes (that map to the same output size) into the same capacity buffer
    size = (64, 80)
    cap = max(h * w * 3 for h, w in RAW_SIZES)
    raw = torch.zeros(cap, dtype=torch.uint8, device=dev)
    desc = torch.zeros(4, dtype=torch.int32, device=dev)
    pair = torch.empty((2,) + size + (3,), dtype=torch.float32, device=dev)

    def stage(i):
        h, w = RAW_SIZES[i]
        raw[:h * w * 3].copy_(images[i].reshape(-1))
        desc.copy_(torch.from_numpy(dataset.resize_desc((h, w), size)))

    stage(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dataset.resize_pair_u8(raw, desc, size, out=pair)                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dataset.resize_pair_u8(raw, desc, size, out=pair)
    for i in (4, 1, 5, 0, 2):
        stage(i)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(pair, _expected_pair(images[i], size)), RAW_SIZES[i]


def test_decoded_sample_through_the_ragged_feed_equals_the_oracle(tmp_path):
    """Slot 0 of the staged + captured-path features == the oracle's preprocess_image(rescale_image(...)) of the decoded JPEG,
    and the labels == the oracle's build_labels (slot 0) and their flip (slot 1): classes and masks bit for bit, the regression
    targets to fp32 rounding."""
    pytest.importorskip('PIL')
    import dataset
    import files_fixtures as ff
    import levels as levels_mod
    from data_loaders.pascal import Pascal
    dev = torch.device('cuda:0')
    root = str(tmp_path / 'voc')
    ff.write_voc(root, ff.render([(75, 100)], seed=4))
    lv = levels_mod.build_levels()
    dl = Pascal(root, 'trainval')
    feed = dataset.DeviceFeed(dl, lv, scale=64, device=dev, ragged=True)
    try:
        feed.stage()
        b = feed.features()
        feed.consumed()
        torch.cuda.synchronize()
    finally:
        feed.close()
    sample = next(iter(Pascal(root, 'trainval')))
    img = dataset.decode_image(sample['image_file'])
    ref = dataset_ref.preprocess_image(dataset_ref.rescale_image(img, 64))
    assert b['image_size'] == ref.shape[:2] == (64, 85)
    assert np.array_equal(b['image'][0].cpu().numpy(), ref)
    assert np.array_equal(b['image'][1].cpu().numpy(), ref[:, ::-1])
    h, w = img.shape[:2]
    boxes = sample['boxes'] / np.asarray([h, w, h, w], np.float32)
    cls, reg, msk = dataset_ref.build_labels(ref.shape[:2], sample['class_ids'], boxes, dl.num_classes)
    fc, fr, fm, _ = dataset_ref.flip(cls, reg, msk)
    for k in lv:
        for slot, (c, r, m) in enumerate(((cls, reg, msk), (fc, fr, fm))):
            assert np.array_equal(b['detection']['classifications'][k][slot].cpu().numpy(), c[k]), (k, slot)
            # the targets' log / division: the device and numpy round differently in the last bit (as in test_gpu_ops)
            np.testing.assert_allclose(b['detection']['regressions'][k][slot].cpu().numpy(), r[k], rtol=1e-5, atol=1e-6)
            assert np.array_equal(b['trainable_masks'][k][slot].cpu().numpy().astype(bool), m[k].astype(bool)), (k, slot)


class _Ragged(object):
    """6 in-memory uint8 samples, 4 raw sizes, 2 network input sizes at scale 64: (80, 64) and (64, 80)."""
    class_names = ['square', 'triangle', 'circle']
    num_classes = 3
    SIZES = [(100, 80), (80, 100), (101, 81), (100, 80), (81, 101), (80, 100)]

    def __iter__(self):
        from data_loaders.shapes import Shapes
        for i, hw in enumerate(self.SIZES):
            yield next(iter(Shapes(None, 1, image_size=hw, seed=40 + i)))

    def max_image_pixels(self):
        return max(h * w for h, w in self.SIZES)

    def max_objects(self):
        return 4


def test_ragged_feed_graph_steps_equal_eager_steps_with_one_graph_per_input_shape():
    import dataset, layers, levels as levels_mod, retinanet, train
    dev = torch.device('cuda:0')
    lv = levels_mod.build_levels()

    def net():
        torch.manual_seed(0)
        layers.Dropout._next_seed[0] = 0x5EED
        return retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0).to(dev)

    eager = train.Trainer(net(), lv, learning_rate=1e-2, device=dev, use_graph=False)
    want = [eager.step(b)['class_loss'].item() for b in dataset.build_dataset(_Ragged(), lv, scale=64, device=dev)]
    torch.cuda.synchronize()
    feed = dataset.DeviceFeed(_Ragged(), lv, scale=64, device=dev, ragged=True)
    tr = train.Trainer(net(), lv, learning_rate=1e-2, device=dev, use_graph=True, input_fn=feed)
    keys = []
    try:
        got = []
        for _ in range(6):
            got.append(tr.step()['class_loss'].item())
            keys.append(feed.shape_key)
        with pytest.raises(StopIteration):
            tr.step()
    finally:
        feed.close()
    torch.cuda.synchronize()
    assert len(set(got)) == 6 and all(np.isfinite(got))
    assert got == want
    assert torch.equal(tr.arena.weights, eager.arena.weights)
    assert len({k[:2] for k in keys}) == 2 and len(set(keys)) == 2
    assert tr.recaptures == 1 and len(tr._graph_cache) == 2
    assert feed.generations == 1 and feed.samples_staged == 6


def test_train_main_on_a_voc_tree_trains_saves_resumes_and_evaluates(tmp_path, capsys):
    pytest.importorskip('PIL')
    import files_fixtures as ff
    import train
    root = str(tmp_path / 'voc')
    ff.write_voc(root, ff.render([(120, 160), (160, 120), (100, 133), (120, 160), (150, 150), (160, 120)], seed=7))
    exp = str(tmp_path / 'exp')
    argv = ['--dataset', 'pascal', root, 'trainval', '--scale', '96', '--epochs', '1', '--experiment', exp,
            '--backbone', 'mobilenet_v2', '--dropout', '0.1', '--shape-runs', '4']
    assert train.main(argv) == 6                                          # one pass over the 6 images
    out = capsys.readouterr().out
    assert 'pascal: 6 images (0 skipped' in out
    assert os.path.exists(os.path.join(exp, 'model.safetensors'))
    steps = train.main(argv + ['--steps-per-epoch', '20', '--eval-dataset', 'pascal', root, 'trainval', '--eval-images', '4'])
    assert steps == 26
    out = capsys.readouterr().out
    assert 'restored step 6' in out
    losses = [float(l.split('class_loss ')[1].split()[0]) for l in out.splitlines() if 'class_loss' in l]
    regr = [float(l.split('regr_loss ')[1].split()[0]) for l in out.splitlines() if 'regr_loss' in l]
    assert len(losses) == 1 and np.isfinite(losses).all() and np.isfinite(regr).all()
    ev = [l for l in out.splitlines() if l.startswith('eval:')]
    assert len(ev) == 1 and 'over 4 images' in ev[0]
