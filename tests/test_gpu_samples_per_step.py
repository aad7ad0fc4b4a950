"""Several samples per step on the MI355X: the batched preprocess kernels (rn_resize_pair_u8_batch, _augment_batch) against the
single-image entries, bit for bit; dataset.DeviceFeed(samples_per_step=K) against the K = 1 feed; the graph-replayed step on
groups against eager steps on concatenated single-sample features; train.main with --samples-per-step."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 64
GROUP_A = [(30, 40), (60, 80), (45, 60)]          # one network input size at scale 64: (64, 85)
GROUP_B = [(40, 30), (80, 60)]                    # (85, 64)
STRIDE = 60 * 80 * 3                              # the 60 x 80 (and 80 x 60) image fills its slot exactly


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _draws(sizes):
    """One augmentation.Draw per image: crop windows with odd offsets (side fractions below 1), contrast on and off."""
    import augmentation
    params = [(1.2, -0.2, 0.8), (1.0, 0.1, 1.5), (0.8, 0.2, 0.9), (1.1, 0.0, 1.0), (0.9, -0.1, 0.0)]
    out = []
    for i, (h, w) in enumerate(sizes):
        y0, x0 = 1 + 2 * (i % 3), 3 + 2 * (i % 2)                       # odd offsets
        ch, cw = (h - y0) * 3 // 4, (w - x0) * 4 // 5
        f, d, k = params[i % len(params)]
        out.append(augmentation.Draw(y0, x0, ch, cw, np.float32(f), np.float32(d), np.float32(k)))
    return out


def _fill(raw, descs, images, rows):
    """Stage `images` into the slots of `raw` (stride STRIDE) and their descriptor rows into `descs`."""
    for i, (img, row) in enumerate(zip(images, rows)):
        raw[i * STRIDE:i * STRIDE + img.size].copy_(torch.from_numpy(img.reshape(-1)))
        descs[i].copy_(torch.from_numpy(row))


def _single(img, row, size, dev):
    import dataset
    raw, desc = torch.from_numpy(img.reshape(-1)).to(dev), torch.from_numpy(row).to(dev)
    if row.size == 12:
        return dataset.resize_pair_u8_augment(raw, desc, size)
    return dataset.resize_pair_u8(raw, desc, size)


def _rows(images, size, augment):
    import dataset
    if augment:
        return [dataset.augment_desc(im.shape[:2], v, size) for im, v in zip(images, _draws([im.shape[:2] for im in images]))]
    return [dataset.resize_desc(im.shape[:2], size) for im in images]


def _batch(raw, descs, size, augment, out=None):
    import dataset
    fn = dataset.resize_pair_u8_augment_batch if augment else dataset.resize_pair_u8_batch
    return fn(raw, descs, size, STRIDE, out=out)


def test_the_groups_map_to_one_network_input_size_each():
    import dataset
    assert {dataset.rescale_size(hw, SCALE) for hw in GROUP_A} == {(64, 85)}
    assert {dataset.rescale_size(hw, SCALE) for hw in GROUP_B} == {(85, 64)}
    assert max(h * w * 3 for h, w in GROUP_A) == STRIDE == max(h * w * 3 for h, w in GROUP_B)


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augment'])
def test_batched_slots_equal_the_single_image_entry_eager_and_in_one_graph(augment):
    dev = torch.device('cuda:0')
    width = 12 if augment else 4
    # eager: both groups, and K = 1 (the image that fills its stride, and a smaller one)
    for sizes, size, seed in ((GROUP_A, (64, 85), 1), (GROUP_B, (85, 64), 2), (GROUP_A[1:2], (64, 85), 3), (GROUP_B[:1], (85, 64), 4)):
        images = _images(sizes, seed)
        rows = _rows(images, size, augment)
        k = len(images)
        raw = torch.zeros(k * STRIDE, dtype=torch.uint8, device=dev)
        descs = torch.zeros((k, width), dtype=torch.int32, device=dev)
        _fill(raw, descs, images, rows)
        got = _batch(raw, descs, size, augment)
        assert tuple(got.shape) == (2 * k,) + size + (3,)
        for i in range(k):
            assert torch.equal(got[2 * i:2 * i + 2], _single(images[i], rows[i], size, dev)), (sizes, i)
    # one captured graph of K = 3, replayed with the raw bytes and the descriptors swapped between replays
    size = (64, 85)
    raw = torch.zeros(3 * STRIDE, dtype=torch.uint8, device=dev)
    descs = torch.zeros((3, width), dtype=torch.int32, device=dev)
    pairs = torch.empty((6,) + size + (3,), dtype=torch.float32, device=dev)
    images = _images(GROUP_A, 5)
    _fill(raw, descs, images, _rows(images, size, augment))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _batch(raw, descs, size, augment, out=pairs)                     # warm-up outside the capture (sizes the workspace)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _batch(raw, descs, size, augment, out=pairs)
    for seed, perm in ((6, (2, 0, 1)), (7, (1, 2, 0)), (8, (0, 1, 2))):
        images = _images([GROUP_A[p] for p in perm], seed)
        rows = _rows(images, size, augment)
        _fill(raw, descs, images, rows)
        pairs.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        for i in range(3):
            assert torch.equal(pairs[2 * i:2 * i + 2], _single(images[i], rows[i], size, dev)), (perm, i)


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augment'])
def test_a_descriptor_beyond_the_stride_reads_its_own_slot_only(augment):
    """Sample 0's descriptor claims 60 x 80 in slots of 30 x 40 x 3 bytes: the result is the single-image entry's with
    raw_capacity = the stride (bytes beyond it read as 0), and it does not depend on what slot 1 holds."""
    import dataset
    dev = torch.device('cuda:0')
    size, stride = (64, 85), 30 * 40 * 3
    big, small = _images([(60, 80), (30, 40)], 9)
    rows = _rows([big, small], size, augment)
    raw = torch.zeros(2 * stride, dtype=torch.uint8, device=dev)
    raw[:stride].copy_(torch.from_numpy(big.reshape(-1)[:stride]))
    raw[stride:].copy_(torch.from_numpy(small.reshape(-1)))
    descs = torch.from_numpy(np.stack(rows)).to(dev)
    fn = dataset.resize_pair_u8_augment_batch if augment else dataset.resize_pair_u8_batch
    one = dataset.resize_pair_u8_augment if augment else dataset.resize_pair_u8
    got = fn(raw, descs, size, stride)
    assert torch.equal(got[0:2], one(raw[:stride].clone(), descs[0].clone(), size))
    assert torch.equal(got[2:4], _single(small, rows[1], size, dev))
    raw[stride:].fill_(255)
    assert torch.equal(fn(raw, descs, size, stride)[0:2], got[0:2])


# ------------------------------------------------------------------------------------------------------------------ feed
VOC_SIZES = [(75, 100), (150, 200), (100, 75), (90, 120), (60, 80), (120, 160)]      # (64, 85) x 2, (85, 64), (64, 85) x 3
VOC_GROUPS = [2, 1, 2, 1]                                                            # the groups of K = 2 over that stream


def _equal_tree(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_tree(a[k], b[k]) for k in a)
    return a == b


def _cat_tree(trees):
    first = trees[0]
    if torch.is_tensor(first):
        return torch.cat(trees)
    if isinstance(first, dict):
        return {k: _cat_tree([t[k] for t in trees]) for k in first}
    assert all(t == first for t in trees)
    return first


def _drain(feed):
    out, keys, infos = [], [], []
    try:
        while True:
            try:
                keys.append(feed.stage())
            except StopIteration:
                break
            out.append(feed.features())
            feed.consumed()
            infos.append(feed.last_sample)
        torch.cuda.synchronize()
    finally:
        feed.close()
    return out, keys, infos


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'policy'])
def test_feed_groups_equal_the_concatenated_single_sample_features(tmp_path, augment):
    pytest.importorskip('PIL')
    import augmentation
    import dataset
    import files_fixtures as ff
    import levels as levels_mod
    from data_loaders.pascal import Pascal
    dev = torch.device('cuda:0')
    root = str(tmp_path / 'voc')
    ff.write_voc(root, ff.render(VOC_SIZES, seed=11))
    assert [dataset.rescale_size(hw, SCALE) for hw in VOC_SIZES] == [(64, 85)] * 2 + [(85, 64)] + [(64, 85)] * 3
    lv = levels_mod.build_levels()
    kw = dict(scale=SCALE, device=dev, ragged=True)
    if augment:
        kw.update(augment=augmentation.Policy(crop_min=0.5, seed=2), first_ordinal=7)
    singles, keys1, infos1 = _drain(dataset.DeviceFeed(Pascal(root, 'trainval'), lv, **kw))
    feed = dataset.DeviceFeed(Pascal(root, 'trainval'), lv, samples_per_step=2, **kw)
    groups, keys, infos = _drain(feed)
    assert len(singles) == 6 and all(len(k) == 4 for k in keys1)
    assert [len(i) for i in infos] == VOC_GROUPS and feed.samples_staged == 6 and feed.generations == 1
    assert all(len(k) == 5 for k in keys)
    assert [k[4] for k in keys] == VOC_GROUPS and [k[:2] for k in keys] == [(64, 85), (85, 64), (64, 85), (64, 85)]
    assert keys[0] == keys[2] and len(set(keys)) == 3 and [k[:4] for k in keys[:2]] == keys1[1:3]
    at = 0
    for g, n in zip(groups, VOC_GROUPS):
        assert tuple(g['image'].shape) == (2 * n,) + g['image_size'] + (3,)
        assert _equal_tree(g, _cat_tree(singles[at:at + n])), at
        at += n
    flat = [i for group in infos for i in group]
    for a, b in zip(flat, infos1):                            # the host-side record of every sample: the K = 1 feed's
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    if augment:
        assert sum(1 for i in flat if tuple(i['augment_desc'][2:6]) != (0, 0) + tuple(i['augment_desc'][:2])) > 0     # really cropped


# ------------------------------------------------------------------------------------------------------------------ step
class _Ragged(object):
    """7 in-memory uint8 samples; at scale 64 the groups of K = 2 are [A, A'], [B], [A, A'], [B, B'] with A (80, 64), B (64, 80)."""
    class_names = ['square', 'triangle', 'circle']
    num_classes = 3
    SIZES = [(100, 80), (101, 81), (80, 100), (100, 80), (101, 81), (80, 100), (81, 101)]
    GROUPS = [2, 1, 2, 2]

    def __iter__(self):
        from data_loaders.shapes import Shapes
        for i, hw in enumerate(self.SIZES):
            yield next(iter(Shapes(None, 1, image_size=hw, seed=60 + i)))

    def max_image_pixels(self):
        return max(h * w for h, w in self.SIZES)

    def max_objects(self):
        return 4


def test_graph_steps_on_groups_equal_eager_steps_on_concatenated_features():
    """Exact, like test_ragged_feed_graph_steps_equal_eager_steps_with_one_graph_per_input_shape."""
    import dataset, layers, levels as levels_mod, retinanet, train
    dev = torch.device('cuda:0')
    lv = levels_mod.build_levels()

    def net():
        torch.manual_seed(0)
        layers.Dropout._next_seed[0] = 0x5EED
        return retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0).to(dev)

    keep = ('image', 'detection', 'trainable_masks')
    singles = [{k: b[k] for k in keep} for b in dataset.build_dataset(_Ragged(), lv, scale=SCALE, device=dev)]
    eager = train.Trainer(net(), lv, learning_rate=1e-2, device=dev, use_graph=False)
    want, at = [], 0
    for n in _Ragged.GROUPS:
        want.append(eager.step(_cat_tree(singles[at:at + n]))['class_loss'].item())
        at += n
    torch.cuda.synchronize()
    feed = dataset.DeviceFeed(_Ragged(), lv, scale=SCALE, device=dev, ragged=True, samples_per_step=2)
    tr = train.Trainer(net(), lv, learning_rate=1e-2, device=dev, use_graph=True, input_fn=feed)
    got, keys = [], []
    try:
        for _ in range(4):
            got.append(tr.step()['class_loss'].item())
            keys.append(feed.shape_key)
        with pytest.raises(StopIteration):
            tr.step()
    finally:
        feed.close()
    torch.cuda.synchronize()
    assert len(set(got)) == 4 and all(np.isfinite(got))
    assert got == want
    assert torch.equal(tr.arena.weights, eager.arena.weights)
    assert [k[4] for k in keys] == _Ragged.GROUPS and keys[0] == keys[2] and len(set(keys)) == 3
    assert tr.recaptures == 2 and len(tr._graph_cache) == 3                  # one graph set per distinct key
    assert feed.generations == 1 and feed.samples_staged == 7


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_train_main_with_samples_per_step_trains_saves_and_resumes(tmp_path, capsys, monkeypatch):
    pytest.importorskip('PIL')
    import checkpoint
    import dataset
    import files_fixtures as ff
    import train
    from data_loaders.inferred import Inferred
    root = str(tmp_path / 'voc')
    # at scale 96: four (96, 128), two (128, 96), one (96, 96) -> an epoch is 2 + 1 + 1 groups of K = 2
    sizes = [(120, 160), (160, 120), (100, 133), (120, 160), (150, 150), (160, 120), (90, 120)]
    ff.write_voc(root, ff.render(sizes, seed=7))
    staged = []
    stage = dataset.DeviceFeed.stage

    def recording_stage(self):
        key = stage(self)
        staged.append([info['image_hw'] for info in self.last_sample])
        assert len(key) == 5 and key[4] == len(self.last_sample)
        return key

    monkeypatch.setattr(dataset.DeviceFeed, 'stage', recording_stage)
    exp = str(tmp_path / 'exp')
    path = os.path.join(exp, 'model.safetensors')
    argv = ['--dataset', 'pascal', root, 'trainval', '--scale', '96', '--epochs', '1', '--experiment', exp,
            '--backbone', 'mobilenet_v2', '--dropout', '0.1', '--samples-per-step', '2', '--steps-per-epoch', '3']
    assert train.main(argv) == 3
    out = capsys.readouterr().out
    assert '4 images per step' in out
    first = list(staged)
    n1 = sum(len(g) for g in first)
    assert len(first) == 3 and train.LAST_RUN['samples'] == n1
    assert checkpoint.load_extra(path)['samples_drawn'] == n1                # a sample count, not a step count
    assert train.main(argv) == 6                                             # resumed for 3 more steps
    assert 'restored step 3' in capsys.readouterr().out
    second = staged[3:]
    n2 = sum(len(g) for g in second)
    assert len(second) == 3 and train.LAST_RUN['samples'] == n2
    assert checkpoint.load_extra(path)['samples_drawn'] == n1 + n2
    # the two runs together staged the loader's stream from its start, nothing dropped or repeated at the resume
    loader = Inferred('pascal', [root, 'trainval']).configure(seed=0, scale=96, repeat=True, shape_runs=8, group=2)
    it = iter(loader)
    stream = [tuple(next(it)['image_size']) for _ in range(n1 + n2)]
    assert [hw for g in first + second for hw in g] == stream
    assert n1 + n2 > 7                                                       # ... across the end of the first epoch
    assert all(len({dataset.rescale_size(hw, 96) for hw in g}) == 1 and 1 <= len(g) <= 2 for g in first + second)
    assert loader.epoch_steps(0) == 4
