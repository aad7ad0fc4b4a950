"""Training-time augmentation on the MI355X: rn_resize_pair_u8_augment against the numpy restatement of its contract
(tests/augment_ref.py), its two identity cases, one captured graph serving every descriptor, the ragged DeviceFeed with a
Policy, and train.main with --augment on a VOC tree written at test time."""
import os

import numpy as np
import pytest
import torch

import augment_ref

pytestmark = pytest.mark.gpu

# 1e-5 absolute on the normalised output, derived, not measured: fewer than 16 fp32 roundings of 2^-24 on magnitudes <= 1.5,
# divided by the smallest STD 0.275, give 5.2e-6; the bar is twice that.  (The mean is exact to one rounding: fp64 sums.)
BAR = 1e-5


def _image(h, w, seed, grey=False):
    rng = np.random.default_rng(seed)
    if grey:
        return np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, axis=2)
    # smooth colour gradients plus noise: saturated and pale pixels, bright and dark ones, so that every branch is taken
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * yy / max(h - 1, 1), 255.0 * xx / max(w - 1, 1), 255.0 * (yy + xx) / max(h + w - 2, 1)], -1)
    return np.clip(0.7 * base + 0.3 * rng.integers(0, 256, (h, w, 3)), 0, 255).astype(np.uint8)


def _run(img, window, f, d, k, size, dev, normalize=True):
    import augmentation
    import dataset
    v = augmentation.Draw(window[0], window[1], window[2], window[3], np.float32(f), np.float32(d), np.float32(k))
    desc = torch.from_numpy(dataset.augment_desc(img.shape[:2], v, size)).to(dev)
    return dataset.resize_pair_u8_augment(torch.from_numpy(img.reshape(-1)).to(dev), desc, size, normalize=normalize)


# (raw size, window (y0, x0, ch, cw)): odd raw sizes, a window on each border, a corner, a 2x2 window, the full image
GEOMETRY = [
    ((37, 53), (0, 0, 37, 53)),
    ((37, 53), (0, 7, 20, 31)),           # top border
    ((37, 53), (12, 9, 25, 40)),          # bottom border
    ((53, 37), (5, 0, 33, 21)),           # left border
    ((53, 37), (11, 14, 30, 23)),         # right border
    ((101, 81), (60, 50, 41, 31)),        # bottom right corner
    ((101, 81), (40, 33, 2, 2)),          # 2 x 2 window
    ((375, 500), (17, 101, 301, 333)),
    ((2, 2), (0, 0, 2, 2)),
]
# (f, d, k): both ends of every range of the default policy, k > 1 where the saturation clamp binds, strong settings that clip
PARAMS = [(0.8, -0.2, 0.8), (1.2, 0.2, 1.0), (0.8, 0.2, 1.0), (1.2, -0.2, 0.8), (1.0, 0.0, 1.5), (1.2, 0.2, 1.5), (1.0, 0.1, 1.0),
          (1.1, 0.0, 0.0)]


def test_kernel_equals_the_restatement_of_the_contract():
    import dataset
    dev = torch.device('cuda:0')
    worst, clamp_binds, clipped = 0.0, 0, 0
    for gi, (hw, window) in enumerate(GEOMETRY):
        for grey in (False, True):
            img = _image(hw[0], hw[1], seed=gi, grey=grey)
            for size in (dataset.rescale_size(hw, 96), (33, 47)):
                r = augment_ref.resized(img, window, size)
                for f, d, k in PARAMS:
                    got = _run(img, window, f, d, k, size, dev).cpu().numpy()
                    want = augment_ref.expected_pair(img, window, f, d, k, size)
                    err = float(np.abs(got.astype(np.float64) - want).max())
                    worst = max(worst, err)
                    assert err <= BAR, (hw, window, grey, size, (f, d, k), err)
                    assert np.array_equal(got[1], got[0][:, ::-1]), (hw, window, size, (f, d, k))     # slot 1: the flip, bit for bit
                    if not grey and k > 1:
                        b = np.clip((r - r.reshape(-1, 3).mean(0)) * f + r.reshape(-1, 3).mean(0) + d, 0, 1)
                        M, n = b.max(-1), b.min(-1)
                        clamp_binds += int(((M > n) & (M / np.where(M > n, M - n, 1) < k)).sum())
                        clipped += int(((b == 0) | (b == 1)).sum())
            if grey:                          # M == n everywhere: saturation changes nothing, whatever k
                a = _run(img, window, 1.1, 0.05, 0.0, (33, 47), dev)
                b = _run(img, window, 1.1, 0.05, 1.5, (33, 47), dev)
                assert torch.equal(a, b)
    print('worst absolute error %.3g (bar %.3g)' % (worst, BAR))
    assert clamp_binds > 0 and clipped > 0        # the cases do reach the saturation clamp and the [0, 1] clip
    # un-normalised output too
    img = _image(37, 53, seed=99)
    got = _run(img, (3, 4, 30, 40), 1.2, -0.1, 0.9, (40, 56), dev, normalize=False).cpu().numpy()
    want = augment_ref.expected_pair(img, (3, 4, 30, 40), 1.2, -0.1, 0.9, (40, 56), normalize=False)
    assert np.abs(got - want).max() <= BAR * 0.275 and got.min() >= 0.0 and got.max() <= 1.0


def test_identity_parameters_and_window_only_are_bit_equal_to_the_plain_pair():
    import dataset
    dev = torch.device('cuda:0')
    for gi, (hw, window) in enumerate(GEOMETRY):
        img = _image(hw[0], hw[1], seed=20 + gi)
        for size in (hw, dataset.rescale_size(hw, 96), (1, 1), (5, 1), (64, 80)):
            # full window, f = 1, d = 0, k = 1: rn_resize_pair_u8 of the image
            plain = dataset.resize_pair_u8(torch.from_numpy(img.reshape(-1)).to(dev),
                                           torch.from_numpy(dataset.resize_desc(hw, size)).to(dev), size)
            assert torch.equal(_run(img, (0, 0, hw[0], hw[1]), 1.0, 0.0, 1.0, size, dev), plain), (hw, size)
            # a window alone: rn_resize_pair_u8 of a contiguous copy of the crop
            y0, x0, ch, cw = window
            crop = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
            plain = dataset.resize_pair_u8(torch.from_numpy(crop.reshape(-1)).to(dev),
                                           torch.from_numpy(dataset.resize_desc((ch, cw), size)).to(dev), size)
            assert torch.equal(_run(img, window, 1.0, 0.0, 1.0, size, dev), plain), (hw, window, size)


def test_one_captured_graph_serves_every_descriptor_bit_equal_to_eager():
    import augmentation
    import dataset
    dev = torch.device('cuda:0')
    size = (64, 80)
    cases = [((375, 500), (17, 101, 301, 333), (1.2, -0.2, 0.8)), ((53, 37), (11, 14, 30, 23), (0.8, 0.2, 1.5)),
             ((101, 81), (0, 0, 101, 81), (1.0, 0.0, 1.0)), ((37, 53), (12, 9, 25, 40), (1.1, 0.1, 0.9))]
    images = [_image(hw[0], hw[1], seed=40 + i) for i, (hw, _, _) in enumerate(cases)]
    cap = max(im.size for im in images)
    raw = torch.zeros(cap, dtype=torch.uint8, device=dev)
    desc = torch.zeros(12, dtype=torch.int32, device=dev)
    pair = torch.empty((2,) + size + (3,), dtype=torch.float32, device=dev)

    def stage(i):
        hw, window, (f, d, k) = cases[i]
        v = augmentation.Draw(window[0], window[1], window[2], window[3], np.float32(f), np.float32(d), np.float32(k))
        raw[:images[i].size].copy_(torch.from_numpy(images[i].reshape(-1)))
        desc.copy_(torch.from_numpy(dataset.augment_desc(hw, v, size)))

    stage(3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dataset.resize_pair_u8_augment(raw, desc, size, out=pair)             # warm-up outside the capture (sizes the workspace)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dataset.resize_pair_u8_augment(raw, desc, size, out=pair)
    for i in (0, 1, 2, 0):
        stage(i)
        g.replay()
        torch.cuda.synchronize()
        first = pair.clone()
        hw, window, (f, d, k) = cases[i]
        assert torch.equal(first, _run(images[i], window, f, d, k, size, dev)), cases[i]      # replay == eager
        pair.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(pair, first), cases[i]                                             # replay == replay


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


def _net(lv, dev):
    import layers, retinanet
    torch.manual_seed(0)
    layers.Dropout._next_seed[0] = 0x5EED
    return retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0).to(dev)


def test_ragged_feed_with_a_policy_graph_steps_equal_eager_steps():
    import augmentation, dataset, levels as levels_mod, train
    dev = torch.device('cuda:0')
    lv = levels_mod.build_levels()
    policy = augmentation.Policy(crop_min=0.5, seed=2)
    eager = train.Trainer(_net(lv, dev), lv, learning_rate=1e-2, device=dev, use_graph=False)
    want = [eager.step(b)['class_loss'].item() for b in dataset.build_dataset(_Ragged(), lv, scale=64, device=dev, augment=policy)]
    torch.cuda.synchronize()
    feed = dataset.DeviceFeed(_Ragged(), lv, scale=64, device=dev, ragged=True, augment=policy)
    tr = train.Trainer(_net(lv, dev), lv, learning_rate=1e-2, device=dev, use_graph=True, input_fn=feed)
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
    # still one graph per network input shape, and the key is the one of a feed without a policy
    assert len({k[:2] for k in keys}) == 2 and len(set(keys)) == 2
    assert tr.recaptures == 1 and len(tr._graph_cache) == 2
    assert feed.generations == 1 and feed.samples_staged == 6
    plain = dataset.DeviceFeed(_Ragged(), lv, scale=64, device=dev, ragged=True)
    try:
        assert plain.stage() == keys[0]
        plain.consumed()
    finally:
        plain.close()
    # the augmented stream is not the plain one
    plain_eager = train.Trainer(_net(lv, dev), lv, learning_rate=1e-2, device=dev, use_graph=False)
    first = next(iter(dataset.build_dataset(_Ragged(), lv, scale=64, device=dev)))
    assert plain_eager.step(first)['class_loss'].item() != want[0]


def test_ragged_feed_with_a_policy_stages_transformed_boxes_labels_and_pixels():
    import augmentation, dataset, levels as levels_mod
    dev = torch.device('cuda:0')
    lv = levels_mod.build_levels()
    policy = augmentation.Policy(crop_min=0.5, seed=2)
    samples = list(_Ragged())
    feed = dataset.DeviceFeed(_Ragged(), lv, scale=64, device=dev, ragged=True, augment=policy, first_ordinal=10)
    cropped = fewer = 0
    try:
        for i, sample in enumerate(samples):
            feed.stage()
            b = feed.features()
            feed.consumed()
            torch.cuda.synchronize()
            info = feed.last_sample
            img = sample['image']
            h, w = img.shape[:2]
            norm = np.asarray(sample['boxes'], np.float32).reshape(-1, 4) / np.asarray([h, w, h, w], np.float32)
            v, boxes, ids = policy.draw(0, 10 + i, (h, w), norm, sample['class_ids'])           # ordinal = first_ordinal + position
            size = dataset.rescale_size((h, w), 64)                                               # of the FULL image
            assert b['image_size'] == size
            assert np.array_equal(info['augment_desc'], dataset.augment_desc((h, w), v, size))
            assert np.array_equal(info['boxes'], boxes) and np.array_equal(info['class_ids'], ids)
            is_crop = (v.y0, v.x0, v.ch, v.cw) != (0, 0, h, w)
            cropped += is_crop
            fewer += len(ids) < len(sample['class_ids'])
            if is_crop:
                assert v.ch < h and v.cw < w and abs(v.ch / h - v.cw / w) < 0.02               # the raw aspect
            want = augment_ref.expected_pair(img, (v.y0, v.x0, v.ch, v.cw), v.f, v.d, v.k, size)
            assert np.abs(b['image'].cpu().numpy() - want).max() <= BAR
            c, r, m = dataset.build_labels(size, torch.from_numpy(np.asarray(ids, np.int32)).to(dev)[None],
                                           torch.from_numpy(boxes).to(dev)[None], lv, 3, flip_pair=True)
            for k in lv:
                assert torch.equal(b['detection']['classifications'][k], c[k]), k
                assert torch.equal(b['detection']['regressions'][k], r[k]), k
                assert torch.equal(b['trainable_masks'][k], m[k]), k
    finally:
        feed.close()
    assert cropped > 0, "no staged sample was cropped: the test would not see the crop path"
    print('cropped %d of %d samples, %d lost a box' % (cropped, len(samples), fewer))


def test_policy_off_is_the_run_that_never_passes_the_argument():
    import dataset, levels as levels_mod, train
    dev = torch.device('cuda:0')
    lv = levels_mod.build_levels()
    weights = []
    for kw in ({}, {'augment': None}, {'augment': False, 'first_ordinal': 5}):
        feed = dataset.DeviceFeed(_Ragged(), lv, scale=64, device=dev, ragged=True, **kw)
        tr = train.Trainer(_net(lv, dev), lv, learning_rate=1e-2, device=dev, use_graph=True, input_fn=feed)
        try:
            for _ in range(4):
                tr.step()
        finally:
            feed.close()
        torch.cuda.synchronize()
        assert 'augment_desc' not in feed.last_sample and 'adesc' not in feed._static
        weights.append(tr.arena.weights.clone())
    assert torch.equal(weights[0], weights[1]) and torch.equal(weights[0], weights[2])


def test_train_main_with_augment_trains_saves_resumes_and_evaluates(tmp_path, capsys, monkeypatch):
    pytest.importorskip('PIL')
    import dataset
    import files_fixtures as ff
    import train
    root = str(tmp_path / 'voc')
    ff.write_voc(root, ff.render([(120, 160), (160, 120), (100, 133), (120, 160), (150, 150), (160, 120)], seed=7))
    staged = []
    stage = dataset.DeviceFeed.stage

    def recording_stage(self):
        key = stage(self)
        staged.append(np.array(self.last_sample['augment_desc']))
        return key

    monkeypatch.setattr(dataset.DeviceFeed, 'stage', recording_stage)

    def argv(exp, steps):
        return ['--dataset', 'pascal', root, 'trainval', '--scale', '96', '--epochs', '1', '--experiment', str(tmp_path / exp),
                '--backbone', 'mobilenet_v2', '--dropout', '0.1', '--shape-runs', '4', '--steps-per-epoch', str(steps),
                '--augment', '--augment-crop', '0.6', '--augment-seed', '3']

    assert train.main(argv('whole', 6)) == 6                                 # uninterrupted: 6 steps
    whole, staged[:] = list(staged), []
    assert train.main(argv('parts', 3)) == 3                                 # 3 steps, saved ...
    assert os.path.exists(str(tmp_path / 'parts' / 'model.safetensors'))
    first, staged[:] = list(staged), []
    capsys.readouterr()
    steps = train.main(argv('parts', 3) + ['--eval-dataset', 'pascal', root, 'trainval', '--eval-images', '4'])
    assert steps == 6                                                        # ... resumed for 3 more, evaluated
    out = capsys.readouterr().out
    assert 'restored step 3' in out
    ev = [l for l in out.splitlines() if l.startswith('eval:')]
    assert len(ev) == 1 and 'over 4 images' in ev[0]
    resumed = list(staged)                                                   # (the evaluation loader stages nothing: it never augments)
    assert len(whole) == 6 and len(first) == 3 and len(resumed) == 3
    for a, b in zip(whole, first + resumed):
        assert np.array_equal(a, b)                                          # steps N+1.. of the resumed run: the uninterrupted run's
    assert len({d.tobytes() for d in whole}) == 6
    assert sum(1 for d in whole if (d[2], d[3], d[4], d[5]) != (0, 0, d[0], d[1])) > 0        # really cropped
    assert train.LAST_RUN['graph_sets'] <= 3                                 # one graph set per network input shape (3 raw aspects)
