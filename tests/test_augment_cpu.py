"""Host side of the training-time augmentation, without a GPU: the library's new entry and its argument checks, the draws of
augmentation.Policy, the crop's box rule against a per-box restatement, and the CLI's refusal for the synthetic stream."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_augment_entry_and_reports_bad_arguments():
    import _rn
    raw = ctypes.CDLL(_rn.LIB_PATH)
    for sym in ("rn_resize_pair_u8_augment", "rn_resize_pair_u8_augment_workspace"):
        assert hasattr(raw, sym), "librn_hip.so does not export %s" % sym
        assert sym in _rn.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    version = int(re.search(r"#define RN_API_VERSION (\d+)", hdr).group(1))
    assert version >= 409 and raw.rn_version() == version == _rn.API_VERSION
    assert "dataset.py:206-212" in hdr and "train.py:190-198" in hdr and "rn_augment_desc" in hdr
    L = _rn.lib()
    # the workspace is a function of (oh, ow) only: 3 fp64 sums per block of 1024 pixels, at most 256 blocks
    assert L.rn_resize_pair_u8_augment_workspace(512, 512) == 256 * 3 * 8
    assert L.rn_resize_pair_u8_augment_workspace(1, 1) == 3 * 8
    assert L.rn_resize_pair_u8_augment_workspace(32, 33) == 2 * 3 * 8
    assert L.rn_resize_pair_u8_augment_workspace(1024, 1365) <= 256 * 3 * 8
    assert L.rn_resize_pair_u8_augment_workspace(0, 5) == 0
    # bad arguments: the negative status, before any launch (no device here); 8 stands for "some non-null pointer"
    p = ctypes.c_void_p(8)
    big = ctypes.c_size_t(1 << 20)
    assert L.rn_resize_pair_u8_augment(None, 64, p, p, 4, 4, None, None, p, big, None) == -1          # RN_EINVAL
    assert b"resize_pair_u8_augment" in L.rn_last_error()
    assert L.rn_resize_pair_u8_augment(p, 64, None, p, 4, 4, None, None, p, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 64, p, None, 4, 4, None, None, p, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 64, p, p, 4, 4, None, None, None, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 64, p, p, 0, 4, None, None, p, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 64, p, p, 4, -1, None, None, p, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 0, p, p, 4, 4, None, None, p, big, None) == -1
    assert L.rn_resize_pair_u8_augment(p, 64, p, p, 4, 4, None, None, p, ctypes.c_size_t(8), None) == -1   # workspace too small
    assert b"workspace" in L.rn_last_error()
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert L.rn_resize_pair_u8_augment(p, 64, p, p, 4, 4, mean, None, p, big, None) == -1               # mean without std


def test_augment_desc_layout_matches_the_header_struct():
    import augmentation
    import dataset
    v = augmentation.Draw(3, 5, 20, 30, np.float32(1.1), np.float32(-0.05), np.float32(0.9))
    d = dataset.augment_desc((40, 50), v, (64, 80))
    assert d.dtype == np.int32 and d.shape == (12,)
    assert list(d[:6]) == [40, 50, 3, 5, 20, 30] and d[11] == 0
    fl = d[6:11].view(np.float32)
    assert fl[0] == np.float32(19) / np.float32(63) and fl[1] == np.float32(29) / np.float32(79)
    assert list(fl[2:]) == [np.float32(1.1), np.float32(-0.05), np.float32(0.9)]
    # the full window's ratios are resize_desc's, bit for bit
    full = dataset.augment_desc((40, 50), augmentation.Draw(0, 0, 40, 50, 1, 0, 1), (64, 80))
    assert np.array_equal(full[6:8], dataset.resize_desc((40, 50), (64, 80))[2:])
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    body = re.search(r"typedef struct rn_augment_desc \{(.*?)\} rn_augment_desc;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == ["h", "w", "y0", "x0", "ch", "cw", "hs", "ws", "f", "d", "k", "reserved"]


def test_policy_draws_are_a_pure_function_of_seed_rank_and_ordinal_and_stay_in_range():
    import augmentation
    pol = augmentation.Policy(seed=3)
    assert pol.contrast == (0.8, 1.2) and pol.brightness == 0.2 and pol.saturation == (0.8, 1.0) and pol.crop_min == 1.0
    boxes = np.array([[0.1, 0.2, 0.5, 0.6]], np.float32)
    ids = np.array([2], np.int32)
    seen = set()
    for rank in (0, 1):
        for ordinal in range(200):
            v, b, c = pol.draw(rank, ordinal, (375, 500), boxes, ids)
            v2, b2, c2 = augmentation.Policy(seed=3).draw(rank, ordinal, (375, 500), boxes, ids)
            assert v == v2 and np.array_equal(b, b2) and np.array_equal(c, c2)
            assert (v.y0, v.x0, v.ch, v.cw) == (0, 0, 375, 500)                   # crop_min = 1: the full window ...
            assert np.array_equal(b, boxes) and np.array_equal(c, ids)            # ... and the boxes as they came
            assert np.float32(0.8) <= v.f <= np.float32(1.2) and abs(v.d) <= np.float32(0.2)
            assert np.float32(0.8) <= v.k <= np.float32(1.0)
            assert all(isinstance(x, np.float32) for x in (v.f, v.d, v.k))
            seen.add((float(v.f), float(v.d), float(v.k)))
    assert len(seen) == 400                                                        # other ordinals / ranks: other draws
    assert augmentation.Policy(seed=4).draw(0, 0, (375, 500), boxes, ids)[0] != pol.draw(0, 0, (375, 500), boxes, ids)[0]
    # the ranges are the policy's: a degenerate range pins the value
    v = augmentation.Policy(contrast=(1.0, 1.0), brightness=0.0, saturation=(1.0, 1.0)).draw(0, 7, (10, 10), boxes, ids)[0]
    assert (v.f, v.d, v.k) == (1.0, 0.0, 1.0)
    for bad in (dict(contrast=(0.0, 1.0)), dict(saturation=(-0.1, 1.0)), dict(brightness=-1.0), dict(crop_min=0.0), dict(crop_min=1.5)):
        with pytest.raises(ValueError):
            augmentation.Policy(**bad)


def _brute_force_boxes(boxes, ids, hw, window):
    """The crop's box rule, one box at a time, in Python floats."""
    h, w = float(hw[0]), float(hw[1])
    y0, x0, ch, cw = window
    wy0, wx0, wy1, wx1 = y0 / h, x0 / w, (y0 + ch) / h, (x0 + cw) / w
    out_b, out_i, clipped, dropped = [], [], 0, 0
    for b, c in zip(boxes, ids):
        by0, bx0, by1, bx1 = (float(t) for t in b)
        cy, cx = (by0 + by1) / 2, (bx0 + bx1) / 2
        if not (wy0 <= cy <= wy1 and wx0 <= cx <= wx1):
            dropped += 1
            continue
        ny0, nx0, ny1, nx1 = max(by0, wy0), max(bx0, wx0), min(by1, wy1), min(bx1, wx1)
        clipped += (ny0, nx0, ny1, nx1) != (by0, bx0, by1, bx1)
        out_b.append([(ny0 - wy0) / (wy1 - wy0), (nx0 - wx0) / (wx1 - wx0), (ny1 - wy0) / (wy1 - wy0), (nx1 - wx0) / (wx1 - wx0)])
        out_i.append(int(c))
    return np.asarray(out_b, np.float32).reshape(-1, 4), np.asarray(out_i, np.int32), clipped, dropped


def test_crop_box_rule_against_a_per_box_check():
    import augmentation
    pol = augmentation.Policy(crop_min=0.4, seed=11)
    nodrop = augmentation.Policy(crop_min=1.0, seed=11)
    rng = np.random.default_rng(5)
    n_drop = n_clip = n_fallback = n_cropped = 0
    for ordinal in range(300):
        h, w = int(rng.integers(2, 400)), int(rng.integers(2, 400))
        o = int(rng.integers(1, 6))
        c = rng.uniform(0.05, 0.95, (o, 2))
        half = rng.uniform(0.01, 0.3, (o, 2))
        boxes = np.clip(np.concatenate([c - half, c + half], 1), 0.0, 1.0).astype(np.float32)
        ids = np.arange(100, 100 + o, dtype=np.int32)                            # distinct: the order of the survivors is visible
        v, b, i = pol.draw(0, ordinal, (h, w), boxes, ids)
        p = nodrop.draw(0, ordinal, (h, w), boxes, ids)[0]
        assert (v.f, v.d, v.k) == (p.f, p.d, p.k)                                # the photometric draws do not depend on the crop
        assert 0 <= v.y0 and v.y0 + v.ch <= h and 0 <= v.x0 and v.x0 + v.cw <= w and v.ch >= min(2, h) and v.cw >= min(2, w)
        # the window the policy drew, restated from the same stream
        g = np.random.default_rng([11, 0, ordinal])
        g.uniform(0.8, 1.2), g.uniform(-0.2, 0.2), g.uniform(0.8, 1.0)
        s = g.uniform(0.4, 1.0)
        assert 0.4 <= s <= 1.0
        ch, cw = min(h, max(2, int(round(h * s)))), min(w, max(2, int(round(w * s))))
        win = (int(g.integers(0, h - ch + 1)), int(g.integers(0, w - cw + 1)), ch, cw)
        want_b, want_i, clipped, dropped = _brute_force_boxes(boxes, ids, (h, w), win)
        if len(want_i) == 0:                                                     # no survivor: the full window, the boxes untouched
            n_fallback += 1
            assert (v.y0, v.x0, v.ch, v.cw) == (0, 0, h, w)
            assert np.array_equal(b, boxes) and np.array_equal(i, ids)
            continue
        n_cropped += 1
        n_drop += dropped > 0
        n_clip += clipped > 0
        assert (v.y0, v.x0, v.ch, v.cw) == win
        assert np.array_equal(i, want_i) and list(i) == sorted(i)                # survivors in their order
        assert b.dtype == np.float32 and b.shape == want_b.shape
        np.testing.assert_allclose(b, want_b, rtol=0, atol=1e-6)
        assert (b >= 0).all() and (b <= 1).all() and (b[:, :2] <= b[:, 2:]).all()
    assert n_drop > 0 and n_clip > 0 and n_fallback > 0 and n_cropped > 0, (n_drop, n_clip, n_fallback, n_cropped)


def test_train_cli_refuses_augment_for_the_synthetic_stream(capsys):
    import train
    for argv in (['--augment', '--dataset', 'shapes'], ['--augment'], ['--augment-crop', '0.6', '--dataset', 'shapes']):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2
        assert '--augment' in capsys.readouterr().err
    a = train.build_parser().parse_args(['--augment', '--augment-crop', '0.6', '--augment-seed', '5'])
    assert a.augment and a.augment_crop == 0.6 and a.augment_seed == 5
    a = train.build_parser().parse_args([])
    assert not a.augment and a.augment_crop is None and a.augment_seed is None


def test_feed_and_dataset_refuse_what_the_kernel_cannot_read():
    import augmentation
    import dataset
    import levels

    class _Floats(object):
        num_classes = 3

        def __iter__(self):
            yield {'image': np.zeros((8, 8, 3), np.float32), 'boxes': np.array([[1, 1, 5, 5]], np.float32),
                   'class_ids': np.array([0], np.int32)}

    with pytest.raises(ValueError, match='uint8'):
        next(dataset.build_dataset(_Floats(), levels.build_levels(), augment=augmentation.Policy(), device='cpu'))
    # a policy without the ragged staging: refused before anything touches a device
    with pytest.raises(ValueError, match='ragged=True'):
        dataset.DeviceFeed(_Floats(), levels.build_levels(), augment=augmentation.Policy())
    # only a Policy (or None / False) is an augmentation; the feed does not take the reference's literal True either
    for bad in (True, 1, 'yes', object()):
        with pytest.raises(TypeError, match='augmentation.Policy'):
            dataset.DeviceFeed(_Floats(), levels.build_levels(), ragged=True, augment=bad)
    for bad in (1, 'yes', object()):
        with pytest.raises(TypeError, match='augmentation.Policy'):
            next(dataset.build_dataset(_Floats(), levels.build_levels(), augment=bad, device='cpu'))
    assert dataset._policy_or_none(True, allow_true=True) is None             # build_dataset(augment=True): accepted, no transform
    assert dataset._policy_or_none(None) is None and dataset._policy_or_none(False) is None
    pol = augmentation.Policy()
    assert dataset._policy_or_none(pol) is pol
