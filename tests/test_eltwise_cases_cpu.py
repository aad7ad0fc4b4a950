"""The case tables of tests/eltwise_ref.py without a GPU: the conditions the cases were picked for hold, and the references agree
with their independent restatements.

  * tied max-pool inputs: at least 25 % of the windows of every tied case have a repeated maximum (computed from the inputs
    alone), the continuous cases have none; the oracle's autograd gives the gradient to the FIRST valid maximum in row-major
    window order (the numpy restatement scattered by tap index), which is what the kernels are then held to;
  * the grid-cap pool is above the 4096-block cap of grid_for in forward, rn_maxpool_bwd_arg and the rescanning rn_maxpool_bwd
    (a Python model of that rule: elementwise.hip has no plan query);
  * the upsample sweep contains pairs whose dst * scale is exactly x.5 (the roundf tie), in rows and in columns;
  * activation inputs hold the kinks; the add_segs counts reach the tail path; host-side refusals of the entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import eltwise_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T


def _one_cell_windows(p):
    return int(R.valid_cells(p).max()) == 1


@pytest.mark.parametrize("p", R.POOLS, ids=R.pool_id)
def test_tied_inputs_tie(p):
    x = R.pool_input(p, R.CONTINUOUS)[0]
    assert R.tied_fraction(x, p.k, p.s) == 0.0
    for kind in R.TIED:
        x = R.pool_input(p, kind)[0]
        if _one_cell_windows(p):          # a 1 x 1 map: every window holds one valid cell and cannot tie
            assert (p.h, p.w) == (1, 1) and R.tied_fraction(x, p.k, p.s) == 0.0
        else:
            frac = R.tied_fraction(x, p.k, p.s)
            assert frac >= 0.25, "%s %s: only %.3f of the windows tie" % (R.pool_id(p), kind, frac)


def test_pool_table():
    assert len(R.POOLS) == 21 and len(set(R.POOLS)) == 21
    assert {(p.k, p.s) for p in R.POOLS} == {(3, 2), (2, 2), (3, 1), (2, 1), (3, 3)}
    assert any(p.k > p.h for p in R.POOLS) and any(p.h * p.w == 1 for p in R.POOLS)
    # padding after only (k = 2, s = 1), before and after (k = 3), none (k = s on a multiple)
    assert T.same_pad_1d(16, 2, 1)[1:] == (0, 1) and T.same_pad_1d(16, 3, 1)[1:] == (1, 1) and T.same_pad_1d(16, 2, 2)[1:] == (0, 0)
    assert T.same_pad_1d(7, 3, 3)[1:] == (1, 1) and T.same_pad_1d(16, 3, 2)[1:] == (0, 1) and T.same_pad_1d(7, 3, 2)[1:] == (1, 1)
    # the grid cap: forward and rn_maxpool_bwd_arg have a thread per channel quad, rn_maxpool_bwd one per element
    p = R.POOL_GRID_CAP
    oh, ow = R.pool_out(p)
    for total in (p.n * oh * ow * p.c // 4, p.n * p.h * p.w * p.c // 4, p.n * p.h * p.w * p.c):
        assert -(-total // R.BLOCK) > R.GRID_CAP and R.blocks(total) == R.GRID_CAP
    assert all(R.blocks(q.n * q.h * q.w * q.c) < R.GRID_CAP for q in R.POOLS if q != p)
    assert R.blocks(0) == 1 and R.blocks(256) == 1 and R.blocks(257) == 2
    assert all(q in R.POOLS for q in R.POOLS_F16) and len(R.POOLS_F16) == 2


@pytest.mark.parametrize("p", [q for q in R.POOLS if q != R.POOL_GRID_CAP], ids=R.pool_id)
def test_oracle_gives_the_gradient_to_the_first_maximum(p):
    """max_pool_same's autograd == dy scattered to the tap argmax_taps names, on continuous and on tied inputs; the forward
    is the maximum over the valid cells."""
    for kind in (R.CONTINUOUS,) + R.TIED:
        x, dy = R.pool_input(p, kind)
        y, dx = R.pool_ref("max", x, dy, p.k, p.s, torch.float64)
        taps = R.window_taps(x, p.k, p.s)
        arg = R.argmax_taps(x, p.k, p.s)
        assert np.array_equal(y, taps.max(axis=0))
        assert np.array_equal(np.take_along_axis(taps, arg[None].astype(np.int64), 0)[0], y)
        assert rel_err(dx, R.dx_from_argmax(arg, dy, p)) < 1e-15, kind
        if kind in R.TIED and not _one_cell_windows(p):      # ... and an earlier equal cell does exist in some window
            first = (taps == taps.max(axis=0)).argmax(axis=0)
            last = taps.shape[0] - 1 - (taps[::-1] == taps.max(axis=0)).argmax(axis=0)
            assert np.array_equal(first, arg) and np.any(last != first)


@pytest.mark.parametrize("p", [q for q in R.POOLS if q != R.POOL_GRID_CAP], ids=R.pool_id)
def test_average_pool_reference(p):
    """avg_pool_same divides by the valid cells; windows_per_cell / valid_cells (the T of the bounds) against plain loops."""
    x, dy = R.pool_input(p, R.CONTINUOUS)
    y, dx = R.pool_ref("avg", x, dy, p.k, p.s, torch.float64)
    taps = R.window_taps(x, p.k, p.s)
    valid = np.isfinite(taps)
    assert rel_err(y, np.where(valid, taps, 0).sum(0) / valid.sum(0)) < 1e-15
    oh, pt, _ = T.same_pad_1d(p.h, p.k, p.s)
    ow, pl, _ = T.same_pad_1d(p.w, p.k, p.s)
    per_cell, cells = np.zeros((p.h, p.w)), np.zeros((oh, ow))
    for i in range(oh):
        for j in range(ow):
            for a in range(p.k):
                for b in range(p.k):
                    if 0 <= i * p.s + a - pt < p.h and 0 <= j * p.s + b - pl < p.w:
                        per_cell[i * p.s + a - pt, j * p.s + b - pl] += 1
                        cells[i, j] += 1
    assert np.array_equal(R.windows_per_cell(p), per_cell) and np.array_equal(R.valid_cells(p), cells)


def test_upsample_sweep():
    assert len(R.UPS) == 96 + 3 and len(set(R.UPS)) == len(R.UPS)
    sweep = R.UPS[:96]
    assert {(u.th, u.h) for u in sweep} == {(th, h) for th in range(1, 9) for h in range(th, 3 * th + 3)}
    assert all((u.th, u.h) != (u.tw, u.w) and u.h >= u.th and u.w >= u.tw and (u.n, u.c) == (1, 4) for u in sweep)
    assert sum(u.h < u.th and u.w < u.tw for u in R.UPS) == 2 and R.Up(2, 8, 38, 75, 38, 75) in R.UPS
    # the roundf tie: dst * scale exactly on x.5, where half-away-from-zero and half-to-even differ
    rows = [u for u in sweep if R.has_rounding_tie(u.h, u.th)]
    cols = [u for u in sweep if R.has_rounding_tie(u.w, u.tw)]
    assert len(rows) >= 5 and len(cols) >= 5
    assert R.has_rounding_tie(3, 2) and list(T.nn_resize_index(3, 2)) == [0, 1, 1]          # 0.5 -> 1, away from zero
    assert list(T.nn_resize_index(5, 3)) == [0, 1, 1, 2, 2] and R.has_rounding_tie(5, 3)    # 0.5 -> 1 and 1.5 -> 2: to-even would give 0 and 2
    assert all(u in R.UPS for u in R.UPS_F16) and len(R.UPS_F16) == 3
    for u in R.UPS:          # every coarse cell's sources are counted; shrinking leaves cells without any
        src = R.up_sources(u)
        assert src.sum() == u.h * u.w and ((src == 0).any() == (u.h < u.th or u.w < u.tw))


def test_upsample_reference_is_a_gather():
    for u in (R.UPS[7], R.UPS[50], R.UPS[-1]):
        lat, top, dy = R.up_input(u)
        y, dtop = R.up_ref(lat, top, dy, torch.float64)
        iy, ix = T.nn_resize_index(u.h, u.th), T.nn_resize_index(u.w, u.tw)
        want_y, want_d = lat.double().numpy().copy(), np.zeros(tuple(top.shape))
        for a in range(u.h):
            for b in range(u.w):
                want_y[:, a, b] += top.double().numpy()[:, iy[a], ix[b]]
                want_d[:, iy[a], ix[b]] += dy.double().numpy()[:, a, b]
        assert np.array_equal(y, want_y) and rel_err(dtop, want_d) < 1e-15


def test_activation_inputs_and_oracle_at_the_kinks():
    big = R.act_input(R.ACT_COUNTS[-1])[0].numpy()
    assert np.array_equal(big[:len(R.SPECIALS)].view(np.uint32), R.SPECIALS.view(np.uint32))
    seen = np.concatenate([R.act_input(n)[0].numpy() for n in R.ACT_COUNTS])
    for v in (0.0, 6.0, 88.0, -88.0, 100.0, -100.0, 1.401298464324817e-45, -1.401298464324817e-45):
        assert (seen == np.float32(v)).any(), v
    assert np.signbit(seen[seen == 0]).any() and not np.signbit(seen[seen == 0]).all()
    assert (seen == np.nextafter(np.float32(6), np.float32(7))).any() and (seen == np.nextafter(np.float32(6), np.float32(0))).any()
    assert {R.act_input(n)[0].numel() for n in R.ACT_COUNTS} == set(R.ACT_COUNTS)
    # counts around the block (256) and above the grid cap (4096 x 256): the last blocks loop twice
    assert R.blocks(255) == R.blocks(256) == 1 and R.blocks(257) == 2 and R.ACT_COUNTS[-1] > R.GRID_CAP * R.BLOCK
    # [TF-sem] the gradients at the kinks: relu 0 at 0; relu6 0 at 0 and at 6 (Relu6Grad: 0 < x < 6), 1 just inside
    x = torch.from_numpy(R.SPECIALS[:7].copy())
    one = torch.ones(7)
    assert list(R.act_ref(x, one, "relu", torch.float32)[1]) == [0, 0, 1, 1, 0, 1, 1]
    assert list(R.act_ref(x, one, "relu6", torch.float32)[1]) == [0, 0, 0, 1, 0, 0, 1]
    assert list(R.act_ref(x, one, None, torch.float32)[1]) == [1] * 7
    assert np.array_equal(R.act_ref(x, one, "relu6", torch.float32)[0], np.clip(R.SPECIALS[:7], 0, 6))
    assert [k for _, k in R.ACTS] == [None, "relu", "elu", "relu6", "sigmoid"]
    import _rn
    assert all(_rn.ACT[k] == i for i, k in R.ACTS)


def test_host_refusals():
    """What the entry points refuse before they launch (the host word stands for device memory)."""
    import _rn
    L = _rn.lib()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p = p if p % 16 == 0 else p + 8
    assert L.rn_maxpool_fwd(p, p, p, 1, 4, 4, 4, 16, 1, None) == -2          # 16 x 16 = 256 taps do not fit a byte
    assert L.rn_maxpool_fwd(p, p, p, 1, 4, 4, 6, 3, 1, None) == -2           # c % 4
    assert L.rn_avgpool_fwd(p, p, 1, 4, 4, 6, 3, 1, None) == -2 and L.rn_avgpool_bwd(p, p, 1, 4, 4, 4, 0, 1, None) == -1
    assert L.rn_maxpool_bwd_arg(None, p, p, 1, 4, 4, 4, 3, 1, None) == -1
    assert L.rn_act_fwd_f16(p, p, 6, 1, None) == -1 and L.rn_act_fwd_f16(p, p, 0, 1, None) == 0
    assert L.rn_act_fwd(p, p, 0, 1, None) == 0 and L.rn_act_fwd(p, p, -1, 1, None) == -1 and L.rn_act_bwd(p, None, p, 4, 1, None) == -1
    assert L.rn_upsample_add_fwd(p, p, p, 1, 4, 4, 2, 2, 6, None) == -2 and L.rn_upsample_add_bwd_top(p, p, 1, 4, 4, 0, 2, 4, None) == -1
    segs = (_rn.AddSeg * (_rn.MAX_SEG + 1))()
    for s in segs:
        s.a, s.b, s.out, s.count = p, p, p, 4
    assert L.rn_add_segs(segs, 0, None) == -1 and L.rn_add_segs(segs, _rn.MAX_SEG + 1, None) == -1 and L.rn_add_segs(None, 1, None) == -1
    for field in ("a", "b", "out"):          # a pointer off 16 bytes
        setattr(segs[1], field, p + 4)
        assert L.rn_add_segs(segs, 2, None) == -1
        setattr(segs[1], field, p)
    segs[0].count = 0
    assert L.rn_add_segs(segs, 1, None) == -1
    assert L.rn_flip_width(p, p, 0, 3, 4, 4, 0, 0, None) == 0 and L.rn_flip_width(p, p, 1, 3, 4, 2, 0, 0, None) == -1
    assert L.rn_flip_width(p, p, 1, 3, 4, 1, 4, 1, None) == -1               # negation needs fp32
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rn_hip.h")).read()
    assert int(re.search(r"#define RN_MAX_SEG (\d+)", hdr).group(1)) == _rn.MAX_SEG
