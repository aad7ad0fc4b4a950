"""The depthwise kernels' tap loops (csrc/mbconv.hip: mb_dw_bwd_kernel's data gradient by base address + fixed offsets at
stride 1 and by the pixel's parity class at stride 2, its weight-gradient loop, mb_dw_fwd_kernel's stencil) through ops_mb.mb_chain, the
way tests/test_gpu_mbchain_cases.py runs it, at the smallest shapes at which those loops can still go wrong.

Two checks per case, on the GPU:
  * against the fp64 evaluation of tests/mbchain_ref.py: every output and every gradient under the three bars of
    tests/test_gpu_mbchain_cases.py (OUT_BAR, GRAD_BAR, RATIO_BOUND: imported, not restated);
  * against the earlier loops in the same process (rn_set_mb_dw_taps): rn_mb_depthwise_bwd is called with the chain's own
    arguments once per variant, each into buffers of its own.  torch.equal (value equality: -0 == +0) on the data gradient
    g1, on dw and on the gradient rows and planes, at either stride: the stride-2 loop leaves out exact zeros only and keeps
    every pixel on its thread in its order, so the per-channel sums add the same terms in the same order (more than the
    equality of g1 and dw that was asked for at stride 2: what the step computes must not move).  The chain's outputs (the
    forward stencil) and every gradient are equal under either variant.

The cases and the instantiation of mb_dw_bwd_kernel<ACT, MULTI, S, TAPS, NPA, NPD, PF> each one reaches (slab = channels per
block, tile and tiles per block tpb from dw_slab / dw_bwd_plan / dw_tiles_per_block; the rows per sample the planner query
returns = tiles / tpb are checked below without a GPU, as tests/test_mbchain_cases_cpu.py does for its table):
  a   2, 16x16, 192 ch, stride 2, elu, rate 0.2, device counter 3: slab 48, 4x4 tiles (all four parity classes among the 16
      pixels of one pass over the 21 pixel lanes), tpb 1: <ELU, false, 2>; pad_t = pad_l = 0; the dropout mask in the epilogue
  b   1, 128x5, stride 2: odd width, pad_l = 1, ow = 3; 32x2 tiles of 4x4, the second tile column holds one image column:
      <ELU, false, 2>
  c   1, 5x128, stride 2: odd height, pad_t = 1; the second tile row holds one image row
  d   1, 20x16, 144 ch, stride 1: slab 36, 5x4 tiles of 4x4 (the planner halves the 8-row tile of this small map, so 20 rows
      are whole tiles): <ELU, false, 1>
  d2  1, 18x32, stride 1: 5x8 tiles of 4x4, the last tile row holds two image rows: the taps at a ragged bottom edge
  e   1, 128x128, 96 ch, stride 2: slab 48, 8x8 tiles (four passes over the lanes), 512 blocks: tpb 1, <ELU, false, 2>
  e2  as e with n = 2: 1024 blocks, tpb 2, 5 + 2 patch loads per thread: the prefetching <ELU, true, 2, TAPS, 5, 2, true>
  f   as a with relu6, no dropout: <RELU6, true, 2>; the seed keeps every pre-activation off the kinks (checked below)
  g   1, 128x128, 144 ch, stride 1 (the shape of mbchain_ref case 10): tpb 2: the prefetching <ELU, true, 1, TAPS, 4, 4, true>
b and c stand for 64x5 and 5x64, whose 32x3 and 3x32 outputs (96 pixels) the pointwise kernels do not take (a multiple of 64
pixels per sample): twice the long side reaches the same paddings and ragged tiles.  e alone does not reach tpb > 1 (one
sample gives 512 blocks), d alone no ragged tile: e2 and d2 do.

Measured on an MI355X with either variant (the figures agree to the digits shown): the largest ratio of any tensor of any
case is 3.26 (d2, the gradient of the tail kernel -- a pointwise product that the depthwise kernels do not enter: ek 1.0e-6,
e32 3.1e-7), the next 1.60 (d, the same tensor); no gradient that the depthwise backward feeds exceeds 1.33.  The kernels
are bitwise reproducible, so these figures do not move from run to run.

The CPU tests carry no gpu mark: they run wherever the library builds."""
import ctypes as C

import pytest
import torch

import mbchain_ref as R
import test_gpu_mbchain_cases as G
from oracle import tf_ops_ref as T

BLOCK_S2 = (32, 192, 64, 2, False)
CASES = {
    "a": R._case(2, 16, 16, BLOCK_S2, rate=0.2, counter=3),
    "b": R._case(1, 128, 5, BLOCK_S2, rate=0.2),
    "c": R._case(1, 5, 128, BLOCK_S2, rate=0.2),
    "d": R._case(1, 20, 16, (24, 144, 32, 1, False), rate=0.2),
    "d2": R._case(1, 18, 32, (24, 144, 32, 1, False), rate=0.2),
    "e": R._case(1, 128, 128, (16, 96, 24, 2, False), rate=0.2),
    "e2": R._case(2, 128, 128, (16, 96, 24, 2, False), rate=0.2),
    "f": R._case(2, 16, 16, BLOCK_S2, act="relu6", seed=1),
    "g": R._case(1, 128, 128, (24, 144, 24, 1, True)),
}
# rows per sample of rn_mb_depthwise_bwd_rows (= blocks per sample and slab), (pad_t, pad_l)
EXPECT = {"a": (16, (0, 0)), "b": (64, (0, 1)), "c": (64, (1, 0)), "d": (20, (1, 1)), "d2": (40, (1, 1)), "e": (256, (0, 0)),
          "e2": (128, (0, 0)), "f": (16, (0, 0)), "g": (128, (1, 1))}
KEY = "dw-taps-%s"


@pytest.fixture(autouse=True)
def _table(monkeypatch):
    """The cases under keys of their own in mbchain_ref.CASES for the length of a test: run_chain / measure / reference of
    tests/test_gpu_mbchain_cases.py then serve them unchanged (reference() computes each fp64 / fp32 evaluation once)."""
    for k, case in CASES.items():
        monkeypatch.setitem(R.CASES, KEY % k, case)


@pytest.fixture()
def taps():
    import _rn
    L = _rn.lib()
    before = L.rn_get_mb_dw_taps()
    yield L.rn_set_mb_dw_taps
    L.rn_set_mb_dw_taps(before)


# ---- without a GPU
@pytest.mark.parametrize("k", list(CASES))
def test_case_is_supported_and_takes_its_branch(k):
    import _rn
    import ops
    import ops_mb
    L = _rn.lib()
    case = CASES[k]
    spec = case.specs[0]
    assert all(h * w % 64 == 0 for h, w in R.out_hw(case))
    assert ops_mb.chain_supported((case.n, case.h, case.w, spec.cin), R.make_case(case)[1])
    lay = _rn.MbRows()
    assert L.rn_mb_depthwise_bwd_rows(case.n, case.h, case.w, spec.wide, spec.stride, ops.gn_groups(spec.wide, 32), C.byref(lay))
    pads = (T.same_pad_1d(case.h, 3, spec.stride)[1], T.same_pad_1d(case.w, 3, spec.stride)[1])
    assert (lay.rows_per_sample, pads) == EXPECT[k], "case %s left its branch: pick another shape for it" % k


def test_switch_sets_and_reads_back(taps):
    import _rn
    L = _rn.lib()
    for v in (0, 1, 0, 5):
        assert taps(v) == 0 and L.rn_get_mb_dw_taps() == (1 if v else 0)


def test_relu6_case_sits_on_no_kink():
    """As tests/test_mbchain_cases_cpu.py picks its seeds: the first one whose smallest distance of a pre-activation from 0 / 6
    (fp64 reference) exceeds KINK_MARGIN; pinned, so that a change of the generator is noticed."""
    margin = R.kink_margin(CASES["f"])
    assert margin > R.KINK_MARGIN, margin
    assert abs(margin - 1.4305e-5) < 2e-8, margin


# ---- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("k", list(CASES))
def test_case_matches_fp64(k):
    import _rn
    variant = _rn.lib().rn_get_mb_dw_taps()                # (1 unless the environment says RN_MB_DW_TAPS=0: the same bars hold)
    dev = torch.device("cuda:0")
    rows = G.measure(KEY % k, False, dev)
    for kind in ("out", "grad"):
        print("case %s (taps %d) worst %s ratio: %s ek %.3e e32 %.3e ratio %.2f" % ((k, variant, kind) + G.worst(rows, kind)[1:]))
    bad = ["%s %s: ek %.3e (bar %.0e), e32 %.3e, ratio %.2f (bound %s)" % (kind, name, ek, G.OUT_BAR if kind == "out" else G.GRAD_BAR, e32, ratio, G.RATIO_BOUND)
           for kind, name, ek, e32, ratio in rows
           if ek > (G.OUT_BAR if kind == "out" else G.GRAD_BAR) or ratio > G.RATIO_BOUND]
    assert not bad, "case %s: %d of %d tensors off: %s" % (k, len(bad), len(rows), "; ".join(bad))


def _both_variants(monkeypatch, L):
    """Wrap rn_mb_depthwise_bwd: before the chain's own call, the same arguments once per variant into fresh NaN-filled
    buffers -> list of {variant: (g1, dw, rows, planes)} per depthwise backward launch."""
    import _rn
    real = L.rn_mb_depthwise_bwd
    seen = []

    def call(nm, dy, w, dw, gout, n, h, wd, stride, ws, ws_bytes, st, defer):
        g, c = gout._obj, nm._obj.c
        dev = torch.device("cuda:0")
        R_, W_ = g.grows.rows_per_sample, g.grows.width
        need = L.rn_mb_depthwise_bwd_workspace(n, h, wd, c, stride)
        res = {}
        for variant in (0, 1):
            def buf(*shape):
                return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)

            g1, dwt, rows, planes = buf(n, h, wd, c), buf(3, 3, c), buf(n * R_, W_, 2), buf(2, n * R_, c)
            wsp = torch.empty((need,), dtype=torch.uint8, device=dev)
            alt = _rn.MbGout(g1.data_ptr(), None, None, g.norm, 0, _rn.MbRows(rows.data_ptr(), R_, W_, g.grows.bn), planes.data_ptr())
            L.rn_set_mb_dw_taps(variant)
            _rn.check(real(nm, dy, w, dwt.data_ptr(), C.byref(alt), n, h, wd, stride, wsp.data_ptr(), need, st, None), "rn_mb_depthwise_bwd")
            res[variant] = (g1, dwt, rows, planes, wsp)
        seen.append((stride, res))
        return real(nm, dy, w, dw, gout, n, h, wd, stride, ws, ws_bytes, st, defer)

    monkeypatch.setattr(L, "rn_mb_depthwise_bwd", call)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("k", list(CASES))
def test_new_loops_equal_the_earlier_ones(k, taps, monkeypatch):
    import _rn
    L = _rn.lib()
    dev = torch.device("cuda:0")
    stride = CASES[k].specs[0].stride
    taps(0)
    out_old, grads_old = G.run_chain(KEY % k, False, dev)
    taps(1)
    seen = _both_variants(monkeypatch, L)
    out_new, grads_new = G.run_chain(KEY % k, False, dev)
    torch.cuda.synchronize()
    assert L.rn_get_mb_dw_taps() == 1 and len(seen) == 1 and seen[0][0] == stride
    (g1_o, dw_o, rows_o, planes_o, _), (g1_n, dw_n, rows_n, planes_n, _) = seen[0][1][0], seen[0][1][1]
    for name, t in (("g1", g1_n), ("dw", dw_n), ("rows", rows_n), ("planes", planes_n)):
        assert torch.isfinite(t).all(), name
    assert torch.equal(g1_n, g1_o), "g1: %d elements differ" % int((g1_n != g1_o).sum())
    assert torch.equal(dw_n, dw_o), "dw"
    assert torch.equal(dw_n.reshape(-1), grads_new["b0.wd"].reshape(-1)), "the chain's own launch"
    for name in out_new:                                   # the forward stencil
        assert torch.equal(out_new[name], out_old[name]), name
    assert torch.equal(grads_new["b0.wd"], grads_old["b0.wd"])
    assert torch.equal(rows_n, rows_o), "rows"
    assert torch.equal(planes_n, planes_o), "planes"
    for name in grads_new:
        assert torch.equal(grads_new[name], grads_old[name]), name
