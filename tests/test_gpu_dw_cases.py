"""rn_depthwise_fwd / _fwd_stats / _dgrad / _wgrad / _bwd at every branch of their host decision against the fp64 reference of
tests/dw_ref.py.

The entry points are driven directly (ctypes).  Every case first asserts, through rn_depthwise_plan, that it runs the branch
tests/test_dw_cases_cpu.py lists for it.  Per entry point: outputs are pre-filled with a sentinel and must be written everywhere;
x, w and dy come back bit-unchanged; the workspace (and the statistics rows) are exactly the size the library asks for, followed
by a guard area that must stay untouched; one byte less returns RN_EWORKSPACE and leaves dw alone; a second call gives the same
bits; rn_depthwise_fwd_stats writes the y of rn_depthwise_fwd bit for bit; rn_depthwise_bwd writes the dx of rn_depthwise_dgrad
and the dw of rn_depthwise_wgrad bit for bit.  The generic cases (k != 3): rn_depthwise_wgrad and rn_depthwise_bwd return
RN_EUNSUPPORTED and leave dw and dx bit-unchanged.

Two bars, both against fp64 (helpers.rel_err divides by the tensor's maximum):
  * the project's: y and the statistic rows 1e-4 (BASELINE north_star), gradients 5e-4 (what tests/test_gpu_conv_cases.py grants);
  * per element, from the arithmetic alone and for any summation order: |got - ref64| <= (T + 1) 2^-24 sum|terms| with T the
    products summed into the element (k^2 for y, the valid taps for dx, n oh ow for dw) and sum|terms| from the reference run on
    |x|, |w|, |dy|; for a statistics row T = chunk pixels x channels per group over |y| resp. y^2, plus what the rows inherit
    from the fp32 y they sum.  (First order in 2^-24: at T = 34848, the dw of grid-cap, the rigorous worst case is 0.2 % larger;
    measured errors stay far below either, see `bound` below.)
Measured on an MI355X on 2026-10-21 (profiles/dw_cases_err.txt; ek = rel_err(kernel, fp64), e32 = rel_err(reference in fp32,
fp64) -- from the reference alone --, bound = the largest |got - ref64| / bound of any element):
  tensor  worst ek (case)             its e32    ek / e32   worst ratio ek / max(e32, 2^-23)   worst bound (case)
  y       1.51e-7 (k5-s1)             1.51e-7    1.00       1.00                               0.486 (k1)
  rows    2.56e-7 (stats-r8)          1.80e-7    1.43       1.74 (c1024)                       0.129 (c4-row)
  dx      1.60e-7 (stats-r8)          1.60e-7    1.00       1.00                               0.604 (k3-s2-even)
  dw      1.73e-7 (stats-r16)         4.60e-6    0.04       1.31 (k3-s3)                       0.169 (c4-1x1)
y and dx equal the fp32 reference's own error in most cases (the same nine products in a fused chain); the weight gradient of
the large maps is 25 x closer to fp64 than the fp32 reference, whose single running sum over 18 496 pixels the kernel's
chunked sums avoid.
The kernels are bitwise reproducible, so the figures have no run-to-run noise."""
import ctypes as C

import numpy as np
import pytest
import torch

import dw_ref as R
from helpers import rel_err
from test_dw_cases_cpu import EXPECT

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
SENTINEL = 12345.0
GUARD = 1 << 16
FILL = 0xA5
FILL_WORD = -1515870811          # 0xA5A5A5A5 as int32
EUNSUPPORTED, EWORKSPACE = -2, -4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


def _sent(shape, dev):
    return torch.full(tuple(shape), SENTINEL, device=dev)


def _written(t):
    return not bool((t == SENTINEL).any())


def _untouched(t):
    return bool((t == SENTINEL).all())


class Run:
    """The device tensors of one case and the calls on them."""

    def __init__(self, name, dev):
        import _rn
        self.L, self.rn, self.dev = _rn.lib(), _rn, dev
        self.name, self.case = name, R.CASES[name]
        case = self.case
        st, self.plan = R.query(case)
        assert st == 0 and R.row_of(self.plan) == EXPECT[name], "the calls take %s, not %s" % (R.row_of(self.plan), EXPECT[name])
        self.host = R.make_case(case)
        self.x, self.w, self.dy = (t.to(dev) for t in self.host)
        self.keep = [t.clone() for t in (self.x, self.w, self.dy)]
        self.shape = (case.n, case.h, case.w, case.c, case.k, case.s)
        self.need = self.L.rn_depthwise_wgrad_workspace(*self.shape)
        assert self.need == self.plan.wgrad_workspace_bytes > 0

    def inputs_unchanged(self):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip((self.x, self.w, self.dy), self.keep))

    def fwd(self):
        y = _sent(self.dy.shape, self.dev)
        self.rn.check(self.L.rn_depthwise_fwd(self.rn.f32(self.x), self.rn.f32(self.w), self.rn.f32(y), *self.shape, self.rn.stream()), "rn_depthwise_fwd")
        return y

    def fwd_stats(self):
        """-> (y, rows [n, rows per sample, groups, 2])"""
        case, plan = self.case, self.plan
        lay = self.rn.GnRows()
        nbytes = self.L.rn_depthwise_stats_rows(*self.shape, case.groups, C.byref(lay))
        assert nbytes == plan.stats_blocks * case.groups * 8 > 0
        raw = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        lay.rows = raw.data_ptr()
        y = _sent(self.dy.shape, self.dev)
        self.rn.check(self.L.rn_depthwise_fwd_stats(self.rn.f32(self.x), self.rn.f32(self.w), self.rn.f32(y), *self.shape, C.byref(lay), self.rn.stream()),
                      "rn_depthwise_fwd_stats")
        torch.cuda.synchronize()
        assert bool((raw[nbytes:] == FILL).all()), "the call wrote behind its rows"
        assert not bool((raw[:nbytes].view(torch.int32) == FILL_WORD).any()), "a row was not written"
        return y, raw[:nbytes].view(torch.float32).reshape(case.n, plan.stats_rows_per_sample, case.groups, 2).clone()

    def dgrad(self):
        dx = _sent(self.x.shape, self.dev)
        self.rn.check(self.L.rn_depthwise_dgrad(self.rn.f32(self.dy), self.rn.f32(self.w), self.rn.f32(dx), *self.shape, self.rn.stream()), "rn_depthwise_dgrad")
        return dx

    def workspace(self):
        return torch.full((self.need + GUARD,), FILL, dtype=torch.uint8, device=self.dev)

    def guard_ok(self, ws):
        torch.cuda.synchronize()
        return bool((ws[self.need:] == FILL).all())

    def wgrad_status(self, dw, ws, nbytes, defer=None):
        return self.L.rn_depthwise_wgrad(self.rn.f32(self.x), self.rn.f32(self.dy), self.rn.f32(dw), *self.shape, ws.data_ptr(), nbytes, self.rn.stream(),
                                         C.byref(defer) if defer is not None else None)

    def bwd_status(self, dx, dw, ws, nbytes, defer=None):
        return self.L.rn_depthwise_bwd(self.rn.f32(self.x), self.rn.f32(self.dy), self.rn.f32(self.w), self.rn.f32(dx), self.rn.f32(dw), *self.shape,
                                       ws.data_ptr(), nbytes, self.rn.stream(), C.byref(defer) if defer is not None else None)


def _frac(err, bound):
    """max over the elements of err / bound (an element whose bound is 0 -- no term reaches it -- must be exact)"""
    assert not np.any((bound == 0) & (err > 0)), "an element no term reaches is not zero"
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def compare(got, ref64, ref32, bnd):
    """-> [(tensor, ek, e32, ratio, bound fraction)]"""
    out = []
    for t in sorted(got):
        ek, e32 = rel_err(got[t], ref64[t]), rel_err(ref32[t], ref64[t])
        out.append((t, ek, e32, ek / max(e32, 2.0 ** -23), _frac(np.abs(got[t].astype(np.float64) - ref64[t]), bnd[t])))
    return out


def record_line(name, rows):
    """The case's line of profiles/dw_cases_err.txt."""
    return "DWCASE %-16s " % name + " | ".join("%-4s ek %.3e e32 %.3e ratio %5.2f bound %.3f" % r for r in rows)


def check(name, rows):
    bad = ["%s: ek %.3e (bar %.0e), e32 %.3e, %.3f of the element bound" % (t, ek, GRAD_BAR if t[0] == "d" else OUT_BAR, e32, frac)
           for t, ek, e32, _, frac in rows if ek > (GRAD_BAR if t[0] == "d" else OUT_BAR) or frac > 1.0]
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def references(name):
    case = R.CASES[name]
    if name not in R.LARGE:
        return R.small_case_data(name)[1:]
    x, w, dy = R.make_case(case)
    return R.reference(x, w, dy, case.s, torch.float64), R.reference(x, w, dy, case.s, torch.float32), R.bounds(case, x, w, dy)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matches_fp64(dev, name):
    run = Run(name, dev)
    case, plan = run.case, run.plan
    got = {}
    # ---- forward, twice
    y = run.fwd()
    assert _written(y)
    assert torch.equal(y, run.fwd()), "a second rn_depthwise_fwd gives other bits"
    got["y"] = y.cpu().numpy()
    # ---- forward with statistics
    if plan.stats_r:
        y2, rows = run.fwd_stats()
        assert torch.equal(y2, y), "rn_depthwise_fwd_stats writes another y than rn_depthwise_fwd"
        assert torch.equal(run.fwd_stats()[1], rows), "a second rn_depthwise_fwd_stats gives other rows"
        got["rows"] = rows.cpu().numpy()
    else:
        assert case.k != 3
    # ---- dgrad, twice
    dx = run.dgrad()
    assert _written(dx)
    assert torch.equal(dx, run.dgrad()), "a second rn_depthwise_dgrad gives other bits"
    got["dx"] = dx.cpu().numpy()
    # ---- weight gradient and fused backward
    dw, ws = _sent(run.w.shape, dev), run.workspace()
    dx2, dw2, ws2 = _sent(run.x.shape, dev), _sent(run.w.shape, dev), run.workspace()
    if plan.wgrad_ok:
        assert run.wgrad_status(dw, ws, run.need - 1) == EWORKSPACE and run.bwd_status(dx2, dw2, ws2, run.need - 1) == EWORKSPACE
        torch.cuda.synchronize()
        assert _untouched(dw) and _untouched(dw2) and _untouched(dx2) and bool((ws == FILL).all()) and bool((ws2 == FILL).all())
        run.rn.check(run.wgrad_status(dw, ws, run.need), "rn_depthwise_wgrad")
        run.rn.check(run.bwd_status(dx2, dw2, ws2, run.need), "rn_depthwise_bwd")
        assert run.guard_ok(ws) and run.guard_ok(ws2), "a call wrote behind its workspace"
        assert _written(dw) and _written(dw2) and _written(dx2)
        assert torch.equal(dx2, dx), "rn_depthwise_bwd writes another dx than rn_depthwise_dgrad"
        assert torch.equal(dw2, dw), "rn_depthwise_bwd writes another dw than rn_depthwise_wgrad"
        dw3, ws3 = _sent(run.w.shape, dev), run.workspace()
        run.rn.check(run.wgrad_status(dw3, ws3, run.need), "rn_depthwise_wgrad")
        assert run.guard_ok(ws3) and torch.equal(dw3, dw), "a second rn_depthwise_wgrad gives other bits"
        got["dw"] = dw.cpu().numpy()
    else:
        assert run.wgrad_status(dw, ws, run.need) == EUNSUPPORTED and run.bwd_status(dx2, dw2, ws2, run.need) == EUNSUPPORTED
        torch.cuda.synchronize()
        assert _untouched(dw) and _untouched(dw2) and _untouched(dx2) and bool((ws == FILL).all()) and bool((ws2 == FILL).all())
    assert run.inputs_unchanged()
    # ---- against fp64
    ref64, ref32, bnd = references(name)
    if "rows" in got:
        ref64, ref32, bnd = dict(ref64), dict(ref32), dict(bnd)
        ref64["rows"] = R.stat_rows(ref64["y"], case.groups, plan.stats_ppc)
        ref32["rows"] = R.stat_rows(ref32["y"], case.groups, plan.stats_ppc, np.float32)
        bnd["rows"] = R.stat_bounds(ref64["y"], bnd["y"], case.groups, plan.stats_ppc)
    assert sorted(got) == sorted(k for k in ref64 if k != "dw" or plan.wgrad_ok)
    rows = compare(got, ref64, ref32, bnd)
    print(record_line(name, rows))
    check(name, rows)


def test_deferred_weight_gradient(dev):
    """With a defer list the row reduction of the dw partials is recorded, not launched: dw stays untouched until
    rn_flush_reductions, and then holds the bits of the undeferred call -- for rn_depthwise_wgrad and for rn_depthwise_bwd."""
    run = Run(R.DEFER_CASE, dev)
    dw, ws = _sent(run.w.shape, dev), run.workspace()
    run.rn.check(run.wgrad_status(dw, ws, run.need), "rn_depthwise_wgrad")
    dx = run.dgrad()
    for which in ("wgrad", "bwd"):
        lst = run.rn.ReduceList.make()
        dwd, dxd, wsd = _sent(run.w.shape, dev), _sent(run.x.shape, dev), run.workspace()
        st = run.wgrad_status(dwd, wsd, run.need, lst) if which == "wgrad" else run.bwd_status(dxd, dwd, wsd, run.need, lst)
        run.rn.check(st, which)
        torch.cuda.synchronize()
        assert lst.count == 1 and _untouched(dwd), which
        assert which == "wgrad" or torch.equal(dxd, dx)
        run.rn.check(run.L.rn_flush_reductions(C.byref(lst), run.rn.stream()), "rn_flush_reductions")
        assert run.guard_ok(wsd) and torch.equal(dwd, dw), which
    assert run.inputs_unchanged()
