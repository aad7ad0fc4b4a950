"""rn_conv2d_fwd / _fwd_stats / _dgrad / _wgrad / _bwd / _bias_grad and rn_gemm_batched at every branch of their dispatch against
the fp64 reference of tests/conv_ref.py.

The entry points are driven directly (ctypes structs), so that the workspace, the channel slices, dw's old content and the
defer list are in the test's hands.  Every call first asserts, through rn_conv2d_plan with the real pointers and the real
workspace size, that it runs the branch tests/test_conv_cases_cpu.py lists for it.  The workspace is what the case's rule
says -- exactly rn_conv2d_*_workspace bytes, NULL, or one byte less -- followed by a guard area that must stay untouched.
Outputs are pre-filled with a sentinel and must be written everywhere; x's buffer comes back bit-unchanged; for channel
slices the channels of dx's buffer outside [x_coff, x_coff + cin) come back bit-unchanged; with accumulate dw is the old
content plus the gradient; with a defer list dw is untouched until rn_flush_reductions and the list holds one entry.

Every y, statistic row, dx, dw and dbias is compared with the fp64 reference, each against its own maximum (helpers.rel_err),
under two bars:
  * the project's: outputs and statistic rows 1e-4 (BASELINE north_star), gradients 5e-4 (what tests/test_gpu_wino_tower.py
    and tests/test_gpu_gn_cases.py grant);
  * one tied to the arithmetic: with e32 = rel_err(reference in fp32, reference in fp64) and ek = rel_err(kernel, fp64),
    ek / max(e32, 2^-23) <= RATIO_BOUND[family].  e32 comes from the reference alone.  Families (conv_ref.family): the
    split-bf16 products (1x1 and patch matrix: three bf16 pieces per operand, six products with fp32 accumulation); the fp32
    kernels (implicit GEMM on the fp32 matrix cores, stem, direct grouped kernels: fmaf chains); and, split from them by
    design, the fp32 weight gradient whose split runs in windows: there ONE accumulator takes 1026 .. 2100 products in a
    row, where every other weight gradient cuts the pixel range into splits of 64 .. 1024 and sums the slabs afterwards.
RATIO_BOUND = {fp32: 8, fp32-long: 16, split-bf16: 8}, set on 2026-10-20: per family twice the largest ratio of any tensor of
any call of that family in one run of the table on an MI355X, rounded up to a power of two (figures:
profiles/conv_cases_err.txt, 181 lines).  The kernels are bitwise reproducible, so the figures have no run-to-run noise.
  fp32:        largest ratio 3.34 (dense-cfg1-dgrad-cfg3, the data gradient: a chain of 4608 products per element without
               split-K; ek 2.5e-6, e32 7.4e-7); next 2.66 (gconv-cg32, direct grouped data gradient), the rest <= 2.5
  fp32-long:   largest ratio 6.10 (wg-window-1k, dw: ek 1.1e-6, e32 1.8e-7); 4.62 at 2052 pixels, 2.88 unforced (wg-window-own)
  split-bf16:  largest ratio 2.08 (x3-1x1-m128, dw: ek 4.7e-7, e32 2.3e-7); forward and data gradient <= 1.5
The largest ek of any tensor of any call is that 2.5e-6 (an output: 1.5e-6, patch-none): every family stays a factor of 40
or more inside the project's bars."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_ref as R
from helpers import rel_err
from test_conv_cases_cpu import EXPECT, GEMM_EXPECT, PROCESS_ROWS

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
RATIO_BOUND = {R.FP32: 8.0, R.FP32_LONG: 16.0, R.X3: 8.0}
SENTINEL = 12345.0
GUARD = 1 << 16
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


def _sentinel(shape, dev):
    return torch.full(tuple(shape), SENTINEL, device=dev)


def _written(t, what):
    assert not bool((t == SENTINEL).any()), "%s: elements were not written" % what


class Buffers:
    """The device tensors of a case: x (inside its wider buffer for channel slices), w, bias, dy."""

    def __init__(self, case, dev):
        xs, w, b, dys, dw0 = R.make_case(case)
        gen = torch.Generator().manual_seed(11)
        self.case, self.dev = case, dev
        self.lo, self.hi = case.x_coff, case.x_coff + case.cin
        self.xbufs = []
        for x in xs:
            if case.x_ld:
                buf = torch.randn(tuple(x.shape[:3]) + (case.x_ld,), generator=gen)
                buf[..., self.lo:self.hi] = x
                self.xbufs.append(buf.to(dev))
            else:
                self.xbufs.append(x.to(dev).contiguous())
        self.xkeep = [t.clone() for t in self.xbufs]
        self.w = w.to(dev).contiguous()
        self.bias = b.to(dev) if b is not None else None
        self.dys = [d.to(dev).contiguous() for d in dys]
        self.dw0 = dw0
        self.dx_old = [torch.randn(tuple(t.shape), generator=gen) if case.x_ld else None for t in self.xbufs]

    def x_unchanged(self):
        for t, k in zip(self.xbufs, self.xkeep):
            assert torch.equal(t, k), "x's buffer changed"


def run_op(case, name, op, dev, monkeypatch, bufs=None):
    """One call of `op` for the case -> (dict of numpy arrays named like conv_ref.run_ref's, plus 'rows'; the plan row)"""
    import _rn
    L = _rn.lib()
    R.configure(case, monkeypatch)
    b = bufs or Buffers(case, dev)
    segs, nseg, geom = R.host_call(case)
    ys = [_sentinel(d.shape, dev) for d in b.dys]
    dxs = [o.to(dev) if o is not None else _sentinel(x.shape, dev) for o, x in zip(b.dx_old, b.xbufs)]
    for i, s in enumerate(segs):
        s.x, s.wgt, s.y, s.dy, s.dx = b.xbufs[i].data_ptr(), b.w.data_ptr(), ys[i].data_ptr(), b.dys[i].data_ptr(), dxs[i].data_ptr()
        s.bias = b.bias.data_ptr() if b.bias is not None else None
    dw = b.dw0.to(dev).contiguous() if case.accumulate and op == "wgrad" else _sentinel(b.w.shape, dev)
    dw_before = dw.clone()
    need = R.workspace_need(case, op, segs, nseg, geom)
    given, null = R.workspace_given(case, op, need)
    ws = torch.full((given + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    wsp = None if null else ws.data_ptr()
    lst = _rn.ReduceList.make() if case.defer and op in ("wgrad", "bwd", "bias_grad") else None
    lp = C.byref(lst) if lst is not None else None
    out, row = {}, None
    if op != "bias_grad":
        expect = EXPECT[name][op]
        refused = expect[0] == "refused"
        plan = R.query(case, op, segs, nseg, geom, given, wsp, dw.data_ptr(), status=EUNSUPPORTED if refused else 0)
        row = R.row_of(plan, op)
        assert ("refused",) + row == expect if refused else row == expect, "%s %s takes %s, not %s" % (name, op, row, expect)
    if op == "fwd":
        _rn.check(L.rn_conv2d_fwd(segs, nseg, C.byref(geom), wsp, given, _rn.stream()), "rn_conv2d_fwd")
    elif op == "fwd_stats":
        layout = _rn.GnRows()
        nbytes = L.rn_conv2d_stats_rows(segs, nseg, C.byref(geom), given, case.stats, C.byref(layout))
        n = case.segs[0][0]
        if refused:
            assert nbytes == 0
            rows = _sentinel((n, case.cout, 2), dev)
            req = _rn.GnRows(rows.data_ptr(), 1, 0, case.stats)
            assert L.rn_conv2d_fwd_stats(segs, nseg, C.byref(geom), wsp, given, C.byref(req), _rn.stream()) == EUNSUPPORTED
            torch.cuda.synchronize()
            assert bool((rows == SENTINEL).all()) and bool((ys[0] == SENTINEL).all()), "a refused call wrote"
            return out, row
        rps = plan.call.rows_per_sample
        assert (layout.rows_per_sample, layout.per_group, layout.groups) == (rps, 0, case.stats) and nbytes == n * rps * case.cout * 8
        rows = _sentinel((n * rps, case.cout, 2), dev)
        guard = torch.full((GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        req = _rn.GnRows(rows.data_ptr(), rps, 0, case.stats)
        _rn.check(L.rn_conv2d_fwd_stats(segs, nseg, C.byref(geom), wsp, given, C.byref(req), _rn.stream()), "rn_conv2d_fwd_stats")
        torch.cuda.synchronize()
        _written(rows, "statistic rows")
        assert bool((guard == 0xA5).all())
        out["rows"] = rows.cpu().numpy()
    elif op == "dgrad":
        _rn.check(L.rn_conv2d_dgrad(segs, nseg, C.byref(geom), wsp, given, _rn.stream()), "rn_conv2d_dgrad")
    elif op == "wgrad":
        _rn.check(L.rn_conv2d_wgrad(segs, nseg, C.byref(geom), dw.data_ptr(), 1 if case.accumulate else 0, wsp, given, _rn.stream(), lp),
                  "rn_conv2d_wgrad")
    elif op == "bwd":
        _rn.check(L.rn_conv2d_bwd(segs, nseg, C.byref(geom), dw.data_ptr(), wsp, given, _rn.stream(), lp), "rn_conv2d_bwd")
    else:
        dbias = _sentinel((case.cout,), dev)
        dw_before, dw = dbias.clone(), dbias
        _rn.check(L.rn_conv2d_bias_grad(segs, nseg, C.byref(geom), dbias.data_ptr(), wsp, given, _rn.stream(), lp), "rn_conv2d_bias_grad")
    torch.cuda.synchronize()
    if lst is not None:
        assert torch.equal(dw, dw_before), "the gradient changed before the flush"
        assert lst.count == 1, lst.count
        _rn.check(L.rn_flush_reductions(lp, _rn.stream()), "rn_flush_reductions")
        torch.cuda.synchronize()
    assert bool((ws[given:] == 0xA5).all()), "%s %s wrote behind its workspace" % (name, op)
    b.x_unchanged()
    if op in ("fwd", "fwd_stats"):
        for i, y in enumerate(ys):
            _written(y, "y%d" % i)
            out["y%d" % i] = y.cpu().numpy()
    if op in ("dgrad", "bwd"):
        for i, dx in enumerate(dxs):
            dx = dx.cpu()
            if b.dx_old[i] is not None:
                keep = torch.ones(case.x_ld, dtype=torch.bool)
                keep[b.lo:b.hi] = False
                assert torch.equal(dx[..., keep], b.dx_old[i][..., keep]), "channels outside the slice of dx's buffer changed"
                assert not torch.equal(dx[..., b.lo:b.hi], b.dx_old[i][..., b.lo:b.hi])
                out["dx%d" % i] = dx[..., b.lo:b.hi].numpy()
            else:
                _written(dx, "dx%d" % i)
                out["dx%d" % i] = dx.numpy()
    if op in ("wgrad", "bwd"):
        if case.accumulate and op == "wgrad":
            out["dw"] = (dw.cpu().double() - b.dw0.double()).numpy()        # dw = old + gradient
        else:
            _written(dw, "dw")
            out["dw"] = dw.cpu().numpy()
    if op == "bias_grad":
        _written(dw, "dbias")
        out["dbias"] = dw.cpu().numpy()
    return out, row


def families(op, row):
    """tensor name prefix -> family of the call that wrote it"""
    if op == "bias_grad":
        return {"dbias": R.FP32}
    if op == "bwd":
        return {"dx": R.family(row[2]), "dw": R.family(row[3])}
    return {"": R.family(row)}


def compare(case, op, row, got):
    """-> [(kind, tensor, family, ek, e32, ratio)]; kind: 'out' (y, rows) or 'grad'"""
    ref64, ref32 = R.run_ref(case, torch.float64), R.run_ref(case, torch.float32)
    fam = families(op, row)
    rows = []
    for tname in sorted(got):
        if tname == "rows":
            rps = got[tname].shape[0] // case.segs[0][0]
            r64, r32 = R.stat_rows(ref64["y0"], rps), R.stat_rows(ref32["y0"], rps)
        else:
            r64, r32 = ref64[tname], ref32[tname]
        assert got[tname].shape == r64.shape, (tname, got[tname].shape, r64.shape)
        ek, e32 = rel_err(got[tname], r64), rel_err(r32, r64)
        f = next(v for k, v in fam.items() if tname.startswith(k))
        rows.append(("out" if tname[0] in "yr" else "grad", tname, f, ek, e32, ek / max(e32, 2.0 ** -23)))
    return rows


def record_lines(name, op, rows):
    """The call's lines of profiles/conv_cases_err.txt."""
    return ["CONV_ERR %-24s %-9s %-10s %-5s ek %.3e  e32 %.3e  ratio %7.2f" % (name, op, f, tname, ek, e32, ratio) for _, tname, f, ek, e32, ratio in rows]


def check(name, op, rows):
    bad = ["%s %s: ek %.3e (bar %.0e), e32 %.3e, ratio %.2f (bound %s)" % (kind, tname, ek, OUT_BAR if kind == "out" else GRAD_BAR, e32, ratio, RATIO_BOUND[f])
           for kind, tname, f, ek, e32, ratio in rows
           if ek > (OUT_BAR if kind == "out" else GRAD_BAR) or ratio > RATIO_BOUND[f]]
    assert not bad, "%s %s: %s" % (name, op, "; ".join(bad))


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matches_fp64(dev, monkeypatch, name):
    case = R.CASES[name]
    bufs = Buffers(case, dev)
    failures = []
    for op in case.ops:
        got, row = run_op(case, name, op, dev, monkeypatch, bufs)
        if not got:
            continue                                    # a refusal: asserted in run_op
        rows = compare(case, op, row, got)
        print("\n".join(record_lines(name, op, rows)))
        try:
            check(name, op, rows)
        except AssertionError as e:                     # (every op's figures are printed before the case fails)
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(R.GEMMS))
def test_batched_product_matches_fp64(dev, name):
    import _rn
    L = _rn.lib()
    m, k, n, nb, b_nk, mode = R.GEMMS[name]
    row = R.gemm_row(name)                              # (sets the product mode)
    assert row == GEMM_EXPECT[name], "%s takes %s" % (name, row)
    a, b = R.gemm_data(name)
    ad, bd, c = a.to(dev).contiguous(), b.to(dev).contiguous(), _sentinel((nb, m, n), dev)
    _rn.check(L.rn_gemm_batched(ad.data_ptr(), bd.data_ptr(), c.data_ptr(), m, k, n, nb, b_nk, _rn.stream()), "rn_gemm_batched")
    torch.cuda.synchronize()
    L.rn_set_product_mode(1)
    _written(c, "C")
    r64, r32 = R.gemm_ref(name, torch.float64), R.gemm_ref(name, torch.float32)
    ek, e32 = rel_err(c.cpu().numpy(), r64), rel_err(r32, r64)
    rows = [("out", "y", R.family(row), ek, e32, ek / max(e32, 2.0 ** -23))]
    print("\n".join(record_lines(name, "gemm", rows)))
    check(name, "gemm", rows)


def test_no_splitk_equals_null_workspace(dev, monkeypatch):
    """RN_NO_SPLITK and a NULL workspace are the same plain kernel: the same bits."""
    for op in ("fwd", "dgrad"):
        a, _ = run_op(R.CASES["splitk-off"], "splitk-off", op, dev, monkeypatch)
        b, _ = run_op(R.CASES["splitk-none"], "splitk-none", op, dev, monkeypatch)
        c, _ = run_op(R.CASES["splitk-short"], "splitk-short", op, dev, monkeypatch)
        for k in a:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (op, k)


def _reduces(op, row):
    """whether the call ends in a row reduction of split partial results"""
    if op == "bias_grad":
        return True
    if op == "bwd":
        return _reduces("dgrad", row[2]) or _reduces("wgrad", row[3])
    if row[0] == "fp32":
        return row[3] > 1
    return op == "wgrad" and row[0] in ("x3_1x1", "x3_patch", "direct_grouped")


# every call of the table with nsplit > 1: split-K forward / data gradient, the weight gradients of every path, the merged
# backward launch, the bias gradient
REPEAT = [(name, op) for name, case in R.CASES.items() for op in case.ops if op != "fwd_stats" and _reduces(op, EXPECT[name].get(op))]


@pytest.mark.parametrize("name,op", REPEAT)
def test_second_call_is_bit_identical(dev, monkeypatch, name, op):
    """Fixed-order reductions: a second identical call gives identical bits."""
    a, _ = run_op(R.CASES[name], name, op, dev, monkeypatch)
    b, _ = run_op(R.CASES[name], name, op, dev, monkeypatch)
    assert a and sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


class _Env:
    """monkeypatch's two calls, for the child process below"""

    def delenv(self, name, raising=False):
        os.environ.pop(name, None)

    def setenv(self, name, value):
        os.environ[name] = value


def _child(name):
    """(in a fresh process started with the switch) the ops of conv_ref.EXTRA[name] like test_case_matches_fp64"""
    dev = torch.device("cuda:0")
    case = R.EXTRA[name]
    R.PROCESS_SWITCHES = ()
    row = PROCESS_ROWS["RN_X3_IM2COL_PIECE_MB"][3]
    ohw = np.prod(R.out_hw(case, *case.segs[0][1:]))
    EXPECT[name] = {"fwd": row, "fwd_stats": row + (int(ohw) // row[1],)}
    bufs = Buffers(case, dev)
    for op in case.ops:
        got, r = run_op(case, name, op, dev, _Env(), bufs)
        rows = compare(case, op, r, got)
        print("\n".join(record_lines(name, op, rows)))
        check(name, op, rows)


def test_patch_matrix_in_pieces(dev):
    """RN_X3_IM2COL_PIECE_MB is read once per process: the forward call (and its statistic rows, each piece's in their place) of
    a batch whose patch matrix is built in two pieces, in a fresh process."""
    value, name, _, row = PROCESS_ROWS["RN_X3_IM2COL_PIECE_MB"]
    assert row[0] == "x3_patch" and row[2] < R.EXTRA[name].segs[0][0]
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [os.path.dirname(here), os.path.join(os.path.dirname(here), "retinanet-tensorflow_amd"), here]
    code = "import sys; sys.path[:0] = %r; import test_gpu_conv_cases as G; G._child(%r)" % (paths, name)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RN_X3_IM2COL_PIECE_MB=value), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
