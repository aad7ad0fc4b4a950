"""The fp16 depthwise 3 x 3 (csrc/depthwise_f16.hip) on the device over the case table of tests/dw_f16_ref.py
(tests/test_dw_f16_cases_cpu.py proves which kernel variant each row takes).

  * every element within dw_f16_ref.element_bound of the fp64 reference (derived in that module's docstring, nothing measured);
  * the statistic rows against fp64 sums of the kernel's own stored y over each chunk, at the bars tests/test_gpu_f16_conv_cases.py
    applies to the conv's rows: |sum y| within M 2^-24 sum |y|, sum y^2 within M 2^-23 sum y^2, M the pixels of the chunk (at most
    M - 1 fp32 additions of partial sums no larger than sum |y|; the squares are exact products of fp16 values rounded once in the
    fused multiply-add); rn_group_norm_finalize of the rows against the fp64 mean / rstd of y at the 1e-5 / 1e-4 that file grants;
  * y is the same tensor with and without the statistics;
  * folded equals materialised: depthwise_norm(P) and depthwise_norm(P.materialise()) are torch.equal on y, mean and rstd for all
    four activations -- the rule test_super_group_conv_with_pending_groupnorm_equals_materialised applies to the fp32-arithmetic fold;
  * zero padding AFTER the activation: with beta != 0 the border outputs of a folded call differ from a call that padded first
    (the reference's own version of this is in the CPU test) and match the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import dw_f16_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_case(case, dev, stats=None):
    """-> (y fp16 numpy, partial [2, n rows, c] numpy or None, plan, (mean, rstd) of the finalised rows or None)"""
    import _rn
    stats = case.stats if stats is None else stats
    x, w, gn = R.make_case(case)
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    d = R.descriptor(case)
    plan = R.query(d)
    y = torch.full((case.n, plan.oh, plan.ow, case.c), float("nan"), dtype=torch.float16, device=dev)
    d.x, d.wgt, d.y = xd.data_ptr(), wd.data_ptr(), y.data_ptr()
    keep = []
    if case.fold:
        keep = [torch.from_numpy(a).to(dev) for a in gn]
        d.in_mean, d.in_rstd, d.in_gamma, d.in_beta = [t.data_ptr() for t in keep]
    partial, fin = None, None
    d.partial = None
    if stats:
        partial = torch.full((2, case.n * plan.rows_per_sample, case.c), float("nan"), dtype=torch.float32, device=dev)
        d.partial = partial.data_ptr()
    _rn.check(_rn.lib().rn_depthwise_fwd_f16(C.byref(d), _rn.stream()), "rn_depthwise_fwd_f16")
    if stats:
        g = case.groups if case.fold else min(case.c, 8)
        mean = torch.empty((case.n, g), dtype=torch.float32, device=dev)
        rstd = torch.empty_like(mean)
        _rn.check(_rn.lib().rn_group_norm_finalize(_rn.f32(partial), case.n, plan.rows_per_sample, plan.oh * plan.ow, case.c, g, R.EPS,
                                                   _rn.f32(mean), _rn.f32(rstd), _rn.stream()), "rn_group_norm_finalize")
        fin = (g, mean.cpu().numpy(), rstd.cpu().numpy())
    torch.cuda.synchronize()
    return y.cpu().numpy(), (partial.cpu().numpy() if stats else None), plan, fin


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_fp64(dev, name):
    case = R.CASES[name]
    ref = R.run_ref(case)
    y, partial, plan, fin = run_case(case, dev)
    assert y.shape == ref.y64.shape
    g64 = y.astype(np.float64)
    assert np.isfinite(g64).all(), "y holds NaN / inf (an element was not written)"
    ratio = np.abs(g64 - ref.y64) / R.element_bound(ref)
    print("DW_F16 %-22s worst element at %.3f of its bound" % (name, ratio.max()))
    worst = [(tuple(int(v) for v in i), float(g64[tuple(i)]), float(ref.y64[tuple(i)]), float(R.element_bound(ref)[tuple(i)])) for i in np.argwhere(ratio > 1)[:4]]
    assert ratio.max() <= 1.0, "%d elements outside the bound, worst at %.3f; (index, got, fp64, bound): %s" % ((ratio > 1).sum(), ratio.max(), worst)
    if not case.stats:
        return
    s1, s2, sa, pixels = R.rows_of(y, plan)
    rows = partial.astype(np.float64)
    assert np.isfinite(rows).all() and rows.shape == (2,) + s1.shape
    b1, b2 = pixels[:, None] * 2.0 ** -24 * sa, pixels[:, None] * 2.0 ** -23 * s2
    e1, e2 = np.abs(rows[0] - s1), np.abs(rows[1] - s2)
    print("DW_F16 %-22s rows: sum %.3f, sum of squares %.3f of their bounds" % (
        name, (e1 / np.maximum(b1, 1e-300)).max(), (e2 / np.maximum(b2, 1e-300)).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all(), "%d sums, %d sums of squares outside their bound" % ((e1 > b1).sum(), (e2 > b2).sum())
    g, mean, rstd = fin
    t = g64.reshape(case.n, -1, g, case.c // g)
    m64, r64 = t.mean((1, 3)), 1.0 / np.sqrt(t.var((1, 3)) + R.EPS)
    assert rel_err(mean, m64) <= 1e-5 and rel_err(rstd, r64) <= 1e-4
    # the statistics epilogue does not change y
    y_plain, _, _, _ = run_case(case, dev, stats=False)
    assert np.array_equal(y_plain.view(np.uint16), y.view(np.uint16))


class _Norm(object):
    """what ops_f16.depthwise_norm reads of a layers.GroupNormalization"""

    def __init__(self, c, groups, dev, seed):
        g = torch.Generator().manual_seed(seed)
        self.gamma = (1 + 0.3 * torch.randn(c, generator=g)).to(dev)
        self.beta = (0.5 + 0.2 * torch.randn(c, generator=g)).to(dev)
        self.groups, self.eps = groups, 1e-5


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("shape", [(2, 9, 12, 96, 1, 16), (3, 33, 17, 144, 2, 24), (2, 2, 3, 24, 1, 8), (1, 16, 16, 960, 2, 32)])
def test_folded_equals_materialised(dev, act, shape):
    import ops_f16
    n, h, w, c, stride, groups = shape
    g = torch.Generator().manual_seed(h * 100 + c)
    raw = (2.0 * torch.randn(n, h, w, c, generator=g) + 0.3).to(dev).half()
    wgt = (torch.randn(3, 3, c, 1, generator=g) / 3).to(dev)
    front, behind = _Norm(c, groups, dev, 1), _Norm(c, groups, dev, 2)
    t = raw.float().reshape(n, h * w, groups, c // groups)
    mean = t.mean((1, 3)).contiguous()
    rstd = (1.0 / torch.sqrt(t.var((1, 3), unbiased=False) + 1e-5)).contiguous()
    p = ops_f16.Pending(raw, mean, rstd, front.gamma, front.beta, groups, act)
    folded = ops_f16.depthwise_norm(p, wgt, behind, "relu", stride)
    mat = ops_f16.depthwise_norm(p.materialise(), wgt, behind, "relu", stride)
    plain = ops_f16.depthwise(p.materialise(), wgt, stride)
    torch.cuda.synchronize()
    assert folded.y.dtype == torch.float16 and torch.isfinite(folded.y.float()).all()
    assert torch.equal(folded.y, mat.y) and torch.equal(folded.mean, mat.mean) and torch.equal(folded.rstd, mat.rstd)
    assert torch.equal(plain, mat.y)
    assert folded.groups == mat.groups and folded.act == "relu"


def test_zero_padding_after_the_activation_at_the_borders(dev):
    """beta != 0: a fold that padded the RAW tensor would feed act(beta - mean sc) into the border taps.  The kernel's borders match
    the reference (test_case_against_fp64) and differ from that wrong tensor, everywhere along the four edges."""
    import ops_f16
    case = R.CASES["c24-5x7"]
    x, w, gn = R.make_case(case)
    y, _, _, _ = run_case(case, dev)
    wrong_in = np.zeros((case.n, case.h + 2, case.w + 2, case.c), np.float16)
    wrong_in[:, 1:-1, 1:-1] = x
    mean, rstd, gamma, beta = [torch.from_numpy(t).to(dev) for t in gn]
    a = ops_f16.Pending(torch.from_numpy(wrong_in).to(dev), mean, rstd, gamma, beta, case.groups, case.act).materialise()   # the activation applied to the padding too
    full = ops_f16.depthwise(a, torch.from_numpy(w).to(dev).reshape(3, 3, case.c, 1), 1)
    wrong = full[:, 1:-1, 1:-1].float().cpu().numpy()                                  # = a VALID conv of the padded-first operand
    d = y.astype(np.float32) != wrong
    assert d[:, 0].mean() > 0.9 and d[:, -1].mean() > 0.9 and d[:, :, 0].mean() > 0.9 and d[:, :, -1].mean() > 0.9
    assert not d[:, 1:-1, 1:-1].any()
