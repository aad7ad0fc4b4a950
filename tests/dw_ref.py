"""Reference and case table for the depthwise kernels (csrc/depthwise.hip: rn_depthwise_fwd / _fwd_stats / _dgrad / _wgrad / _bwd).

The reference is plain torch on the CPU in a chosen dtype: zero padding by oracle.tf_ops_ref.same_pad_1d, F.conv2d(groups=c),
gradients by autograd for a fixed cotangent.  reference_loops is an independent numpy loop nest (tests/test_dw_cases_cpu.py
checks one against the other on a tiny case).  stat_rows restates what rn_depthwise_fwd_stats writes beside y: per (sample,
pixel chunk, group) the sum and the sum of squares of y over the chunk's pixels, in the rn_gn_rows layout with per_group = 1.

CASES names one shape per branch of the host decision (`decide` in depthwise.hip, read through the host-only
rn_depthwise_plan) and per layout edge; tests/test_dw_cases_cpu.py proves on the CPU that every case takes the branch it was
picked for, tests/test_gpu_dw_cases.py runs the table against this reference in fp64."""
import collections
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tf_ops_ref as T

Case = collections.namedtuple("Case", "n h w c k s groups")
U = 2.0 ** -24          # unit roundoff of fp32


def _case(n, h, w, c, k, s, groups=None):
    """groups: of the GroupNorm behind rn_depthwise_fwd_stats (default: the model's rule, oracle.tf_ops_ref.gn_groups)"""
    return Case(n, h, w, c, k, s, groups or T.gn_groups(c))


CASES = collections.OrderedDict([
    ("k3-s1-odd", _case(2, 17, 15, 32, 3, 1)),           # 3x3 forward, dgrad at a stride other than 2
    ("k3-s2-even", _case(2, 16, 16, 144, 3, 2)),         # pad before = 0
    ("k3-s2-odd", _case(2, 9, 7, 96, 3, 2)),             # pad before = 1; 24 quads divide neither 256 nor 512; ragged grids (12 dgrad blocks, 14 fused)
    ("k3-s3", _case(1, 10, 8, 8, 3, 3)),                 # dgrad 3x3 above stride 2: most taps masked by divisibility
    ("c4-1x1", _case(2, 1, 1, 4, 3, 1)),                 # one quad, one pixel
    ("c4-row", _case(1, 1, 5, 4, 3, 2)),                 # one quad, one row
    ("c1024", _case(1, 5, 6, 1024, 3, 1)),               # one pixel lane in the weight gradient, two in the statistics kernel
    ("k5-s1", _case(2, 9, 7, 8, 5, 1)),                  # generic forward + dgrad
    ("k5-s2", _case(1, 10, 9, 8, 5, 2)),
    ("k1", _case(1, 4, 5, 8, 1, 1)),
    ("k2-s1", _case(1, 5, 4, 8, 2, 1)),                  # even kernel: padding after only
    ("grid-cap", _case(2, 132, 132, 256, 3, 1)),         # 8.9 M elements: above 8192 blocks, weight gradient capped at 4096 chunks
    ("stats-r4-ragged", _case(2, 33, 29, 96, 3, 1)),     # ragged last chunk
    ("stats-r4-s2", _case(2, 16, 16, 144, 3, 2, groups=16)),
    ("stats-r8", _case(1, 96, 96, 1024, 3, 1)),
    ("stats-r16", _case(1, 136, 136, 1024, 3, 1)),
])
DEFER_CASE = "k3-s2-odd"      # runs once more with a defer list
LARGE = ("grid-cap", "stats-r8", "stats-r16")


def out_hw(case):
    return T.same_pad_1d(case.h, case.k, case.s)[0], T.same_pad_1d(case.w, case.k, case.s)[0]


def elements(case):
    return case.n * case.h * case.w * case.c


def make_case(case, seed=0):
    """-> (x [n,h,w,c], w [k,k,c], dy [n,oh,ow,c]): fp32 CPU tensors"""
    rng = np.random.default_rng(4000 + seed)
    oh, ow = out_hw(case)
    x = rng.standard_normal((case.n, case.h, case.w, case.c), dtype=np.float32)
    w = rng.standard_normal((case.k, case.k, case.c), dtype=np.float32)
    dy = rng.standard_normal((case.n, oh, ow, case.c), dtype=np.float32)
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(dy)


def reference(x, w, dy, stride, dtype):
    """-> dict(y, dx, dw) of numpy arrays in `dtype`: SAME-padded depthwise conv and its two gradients for the cotangent dy"""
    k, c = w.shape[0], w.shape[2]
    x = x.detach().to(dtype).clone().requires_grad_(True)
    w = w.detach().to(dtype).clone().requires_grad_(True)
    _, pt, pb = T.same_pad_1d(x.shape[1], k, stride)
    _, pl, pr = T.same_pad_1d(x.shape[2], k, stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.permute(2, 0, 1).unsqueeze(1), stride=stride, groups=c).permute(0, 2, 3, 1)
    dx, dw = torch.autograd.grad(y, (x, w), dy.to(dtype))
    return {"y": y.detach().contiguous().numpy(), "dx": dx.contiguous().numpy(), "dw": dw.contiguous().numpy()}


def reference_loops(x, w, dy, stride):
    """The same three tensors from loops over (output pixel, tap) in float64 numpy: no padding, no conv call, no autograd."""
    x, w, dy = (np.asarray(t, dtype=np.float64) for t in (x, w, dy))
    n, h, wd, c = x.shape
    k = w.shape[0]
    oh, pt, _ = T.same_pad_1d(h, k, stride)
    ow, pl, _ = T.same_pad_1d(wd, k, stride)
    y, dx, dw = np.zeros((n, oh, ow, c)), np.zeros_like(x), np.zeros_like(w)
    for i in range(oh):
        for j in range(ow):
            for a in range(k):
                for b in range(k):
                    ih, iw = i * stride + a - pt, j * stride + b - pl
                    if 0 <= ih < h and 0 <= iw < wd:
                        y[:, i, j] += x[:, ih, iw] * w[a, b]
                        dx[:, ih, iw] += dy[:, i, j] * w[a, b]
                        dw[a, b] += (x[:, ih, iw] * dy[:, i, j]).sum(0)
    return {"y": y, "dx": dx, "dw": dw}


def valid_taps(case):
    """-> [h, w] array: the number of (output pixel, tap) pairs that reach each input pixel (products summed into a dx element)"""
    one = torch.ones((1, case.h, case.w, 1), dtype=torch.float64)
    oh, ow = out_hw(case)
    return reference(one, torch.ones((case.k, case.k, 1), dtype=torch.float64), torch.ones((1, oh, ow, 1), dtype=torch.float64),
                     case.s, torch.float64)["dx"][0, :, :, 0]


def bounds(case, x, w, dy):
    """Per-element bounds |got - ref64| <= (T + 1) 2^-24 sum|terms| that hold for any summation order: T = products summed into
    the element (k^2 for y, the valid taps for dx, n oh ow for dw), sum|terms| from the reference run on |x|, |w|, |dy| (in fp32
    and enlarged by 1e-5: a bound need not be exact)."""
    a = reference(x.abs(), w.abs(), dy.abs(), case.s, torch.float32)
    oh, ow = out_hw(case)
    grow = 1.0 + 1e-5
    return {"y": (case.k ** 2 + 1) * U * grow * a["y"].astype(np.float64),
            "dx": (valid_taps(case)[None, :, :, None] + 1) * U * grow * a["dx"].astype(np.float64),
            "dw": (case.n * oh * ow + 1) * U * grow * a["dw"].astype(np.float64)}


def stat_rows(y, groups, ppc, dtype=np.float64):
    """-> [n, ceil(oh ow / ppc), groups, 2] in `dtype`: (sum, sum of squares) of y over each run of ppc pixels and each group"""
    y = np.asarray(y, dtype=dtype)
    n, oh, ow, c = y.shape
    cps = -(-oh * ow // ppc)
    yg = y.reshape(n, oh * ow, groups, c // groups)
    rows = np.zeros((n, cps, groups, 2), dtype=dtype)
    for r in range(cps):
        part = yg[:, r * ppc:(r + 1) * ppc]
        rows[:, r, :, 0] = part.sum((1, 3), dtype=dtype)
        rows[:, r, :, 1] = (part * part).sum((1, 3), dtype=dtype)
    return rows


def stat_bounds(y64, ybound, groups, ppc):
    """The rows' bound: T = chunk pixels x channels per group products / terms over |y| resp. y^2, plus the error the rows
    inherit from the fp32 y they sum (|dy| <= ybound: sum of ybound resp. of 2 |y| ybound + ybound^2)."""
    n, oh, ow, c = y64.shape
    cpg = c // groups
    absrows = stat_rows(np.abs(y64), groups, ppc)
    absrows[..., 1] = stat_rows(y64, groups, ppc)[..., 1]
    inherit = stat_rows(ybound, groups, ppc)
    inherit[..., 1] = stat_rows(np.sqrt(2 * np.abs(y64) * ybound + ybound ** 2), groups, ppc)[..., 1]
    cps = absrows.shape[1]
    pixels = np.minimum(ppc, oh * ow - ppc * np.arange(cps))
    return (pixels * cpg + 1)[None, :, None, None] * U * absrows + inherit


# --------------------------------------------------------------------------------------------------------- the plan query
def query(case, groups=None):
    """-> (status, _rn.DwPlan) of rn_depthwise_plan (host only)"""
    import _rn
    plan = _rn.DwPlan()
    g = case.groups if groups is None else groups
    return _rn.lib().rn_depthwise_plan(case.n, case.h, case.w, case.c, case.k, case.s, g, C.byref(plan)), plan


def row_of(plan):
    """The plan in EXPECT's form: ((forward kernel, blocks), (dgrad variant, blocks), (chunks, pixels per chunk, workspace bytes)
    or None where the weight gradient refuses, the fused backward's blocks, (R, pixels per block, rows per sample, blocks) or None
    where the statistics kernel declines)."""
    import _rn
    return ((_rn.DW_FWDS[plan.fwd_kernel], plan.fwd_blocks), (_rn.DW_DGRADS[plan.dgrad_kernel], plan.dgrad_blocks),
            (plan.wgrad_chunks, plan.wgrad_ppc, plan.wgrad_workspace_bytes) if plan.wgrad_ok else None, plan.bwd_blocks,
            (plan.stats_r, plan.stats_ppc, plan.stats_rows_per_sample, plan.stats_blocks) if plan.stats_r else None)


@functools.lru_cache(maxsize=None)
def small_case_data(name):
    """Inputs, fp64 / fp32 references and bounds of a case below a million elements (shared; treat as read-only)."""
    case = CASES[name]
    assert name not in LARGE
    x, w, dy = make_case(case)
    return (x, w, dy), reference(x, w, dy, case.s, torch.float64), reference(x, w, dy, case.s, torch.float32), bounds(case, x, w, dy)
