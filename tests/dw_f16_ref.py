"""Reference and case table for the fp16 inference depthwise 3 x 3 (csrc/depthwise_f16.hip; entry points rn_depthwise_fwd_f16,
rn_depthwise_f16_rows, rn_depthwise_f16_plan; host side ops_f16.depthwise / depthwise_norm).

Operands: x is fp16 (subnormals flushed by the generator), the kernel tensor is fp32 [3, 3, c] as the parameter is stored -- NOT
rounded to fp16: the kernel multiplies fp16 activations with fp32 weights in fp32.  With an input side the operand is
a = fp16(act(fma(x, sc, sh))), sc = rstd gamma, sh = beta - mean sc formed in fp32 as the kernel forms them, zero at the padding
taps AFTER the activation; beta is centred at 0.5, so a padding tap that sees act(beta) instead of zero shows up at the borders.
The reference is the SAME-padded depthwise convolution (f16_conv_ref.conv_same with groups = c: oracle.tf_ops_ref.same_pad_1d,
explicit zero padding, torch conv2d) of a, formed in fp64 and rounded once to fp16, with the fp32 kernel, in fp64.

The element bound (element_bound), derived, not tuned:

    |got - y64| <= 18 2^-23 S + slack + 1/2 ulp16(|y64| + 18 2^-23 S + slack),        S = dwconv(|a|, |w|) in fp64

  * one output is nine products a w and nine additions in fp32.  The product of an fp16 and an fp32 value does not fit fp32, so
    each product is rounded: at most half an fp32 spacing of a value <= |a w| <= S, i.e. <= 2^-24 S; each addition is rounded at
    a partial sum whose magnitude is <= S.  Granting every one of the 18 operations a WHOLE fp32 spacing 2^-23 of S covers any
    evaluation order and the fused multiply-add the kernel actually uses (which rounds nine times, not eighteen);
  * slack is f16_conv_ref's rule: the kernel forms the folded operand in fp32 and rounds it to fp16, the reference forms it in
    fp64; where the fp32-formed and the fp64-formed value round to different fp16 numbers the kernel may hold either, so that
    element is granted one fp16 spacing, weighted with |w| like every other operand error: slack = dwconv(u, |w|).  The
    fp32-formed value is every value the device's fp32 formation can give: sh with the product rounded on its own or fused into
    the subtraction, and for ELU -- which rn::act_fwd evaluates as exp(z) - 1 with the hardware exponential, not reproducible
    bit for bit on the host -- the two ends of the interval csrc/rn_common.h documents for it: within ELU_ABS = 7.2e-8 absolute
    of expm1(z) (measured against fp64 over |z| <= 100 by tests/test_gpu_eltwise_cases.py);
  * the accumulator is stored as fp16: half an fp16 spacing at the largest magnitude the accumulator can have under the terms
    above.
No measured figure enters the bound.

Statistic rows: per (chunk, channel) sums of y and y^2 of the stored fp16 output; a chunk is `strips_per_chunk` consecutive strips
of one sample, a strip `pixels_per_thread` output pixels along w by `rows_per_thread` output rows, numbered along w first
(rn_dw_f16_plan); rows_of() forms the chunks on the host.

CASES names the shapes; tests/test_dw_f16_cases_cpu.py proves from rn_depthwise_f16_plan which kernel variant each takes and that
the table reaches every variant and every chunk situation; tests/test_gpu_dw_f16_cases.py runs it."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from f16_conv_ref import conv_same, flush16, fold_operand, fp16_ulp  # noqa: F401  (fold_operand: checked against fold_operand_g)

EPS = 1e-5
EINVAL, EUNSUPPORTED = -1, -2
ACTS = (None, "relu", "relu6", "elu")
ELU_ABS = 7.2e-8        # |rn::act_fwd's exp(z) - 1  -  expm1(z)| in fp32 (csrc/rn_common.h)

# fold: False -- x is a finished activation; else the activation (None, 'relu', 'relu6', 'elu') of the GroupNorm over `groups` groups
# applied on the operand load.  stats: the statistic rows are asked for.
Case = collections.namedtuple("Case", "n h w c stride fold act groups stats seed")


def _case(n, h, w, c, stride=1, act=False, groups=0, stats=True, seed=0):
    fold = act is not False
    return Case(n, h, w, c, stride, fold, act if fold else None, groups if fold else 0, stats, seed)


CASES = collections.OrderedDict([
    # ---- one output pixel per thread (output rows shorter than 4)
    ("c8-1x1", _case(1, 1, 1, 8, stats=False)),                               # one pixel: every tap but the centre is padding
    ("c8-1x1-fold", _case(3, 1, 1, 8, act="elu", groups=8, stats=False)),     # group size 1
    ("c24-2x3", _case(3, 2, 3, 24, act="relu", groups=8)),                    # group size 3: an octet straddles three groups
    ("c24-2x1-s2", _case(1, 2, 1, 24, 2, act=None, groups=8)),                # -> 1 x 1 at stride 2
    ("c32-5x2-s2", _case(3, 5, 2, 32, 2, stats=False)),                       # -> 3 x 1: no fold, no statistics
    ("c32-5x2-s2-fold", _case(1, 5, 2, 32, 2, act="relu", groups=32, stats=False)),
    ("c96-3x1-s2", _case(1, 3, 1, 96, 2)),                                    # -> 2 x 1: statistics without a fold
    ("c96-3x3", _case(1, 3, 3, 96)),                                          # P = 1, statistics without a fold
    # ---- strips of four (stride 1) / two (stride 2) pixels; one, two or four rows tall
    ("c24-2x3-s2", _case(1, 2, 3, 24, 2, act=None, groups=8)),                # even h, odd w -> 1 x 2
    ("c960-5x7-s2", _case(1, 5, 7, 960, 2, act="relu6", groups=32)),          # odd h, odd w -> 3 x 4
    ("c24-5x7", _case(1, 5, 7, 24, act="elu", groups=8)),                     # ragged strips: 7 = 4 + 3
    ("c32-9x12", _case(3, 9, 12, 32, act="relu6", groups=32)),
    ("c32-9x12-s2", _case(1, 9, 12, 32, 2, stats=False)),                     # odd h, even w; plain depthwise
    ("c96-16x16", _case(1, 16, 16, 96, act="elu", groups=16)),                # group size 6
    ("c96-16x16-s2", _case(3, 16, 16, 96, 2, act="relu", groups=16)),         # even extents: SAME pads bottom / right only
    ("c144-33x17", _case(1, 33, 17, 144, act="relu6", groups=24)),            # 18 octets: 14 pixel lanes, 4 threads idle
    ("c144-33x17-s2", _case(3, 33, 17, 144, 2, act="elu", groups=24)),
    ("c144-33x17-nostats", _case(1, 33, 17, 144, act=None, groups=24, stats=False)),
    ("c960-5x7", _case(1, 5, 7, 960, act=None, groups=32)),                   # group size 30; two pixel lanes
    ("c960-16x16-s2", _case(3, 16, 16, 960, 2, act="relu6", groups=32)),
    ("c96-3x3-s2", _case(1, 3, 3, 96, 2)),                                    # the remaining (fold, statistics) pairs of each kernel
    ("c32-5x6-s2", _case(3, 5, 6, 32, 2, stats=False)),
    ("c32-9x12-plain", _case(1, 9, 12, 32, stats=False)),
    ("c96-16x16-s2-nostats", _case(1, 16, 16, 96, 2, act="elu", groups=16, stats=False)),
    ("c144-33x17-s2-plain", _case(1, 33, 17, 144, 2)),
    ("c8-64x65", _case(1, 64, 65, 8, act="relu", groups=8)),                  # 256 pixel lanes, strips four rows tall, two chunks
    # ---- pixel counts below, at and one strip above a chunk (c = 960: a chunk is the strips of 2 pixel lanes = 8 pixels here)
    ("chunk-below", _case(1, 1, 4, 960)),                                     # 1 strip: the second lane idle
    ("chunk-at", _case(3, 2, 4, 960, act="relu", groups=32)),                 # 2 strips
    ("chunk-above", _case(1, 3, 4, 960)),                                     # 3 strips: a second chunk of one strip
])
# (the grid is n x rows per sample, never capped: there is no second grid pass to reach)

_HOST_WORDS = (C.c_uint64 * 4)()       # 16-byte aligned host words: pointers the plan query compares with NULL and checks for alignment
FAKE = (C.addressof(_HOST_WORDS) + 15) & ~15

# (name, field -> value overrides on the valid call REFUSAL_BASE -- no input side, statistics --, status)
REFUSAL_BASE = _case(2, 9, 12, 96)
REFUSALS = collections.OrderedDict([
    ("null x", (dict(x=None), EINVAL)),
    ("null wgt", (dict(wgt=None), EINVAL)),
    ("null y", (dict(y=None), EINVAL)),
    ("in_* partly: no beta", (dict(in_mean=FAKE, in_rstd=FAKE, in_gamma=FAKE, in_groups=4), EINVAL)),
    ("in_* partly: mean only", (dict(in_mean=FAKE, in_groups=4), EINVAL)),
    ("in_groups without pointers", (dict(in_groups=4), EINVAL)),
    ("in_groups does not divide c", (dict(in_mean=FAKE, in_rstd=FAKE, in_gamma=FAKE, in_beta=FAKE, in_groups=5), EINVAL)),
    ("c % 8", (dict(c=12), EINVAL)),
    ("stride 3", (dict(stride=3), EINVAL)),
    ("stride 0", (dict(stride=0), EINVAL)),
    ("x misaligned", (dict(x=FAKE + 8), EINVAL)),
    ("y misaligned", (dict(y=FAKE + 2), EINVAL)),
    ("wgt misaligned", (dict(wgt=FAKE + 4), EINVAL)),
    ("partial misaligned", (dict(partial=FAKE + 4), EINVAL)),
    ("in_mean misaligned", (dict(in_mean=FAKE + 2, in_rstd=FAKE, in_gamma=FAKE, in_beta=FAKE, in_groups=4), EINVAL)),
    ("k = 5", (dict(k=5), EUNSUPPORTED)),
    ("k = 1", (dict(k=1), EUNSUPPORTED)),
])


def descriptor(case, **over):
    """rn_dw_f16 of the case with fake (aligned, never followed) pointers; `over`: field overrides"""
    import _rn
    d = _rn.DwF16()
    d.x = d.wgt = d.y = FAKE
    d.n, d.h, d.w, d.c, d.k, d.stride = case.n, case.h, case.w, case.c, 3, case.stride
    if case.fold:
        d.in_mean = d.in_rstd = d.in_gamma = d.in_beta = FAKE
        d.in_groups, d.in_act = case.groups, _rn.ACT[case.act]
    if case.stats:
        d.partial = FAKE
    for k, v in over.items():
        setattr(d, k, v)
    return d


def query(d, status=0):
    import _rn
    plan = _rn.DwF16Plan()
    e = _rn.lib().rn_depthwise_f16_plan(C.byref(d), C.byref(plan))
    assert e == status, "rn_depthwise_f16_plan returned %d, not %d: %s" % (e, status, _rn.lib().rn_last_error().decode())
    return plan


def row_of(plan):
    """(kernel 's1' | 's2', pixels per thread, pixel lanes, rows per thread, strips per sample, strips per chunk, rows per sample,
    blocks, input fold, statistics)"""
    import _rn
    return (_rn.DW_F16_KERNELS[plan.kernel], plan.pixels_per_thread, plan.pixel_lanes, plan.rows_per_thread, plan.strips_per_sample,
            plan.strips_per_chunk, plan.rows_per_sample, plan.blocks, plan.fold, plan.stats)


def plan_row(case):
    return row_of(query(descriptor(case)))


# ------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def make_case(case):
    """-> x fp16 [n, h, w, c], w fp32 [3, 3, c], gn = (mean, rstd [n, groups], gamma, beta [c]) fp32 or None.  Read-only (shared)."""
    rng = np.random.default_rng(4000 + case.seed + 7 * case.c + case.h)
    x = rng.standard_normal((case.n, case.h, case.w, case.c), dtype=np.float32)
    if case.fold:
        x = 2.0 * x + 0.3               # the raw output of a conv in front of its GroupNorm
    x = flush16(x)
    w = (rng.standard_normal((3, 3, case.c), dtype=np.float32) / 3.0).astype(np.float32)
    gn = None
    if case.fold:
        x64 = x.astype(np.float64).reshape(case.n, -1, case.groups, case.c // case.groups)
        mean, rstd = x64.mean((1, 3)), 1.0 / np.sqrt(x64.var((1, 3)) + EPS)
        gamma = (1.0 + 0.3 * rng.standard_normal(case.c)).astype(np.float32)
        beta = (0.5 + 0.2 * rng.standard_normal(case.c)).astype(np.float32)
        gn = (mean.astype(np.float32), rstd.astype(np.float32), gamma, beta)
    return x, w, gn


def scale_shift(gn, c, groups):
    """f16_conv_ref.scale_shift for any group count: (sc, sh, sh_fused) [n, c] in fp32 as the kernels form them"""
    mean, rstd, gamma, beta = gn
    cpg = c // groups
    m, r = np.repeat(mean, cpg, 1), np.repeat(rstd, cpg, 1)
    sc = (r * gamma[None, :]).astype(np.float32)
    sh = (beta[None, :] - (m * sc).astype(np.float32)).astype(np.float32)
    sh_fused = (beta[None, :].astype(np.float64) - m.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    return sc, sh, sh_fused


def _act(z, kind, elu_shift=0.0):
    if kind is None:
        return z
    if kind == "relu":
        return np.maximum(z, 0)
    if kind == "relu6":
        return np.minimum(np.maximum(z, 0), 6)
    assert kind == "elu"
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)) + z.dtype.type(elu_shift))


def fold_operand_g(x, gn, groups, kind, dtype, fused=False, elu_shift=0.0):
    """f16_conv_ref.fold_operand for any group count and the four activations: fp16(act(fma(x, sc, sh))) of x [n, h, w, c] (fp16);
    dtype fp32 -- the fma rounded to fp32, the activation in fp32 -- or fp64, then one rounding to fp16.  elu_shift: added to the
    ELU's exponential branch (the ends of the interval the device's exp(z) - 1 lies in, formed in fp64 from the fp32 z)."""
    sc, sh, sh_fused = scale_shift(gn, x.shape[3], groups)
    sh = sh_fused if fused else sh
    z = x.astype(np.float64) * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    if dtype == np.float32:
        z = z.astype(np.float32)
    if elu_shift:
        return _act(z.astype(np.float64), kind, elu_shift).astype(np.float16)
    return _act(z, kind).astype(dtype).astype(np.float16)


def dwconv(a, w, stride):
    """SAME depthwise conv of a [n, h, w, c] with w [3, 3, c] (numpy, fp64) -> [n, oh, ow, c]"""
    c = a.shape[3]
    return conv_same(torch.from_numpy(np.ascontiguousarray(a, np.float64)), torch.from_numpy(np.asarray(w, np.float64)).reshape(3, 3, 1, c),
                     stride, groups=c).numpy()


Ref = collections.namedtuple("Ref", "a y64 S slack")


@functools.lru_cache(maxsize=None)
def run_ref(case):
    """a: the operand as the reference holds it (fp16; x itself without a fold); y64 = dwconv(a, w) in fp64; S = dwconv(|a|, |w|);
    slack (see the module docstring; 0 without a fold)"""
    x, w, gn = make_case(case)
    slack = 0.0
    a = x
    if case.fold:
        a = fold_operand_g(x, gn, case.groups, case.act, np.float64)
        forms = [fold_operand_g(x, gn, case.groups, case.act, np.float32, fused, shift)
                 for fused in (False, True) for shift in ((0.0, -ELU_ABS, ELU_ABS) if case.act == "elu" else (0.0,))]
        differ = np.zeros(a.shape, bool)
        u = np.zeros(a.shape, np.float64)
        for o in forms:
            differ |= (o != a)
            u = np.maximum(u, fp16_ulp(o))
        u = np.where(differ, np.maximum(u, fp16_ulp(a)), 0.0)
        slack = dwconv(u, np.abs(w), case.stride)
    a64 = a.astype(np.float64)
    return Ref(a, dwconv(a64, w, case.stride), dwconv(np.abs(a64), np.abs(w), case.stride), slack)


def element_bound(ref):
    acc = 18 * 2.0 ** -23 * ref.S + ref.slack
    return acc + 0.5 * fp16_ulp(np.abs(ref.y64) + acc)


def rows_of(y, plan):
    """the stored output y [n, oh, ow, c] -> fp64 (sum y, sum y^2, sum |y|, pixels) [n * rows, c] over the kernel's chunks: strip u of a
    sample is the pixels [P (u % spr), + P) of the output rows [R (u // spr), + R) (spr strips side by side), a chunk strips_per_chunk of
    them"""
    y = np.asarray(y, np.float64)
    n, oh, ow, c = y.shape
    P, R, spc, rows = plan.pixels_per_thread, plan.rows_per_thread, plan.strips_per_chunk, plan.rows_per_sample
    spr, sph = -(-ow // P), -(-oh // R)
    assert sph * spr == plan.strips_per_sample and rows == -(-(sph * spr) // spc)
    padded = np.zeros((n, sph * R, spr * P, c))
    padded[:, :oh, :ow] = y
    count = np.zeros((sph * R, spr * P))
    count[:oh, :ow] = 1
    strips = np.zeros((n, rows * spc, R * P, c))
    strips[:, :sph * spr] = padded.reshape(n, sph, R, spr, P, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, sph * spr, R * P, c)
    cnt = np.zeros((rows * spc, R * P))
    cnt[:sph * spr] = count.reshape(sph, R, spr, P).transpose(0, 2, 1, 3).reshape(sph * spr, R * P)
    t = strips.reshape(n * rows, spc * R * P, c)
    pixels = np.tile(cnt.reshape(rows, spc * R * P).sum(1), n)
    return t.sum(1), (t * t).sum(1), np.abs(t).sum(1), pixels
