"""References, case tables and bounds for the fp16 inference DenseNet kernels (csrc/dense_f16.hip: rn_avgpool_gn_fwd_f16,
rn_dense_f16_put / _finalize / _norm / _plan / _rows; host side ops_f16.avg_pool / avg_pool_norm / DenseBuffer / dense_block), and
the yardstick of the whole-net test: the fp16-STORAGE MODEL of the DenseNet-121-FPN RetinaNet.

    python tests/dense_f16_ref.py       prints the model's figures (CPU, a few minutes); they are quoted in tests/test_gpu_dense_f16.py

Every bound below is derived from the arithmetic; no measured figure enters one.  u = 2^-24 is the unit roundoff of fp32.

AVERAGE POOL (pool_bound).  One output is the fp32 sum of cnt <= 4 fp16 values (cnt = 1, 2 or 4 in-bounds cells of a 2 x 2 / 2
SAME window: the padding is at the bottom / right only) times 1 / cnt, which is exact for these counts, rounded once to fp16.
The three additions and the multiplication are each granted a WHOLE fp32 spacing 2^-23 of A / cnt, A = sum |tap| (any order):

    |got - avg64| <= acc + 1/2 ulp16(|avg64| + acc),      acc = 4 2^-23 A / cnt + slack

With the GroupNorm folded in, a tap is a = fp16(act(fma(x, sc, sh))) formed in fp32 by the kernel and in fp64 by the reference;
where the two can round to different fp16 numbers the element is granted one fp16 spacing (dw_f16_ref's rule and code:
fold_operand_g over every fp32 formation the device can give, the ELU's hardware exponential included), weighted 1 / cnt like
the tap itself: slack = avgpool(spacing where the formations differ).  The folded kernel rounds every tap to fp16 exactly as
rn_group_norm_apply_f16 stores it and sums in the plain pool's order, so it is ALSO bit-equal to apply + plain pool (the GPU test
asserts that); the bound is the independent check against fp64.

STATISTICS (stat_bounds).  A table entry is the fp32 sum of the P <= CHUNK = 256 fp16 values (or their squares) of one channel over
one pixel chunk, in a fixed order.  Any summation order of P terms satisfies |fl(sum) - sum| <= g sum|t|, g = (P - 1) u / (1 -
(P - 1) u).  The squares are exact in fp32 (an 11-bit significand squared has 22 bits; the smallest nonzero fp16 squared is 2^-48),
and fma(f, f, s) rounds once, so the same g holds for them.  rn_dense_f16_finalize adds the rows x channels-of-the-group entries
in fp64 (error below 2^-40 relative to sum|t| for any group of this file: granted) and forms, with M = hw x channels per group,

    mean^ = S1^ / M                  |mean^ - mean| <= dm = (g + 2^-40) A1 / M            A1 = sum |x|
    var^  = S2^ / M - mean^2         |var^  - var | <= dv = (g + 2^-40) E2 + 2 |mean| dm + dm^2     E2 = sum x^2 / M
    rstd^ = (var^ + eps)^-1/2        rstd^ in [ (var + dv + eps)^-1/2, (max(var - dv, 0) + eps)^-1/2 ]

each then rounded to fp32 (a further u relative).  eps is the fp32 number nearest 1e-5, as the kernel receives it.

NORM (norm_bound).  The kernel forms sc = fl(rstd^ gamma), sh = fl(beta - mean^ sc), z = fma(x, sc, sh), a = act(z) in fp32 and rounds
a to fp16; the reference is act((x - mean) rstd gamma + beta) in fp64 with the EXACT statistics.  With dm, dr the statistics bounds
above (rounding to fp32 included):

    |z^ - z| <= |x gamma| dr + |gamma| (|mean| dr + rstd dm + dm dr)  +  4 2^-23 (|x sc| + |mean sc| + |beta|)
    |a^ - a| <= |z^ - z| + ELU_ABS (elu only: rn::act_fwd's exp(z) - 1 against expm1, csrc/rn_common.h) + 2^-23 |a|
    |got - a| <= |a^ - a| + 1/2 ulp16(|a| + |a^ - a|)

(the second term of the first line grants every one of the four fp32 roundings -- sc, the product in sh, sh, the fma -- a whole
spacing of the largest magnitude involved; ELU and ReLU are 1-Lipschitz).

BLOCK TABLES (growth k = 32 throughout; the GPU test fills a sentinel buffer slice by slice and checks every prefix):
    t16x16   2,16,16,64,4    group sizes 2 - 5, whole m-tiles
    t19x25   2,19,25,64,3    475 pixels: the 1 x 1 conv cannot fold, a ragged last chunk
    t8x8     1,8,8,992,2     prefixes 992 / 1024 (group sizes 31 / 32), the block ends at 1056 channels
    t5x7     3,5,7,128,2     fewer pixels than one chunk, n = 3
    t23x25   1,23,25,64,2    575 pixels = 256 + 256 + 63: three rows per sample, the last one ragged (proved from the plan on the CPU)"""
import collections
import ctypes as C
import functools
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "retinanet-tensorflow_amd"), os.path.join(_ROOT, "tests")):      # (run as a script: see below)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dw_f16_ref import ELU_ABS, fold_operand_g
from f16_conv_ref import flush16, fp16_ulp
from mb_f16_ref import output_errors, rel_l2  # noqa: F401  (the whole-net tests use the MobileNetV2 file's error measure)

EPS = float(np.float32(1e-5))
EINVAL, EUNSUPPORTED = -1, -2
U = 2.0 ** -24
GROWTH = 32
GROUPS = 32

# ------------------------------------------------------------------------------------------------------------- average pool
# (n, h, w, c, groups of the folded GroupNorm)
POOL_SHAPES = collections.OrderedDict([
    ("2x16x16x64", (2, 16, 16, 64, 32)),
    ("1x5x7x32", (1, 5, 7, 32, 32)),
    ("3x19x25x8", (3, 19, 25, 8, 8)),
    ("1x1x1x64", (1, 1, 1, 64, 32)),
    ("1x2x3x40", (1, 2, 3, 40, 8)),
    ("2x6x6x96", (2, 6, 6, 96, 32)),          # 32 groups of 3: an octet straddles groups
])
POOL_MODES = ("plain", "gn-none", "gn-elu")


@functools.lru_cache(maxsize=None)
def pool_case(name):
    """-> x fp16 [n, h, w, c], gn = (mean, rstd [n, groups], gamma, beta [c]) fp32.  Read-only (shared)."""
    n, h, w, c, groups = POOL_SHAPES[name]
    rng = np.random.default_rng(7000 + 13 * c + h)
    x = flush16(2.0 * rng.standard_normal((n, h, w, c), dtype=np.float32) + 0.3)
    x64 = x.astype(np.float64).reshape(n, -1, groups, c // groups)
    mean, rstd = x64.mean((1, 3)), 1.0 / np.sqrt(x64.var((1, 3)) + EPS)
    gamma = (1.0 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    beta = (0.5 + 0.2 * rng.standard_normal(c)).astype(np.float32)
    return x, (mean.astype(np.float32), rstd.astype(np.float32), gamma, beta)


def avg_pool_np(a):
    """2 x 2 / 2 SAME average pool of a [n, h, w, c] (fp64): the sum over the in-bounds cells divided by their number -> (avg, cnt)"""
    a = np.asarray(a, np.float64)
    n, h, w, c = a.shape
    oh, ow = -(-h // 2), -(-w // 2)
    p = np.zeros((n, oh * 2, ow * 2, c))
    p[:, :h, :w] = a
    one = np.zeros((oh * 2, ow * 2))
    one[:h, :w] = 1
    s = p.reshape(n, oh, 2, ow, 2, c).sum((2, 4))
    cnt = one.reshape(oh, 2, ow, 2).sum((1, 3))
    return s / cnt[None, :, :, None], cnt[None, :, :, None]


PoolRef = collections.namedtuple("PoolRef", "a y64 bound")


@functools.lru_cache(maxsize=None)
def pool_ref(name, mode):
    """a: the taps as the reference holds them (fp16); y64 their pool in fp64; bound per output element (module docstring)"""
    x, gn = pool_case(name)
    groups = POOL_SHAPES[name][4]
    a, slack = x, 0.0
    if mode != "plain":
        kind = None if mode == "gn-none" else "elu"
        a = fold_operand_g(x, gn, groups, kind, np.float64)
        differ = np.zeros(a.shape, bool)
        u = np.zeros(a.shape, np.float64)
        for fused in (False, True):
            for shift in ((0.0, -ELU_ABS, ELU_ABS) if kind == "elu" else (0.0,)):
                o = fold_operand_g(x, gn, groups, kind, np.float32, fused, shift)
                differ |= (o != a)
                u = np.maximum(u, fp16_ulp(o))
        u = np.where(differ, np.maximum(u, fp16_ulp(a)), 0.0)
        slack = avg_pool_np(u)[0]
    a64 = a.astype(np.float64)
    y64, cnt = avg_pool_np(a64)
    acc = 4 * 2.0 ** -23 * avg_pool_np(np.abs(a64))[0] + slack
    return PoolRef(a, y64, acc + 0.5 * fp16_ulp(np.abs(y64) + acc))


# ------------------------------------------------------------------------------------------------------------- block tables
Table = collections.namedtuple("Table", "n h w c_in depth")
TABLES = collections.OrderedDict([
    ("t16x16", Table(2, 16, 16, 64, 4)),
    ("t19x25", Table(2, 19, 25, 64, 3)),
    ("t8x8", Table(1, 8, 8, 992, 2)),
    ("t5x7", Table(3, 5, 7, 128, 2)),
    ("t23x25", Table(1, 23, 25, 64, 2)),
])
BLOCK_TABLES = ("t16x16", "t19x25", "t8x8", "t5x7")       # the tables the DenseNet_Block test runs


def table_ld(t):
    return t.c_in + t.depth * GROWTH


def prefixes(t):
    """the channel prefixes a block normalises: c_in, c_in + k, ... and the whole buffer (the transition's)"""
    return [t.c_in + i * GROWTH for i in range(t.depth + 1)]


def plan(op, n, hw, c, ld, coff=0, groups=1, status=0):
    import _rn
    p = _rn.DenseF16Plan()
    e = _rn.lib().rn_dense_f16_plan(_rn.DENSE_F16_OPS[op], n, hw, c, ld, coff, groups, C.byref(p))
    assert e == status, "rn_dense_f16_plan(%s) returned %d, not %d: %s" % (op, e, status, _rn.lib().rn_last_error().decode())
    return p


def plan_row(p):
    return (p.op, p.vec, p.chunk, p.rows, p.octets_per_block, p.lanes, p.grid_x, p.grid_y, p.grid_z, p.threads)


@functools.lru_cache(maxsize=None)
def table_data(name):
    """-> slices: [x fp16 [n, hw, c_in], y_1 .. y_depth fp16 [n, hw, k]], and per prefix (gamma, beta) fp32.  Read-only (shared)."""
    t = TABLES[name]
    rng = np.random.default_rng(9000 + t.h * 31 + t.c_in)
    hw = t.h * t.w
    slices = [flush16(1.5 * rng.standard_normal((t.n, hw, t.c_in), dtype=np.float32) + 0.4)]
    for i in range(t.depth):
        slices.append(flush16((0.5 + i) * rng.standard_normal((t.n, hw, GROWTH), dtype=np.float32) - 0.2 * i))
    params = []
    for c in prefixes(t):
        params.append(((1.0 + 0.3 * rng.standard_normal(c)).astype(np.float32), (0.3 + 0.2 * rng.standard_normal(c)).astype(np.float32)))
    return slices, params


Stats = collections.namedtuple("Stats", "mean rstd dm dr")


def stat_bounds(prefix, groups, chunk):
    """prefix: the stored values [n, hw, c] (fp16) -> fp64 mean / rstd [n, groups] and the bounds dm / dr on what
    rn_dense_f16_finalize returns (module docstring); chunk: the plan's pixels per statistic row"""
    x = prefix.astype(np.float64)
    n, hw, c = x.shape
    xg = x.reshape(n, hw, groups, c // groups)
    m = float(hw * (c // groups))
    mean = xg.mean((1, 3))
    e2 = (xg * xg).mean((1, 3))
    var = np.maximum(e2 - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + EPS)
    p = min(chunk, hw)
    g = (p - 1) * U / (1.0 - (p - 1) * U) + 2.0 ** -40
    dm = g * np.abs(xg).sum((1, 3)) / m
    dv = g * e2 + 2.0 * np.abs(mean) * dm + dm * dm
    lo, hi = 1.0 / np.sqrt(var + dv + EPS), 1.0 / np.sqrt(np.maximum(var - dv, 0.0) + EPS)
    dr = np.maximum(rstd - lo, hi - rstd)
    return Stats(mean, rstd, dm + U * (np.abs(mean) + dm), dr + U * (rstd + dr))


def act64(z, kind):
    if kind is None:
        return z
    if kind == "relu":
        return np.maximum(z, 0.0)
    assert kind == "elu"
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def norm_ref(prefix, st, gamma, beta, groups, kind):
    """-> (a64, bound) [n, hw, c]: act(GN(prefix)) in fp64 with the exact statistics `st`, and the element bound on
    rn_dense_f16_norm's fp16 output computed from rn_dense_f16_finalize's statistics (module docstring)"""
    x = prefix.astype(np.float64)
    c = x.shape[2]
    cpg = c // groups
    mean, rstd = np.repeat(st.mean, cpg, 1)[:, None, :], np.repeat(st.rstd, cpg, 1)[:, None, :]
    dm, dr = np.repeat(st.dm, cpg, 1)[:, None, :], np.repeat(st.dr, cpg, 1)[:, None, :]
    ga, be = gamma.astype(np.float64)[None, None, :], beta.astype(np.float64)[None, None, :]
    sc = rstd * ga
    z = (x - mean) * sc + be
    a = act64(z, kind)
    dz = np.abs(x * ga) * dr + np.abs(ga) * (np.abs(mean) * dr + rstd * dm + dm * dr)
    dz = dz + 4 * 2.0 ** -23 * (np.abs(x * sc) + np.abs(mean * sc) + np.abs(be))
    da = dz + (ELU_ABS if kind == "elu" else 0.0) + 2.0 ** -23 * np.abs(a)
    return a, da + 0.5 * fp16_ulp(np.abs(a) + da)


def row_sums(sl, chunk):
    """a stored slice [n, hw, c] -> fp64 (sum x, sum x^2, sum |x|) [n, rows, c] over the chunks of `chunk` pixels"""
    x = sl.astype(np.float64)
    n, hw, c = x.shape
    rows = -(-hw // chunk)
    p = np.zeros((n, rows * chunk, c))
    p[:, :hw] = x
    p = p.reshape(n, rows, chunk, c)
    return p.sum(2), (p * p).sum(2), np.abs(p).sum(2)


# ------------------------------------------------------------------------------------------------------------- whole net
NUM_CLASSES = 80
IMAGE_SHAPE = (2, 256, 256, 3)
LEVELS = ("P3", "P4", "P5", "P6", "P7")


def build_net(backbone='densenet_121'):
    """the product net with the test's seeds, gamma / beta perturbed as tests/mb_f16_ref.py does"""
    import layers, levels, retinanet
    torch.manual_seed(5)
    net = retinanet.RetinaNet(backbone, levels.build_levels(), NUM_CLASSES, layers.elu, 0.0)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("gamma"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("beta"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return net


def image():
    return torch.randn(IMAGE_SHAPE, generator=torch.Generator().manual_seed(7))


def _oracle_forward(net, x, dropout):
    from helpers import to_oracle_name
    from oracle import backbones_ref, model_ref
    params = {to_oracle_name(k): v.detach().double() for k, v in net.named_parameters()}
    bparams = {k[len("base."):]: v.detach().double() for k, v in net.named_parameters() if k.startswith("base.backbone")}
    feats = backbones_ref.backbone_forward('densenet_121', bparams, x, "elu", dropout=dropout)
    pyr = model_ref.fpn_forward(params, feats, "elu")
    cls = {k: model_ref.subnet_forward(params, v, "classification_subnet", 9, NUM_CLASSES, "elu") for k, v in pyr.items()}
    reg = {k: model_ref.subnet_forward(params, v, "regression_subnet", 9, 4, "elu") for k, v in pyr.items()}
    return feats, {"classifications": cls, "regressions": reg}


def model_figures():
    """the fp16-storage model: oracle.backbones_ref + model_ref in fp64, plain, against the same with the backbone's
    `dropout(site, x)` hook (behind every 1 x 1, 3 x 3 and transition conv) rounding the hooked activation to fp16 -> relative
    L2 per output (C3 - C5, P3 - P7)"""
    net = build_net()
    x = image().double()

    def store_f16(site, t):
        return t.half().double()

    with torch.no_grad():
        feats64, out64 = _oracle_forward(net, x, None)
        feats16, out16 = _oracle_forward(net, x, store_f16)
    return output_errors(feats16, out16, feats64, out64)


if __name__ == "__main__":
    for k, v in model_figures().items():
        print("DENSE_F16_MODEL %-3s rel L2 %.3e" % (k, v))
