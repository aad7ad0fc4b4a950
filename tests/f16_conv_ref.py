"""Reference and case table for the fp16 inference convolution (csrc/conv_f16.hip; entry points rn_pack_weights_f16,
rn_conv2d_fwd_f16, rn_conv2d_fwd_f16_fold).

Operands: x is fp16, the kernel tensor holds fp32 values already rounded to fp16 (so packing is exact), the bias is fp32; fp16
subnormals are flushed to zero by the generator, so the reference need not model how the matrix core treats them.  The
reference is a plain grouped SAME convolution (oracle/tf_ops_ref.same_pad_1d, explicit zero padding, then
torch.nn.functional.conv2d) of those values in fp64 and again in fp32, and S, the same convolution of |x| with |w| in fp64 (the
scale of the rounding errors of one output).  For an input fold the operand is fp16(act(fma(x, sc, sh))) with
sc = rstd gamma, sh = beta - mean sc formed in fp32 as the kernel forms them, zero at the padding taps AFTER the activation;
the fp32 reference forms the whole operand in fp32, the fp64 one in fp64 and then rounds to fp16.  beta is centred at 0.5, so
a padding tap that sees act(beta) instead of zero shows up.

CASES names one shape per branch of the dispatch (conv_f16_impl, read through the host-only rn_conv2d_f16_plan);
tests/test_f16_conv_cases_cpu.py proves on the CPU that every case takes the branch it was picked for and that the table
reaches every branch, tests/test_gpu_f16_conv_cases.py runs the table against this reference."""
import collections
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tf_ops_ref as T

# the switch the library reads at every call (set per case) ...
SWITCHES = ("RN_CONV_CFG",)
# ... and once per process (tested in fresh child processes; no case of the table sets them)
PROCESS_SWITCHES = ("RN_F16_SG", "RN_F16_PIPE", "RN_F16_NT", "RN_F16_PIPE_MIN_K")
BM = (128, 128, 64, 128, 256, 256)        # rows of the tile shapes 0..5
BN = (128, 64, 64, 32, 128, 256)
IN_GROUPS = 4                             # groups of the GroupNorm folded into the operand load
EPS = 1e-5

Case = collections.namedtuple("Case", "segs cin cout k stride groups bias out_f32 x_ld x_coff cfg fold stats wgt launch seed")


def _case(segs, cin, cout, k=3, stride=1, groups=1, bias=False, out_f32=False, x_ld=0, x_coff=0, cfg=None, fold=None, stats=0,
          wgt="full", launch=True, seed=0):
    """segs: (n, h, w) per segment.  cout: one int, or one per segment (each segment then has a kernel tensor of its own).
    x_ld / x_coff: x is the channel slice [x_coff, x_coff + cin) of a buffer with x_ld channels (0: dense); the rest of the buffer
    holds NaN.  cfg: RN_CONV_CFG for the call (None: the dispatch's own choice).  fold: None, or the activation ('relu', 'elu') of
    a GroupNorm over IN_GROUPS groups folded into the operand load.  stats: 0 none, 1 statistic rows of one segment
    (rn_f16_fold.partial), 2 several segments' rows in one array (seg_chunk_start).  wgt: 'full' -- wgt_bytes is the packed
    buffer's size -- or 'wt' -- it covers Wt only (the buffer itself is always whole).  launch: False for near misses that are
    only planned."""
    segs = tuple(segs)
    couts = tuple(cout) if isinstance(cout, (tuple, list)) else (cout,) * len(segs)
    return Case(segs, cin, couts, k, stride, groups, bias, out_f32, x_ld, x_coff, cfg, fold, stats, wgt, launch, seed)


SMALL = [(2, 13, 11)]            # 286 pixels: two ragged tiles of 256 rows, three of 128, five of 64
WHOLE = [(2, 16, 16)]            # 256 pixels per sample: whole m-tiles of every shape (the folds need them)
LOADS = (("vec4", 12), ("vec8", 24), ("tap", 64))        # cin: % 8 != 0, % 64 != 0, % 64 == 0 (K = 108, 216, 576 = 9 K tiles)
AUTO5 = [(2, 256, 256)]          # 1 x 1, 128 -> 256: 512 tiles of 256 x 256, x exactly 32 MiB

CASES = collections.OrderedDict()
# ---------------------------------------------------------------- implicit GEMM: every tile shape x gather variant, forced.  264
# output channels: two ragged n-tiles of 256 / 128, five of 64, nine of 32.  vec4: staged fp16 epilogue with bias; vec8: fp32 output
# (bias at the odd tiles); tap-uniform: staged, no bias (tile 5: the pipelined loop on 9 K tiles)
for _c in range(6):
    CASES["cfg%d-vec4" % _c] = _case(SMALL, 12, 264, cfg=_c, bias=True)
    CASES["cfg%d-vec8" % _c] = _case(SMALL, 24, 264, cfg=_c, out_f32=True, bias=bool(_c & 1))
    CASES["cfg%d-tap" % _c] = _case(SMALL, 64, 264, cfg=_c)
CASES.update([
    # ---------------------------------------------------------------- epilogues and kernel sizes
    ("scalar16-cfg3", _case(SMALL, 24, 36, cfg=3, bias=True)),                # cout % 8 != 0: two-byte stores; two n-tiles of 32
    ("scalar16-cfg5", _case(SMALL, 24, 36, cfg=5)),
    ("stride2", _case(SMALL, 24, 264, stride=2)),
    ("k1", _case(SMALL, 24, 264, k=1)),                                       # K = 24: one K tile, all tail
    ("stem", _case([(2, 32, 32)], 4, 64, k=7, stride=2, stats=1)),            # 7 x 7 / 2 on the 4-channel image, 16 x 16 outputs per sample
    # ---------------------------------------------------------------- the dispatch's own choice of tile
    ("auto-0", _case([(2, 40, 41)], 8, 1024, k=1)),                           # 208 tiles of 128 x 128: one round; 416 / 832 of the smaller ones
    ("auto-1", _case([(2, 68, 68)], 8, 1024, k=1)),                           # 1168 of 128 x 64: five rounds; 2320 of 64 x 64: ten
    ("auto-2", _case(SMALL, 24, 40)),
    ("auto-3", _case([(2, 96, 97)], 8, 32, k=1)),                             # 146 of 128 x 32: one round; 291 of 64 x 64: two
    ("group-w24", _case([(2, 9, 7)], 48, 48, groups=2)),                      # cout / G <= 32 -> 3
    ("group-w48", _case([(2, 9, 7)], 48, 96, groups=2)),                      # 33 .. 64 -> 2
    ("group-w96", _case([(2, 9, 7)], 144, 192, groups=2)),                    # above 64: the cost model
    ("auto-5", _case(AUTO5, 128, 256, k=1)),                                  # big = 512, K = 128 = min_k, x = 32 MiB: non-temporal loads
    ("auto-5-miss-big", _case([(1, 511, 256)], 128, 256, k=1, launch=False)),       # big = 511
    ("auto-5-miss-k128", _case(AUTO5, 64, 256, k=1, launch=False)),                 # K = 64 < 128
    ("auto-5-miss-k512", _case(AUTO5, 128, 264, k=1, launch=False)),                # cout % 256 != 0: K = 128 < 512
    ("auto-5-miss-vec4", _case(AUTO5, 132, 256, k=1, launch=False)),                # cin % 8 != 0
    # ---------------------------------------------------------------- the K loop at tile 5
    ("pipe2-k1", _case(SMALL, 64, 264, k=1, cfg=5)),                          # 1, 2, 3 K tiles (9: cfg5-tap): the prologue alone, both buffer parities
    ("pipe2-k2", _case(SMALL, 128, 264, k=1, cfg=5)),
    ("pipe2-k3", _case(SMALL, 192, 264, k=1, cfg=5)),
    ("pipe2-one-n-tile", _case(SMALL, 128, 256, k=1, cfg=5)),                 # the operand is read once: what RN_F16_NT=1 switches
    ("pipe2-stats", _case(WHOLE, 64, 264, cfg=5, stats=1)),
    ("pipe1-short", _case(SMALL, 64, 264, cfg=5, wgt="wt")),                  # wgt_bytes does not prove the fragment copy
    ("pipe1-short-stats", _case(WHOLE, 64, 264, cfg=5, stats=1, wgt="wt")),
    ("fin7-plain-short", _case(WHOLE, 128, 264, k=1, cfg=5, fold="relu", stats=1, wgt="wt")),
    ("fin7-pipe-k2", _case(WHOLE, 128, 264, k=1, cfg=5, fold="relu", stats=1)),
    ("fin7-pipe-k5", _case(WHOLE, 320, 264, k=1, cfg=5, fold="relu", stats=1)),
    ("fin7-pipe-2048", _case(WHOLE, 2048, 256, k=1, cfg=5, fold="relu", stats=1)),      # the fold table's limit: 32 K tiles
    ("fin3-elu", _case(WHOLE, 128, 264, k=1, cfg=5, fold="elu", stats=1)),
    ("fin7-3x3", _case(WHOLE, 64, 264, cfg=5, fold="relu", stats=1)),         # padding on all four edges
    ("fin7-3x3-cfg2", _case([(2, 8, 8)], 64, 72, cfg=2, fold="relu", stats=1)),
    ("fin3-3x3-cin96", _case(WHOLE, 96, 72, fold="elu", stats=1)),            # the input fold, not tap-uniform
    # ---------------------------------------------------------------- channel slices
    ("slice-plain", _case(SMALL, 64, 264, x_ld=160, x_coff=32)),
    ("slice-pipe", _case(SMALL, 64, 264, x_ld=160, x_coff=32, cfg=5)),
    # ---------------------------------------------------------------- several segments
    ("multi-plain", _case([(2, 13, 11), (1, 7, 5), (1, 1, 1)], 24, (264, 40, 72))),
    ("multi-stats", _case([(2, 16, 16), (2, 8, 8), (2, 4, 4)], 64, 72, stats=2)),       # the last level's tiles straddle samples
    ("multi-stats-cfg5", _case([(2, 32, 32), (2, 16, 16), (2, 8, 8)], 64, 264, cfg=5, stats=2)),
    ("multi-stats-vec4", _case([(2, 16, 16), (2, 8, 8)], 12, 72, stats=2)),
])
# ---------------------------------------------------------------- the super-group kernel: whole-tile maps with more than one tile
# in both directions, C = 64 (two super-groups), n = 2
SG_MAP = {1: [(2, 32, 48)], 2: [(2, 64, 64)]}
for _s in (1, 2):
    CASES["sg%d-plain" % _s] = _case(SG_MAP[_s], 64, 64, stride=_s, groups=2)
    CASES["sg%d-stats" % _s] = _case(SG_MAP[_s], 64, 64, stride=_s, groups=2, stats=1)
    CASES["sg%d-elu" % _s] = _case(SG_MAP[_s], 64, 64, stride=_s, groups=2, stats=1, fold="elu")
    CASES["sg%d-relu" % _s] = _case(SG_MAP[_s], 64, 64, stride=_s, groups=2, stats=1, fold="relu")
for _g in (4, 8, 16):
    CASES["sg1-cg%d" % _g] = _case(SG_MAP[1], 64, 64, groups=64 // _g, stats=1)
CASES.update([
    ("sg-miss-map", _case([(2, 24, 32)], 64, 64, groups=2)),
    ("sg-miss-bias", _case(SG_MAP[1], 64, 64, groups=2, bias=True)),
    ("sg-miss-f32", _case(SG_MAP[1], 64, 64, groups=2, out_f32=True)),
    ("sg-miss-short", _case(SG_MAP[1], 64, 64, groups=2, wgt="wt")),
    ("sg-miss-slice", _case(SG_MAP[1], 64, 64, groups=2, x_ld=128, x_coff=32)),
])
# calls that are refused: (case, tweak of the fold struct or None, status).  Tweaks: 'no_partial' -- the fold has no statistics
# array; 'empty' -- neither side; 'f32' -- the plan is asked for a fold with fp32 output (no entry point can launch that)
EINVAL, EUNSUPPORTED = -1, -2
REFUSALS = collections.OrderedDict([
    ("cin/G % 4", (_case(WHOLE, 6, 72), None, EUNSUPPORTED)),
    ("grouped segments, different cout", (_case([(2, 16, 16), (2, 8, 8)], 64, (72, 48), groups=2), None, EUNSUPPORTED)),
    ("fold, fp32 output", (_case(WHOLE, 64, 72, out_f32=True, stats=1), "f32", EUNSUPPORTED)),
    ("several segments' statistics, fp32 output", (_case([(2, 16, 16), (2, 8, 8)], 64, 72, out_f32=True, stats=2), "f32", EUNSUPPORTED)),
    ("fold, ragged map", (_case(SMALL, 64, 72, stats=1), None, EUNSUPPORTED)),
    ("fold, cout % 8", (_case(WHOLE, 64, 36, stats=1), None, EUNSUPPORTED)),
    ("fold, bias", (_case(WHOLE, 64, 72, stats=1, bias=True), None, EINVAL)),
    ("several segments' statistics, bias", (_case([(2, 16, 16), (2, 8, 8)], 64, 72, stats=2, bias=True), None, EINVAL)),
    ("input fold, cin % 8", (_case(WHOLE, 12, 72, fold="relu", stats=1), None, EUNSUPPORTED)),
    ("input fold, cin > 2048", (_case(WHOLE, 2112, 72, k=1, fold="relu", stats=1), None, EUNSUPPORTED)),
    ("input fold, channel slice", (_case(WHOLE, 64, 72, fold="relu", stats=1, x_ld=160, x_coff=32), None, EUNSUPPORTED)),
    ("input fold, no partial", (_case(WHOLE, 64, 72, fold="relu", stats=1), "no_partial", EUNSUPPORTED)),
    ("input fold, several segments", (_case([(2, 16, 16), (2, 8, 8)], 64, 72, fold="relu", stats=2), None, EUNSUPPORTED)),
    ("input fold, two segments, one array", (_case([(2, 16, 16), (2, 8, 8)], 64, 72, fold="relu", stats=1), None, EUNSUPPORTED)),
    ("empty fold", (_case(WHOLE, 64, 72, stats=1), "empty", EINVAL)),
    ("super-group, input fold without partial", (_case(SG_MAP[1], 64, 64, groups=2, fold="elu", stats=1), "no_partial", EINVAL)),
])


def out_hw(case, h, w):
    return T.same_pad_1d(h, case.k, case.stride)[0], T.same_pad_1d(w, case.k, case.stride)[0]


def k_products(case):
    """products per output"""
    return case.k * case.k * case.cin // case.groups


def math_key(case):
    """Cases with equal keys share data and reference."""
    return (case.segs, case.cin, case.cout, case.k, case.stride, case.groups, case.bias, case.fold, case.seed)


def flush16(a):
    """fp32 array -> the nearest fp16 values, subnormals flushed to zero"""
    h = np.asarray(a, np.float32).astype(np.float16)
    h[np.abs(h) < np.float16(2.0 ** -14)] = 0
    return h


@functools.lru_cache(maxsize=3)
def _make(key):
    segs, cin, couts, k, stride, groups, bias, fold, seed = key
    rng = np.random.default_rng(1000 + seed)
    cin_g = cin // groups
    xs, ws, bs, gns = [], [], [], []
    for (n, h, w), cout in zip(segs, couts):
        x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
        if fold:
            x = 2.0 * x + 0.3           # the raw output of a conv in front of its GroupNorm
        xs.append(flush16(x))
        ws.append(flush16(rng.standard_normal((k, k, cin_g, cout), dtype=np.float32) / np.sqrt(k * k * cin_g)).astype(np.float32))
        bs.append((0.5 * rng.standard_normal(cout)).astype(np.float32) if bias else None)
    if len(set(couts)) == 1:            # the shared heads: one kernel tensor
        ws, bs = [ws[0]] * len(segs), [bs[0]] * len(segs)
    gn = None
    if fold:
        x64 = xs[0].astype(np.float64).reshape(segs[0][0], -1, IN_GROUPS, cin // IN_GROUPS)
        mean = x64.mean((1, 3))
        rstd = 1.0 / np.sqrt(x64.var((1, 3)) + EPS)
        gamma = (1.0 + 0.3 * rng.standard_normal(cin)).astype(np.float32)
        beta = (0.5 + 0.2 * rng.standard_normal(cin)).astype(np.float32)
        gn = (mean.astype(np.float32), rstd.astype(np.float32), gamma, beta)
    return xs, ws, bs, gn


def make_case(case):
    """-> (xs fp16 NHWC, kernels fp32 HWIO [k, k, cin / groups, cout] holding fp16 values, biases fp32 or None -- one per segment --
    and, for a fold, (mean, rstd [n, IN_GROUPS], gamma, beta [cin]) in fp32): numpy arrays.  Treat as read-only (shared)."""
    return _make(math_key(case))


def scale_shift(gn, cin):
    """(sc, sh) [n, cin] in fp32 as the kernels form them: sc = rstd gamma, sh = beta - mean sc; sh both with the product rounded
    on its own and fused into the subtraction (the compiler is free to contract it) -> (sc, sh, sh_fused)"""
    mean, rstd, gamma, beta = gn
    cpg = cin // IN_GROUPS
    m, r = np.repeat(mean, cpg, 1), np.repeat(rstd, cpg, 1)
    sc = (r * gamma[None, :]).astype(np.float32)
    sh = (beta[None, :] - (m * sc).astype(np.float32)).astype(np.float32)
    sh_fused = (beta[None, :].astype(np.float64) - m.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    return sc, sh, sh_fused


def _act(z, kind):
    if kind == "relu":
        return np.maximum(z, 0)
    assert kind == "elu"
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def fold_operand(x, gn, kind, dtype, fused=False):
    """fp16(act(fma(x, sc, sh))) of x [n, h, w, cin] (fp16): dtype fp32 -- the fma rounded to fp32, the activation in fp32 -- or
    fp64 -- everything in fp64 -- then one rounding to fp16."""
    sc, sh, sh_fused = scale_shift(gn, x.shape[3])
    sh = sh_fused if fused else sh
    z = x.astype(np.float64) * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]   # (the product is exact in fp64)
    if dtype == np.float32:
        z = z.astype(np.float32)
    return _act(z, kind).astype(dtype).astype(np.float16)


def conv_same(x, w, stride, groups=1, bias=None):
    """NHWC x, [kh, kw, cin / groups, cout] w (torch tensors of one dtype) -> NHWC y"""
    _, pt, pb = T.same_pad_1d(x.shape[1], w.shape[0], stride)
    _, pl, pr = T.same_pad_1d(x.shape[2], w.shape[1], stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), bias=bias, stride=stride, groups=groups).permute(0, 2, 3, 1).contiguous()


def fp16_ulp(v):
    """the spacing of fp16 at |v| (subnormal spacing 2^-24 below 2^-14)"""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)


Ref = collections.namedtuple("Ref", "y64 y32 S slack")


def run_ref(case):
    """-> one Ref per segment: y64 / y32 the convolution in fp64 / in fp32 (fp32: [n, oh, ow, cout] of that dtype, not yet rounded
    to the output type), S = conv(|operand|, |w|) in fp64, slack: for an input fold, conv(u, |w|) with u one fp16 spacing of every
    operand element whose fp32-formed (either way of forming sh) and fp64-formed values differ, else 0."""
    return _run_ref(math_key(case))


@functools.lru_cache(maxsize=3)
def _run_ref(key):
    segs, cin, couts, k, stride, groups, bias, fold, seed = key
    xs, ws, bs, gn = _make(key)
    out = []
    for x, w, b in zip(xs, ws, bs):
        slack = 0.0
        w64 = torch.from_numpy(w).double()
        if fold:
            o64, o32, o32f = fold_operand(x, gn, fold, np.float64), fold_operand(x, gn, fold, np.float32), fold_operand(x, gn, fold, np.float32, True)
            differ = (o64 != o32) | (o64 != o32f)
            u = np.where(differ, np.maximum(fp16_ulp(o64), fp16_ulp(o32)), 0.0)
            slack = conv_same(torch.from_numpy(u), w64.abs(), stride, groups).numpy()
            x64, x32 = torch.from_numpy(o64.astype(np.float64)), torch.from_numpy(o32.astype(np.float32))
        else:
            x64, x32 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(x.astype(np.float32))
        y64 = conv_same(x64, w64, stride, groups, torch.from_numpy(b).double() if b is not None else None).numpy()
        y32 = conv_same(x32, torch.from_numpy(w), stride, groups, torch.from_numpy(b) if b is not None else None).numpy()
        S = conv_same(x64.abs(), w64.abs(), stride, groups).numpy()
        out.append(Ref(y64, y32, S, slack))
    return out


def element_bound(case, ref, bias):
    """|got - y64| <= K 2^-23 S + 2^-23 (S + |bias|) + 1/2 ulp_out(|y64| + that) (+ the fold's slack): products of fp16 values are
    exact in fp32, each of at most K accumulations is allowed one fp32 spacing of a partial sum no larger than S, the bias addition
    one of the result; the last term is half a spacing of the output type and absent for fp32 output."""
    ab = np.abs(bias.astype(np.float64)) if bias is not None else 0.0
    acc = k_products(case) * 2.0 ** -23 * ref.S + 2.0 ** -23 * (ref.S + ab) + ref.slack
    if case.out_f32:
        return acc
    return acc + 0.5 * fp16_ulp(np.abs(ref.y64) + acc)


def stat_rows(y, bm):
    """y [n, oh, ow, c] (the kernel's stored output) -> fp64 (sum y, sum y^2, sum |y|) [n * oh ow / bm, c] over each m-tile"""
    y = np.asarray(y, np.float64)
    t = y.reshape(-1, bm, y.shape[3])
    return t.sum(1), (t * t).sum(1), np.abs(t).sum(1)


# --------------------------------------------------------------------------------------------------------- the plan query
def configure(case, monkeypatch):
    """The per-call switch of the case; the once-per-process switches must not be set."""
    import os
    for name in PROCESS_SWITCHES:
        assert name not in os.environ, "%s is set: the table's rows hold for the defaults" % name
    if case.cfg is None:
        monkeypatch.delenv("RN_CONV_CFG", raising=False)
    else:
        monkeypatch.setenv("RN_CONV_CFG", str(case.cfg))


_HOST_WORD = C.c_uint64(0)   # something non-NULL for the pointers the query only compares with NULL
FAKE = C.addressof(_HOST_WORD)


def wgt_bytes(case, cout):
    """-> (bytes of the packed buffer, bytes the segment reports in wgt_bytes)"""
    import _rn
    cin_g = case.cin // case.groups
    full = int(_rn.lib().rn_pack_weights_f16_bytes(case.k, case.k, cin_g, cout))
    return full, (full if case.wgt == "full" else case.k * case.k * cin_g * cout * 2)


class HostCall(object):
    """The ctypes arguments of the case: segs, nseg, geom, fold (None for rn_conv2d_fwd_f16) and the arrays they point at.  Every data
    pointer the entry points compare with NULL points at a host word (the query follows none of them); the GPU test overwrites them."""

    def __init__(self, case, tiles=None, tweak=None):
        import _rn
        self.case, self.nseg = case, len(case.segs)
        self.segs = (_rn.ConvSeg * self.nseg)()
        for s, (n, h, w), cout in zip(self.segs, case.segs, case.cout):
            s.n, s.h, s.w, s.cout, s.x_ld, s.x_coff = n, h, w, cout, case.x_ld, case.x_coff
            s.x = s.wgt = s.y = FAKE
            s.bias = FAKE if case.bias else None
            s.wgt_bytes = wgt_bytes(case, cout)[1]
        self.geom = _rn.ConvGeom(case.k, case.k, case.stride, case.cin, case.groups)
        self.fold = None
        if case.fold or case.stats:
            f = self.fold = _rn.F16Fold()
            f.partial = FAKE
            if case.fold:
                f.in_mean = f.in_rstd = f.in_gamma = f.in_beta = FAKE
                f.in_groups, f.in_act = IN_GROUPS, _rn.ACT[case.fold]
            if case.stats == 2:
                # rows of the segments one behind the other, by the tiles per sample the plain call's plan reports
                tiles = tiles if tiles is not None else self.query_plain().tiles_per_sample
                self.starts = (C.c_int32 * self.nseg)()
                total = 0
                for i, (n, _, _) in enumerate(case.segs):
                    self.starts[i] = total
                    total += n * tiles[i]
                f.seg_chunk_start, f.total_chunks = C.cast(self.starts, C.c_void_p), total
            if tweak in ("no_partial", "empty"):
                f.partial = None
            if tweak == "empty":
                f.in_mean = None

    def fold_ref(self):
        return C.byref(self.fold) if self.fold is not None else None

    def query_plain(self):
        import _rn
        plan = _rn.F16Plan()
        _rn.check(_rn.lib().rn_conv2d_f16_plan(self.segs, self.nseg, C.byref(self.geom), 0, None, C.byref(plan)), "rn_conv2d_f16_plan")
        return plan

    def query(self, status=0):
        import _rn
        plan = _rn.F16Plan()
        e = _rn.lib().rn_conv2d_f16_plan(self.segs, self.nseg, C.byref(self.geom), 1 if self.case.out_f32 else 0, self.fold_ref(), C.byref(plan))
        assert e == status, "rn_conv2d_f16_plan returned %d, not %d: %s" % (e, status, _rn.lib().rn_last_error().decode())
        return plan


def row_of(plan, nseg):
    """The plan in EXPECT's form.
      implicit GEMM: ('igemm', tile 0..5, gather 4 | 8, tap-uniform, F, pipe, epilogue, a_nt, frag_copy, blocks, K tiles,
                      rows per sample, (tiles per sample of every segment))
      super-group:   ('sg', stride, FIN, statistics, blocks, rows per sample)"""
    import _rn
    kernel = _rn.F16_KERNELS[plan.kernel]
    if kernel == "sg":
        return (kernel, plan.cfg, plan.fold, plan.stats, plan.blocks, plan.rows_per_sample)
    assert plan.stats == (1 if plan.fold & 2 else 0)
    return (kernel, plan.cfg, plan.vec, plan.tap_uniform, plan.fold, plan.pipe, _rn.F16_EPILOGUES[plan.epilogue], plan.a_nt, plan.frag_copy,
            plan.blocks, plan.k_tiles, plan.rows_per_sample, tuple(plan.tiles_per_sample[:nseg]))


def plan_row(case):
    call = HostCall(case)
    return row_of(call.query(), call.nseg)


FP32_OUT, FP16_OUT, FP16_FOLD = "fp32-out", "fp16-out", "fp16-fold"


def family(case):
    """The arithmetic family of a call: fp32 output (the accumulator as it is), fp16 output (one more rounding), fp16 output with an
    input fold (the operand itself is formed in fp32 and rounded to fp16 by the kernel)."""
    return FP32_OUT if case.out_f32 else (FP16_FOLD if case.fold else FP16_OUT)
