"""Reference and case table for the generic convolution (csrc/conv_gemm.hip and the files it routes to: gemm_x3.hip, im2col.hip,
grouped_conv.hip; entry points rn_conv2d_fwd / _fwd_stats / _dgrad / _wgrad / _bwd / _bias_grad, and rn_gemm_batched).

The reference is a plain torch evaluation in a chosen dtype: TF 'SAME' padding by the rn_same_pad rule (explicit asymmetric
zero padding, then torch.nn.functional.conv2d, grouped convs included), the gradients by autograd for fixed cotangents, the
bias gradient, and the GroupNorm statistic rows of the output in the rn_gn_rows layout.  run_ref(case, dtype) gives the fp64
result and its fp32 twin, so that the error of fp32 arithmetic itself (e32) comes from the reference alone.

CASES names one shape per branch of the dispatch (conv_fwd_impl, conv_dgrad_impl, plan_wgrad / conv_wgrad_impl and
rn_conv2d_bwd, read through the host-only rn_conv2d_plan); tests/test_conv_cases_cpu.py proves on the CPU that every case
takes the branch it was picked for and that the table reaches every branch, tests/test_gpu_conv_cases.py runs the table
against this reference in fp64.  Every segment of a case shares one kernel tensor (the shared heads)."""
import collections
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

# switches the library reads at every call (set per case) ...
SWITCHES = ("RN_CONV_CFG", "RN_WGRAD_CFG", "RN_WGRAD_SPLITS", "RN_NO_SPLITK", "RN_NO_PHASE_DGRAD")
# ... and once per process (tested in fresh child processes; no case of the table sets them)
PROCESS_SWITCHES = ("RN_STEM_DIRECT", "RN_X3_CONV1X1", "RN_X3_IM2COL", "RN_GCONV_DIRECT", "RN_NO_MERGED_BWD", "RN_X3_IM2COL_PIECE_MB")
OPS = ("fwd", "fwd_stats", "dgrad", "wgrad", "bwd", "bias_grad")
WG_MAXPIX = 1024      # pixels of the weight-gradient kernel's table: longer splits run in windows

Case = collections.namedtuple("Case", "segs cin cout k stride groups bias x_ld x_coff mode env ws accumulate defer stats ops seed")


def _case(segs, cin, cout, k=3, stride=1, groups=1, bias=False, x_ld=0, x_coff=0, mode=1, env=(), ws="exact", accumulate=False,
          defer=False, stats=0, ops=("fwd", "dgrad", "wgrad"), seed=0):
    """segs: (n, h, w) per segment.  x_ld / x_coff: x and dx are the channel slice [x_coff, x_coff + cin) of buffers with x_ld
    channels (0: dense).  mode: the product mode (1: split-bf16 where the shape allows, 0: fp32 only).  env: the per-call
    switches set for the calls.  ws: the workspace handed to the forward and data-gradient calls -- 'exact' (what
    rn_conv2d_*_workspace returns), 'none' (NULL) or 'short' (one byte less); the weight gradient always gets its exact size
    (it refuses less).  accumulate: dw += ; defer: the weight-gradient reduction waits in a defer list.  stats: GroupNorm groups of
    the fwd_stats op.  ops: the entry points the case drives."""
    return Case(tuple(segs), cin, cout, k, stride, groups, bias, x_ld, x_coff, mode, tuple(env), ws, accumulate, defer, stats, tuple(ops), seed)


def _env(**kw):
    return tuple(sorted(("RN_" + k.upper(), str(v)) for k, v in kw.items()))


ALL = ("fwd", "dgrad", "wgrad")
PYRAMID5 = [(2, 16, 16), (2, 8, 8), (2, 4, 4), (2, 2, 2), (2, 1, 1)]
SMALL = [(2, 13, 11)]            # 286 pixels: three 128-row tiles, the last one ragged
LOADS = {"scalar": (6, 10), "vec4": (12, 20), "tap": (32, 64)}      # (cin, cout): neither % 4 / % 4 / % 32

CASES = collections.OrderedDict()
# ---------------------------------------------------------------- fp32 kernels: every tile shape x load variant, forced
# (the instantiations choose_cfg / cfg_for_group_width / plan_wgrad pick are the same ones; the three that shapes further down
# reach on their own are left to them)
for _c in range(4):
    for _l, (_ci, _co) in LOADS.items():
        if (_c, _l) in ((2, "vec4"), (2, "tap"), (3, "vec4")):
            continue
        CASES["f32-cfg%d-%s" % (_c, _l)] = _case(SMALL, _ci, _co, env=_env(conv_cfg=_c, wgrad_cfg=_c), bias=(_l == "vec4"),
                                                 ops=ALL + (("bias_grad",) if _l != "tap" else ()))
CASES.update([
    # ---------------------------------------------------------------- tile shapes reached by the planner itself
    ("dense-cfg0", _case([(2, 40, 40)], 8, 1024)),                     # 200 tiles of 128 x 128: one round; 800 of 64 x 64: four
    ("dense-cfg1-dgrad-cfg3", _case([(3, 80, 80)], 8, 512)),           # 1200 tiles of 128 x 64; dgrad: 150 of 128 x 32
    ("group-w64", _case([(2, 9, 7)], 64, 128, groups=2)),              # 64 outputs / 32 inputs per group: 64 x 64 / 128 x 32
    ("group-w96", _case([(2, 9, 7)], 144, 192, groups=2)),             # 96 / 72 per group: choose_cfg, two N-tiles per group
    # ---------------------------------------------------------------- split-K
    ("splitk", _case([(2, 4, 4)], 100, 64)),                           # K = 900: 29 K-tiles (K % 32 = 4), ranges of unequal length
    ("splitk-none", _case([(2, 4, 4)], 100, 64, ws="none")),
    ("splitk-short", _case([(2, 4, 4)], 100, 64, ws="short")),
    ("splitk-off", _case([(2, 4, 4)], 100, 64, env=_env(no_splitk=1))),
    ("splitk-80-tiles", _case([(2, 40, 64)], 64, 64, ops=("fwd", "dgrad"))),   # 80 tiles of 64 x 64: the largest grids that still split (< 96)
    ("splitk-s2", _case([(2, 8, 8)], 256, 256, stride=2)),             # the convs that make P6 / P7
    # ---------------------------------------------------------------- several segments
    ("pyramid5", _case(PYRAMID5, 64, 36, bias=True, ops=ALL + ("bias_grad", "bwd"))),
    ("pyramid4-bwd", _case(PYRAMID5[:4], 64, 64, ops=("bwd",))),       # merged, four segments, tap-uniform
    ("pyramid4-bwd-vec", _case(PYRAMID5[:4], 24, 40, ops=("bwd",))),   # merged, not tap-uniform
    # ---------------------------------------------------------------- stem
    ("stem", _case([(2, 16, 64)], 3, 32, stride=2, stats=32, ops=("fwd", "fwd_stats"))),      # 8 x 32 outputs: ow % 32 == 0, 256 pixels = one block per sample
    ("stem-off", _case([(2, 14, 64)], 3, 32, stride=2, ops=("fwd",))),                        # 7 x 32 = 224 outputs: fp32 scalar
    # ---------------------------------------------------------------- split-bf16 1x1
    ("x3-1x1-m128", _case([(2, 80, 64)], 64, 512, k=1, stats=32, ops=ALL + ("fwd_stats",))),            # 80 x 4 = 320 tiles of 128 x 128
    ("x3-1x1-m64", _case([(2, 32, 32)], 64, 192, k=1, stats=32, ops=ALL + ("bwd", "fwd_stats"))),       # 32 x 3 = 96 tiles of 64 x 64
    ("x3-1x1-slice", _case([(2, 32, 32)], 64, 192, k=1, x_ld=160, x_coff=32)),
    ("x3-1x1-mode0", _case([(2, 32, 32)], 64, 192, k=1, mode=0)),
    ("x3-1x1-under", _case([(2, 31, 32)], 64, 192, k=1)),              # 31 x 3 = 93 tiles: the fp32 kernels
    # ---------------------------------------------------------------- patch matrix
    ("patch", _case([(2, 77, 77)], 128, 512, stride=2, stats=32, ops=ALL + ("bwd",))),
    ("patch-none", _case([(2, 77, 77)], 128, 512, stride=2, ws="none", ops=("fwd", "dgrad"))),
    ("patch-stats", _case([(3, 64, 64)], 128, 512, stride=2, stats=32, ops=("fwd_stats",))),            # 1024 outputs per sample: whole m-tiles
    # ---------------------------------------------------------------- direct grouped kernels (h % 8, w % 16 != 0; grid >= 256)
    ("gconv-cg4", _case([(2, 28, 50)], 256, 256, groups=64, ops=ALL + ("bwd",))),             # 2 x 4 x 4 tiles x 8 slabs = 256 blocks
    ("gconv-cg8", _case([(2, 28, 50)], 256, 256, groups=32)),
    ("gconv-cg16", _case([(2, 28, 50)], 256, 256, groups=16)),
    ("gconv-cg32", _case([(2, 28, 50)], 256, 256, groups=8, accumulate=True)),
    ("gconv-under", _case([(2, 20, 50)], 256, 256, groups=32)),                               # 2 x 3 x 4 x 8 = 192: the grouped fp32 kernels
    # ---------------------------------------------------------------- phase-decomposed data gradient (stride 2, >= 4096 input pixels)
    ("phase-3x3-odd", _case([(2, 47, 45)], 16, 24, stride=2, ops=("dgrad", "bwd"))),
    ("phase-3x3-even", _case([(2, 48, 44)], 32, 32, stride=2, ops=("dgrad",))),
    ("phase-1x1", _case([(2, 47, 45)], 16, 24, k=1, stride=2, mode=0, ops=("dgrad",))),
    ("phase-7x7", _case([(2, 47, 45)], 8, 12, k=7, stride=2, ops=("dgrad",))),
    ("phase-h1", _case([(2, 1, 2100)], 16, 24, stride=2, ops=("dgrad",))),
    ("phase-2seg", _case([(2, 47, 45), (1, 10, 9)], 16, 24, stride=2, ops=("dgrad",))),
    ("phase-slice", _case([(2, 47, 45)], 16, 24, stride=2, x_ld=40, x_coff=8, ops=("dgrad",))),
    ("phase-off-3x3", _case([(2, 47, 45)], 16, 24, stride=2, env=_env(no_phase_dgrad=1), ops=("dgrad",))),
    ("phase-off-1x1", _case([(2, 47, 45)], 16, 24, k=1, stride=2, mode=0, env=_env(no_phase_dgrad=1), ops=("dgrad",))),
    ("phase-off-h1", _case([(2, 1, 2100)], 16, 24, stride=2, env=_env(no_phase_dgrad=1), ops=("dgrad",))),
    ("slice-f32", _case([(2, 13, 11)], 12, 20, x_ld=32, x_coff=8)),    # the fp32 kernels on a channel slice
    # ---------------------------------------------------------------- fp32 weight gradient
    ("wg-window-1k", _case([(2, 27, 19)], 16, 24, env=_env(wgrad_splits=1), ops=("wgrad",))),      # 1026 pixels in one split: 2 windows
    ("wg-window-2k", _case([(2, 27, 38)], 16, 24, env=_env(wgrad_splits=1), ops=("wgrad",))),      # 2052: 3 windows
    # unforced: 36 x 11 = 396 output tiles of 128 x 64 want two splits, 2100 pixels make them 1056 long (13.6 GFLOP: the least that gets there)
    ("wg-window-own", _case([(1, 50, 42)], 512, 704, mode=0, ops=("wgrad",))),
    ("wg-acc-1", _case([(2, 9, 7)], 16, 24, env=_env(wgrad_splits=1), accumulate=True, ops=("wgrad",))),
    ("wg-acc-n", _case([(2, 27, 19)], 16, 24, accumulate=True, ops=("wgrad",))),                    # 1026 pixels: no multiple of chunk nor of 32
    ("wg-defer", _case([(2, 27, 19)], 16, 24, defer=True, ops=("wgrad", "bwd", "bias_grad"))),
    # ---------------------------------------------------------------- rn_conv2d_bwd
    ("bwd-merged-tap", _case([(2, 13, 11)], 32, 64, ops=("bwd",))),
    ("bwd-merged-vec", _case([(2, 13, 11)], 12, 20, ops=("bwd",))),
    ("bwd-scalar", _case([(2, 13, 11)], 6, 10, ops=("bwd",))),          # scalar loads: two calls
    # ---------------------------------------------------------------- statistic rows
    ("stats-f32", _case([(2, 16, 16)], 16, 64, stats=32, ops=("fwd_stats",))),
    ("stats-refused-ragged", _case([(2, 13, 11)], 16, 64, stats=32, ops=("fwd_stats",))),           # 143 pixels: no tile height divides them
    ("stats-refused-bias", _case([(2, 16, 16)], 16, 64, bias=True, stats=32, ops=("fwd_stats",))),
    ("stats-refused-splitk", _case([(2, 4, 4)], 128, 64, stats=32, ops=("fwd_stats",))),
])
# cases of single tests, not run as part of the table
EXTRA = {
    "refusals": _case([(2, 9, 7)], 16, 48),
    # RN_X3_IM2COL_PIECE_MB=16 (a fresh process): two pieces of three samples, 3072 rows = 24 x 4 tiles each, 1024 outputs per sample
    "patch-pieces": _case([(6, 64, 64)], 128, 512, stride=2, stats=32, ops=("fwd", "fwd_stats")),
}
# products of rn_gemm_batched: (M, K, N, batches, b_nk, product mode)
GEMMS = collections.OrderedDict([
    ("gemm-kn", (150, 44, 36, 5, 0, 0)),           # K tail: 44 = 32 + 12
    ("gemm-nk", (150, 44, 36, 5, 1, 0)),
    ("gemm-kn-tap", (150, 64, 64, 3, 0, 0)),
    ("gemm-nk-x3", (150, 44, 36, 5, 1, 1)),
])

FP32, FP32_LONG, X3 = "fp32", "fp32-long", "split-bf16"


def out_hw(case, h, w):
    import _rn
    return _rn.same_pad(h, case.k, case.stride)[0], _rn.same_pad(w, case.k, case.stride)[0]


def math_key(case):
    """Cases with equal keys share data and reference."""
    return (case.segs, case.cin, case.cout, case.k, case.stride, case.groups, case.bias, case.seed)


@functools.lru_cache(maxsize=4)
def _make(key):
    segs, cin, cout, k, stride, groups, bias, seed = key
    gen = torch.Generator().manual_seed(100 + seed)
    cin_g = cin // groups
    xs = [torch.randn(n, h, w, cin, generator=gen) for n, h, w in segs]
    wgt = torch.randn(k, k, cin_g, cout, generator=gen) / float(np.sqrt(k * k * cin_g))
    b = 0.1 * torch.randn(cout, generator=gen) if bias else None
    dys = []
    for n, h, w in segs:
        oh, ow = -(-h // stride), -(-w // stride)
        dys.append(torch.randn(n, oh, ow, cout, generator=gen))
    dw0 = torch.randn(k, k, cin_g, cout, generator=gen)
    return xs, wgt, b, dys, dw0


def make_case(case):
    """-> (xs, w [k, k, cin / groups, cout], bias or None, cotangents dy, the old content of dw for accumulate cases): fp32 CPU
    tensors, NHWC / HWIO.  Treat as read-only (shared)."""
    return _make(math_key(case))


def same_pad(n, k, s):
    """rn_same_pad: out = ceil(n / s); before = max((out - 1) s + k - n, 0) // 2 -> (out, before, after)"""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def conv_same(x, w, stride, groups=1, bias=None):
    """NHWC x, [kh, kw, cin / groups, cout] w -> NHWC y, in x's dtype"""
    _, pt, pb = same_pad(x.shape[1], w.shape[0], stride)
    _, pl, pr = same_pad(x.shape[2], w.shape[1], stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), bias=bias, stride=stride, groups=groups).permute(0, 2, 3, 1)


def conv_same_naive(x, w, stride, groups=1, bias=None):
    """The same by a loop over output pixels and taps in numpy fp64 (the check of the reference itself)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, cin = x.shape
    kh, kw, cin_g, cout = w.shape
    cout_g = cout // groups
    oh, pt, _ = same_pad(h, kh, stride)
    ow, pl, _ = same_pad(wd, kw, stride)
    y = np.zeros((n, oh, ow, cout))
    for i in range(oh):
        for j in range(ow):
            for a in range(kh):
                for b in range(kw):
                    ih, iw = i * stride - pt + a, j * stride - pl + b
                    if 0 <= ih < h and 0 <= iw < wd:
                        for g in range(groups):
                            y[:, i, j, g * cout_g:(g + 1) * cout_g] += x[:, ih, iw, g * cin_g:(g + 1) * cin_g] @ w[a, b, :, g * cout_g:(g + 1) * cout_g]
    return y + (np.asarray(bias, np.float64) if bias is not None else 0.0)


def run_ref(case, dtype):
    """-> dict of numpy arrays: y<i>, dx<i> per segment, dw (the gradient alone, summed over the segments), dbias (dy's column
    sums, whether or not the case has a bias)."""
    return _run_ref(math_key(case), dtype)


@functools.lru_cache(maxsize=8)
def _run_ref(key, dtype):
    segs, cin, cout, k, stride, groups, bias, seed = key
    xs, wgt, b, dys, _ = _make(key)
    xs = [x.to(dtype).requires_grad_(True) for x in xs]
    w = wgt.to(dtype).requires_grad_(True)
    bb = b.to(dtype) if b is not None else None
    ys = [conv_same(x, w, stride, groups, bb) for x in xs]
    grads = torch.autograd.grad(ys, xs + [w], [d.to(dtype) for d in dys])
    out = {}
    for i, y in enumerate(ys):
        out["y%d" % i], out["dx%d" % i] = y.detach().numpy(), grads[i].numpy()
    out["dw"] = grads[-1].numpy()
    out["dbias"] = sum(d.to(dtype).reshape(-1, cout).sum(0) for d in dys).numpy()
    return out


def stat_rows(y, rows_per_sample):
    """y [n, oh, ow, c] -> [n * rows_per_sample, c, 2]: per channel (sum, sum of squares) over the output pixels
    [r bm, (r + 1) bm) of a sample, bm = oh ow / rows_per_sample (the rn_gn_rows layout with per_group 0), in y's dtype"""
    y = torch.as_tensor(y)
    n, oh, ow, c = y.shape
    t = y.reshape(n * rows_per_sample, oh * ow // rows_per_sample, c)
    return torch.stack([t.sum(1), (t * t).sum(1)], -1).numpy()


def gemm_data(name):
    m, k, n, nb, b_nk, _ = GEMMS[name]
    gen = torch.Generator().manual_seed(7)
    a = torch.randn(nb, m, k, generator=gen)
    b = torch.randn((nb, n, k) if b_nk else (nb, k, n), generator=gen) / float(np.sqrt(k))
    return a, b


def gemm_ref(name, dtype):
    a, b = gemm_data(name)
    b = b.to(dtype)
    return torch.matmul(a.to(dtype), b.transpose(1, 2) if GEMMS[name][4] else b).numpy()


# --------------------------------------------------------------------------------------------------------- the plan query
def configure(case, monkeypatch):
    """The per-call switches of the case and its product mode; the once-per-process switches must not be set."""
    import _rn
    import os
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in PROCESS_SWITCHES:
        assert name not in os.environ, "%s is set: the table's rows hold for the defaults" % name
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    _rn.lib().rn_set_product_mode(case.mode)


_HOST_WORD = C.c_uint64(0)   # something non-NULL for the pointers the query only compares with NULL
FAKE = C.addressof(_HOST_WORD)


def host_call(case):
    """-> (segs, nseg, geom): the ctypes arguments of the case; every data pointer the entry points compare with NULL points at
    a host word (the query follows none of them)."""
    import _rn
    segs = (_rn.ConvSeg * len(case.segs))()
    for s, (n, h, w) in zip(segs, case.segs):
        s.n, s.h, s.w, s.cout, s.x_ld, s.x_coff = n, h, w, case.cout, case.x_ld, case.x_coff
        s.x = s.wgt = s.y = s.dy = s.dx = FAKE
        s.bias = FAKE if case.bias else None
    return segs, len(case.segs), _rn.ConvGeom(case.k, case.k, case.stride, case.cin, case.groups)


def workspace_need(case, op, segs, nseg, geom):
    """what rn_conv2d_*_workspace returns for the op (rn_conv2d_bwd takes the weight gradient's)"""
    import _rn
    L = _rn.lib()
    if op in ("fwd", "fwd_stats"):
        return L.rn_conv2d_fwd_workspace(segs, nseg, C.byref(geom))
    if op == "dgrad":
        return L.rn_conv2d_dgrad_workspace(segs, nseg, C.byref(geom))
    if op in ("wgrad", "bwd"):
        return L.rn_conv2d_wgrad_workspace(segs, nseg, C.byref(geom))
    return L.rn_conv2d_bias_grad_workspace(case.cout)


def workspace_given(case, op, need):
    """-> (bytes handed to the call, whether the pointer is NULL), by the case's workspace rule"""
    if op in ("fwd", "fwd_stats", "dgrad"):
        if case.ws == "none":
            return 0, True
        if case.ws == "short":
            return max(need - 1, 0), False
    return need, False


def query(case, op, segs, nseg, geom, ws_bytes, ws_ptr=FAKE, dw_ptr=FAKE, status=0):
    import _rn
    plan = _rn.ConvPlan()
    e = _rn.lib().rn_conv2d_plan(segs, nseg, C.byref(geom), _rn.CONV_OPS[op], case.stats, 1 if case.accumulate else 0, 1 if case.defer else 0,
                                 dw_ptr, ws_ptr, ws_bytes, C.byref(plan))
    assert e == status, "rn_conv2d_plan(%s) returned %d, not %d: %s" % (op, e, status, _rn.lib().rn_last_error().decode())
    return plan


def _call_row(c, op):
    import _rn
    path = _rn.CONV_PATHS[c.path]
    if path == "fp32":
        row = (path, c.cfg, _rn.CONV_LOADS[c.load], c.nsplit, c.ksplit, c.blocks)
        if op == "dgrad":
            row += (c.phases, c.phases_no_taps)
        if op == "wgrad":
            row += (c.windows, c.direct, _rn.CONV_REDUCES[c.reduce])
    elif path == "x3_1x1":
        row = (path, c.m_tile) + ((c.nsplit, _rn.CONV_REDUCES[c.reduce]) if op == "wgrad" else ())
    elif path == "x3_patch":
        row = (path, c.m_tile, c.n_piece, c.patch_bytes) + ((c.nsplit, _rn.CONV_REDUCES[c.reduce]) if op == "wgrad" else ())
    elif path == "stem":
        row = (path, c.blocks)
    else:
        row = (path,) + ((_rn.CONV_REDUCES[c.reduce],) if op == "wgrad" and path else ())
    if op == "fwd_stats":
        row += (c.rows_per_sample,)
    return row


def row_of(plan, op):
    """The plan in EXPECT's form.
      fp32:    ('fp32', tile shape, load variant, nsplit, ksplit | chunk, blocks) + (phases, phases without taps) for the data
               gradient, + (windows, straight into dw, the row reduction) for the weight gradient
      x3_1x1:  ('x3_1x1', m-tile rows) + (slabs, the row reduction) for the weight gradient
      x3_patch: ('x3_patch', m-tile rows, samples per piece, patch-matrix bytes) + likewise
      stem:    ('stem', blocks);  direct_grouped: ('direct_grouped',) + (the row reduction,) for the weight gradient
      fwd_stats: the forward row + (rows per sample,)
      bwd:     ('merged_bwd', blocks, dgrad row, wgrad row) or ('two_calls', why, dgrad row, wgrad row)"""
    import _rn
    if op != "bwd":
        return _call_row(plan.call, op)
    head = ("two_calls", _rn.CONV_UNMERGED[plan.unmerged]) if plan.unmerged else ("merged_bwd", plan.call.blocks)
    return head + (_call_row(plan.dgrad, "dgrad"), _call_row(plan.wgrad, "wgrad"))


def gemm_row(name):
    import _rn
    m, k, n, nb, b_nk, mode = GEMMS[name]
    _rn.lib().rn_set_product_mode(mode)
    plan = _rn.ConvPlan()
    _rn.check(_rn.lib().rn_gemm_batched_plan(FAKE, FAKE, FAKE, m, k, n, nb, b_nk, C.byref(plan)), "rn_gemm_batched_plan")
    return _call_row(plan.call, "dgrad" if b_nk else "fwd") + (plan.call.batched,)


def family(row):
    """The arithmetic family of a call, from its plan row: the split-bf16 products; the fp32 kernels (implicit GEMM on the fp32
    matrix cores, stem, direct grouped kernels: fmaf chains); and, apart from those, the fp32 weight gradient whose split runs in
    windows -- one accumulator takes more than 1024 products in a row where every other call's chains are cut by split-K or by
    the 64 .. 1024-pixel splits, so its rounding error is the longest chain's."""
    if row[0].startswith("x3"):
        return X3
    return FP32_LONG if row[0] == "fp32" and len(row) == 9 and row[6] else FP32
