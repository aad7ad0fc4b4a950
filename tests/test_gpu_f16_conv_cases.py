"""rn_pack_weights_f16, rn_conv2d_fwd_f16 and rn_conv2d_fwd_f16_fold at every branch of conv_f16_impl against the fp64
reference of tests/f16_conv_ref.py.

The entry points are driven directly (ctypes structs), so that wgt_bytes, the channel slices and the statistic rows' layout are
in the test's hands.  Every call first asserts, through rn_conv2d_f16_plan with the real pointers, that it runs the branch
tests/test_f16_conv_cases_cpu.py lists for it, and where the plan asks for a pipelined K loop, that
rn_conv2d_f16_pipe_available() is 1 (otherwise the launch would silently take the plain loop).  y and the statistic rows are
pre-filled with a sentinel and must be written everywhere; a 64 KiB guard area behind each stays untouched; x's whole buffer
(NaN outside a channel slice) and the packed kernels come back bit-unchanged.

Bars on y, each segment against its own fp64 reference:
  1. the project's (tests/test_gpu_f16.py): helpers.rel_err <= 1e-3 for fp16 output, <= 2e-5 for fp32 output;
  2. one tied to the arithmetic: ek = rel_err(kernel, fp64), e = rel_err(fp32 reference rounded to the output type, fp64) -- from
     the reference alone -- and ek / max(e, 2^-23) <= RATIO_BOUND[family]; families (f16_conv_ref.family): fp32 output, fp16
     output, fp16 output with an input fold;
  3. per element, without any measurement: |got - y64| <= K 2^-23 S + 2^-23 (S + |bias|) + 1/2 ulp_out(|y64| + that)
     (f16_conv_ref.element_bound; S = conv(|x|, |w|), K products per output; for an input fold plus one fp16 spacing of every
     operand element whose fp32-formed and fp64-formed values differ).
Bars on the statistic rows, against fp64 sums of the kernel's own stored y over each m-tile: |sum y| within BM 2^-24 sum |y|,
sum y^2 within BM 2^-23 sum y^2 (order-independent); rn_group_norm_finalize of the rows against the fp64 mean / rstd of y at the
1e-5 / 1e-4 tests/test_gpu_f16.py grants.

RATIO_BOUND = {fp32-out: 1, fp16-out: 4, fp16-fold: 2}, set on 2026-10-21: per family twice the largest ratio of any segment of any
call of that family in one run of the table on an MI355X, rounded up to a power of two (figures as printed in
profiles/f16_conv_cases_err.txt, 101 lines).  The kernels have a fixed reduction order, so the figures have no run-to-run noise.
  fp32-out:   largest ratio 0.4146 (cfg0- / cfg2- / cfg4-vec8: ek 1.99e-7, e 4.81e-7 -- the matrix core's sums of exact products are
              closer to fp64 than the fp32 reference's own); next 0.3993 (cfg5-vec8); largest ek 2.04e-7 (sg-miss-f32)
  fp16-out:   largest ratio 1.0003 (auto-2: ek 2.269e-4, e 2.268e-4); next 1.0000 (pipe2-stats, pipe1-short-stats, sg1-stats, ...): the
              rounding of the output to fp16 is the whole error, of the kernel as of the reference; largest ek 4.54e-4
  fp16-fold:  largest ratio 1.0000 (sg2-relu: ek = e = 4.229e-4); next 1.0000 (sg1-relu, fin7-pipe-2048, fin7-pipe-k5); largest ek 4.23e-4
The worst element stands at 0.998 of its per-element bound (auto-0: K = 8, so the bound is half an fp16 spacing and little else),
0.94 with an input fold (fin7-plain-short); the worst statistic row at 0.013 (sums) / 0.023 (sums of squares) of its bound
(fin3-3x3-cin96).  Every equal-bits claim of the source held on the device: the three K loops, non-temporal loads, y with and
without the statistics epilogue, the super-group kernel's FIN 1 against rn_group_norm_apply_f16's tensor, a second call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import f16_conv_ref as R
from helpers import rel_err
from test_f16_conv_cases_cpu import EXPECT, PROCESS_ROWS, child_paths

pytestmark = pytest.mark.gpu

BAR = {R.FP32_OUT: 2e-5, R.FP16_OUT: 1e-3, R.FP16_FOLD: 1e-3}
RATIO_BOUND = {R.FP32_OUT: 1.0, R.FP16_OUT: 4.0, R.FP16_FOLD: 2.0}
SENTINEL = 12352.0          # exactly representable in fp16, far from any output
GUARD = 1 << 16
FINALIZE_GROUPS = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


def _sync():
    """(a fault of the device ends the whole session: nothing more is started on it)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error, nothing more is started on it: %s" % e, returncode=3)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


class Buffers:
    """The device tensors of a case: x (inside its wider NaN-filled buffer for channel slices), the packed kernels, bias, and the
    GroupNorm folded into the operand load."""

    def __init__(self, case, dev):
        import _rn
        L = _rn.lib()
        xs, ws, bs, gn = R.make_case(case)
        self.case = case
        self.x = []
        for x in xs:
            if case.x_ld:
                buf = np.full(x.shape[:3] + (case.x_ld,), np.nan, np.float16)
                buf[..., case.x_coff:case.x_coff + case.cin] = x
                x = buf
            self.x.append(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
        self.xkeep = [t.clone() for t in self.x]
        packed = {}
        self.w, self.bias = [], []
        cin_g = case.cin // case.groups
        for w, b, cout in zip(ws, bs, case.cout):
            if id(w) not in packed:
                full, _ = R.wgt_bytes(case, cout)
                wt = torch.zeros(full // 2, dtype=torch.float16, device=dev)
                wd = torch.from_numpy(w).to(dev).contiguous()
                _rn.check(L.rn_pack_weights_f16(wd.data_ptr(), wt.data_ptr(), case.k, case.k, cin_g, cout, _rn.stream()), "rn_pack_weights_f16")
                _sync()
                assert np.array_equal(wt[:cout * case.k * case.k * cin_g].cpu().numpy().reshape(cout, -1), w.reshape(-1, cout).T.astype(np.float16))
                packed[id(w)] = (wt, torch.from_numpy(b).to(dev) if b is not None else None)
            self.w.append(packed[id(w)][0])
            self.bias.append(packed[id(w)][1])
        self.wkeep = [t.clone() for t in self.w]
        self.gn = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in gn] if gn else None

    def unchanged(self):
        for t, k in zip(self.x + self.w, self.xkeep + self.wkeep):
            assert torch.equal(_bits(t), _bits(k)), "an input buffer changed"


class Result:
    pass


def run(case, dev, monkeypatch, expect=None, bufs=None, tweak=None, status=0):
    """One call for the case -> Result: ys (numpy, one per segment), part (numpy [2, rows, cout] or None), row, starts / tiles (rows of
    every segment), plan.  status != 0: the call must be refused with it and write nothing."""
    import _rn
    L = _rn.lib()
    R.configure(case, monkeypatch)
    b = bufs or Buffers(case, dev)
    call = R.HostCall(case, tweak=tweak, tiles=[1] * len(case.segs) if status else None)
    ydt = torch.float32 if case.out_f32 else torch.float16
    ys, numels = [], []
    for i, (s, (n, h, w), cout) in enumerate(zip(call.segs, case.segs, case.cout)):
        oh, ow = R.out_hw(case, h, w)
        numels.append(n * oh * ow * cout)
        ys.append(torch.full((numels[-1] + GUARD // (4 if case.out_f32 else 2),), SENTINEL, dtype=ydt, device=dev))
        s.x, s.wgt, s.y = b.x[i].data_ptr(), b.w[i].data_ptr(), ys[-1].data_ptr()
        s.bias = b.bias[i].data_ptr() if b.bias[i] is not None else None
    res = Result()
    res.plan = plan = call.query(status=status)
    res.row = R.row_of(plan, call.nseg)
    part, prows = None, 0
    if call.fold is not None:
        f = call.fold
        if case.stats == 2:
            prows = f.total_chunks
        else:
            prows = case.segs[0][0] * (plan.rows_per_sample if not status else 1)
        part = torch.full((2 * prows * case.cout[0] + GUARD // 4,), SENTINEL, dtype=torch.float32, device=dev)
        if f.partial:
            f.partial = part.data_ptr()
        if case.fold and f.in_mean:
            f.in_mean, f.in_rstd, f.in_gamma, f.in_beta = (t.data_ptr() for t in b.gn)
    if status:
        e = L.rn_conv2d_fwd_f16_fold(call.segs, call.nseg, C.byref(call.geom), call.fold_ref(), _rn.stream()) if call.fold is not None else \
            L.rn_conv2d_fwd_f16(call.segs, call.nseg, C.byref(call.geom), 1 if case.out_f32 else 0, _rn.stream())
        _sync()
        assert e == status, (e, L.rn_last_error().decode())
        assert all(bool((y == SENTINEL).all()) for y in ys) and (part is None or bool((part == SENTINEL).all())), "a refused call wrote"
        b.unchanged()
        return res
    if expect is not None:
        assert res.row == expect, "the call takes %s, not %s" % (res.row, expect)
    if plan.pipe:
        assert L.rn_conv2d_f16_pipe_available() == 1, "the pipelined kernels' dynamic LDS was refused: the launch would take the plain loop"
    if call.fold is not None:
        _rn.check(L.rn_conv2d_fwd_f16_fold(call.segs, call.nseg, C.byref(call.geom), call.fold_ref(), _rn.stream()), "rn_conv2d_fwd_f16_fold")
    else:
        _rn.check(L.rn_conv2d_fwd_f16(call.segs, call.nseg, C.byref(call.geom), 1 if case.out_f32 else 0, _rn.stream()), "rn_conv2d_fwd_f16")
    _sync()
    b.unchanged()
    res.ys = []
    for i, (y, numel, (n, h, w), cout) in enumerate(zip(ys, numels, case.segs, case.cout)):
        assert bool((y[numel:] == SENTINEL).all()), "segment %d: the guard area behind y changed" % i
        assert not bool((y[:numel] == SENTINEL).any()), "segment %d: elements of y were not written" % i
        res.ys.append(y[:numel].cpu().numpy().reshape((n,) + R.out_hw(case, h, w) + (cout,)))
    res.part = None
    if part is not None:
        used = 2 * prows * case.cout[0]
        assert bool((part[used:] == SENTINEL).all()), "the guard area behind the statistic rows changed"
        assert not bool((part[:used] == SENTINEL).any()), "statistic rows were not written"
        res.part = part[:used].cpu().numpy().reshape(2, prows, case.cout[0])
        res.part_dev, res.prows = part, prows
        res.starts = list(call.starts) if case.stats == 2 else [0]
        res.tiles = list(plan.tiles_per_sample[:call.nseg]) if case.stats == 2 else [plan.rows_per_sample]
    return res


def out_round(case, y32):
    return y32 if case.out_f32 else y32.astype(np.float16)


def compare_y(case, res):
    """-> [(segment, family, ek, e, ratio, worst |got - y64| / element bound)]"""
    _, _, bs, _ = R.make_case(case)
    fam, lines = R.family(case), []
    for i, (got, ref) in enumerate(zip(res.ys, R.run_ref(case))):
        assert got.shape == ref.y64.shape, (got.shape, ref.y64.shape)
        g64 = got.astype(np.float64)
        assert np.isfinite(g64).all(), "segment %d: y holds NaN / inf" % i
        ek, e = rel_err(g64, ref.y64), rel_err(out_round(case, ref.y32), ref.y64)
        elem = float((np.abs(g64 - ref.y64) / R.element_bound(case, ref, bs[i])).max())
        lines.append((i, fam, ek, e, ek / max(e, 2.0 ** -23), elem))
    return lines


def sg_rows(y, th, tw=16):
    """y [n, oh, ow, c] -> [n * tiles, th * tw, c]: the super-group kernel's tiles of th x 16 output pixels, row-major per sample"""
    n, oh, ow, c = y.shape
    return y.reshape(n, oh // th, th, ow // tw, tw, c).transpose(0, 1, 3, 2, 4, 5).reshape(-1, th * tw, c)


def check_stats(case, res, dev):
    """The statistic rows against fp64 sums of the kernel's own stored y; -> worst (sum, sum of squares) error over its bound"""
    import _rn
    worst = [0.0, 0.0]
    for i, y in enumerate(res.ys):
        if not res.tiles[i]:
            continue                # (this segment's tiles straddle samples: it has no rows)
        n, oh, ow, c = y.shape
        y64 = y.astype(np.float64)
        if res.row[0] == "sg":
            bm = 256 if res.row[1] == 1 else 128
            t = sg_rows(y64, 16 if res.row[1] == 1 else 8)
        else:
            bm = R.BM[res.row[1]]
            t = y64.reshape(-1, bm, c)
        assert t.shape[0] == n * res.tiles[i] and oh * ow == res.tiles[i] * bm
        s1, s2, sa = t.sum(1), (t * t).sum(1), np.abs(t).sum(1)
        rows = res.part[:, res.starts[i]:res.starts[i] + n * res.tiles[i]].astype(np.float64)
        b1, b2 = bm * 2.0 ** -24 * sa, bm * 2.0 ** -23 * s2
        bad1, bad2 = np.abs(rows[0] - s1) > b1, np.abs(rows[1] - s2) > b2
        assert not bad1.any() and not bad2.any(), "segment %d: %d sums, %d sums of squares outside their bound" % (i, bad1.sum(), bad2.sum())
        worst = [max(worst[0], float((np.abs(rows[0] - s1) / np.maximum(b1, 1e-300)).max())), max(worst[1], float((np.abs(rows[1] - s2) / np.maximum(b2, 1e-300)).max()))]
    if case.stats == 1:
        y = res.ys[0].astype(np.float64)
        n, oh, ow, c = y.shape
        mean, rstd = torch.empty((n, FINALIZE_GROUPS), device=dev), torch.empty((n, FINALIZE_GROUPS), device=dev)
        _rn.check(_rn.lib().rn_group_norm_finalize(res.part_dev.data_ptr(), n, res.tiles[0], oh * ow, c, FINALIZE_GROUPS, R.EPS, mean.data_ptr(),
                                                   rstd.data_ptr(), _rn.stream()), "rn_group_norm_finalize")
        yg = y.reshape(n, oh * ow, FINALIZE_GROUPS, c // FINALIZE_GROUPS)
        assert rel_err(mean.cpu().numpy(), yg.mean((1, 3))) <= 1e-5 and rel_err(rstd.cpu().numpy(), 1.0 / np.sqrt(yg.var((1, 3)) + R.EPS)) <= 1e-4
    return worst


def record_lines(name, lines, stats=None):
    """The call's lines of profiles/f16_conv_cases_err.txt."""
    out = ["F16_ERR %-18s y%d %-9s ek %.3e  e %.3e  ratio %8.4f  elem %5.3f" % ((name, i, fam, ek, e, ratio, elem)) for i, fam, ek, e, ratio, elem in lines]
    if stats:
        out.append("F16_ERR %-18s rows          sum %5.3f  sum of squares %5.3f of their bounds" % (name, stats[0], stats[1]))
    return out


def check(name, lines):
    bad = ["y%d: ek %.3e (bar %.0e), e %.3e, ratio %.2f (bound %s), worst element at %.3f of its bound" % (i, ek, BAR[fam], e, ratio, RATIO_BOUND[fam], elem)
           for i, fam, ek, e, ratio, elem in lines if ek > BAR[fam] or ratio > RATIO_BOUND[fam] or elem > 1.0]
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def run_and_check(name, case, dev, monkeypatch, expect, bufs=None):
    res = run(case, dev, monkeypatch, expect, bufs)
    lines = compare_y(case, res)
    stats = check_stats(case, res, dev) if res.part is not None else None
    print("\n".join(record_lines(name, lines, stats)))
    check(name, lines)
    return res


LAUNCHED = [name for name, case in R.CASES.items() if case.launch]


@pytest.mark.parametrize("name", LAUNCHED)
def test_case_matches_fp64(dev, monkeypatch, name):
    run_and_check(name, R.CASES[name], dev, monkeypatch, EXPECT[name])


def test_near_misses_are_planned_only():
    assert [n for n, c in R.CASES.items() if not c.launch] == ["auto-5-miss-big", "auto-5-miss-k128", "auto-5-miss-k512", "auto-5-miss-vec4"]


@pytest.mark.parametrize("what", [w for w, (_, tweak, _) in R.REFUSALS.items() if tweak != "f32"])
def test_a_refused_call_writes_nothing(dev, monkeypatch, what):
    case, tweak, status = R.REFUSALS[what]
    run(case, dev, monkeypatch, tweak=tweak, status=status)


def _same_bits(a, b, what):
    assert len(a.ys) == len(b.ys)
    for i, (p, q) in enumerate(zip(a.ys, b.ys)):
        assert p.dtype == q.dtype and np.array_equal(p.view(np.uint16 if p.dtype == np.float16 else np.uint32), q.view(np.uint16 if q.dtype == np.float16 else np.uint32)), \
            "%s: y%d differs in %d elements, by up to %g" % (what, i, int((p != q).sum()), float(np.abs(p.astype(np.float64) - q.astype(np.float64)).max()))


# the same data through two K loops of the 256 x 256 tile: the pipelined loops and the plain one give the same bits
# (conv_f16.hip: "the plain loop below computes the same bits")
LOOP_PAIRS = [("pipe1-short", "cfg5-tap"), ("pipe1-short-stats", "pipe2-stats"), ("fin7-plain-short", "fin7-pipe-k2")]


@pytest.mark.parametrize("a,b", LOOP_PAIRS)
def test_k_loops_give_the_same_bits(dev, monkeypatch, a, b):
    assert R.math_key(R.CASES[a]) == R.math_key(R.CASES[b]) and EXPECT[a][5] != EXPECT[b][5]
    bufs = Buffers(R.CASES[a], dev)
    ra, rb = run(R.CASES[a], dev, monkeypatch, EXPECT[a], bufs), run(R.CASES[b], dev, monkeypatch, EXPECT[b], bufs)
    _same_bits(ra, rb, "%s / %s" % (a, b))
    if ra.part is not None:
        assert np.array_equal(ra.part, rb.part), "the statistic rows differ"


@pytest.mark.parametrize("name", ["stem", "pipe2-stats", "pipe1-short-stats", "multi-stats", "multi-stats-cfg5", "multi-stats-vec4", "sg1-stats", "sg2-stats", "sg1-cg4"])
def test_statistics_epilogue_leaves_y_unchanged(dev, monkeypatch, name):
    case = R.CASES[name]
    bufs = Buffers(case, dev)
    with_rows = run(case, dev, monkeypatch, EXPECT[name], bufs)
    plain = run(case._replace(stats=0), dev, monkeypatch, None, bufs)
    assert plain.row[:2] == with_rows.row[:2] and plain.part is None and (plain.row[3] if plain.row[0] == "sg" else plain.row[4]) == 0
    _same_bits(with_rows, plain, name)


@pytest.mark.parametrize("name", ["sg1-elu", "sg2-elu"])
def test_super_group_fold_equals_the_materialised_operand(dev, monkeypatch, name):
    """FIN 1 forms act(GN(x)) once per patch element exactly as rn_group_norm_apply_f16 would have stored it: the same kernel on
    that tensor gives the same bits, y and statistic rows."""
    import _rn
    case = R.CASES[name]
    bufs = Buffers(case, dev)
    folded = run(case, dev, monkeypatch, EXPECT[name], bufs)
    n, h, w = case.segs[0]
    op = torch.empty_like(bufs.x[0])
    mean, rstd, gamma, beta = bufs.gn
    _rn.check(_rn.lib().rn_group_norm_apply_f16(bufs.x[0].data_ptr(), None, op.data_ptr(), n, h * w, case.cin, R.IN_GROUPS, mean.data_ptr(), rstd.data_ptr(),
                                                gamma.data_ptr(), beta.data_ptr(), _rn.ACT[case.fold], 0, _rn.stream()), "rn_group_norm_apply_f16")
    _sync()
    bufs.x, bufs.xkeep, bufs.gn = [op], [op.clone()], None
    plain = run(case._replace(fold=None), dev, monkeypatch, EXPECT[name.replace("elu", "stats")], bufs)
    _same_bits(folded, plain, name)
    assert np.array_equal(folded.part, plain.part), "the statistic rows differ"


@pytest.mark.parametrize("name", ["cfg5-tap", "cfg2-vec4", "fin7-pipe-k5", "fin3-elu", "multi-stats-cfg5", "sg1-relu", "sg2-elu"])
def test_second_call_is_bit_identical(dev, monkeypatch, name):
    bufs = Buffers(R.CASES[name], dev)
    a, b = run(R.CASES[name], dev, monkeypatch, EXPECT[name], bufs), run(R.CASES[name], dev, monkeypatch, EXPECT[name], bufs)
    _same_bits(a, b, name)
    assert (a.part is None) == (b.part is None) and (a.part is None or np.array_equal(a.part, b.part))


# --------------------------------------------------------------------------------- the once-per-process switches, in fresh children
# cases whose child output the parent compares bit for bit with its own (the same kernel family under another K loop / load kind);
# the others (the super-group shapes on the implicit GEMM) meet the bars in the child
BIT_EQUAL = {"pipe0-sg0": ["cfg5-tap", "pipe2-stats", "fin7-pipe-k2"], "pipe1-nt1": ["cfg5-tap", "pipe2-stats", "pipe2-one-n-tile", "fin7-pipe-k2"],
             "nt0-mink64": ["auto-5"]}


class _Env:
    """monkeypatch's two calls, for the child process below"""

    def delenv(self, name, raising=False):
        os.environ.pop(name, None)

    def setenv(self, name, value):
        os.environ[name] = value


def _child(group, outdir):
    """(in a fresh process started with the group's switches) every launched case of the group under the child's plan row; the outputs
    go to `outdir` for the parent to compare"""
    dev = torch.device("cuda:0")
    R.PROCESS_SWITCHES = ()
    for name, row in PROCESS_ROWS[group][1].items():
        case = R.CASES[name]
        if not case.launch:
            continue
        if name in BIT_EQUAL[group]:
            res = run(case, dev, _Env(), row)
        else:
            res = run_and_check(name, case, dev, _Env(), row)
        np.savez(os.path.join(outdir, name + ".npz"), *res.ys, **({"part": res.part} if res.part is not None else {}))


@pytest.mark.parametrize("group", list(PROCESS_ROWS))
def test_once_per_process_switches(dev, monkeypatch, tmp_path, group):
    """RN_F16_PIPE, RN_F16_SG, RN_F16_NT and RN_F16_PIPE_MIN_K are read once per process: each group of switches in a fresh child.
    The plain loop (RN_F16_PIPE=0), the loop with both operands through LDS (1) and the default give the same bits, and so do
    non-temporal and ordinary operand loads."""
    env, rows = PROCESS_ROWS[group]
    code = "import sys; sys.path[:0] = %r; import test_gpu_f16_conv_cases as G; G._child(%r, %r)" % (child_paths(), group, str(tmp_path))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit("the child under %s hung, nothing more is started on the GPU: %s" % (env, e), returncode=3)
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (3, 124, 134, 137, 139):       # a signal (abort, segmentation fault, kill), or the child's own pytest.exit
        pytest.exit("the child under %s ended with %d, nothing more is started on the GPU: %s" % (env, r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for name in BIT_EQUAL[group]:
        assert EXPECT[name] != rows[name]
        mine = run(R.CASES[name], dev, monkeypatch, EXPECT[name])
        with np.load(os.path.join(str(tmp_path), name + ".npz")) as theirs:
            for i, y in enumerate(mine.ys):
                t = theirs["arr_%d" % i]
                assert t.dtype == y.dtype and np.array_equal(t.view(np.uint16), y.view(np.uint16)), \
                    "%s: y%d under %s differs from the default in %d elements" % (name, i, env, int((t != y).sum()))
            if mine.part is not None:
                assert np.array_equal(theirs["part"], mine.part), "%s: the statistic rows differ under %s" % (name, env)
