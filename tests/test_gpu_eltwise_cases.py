"""The kernels of csrc/elementwise.hip -- max / average pool, lateral + upsampled top, stand-alone activations, rn_add_segs,
rn_flip_width -- on the case tables of tests/eltwise_ref.py, driven through the C entry points (ctypes).

Everywhere: outputs are pre-filled with a sentinel and must be written everywhere (and nowhere else: guard areas behind the
arg-max bytes and the add_segs buffers), inputs come back bit-unchanged, a second call gives the same bits.

  max pool     y equals the oracle's fp32 maximum bit for bit, on continuous and on TIED inputs (post-ReLU zeros, integers in
               {-1, 0, 1}: at least a quarter of the windows hold their maximum twice, tests/test_eltwise_cases_cpu.py); the
               arg-max bytes are the tap index of the FIRST valid maximum in row-major order (numpy restatement); dx of
               rn_maxpool_bwd_arg equals dx of the rescanning rn_maxpool_bwd bit for bit, and both are within
               (T + 1) 2^-24 sum|dy| of the oracle's autograd in fp64, T = windows that contain the cell.
  average pool the same bound form with one more rounding (the reciprocal): (T + 2) 2^-24 sum|terms|, T = valid cells of the
               window (forward) / windows that contain the cell (backward).
  upsample-add y bit-equal to lateral + the oracle's nearest-neighbour resize (roundf ties included), dlateral is dy itself,
               dtop within (T + 1) 2^-24 sum|dy| of autograd in fp64 (T = fine cells that read the coarse cell); a coarse cell
               nobody reads gets exactly 0.
  activations  relu, relu6 and identity equal the oracle in value at every element, forward and backward, at the kinks too
               (0, -0, 6 and their neighbours; Relu6Grad is 0 AT 0 and 6).  "In value": a zero may differ in sign -- the kernels
               return +0 for relu(-0) and dy * 0 keeps dy's sign, torch returns -0 and +0 --, every other float is bit-equal.
               elu and sigmoid: the project's 1e-4 (helpers.rel_err) and an ABSOLUTE bar against fp64, set on 2026-10-21 at
               twice the worst figure of one run of this table on an MI355X, rounded up to a power of two
               (profiles/eltwise_cases_err.txt):
                 elu      forward 7.2e-8 -> 2^-22 (2.4e-7),  backward 2.3e-7 -> 2^-21 (4.8e-7)
                 sigmoid  forward 9.2e-8 -> 2^-22,           backward 2.9e-7 -> 2^-20 (9.5e-7)
               (all four worst figures at the count of 4096 x 256 + 5; the backward figures carry |dy| up to 5).  The "6e-8" of
               csrc/rn_common.h for exp(z) - 1 against expm1(z) was an estimate; measured here: 7.2e-8.
  add_segs     bit-equal to the fp32 sum for 1, 3 and RN_MAX_SEG segments of mixed counts (tails of 1 to 3, counts below 4),
               in place (out == a) too; nothing behind a segment's count is touched.
  flip_width   bit-equal to a numpy flip, fp32 (with the negated component) and u8."""
import ctypes as C

import numpy as np
import pytest
import torch

import eltwise_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
SENTINEL = 12345.0
GUARD = 4096
# absolute bars of the transcendental activations against fp64: (forward, backward), see the docstring
ACT_ABS_BAR = {"elu": (2.0 ** -22, 2.0 ** -21), "sigmoid": (2.0 ** -22, 2.0 ** -20)}


@pytest.fixture(scope="module")
def rn():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return _rn


DEV = torch.device("cuda:0")


def _sent(shape, dtype=torch.float32):
    return torch.full(tuple(shape), SENTINEL, dtype=dtype, device=DEV)


def _written(t):
    return not bool((t == SENTINEL).any())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within(got, ref64, bound, what):
    err = np.abs(got.astype(np.float64) - ref64)
    assert not np.any((bound == 0) & (err > 0)), "%s: an element no term reaches is not exact" % what
    frac = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    assert frac <= 1.0, "%s: %.3f of the element bound" % (what, frac)
    return frac


POOL_CASES = [(p, kind) for p in R.POOLS for kind in (R.CONTINUOUS,) + R.TIED]


@pytest.mark.parametrize("p,kind", POOL_CASES, ids=["%s-%s" % (R.pool_id(p), k) for p, k in POOL_CASES])
def test_max_pool(rn, p, kind):
    L = rn.lib()
    x, dy = R.pool_input(p, kind)
    xd, dyd = x.to(DEV), dy.to(DEV)
    keep = xd.clone(), dyd.clone()
    geom = (p.n, p.h, p.w, p.c, p.k, p.s)
    nout = dy.numel()

    def fwd(with_arg):
        y = _sent(dy.shape)
        arg = torch.full((nout + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        rn.check(L.rn_maxpool_fwd(rn.f32(xd), rn.f32(y), arg.data_ptr() if with_arg else None, *geom, rn.stream()), "rn_maxpool_fwd")
        torch.cuda.synchronize()
        assert bool((arg[nout:] == 0xFF).all()) and (with_arg or bool((arg == 0xFF).all()))
        return y, arg[:nout].reshape(dy.shape)

    y, arg = fwd(True)
    y32 = R.pool_ref("max", x, dy, p.k, p.s, torch.float32)[0]
    assert _same_bits(y.cpu(), torch.from_numpy(y32)), "y is not the oracle's maximum bit for bit"
    want = R.argmax_taps(x, p.k, p.s)
    got_arg = arg.cpu().numpy()
    assert np.array_equal(got_arg, want), "%d arg-max bytes are not the first valid maximum's tap" % int((got_arg != want).sum())
    y_b, arg_b = fwd(True)
    assert _same_bits(y_b, y) and torch.equal(arg_b, arg)
    assert _same_bits(fwd(False)[0], y)

    def bwd(use_arg):
        dx = _sent(x.shape)
        if use_arg:
            rn.check(L.rn_maxpool_bwd_arg(arg.data_ptr(), rn.f32(dyd), rn.f32(dx), *geom, rn.stream()), "rn_maxpool_bwd_arg")
        else:
            rn.check(L.rn_maxpool_bwd(rn.f32(xd), rn.f32(dyd), rn.f32(dx), *geom, rn.stream()), "rn_maxpool_bwd")
        return dx

    arg = arg.contiguous()
    dxa, dxr = bwd(True), bwd(False)
    assert _written(dxa) and _written(dxr)
    assert _same_bits(dxa, dxr), "rn_maxpool_bwd_arg and rn_maxpool_bwd differ"
    assert _same_bits(bwd(True), dxa) and _same_bits(bwd(False), dxr)
    ref = R.pool_ref("max", x, dy, p.k, p.s, torch.float64)[1]
    bound = (R.windows_per_cell(p)[None, :, :, None] + 1) * R.U * R.pool_ref("max", x, dy.abs(), p.k, p.s, torch.float64)[1]
    _within(dxa.cpu().numpy(), ref, bound, "dx")
    assert rel_err(dxa.cpu().numpy(), ref) <= GRAD_BAR
    torch.cuda.synchronize()
    assert torch.equal(xd, keep[0]) and torch.equal(dyd, keep[1])


@pytest.mark.parametrize("p", R.POOLS, ids=R.pool_id)
def test_average_pool(rn, p):
    L = rn.lib()
    x, dy = R.pool_input(p, R.CONTINUOUS)
    xd, dyd = x.to(DEV), dy.to(DEV)
    keep = xd.clone(), dyd.clone()
    geom = (p.n, p.h, p.w, p.c, p.k, p.s)

    def fwd():
        y = _sent(dy.shape)
        rn.check(L.rn_avgpool_fwd(rn.f32(xd), rn.f32(y), *geom, rn.stream()), "rn_avgpool_fwd")
        return y

    def bwd():
        dx = _sent(x.shape)
        rn.check(L.rn_avgpool_bwd(rn.f32(dyd), rn.f32(dx), *geom, rn.stream()), "rn_avgpool_bwd")
        return dx

    y, dx = fwd(), bwd()
    assert _written(y) and _written(dx) and _same_bits(fwd(), y) and _same_bits(bwd(), dx)
    y64, dx64 = R.pool_ref("avg", x, dy, p.k, p.s, torch.float64)
    ya, dxa = R.pool_ref("avg", x.abs(), dy.abs(), p.k, p.s, torch.float64)
    _within(y.cpu().numpy(), y64, (R.valid_cells(p)[None, :, :, None] + 2) * R.U * ya, "y")
    _within(dx.cpu().numpy(), dx64, (R.windows_per_cell(p)[None, :, :, None] + 2) * R.U * dxa, "dx")
    assert rel_err(y.cpu().numpy(), y64) <= OUT_BAR and rel_err(dx.cpu().numpy(), dx64) <= GRAD_BAR
    torch.cuda.synchronize()
    assert torch.equal(xd, keep[0]) and torch.equal(dyd, keep[1])


@pytest.mark.parametrize("p", R.POOLS_F16, ids=R.pool_id)
def test_max_pool_f16(rn, p):
    for kind in (R.CONTINUOUS, R.RELU):
        x16 = R.pool_input(p, kind)[0].half()
        xd = x16.to(DEV)
        keep = xd.clone()
        want = T.max_pool_same(x16.float(), p.k, p.s).half()
        ys = []
        for _ in range(2):
            y = _sent(want.shape, torch.float16)
            rn.check(rn.lib().rn_maxpool_fwd_f16(rn.f16(xd), rn.f16(y), p.n, p.h, p.w, p.c, p.k, p.s, rn.stream()), "rn_maxpool_fwd_f16")
            ys.append(y)
        assert _same_bits(ys[0].cpu(), want) and _same_bits(ys[0], ys[1]) and torch.equal(xd, keep)


def test_upsample_add(rn):
    L = rn.lib()
    worst = 0.0
    for u in R.UPS:
        lat, top, dy = R.up_input(u)
        ld, td, dd = lat.to(DEV), top.to(DEV), dy.to(DEV)
        keep = [t.clone() for t in (ld, td, dd)]
        geom = (u.n, u.h, u.w, u.th, u.tw, u.c)
        ys, ds = [], []
        for _ in range(2):
            y, dtop = _sent(lat.shape), _sent(top.shape)
            rn.check(L.rn_upsample_add_fwd(rn.f32(ld), rn.f32(td), rn.f32(y), *geom, rn.stream()), "rn_upsample_add_fwd")
            rn.check(L.rn_upsample_add_bwd_top(rn.f32(dd), rn.f32(dtop), *geom, rn.stream()), "rn_upsample_add_bwd_top")
            ys.append(y)
            ds.append(dtop)
        assert _written(ys[0]) and _written(ds[0]) and _same_bits(ys[0], ys[1]) and _same_bits(ds[0], ds[1]), u
        y32 = R.up_ref(lat, top, dy, torch.float32)[0]
        assert _same_bits(ys[0].cpu(), torch.from_numpy(y32)), "%s: y is not lateral + resized top bit for bit" % (u,)
        d64 = R.up_ref(lat, top, dy, torch.float64)[1]
        bound = (R.up_sources(u)[None, :, :, None] + 1) * R.U * R.up_ref(lat, top, dy.abs(), torch.float64)[1]
        worst = max(worst, _within(ds[0].cpu().numpy(), d64, bound, "%s: dtop" % (u,)))
        assert rel_err(ds[0].cpu().numpy(), d64) <= GRAD_BAR, u
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((ld, td, dd), keep)), u
    print("ELTCASE upsample-add dtop: worst %.3f of the element bound over %d shape pairs" % (worst, len(R.UPS)))


def test_upsample_add_gradient_of_the_lateral_is_dy(rn):
    import ops
    u = R.UPS_F16[0]
    lat, top, dy = (t.to(DEV) for t in R.up_input(u))
    lat.requires_grad_(True)
    top.requires_grad_(True)
    y = ops.upsample_add(lat, top)
    dlat, dtop = torch.autograd.grad(y, (lat, top), dy)
    assert _same_bits(dlat, dy)
    direct = _sent(top.shape)
    rn.check(rn.lib().rn_upsample_add_bwd_top(rn.f32(dy), rn.f32(direct), u.n, u.h, u.w, u.th, u.tw, u.c, rn.stream()), "rn_upsample_add_bwd_top")
    assert _same_bits(dtop, direct)


@pytest.mark.parametrize("u", R.UPS_F16, ids=lambda u: "%dx%d-from-%dx%d" % (u.h, u.w, u.th, u.tw))
def test_upsample_add_f16(rn, u):
    lat, top, _ = R.up_input(u)
    lat16, top16 = lat.half(), top.half()
    want = (lat16.float() + T.upsample_nearest_align_corners(top16.float(), u.h, u.w)).half()      # the fp32 sum, rounded once
    ld, td = lat16.to(DEV), top16.to(DEV)
    keep = ld.clone(), td.clone()
    ys = []
    for _ in range(2):
        y = _sent(lat.shape, torch.float16)
        rn.check(rn.lib().rn_upsample_add_fwd_f16(rn.f16(ld), rn.f16(td), rn.f16(y), u.n, u.h, u.w, u.th, u.tw, u.c, rn.stream()), "rn_upsample_add_fwd_f16")
        ys.append(y)
    assert _same_bits(ys[0].cpu(), want) and _same_bits(ys[0], ys[1]) and torch.equal(ld, keep[0]) and torch.equal(td, keep[1])


def _same_values(got, ref):
    """Equal as floats at every element: bit-equal but for the sign of a zero (no NaN anywhere)."""
    return not np.isnan(got).any() and not np.isnan(ref).any() and np.array_equal(got, ref)


@pytest.mark.parametrize("count", R.ACT_COUNTS)
@pytest.mark.parametrize("act,kind", R.ACTS, ids=[str(k) for _, k in R.ACTS])
def test_activation(rn, act, kind, count):
    L = rn.lib()
    x, dy = R.act_input(count)
    room = count + GUARD
    xd, dyd = x.to(DEV), dy.to(DEV)
    keep = xd.clone(), dyd.clone()
    outs = []
    for _ in range(2):
        y, dx = _sent((room,)), _sent((room,))
        rn.check(L.rn_act_fwd(rn.f32(xd), rn.f32(y), count, act, rn.stream()), "rn_act_fwd")
        rn.check(L.rn_act_bwd(rn.f32(xd), rn.f32(dyd), rn.f32(dx), count, act, rn.stream()), "rn_act_bwd")
        assert bool((y[count:] == SENTINEL).all()) and bool((dx[count:] == SENTINEL).all()), "written behind count"
        outs.append((y[:count], dx[:count]))
    (y, dx), (y_b, dx_b) = outs
    assert _written(y) and _written(dx) and _same_bits(y, y_b) and _same_bits(dx, dx_b)
    assert torch.equal(xd, keep[0]) and torch.equal(dyd, keep[1])
    y, dx = y.cpu().numpy(), dx.cpu().numpy()
    if kind in (None, "relu", "relu6"):
        y32, dx32 = R.act_ref(x, dy, kind, torch.float32)
        assert _same_values(y, y32), "forward differs at x = %s" % x.numpy()[y != y32][:5]
        assert _same_values(dx, dx32), "backward differs at x = %s" % x.numpy()[dx != dx32][:5]
        if kind is None:
            assert _same_bits(torch.from_numpy(y), x) and _same_bits(torch.from_numpy(dx), dy)
    else:
        y64, dx64 = R.act_ref(x, dy, kind, torch.float64)
        ey, ed = float(np.abs(y - y64).max()), float(np.abs(dx - dx64).max())
        print("ELTCASE act %-7s count %8d: abs err fwd %.3e bwd %.3e | rel_err fwd %.3e bwd %.3e" % (kind, count, ey, ed, rel_err(y, y64), rel_err(dx, dx64)))
        assert rel_err(y, y64) <= OUT_BAR and rel_err(dx, dx64) <= OUT_BAR
        fbar, bbar = ACT_ABS_BAR[kind]
        assert fbar is not None and ey <= fbar and ed <= bbar, (ey, ed)


def test_activation_f16_needs_whole_quads(rn):
    x = torch.zeros(8, dtype=torch.float16, device=DEV)
    y = _sent((8,), torch.float16)
    assert rn.lib().rn_act_fwd_f16(rn.f16(x), rn.f16(y), 6, 1, rn.stream()) == -1
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


ADD_COUNTS = [1, 3, 4, 5, 1023, 1024 * 1024 + 2]
ADD_CALLS = {"1-seg-tail": [5], "1-seg-large": [1024 * 1024 + 2], "3-segs": [3, 1024 * 1024 + 2, 1],
             "max-segs": [ADD_COUNTS[i % 6] for i in range(16)]}


@pytest.mark.parametrize("which", list(ADD_CALLS))
def test_add_segs(rn, which):
    counts = ADD_CALLS[which]
    assert len(counts) in (1, 3, rn.MAX_SEG)
    rng = np.random.default_rng(8000 + len(counts))
    pad = 64

    def buf(values):
        t = _sent((len(values) + pad,))
        t[:len(values)] = torch.from_numpy(values).to(DEV)
        return t

    host = [(rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)) for n in counts]
    for _ in range(2):
        bufs = [(buf(a), buf(b), None if i % 2 else _sent((n + pad,))) for i, ((a, b), n) in enumerate(zip(host, counts))]   # odd: out == a
        segs = (rn.AddSeg * len(counts))()
        for s, (a, b, o), n in zip(segs, bufs, counts):
            s.a, s.b, s.out, s.count = a.data_ptr(), b.data_ptr(), (o if o is not None else a).data_ptr(), n
            assert s.a % 16 == 0 and s.b % 16 == 0 and s.out % 16 == 0
        rn.check(rn.lib().rn_add_segs(segs, len(counts), rn.stream()), "rn_add_segs")
        torch.cuda.synchronize()
        for i, ((a, b, o), (ha, hb), n) in enumerate(zip(bufs, host, counts)):
            out = o if o is not None else a
            assert _same_bits(out[:n].cpu(), torch.from_numpy(ha + hb)), "segment %d (count %d)" % (i, n)
            assert all(bool((t[n:] == SENTINEL).all()) for t in (a, b, out)), "segment %d: written behind count %d" % (i, n)
            assert _same_bits(b[:n].cpu(), torch.from_numpy(hb)) and (o is None or _same_bits(a[:n].cpu(), torch.from_numpy(ha)))
    # a pointer off 16 bytes is refused and nothing is written
    a, b, o = buf(host[0][0]), buf(host[0][1]), _sent((counts[0] + pad,))
    seg = (rn.AddSeg * 1)()
    seg[0].a, seg[0].b, seg[0].out, seg[0].count = a.data_ptr(), b.data_ptr(), o.data_ptr() + 4, counts[0]
    assert rn.lib().rn_add_segs(seg, 1, rn.stream()) == -1
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())


@pytest.mark.parametrize("elem", ["f32", "u8"])
def test_flip_width(rn, elem):
    rng = np.random.default_rng(9000)
    for outer in (0, 3):
        for w in (1, 2, 7):
            for inner in (1, 4, 5):
                for neg in ((0, 0), (4, 1)) if elem == "f32" else ((0, 0),):
                    shape = (max(outer, 1), w, inner)
                    if elem == "f32":
                        x = rng.standard_normal(shape, dtype=np.float32)
                        want = x[:, ::-1, :].copy()
                        if neg[0]:
                            want[:, :, np.arange(inner) % neg[0] == neg[1]] *= -1
                    else:
                        x = rng.integers(0, 256, shape, dtype=np.uint8)
                        want = x[:, ::-1, :].copy()
                    xd = torch.from_numpy(x).to(DEV)
                    keep = xd.clone()
                    ys = []
                    for _ in range(2):
                        y = torch.full(shape, 77, dtype=xd.dtype, device=DEV)
                        rn.check(rn.lib().rn_flip_width(xd.data_ptr(), y.data_ptr(), outer, w, inner, xd.element_size(), neg[0], neg[1], rn.stream()),
                                 "rn_flip_width")
                        ys.append(y)
                    torch.cuda.synchronize()
                    what = (elem, outer, w, inner, neg)
                    if outer == 0:
                        assert bool((ys[0] == 77).all()), what          # nothing to flip: nothing written
                    else:
                        assert _same_bits(ys[0].cpu(), torch.from_numpy(want)) and _same_bits(ys[0], ys[1]), what
                    assert torch.equal(xd, keep), what
