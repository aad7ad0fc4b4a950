"""The tail of the training step -- csrc/loss.hip through ops.detection_loss, csrc/optimizer.hip through train.ParamArena /
train.Optimizer -- against the float64 reference of tests/step_tail_ref.py, element by element, at the edges of the kernels: every
quads-per-lane instantiation of the four-lane loss kernels, the wave-per-row kernels, 16-row groups over three segments, one-row
and RN_MAX_SEG segments, both grids past their first pass, saturated logits, non-finite logits on masked rows, weight decay that
matters, clipping that binds and clipping that does not, the padding of the arena (runs on the MI355X box: -m gpu).

The bar: assert_close(..., TOL, what, elementwise_tol=TOL) with TOL = 1e-4 (BASELINE.json's north_star), i.e. max-norm AND
element-wise (floor 1e-3 of the largest element); what is called exact is compared with np.array_equal / ==.  The worst
element-wise error of every family is printed when the module ends (-s shows it)."""
import collections
import functools

import numpy as np
import pytest
import torch

import step_tail_ref as ref
from helpers import assert_close, elementwise_rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
MODES = ("bce_dice", "focal")
WORST = collections.OrderedDict()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    yield torch.device("cuda:0")
    print("\nworst element-wise relative error against float64, by family (bar %.0e):" % TOL)
    for family, e in WORST.items():
        print("  %-28s %.3e" % (family, e))


def _t(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_(grad)


def _close(family, got, want, what):
    e = elementwise_rel_err(got, want)
    WORST[family] = max(WORST.get(family, 0.0), e)
    print("%s [%s]: element-wise %.3e" % (what, family, e))
    assert_close(got, want, TOL, what, elementwise_tol=TOL)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ loss

LossGot = collections.namedtuple("LossGot", "cls reg stats dz dr")


def _run_loss(dev, inp, mode, g_cls=ref.G_CLS, g_reg=ref.G_REG):
    import ops
    segs = ref.segments(inp)
    zg = [_t(s[0], dev, True) for s in segs]
    rg = [_t(s[2], dev, True) for s in segs]
    cl, rl, stats = ops.detection_loss(zg, rg, [_t(s[1], dev) for s in segs], [_t(s[3], dev) for s in segs],
                                       [_t(s[4].astype(np.uint8), dev) for s in segs], inp.c, mode)
    total = 0.0
    if g_cls is not None:
        total = total + g_cls * cl
    if g_reg is not None:
        total = total + g_reg * rl
    total.backward()
    torch.cuda.synchronize()
    return LossGot(cl.item(), rl.item(), stats.cpu().numpy(), np.concatenate([t.grad.cpu().numpy() for t in zg]),
                   np.concatenate([t.grad.cpu().numpy() for t in rg]))


@functools.lru_cache(maxsize=None)
def _loss_ref(name, mode, g_cls=ref.G_CLS, g_reg=ref.G_REG, dtype=torch.float64):
    return ref.loss_ref(ref.loss_case(name), mode, g_cls, g_reg, dtype)


def _check_loss(inp, mode, got, want, tag, keep=None, cls_want=None):
    """Everything the loss returns against the reference.  `keep`: the elements of dz that are compared; `cls_want`: another
    expected class loss than the float64 one."""
    _close("loss scalars", got.cls, want.cls if cls_want is None else cls_want, "%s class loss" % tag)
    _close("loss scalars", got.reg, want.reg, "%s regr loss" % tag)
    assert got.stats[0] == np.float32(got.cls) and got.stats[1] == np.float32(got.reg)
    assert got.stats[2] == want.M and got.stats[3] == want.nfg, (got.stats[:4], want.M, want.nfg)
    if mode == "bce_dice":
        import _rn
        per_class = got.stats[_rn.LOSS_STATS_HEADER:_rn.LOSS_STATS_HEADER + 3 * inp.c].reshape(inp.c, 3)
        for col, (what, w) in enumerate((("I", want.I), ("L", want.L), ("P", want.P))):
            _close("dice statistics", per_class[:, col], w, "%s per-class %s" % (tag, what))
    dz, dz_want = (got.dz, want.dz) if keep is None else (np.where(keep, got.dz, 0.0), np.where(keep, want.dz, 0.0))
    _close("dz " + mode, dz, dz_want, "%s d cls logits" % tag)
    _close("dr", got.dr, want.dr, "%s d reg" % tag)
    # rows outside the trainable mask: exactly zero (the buffers come from torch.empty: every element was written)
    assert not got.dz[~inp.mask].any() and not got.dr[~inp.mask].any()
    assert np.isfinite(got.dz).all() and np.isfinite(got.dr).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ref.SWEEP_CASES)
def test_loss_dispatch_sweep(dev, name, mode):
    """Segments of (37, 1, 250, 15, 1209) rows: boundaries off the multiples of 16, one 16-row group over three segments, a
    one-row segment, a ragged last group.  C = 16 NK - 12 and 16 NK for every NK of the four-lane kernels (a lone quad in the
    last k and a full one), and the wave-per-row kernels on both sides of their 64-class lanes."""
    inp = ref.loss_case(name)
    _check_loss(inp, mode, _run_loss(dev, inp, mode), _loss_ref(name, mode), name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ref.MAXSEG_CASES)
def test_loss_max_segments(dev, name, mode):
    inp = ref.loss_case(name)
    assert len(inp.seg_rows) == ref.MAX_SEG
    _check_loss(inp, mode, _run_loss(dev, inp, mode), _loss_ref(name, mode), name)


def test_loss_refuses_what_it_cannot_do(dev):
    import _rn
    assert _rn.MAX_SEG == ref.MAX_SEG
    with pytest.raises(_rn.RnError):
        _run_loss(dev, ref.loss_inputs(1, 257, seg_rows=(40,)), "focal")
    with pytest.raises(_rn.RnError):
        _run_loss(dev, ref.loss_inputs(2, 20, seg_rows=ref.SEG_ROWS_MAX + (5,)), "bce_dice")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ref.WRAP_CASES)
def test_loss_grid_wrap(dev, name, mode):
    """More rows than one pass of the capped grid: 262144 + 389 in two unequal segments for the four-lane kernels (some waves
    go round again, most do not), 40000 for the wave-per-row kernels."""
    inp = ref.loss_case(name)
    _check_loss(inp, mode, _run_loss(dev, inp, mode), _loss_ref(name, mode), name)


@pytest.mark.parametrize("name", ref.PLANT_CASES)
def test_loss_saturated_logits(dev, name):
    """24 planted logits on trainable rows, half under a label of 1.  bce_dice: +-8, +-17, +-30, +-90, all compared with float64.
    focal: -90 .. 8 compared with float64; 12, 17, 30 and 90 (8 elements) are not -- there the reference's own float32 formula
    loses 1 - p against eps = 1e-7 (1.4e-4 at z = 12, 26 % at z >= 17) -- and must be finite and of the right sign, and the class
    loss of that set is compared at TOL with the float32 oracle instead of float64."""
    mode = name.split("-")[1]
    inp = ref.loss_case(name)
    got, want = _run_loss(dev, inp, mode), _loss_ref(name, mode)
    ill = ref.ill_conditioned(inp, mode)
    if mode == "focal":
        assert 0 < ill.sum() <= 12
        _check_loss(inp, mode, got, want, name, keep=~ill, cls_want=_loss_ref(name, mode, dtype=torch.float32).cls)
        assert np.isfinite(got.cls) and np.isfinite(got.dz[ill]).all()
        assert (got.dz[ill & (inp.lab == 0.0)] >= 0.0).all() and (got.dz[ill & (inp.lab == 1.0)] <= 0.0).all()
    else:
        assert not ill.any()
        _check_loss(inp, mode, got, want, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", ref.MASKING_C)
def test_loss_masked_rows_never_reach_a_sum(dev, c, mode):
    """NaN, +inf and -inf logits on rows outside the trainable mask: the reference removes those rows (boolean_mask), so the
    losses, the statistics and every gradient on every other row equal the run without them, and those rows get exactly 0."""
    clean, dirty = ref.loss_case("clean-%d" % c), ref.loss_case("nonfinite-%d" % c)
    rows = ref.nonfinite_rows(c)
    a, b = _run_loss(dev, clean, mode), _run_loss(dev, dirty, mode)
    _check_loss(clean, mode, a, _loss_ref("clean-%d" % c, mode), "clean-%d" % c)
    assert (a.cls, a.reg) == (b.cls, b.reg), (a.cls, b.cls, a.reg, b.reg)
    assert np.array_equal(a.stats, b.stats)
    assert np.array_equal(a.dz, b.dz) and np.array_equal(a.dr, b.dr)
    assert not b.dz[rows].any() and not b.dr[rows].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ref.SMALL_END_CASES)
def test_loss_small_ends(dev, name, mode):
    """One row in all; one trainable row among masked ones; exactly one foreground row."""
    inp = ref.loss_case(name)
    _check_loss(inp, mode, _run_loss(dev, inp, mode), _loss_ref(name, mode), name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", ref.MASKING_C)
def test_loss_backward_of_one_loss_alone(dev, c, mode):
    name = "sweep-%d" % c
    inp = ref.loss_case(name)
    got, want = _run_loss(dev, inp, mode, g_reg=None), _loss_ref(name, mode, ref.G_CLS, None)
    assert not got.dr.any() and not want.dr.any()
    _check_loss(inp, mode, got, want, name + " class loss alone")
    got, want = _run_loss(dev, inp, mode, g_cls=None), _loss_ref(name, mode, None, ref.G_REG)
    assert not got.dz.any() and not want.dz.any()
    _check_loss(inp, mode, got, want, name + " regr loss alone")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["clean-20", "clean-3", "wrap4"])
def test_loss_is_bitwise_reproducible(dev, name, mode):
    inp = ref.loss_case(name)
    a, b = _run_loss(dev, inp, mode), _run_loss(dev, inp, mode)
    assert np.float32(a.cls).tobytes() == np.float32(b.cls).tobytes() and np.float32(a.reg).tobytes() == np.float32(b.reg).tobytes()
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------------------- optimizer

OptGot = collections.namedtuple("OptGot", "w state1 state2 norm_reg counter")
KINDS = ("momentum", "rmsprop", "adam")


def _run_optimizer(dev, inp, kind, clip=None, slices=None, counter_slices=(0, 2)):
    """Three steps on a synthetic module laid out as `inp`; one OptGot per step.  `slices`: begin_step / step_slice /
    finish_step over these ranges, the dropout counter given to the slices of `counter_slices`."""
    import ops
    import train
    assert train.FUSED_OPT_NORM
    mod = torch.nn.Module()
    for i, (off, s, l2) in enumerate(zip(inp.offsets, inp.sizes, inp.l2)):
        p = torch.nn.Parameter(torch.from_numpy(inp.w0[off:off + s].copy()))
        if l2 is not None:
            p.l2_scale = l2
        setattr(mod, "p%d" % i, p)
    mod.to(dev)
    arena = train.ParamArena(mod, dev)
    assert arena.count == inp.count and tuple(o for o, _ in arena.offsets) == inp.offsets
    assert np.array_equal(arena.wd_per_block.cpu().numpy(), inp.wd_elem[::ref.OPT_BLOCK])
    opt = train.Optimizer(arena, kind, inp.lr, grad_clip_norm=clip)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out, launches = [], 0
    for g in inp.grads:
        for p, off, s in zip(arena.params, inp.offsets, inp.sizes):
            p.grad.copy_(torch.from_numpy(g[off:off + s]).to(dev))
        if slices is None:
            opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
            launches += 1
        else:
            opt.begin_step()
            for i, (lo, hi) in enumerate(slices):
                opt.step_slice(lo, hi, inp.grad_scale, counter if i in counter_slices else None)
                launches += i in counter_slices
            opt.finish_step()
        torch.cuda.synchronize()
        # exactly once per launch that was given the counter, however often the grid goes round
        assert counter.item() == launches * ops.DROPOUT_COUNTER_STEP
        out.append(OptGot(arena.weights.cpu().numpy(), opt.state1.cpu().numpy(),
                          opt.state2.cpu().numpy() if opt.state2 is not None else None, opt.norm_reg.cpu().numpy(), counter.item()))
    for p, off, s in zip(arena.params, inp.offsets, inp.sizes):        # the module's parameters are the arena
        assert np.array_equal(p.detach().cpu().numpy(), out[-1].w[off:off + s])
    return out


@functools.lru_cache(maxsize=None)
def _optimizer_ref(name, kind, clip):
    return ref.optimizer_ref(ref.optimizer_case(name), kind, clip)


def _check_optimizer(inp, kind, got, want, tag):
    pad = ref.padding_mask(inp)
    for step, (a, b) in enumerate(zip(got, want), 1):
        what = "%s step %d" % (tag, step)
        _close("weights", a.w, b.w, what + " weights")
        _close("state1 " + kind, a.state1, b.state1, what + " state1")
        if kind != "momentum":
            _close("state2 " + kind, a.state2, b.state2, what + " state2")
        _close("global norm", float(a.norm_reg[0]) ** 0.5, b.norm, what + " global norm")
        _close("regulariser", float(a.norm_reg[1]), b.reg, what + " regulariser")
        # the padding: weights exactly zero, the states at their initial value evolved on a zero gradient
        assert not a.w[pad].any()
        if kind == "rmsprop":
            assert len(np.unique(a.state1[pad])) == 1 and abs(a.state1[pad][0] / 0.9 ** step - 1.0) <= TOL
            assert not a.state2[pad].any()
        else:
            assert not a.state1[pad].any() and (a.state2 is None or not a.state2[pad].any())


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_small_arena_fused_norm(dev, kind):
    """grad_clip_norm=None: rn_optimizer_update (RN_OPT_F_NORM) + rn_norm_reg_finalize, whole and in three slices at non-zero offsets.
    Parameters of 1152, 700, 1, 1025 and 3000 elements with l2 scales 0.3, 0.05, 1.0, none and 0.6: a wrong block index, or
    a decay that is dropped, moves the weights by far more than TOL."""
    inp = ref.optimizer_case("small")
    want = _optimizer_ref("small", kind, None)
    whole = _run_optimizer(dev, inp, kind)
    _check_optimizer(inp, kind, whole, want, "small %s fused" % kind)
    sliced = _run_optimizer(dev, inp, kind, slices=ref.SMALL_SLICES)
    _check_optimizer(inp, kind, sliced, want, "small %s sliced" % kind)
    for a, b in zip(whole, sliced):        # the update is element-wise: the slicing only regroups the sums of norm_reg
        assert np.array_equal(_bits(a.w), _bits(b.w)) and np.array_equal(_bits(a.state1), _bits(b.state1))


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_small_arena_clipping(dev, kind):
    """The norm pass + rn_optimizer_update (RN_OPT_F_CLIP).  Clip 0.5 binds (the norm is about 100).  Clip 1e6 does not: clip / max(norm,
    clip) is exactly 1, so the weights equal the unclipped run's bit for bit and norm_reg agrees with the fused path's."""
    inp = ref.optimizer_case("small")
    binds = _run_optimizer(dev, inp, kind, clip=ref.CLIP_BINDS)
    _check_optimizer(inp, kind, binds, _optimizer_ref("small", kind, ref.CLIP_BINDS), "small %s clip binds" % kind)
    loose = _run_optimizer(dev, inp, kind, clip=ref.CLIP_LOOSE)
    _check_optimizer(inp, kind, loose, _optimizer_ref("small", kind, ref.CLIP_LOOSE), "small %s clip loose" % kind)
    fused = _run_optimizer(dev, inp, kind)
    for a, b in zip(loose, fused):
        assert np.array_equal(_bits(a.w), _bits(b.w))
        _close("norm_reg, two paths", a.norm_reg, b.norm_reg, "small %s norm_reg clipped path against fused path" % kind)
    assert not np.array_equal(binds[0].w, fused[0].w)


@pytest.mark.parametrize("clip", [None, ref.CLIP_BINDS], ids=["fused", "clipped"])
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_optimizer_large_arena(dev, kind, clip):
    """One parameter of 2097152 + 5 * 1024 + 7 elements, then three small ones with their own l2 scales: more than 2048 blocks
    of 256 threads x 4 elements, so the grid cap binds, part of the grid goes round again, and the small parameters' decay
    lies in the wrapped region; the clipped path runs rn_grad_norm_l2reg with its block count clamped."""
    inp = ref.optimizer_case("large")
    _check_optimizer(inp, kind, _run_optimizer(dev, inp, kind, clip=clip), _optimizer_ref("large", kind, clip),
                     "large %s %s" % (kind, "fused" if clip is None else "clipped"))


@pytest.mark.parametrize("clip", [None, ref.CLIP_BINDS], ids=["fused", "clipped"])
@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_is_bitwise_reproducible(dev, kind, clip):
    inp = ref.optimizer_case("small")
    for a, b in zip(_run_optimizer(dev, inp, kind, clip=clip), _run_optimizer(dev, inp, kind, clip=clip)):
        for x, y in zip(a[:4], b[:4]):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
