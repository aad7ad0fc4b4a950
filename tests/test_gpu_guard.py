"""The guard against non-finite gradients (skip_nonfinite) on the MI355X (-m gpu): rn_step_control_eval's gate and the gated update
against the float64 reference (guard_ref.py), a skipped update bit for bit, guard on against guard off on finite gradients,
Optimizer.step() captured and replayed, the two entries called directly, the one launch sequence of every configuration, and a
guarded trainer's ONE captured graph over a poisoned step, against eager launches, a checkpoint and the command line.

TOL = 1e-4, element-wise, is test_gpu_clip_graph.py's bar for this arithmetic; everything that is not a comparison with float64
is bit equality."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import ema_ref
import guard_ref as ref
import lr_schedule_ref
import step_tail_ref
from helpers import assert_close, elementwise_rel_err, step_control

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = ("momentum", "rmsprop", "adam")
SETTING = "warm"            # ema_ref's setting with warm-up: d = 1/10, 2/11, 3/12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    return torch.device("cuda:0")


def _close(got, want, what):
    print("%s: element-wise %.3e" % (what, elementwise_rel_err(got, want)))
    assert_close(got, want, TOL, what, elementwise_tol=TOL)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the optimizer alone
Got = collections.namedtuple("Got", "w state1 state2 norm_reg e step_dev lr_dev ema_updates_dev ema_dev gate skipped counter")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _snapshot(arena, opt, counter):
    torch.cuda.synchronize()
    return Got(_np(arena.weights), _np(opt.state1), _np(opt.state2), _np(opt.norm_reg), _np(opt.ema), _np(opt.step_dev), _np(opt.lr_dev),
               _np(opt.ema_updates_dev), _np(opt.ema_dev), _np(opt.gate_dev), _np(opt.skipped_dev), int(counter.item()))


def _make(dev, inp, kind, clip=None, scheduled=False, setting=None, guard=True, schedule=None, accumulate_steps=1):
    """test_gpu_clip_graph._make with the guard's keyword: a synthetic module laid out as `inp` and its optimizer."""
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
    kw = {}
    if setting is not None:
        kw.update(ema_decay=ema_ref.SETTINGS[setting].decay, ema_warmup=ema_ref.SETTINGS[setting].warmup)
    if schedule is not None:
        kw.update(schedule=schedule)
    elif scheduled:
        kw.update(schedule=train.LRSchedule(base_lr=inp.lr, **ref.SCHEDULE))
    if guard:
        kw.update(skip_nonfinite=True)
    return mod, arena, train.Optimizer(arena, kind, inp.lr, grad_clip_norm=clip, accumulate_steps=accumulate_steps, **kw)


def _load_grad(arena, inp, g, dev):
    for p, off, s in zip(arena.params, inp.offsets, inp.sizes):
        p.grad.copy_(torch.from_numpy(np.asarray(g[off:off + s], np.float32)).to(dev))


def _run(dev, inp, grads, kind, clip=None, scheduled=False, setting=None, guard=True, schedule=None):
    """Every gradient of `grads` as one opt.step().  Returns the state before the first step and after each."""
    _, arena, opt = _make(dev, inp, kind, clip, scheduled, setting, guard, schedule)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out = [_snapshot(arena, opt, counter)]
    for g in grads:
        _load_grad(arena, inp, g, dev)
        opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
        out.append(_snapshot(arena, opt, counter))
    return out, opt


@functools.lru_cache(maxsize=None)
def _want(which, kind, clip, scheduled, setting):
    inp = ref.guard_case()
    g0, g1, g2 = inp.grads
    return ref.guard_ref(inp, [g0, ref.poisoned(inp, which), g1, g2], kind, clip, scheduled, setting)


def _unchanged(a, b, what):
    """A skipped update: everything the optimizer owns but norm_reg, the gate and the skip counters keeps its bits."""
    for f in ("w", "state1", "state2", "e", "step_dev", "lr_dev", "ema_updates_dev", "ema_dev"):
        assert _same_bits(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("setting", [None, SETTING], ids=["no-average", "average"])
@pytest.mark.parametrize("scheduled", [False, True], ids=["constant", "scheduled"])
@pytest.mark.parametrize("clip", [None, ref.CLIP_BINDS], ids=["unclipped", "binds"])
@pytest.mark.parametrize("kind", KINDS)
def test_small_arena_against_the_reference(dev, kind, clip, scheduled, setting):
    """[g0, BAD, g1, g2] for each of the three poisons on the small arena (9 blocks): w, the slots, the average and norm_reg after
    each APPLIED update against float64, the skipped one leaving them as they were; padding stays zero.  Scheduled: the rates
    base / 3, 2 base / 3, base go to the three applied updates, Adam's bias correction with them."""
    import ops
    inp = ref.guard_case()
    pad = step_tail_ref.padding_mask(inp)
    g0, g1, g2 = inp.grads
    for which in ref.POISONS:
        want = _want(which, kind, clip, scheduled, setting)
        assert want.applied == (True, False, True, True)
        got, opt = _run(dev, inp, [g0, ref.poisoned(inp, which), g1, g2], kind, clip, scheduled, setting)
        assert _same_bits(got[0].w, inp.w0) and not got[0].norm_reg.any()
        u = 0
        for i, applied in enumerate(want.applied):
            a, tag = got[i + 1], "%s %s clip %s step %d" % (which, kind, clip, i + 1)
            assert tuple(int(v) for v in a.skipped) == want.counters[i] and tuple(a.gate) == (0, int(applied)), tag
            assert a.counter == (i + 1) * ops.DROPOUT_COUNTER_STEP
            if not applied:
                _unchanged(a, got[i], tag)
                assert not np.isfinite(a.norm_reg[0]) and not np.isfinite(want.norm_sq[i])
                continue
            st = want.run.steps[u]
            _close(a.w, st.w, tag + " weights")
            _close(a.state1, st.state1, tag + " state1")
            if kind != "momentum":
                _close(a.state2, st.state2, tag + " state2")
            _close(float(a.norm_reg[0]) ** 0.5, st.norm, tag + " global norm")
            _close(float(a.norm_reg[1]), st.reg, tag + " regulariser")
            if want.run.e is not None:
                _close(a.e, want.run.e[u], tag + " average")
                assert not _bits(a.e[pad]).any()
            assert not a.w[pad].any()
            u += 1
            if a.step_dev is not None:
                assert int(a.step_dev[0]) == u
            if a.ema_updates_dev is not None:
                assert int(a.ema_updates_dev[0]) == u
        assert u == 3 and opt.step_count == 4                    # (the host has not looked yet: it runs ahead by the skip)
        assert opt.reconcile_skips() == (1, 0) and opt.step_count == 3 and opt.reconcile_skips() == (1, 0) and opt.step_count == 3
        if scheduled:
            assert opt.current_lr() == float(opt.schedule.value(3))
            assert lr_schedule_ref.ulp_distance(opt.lr_dev[0].item(), opt.schedule.value(2)) <= 1


@pytest.mark.parametrize("kind", KINDS)
def test_a_skipped_update_changes_nothing(dev, kind):
    """Scheduled, clipped, with the average: before and after the BAD step w, state1, state2, ema, step_dev, lr_dev,
    ema_updates_dev and ema_dev are bit-identical; the dropout counter moved by DROPOUT_COUNTER_STEP; norm_reg[0] is not finite;
    counters (1, 1), then (1, 0) after g1.  Two BAD steps in a row: (2, 2)."""
    import ops
    inp = ref.guard_case()
    g0, g1, _ = inp.grads
    for which in ref.POISONS:
        got, opt = _run(dev, inp, [g0, ref.poisoned(inp, which), g1, ref.poisoned(inp, "nan"), ref.poisoned(inp, which)], kind,
                        ref.CLIP_BINDS, True, SETTING)
        before, after, then = got[1], got[2], got[3]
        _unchanged(after, before, which)
        assert int(before.step_dev[0]) == 1 == int(after.step_dev[0]) and int(after.ema_updates_dev[0]) == 1
        assert after.counter - before.counter == ops.DROPOUT_COUNTER_STEP
        assert not np.isfinite(after.norm_reg[0]) and np.isfinite(before.norm_reg[0])
        assert (np.isnan(after.norm_reg[0]), np.isposinf(after.norm_reg[0])) == {"nan": (True, False)}.get(which, (False, True))
        assert tuple(after.skipped) == (1, 1) and tuple(after.gate) == (0, 0) and tuple(before.skipped) == (0, 0)
        assert tuple(then.skipped) == (1, 0) and tuple(then.gate) == (0, 1) and int(then.step_dev[0]) == 2
        assert not _same_bits(then.w, after.w) and not _same_bits(then.e, after.e)
        assert tuple(got[4].skipped) == (2, 1) and tuple(got[5].skipped) == (3, 2)
        _unchanged(got[5], then, which + ", two in a row")
        assert opt.reconcile_skips() == (3, 2) and opt.step_count == 2


@pytest.mark.parametrize("setting", [None, SETTING], ids=["no-average", "average"])
@pytest.mark.parametrize("scheduled", [False, True], ids=["constant", "scheduled"])
@pytest.mark.parametrize("clip", [None, ref.CLIP_BINDS], ids=["unclipped", "binds"])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_on_finite_gradients_equals_guard_off(dev, kind, clip, scheduled, setting):
    """Three finite gradients, the same LRSchedule object on both sides: w, the slots and the average bit-identical after every
    update; norm_reg within TOL of the unclipped fused path's (another kernel sums it in another order) and bit-identical to the
    clipped path's (the same pass).  Constant rate: momentum takes it as a launch argument on both sides; guarded Adam / RMSProp
    read it from the device, so the guard-off side is given the same LRSchedule('constant', lr) object (Adam's bias correction is
    then formed by the same device code on both sides, not by the host's pow on one of them)."""
    import train
    inp = ref.guard_case()
    sched = train.LRSchedule(base_lr=inp.lr, **ref.SCHEDULE) if scheduled else None
    if sched is None and kind != "momentum":
        sched = train.LRSchedule("constant", inp.lr)
    on, opt_on = _run(dev, inp, inp.grads, kind, clip, False, setting, True, sched)
    off, opt_off = _run(dev, inp, inp.grads, kind, clip, False, setting, False, sched)
    if sched is not None:
        assert opt_on.schedule is sched and opt_off.schedule is sched
        if not scheduled:                                            # what a guarded optimizer builds by itself when given none
            assert _make(dev, inp, kind)[2].schedule == sched
    else:
        assert opt_off.lr_dev is None and opt_on.lr_dev is None
    for u, (a, b) in enumerate(zip(on, off)):
        assert _same_bits(a.w, b.w) and _same_bits(a.state1, b.state1) and _same_bits(a.state2, b.state2) and _same_bits(a.e, b.e), u
        if u and clip is not None:
            assert _same_bits(a.norm_reg, b.norm_reg), u
        elif u:
            _close(a.norm_reg, b.norm_reg, "norm_reg, guarded path against fused path, update %d" % u)
        if sched is not None:
            assert _same_bits(a.lr_dev, b.lr_dev) and _same_bits(a.step_dev, b.step_dev)
        assert a.counter == b.counter
    assert not _same_bits(on[-1].w, on[0].w) and tuple(on[-1].skipped) == (0, 0) and opt_on.step_count == 3 == opt_off.step_count


def test_step_captured_and_replayed_equals_eager(dev):
    """opt.step() with the guard -- scheduled Adam, the average, CLIP_BINDS -- captured once and replayed over [g0, BAD, g1, g2]
    with the next gradient copied into arena.grads before each replay, against four eager calls: everything bit-identical, the
    device words and the counters included."""
    import ops
    inp = ref.guard_case()
    g0, g1, g2 = inp.grads
    grads = [g0, ref.poisoned(inp, "overflow"), g1, g2]
    eager, _ = _run(dev, inp, grads, "adam", ref.CLIP_BINDS, True, SETTING)
    _, arena, opt = _make(dev, inp, "adam", ref.CLIP_BINDS, True, SETTING)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    w_before = arena.weights.clone()
    _load_grad(arena, inp, g0, dev)
    # (no warm-up call: step() allocates nothing, and the eager run above has launched every kernel of it once already)
    g = torch.cuda.CUDAGraph()
    count = opt.step_count
    with torch.cuda.graph(g):
        opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
    opt.step_count = count                                                         # (recorded, not run)
    torch.cuda.synchronize()
    assert torch.equal(arena.weights, w_before) and opt.step_dev.item() == 0 and counter.item() == 0 and not opt.skipped_dev.any()
    for i, grad in enumerate(grads):
        _load_grad(arena, inp, grad, dev)
        g.replay()
        opt.count_step()
        got = _snapshot(arena, opt, counter)
        for f, x, y in zip(Got._fields, got, eager[i + 1]):
            assert x == y if f == "counter" else _same_bits(x, y), (i, f)
    assert opt.step_dev.item() == 3 == opt.ema_updates_dev.item() and tuple(opt.skipped_dev.tolist()) == (1, 0)
    assert opt.reconcile_skips() == (1, 0) and opt.step_count == 3
    assert counter.item() == 4 * ops.DROPOUT_COUNTER_STEP
    r = opt.lr_dev.cpu().numpy()
    assert lr_schedule_ref.ulp_distance(r[1], lr_schedule_ref.adam_rate(r[0], 2)) <= 1 and r[1] != r[0]


def test_entries_called_directly(dev):
    """rn_step_control_eval (GUARD) on norm_sq 1, 0, inf, nan (and -inf, FLT_MAX): gates 1, 1, 0, 0 (0, 1) and the counters that go with
    them; the gated update with the gate closed touches nothing but the counter; bad arguments come back negative."""
    import _rn
    L = _rn.lib()
    norm = torch.zeros(2, dtype=torch.float32, device=dev)
    gate = torch.full((2,), 7, dtype=torch.int32, device=dev)
    skipped = torch.zeros(2, dtype=torch.int64, device=dev)
    fmax = float(np.finfo(np.float32).max)
    want_total = want_row = 0

    def finite_gate(norm_sq, gate_dev, skipped_dev, stream):
        return step_control(stream, features=_rn.CTL_F_GUARD, norm_sq=norm_sq, gate_dev=gate_dev, skipped_dev=skipped_dev)
    for v, g in ((1.0, 1), (0.0, 1), (float("inf"), 0), (float("nan"), 0), (float("nan"), 0), (fmax, 1), (float("-inf"), 0), (1.0, 1)):
        norm[0] = v
        _rn.check(finite_gate(_rn.f32(norm), gate.data_ptr(), skipped.data_ptr(), _rn.stream()), "rn_step_control_eval")
        want_total, want_row = want_total + (1 - g), (0 if g else want_row + 1)
        assert gate.tolist() == [0, g] and skipped.tolist() == [want_total, want_row], v
    assert want_total == 4
    # the gated update, gate closed and then open, momentum on one block
    n = step_tail_ref.OPT_BLOCK
    w = torch.randn(n, device=dev)
    grad, s1, wd = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(1, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    w0 = w.clone()

    def gated(kind, w, grad, state1, state2, wd, count, lr, lr_dev, grad_scale, clip_norm, norm_sq, step, advance_counter, advance_by,
              ema, ema_dev, gate_dev, stream):
        f = (_rn.OPT_F_GATE | (_rn.OPT_F_CLIP if clip_norm > 0 else 0) | (_rn.OPT_F_LRDEV if lr_dev is not None else 0)
             | (_rn.OPT_F_EMA if None not in (ema, ema_dev) else 0))
        u = _rn.OptUpdate(kind=kind, features=f, w=w, grad=grad, state1=state1, state2=state2, wd_per_block=wd, count=count, lr=lr,
                          grad_scale=grad_scale, step=step, advance_counter=advance_counter, advance_by=advance_by, lr_dev=lr_dev,
                          ema=ema, ema_dev=ema_dev, clip_norm=clip_norm, norm_sq=norm_sq, gate_dev=gate_dev)
        return L.rn_optimizer_update(ctypes.byref(u), stream)

    def update(g):
        gate[1] = g
        _rn.check(gated(0, _rn.f32(w), _rn.f32(grad), _rn.f32(s1), None, _rn.f32(wd), n, 0.5, None, 1.0, 0.0, None, 1,
                        counter.data_ptr(), 3, None, None, gate.data_ptr(), _rn.stream()), "rn_optimizer_update")
        torch.cuda.synchronize()
    update(0)
    assert torch.equal(w, w0) and not s1.any() and counter.item() == 3
    update(1)
    assert torch.equal(s1, grad) and torch.equal(w, w0 - 0.5 * grad) and counter.item() == 6
    # refusals (no launch)
    q = ctypes.c_void_p(norm.data_ptr())
    assert finite_gate(None, q, q, None) < 0 and finite_gate(q, None, q, None) < 0 and finite_gate(q, q, None, None) < 0
    assert finite_gate(q, ctypes.c_void_p(norm.data_ptr() + 2), q, None) < 0
    args = [0, _rn.f32(w), _rn.f32(grad), _rn.f32(s1), None, _rn.f32(wd), n, 0.5, None, 1.0, 0.0, None, 1, None, 0, None, None]
    assert gated(*(args + [None, None])) < 0
    assert gated(*(args[:10] + [-1.0] + args[11:] + [gate.data_ptr(), None])) < 0
    assert gated(*(args[:10] + [0.5] + args[11:] + [gate.data_ptr(), None])) < 0          # clipping without norm_sq
    assert gated(*(args[:6] + [n - 24] + args[7:] + [gate.data_ptr(), None])) < 0
    assert gated(*([2] + args[1:] + [gate.data_ptr(), None])) < 0                         # Adam without state2
    torch.cuda.synchronize()
    assert torch.equal(w, w0 - 0.5 * grad)


# ---------------------------------------------------------------------------------------------- the one sequence
class _RecordingLib(object):
    """_rn.lib() with the name of every rn_* entry called appended to `calls`; the call itself goes through."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rn_"):
            return fn

        def call(*args):
            self._calls.append(name)
            return fn(*args)
        return call


NORM_AHEAD = ["rn_grad_norm_partial", "rn_norm_reg_finalize"]
CONTROL, UPDATE, FINALIZE = "rn_step_control_eval", "rn_optimizer_update", "rn_norm_reg_finalize"
SEQUENCES = {
    # name: (keywords of _make, steps, the launches of ONE step in order)
    "plain": (dict(guard=False), 1, [UPDATE, FINALIZE]),
    "schedule": (dict(guard=False, scheduled=True), 1, [CONTROL, UPDATE, FINALIZE]),
    "ema": (dict(guard=False, setting=SETTING), 1, [CONTROL, UPDATE, FINALIZE]),
    "schedule+ema": (dict(guard=False, scheduled=True, setting=SETTING), 1, [CONTROL, UPDATE, FINALIZE]),
    "clip": (dict(guard=False, clip=ref.CLIP_BINDS), 1, NORM_AHEAD + [UPDATE]),
    "clip+schedule": (dict(guard=False, clip=ref.CLIP_BINDS, scheduled=True), 1, NORM_AHEAD + [CONTROL, UPDATE]),
    "accum": (dict(guard=False, accumulate_steps=2), 2, [CONTROL, UPDATE, FINALIZE]),
    "guard": (dict(guard=True), 1, NORM_AHEAD + [CONTROL, UPDATE]),
    "guard+clip+schedule+ema": (dict(guard=True, clip=ref.CLIP_BINDS, scheduled=True, setting=SETTING), 1, NORM_AHEAD + [CONTROL, UPDATE]),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_every_configuration_takes_the_one_sequence(dev, name, monkeypatch):
    """Optimizer.step() on the small arena with every entry of librn_hip.so it calls recorded: norm ahead (clip, guard) ->
    control (one launch; none for plain momentum at a constant rate) -> update -> finalize (where the norm is formed beside the
    update), the same for every micro-step of an accumulation cycle.  Size queries launch nothing and are left out."""
    import _rn
    kw, steps, want = SEQUENCES[name]
    inp = ref.guard_case()
    _, arena, opt = _make(dev, inp, "momentum", **kw)
    assert (opt._control is None) == (CONTROL not in want)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    w_before = arena.weights.clone()
    calls, lib = [], _rn.lib()
    monkeypatch.setattr(_rn, "lib", lambda: _RecordingLib(lib, calls))
    for i in range(steps):
        _load_grad(arena, inp, inp.grads[i], dev)
        del calls[:]
        opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
        got = [c for c in calls if c not in ("rn_optimizer_norm_pairs", "rn_last_error")]
        assert got == want, (name, i, calls)
        assert got.count(CONTROL) <= 1 and got.count(UPDATE) == 1
        if CONTROL in got and NORM_AHEAD[0] in got:
            assert got.index(NORM_AHEAD[0]) < got.index(FINALIZE) < got.index(CONTROL) < got.index(UPDATE)
    torch.cuda.synchronize()
    assert opt.step_count == 1 and not torch.equal(arena.weights, w_before)
    if opt.skipped_dev is not None:
        assert opt.skipped_dev.tolist() == [0, 0] and opt.gate_dev.tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------- trainer
BASE = 1e-2
CLIP = 1.0
SIZE = 256


def _build(dev, use_graph, optimizer="adam", scheduled=True, ema=True, clip=CLIP, guard=True):
    """The recipe of test_gpu_clip_graph._build (MobileNetV2, 4 classes, dropout 0.2, focal loss) with the guard's keyword."""
    import layers, levels as levels_mod, retinanet, train
    lv = levels_mod.build_levels()
    layers.Dropout._next_seed[0] = 0x5EED
    torch.manual_seed(4)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    kw = {"lr_schedule": train.LRSchedule("step", BASE, warmup_steps=2, boundaries=(4,))} if scheduled else {}
    if ema:
        kw["ema_decay"] = 0.9
    if clip is not None:
        kw["grad_clip_norm"] = clip
    if guard:
        kw["skip_nonfinite"] = True
    tr = train.Trainer(net, lv, optimizer=optimizer, learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph, **kw)
    return net, tr


def _features(dev, image, boxes):
    import dataset, levels as levels_mod
    lv = levels_mod.build_levels()
    cids = torch.tensor([[1, 3]], dtype=torch.int32, device=dev)
    c, r, m = dataset.build_labels((SIZE, SIZE), cids, torch.tensor([boxes], device=dev), lv, 4, flip_pair=True)
    return {"image": image, "detection": {"classifications": c, "regressions": r}, "trainable_masks": m}


@pytest.fixture(scope="module")
def feats(dev):
    """good: the inputs of test_gpu_clip_graph.py (256 x 256, two boxes); pixel: the same with ONE pixel of the image NaN;
    flat: the same image with the second ground-truth box of zero height."""
    rng = np.random.default_rng(2)
    image = torch.from_numpy(rng.standard_normal((2, SIZE, SIZE, 3)).astype(np.float32)).to(dev)
    boxes = [[0.1, 0.2, 0.7, 0.8], [0.4, 0.1, 0.9, 0.5]]
    bad = image.clone()
    bad[0, 100, 37, 1] = float("nan")
    return {"good": _features(dev, image, boxes), "pixel": _features(dev, bad, boxes),
            "flat": _features(dev, image, [boxes[0], [0.4, 0.1, 0.4, 0.5]])}


def _state(tr):
    torch.cuda.synchronize()
    o = tr.opt
    return {"weights": tr.arena.weights.clone(), "state1": o.state1.clone(), "state2": o.state2.clone() if o.state2 is not None else None,
            "ema": o.ema.clone() if o.ema is not None else None, "norm_reg": o.norm_reg.clone(),
            "step_dev": o.step_dev.clone() if o.step_dev is not None else None, "lr_dev": o.lr_dev.clone() if o.lr_dev is not None else None,
            "ema_updates_dev": o.ema_updates_dev.clone() if o.ema_updates_dev is not None else None}


def _tensor_bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _equal_states(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert _tensor_bits_equal(a[k], b[k]), (what, k)


ORDER = ("good", "pixel", "good", "good")


@pytest.fixture(scope="module")
def guarded_run(dev, feats, tmp_path_factory):
    """Scheduled Adam with ema_decay 0.9, clipping and the guard, the one-graph step: good, poisoned (NaN pixel), good, good;
    the state after every step and a checkpoint written after the third."""
    import checkpoint
    net, tr = _build(dev, True)
    path = str(tmp_path_factory.mktemp("guard") / "model.safetensors")
    states, counts = [_state(tr)], []
    for i, name in enumerate(ORDER):
        tr.step(feats[name])
        states.append(_state(tr))
        if i == 2:
            assert tr.opt.step_count == 3                                # (not reconciled yet: ahead by the skip)
            checkpoint.save(path, net, tr, step=3)
            counts.append(tr.opt.step_count)
    return {"trainer": tr, "states": states, "checkpoint": path, "count_at_save": counts[0]}


def test_trainer_skips_the_poisoned_step_in_one_graph(dev, feats, guarded_run):
    """One NaN pixel (the value only flows through arithmetic: no kernel of the step indexes memory by an activation, and the
    labels are built from the boxes beforehand) makes the whole gradient non-finite.  With the guard the four steps are one graph,
    the poisoned one leaves weights, slots, average and the device words bit-identical, the final weights are finite, and after
    the reconcile step_count is 3.  The same four steps without the guard end with non-finite weights."""
    import ops
    tr, s = guarded_run["trainer"], guarded_run["states"]
    assert tr._graphs[5] and len(tr._graph_cache) == 1 and tr.recaptures == 0
    _equal_states(s[2], s[1], "the poisoned step", skip=("norm_reg",))
    assert not torch.isfinite(s[2]["norm_reg"][0]) and torch.isfinite(s[1]["norm_reg"][0]) and torch.isfinite(s[3]["norm_reg"][0])
    for i in (1, 3, 4):
        assert not torch.equal(s[i]["weights"], s[i - 1]["weights"]), i
    assert [int(x["step_dev"].item()) for x in s] == [0, 1, 1, 2, 3] == [int(x["ema_updates_dev"].item()) for x in s]
    for k in ("weights", "state1", "state2", "ema"):
        assert torch.isfinite(s[-1][k]).all(), k
    assert guarded_run["count_at_save"] == 2                              # checkpoint.save reconciled: 3 steps, 1 skipped
    assert tr.skipped_updates() == (1, 0) and tr.opt.step_count == 3
    assert tr.drop_counter.item() == 4 * ops.DROPOUT_COUNTER_STEP
    _, tn = _build(dev, True, guard=False)
    for name in ORDER:
        tn.step(feats[name])
    torch.cuda.synchronize()
    assert tn._graphs[5] and not torch.isfinite(tn.arena.weights).all() and not torch.isfinite(tn.opt.ema).all()
    assert tn.skipped_updates() == (0, 0) and tn.opt.step_count == 4


def test_guarded_graph_equals_eager_and_the_guard_off(dev, feats):
    """Three finite steps with the guard: the one-graph trainer against eager launches, bit-identical states after every step --
    and against the one-graph trainer WITHOUT the guard: the same weights, slots and average (clipped: the same norm pass)."""
    _, tg = _build(dev, True)
    _, te = _build(dev, False)
    _, tn = _build(dev, True, guard=False)
    for i in range(3):
        tg.step(feats["good"]), te.step(feats["good"]), tn.step(feats["good"])
        a, b, c = _state(tg), _state(te), _state(tn)
        _equal_states(a, b, "graph against eager, step %d" % (i + 1))
        _equal_states(a, c, "guard on against guard off, step %d" % (i + 1))
    assert tg._graphs[5] and tn._graphs[5] and tg.recaptures == 0 and tg.skipped_updates() == (0, 0) == te.skipped_updates()
    assert tg.opt.step_count == 3 == te.opt.step_count


def test_a_zero_height_box_is_skipped_too(dev, feats):
    """The poison real data brings: a ground-truth box of zero height gives NaN regression targets (csrc/assign.hip), the loss
    multiplies them through, and norm_reg[0] of that step is not finite at this shape -- asserted first, on a trainer without the
    guard, whose weights it destroys.  With the guard (eager, momentum at a constant rate, unclipped: the other end of the
    configurations) the step is skipped and the next one applies."""
    assert torch.isnan(torch.cat([v.reshape(-1) for v in feats["flat"]["detection"]["regressions"].values()])).any()
    _, tn = _build(dev, False, "momentum", scheduled=False, ema=False, clip=None, guard=False)
    tn.step(feats["flat"])
    torch.cuda.synchronize()
    assert not torch.isfinite(tn.opt.norm_reg[0]) and not torch.isfinite(tn.arena.weights).all()
    _, tg = _build(dev, False, "momentum", scheduled=False, ema=False, clip=None, guard=True)
    assert tg.opt.lr_dev is None
    s0 = _state(tg)
    tg.step(feats["flat"])
    s1 = _state(tg)
    _equal_states(s1, s0, "the flat box", skip=("norm_reg",))
    assert not torch.isfinite(s1["norm_reg"][0])
    # --nonfinite-limit, as the training loop checks it at a log line: one skipped update in a row so far
    import _rn
    import train
    assert train.check_nonfinite_limit(tg, None) == 1 == train.check_nonfinite_limit(tg, 2) and tg.opt.step_count == 0
    with pytest.raises(_rn.RnError, match="--nonfinite-limit 1: the last 1 updates in a row were skipped"):
        train.check_nonfinite_limit(tg, 1)
    tg.step(feats["good"])
    torch.cuda.synchronize()
    assert torch.isfinite(tg.arena.weights).all() and not torch.equal(tg.arena.weights, s0["weights"])
    assert tg.skipped_updates() == (1, 0) and tg.opt.step_count == 1


def test_resume_continues_the_guarded_run(dev, feats, guarded_run):
    """The checkpoint written after good, poisoned, good, loaded into a fresh guarded trainer: the fourth step reproduces the
    uninterrupted run bit for bit, the skip count is back, and the scheduled rate is that of update 3."""
    import checkpoint
    from safetensors import safe_open
    with safe_open(guarded_run["checkpoint"], framework="pt") as f:
        meta = f.metadata()
    assert meta["format"] == "retinanet-amd-v2" and meta["nonfinite_skipped"] == "1" and meta["step_count"] == "2" and meta["step"] == "3"
    net, tr = _build(dev, True)
    assert checkpoint.load(guarded_run["checkpoint"], net, tr) == 3
    assert tr.opt.step_count == 2 == tr.opt.step_dev.item() == tr.opt.ema_updates_dev.item()
    assert tr.skipped_updates() == (1, 0) and tr.opt.step_count == 2
    tr.step(feats["good"])
    got, want = _state(tr), guarded_run["states"][4]
    assert tr._graphs[5] and len(tr._graph_cache) == 1
    assert tr.skipped_updates()[0] == 1 and tr.opt.step_count == 3 == tr.opt.step_dev.item()
    for k in ("weights", "ema", "lr_dev", "step_dev", "ema_updates_dev"):
        assert _tensor_bits_equal(got[k], want[k]), k
    for off, size in tr.arena.offsets:             # (a checkpoint holds the slots per parameter: compared there, not on the padding)
        for k in ("state1", "state2"):
            assert torch.equal(got[k][off:off + size], want[k][off:off + size]), (k, off)
    assert lr_schedule_ref.ulp_distance(tr.opt.lr_dev[0].item(), tr.opt.schedule.value(2)) <= 1     # the third update's rate ...
    assert tr.opt.current_lr() == float(tr.opt.schedule.value(3))                                     # ... and update 3 comes next
    # a trainer without the guard ignores the key; a file without it loads as 0
    net2, t2 = _build(dev, False, guard=False)
    assert checkpoint.load(guarded_run["checkpoint"], net2, t2) == 3 and t2.opt.step_count == 2 and t2.skipped_updates() == (0, 0)
    plain = guarded_run["checkpoint"] + ".plain"
    checkpoint.save(plain, net2, t2, step=3)
    tr.opt.set_skipped(5)
    assert checkpoint.load(plain, net, tr) == 3 and tr.skipped_updates() == (0, 0) and tr.opt.step_count == 2


def test_cli_guarded_run_is_one_graph(tmp_path, capsys):
    import train
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "6", "--scale", "128", "--experiment", str(tmp_path / "exp"),
            "--backbone", "mobilenet_v2", "--dropout", "0.1", "--optimizer", "adam", "--skip-nonfinite", "--nonfinite-limit", "3",
            "--lr-schedule", "cosine", "--lr-warmup-steps", "2"]
    assert train.main(argv) == 6
    assert train.LAST_RUN["graph_sets"] == 1 and train.LAST_RUN["recaptures"] == 0
    assert train.LAST_RUN["updates"] + train.LAST_RUN["skipped"] == 6 and train.LAST_RUN["skipped"] == 0
    with pytest.raises(SystemExit):
        train.main(["--dataset", "shapes", "--accumulate-steps", "2", "--skip-nonfinite"])
    assert "--skip-nonfinite" in capsys.readouterr().err
