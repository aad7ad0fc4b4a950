"""Global-norm clipping inside the one-graph training step, on the MI355X (-m gpu): the clipped update that reads norm, rate and
decay from the device (rn_grad_norm_partial + rn_norm_reg_finalize + rn_optimizer_update under RN_OPT_F_CLIP) against the float64 reference
(clip_ref.py), a loose clip against the unclipped fused path bit for bit, the slice entry of the norm pass, Optimizer.step()
captured and replayed by itself, and a clipped trainer's ONE captured graph against eager launches, against one graph per part,
the reference, a checkpoint and the command line.

TOL = 1e-4, element-wise, is the bar test_gpu_step_tail.py and test_gpu_accum.py hold this arithmetic to over three updates;
everything that is not a comparison with float64 is bit equality."""
import collections
import functools

import numpy as np
import pytest
import torch

import clip_ref as ref
import ema_ref
import lr_schedule_ref
import step_tail_ref
from helpers import assert_close, elementwise_rel_err

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
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the optimizer alone
Got = collections.namedtuple("Got", "w state1 state2 norm_reg e")


def _snapshot(arena, opt):
    torch.cuda.synchronize()
    return Got(arena.weights.cpu().numpy(), opt.state1.cpu().numpy(), opt.state2.cpu().numpy() if opt.state2 is not None else None,
               opt.norm_reg.cpu().numpy(), opt.ema.cpu().numpy() if opt.ema is not None else None)


def _make(dev, inp, kind, clip=None, scheduled=False, setting=None):
    """A synthetic module laid out as `inp` (test_gpu_accum._run) and its optimizer."""
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
    if scheduled:
        kw.update(schedule=train.LRSchedule(base_lr=inp.lr, **ref.SCHEDULE))
    return mod, arena, train.Optimizer(arena, kind, inp.lr, grad_clip_norm=clip, **kw)


def _load_grad(arena, inp, g, dev):
    for p, off, s in zip(arena.params, inp.offsets, inp.sizes):
        p.grad.copy_(torch.from_numpy(np.asarray(g[off:off + s], np.float32)).to(dev))


def _run(dev, inp, kind, clip=None, scheduled=False, setting=None):
    """Every gradient of `inp` as one opt.step().  Returns the state before the first update and after each."""
    _, arena, opt = _make(dev, inp, kind, clip, scheduled, setting)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out = [_snapshot(arena, opt)]
    for u, g in enumerate(inp.grads):
        _load_grad(arena, inp, g, dev)
        opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
        out.append(_snapshot(arena, opt))
        assert opt.step_count == u + 1
        if scheduled:
            assert opt.step_dev.item() == u + 1 and opt.current_lr() == float(opt.schedule.value(u + 1))
            assert lr_schedule_ref.ulp_distance(opt.lr_dev[0].item(), opt.schedule.value(u)) <= 1
        if setting is not None:
            assert opt.ema_updates_dev.item() == u + 1
    import ops
    assert counter.item() == len(inp.grads) * ops.DROPOUT_COUNTER_STEP
    return out


@functools.lru_cache(maxsize=None)
def _want(name, kind, clip, scheduled, setting):
    inp = ref.clip_case(name)
    return ref.clip_ref(inp, kind, clip, ref.rates(inp) if scheduled else None, setting)


def _check(inp, kind, got, want, tag):
    pad = step_tail_ref.padding_mask(inp)
    assert _same_bits(got[0].w, inp.w0) and not got[0].norm_reg.any()
    for u, st in enumerate(want.steps):
        a, what = got[u + 1], "%s update %d" % (tag, u + 1)
        _close(a.w, st.w, what + " weights")
        _close(a.state1, st.state1, what + " state1")
        if kind != "momentum":
            _close(a.state2, st.state2, what + " state2")
        _close(float(a.norm_reg[0]) ** 0.5, st.norm, what + " global norm")
        _close(float(a.norm_reg[1]), st.reg, what + " regulariser")
        if want.e is not None:
            _close(a.e, want.e[u], what + " average")
            assert not _bits(a.e[pad]).any()
        assert not a.w[pad].any()


@pytest.mark.parametrize("setting", [None, SETTING], ids=["no-average", "average"])
@pytest.mark.parametrize("scheduled", [False, True], ids=["constant", "scheduled"])
@pytest.mark.parametrize("clip", [ref.CLIP_BINDS, ref.CLIP_LOOSE], ids=["binds", "loose"])
@pytest.mark.parametrize("kind", KINDS)
def test_small_arena_against_the_reference(dev, kind, clip, scheduled, setting):
    """Parameters of 1152, 700, 1, 1025 and 3000 elements (9 blocks), three updates: w, the slots, the average and norm_reg (the
    norm and the regulariser at the weights before the update) against float64.  Scheduled: rates base / 3, 2 base / 3, base read
    from the device, Adam's bias correction with them."""
    inp = ref.clip_case("small")
    got = _run(dev, inp, kind, clip, scheduled, setting)
    _check(inp, kind, got, _want("small", kind, clip, scheduled, setting), "small %s clip %g" % (kind, clip))
    if clip == ref.CLIP_BINDS:
        # the clip does bind: the first slot is far from an unclipped update's
        free = _want("small", kind, None, scheduled, None).steps[0].state1
        assert elementwise_rel_err(got[1].state1, free) > 10 * TOL


@pytest.mark.parametrize("setting", [None, SETTING], ids=["no-average", "average"])
@pytest.mark.parametrize("scheduled", [False, True], ids=["constant", "scheduled"])
@pytest.mark.parametrize("kind", KINDS)
def test_loose_clip_equals_the_unclipped_fused_path(dev, kind, scheduled, setting):
    """clip / max(norm, clip) is exactly 1 under CLIP_LOOSE: w, the slots and the average equal, bit for bit, what the unclipped
    path (RN_OPT_F_NORM, the norm formed beside the update) leaves; norm_reg, summed in another order by
    another kernel, agrees within TOL."""
    inp = ref.clip_case("small")
    loose = _run(dev, inp, kind, ref.CLIP_LOOSE, scheduled, setting)
    plain = _run(dev, inp, kind, None, scheduled, setting)
    for u, (a, b) in enumerate(zip(loose, plain)):
        assert _same_bits(a.w, b.w) and _same_bits(a.state1, b.state1) and _same_bits(a.state2, b.state2) and _same_bits(a.e, b.e), u
        if u:
            _close(a.norm_reg, b.norm_reg, "norm_reg, clipped path against fused path, update %d" % u)
    assert not _same_bits(loose[-1].w, loose[0].w)


def test_large_arena(dev):
    """One parameter of 2097152 + 5 * 1024 + 7 elements, then three small ones, the last of 37 elements: the 2048-block grid cap
    binds in the norm pass and in the update, part of each grid goes round again, and the arena ends off a block boundary."""
    inp = ref.clip_case("large")
    import _rn
    assert int(_rn.lib().rn_optimizer_norm_pairs(inp.count)) == 2048 and inp.count // 4 > 2048 * 256
    assert (inp.offsets[-1] + inp.sizes[-1]) % step_tail_ref.OPT_BLOCK != 0
    _check(inp, "momentum", _run(dev, inp, "momentum", ref.CLIP_BINDS), _want("large", "momentum", ref.CLIP_BINDS, False, None),
           "large momentum clip binds")


def test_norm_pass_in_slices(dev):
    """rn_grad_norm_partial called directly on the small arena: three slices at block offsets 0, 2 and 4 (SMALL_SLICES), each with
    its own wd_per_block pointer, their pairs laid end to end and finalised once -- against the float64 norm and regulariser,
    and against the one-slice call."""
    import _rn
    L = _rn.lib()
    inp = ref.clip_case("small")
    _, arena, _ = _make(dev, inp, "momentum")
    _load_grad(arena, inp, inp.grads[0], dev)
    B = step_tail_ref.OPT_BLOCK

    def run(slices):
        total = sum(int(L.rn_optimizer_norm_pairs(hi - lo)) for lo, hi in slices)
        partial = torch.full((2 * total + 8,), float("nan"), dtype=torch.float64, device=dev)    # (NaN: an unwritten pair shows)
        out2 = torch.zeros(2, dtype=torch.float32, device=dev)
        at = 0
        for lo, hi in slices:
            assert 0 <= lo < hi <= arena.count and lo % B == 0 and hi % B == 0          # the kernel reads [lo, hi) only
            n = int(L.rn_optimizer_norm_pairs(hi - lo))
            _rn.check(L.rn_grad_norm_partial(arena.weights[lo:].data_ptr(), arena.grads[lo:].data_ptr(),
                                             arena.wd_per_block[lo // B:].data_ptr(), hi - lo, inp.grad_scale,
                                             partial[2 * at:].data_ptr(), _rn.stream()), "rn_grad_norm_partial")
            at += n
        assert at == total
        _rn.check(L.rn_norm_reg_finalize(partial.data_ptr(), total, _rn.f32(out2), _rn.stream()), "rn_norm_reg_finalize")
        torch.cuda.synchronize()
        assert torch.isnan(partial[2 * total:]).all() and not torch.isnan(partial[:2 * total]).any()
        return out2.cpu().numpy(), partial[:2 * total].cpu().numpy()

    sliced, pairs = run(step_tail_ref.SMALL_SLICES)
    whole, _ = run(((0, inp.count),))
    n2, reg = ref.norm_and_reg(inp, inp.grads[0])
    _close(float(sliced[0]), n2, "sum g'^2 in three slices")
    _close(float(sliced[1]), reg, "regulariser in three slices")
    _close(sliced, whole, "three slices against one")
    # the pairs of each slice are that slice's own share
    at = 0
    for lo, hi in step_tail_ref.SMALL_SLICES:
        n = int(L.rn_optimizer_norm_pairs(hi - lo))
        want = ref.norm_and_reg(inp, inp.grads[0], lo=lo, hi=hi)
        _close(pairs[2 * at:2 * (at + n)].reshape(-1, 2).sum(0), np.asarray(want), "pairs of slice [%d, %d)" % (lo, hi))
        at += n


def test_step_captured_and_replayed_equals_eager(dev):
    """opt.step() -- scheduled Adam, the average, CLIP_BINDS -- captured into a graph by itself and replayed three times with the
    next gradient copied into arena.grads before each replay, against three eager calls: bit-identical w, slots, average and
    norm_reg; the step word, the average's word and the dropout counter end at 3, 3 and 3 * DROPOUT_COUNTER_STEP.  Rate, bias
    correction and decay differ at every update: a host scalar baked into the graph would show at the second."""
    import ops
    inp = ref.clip_case("small")
    eager = _run(dev, inp, "adam", ref.CLIP_BINDS, True, SETTING)
    _, arena, opt = _make(dev, inp, "adam", ref.CLIP_BINDS, True, SETTING)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    w_before = arena.weights.clone()
    _load_grad(arena, inp, inp.grads[0], dev)
    # (no warm-up call: step() allocates nothing, and the eager run above has launched every kernel of it once already)
    g = torch.cuda.CUDAGraph()
    count = opt.step_count
    with torch.cuda.graph(g):
        opt.step(grad_scale=inp.grad_scale, advance_counter=counter)
    opt.step_count = count                                                         # (recorded, not run)
    torch.cuda.synchronize()
    assert torch.equal(arena.weights, w_before) and opt.step_dev.item() == 0 and counter.item() == 0
    for u, grad in enumerate(inp.grads):
        _load_grad(arena, inp, grad, dev)
        g.replay()
        opt.count_step()
        got = _snapshot(arena, opt)
        for x, y in zip(got, eager[u + 1]):
            assert _same_bits(x, y), u
    assert opt.step_dev.item() == 3 == opt.ema_updates_dev.item() == opt.step_count
    assert counter.item() == 3 * ops.DROPOUT_COUNTER_STEP
    r = opt.lr_dev.cpu().numpy()
    assert lr_schedule_ref.ulp_distance(r[1], lr_schedule_ref.adam_rate(r[0], 2)) <= 1 and r[1] != r[0]


# ---------------------------------------------------------------------------------------------- trainer
BASE = 1e-2
STEPS = 3
CLIP = 1.0


def _build(dev, use_graph, optimizer="momentum", scheduled=False, ema=False, clip=CLIP, whole=True):
    """The recipe of test_gpu_accum._build: MobileNetV2, 4 classes, dropout 0.2, focal loss."""
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
    tr = train.Trainer(net, lv, optimizer=optimizer, learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph, **kw)
    if not whole:
        tr.whole_step_graph = False            # (RN_WHOLE_STEP_GRAPH=0: one graph per part, the same Optimizer.step() launched eagerly)
    return net, tr


@pytest.fixture(scope="module")
def feats(dev):
    """The inputs of test_gpu_accum.py (256 x 256, two boxes)."""
    import dataset, levels as levels_mod
    lv = levels_mod.build_levels()
    rng = np.random.default_rng(2)
    size = 256
    image = torch.from_numpy(rng.standard_normal((2, size, size, 3)).astype(np.float32)).to(dev)
    boxes = torch.tensor([[[0.1, 0.2, 0.7, 0.8], [0.4, 0.1, 0.9, 0.5]]], device=dev)
    cids = torch.tensor([[1, 3]], dtype=torch.int32, device=dev)
    c, r, m = dataset.build_labels((size, size), cids, boxes, lv, 4, flip_pair=True)
    return {"image": image, "detection": {"classifications": c, "regressions": r}, "trainable_masks": m}


def _state(tr):
    torch.cuda.synchronize()
    return {"weights": tr.arena.weights.clone(), "state1": tr.opt.state1.clone(),
            "state2": tr.opt.state2.clone() if tr.opt.state2 is not None else None,
            "ema": tr.opt.ema.clone() if tr.opt.ema is not None else None, "norm_reg": tr.opt.norm_reg.clone()}


def _equal_states(a, b, what):
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (what, k)


def _steps(tr, feats, n=STEPS, grads=None):
    states = [_state(tr)]
    for i in range(n):
        tr.step(feats)
        states.append(_state(tr))
        if grads is not None and i == 0:
            grads.append(tr.arena.grads.cpu().numpy().copy())
    return states


@pytest.fixture(scope="module")
def momentum_eager(dev, feats):
    """Momentum at a constant rate, clipped, launched eagerly: the state after each step and the first step's device gradient."""
    grads = []
    _, te = _build(dev, False)
    return {"trainer": te, "states": _steps(te, feats, grads=grads), "grad": grads[0]}


def test_clipped_momentum_step_is_one_graph(dev, feats, momentum_eager):
    """grad_clip_norm with momentum at a constant rate: the step is ONE captured graph, captured once -- and after every step the
    weights and the momentum equal, bit for bit, the eager trainer's and the one-graph-per-part trainer's."""
    import ops
    _, tw = _build(dev, True)
    got = _steps(tw, feats)
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    _, tp = _build(dev, True, whole=False)
    parts = _steps(tp, feats)
    assert not tp._graphs[5] and len(tp._graph_cache) == 1 and tp.recaptures == 0
    for i, (a, b, c) in enumerate(zip(got, momentum_eager["states"], parts)):
        _equal_states(a, b, "graph against eager, step %d" % i)
        _equal_states(a, c, "one graph against one graph per part, step %d" % i)
    assert not torch.equal(got[-1]["weights"], got[0]["weights"])
    assert tw.opt.step_count == STEPS == tp.opt.step_count
    assert tw.drop_counter.item() == tp.drop_counter.item() == momentum_eager["trainer"].drop_counter.item() == STEPS * ops.DROPOUT_COUNTER_STEP


@pytest.fixture(scope="module")
def adam_run(dev, feats, tmp_path_factory):
    """Scheduled Adam with ema_decay 0.9 and clipping, the one-graph step, three steps, a checkpoint written after the second."""
    import checkpoint
    net, tw = _build(dev, True, "adam", scheduled=True, ema=True)
    path = str(tmp_path_factory.mktemp("clip") / "model.safetensors")
    states = [_state(tw)]
    for i in range(STEPS):
        tw.step(feats)
        states.append(_state(tw))
        if i == 1:
            checkpoint.save(path, net, tw, step=2)
    return {"trainer": tw, "states": states, "checkpoint": path}


def test_clipped_scheduled_adam_with_average_is_one_graph(dev, feats, adam_run):
    """Rate, bias correction, decay and clip scale all change from step to step, and the step stays one graph: weights, both slots
    and the average bit-identical to eager launches and to one graph per part after every step."""
    tw = adam_run["trainer"]
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    _, te = _build(dev, False, "adam", scheduled=True, ema=True)
    eager = _steps(te, feats)
    _, tp = _build(dev, True, "adam", scheduled=True, ema=True, whole=False)
    parts = _steps(tp, feats)
    assert not tp._graphs[5]
    for i, (a, b, c) in enumerate(zip(adam_run["states"], eager, parts)):
        _equal_states(a, b, "graph against eager, step %d" % i)
        _equal_states(a, c, "one graph against one graph per part, step %d" % i)
    assert tw.opt.step_dev.item() == tw.opt.ema_updates_dev.item() == STEPS == te.opt.step_dev.item() == tw.opt.step_count
    assert torch.equal(tw.opt.lr_dev, te.opt.lr_dev) and torch.equal(tw.opt.ema_dev, te.opt.ema_dev)
    r = tw.opt.lr_dev.cpu().numpy()
    assert lr_schedule_ref.ulp_distance(r[0], tw.opt.schedule.value(2)) <= 1
    assert lr_schedule_ref.ulp_distance(r[1], lr_schedule_ref.adam_rate(r[0], 2)) <= 1
    s = adam_run["states"]
    assert not torch.equal(s[-1]["weights"], s[0]["weights"]) and not torch.equal(s[-1]["ema"], s[-1]["weights"])


def test_first_update_matches_the_reference(dev, momentum_eager):
    """The first update from the eager run's device gradient and the initial weights, in float64.  The norm of g' there was
    observed as 5.76 on this recipe, above CLIP = 1.0 (asserted below from the reference): the clip binds, and the momentum slot
    is far from an unclipped update's."""
    te = momentum_eager["trainer"]
    w0 = momentum_eager["states"][0]["weights"].cpu().numpy()
    wd = te.arena.wd_per_block.repeat_interleave(step_tail_ref.OPT_BLOCK).cpu().numpy()
    inp = step_tail_ref.OptInputs((), (), (), te.arena.count, w0, (momentum_eager["grad"],), wd, 1.0, BASE)
    want = ref.optimizer_steps(inp, "momentum", CLIP)[0]
    print("trainer recipe: global norm of g' at the first update %.6g (clip %g)" % (want.norm, CLIP))
    assert want.norm > CLIP, "the clip %g does not bind at the first update: the norm is %g" % (CLIP, want.norm)
    after = momentum_eager["states"][1]
    _close(after["weights"].cpu().numpy(), want.w, "trainer weights after update 1")
    _close(after["state1"].cpu().numpy(), want.state1, "trainer momentum after update 1")
    _close(float(after["norm_reg"][0]) ** 0.5, want.norm, "trainer global norm at update 1")
    _close(float(after["norm_reg"][1]), want.reg, "trainer regulariser at update 1")
    free = ref.optimizer_steps(inp, "momentum", None)[0]
    assert elementwise_rel_err(after["state1"].cpu().numpy(), free.state1) > 10 * TOL


def test_loose_clip_equals_a_trainer_without_clipping(dev, feats):
    """grad_clip_norm=1e6: the clip scale is exactly 1 and the weights are those of a trainer built without clipping, bit for
    bit; both run one graph."""
    _, tl = _build(dev, True, clip=1e6)
    _, tn = _build(dev, True, clip=None)
    for _ in range(STEPS):
        tl.step(feats), tn.step(feats)
    torch.cuda.synchronize()
    assert tl._graphs[5] and tn._graphs[5] and len(tl._graph_cache) == 1 == len(tn._graph_cache)
    assert tl.recaptures == 0 == tn.recaptures and tl.opt.clip == 1e6 and tn.opt.clip == 0.0
    assert torch.equal(tl.arena.weights, tn.arena.weights) and torch.equal(tl.opt.state1, tn.opt.state1)
    assert_close(tl.opt.norm_reg.cpu().numpy(), tn.opt.norm_reg.cpu().numpy(), TOL, "norm_reg, clipped against fused", elementwise_tol=TOL)


def test_resume_continues_the_clipped_scheduled_run(dev, feats, adam_run):
    """The checkpoint written after step 2, loaded into a fresh trainer: step 3 reproduces the uninterrupted run's state bit for
    bit, in one graph."""
    import checkpoint
    net, tr = _build(dev, True, "adam", scheduled=True, ema=True)
    assert checkpoint.load(adam_run["checkpoint"], net, tr) == 2
    assert tr.opt.step_count == 2 and tr.opt.step_dev.item() == 2 and tr.opt.ema_updates_dev.item() == 2
    tr.step(feats)
    got, want = _state(tr), adam_run["states"][STEPS]
    assert tr._graphs[5] and len(tr._graph_cache) == 1 and tr.opt.step_count == 3 == tr.opt.step_dev.item()
    for k in ("weights", "ema"):
        assert torch.equal(got[k], want[k]), k
    # (a checkpoint holds the slots per parameter: compared there, not on the arena's padding)
    for off, size in tr.arena.offsets:
        for k in ("state1", "state2"):
            assert torch.equal(got[k][off:off + size], want[k][off:off + size]), (k, off)


def test_cli_clipped_scheduled_run_is_one_graph(tmp_path, capsys):
    import train
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "6", "--scale", "128", "--experiment", str(tmp_path / "exp"),
            "--backbone", "mobilenet_v2", "--dropout", "0.1", "--grad-clip-norm", "1.0", "--lr-schedule", "cosine",
            "--lr-warmup-steps", "2", "--ema-decay", "0.9"]
    assert train.main(argv) == 6
    assert train.LAST_RUN["graph_sets"] == 1 and train.LAST_RUN["recaptures"] == 0 and train.LAST_RUN["updates"] == 6
