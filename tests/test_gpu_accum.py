"""Gradient accumulation on the MI355X (-m gpu): rn_step_control_eval's phase and what runs behind its gate, the accumulating update
kernel against the float64 reference (accum_ref.py) and, bit for bit, against a plain update on exact means, an accumulating
trainer's ONE captured graph against eager launches, the reference and a checkpoint taken in the middle of a cycle, and the command
line."""
import collections
import os

import numpy as np
import pytest
import torch

import accum_ref as ref
import ema_ref
import lr_schedule_ref
import step_tail_ref
from helpers import assert_close, elementwise_rel_err, step_control

pytestmark = pytest.mark.gpu
TOL = 1e-4          # (test_gpu_ema.TOL: max-norm and element-wise, through assert_close)
KINDS = ("momentum", "rmsprop", "adam")


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


# ------------------------------------------------------------------------------------------------ the one-thread kernels
def test_phase_kernel_and_gates(dev):
    """A = 3, 7 launches of the control kernel (ACCUM | LR | EMA): accum_dev = [m % 3, m % 3 == 2] and the micro-step word exact after each;
    the gated schedule (Adam: with the bias correction) and average kernels act on launches 3 and 6 only -- there within 1 ulp of
    the float64 formulas, words advanced -- and leave lr_dev / ema_dev bit-unchanged, words untouched, on the others."""
    import _rn, train
    A = 3
    sched = train.LRSchedule("cosine", 1e-2, warmup_steps=1, total_steps=5, final_factor=0.05)
    kw = dict(kind="cosine", base=1e-2, warmup_steps=1, total_steps=5, final_factor=0.05)
    d = sched.struct()
    micro = torch.zeros(1, dtype=torch.int64, device=dev)
    pair = torch.full((2,), -7, dtype=torch.int32, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    upd_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    lr_dev = torch.tensor([7.0, 9.0], dtype=torch.float32, device=dev)            # (sentinels: a closed gate leaves them)
    ema_dev = torch.tensor([5.0, 3.0], dtype=torch.float32, device=dev)
    prev_lr, prev_ema, u = lr_dev.cpu().numpy(), ema_dev.cpu().numpy(), 0
    lr_ema = dict(optimizer_kind=_rn.OPT["adam"], schedule=d, step_dev=step_dev.data_ptr(), lr_dev=_rn.f32(lr_dev),
                  ema_decay=0.22, ema_warmup=1, ema_updates_dev=upd_dev.data_ptr(), ema_dev=_rn.f32(ema_dev))
    for m in range(7):
        _rn.check(step_control(_rn.stream(), features=_rn.CTL_F_ACCUM | _rn.CTL_F_LR | _rn.CTL_F_EMA, accumulate_steps=A,
                               micro_dev=micro.data_ptr(), accum_dev=pair.data_ptr(), **lr_ema), "rn_step_control_eval")
        assert pair.cpu().tolist() == [m % A, int(m % A == A - 1)] and int(micro.item()) == m + 1
        got_lr, got_ema = lr_dev.cpu().numpy(), ema_dev.cpu().numpy()
        if m % A == A - 1:
            assert lr_schedule_ref.ulp_distance(got_lr[0], sched.value(u)) <= 1
            assert lr_schedule_ref.ulp_distance(got_lr[0], lr_schedule_ref.lr_value(u, **kw)) <= 1
            assert lr_schedule_ref.ulp_distance(got_lr[1], lr_schedule_ref.adam_rate(got_lr[0], u)) <= 1 and got_lr[1] != got_lr[0]
            dd, om = ema_ref.decay_pair(u, 0.22, True)
            assert lr_schedule_ref.ulp_distance(got_ema[0], dd) <= 1 and lr_schedule_ref.ulp_distance(got_ema[1], om) <= 1
            u += 1
        else:
            assert _same_bits(got_lr, prev_lr) and _same_bits(got_ema, prev_ema)
        assert int(step_dev.item()) == u == int(upd_dev.item())
        prev_lr, prev_ema = got_lr, got_ema
    assert u == 2 and prev_lr[0] != 7.0 and prev_ema[0] != 5.0
    # LR | EMA without ACCUM / GUARD has no gate: it acts on every launch (micro-step 7 is phase 1: the gated launch would not)
    _rn.check(step_control(_rn.stream(), features=_rn.CTL_F_LR | _rn.CTL_F_EMA, **lr_ema), "rn_step_control_eval")
    assert int(step_dev.item()) == 3 == int(upd_dev.item())
    assert lr_schedule_ref.ulp_distance(lr_dev[0].item(), sched.value(2)) <= 1


# ------------------------------------------------------------------------------------------------ the sum on an arena
Got = collections.namedtuple("Got", "w state1 state2 norm_reg e acc")
SCHEDULE = dict(kind="step", warmup_steps=1, boundaries=(1,))            # update 0: LR / 3 (warm-up), update 1: LR / 10


def _rates(n):
    return [float(lr_schedule_ref.lr_value(s, base=ref.LR, **SCHEDULE)) for s in range(n)]


def _snapshot(arena, opt):
    torch.cuda.synchronize()
    return Got(arena.weights.cpu().numpy(), opt.state1.cpu().numpy(), opt.state2.cpu().numpy() if opt.state2 is not None else None,
               opt.norm_reg.cpu().numpy(), opt.ema.cpu().numpy() if opt.ema is not None else None,
               opt.acc.cpu().numpy() if opt.acc is not None else None)


def _run(dev, inp, kind, A, setting=None, scheduled=False, slices=None):
    """Every gradient of `inp` as one micro-step on a synthetic module laid out as `inp` (test_gpu_ema._run).  Returns the state
    before the first micro-step and after each.  `slices`: begin_step / step_slice / finish_step, the LAST slice on a side stream."""
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
        kw.update(schedule=train.LRSchedule(base_lr=inp.lr, **SCHEDULE))
    opt = train.Optimizer(arena, kind, inp.lr, accumulate_steps=A, **kw)
    if A > 1:
        assert opt.acc.shape == arena.weights.shape and not opt.acc.any() and opt.acc.data_ptr() % 16 == 0
        assert opt.micro_dev.item() == 0 and opt.accum_dev.dtype == torch.int32 and opt.accum_dev.shape == (2,)
    else:
        assert opt.acc is None and opt.micro_dev is None and opt.accum_dev is None
    side = torch.cuda.Stream()
    out = [_snapshot(arena, opt)]
    for m, g in enumerate(inp.grads):
        for p, off, s in zip(arena.params, inp.offsets, inp.sizes):
            p.grad.copy_(torch.from_numpy(np.asarray(g[off:off + s], np.float32)).to(dev))
        if slices is None:
            opt.step(grad_scale=inp.grad_scale)
        else:
            side.wait_stream(torch.cuda.current_stream())          # (the gradients were copied on the main stream)
            opt.begin_step()
            for i, (lo, hi) in enumerate(slices):
                opt.step_slice(lo, hi, inp.grad_scale, stream=side if i == len(slices) - 1 else None)
            torch.cuda.current_stream().wait_stream(side)
            opt.finish_step()
        out.append(_snapshot(arena, opt))
        u = (m + 1) // A
        assert opt.step_count == u
        if A > 1:
            assert opt.micro_dev.item() == m + 1 and opt.accum_dev.cpu().tolist() == [m % A, int(m % A == A - 1)]
        if setting is not None:
            assert opt.ema_updates_dev.item() == u
        if scheduled:
            assert opt.step_dev.item() == u and opt.current_lr() == float(opt.schedule.value(u))
    return out


def _check(inp, kind, A, got, want, tag):
    """got[0] is the initial state, got[m + 1] the state after micro-step m."""
    pad = step_tail_ref.padding_mask(inp)
    assert _same_bits(got[0].w, inp.w0) and not got[0].norm_reg.any()
    for m in range(len(inp.grads)):
        a, prev, what = got[m + 1], got[m], "%s micro-step %d" % (tag, m + 1)
        _close(a.acc, want.acc[m], what + " sum")
        assert not _bits(a.acc[pad]).any()                                   # the padding of acc: exactly +0
        if m % A != A - 1:
            # a micro-step that only sums: nothing but acc changes (norm_reg keeps the last update's values)
            for x, y in zip(a[:5], prev[:5]):
                assert _same_bits(x, y), what
            assert not _same_bits(a.acc, prev.acc)
            continue
        assert _same_bits(a.acc, prev.acc)                                   # the applying micro-step does not store its sum
        st = want.steps[(m + 1) // A - 1]
        _close(a.w, st.w, what + " weights")
        _close(a.state1, st.state1, what + " state1")
        if kind != "momentum":
            _close(a.state2, st.state2, what + " state2")
        _close(float(a.norm_reg[0]) ** 0.5, st.norm, what + " global norm")
        _close(float(a.norm_reg[1]), st.reg, what + " regulariser")
        if want.e is not None:
            _close(a.e, want.e[(m + 1) // A - 1], what + " average")
            assert not _bits(a.e[pad]).any()
        assert not a.w[pad].any()


def _whole_and_sliced(dev, inp, kind, A, tag, **kw):
    want = ref.accum_ref(inp, kind, A, setting=kw.get("setting"), rates=_rates(ref.UPDATES) if kw.get("scheduled") else None)
    whole = _run(dev, inp, kind, A, **kw)
    _check(inp, kind, A, whole, want, tag + " whole")
    sliced = _run(dev, inp, kind, A, slices=step_tail_ref.SMALL_SLICES, **kw)
    _check(inp, kind, A, sliced, want, tag + " sliced")
    for a, b in zip(whole, sliced):
        for x, y in zip(a, b):
            assert _same_bits(x, y)


@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_small_arena_accumulates(dev, kind, A):
    """Parameters of 1152, 700, 1, 1025 and 3000 elements (9 blocks), 2A + 1 micro-steps, whole and in SMALL_SLICES with the last
    slice on a side stream: after every micro-step acc, w, the slots and norm_reg against float64; w, the slots and norm_reg
    bit-unchanged by a micro-step that only sums; the padding of acc exactly +0; whole and sliced bit-identical."""
    _whole_and_sliced(dev, ref.accum_case("small", A), kind, A, "small %s A=%d" % (kind, A))


@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_small_arena_accumulates_with_average(dev, kind, A):
    """... with a moving average of the weights (`warm`: d = 1/10, 2/11): e follows the UPDATES and stands still in between."""
    _whole_and_sliced(dev, ref.accum_case("small", A), kind, A, "small %s A=%d warm" % (kind, A), setting="warm")


@pytest.mark.parametrize("A", [2, 3])
def test_small_arena_accumulates_scheduled_adam(dev, A):
    """... Adam on a `step` schedule (LR / 3 at update 0, LR / 10 at update 1) and an average without warm-up: rate and bias
    correction are those of the update, not of the micro-step."""
    _whole_and_sliced(dev, ref.accum_case("small", A), "adam", A, "small adam A=%d scheduled plain" % A, setting="plain", scheduled=True)


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_sums_equal_a_plain_update_on_the_means(dev, kind, A):
    """No L2, grad_scale 1, gradients k / 64 in [-1024, 1024]: every sum and the division by A are exact in float32, so after each
    update w, the slots and norm_reg equal, bit for bit, what the update without RN_OPT_F_ACCUM leaves when it is given the exact means."""
    inp = ref.exact_case(A)
    got = _run(dev, inp, kind, A)
    means = tuple(m.astype(np.float32) for m in ref.cycle_means(inp, A))
    assert all(np.array_equal(m.astype(np.float64), m64) for m, m64 in zip(means, ref.cycle_means(inp, A)))
    plain = _run(dev, inp._replace(grads=means), kind, 1)
    assert len(plain) == ref.UPDATES + 1 and len(got) == A * ref.UPDATES + 1
    for u in range(1, ref.UPDATES + 1):
        a, b = got[u * A], plain[u]
        for x, y in zip(a[:4], b[:4]):
            assert _same_bits(x, y), (kind, A, u)
    assert not _same_bits(got[-1].w, got[0].w)


def test_large_arena_accumulates(dev):
    """One parameter of 2097152 + 5 * 1024 + 7 elements, then three small ones: the 2048-block grid cap binds and part of the grid
    goes round again; a wrong stride or offset of acc shows in the wrapped region.  A = 2, momentum, 4 micro-steps."""
    inp = ref.accum_case("large", 2, ref.UPDATES, 0)
    assert len(inp.grads) == 4
    _check(inp, "momentum", 2, _run(dev, inp, "momentum", 2), ref.accum_ref(inp, "momentum", 2), "large momentum A=2")


# ---------------------------------------------------------------------------------------------- trainer
BASE = 1e-2
MICRO = 5
A_TRAINER = 2


def _build(dev, use_graph, optimizer="momentum", scheduled=False, ema=False, A=A_TRAINER):
    """The recipe of test_gpu_ema._build: MobileNetV2, 4 classes, dropout 0.2."""
    import layers, levels as levels_mod, retinanet, train
    lv = levels_mod.build_levels()
    layers.Dropout._next_seed[0] = 0x5EED
    torch.manual_seed(4)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    kw = {"lr_schedule": train.LRSchedule("step", BASE, warmup_steps=1, boundaries=(1,))} if scheduled else {}
    if ema:
        kw["ema_decay"] = 0.9
    if A != 1:
        kw["accumulate_steps"] = A
    return net, train.Trainer(net, lv, optimizer=optimizer, learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph, **kw)


@pytest.fixture(scope="module")
def feats(dev):
    """The inputs of test_gpu_ema.py (256 x 256, two boxes)."""
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
    return {"weights": tr.arena.weights.clone(), "state1": tr.opt.state1.clone(), "acc": tr.opt.acc.clone(),
            "state2": tr.opt.state2.clone() if tr.opt.state2 is not None else None,
            "ema": tr.opt.ema.clone() if tr.opt.ema is not None else None}


@pytest.fixture(scope="module")
def graph_run(dev, feats, tmp_path_factory):
    """The uninterrupted run: momentum, A = 2, the one-graph step, five micro-steps, the state after each, a checkpoint written after
    the third (the middle of the second cycle)."""
    import checkpoint
    net, tw = _build(dev, True)
    path = str(tmp_path_factory.mktemp("accum") / "model.safetensors")
    states = [_state(tw)]
    for i in range(MICRO):
        tw.step(feats)
        states.append(_state(tw))
        if i == 2:
            checkpoint.save(path, net, tw, step=3)
    return {"net": net, "trainer": tw, "checkpoint": path, "states": states}


@pytest.fixture(scope="module")
def eager_run(dev, feats):
    """The same run launched eagerly; the gradient arena after each of the first two micro-steps is kept for the reference."""
    _, te = _build(dev, False)
    states, grads = [_state(te)], []
    for i in range(MICRO):
        te.step(feats)
        states.append(_state(te))
        if i < A_TRAINER:
            grads.append(te.arena.grads.cpu().numpy().copy())
    return {"trainer": te, "states": states, "grads": grads}


def test_accumulating_step_is_one_graph_and_equals_eager(dev, graph_run, eager_run):
    """Five micro-steps with A = 2: ONE graph, captured once, replayed for both phases; two updates; the weights stand still over
    micro-steps 1, 3 and 5; weights, slots and acc bit-identical to eager launches after every micro-step."""
    import ops
    tw, te = graph_run["trainer"], eager_run["trainer"]
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    assert tw.opt.step_count == 2 == te.opt.step_count and tw.opt.micro_dev.item() == MICRO == te.opt.micro_dev.item()
    assert tw.opt.accum_dev.cpu().tolist() == [0, 0] and tw.opt._phase == 1 == te.opt._phase
    assert tw.drop_counter.item() == te.drop_counter.item() == MICRO * ops.DROPOUT_COUNTER_STEP      # fresh masks every micro-step
    s = graph_run["states"]
    for m in (1, 3, 5):
        assert torch.equal(s[m]["weights"], s[m - 1]["weights"]) and torch.equal(s[m]["state1"], s[m - 1]["state1"])
        assert not torch.equal(s[m]["acc"], s[m - 1]["acc"])
    for m in (2, 4):
        assert not torch.equal(s[m]["weights"], s[m - 1]["weights"]) and torch.equal(s[m]["acc"], s[m - 1]["acc"])
    for m, (a, b) in enumerate(zip(s, eager_run["states"])):
        for k in ("weights", "state1", "acc"):
            assert torch.equal(a[k], b[k]), (m, k)
    pad = torch.ones(tw.arena.count, dtype=torch.bool, device=dev)
    for off, size in tw.arena.offsets:
        pad[off:off + size] = False
    assert not s[-1]["acc"][pad].any() and s[-1]["acc"][~pad].any()


def test_first_update_matches_the_reference(dev, eager_run):
    """The dropout masks advance per micro-step, so the two micro-step gradients are taken from the device; the float64 reference
    averages them and applies one momentum update: the weights after micro-step 2."""
    te = eager_run["trainer"]
    w0 = eager_run["states"][0]["weights"].cpu().numpy()
    wd = te.arena.wd_per_block.repeat_interleave(step_tail_ref.OPT_BLOCK).cpu().numpy()
    g1, g2 = eager_run["grads"]
    assert not np.array_equal(g1, g2)                                          # other masks: another gradient
    inp = step_tail_ref.OptInputs((), (), (), te.arena.count, w0, (g1, g2), wd, 1.0, BASE)
    want = ref.accum_ref(inp, "momentum", 2)
    _close(eager_run["states"][2]["weights"].cpu().numpy(), want.steps[0].w, "trainer weights after update 1")
    _close(eager_run["states"][2]["state1"].cpu().numpy(), want.steps[0].state1, "trainer momentum after update 1")
    _close(eager_run["states"][1]["acc"].cpu().numpy(), want.acc[0], "trainer sum after micro-step 1")
    # ... and not what an update from the second gradient alone would leave
    alone = step_tail_ref.optimizer_ref(inp._replace(grads=(g2,)), "momentum")[0].state1
    assert elementwise_rel_err(eager_run["states"][2]["state1"].cpu().numpy(), alone) > 10 * TOL


def test_scheduled_adam_with_ema_accumulates_in_one_graph(dev, feats):
    _, tw = _build(dev, True, "adam", scheduled=True, ema=True)
    _, te = _build(dev, False, "adam", scheduled=True, ema=True)
    w0 = tw.arena.weights.clone()
    for i in range(MICRO):
        tw.step(feats), te.step(feats)
        if i == 0:
            torch.cuda.synchronize()
            assert torch.equal(tw.arena.weights, w0) and torch.equal(tw.opt.ema, w0) and tw.opt.step_dev.item() == 0
    a, b = _state(tw), _state(te)
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert tw.opt.step_dev.item() == tw.opt.ema_updates_dev.item() == 2 == te.opt.step_dev.item() == te.opt.ema_updates_dev.item()
    assert tw.opt.step_count == 2 and torch.equal(tw.opt.lr_dev, te.opt.lr_dev) and torch.equal(tw.opt.ema_dev, te.opt.ema_dev)
    r = tw.opt.lr_dev.cpu().numpy()                                             # the rate and bias correction of update 1
    assert lr_schedule_ref.ulp_distance(r[0], tw.opt.schedule.value(1)) <= 1
    assert lr_schedule_ref.ulp_distance(r[1], lr_schedule_ref.adam_rate(r[0], 1)) <= 1
    assert not torch.equal(a["weights"], w0) and not torch.equal(a["ema"], a["weights"])


def test_resume_in_the_middle_of_a_cycle(dev, feats, graph_run):
    """The checkpoint written after micro-step 3 holds the half-summed cycle; a fresh trainer continues it bit for bit."""
    import checkpoint
    from safetensors import safe_open
    with safe_open(graph_run["checkpoint"], framework="pt") as f:
        meta, keys = f.metadata(), set(f.keys())
    assert meta["accum_steps"] == "2" and meta["accum_micro"] == "3" and meta["step_count"] == "1" and meta["step"] == "3"
    assert all("accum/" + k in keys for k, _ in graph_run["net"].named_parameters())
    net, tr = _build(dev, True)
    assert checkpoint.load(graph_run["checkpoint"], net, tr) == 3
    assert tr.opt.step_count == 1 and tr.opt.micro_dev.item() == 3 and tr.opt._phase == 1
    assert torch.equal(tr.opt.acc, graph_run["states"][3]["acc"]) and tr.opt.acc.any()
    for i in range(3, MICRO):
        tr.step(feats)
    got, want = _state(tr), graph_run["states"][MICRO]
    assert tr._graphs[5] and tr.opt.step_count == 2
    for k in ("weights", "state1", "acc"):
        assert torch.equal(got[k], want[k]), k


def test_checkpoint_without_a_sum_starts_a_fresh_cycle(dev, feats, tmp_path, capsys):
    import checkpoint
    from safetensors import safe_open
    net, t1 = _build(dev, False, A=1)
    assert t1.opt.acc is None
    for _ in range(3):
        t1.step(feats)
    path = str(tmp_path / "plain.safetensors")
    checkpoint.save(path, net, t1, step=3)
    with safe_open(path, framework="pt") as f:
        assert not any(k.startswith("accum/") for k in f.keys()) and "accum_steps" not in f.metadata()
    checkpoint._fresh_cycle_note[0] = False          # (said once per process: this is the test of that line)
    net2, tr = _build(dev, False)
    tr.step(feats)                                   # (leaves a sum and phase 1 behind: the load must clear both)
    assert checkpoint.load(path, net2, tr) == 3
    assert "fresh cycle" in capsys.readouterr().err
    assert tr.opt.step_count == 3 and tr.opt._phase == 0 and tr.opt.micro_dev.item() == 0 and not tr.opt.acc.any()
    assert torch.equal(tr.arena.weights, t1.arena.weights)
    w = tr.arena.weights.clone()
    tr.step(feats)
    torch.cuda.synchronize()
    assert torch.equal(tr.arena.weights, w) and tr.opt.step_count == 3 and tr.opt.acc.any()
    tr.step(feats)
    torch.cuda.synchronize()
    assert not torch.equal(tr.arena.weights, w) and tr.opt.step_count == 4
    # ... and a file WITH a sum loads into a trainer without accumulation: the keys are ignored
    path2 = str(tmp_path / "accum.safetensors")
    checkpoint.save(path2, net2, tr, step=5)
    net3, t3 = _build(dev, False, A=1)
    assert checkpoint.load(path2, net3, t3) == 5 and t3.opt.acc is None and t3.opt.step_count == 4
    assert torch.equal(t3.arena.weights, tr.arena.weights)


def test_cli_accumulates_and_resumes(tmp_path, capsys):
    """21 steps with --accumulate-steps 2 end in the middle of a cycle: 10 updates, the sum in the checkpoint; the rerun picks the
    cycle up (21 more steps: 21 updates in all)."""
    import train
    from safetensors import safe_open
    exp = str(tmp_path / "exp")
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "21", "--scale", "128", "--experiment", exp,
            "--backbone", "mobilenet_v2", "--dropout", "0.1", "--accumulate-steps", "2"]
    assert train.main(argv) == 21
    out = capsys.readouterr().out
    assert "step 20 " in out and out.strip().splitlines()[-1].endswith("update 10")
    assert train.LAST_RUN["updates"] == 10 and train.LAST_RUN["graph_sets"] == 1 and train.LAST_RUN["recaptures"] == 0
    with safe_open(os.path.join(exp, "model.safetensors"), framework="pt") as f:
        meta = f.metadata()
        assert meta["step"] == "21" and meta["step_count"] == "10" and meta["accum_steps"] == "2" and meta["accum_micro"] == "21"
        keys = [k for k in f.keys() if k.startswith("accum/")]
        assert keys and any(f.get_tensor(k).any() for k in keys)
    assert train.main(argv) == 42
    out = capsys.readouterr().out
    assert "restored step 21" in out and "update 20" in out
    assert train.LAST_RUN["updates"] == 21
    with safe_open(os.path.join(exp, "model.safetensors"), framework="pt") as f:
        assert f.metadata()["step_count"] == "21" and f.metadata()["accum_micro"] == "42"
    with pytest.raises(SystemExit):
        train.main(argv + ["--grad-clip-norm", "1.0"])
