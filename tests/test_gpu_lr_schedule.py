"""Learning-rate schedules on the MI355X (-m gpu): rn_step_control_eval (LR) against train.LRSchedule.value, the device-rate update
against the CPU oracle, and a scheduled trainer's ONE captured graph against eager launches, against a constant-rate trainer fed the
same rates by hand, and across a checkpoint."""
import numpy as np
import pytest
import torch

import lr_schedule_ref as ref
from helpers import assert_close, step_control
from oracle import train_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4          # (the bar of the other optimizer / kernel parity tests: test_gpu_ops.TOL)
BASE = 1e-2
SCHEDULES = {
    "constant": dict(kind="constant", warmup_steps=3, total_steps=9),
    "step": dict(kind="step", warmup_steps=2, boundaries=(4, 7), total_steps=9),
    "cosine": dict(kind="cosine", warmup_steps=2, total_steps=9, final_factor=0.05),
}
KINDS = ["momentum", "rmsprop", "adam"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    return torch.device("cuda:0")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_device_schedule_values(dev, name, kind):
    """12 launches of the one-thread kernel: lr_dev[0] follows LRSchedule.value(s) (both float64, rounded once: <= 1 ulp), lr_dev[1]
    carries Adam's bias correction (the other kinds: the rate itself), the step word counts the launches."""
    import _rn, train
    sched = train.LRSchedule(base_lr=BASE, **SCHEDULES[name])
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    lr_dev = torch.zeros(2, dtype=torch.float32, device=dev)
    d = sched.struct()
    for s in range(12):
        _rn.check(step_control(_rn.stream(), features=_rn.CTL_F_LR, optimizer_kind=_rn.OPT[kind], schedule=d, step_dev=step_dev.data_ptr(),
                               lr_dev=_rn.f32(lr_dev)), "rn_step_control_eval")
        got = lr_dev.cpu().numpy()
        want = sched.value(s)
        assert ref.ulp_distance(got[0], want) <= 1, (name, kind, s, got[0], want)
        assert ref.ulp_distance(got[0], ref.lr_value(s, base=BASE, **SCHEDULES[name])) <= 1
        if kind == "adam":
            assert ref.ulp_distance(got[1], ref.adam_rate(got[0], s)) <= 1, (name, s, got[1], ref.adam_rate(got[0], s))
        else:
            assert got[1] == got[0]
        assert int(step_dev.item()) == s + 1
    assert int(step_dev.item()) == 12


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_scheduled_optimizer_matches_tf_semantics(dev, kind, sliced):
    """The module of test_optimizer_matches_tf_semantics (three arena blocks), no clipping, warm-up 2 + a drop at update 3: five
    updates whose rate the kernel reads from the device, against the oracle fed LRSchedule.value(s).  `sliced`: the update in two
    slices, the second on another stream (ordered behind the schedule kernel by the optimizer)."""
    import _rn, train
    torch.manual_seed(0)
    lin = torch.nn.Module()
    lin.a = torch.nn.Parameter(torch.randn(3, 3, 8, 16))
    lin.a.l2_scale = 1e-4
    lin.b = torch.nn.Parameter(torch.randn(700))
    params = {"a": lin.a.detach().clone(), "b": lin.b.detach().clone()}
    lin.to(dev)
    arena = train.ParamArena(lin, dev)
    assert arena.count == 3 * train.OPT_BLOCK
    sched = train.LRSchedule("step", BASE, warmup_steps=2, boundaries=(3,))
    opt = train.Optimizer(arena, kind, 123.0, schedule=sched)
    assert opt.lr == BASE and opt.lr_dev is not None and opt.step_dev is not None
    side = torch.cuda.Stream()
    state = {}
    for s in range(5):
        grads = {"a": torch.randn(3, 3, 8, 16), "b": torch.randn(700)}
        lin.a.grad.copy_(grads["a"].to(dev)); lin.b.grad.copy_(grads["b"].to(dev))
        assert opt.current_lr() == float(sched.value(s))
        if sliced:
            opt.begin_step()
            opt.step_slice(0, 2 * train.OPT_BLOCK, 0.5)
            opt.step_slice(2 * train.OPT_BLOCK, arena.count, 0.5, stream=side)
            torch.cuda.current_stream().wait_stream(side)
            opt.finish_step()
        else:
            opt.step(grad_scale=0.5)
        tot = {"a": grads["a"] * 0.5 + 1e-4 * params["a"], "b": grads["b"] * 0.5}
        gn = float(np.sqrt(sum(float((t.double() ** 2).sum()) for t in tot.values())))
        assert_close(opt.norm_reg[0].item() ** 0.5, gn, TOL, "global norm")
        train_ref.apply_optimizer(kind, params, tot, state, float(sched.value(s)), s + 1)
        assert_close(lin.a.detach().cpu().numpy(), params["a"].numpy(), TOL, "weights a update %d" % s)
        assert_close(lin.b.detach().cpu().numpy(), params["b"].numpy(), TOL, "weights b update %d" % s)
        assert ref.ulp_distance(opt.lr_dev[0].item(), sched.value(s)) <= 1
    assert int(opt.step_dev.item()) == opt.step_count == 5
    opt.set_step_count(2)
    assert int(opt.step_dev.item()) == opt.step_count == 2 and opt.current_lr() == float(sched.value(2))


# ---------------------------------------------------------------------------------------------- trainer
STEPS = 6


def _trainer_schedule():
    import train
    return train.LRSchedule("step", BASE, warmup_steps=2, boundaries=(4,))


def _build(dev, use_graph, optimizer="momentum", scheduled=True):
    import layers, levels as levels_mod, retinanet, train
    lv = levels_mod.build_levels()
    layers.Dropout._next_seed[0] = 0x5EED
    torch.manual_seed(4)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    kw = {"lr_schedule": _trainer_schedule()} if scheduled else {}
    return net, train.Trainer(net, lv, optimizer=optimizer, learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph, **kw)


@pytest.fixture(scope="module")
def feats(dev):
    """The inputs of test_whole_step_graph_equals_segments_and_eager."""
    import dataset, levels as levels_mod
    lv = levels_mod.build_levels()
    rng = np.random.default_rng(2)
    size = 256
    image = torch.from_numpy(rng.standard_normal((2, size, size, 3)).astype(np.float32)).to(dev)
    boxes = torch.tensor([[[0.1, 0.2, 0.7, 0.8], [0.4, 0.1, 0.9, 0.5]]], device=dev)
    cids = torch.tensor([[1, 3]], dtype=torch.int32, device=dev)
    c, r, m = dataset.build_labels((size, size), cids, boxes, lv, 4, flip_pair=True)
    return {"image": image, "detection": {"classifications": c, "regressions": r}, "trainable_masks": m}


@pytest.fixture(scope="module")
def graph_run(dev, feats, tmp_path_factory):
    """The uninterrupted run every trainer test compares against, computed once: a scheduled momentum trainer's one-graph step, six
    steps, a checkpoint written after the third."""
    import checkpoint
    net, tw = _build(dev, True)
    path = str(tmp_path_factory.mktemp("lr_schedule") / "model.safetensors")
    losses, rates = [], []
    for i in range(STEPS):
        out = tw.step(feats)
        losses.append(tuple(out[k].item() for k in ("class_loss", "regr_loss", "regularization_loss")))
        rates.append(tw.opt.lr_dev.cpu().numpy().copy())
        if i == 2:
            checkpoint.save(path, net, tw, step=3)
    torch.cuda.synchronize()
    return {"trainer": tw, "losses": losses, "rates": rates, "checkpoint": path, "weights": tw.arena.weights.clone(),
            "state1": tw.opt.state1.clone()}


def test_scheduled_whole_step_graph_equals_eager(dev, feats, graph_run):
    """Warm-up 2, a drop at update 4, six steps: the rate changes five times and the step stays ONE graph, captured once -- and
    computes, bit for bit, what eager launches of the same kernels compute."""
    import ops
    tw = graph_run["trainer"]
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    sched = _trainer_schedule()
    for s, r in enumerate(graph_run["rates"]):
        assert ref.ulp_distance(r[0], sched.value(s)) <= 1 and r[1] == r[0]
    assert len(set(float(r[0]) for r in graph_run["rates"])) == 4            # (1/3, 2/3, 1, 1, 0.1, 0.1) x base
    _, te = _build(dev, False)
    for i in range(STEPS):
        out = te.step(feats)
        got = tuple(out[k].item() for k in ("class_loss", "regr_loss", "regularization_loss"))
        assert got == graph_run["losses"][i], (i, got, graph_run["losses"][i])
        assert np.array_equal(te.opt.lr_dev.cpu().numpy(), graph_run["rates"][i])
    torch.cuda.synchronize()
    assert torch.equal(te.arena.weights, graph_run["weights"]) and torch.equal(te.opt.state1, graph_run["state1"])
    assert te.drop_counter.item() == tw.drop_counter.item() == STEPS * ops.DROPOUT_COUNTER_STEP
    assert torch.equal(te.opt.lr_dev, tw.opt.lr_dev)
    assert te.opt.step_dev.item() == tw.opt.step_dev.item() == STEPS == te.opt.step_count == tw.opt.step_count
    assert tw.opt.current_lr() == te.opt.current_lr() == float(sched.value(STEPS)) and tw.opt.lr == BASE


def test_device_rate_is_the_same_scalar_as_a_launch_argument(dev, feats, graph_run):
    """A trainer without a schedule, launched eagerly, whose opt.lr is set before every step to the float the scheduled trainer's
    kernel left in lr_dev[0]: bit-identical weights -- the device rate is only another source of the same scalar."""
    _, tc = _build(dev, False, scheduled=False)
    assert tc.opt.lr_dev is None and tc.opt.schedule is None
    for i in range(STEPS):
        tc.opt.lr = float(graph_run["rates"][i][0])
        tc.step(feats)
    torch.cuda.synchronize()
    assert torch.equal(tc.arena.weights, graph_run["weights"]) and torch.equal(tc.opt.state1, graph_run["state1"])


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_adam_and_rmsprop_enter_the_one_graph_step(dev, feats, optimizer):
    """With a schedule no scalar of the update is a launch argument (Adam's bias correction is formed on the device): both
    optimizers run inside the one captured graph and match eager launches bit for bit."""
    _, tw = _build(dev, True, optimizer)
    _, te = _build(dev, False, optimizer)
    for i in range(3):
        ow, oe = tw.step(feats), te.step(feats)
        for k in ("class_loss", "regr_loss", "regularization_loss"):
            assert ow[k].item() == oe[k].item(), (i, k, ow[k].item(), oe[k].item())
    torch.cuda.synchronize()
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    assert torch.equal(tw.arena.weights, te.arena.weights)
    assert torch.equal(tw.opt.state1, te.opt.state1) and torch.equal(tw.opt.state2, te.opt.state2)
    assert torch.equal(tw.opt.lr_dev, te.opt.lr_dev) and tw.opt.step_dev.item() == te.opt.step_dev.item() == 3
    if optimizer == "adam":
        r = tw.opt.lr_dev.cpu().numpy()
        assert ref.ulp_distance(r[1], ref.adam_rate(r[0], 2)) <= 1 and r[1] != r[0]


def test_resume_continues_the_schedule(dev, feats, graph_run):
    """The checkpoint written after step 3, loaded into a fresh scheduled trainer: steps 4-6 (the last warm-up-free steps and the
    drop at update 4) reproduce the uninterrupted run's weights bit for bit."""
    import checkpoint
    net, tr = _build(dev, True)
    assert checkpoint.load(graph_run["checkpoint"], net, tr) == 3
    assert tr.opt.step_count == 3 and tr.opt.step_dev.item() == 3
    for i in range(3, STEPS):
        out = tr.step(feats)
        got = tuple(out[k].item() for k in ("class_loss", "regr_loss", "regularization_loss"))
        assert got == graph_run["losses"][i], (i, got, graph_run["losses"][i])
    torch.cuda.synchronize()
    assert tr._graphs[5] and torch.equal(tr.arena.weights, graph_run["weights"]) and torch.equal(tr.opt.state1, graph_run["state1"])
    assert np.array_equal(tr.opt.lr_dev.cpu().numpy(), graph_run["rates"][-1]) and tr.opt.step_dev.item() == STEPS
