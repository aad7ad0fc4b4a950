"""The moving average of the weights on the MI355X (-m gpu): rn_step_control_eval (EMA) against the float64 formula, the average the
update kernel keeps against the float64 reference (ema_ref.py) on the synthetic arenas of test_gpu_step_tail.py, an EMA trainer's
ONE captured graph against eager launches and across a checkpoint, Trainer.ema_weights(), and the command line."""
import collections
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import ema_ref as ref
import lr_schedule_ref
import step_tail_ref
from helpers import assert_close, elementwise_rel_err, step_control

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = ("momentum", "rmsprop", "adam")
SETTINGS = tuple(ref.SETTINGS)          # warm (D = 0.9999 with warm-up), plain (D = 0.5 without), capped (D = 0.22 with: D binds)


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


def _decay_eval(decay, warmup, word, ema_dev):
    """The control launch with the average's part alone: word and ema_dev are device pointers (or None)."""
    import _rn
    return step_control(_rn.stream(), features=_rn.CTL_F_EMA, ema_decay=decay, ema_warmup=int(warmup), ema_updates_dev=word, ema_dev=ema_dev)


# ------------------------------------------------------------------------------------------------ the one-thread kernel
@pytest.mark.parametrize("setting", SETTINGS)
def test_device_decay_values(dev, setting):
    """12 launches: ema_dev = [d(n), 1 - d(n)], each within 1 ulp of the float64 formula rounded once; the word counts the launches."""
    import _rn
    s = ref.SETTINGS[setting]
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    ema_dev = torch.zeros(2, dtype=torch.float32, device=dev)
    for n in range(12):
        _rn.check(_decay_eval(s.decay, s.warmup, word.data_ptr(), _rn.f32(ema_dev)), "rn_step_control_eval")
        got = ema_dev.cpu().numpy()
        d, om = ref.decay_pair(n, s.decay, s.warmup)
        assert lr_schedule_ref.ulp_distance(got[0], d) <= 1, (setting, n, got[0], d)
        assert lr_schedule_ref.ulp_distance(got[1], om) <= 1, (setting, n, got[1], om)
        assert int(word.item()) == n + 1
    assert int(word.item()) == 12
    # a late update: D binds under warm-up, and 1 - D is rounded from float64 (not 1 - float32(D))
    word.fill_(10 ** 6)
    _rn.check(_decay_eval(s.decay, s.warmup, word.data_ptr(), _rn.f32(ema_dev)), "rn_step_control_eval")
    d, om = ref.decay_pair(10 ** 6, s.decay, s.warmup)
    got = ema_dev.cpu().numpy()
    assert lr_schedule_ref.ulp_distance(got[0], d) <= 1 and lr_schedule_ref.ulp_distance(got[1], om) <= 1
    assert int(word.item()) == 10 ** 6 + 1


def test_entries_refuse_bad_arguments(dev):
    import _rn
    L = _rn.lib()
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    ema_dev = torch.zeros(2, dtype=torch.float32, device=dev)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert _decay_eval(bad, 1, word.data_ptr(), _rn.f32(ema_dev)) != 0
    assert _decay_eval(0.5, 1, None, _rn.f32(ema_dev)) != 0
    assert _decay_eval(0.5, 1, word.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and not ema_dev.cpu().numpy().any()          # nothing was launched
    w = torch.zeros(1024, dtype=torch.float32, device=dev)
    wd = torch.zeros(1, dtype=torch.float32, device=dev)

    def step_ema(e, ed):
        u = _rn.OptUpdate(kind=0, features=_rn.OPT_F_EMA, w=_rn.f32(w), grad=_rn.f32(w), state1=_rn.f32(w), wd_per_block=_rn.f32(wd),
                          count=1024, lr=0.1, grad_scale=1.0, step=1, ema=e, ema_dev=ed)
        return L.rn_optimizer_update(ctypes.byref(u), _rn.stream())
    assert step_ema(None, _rn.f32(ema_dev)) != 0
    assert step_ema(_rn.f32(w), None) != 0
    assert step_ema(w[1:].data_ptr(), _rn.f32(ema_dev)) != 0      # not 16-byte aligned
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the average on an arena
EmaGot = collections.namedtuple("EmaGot", "w state1 state2 norm_reg e")


def _run(dev, inp, kind, setting=None, clip=None, slices=None):
    """Three steps on a synthetic module laid out as `inp` (test_gpu_step_tail._run_optimizer); one EmaGot per step.  `slices`:
    begin_step / step_slice / finish_step over these ranges, the LAST slice on a side stream.  setting=None: no average."""
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
        s = ref.SETTINGS[setting]
        kw = dict(ema_decay=s.decay, ema_warmup=s.warmup)
    opt = train.Optimizer(arena, kind, inp.lr, grad_clip_norm=clip, **kw)
    if setting is not None:
        assert torch.equal(opt.ema, arena.weights) and opt.ema.data_ptr() != arena.weights.data_ptr()
        assert opt.ema_updates_dev.item() == 0 and opt.ema_dev.shape == (2,)
    else:
        assert opt.ema is None and opt.ema_dev is None and opt.ema_updates_dev is None
    side = torch.cuda.Stream()
    out = []
    for n, g in enumerate(inp.grads):
        for p, off, s in zip(arena.params, inp.offsets, inp.sizes):
            p.grad.copy_(torch.from_numpy(g[off:off + s]).to(dev))
        if slices is None:
            opt.step(grad_scale=inp.grad_scale)
        else:
            side.wait_stream(torch.cuda.current_stream())          # (the gradients were copied on the main stream)
            opt.begin_step()
            for i, (lo, hi) in enumerate(slices):
                opt.step_slice(lo, hi, inp.grad_scale, stream=side if i == len(slices) - 1 else None)
            torch.cuda.current_stream().wait_stream(side)
            opt.finish_step()
        torch.cuda.synchronize()
        if setting is not None:
            assert opt.ema_updates_dev.item() == n + 1 == opt.step_count
            d, om = ref.decay_pair(n, s_decay(setting), ref.SETTINGS[setting].warmup)
            got = opt.ema_dev.cpu().numpy()
            assert lr_schedule_ref.ulp_distance(got[0], d) <= 1 and lr_schedule_ref.ulp_distance(got[1], om) <= 1
            assert abs(opt.ema_decay_value(n) - float(ref.decay_value(n, s_decay(setting), ref.SETTINGS[setting].warmup))) <= 1e-15
        out.append(EmaGot(arena.weights.cpu().numpy(), opt.state1.cpu().numpy(),
                          opt.state2.cpu().numpy() if opt.state2 is not None else None, opt.norm_reg.cpu().numpy(),
                          opt.ema.cpu().numpy() if opt.ema is not None else None))
    return out


def s_decay(setting):
    return ref.SETTINGS[setting].decay


@functools.lru_cache(maxsize=None)
def _ref(name, kind, setting, clip=None):
    return ref.ema_ref(ref.ema_case(name), kind, setting, clip)


@functools.lru_cache(maxsize=None)
def _plain_run(name, kind, clip=None):
    """The run WITHOUT an average, once per (arena, kind, clip): what an EMA run must leave untouched."""
    return _run(torch.device("cuda:0"), ref.ema_case(name), kind, None, clip)


def _check(inp, kind, got, want, tag):
    pad = step_tail_ref.padding_mask(inp)
    for step, (a, b, e) in enumerate(zip(got, want.steps, want.e), 1):
        what = "%s step %d" % (tag, step)
        _close(a.e, e, what + " average")
        _close(a.w, b.w, what + " weights")
        _close(a.state1, b.state1, what + " state1")
        if kind != "momentum":
            _close(a.state2, b.state2, what + " state2")
        _close(float(a.norm_reg[0]) ** 0.5, b.norm, what + " global norm")
        _close(float(a.norm_reg[1]), b.reg, what + " regulariser")
        assert not _bits(a.e[pad]).any() and not a.w[pad].any()          # the padding of e: exactly +0
    # the average is neither the weights nor the initial weights: it was formed
    assert elementwise_rel_err(got[-1].e, got[-1].w) > 10 * TOL and elementwise_rel_err(got[-1].e, inp.w0) > 10 * TOL


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_small_arena_average(dev, kind, setting):
    """Parameters of 1152, 700, 1, 1025 and 3000 elements (9 blocks), three steps, whole and in SMALL_SLICES with the last slice on
    a side stream: e, w, the slots and norm_reg against float64; whole and sliced e bit-identical; w and the slots bit-identical to
    a run that keeps no average."""
    inp = ref.ema_case("small")
    want = _ref("small", kind, setting)
    whole = _run(dev, inp, kind, setting)
    _check(inp, kind, whole, want, "small %s %s whole" % (kind, setting))
    sliced = _run(dev, inp, kind, setting, slices=step_tail_ref.SMALL_SLICES)
    _check(inp, kind, sliced, want, "small %s %s sliced" % (kind, setting))
    for a, b, c in zip(whole, sliced, _plain_run("small", kind)):
        assert np.array_equal(_bits(a.e), _bits(b.e))
        for x, y, z in zip(a[:3], b[:3], c[:3]):
            assert (x is None and y is None and z is None) or (np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z)))
        assert np.array_equal(_bits(a.norm_reg), _bits(c.norm_reg))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_small_arena_average_with_clipping(dev, kind, setting):
    """The norm pass + rn_optimizer_update (CLIP + EMA): clip 0.5 binds, clip 1e6 does not -- then e equals the fused
    path's bit for bit.  w and the slots equal a clipped run's without the average bit for bit."""
    inp = ref.ema_case("small")
    binds = _run(dev, inp, kind, setting, clip=step_tail_ref.CLIP_BINDS)
    _check(inp, kind, binds, _ref("small", kind, setting, step_tail_ref.CLIP_BINDS), "small %s %s clip binds" % (kind, setting))
    loose = _run(dev, inp, kind, setting, clip=step_tail_ref.CLIP_LOOSE)
    _check(inp, kind, loose, _ref("small", kind, setting, step_tail_ref.CLIP_LOOSE), "small %s %s clip loose" % (kind, setting))
    fused = _run(dev, inp, kind, setting)
    for a, b in zip(loose, fused):
        assert np.array_equal(_bits(a.e), _bits(b.e)) and np.array_equal(_bits(a.w), _bits(b.w))
    assert not np.array_equal(binds[0].e, fused[0].e)
    for a, c in zip(binds, _plain_run("small", kind, step_tail_ref.CLIP_BINDS)):
        for x, z in zip(a[:4], c[:4]):
            assert (x is None and z is None) or np.array_equal(_bits(x), _bits(z))


def test_large_arena_average(dev):
    """One parameter of 2097152 + 5 * 1024 + 7 elements, then three small ones: the 2048-block grid cap binds and part of the grid
    goes round again; a wrong stride or offset of e shows in the wrapped region."""
    inp = ref.ema_case("large")
    _check(inp, "momentum", _run(dev, inp, "momentum", "warm"), _ref("large", "momentum", "warm"), "large momentum warm")


# ---------------------------------------------------------------------------------------------- trainer
BASE = 1e-2
DECAY = 0.9
STEPS = 6


def _build(dev, use_graph, optimizer="momentum", scheduled=False, ema=True):
    import layers, levels as levels_mod, retinanet, train
    lv = levels_mod.build_levels()
    layers.Dropout._next_seed[0] = 0x5EED
    torch.manual_seed(4)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    kw = {"lr_schedule": train.LRSchedule("step", BASE, warmup_steps=2, boundaries=(4,))} if scheduled else {}
    if ema:
        kw["ema_decay"] = DECAY
    return net, train.Trainer(net, lv, optimizer=optimizer, learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph, **kw)


@pytest.fixture(scope="module")
def feats(dev):
    """The inputs of test_whole_step_graph_equals_segments_and_eager (the recipe of test_gpu_lr_schedule.py)."""
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
    """The uninterrupted run the trainer tests compare against, computed once: a constant-rate momentum trainer with
    ema_decay=0.9, the one-graph step, six steps, a checkpoint written after the third."""
    import checkpoint
    net, tw = _build(dev, True)
    w0 = tw.arena.weights.clone()
    path = str(tmp_path_factory.mktemp("ema") / "model.safetensors")
    for i in range(STEPS):
        tw.step(feats)
        if i == 2:
            checkpoint.save(path, net, tw, step=3)
    torch.cuda.synchronize()
    return {"net": net, "trainer": tw, "checkpoint": path, "w0": w0, "weights": tw.arena.weights.clone(),
            "state1": tw.opt.state1.clone(), "ema": tw.opt.ema.clone()}


def test_ema_step_is_one_graph_and_equals_eager(dev, feats, graph_run):
    """Six steps with ema_decay=0.9 (d = 0.1, 2/11, ..., 6/15 under the warm-up): ONE graph, captured once; weights, slots and e
    bit-identical to eager launches; weights and slots bit-identical to a trainer that keeps no average."""
    tw = graph_run["trainer"]
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    assert tw.opt.ema_updates_dev.item() == STEPS == tw.opt.step_count
    d, om = ref.decay_pair(STEPS - 1, DECAY, True)
    got = tw.opt.ema_dev.cpu().numpy()
    assert lr_schedule_ref.ulp_distance(got[0], d) <= 1 and lr_schedule_ref.ulp_distance(got[1], om) <= 1
    _, te = _build(dev, False)
    assert torch.equal(te.arena.weights, graph_run["w0"]) and torch.equal(te.opt.ema, graph_run["w0"])
    _, tn = _build(dev, True, ema=False)
    assert tn.opt.ema is None
    for i in range(STEPS):
        te.step(feats)
        tn.step(feats)
    torch.cuda.synchronize()
    assert tn._graphs[5] and tn.recaptures == 0
    assert torch.equal(te.arena.weights, graph_run["weights"]) and torch.equal(te.opt.state1, graph_run["state1"])
    assert torch.equal(te.opt.ema, graph_run["ema"]) and torch.equal(te.opt.ema_dev, tw.opt.ema_dev)
    assert te.opt.ema_updates_dev.item() == STEPS
    assert torch.equal(tn.arena.weights, graph_run["weights"]) and torch.equal(tn.opt.state1, graph_run["state1"])
    # the average moved, lags behind the weights, and its padding is still zero
    e, w = graph_run["ema"], graph_run["weights"]
    assert not torch.equal(e, w) and not torch.equal(e, graph_run["w0"])
    pad = torch.ones(tw.arena.count, dtype=torch.bool, device=dev)
    for off, size in tw.arena.offsets:
        pad[off:off + size] = False
    assert not e[pad].any() and not w[pad].any()


def test_scheduled_adam_with_ema_is_one_graph_and_equals_eager(dev, feats):
    _, tw = _build(dev, True, "adam", scheduled=True)
    _, te = _build(dev, False, "adam", scheduled=True)
    _, tn = _build(dev, True, "adam", scheduled=True, ema=False)
    for i in range(3):
        tw.step(feats), te.step(feats), tn.step(feats)
    torch.cuda.synchronize()
    assert tw._graphs[5] and len(tw._graph_cache) == 1 and tw.recaptures == 0
    assert torch.equal(tw.arena.weights, te.arena.weights) and torch.equal(tw.opt.ema, te.opt.ema)
    assert torch.equal(tw.opt.state1, te.opt.state1) and torch.equal(tw.opt.state2, te.opt.state2)
    assert torch.equal(tw.arena.weights, tn.arena.weights) and torch.equal(tw.opt.state2, tn.opt.state2)
    assert tw.opt.ema_updates_dev.item() == te.opt.ema_updates_dev.item() == tw.opt.step_dev.item() == 3
    assert not torch.equal(tw.opt.ema, tw.arena.weights)


def test_resume_continues_the_average(dev, feats, graph_run):
    """The checkpoint written after step 3, loaded into a fresh EMA trainer: steps 4-6 reproduce e and the weights bit for bit."""
    import checkpoint
    from safetensors import safe_open
    with safe_open(graph_run["checkpoint"], framework="pt") as f:
        meta, keys = f.metadata(), set(f.keys())
    assert meta["format"] == "retinanet-amd-v2" and meta["ema_updates"] == "3" and meta["ema_warmup"] == "1"
    assert float(meta["ema_decay"]) == DECAY
    names = [k for k, _ in graph_run["net"].named_parameters()]
    assert all("ema/" + k in keys and "model/" + k in keys for k in names)
    net, tr = _build(dev, True)
    assert checkpoint.load(graph_run["checkpoint"], net, tr) == 3
    assert tr.opt.step_count == 3 and tr.opt.ema_updates_dev.item() == 3
    assert not torch.equal(tr.opt.ema, tr.arena.weights)
    for i in range(3, STEPS):
        tr.step(feats)
    torch.cuda.synchronize()
    assert tr._graphs[5] and torch.equal(tr.arena.weights, graph_run["weights"]) and torch.equal(tr.opt.state1, graph_run["state1"])
    assert torch.equal(tr.opt.ema, graph_run["ema"]) and tr.opt.ema_updates_dev.item() == STEPS


def test_checkpoint_without_average_seeds_it(dev, feats, tmp_path, capsys):
    import checkpoint
    net, tn = _build(dev, False, ema=False)
    for i in range(2):
        tn.step(feats)
    path = str(tmp_path / "plain.safetensors")
    checkpoint.save(path, net, tn, step=2)
    checkpoint._seeded_note[0] = False          # (said once per process: this is the test of that line)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        assert not any(k.startswith("ema/") for k in f.keys()) and "ema_decay" not in f.metadata()
    net2, tr = _build(dev, False)
    assert checkpoint.load(path, net2, tr) == 2
    assert torch.equal(tr.opt.ema, tr.arena.weights) and torch.equal(tr.arena.weights, tn.arena.weights)
    assert tr.opt.ema_updates_dev.item() == tr.opt.step_count == 2
    assert "no moving average" in capsys.readouterr().err
    with pytest.raises(ValueError, match="plain.safetensors"):
        checkpoint.load(path, net2, use_ema=True)
    # ... and a file WITH averages loads into a trainer without: the keys are ignored
    net3, t3 = _build(dev, False, ema=False)
    path2 = str(tmp_path / "ema.safetensors")
    checkpoint.save(path2, net2, tr, step=2)
    assert checkpoint.load(path2, net3, t3) == 2 and t3.opt.ema is None and torch.equal(t3.arena.weights, tr.arena.weights)


def test_misshapen_average_is_refused_before_anything_is_overwritten(dev, graph_run, tmp_path):
    import checkpoint
    from safetensors import safe_open
    from safetensors.torch import save_file
    with safe_open(graph_run["checkpoint"], framework="pt") as f:
        meta = f.metadata()
        tensors = {k: f.get_tensor(k) for k in f.keys()}
    name = next(k for k in tensors if k.startswith("ema/"))
    net, tr = _build(dev, False)
    before = tr.arena.weights.clone()
    bad = dict(tensors)
    bad[name] = torch.zeros(tuple(tensors[name].shape) + (2,))
    save_file(bad, str(tmp_path / "misshapen.safetensors"), metadata=meta)
    with pytest.raises(ValueError, match=name):
        checkpoint.load(str(tmp_path / "misshapen.safetensors"), net, tr)
    bad = dict(tensors)
    del bad[name]
    save_file(bad, str(tmp_path / "missing.safetensors"), metadata=meta)
    with pytest.raises(ValueError, match=name):
        checkpoint.load(str(tmp_path / "missing.safetensors"), net, tr)
    assert torch.equal(tr.arena.weights, before) and torch.equal(tr.opt.ema, before)


def test_ema_weights_swaps_and_restores(dev, feats, graph_run, tmp_path):
    """Inside the block the net's parameters are the average; outside everything is as before, bit for bit, also after an
    exception in the body; checkpoint.load(use_ema=True) gives a net the same parameters."""
    import checkpoint, layers, levels as levels_mod, retinanet
    tw, net = graph_run["trainer"], graph_run["net"]
    w, e = graph_run["weights"], graph_run["ema"]
    with torch.no_grad():
        raw_out = net(feats["image"], training=False)["classifications"]
        raw_out = {k: v.clone() for k, v in raw_out.items()}
    with tw.ema_weights():
        assert torch.equal(tw.arena.weights, e) and torch.equal(tw.opt.ema, w)
        for p, (off, size) in zip(tw.arena.params, tw.arena.offsets):
            assert torch.equal(p.detach().reshape(-1), e[off:off + size])
        inside = {k: v.detach().clone() for k, v in net.named_parameters()}
        with torch.no_grad():
            ema_out = {k: v.clone() for k, v in net(feats["image"], training=False)["classifications"].items()}
    assert torch.equal(tw.arena.weights, w) and torch.equal(tw.opt.ema, e)
    assert any(not torch.equal(ema_out[k], raw_out[k]) for k in raw_out)           # the net really ran on other weights
    with pytest.raises(RuntimeError, match="boom"):
        with tw.ema_weights():
            raise RuntimeError("boom")
    assert torch.equal(tw.arena.weights, w) and torch.equal(tw.opt.ema, e)
    path = str(tmp_path / "final.safetensors")
    checkpoint.save(path, net, tw, step=STEPS)
    lv = levels_mod.build_levels()
    net2 = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    assert checkpoint.load(path, net2, use_ema=True) == STEPS
    for k, v in net2.named_parameters():
        assert torch.equal(v.detach(), inside[k]), k
    _, tn = _build(dev, False, ema=False)
    with pytest.raises(ValueError, match="ema_decay"):
        with tn.ema_weights():
            pass


def test_cli_trains_evaluates_and_resumes_with_ema(tmp_path, capsys):
    import train
    from safetensors import safe_open
    exp = str(tmp_path / "exp")
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "20", "--scale", "128", "--experiment", exp,
            "--backbone", "mobilenet_v2", "--dropout", "0.1", "--ema-decay", "0.9", "--eval-images", "2"]
    assert train.main(argv) == 20
    out = capsys.readouterr().out.splitlines()
    raw = [l for l in out if l.startswith("eval:")]
    ema = [l for l in out if l.startswith("eval (ema):")]
    assert len(raw) == 1 and len(ema) == 1 and "over 2 images" in raw[0] and "over 2 images" in ema[0]
    assert raw[0].split()[1::2] == ema[0].split()[2::2]                          # the same format: the same field names
    with safe_open(os.path.join(exp, "model.safetensors"), framework="pt") as f:
        meta = f.metadata()
        keys = [k for k in f.keys() if k.startswith("ema/")]
        assert keys and meta["ema_updates"] == "20" and float(meta["ema_decay"]) == 0.9 and meta["ema_warmup"] == "1"
        assert all("model/" + k[4:] in f.keys() for k in keys)
        assert any(not torch.equal(f.get_tensor(k), f.get_tensor("model/" + k[4:])) for k in keys)
    assert train.main(argv) == 40                                                # resumed from step 20
    out = capsys.readouterr().out
    assert "restored step 20" in out and out.count("eval (ema):") == 1
    with safe_open(os.path.join(exp, "model.safetensors"), framework="pt") as f:
        assert f.metadata()["ema_updates"] == "40"
