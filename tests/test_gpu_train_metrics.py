"""The running training metrics on the MI355X (-m gpu): rn_train_metrics_pass / rn_train_metrics_fold through
metrics.TrainMetrics against the float64 reference (train_metrics_ref.py), and Trainer(train_metrics=True): one graph against
eager launches, metrics on against metrics off, the window against the steps' own losses and against metrics.class_iou /
metrics.regr_iou, accumulation, and the command line.

Integer counts are compared exactly.  The bar for regr_iou = sum_iou / iou_rows is measured, per case, on the project's existing
float32 path: utils.regression_postprocess -> utils.iou -> a float64 mean on the host, against the float64 reference.  The kernel
runs that same float32 arithmetic and sums in float64, so its error may not exceed TWICE that error (the factor allows for another
instruction contraction of the same formula).  Both errors are printed per case (profiles/train_metrics_err.txt)."""
import math
import re

import numpy as np
import pytest
import torch

import train_metrics_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    return torch.device("cuda:0")


class _TableLevel(object):
    """What TrainMetrics.update asks of a level: its normalised anchor table."""

    def __init__(self, table):
        self.table = np.asarray(table, np.float32)

    def normalized_anchor_sizes(self, image_size, mode='trunc_int'):
        return self.table


def _tuples(case, dev):
    """The `detection_trainable` tuples losses.loss is given, from a tuple of train_metrics_ref.Level."""
    import utils
    keys = ['P%d' % (3 + i) for i in range(len(case))]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    labels = utils.DetectionTrainable(
        classification=utils.Classification(unscaled=None, prob={k: t(lv.label) for k, lv in zip(keys, case)}),
        regression={k: t(lv.reg_label) for k, lv in zip(keys, case)}, regression_postprocessed=None,
        trainable_masks={k: t(lv.mask) for k, lv in zip(keys, case)})
    logits = utils.DetectionTrainable(
        classification=utils.Classification(unscaled={k: t(lv.logit) for k, lv in zip(keys, case)}, prob=None),
        regression={k: t(lv.reg_pred) for k, lv in zip(keys, case)}, regression_postprocessed=None,
        trainable_masks=labels.trainable_masks)
    levels = {k: _TableLevel(lv.anchors) for k, lv in zip(keys, case)}
    return labels, logits, levels


def _scalar(v, dev):
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _step(tm, case, dev, losses=(0.75, 0.5, 0.125)):
    labels, logits, levels = _tuples(case, dev)
    tm.update(labels, logits, levels, (64, 64))
    tm.fold(*(_scalar(v, dev) for v in losses))
    return labels, logits, levels


def _float32_path_mean(case, dev):
    """The existing float32 path on the same inputs: utils.regression_postprocess -> utils.iou at the trainable foreground rows,
    then a float64 mean on the host (nan without rows)."""
    import utils
    vals = []
    for lv in case:
        sel = torch.from_numpy((lv.mask.reshape(-1) != 0) & (lv.label.reshape(-1, lv.label.shape[-1]).max(-1) > 0.5)).to(dev)
        anchors = torch.from_numpy(lv.anchors).to(dev)
        tb = utils.regression_postprocess(torch.from_numpy(lv.reg_label).to(dev), anchors).reshape(-1, 4)[sel]
        pb = utils.regression_postprocess(torch.from_numpy(lv.reg_pred).to(dev), anchors).reshape(-1, 4)[sel]
        vals.append(utils.iou(tb, pb).double().cpu().numpy())
    vals = np.concatenate(vals)
    return float(np.mean(vals)) if len(vals) else float("nan")


def _check_iou(got, want, path, what):
    """The bar of the module docstring; prints both errors."""
    e_kernel, e_path = abs(got - want), abs(path - want)
    print("train_metrics_err %s: kernel %.3e float32_path %.3e (regr_iou %.9f)" % (what, e_kernel, e_path, want))
    assert e_kernel <= 2.0 * e_path, (what, e_kernel, e_path)


SHAPE_SETS = {"five-levels": ref.SMALL_SHAPES, "many-blocks": ref.BIG_SHAPES}


@pytest.mark.parametrize("variant", ref.VARIANTS)
@pytest.mark.parametrize("num_classes", ref.CLASS_COUNTS)
@pytest.mark.parametrize("shapes", sorted(SHAPE_SETS))
def test_pass_and_fold_against_the_reference(dev, shapes, num_classes, variant):
    import metrics
    case = ref.make_case(SHAPE_SETS[shapes], num_classes, variant)
    want_step = ref.step_stats(case)
    window = ref.Window()
    assert window.add(want_step, 0.75, 0.5, 0.125)
    want = window.result()
    tm = metrics.TrainMetrics(dev)
    _step(tm, case, dev)
    sums, counts = tm.raw()
    assert counts.tolist() == window.counts.tolist(), (counts, window.counts)
    assert np.array_equal(sums[:4], window.sums[:4])
    got = tm.result()
    assert got["steps"] == 1 and got["nonfinite_steps"] == 0
    rows = int(window.counts[6])
    if variant == "untrainable":
        assert not counts[2:].any() and math.isnan(got["class_iou"]) and math.isnan(got["regr_iou"])
    elif variant == "no_foreground":
        assert rows == 0 and counts[2] + counts[3] > 0 and math.isnan(got["regr_iou"]) and got["class_iou"] == want["class_iou"]
    else:
        assert rows > 0 and got["class_iou"] == want["class_iou"]
        if variant == "all_foreground":
            assert rows == sum(lv.mask.size for lv in case)
        _check_iou(got["regr_iou"], want["regr_iou"], _float32_path_mean(case, dev), "%s C=%d %s" % (shapes, num_classes, variant))
    # result() reset the window
    sums, counts = tm.raw()
    assert not sums.any() and not counts.any()


@pytest.mark.parametrize("shapes", sorted(SHAPE_SETS))
@pytest.mark.parametrize("num_classes", [4, 36, 52, 80, 84, 100, 128, 132])
def test_every_four_aligned_kernel_against_the_reference(dev, shapes, num_classes):
    """C % 4 == 0 up to 128 takes one of eight kernels by its quads per lane: C = 4, 36, 52, 80 (the headline), 84, 100, 128 reach
    1, 3, 4, 5, 6, 7, 8 (test_pass_and_fold_against_the_reference's C = 20 is 2); C = 132 is past them, back on the general kernel
    with whole rows of 16-byte loads."""
    import metrics
    case = ref.make_case(SHAPE_SETS[shapes], num_classes, "mixed")
    window = ref.Window()
    assert window.add(ref.step_stats(case), 0.75, 0.5, 0.125)
    tm = metrics.TrainMetrics(dev)
    _step(tm, case, dev)
    sums, counts = tm.raw()
    assert counts.tolist() == window.counts.tolist(), (counts, window.counts)
    assert counts[6] > 0 and counts[5] > 0 and counts[3] > 0
    _check_iou(sums[4] / counts[6], window.result()["regr_iou"], _float32_path_mean(case, dev), "%s C=%d mixed" % (shapes, num_classes))


def test_the_partial_rows_are_allocated_once(dev):
    """The buffer the pass writes and the fold reads has its largest size from the start and is never replaced, whatever shapes
    come by: captured graphs of several input shapes hold its address."""
    import _rn
    import metrics
    tm = metrics.TrainMetrics(dev)
    ptr = tm.partial.data_ptr()
    assert tm.partial.numel() * 8 == _rn.TRAIN_METRICS_MAX_WORKSPACE_BYTES == 64 + 1024 * 64
    window = ref.Window()
    # (2, 64, 64) x 9 anchors = 73 728 rows at C = 3: 1152 blocks of 64 rows, past the 1024-block cap -- waves take a second pass
    for shapes in (ref.SMALL_SHAPES, ref.BIG_SHAPES, ((2, 64, 64),), ref.SMALL_SHAPES):
        case = ref.make_case(shapes, 3, "mixed")
        assert window.add(ref.step_stats(case), 0.75, 0.5, 0.125)
        _step(tm, case, dev)
        assert tm.partial.data_ptr() == ptr
        assert tm.raw()[1].tolist() == window.counts.tolist(), shapes
    assert tm.raw()[1][0] == 4
    with pytest.raises(_rn.RnError, match="before any update"):
        metrics.TrainMetrics(dev).fold(_scalar(1.0, dev), _scalar(1.0, dev), _scalar(1.0, dev))


def test_fold_three_steps_and_the_gate(dev):
    """Three steps of known scalars: the loss sums are float64 sums of the float32 scalars, exactly; the counts add up.  A NaN
    class loss, an inf regression loss and a step whose predicted scales (log h, log w) times 100 give a NaN IoU -- a height that
    overflows a float times a width that rounds to nothing, in some rows of the thousand -- each leave every sum and count
    bit-unchanged and advance nonfinite_steps; so does a regulariser of -inf.  reset zeroes everything."""
    import metrics
    tm = metrics.TrainMetrics(dev)
    window = ref.Window()
    scalars = [(0.1, 0.2, 0.3), (1e-3, 7.0, 1e4), (2.5, 1.0 / 3.0, 1e-7)]
    path_sum, path_rows = 0.0, 0
    for seed, losses in enumerate(scalars):
        case = ref.make_case(ref.SMALL_SHAPES, 3, "mixed", seed=seed)
        step = ref.step_stats(case)
        assert window.add(step, *losses)
        _step(tm, case, dev, losses)
        path_sum += _float32_path_mean(case, dev) * len(step.ious)
        path_rows += len(step.ious)
    sums, counts = tm.raw()
    assert counts.tolist() == window.counts.tolist() and counts[0] == 3
    assert np.array_equal(sums[:4], window.sums[:4])
    want = window.result()
    _check_iou(sums[4] / counts[6], want["regr_iou"], path_sum / path_rows, "three steps C=3 mixed")
    good = ref.make_case(ref.SMALL_SHAPES, 3, "mixed", seed=3)
    blown = ref.make_case(ref.SMALL_SHAPES, 3, "all_foreground", seed=3, pred_scale=100.0)
    nan, inf = float("nan"), float("inf")
    for i, (case, losses) in enumerate([(good, (nan, 0.5, 0.125)), (good, (0.75, inf, 0.125)), (blown, (0.75, 0.5, 0.125)),
                                        (good, (0.75, 0.5, -inf))]):
        _step(tm, case, dev, losses)
        s2, c2 = tm.raw()
        assert np.array_equal(s2.view(np.uint64), sums.view(np.uint64)), i
        assert c2[1] == i + 1 and c2[0] == 3 and np.array_equal(c2[2:], counts[2:]), (i, c2)
    got = tm.result(reset=False)
    assert got["steps"] == 3 and got["nonfinite_steps"] == 4
    assert got["class_loss"] == want["class_loss"] and got["total_loss"] == want["total_loss"] and got["class_iou"] == want["class_iou"]
    _step(tm, good, dev)                       # the window goes on after the left-out steps
    assert tm.raw()[1][0] == 4
    tm.reset()
    sums, counts = tm.raw()
    assert not sums.any() and not counts.any()


def test_entries_refuse_bad_arguments(dev):
    """Nothing is launched on a bad segment list, a workspace that is too small or a null pointer."""
    import ctypes
    import _rn
    import metrics
    L = _rn.lib()
    tm = metrics.TrainMetrics(dev)
    case = ref.make_case(ref.BIG_SHAPES, 3, "mixed")
    _step(tm, case, dev)
    before = tm.raw()
    labels, logits, levels = _tuples(case, dev)
    lv = case[0]
    anchors = torch.from_numpy(lv.anchors).to(dev)
    seg = _rn.MetricsSeg(_rn.f32(logits.classification.unscaled['P3']), _rn.f32(labels.classification.prob['P3']),
                         _rn.f32(logits.regression['P3']), _rn.f32(labels.regression['P3']),
                         _rn.ptr(labels.trainable_masks['P3']), _rn.f32(anchors), 2, 16, 16, 9)
    segs = (_rn.MetricsSeg * 1)(seg)
    need = L.rn_train_metrics_workspace(segs, 1, 3)
    assert need == 64 + 64 * ((2 * 16 * 16 * 9 + 63) // 64) and tm.partial.numel() * 8 >= need
    st = _rn.stream()
    assert L.rn_train_metrics_pass(segs, 1, 3, tm.partial.data_ptr(), need - 8, st) < 0
    assert L.rn_train_metrics_pass(segs, 0, 3, tm.partial.data_ptr(), need, st) < 0
    assert L.rn_train_metrics_pass(segs, 1, 0, tm.partial.data_ptr(), need, st) < 0
    assert L.rn_train_metrics_pass(segs, 1, 3, None, need, st) < 0
    bad = (_rn.MetricsSeg * 1)(seg)
    bad[0].anchor_sizes = None
    assert L.rn_train_metrics_pass(bad, 1, 3, tm.partial.data_ptr(), need, st) < 0 and L.rn_train_metrics_workspace(bad, 1, 3) == 0
    one = _scalar(1.0, dev)
    assert L.rn_train_metrics_fold(tm.partial.data_ptr(), 32, _rn.f32(one), _rn.f32(one), _rn.f32(one), tm.state.data_ptr(), st) < 0
    assert L.rn_train_metrics_fold(tm.partial.data_ptr(), need, None, _rn.f32(one), _rn.f32(one), tm.state.data_ptr(), st) < 0
    assert L.rn_train_metrics_reset(None, st) < 0
    after = tm.raw()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---------------------------------------------------------------------------------------------- trainer
BASE = 1e-2
SIZE = 256
STEPS = 4


def _build(dev, use_graph, train_metrics=True, **kw):
    """The recipe of test_gpu_guard._build (MobileNetV2, 4 classes, dropout 0.2, focal loss), scheduled Adam: two optimizer slots,
    the one-graph step."""
    import layers, levels as levels_mod, retinanet, train
    lv = levels_mod.build_levels()
    layers.Dropout._next_seed[0] = 0x5EED
    torch.manual_seed(4)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 4, layers.elu, 0.2).to(dev)
    if train_metrics:
        kw["train_metrics"] = True
    tr = train.Trainer(net, lv, optimizer="adam", learning_rate=BASE, loss_mode="focal", device=dev, use_graph=use_graph,
                       lr_schedule=train.LRSchedule("step", BASE, warmup_steps=2, boundaries=(4,)), **kw)
    return net, tr


def _features(dev, image, boxes):
    import dataset, levels as levels_mod
    lv = levels_mod.build_levels()
    cids = torch.tensor([[1, 3]], dtype=torch.int32, device=dev)
    c, r, m = dataset.build_labels(tuple(image.shape[1:3]), cids, torch.tensor([boxes], device=dev), lv, 4, flip_pair=True)
    return {"image": image, "detection": {"classifications": c, "regressions": r}, "trainable_masks": m}


@pytest.fixture(scope="module")
def feats(dev):
    rng = np.random.default_rng(2)
    image = torch.from_numpy(rng.standard_normal((2, SIZE, SIZE, 3)).astype(np.float32)).to(dev)
    return _features(dev, image, [[0.1, 0.2, 0.7, 0.8], [0.4, 0.1, 0.9, 0.5]])


def _run(dev, feats, use_graph, train_metrics=True, **kw):
    """STEPS steps; the steps' own float32 losses (read after each step: `regularization_loss` is a view of the live word), the
    optimizer's state and the metrics' raw state at the end."""
    _, tr = _build(dev, use_graph, train_metrics, **kw)
    losses = []
    for _ in range(STEPS):
        out = tr.step(feats)
        losses.append(tuple(np.float32(out[k].item()) for k in ("class_loss", "regr_loss", "regularization_loss")))
    torch.cuda.synchronize()
    o = tr.opt
    state = {"weights": tr.arena.weights.clone(), "state1": o.state1.clone(), "state2": o.state2.clone(),
             "drop_counter": tr.drop_counter.clone()}
    return {"trainer": tr, "losses": losses, "state": state, "raw": tr.metrics.raw() if train_metrics else None}


@pytest.fixture(scope="module")
def graph_run(dev, feats):
    return _run(dev, feats, True)


def _same(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_one_graph_equals_eager(dev, feats, graph_run):
    """Four steps with the metrics in ONE captured graph against the same four steps launched eagerly: the whole metrics state
    and the weights are bit-identical."""
    tr = graph_run["trainer"]
    assert tr._graphs[5] and len(tr._graph_cache) == 1 and tr.recaptures == 0
    eager = _run(dev, feats, False)
    assert np.array_equal(graph_run["raw"][0].view(np.uint64), eager["raw"][0].view(np.uint64))
    assert np.array_equal(graph_run["raw"][1], eager["raw"][1])
    assert graph_run["raw"][1][0] + graph_run["raw"][1][1] == STEPS
    assert _same(graph_run["state"]["weights"], eager["state"]["weights"])
    assert graph_run["losses"] == eager["losses"]


def test_metrics_only_observe(dev, feats, graph_run):
    """Weights, both optimizer slots and the dropout counter after four steps with the metrics are those without them."""
    import ops
    off = _run(dev, feats, True, train_metrics=False)
    assert off["trainer"].metrics is None and off["trainer"]._graphs[5]
    for k in ("weights", "state1", "state2", "drop_counter"):
        assert _same(graph_run["state"][k], off["state"][k]), k
    assert graph_run["state"]["drop_counter"].item() == STEPS * ops.DROPOUT_COUNTER_STEP
    assert graph_run["losses"] == off["losses"]


def test_window_means_are_the_steps_losses(graph_run):
    """The window's loss means equal the float64 mean of the four steps' returned float32 losses, exactly."""
    import metrics
    sums, counts = graph_run["raw"]
    assert counts[0] == STEPS and counts[1] == 0
    want = np.zeros(4)
    for cl, rl, rg in graph_run["losses"]:
        cl, rl, rg = np.float64(cl), np.float64(rl), np.float64(rg)
        want += [(cl + rl) + rg, cl, rl, rg]
    assert np.array_equal(sums[:4], want)
    res = metrics.window_result(sums, counts)
    assert (res["total_loss"], res["class_loss"], res["regr_loss"], res["regularization_loss"]) == tuple(want / STEPS)


def test_window_ious_are_the_evaluation_metrics(dev, feats, graph_run, monkeypatch):
    """class_iou / regr_iou of the window against metrics.class_iou / metrics.regr_iou on the same four steps' logits and labels,
    recomputed on a second trainer without the metrics: forward_backward(advance_dropout=False) shows the step's logits
    (losses.loss is watched), the step() that follows repeats that forward pass and updates.  Counts exact, IoU to the bar of the
    module docstring."""
    import losses
    import metrics
    import utils
    _, tr = _build(dev, False, train_metrics=False)
    seen = []
    real = losses.loss

    def watched(labels, logits, **kw):
        seen.append((labels, logits))
        return real(labels=labels, logits=logits, **kw)
    monkeypatch.setattr(losses, "loss", watched)
    lv = tr.levels
    all_labels, all_probs, path_ious, ref_steps = [], [], [], []
    for _ in range(STEPS):
        del seen[:]
        tr.forward_backward(feats, advance_dropout=False)
        labels, logits = seen[0]
        case = []
        for k in logits.regression.keys():
            z = logits.classification.unscaled[k].detach()
            l, m = labels.classification.prob[k], labels.trainable_masks[k].bool()
            sel = m.reshape(-1)
            zl, ll = z.reshape(-1, z.shape[-1])[sel], l.reshape(-1, l.shape[-1])[sel]
            all_labels.append(ll.cpu().numpy().reshape(-1))
            all_probs.append(1.0 / (1.0 + np.exp(-zl.double().cpu().numpy().reshape(-1))))
            fg = ll.max(-1).values > 0.5
            anchors = lv[k].normalized_anchor_sizes((SIZE, SIZE), utils.ANCHOR_SIZE_MODE)
            tb = utils.regression_postprocess(labels.regression[k], anchors).reshape(-1, 4)[sel][fg]
            pb = utils.regression_postprocess(logits.regression[k].detach(), anchors).reshape(-1, 4)[sel][fg]
            path_ious.append(utils.iou(tb, pb).double().cpu().numpy())          # the existing float32 path
            case.append(ref.Level(z.cpu().numpy(), l.cpu().numpy(), logits.regression[k].detach().cpu().numpy(),
                                  labels.regression[k].cpu().numpy(), m.cpu().numpy().astype(np.uint8), anchors))
        ref_steps.append(ref.step_stats(case))
        tr.step(feats)
    monkeypatch.setattr(losses, "loss", real)
    torch.cuda.synchronize()
    assert _same(tr.arena.weights, graph_run["state"]["weights"])          # the second trainer walked the same four states
    sums, counts = graph_run["raw"]
    window = ref.Window()
    for s, (cl, rl, rg) in zip(ref_steps, graph_run["losses"]):
        assert window.add(s, cl, rl, rg)
    assert counts.tolist() == window.counts.tolist()
    assert counts[5] + counts[4] > 0 and counts[6] > 0                      # positives and foreground rows were there
    got = metrics.window_result(sums, counts)
    assert got["class_iou"] == metrics.class_iou(np.concatenate(all_labels), np.concatenate(all_probs))
    want = metrics.regr_iou(np.concatenate([s.label_boxes for s in ref_steps]), np.concatenate([s.pred_boxes for s in ref_steps]))
    assert abs(want - window.result()["regr_iou"]) < 1e-12                  # (float64 boxes: the evaluation's definition is the window's)
    _check_iou(got["regr_iou"], want, float(np.mean(np.concatenate(path_ious))), "trainer, four steps")


class _TwoShapeFeed(object):
    """What Trainer.step asks of a feed (dataset.DeviceFeed): stage() names the coming step's input shape -- one graph set per
    name --, the call returns that shape's static tensors, consumed() moves on."""

    def __init__(self, by_shape, order):
        self.by_shape, self.order, self.i = by_shape, order, 0

    def stage(self):
        return self.order[self.i]

    def __call__(self):
        return self.by_shape[self.order[self.i]]

    def consumed(self):
        self.i += 1


def test_two_input_shapes_under_one_trainer(dev):
    """A ragged feed alternates two network input shapes, the smaller first: the trainer keeps one captured graph per shape, and
    both hold the address of the metrics' partial rows.  Six steps small, large, small, large, small, large as graphs against the
    same six launched eagerly: the metrics state and the weights are bit-identical, every step is counted, and the buffer is the
    one the trainer started with."""
    rng = np.random.default_rng(5)
    boxes = [[0.1, 0.2, 0.7, 0.8], [0.4, 0.1, 0.9, 0.5]]
    by_shape = {}
    for h, w in ((128, 256), (SIZE, SIZE)):
        image = torch.from_numpy(rng.standard_normal((2, h, w, 3)).astype(np.float32)).to(dev)
        by_shape[(h, w)] = _features(dev, image, boxes)
    order = [(128, 256), (SIZE, SIZE)] * 3
    runs = {}
    for use_graph in (True, False):
        _, tr = _build(dev, use_graph, input_fn=_TwoShapeFeed(by_shape, order))
        ptr = tr.metrics.partial.data_ptr()
        for _ in order:
            tr.step()
        torch.cuda.synchronize()
        assert tr.metrics.partial.data_ptr() == ptr
        runs[use_graph] = (tr.metrics.raw(), tr.arena.weights.clone(), tr)
    tg = runs[True][2]
    assert len(tg._graph_cache) == 2 and tg.recaptures == 1 and tg._graphs[5]
    (gs, gc), (es, ec) = runs[True][0], runs[False][0]
    assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)) and np.array_equal(gc, ec)
    assert gc[0] + gc[1] == len(order) and gc[0] == len(order) and gc[6] > 0
    assert _same(runs[True][1], runs[False][1])


def test_every_micro_step_counts(dev, feats):
    """accumulate_steps = 2: four micro-steps are four steps of the window (two updates), still one graph."""
    _, tr = _build(dev, True, accumulate_steps=2)
    for _ in range(4):
        tr.step(feats)
    res = tr.train_metrics()
    assert res["steps"] + res["nonfinite_steps"] == 4 and res["steps"] == 4
    assert tr._graphs[5] and len(tr._graph_cache) == 1 and tr.recaptures == 0 and tr.opt.step_count == 2
    assert tr.train_metrics()["steps"] == 0                                 # the read reset the window


def test_cli_appends_the_window_to_the_log_line(tmp_path, capsys):
    """--train-metrics: the 20-step line starts with the existing text and ends with the window's means over 20 steps; the step is
    still one graph, captured once."""
    import train
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "20", "--scale", "128", "--experiment", str(tmp_path / "exp"),
            "--backbone", "mobilenet_v2", "--dropout", "0.1", "--train-metrics"]
    assert train.main(argv) == 20
    assert train.LAST_RUN["graph_sets"] == 1 and train.LAST_RUN["recaptures"] == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch 0 step 20 ")]
    assert len(lines) == 1, lines
    num = r"-?\d+\.\d{4}"
    m = re.match(r"^epoch 0 step 20 class_loss (%s) regr_loss (%s) reg (%s) lr \S+ \| mean total (%s) class (%s) regr (%s) reg (%s) "
                 r"class_iou (%s) regr_iou (%s) over 20 steps$" % ((num,) * 9), lines[0])
    assert m, lines[0]
    total, cl, rl, rg, ciou, riou = (float(v) for v in m.groups()[3:])
    assert abs(total - (cl + rl + rg)) <= 2e-4 and 0.0 <= ciou <= 1.0 and 0.0 <= riou <= 1.0
