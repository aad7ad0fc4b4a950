"""The running training metrics without a GPU: the float64 reference (train_metrics_ref.py) against hand-computed cases and
against metrics.class_iou / metrics.regr_iou (the evaluation's definitions: training and evaluation must stay one), the
finiteness gate over a two-step window, the host's totals-then-ratio rules (metrics.window_result), the command line, and the
refusal of a CPU arena."""
import math
import os
import re

import numpy as np
import pytest
import torch

import train_metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rn_train_metrics_workspace", "rn_train_metrics_pass", "rn_train_metrics_fold", "rn_train_metrics_reset")
ANCHORS = np.asarray([[0.2, 0.3]], np.float32)


def _level(logit, label, mask=None, reg_pred=None, reg_label=None):
    """One level of one 1 x 1 map per row: rows of [C] logits / labels as [rows,1,1,1,C]."""
    logit, label = np.asarray(logit, np.float32), np.asarray(label, np.float32)
    rows, c = logit.shape
    shape = (rows, 1, 1, 1)
    zeros = np.zeros(shape + (4,), np.float32)
    return ref.Level(logit.reshape(shape + (c,)), label.reshape(shape + (c,)),
                     zeros if reg_pred is None else np.asarray(reg_pred, np.float32).reshape(shape + (4,)),
                     zeros if reg_label is None else np.asarray(reg_label, np.float32).reshape(shape + (4,)),
                     np.ones(shape, np.uint8) if mask is None else np.asarray(mask, np.uint8).reshape(shape), ANCHORS)


def _window(levels, losses=(1.0, 0.5, 0.25)):
    w = ref.Window()
    w.add(ref.step_stats(levels), *losses)
    return w


def _result(w):
    """The reference's result -- and the host's rule (metrics.window_result) over the same totals gives the same, nan for nan."""
    import metrics
    want, got = w.result(), metrics.window_result(w.sums, w.counts)
    assert want.keys() == got.keys()
    for k in want:
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), (k, got[k], want[k])
    return want


def test_all_correct_gives_class_iou_one():
    lv = _level([[2.0, -1.0], [-3.0, -0.5], [-1.0, 4.0]], [[1, 0], [0, 0], [0, 1]])
    s = ref.step_stats([lv])
    assert (s.tn, s.fp, s.fn, s.tp) == (4, 0, 0, 2)
    assert _result(_window([lv]))["class_iou"] == 1.0


def test_all_predicted_negative_with_some_positives():
    """tn = 4, fn = 2: class 0 has inter tn and union tn + fn, class 1 has inter 0 and union fn: mean(4 / 6, 0)."""
    lv = _level([[-2.0, -1.0], [-3.0, -0.5], [-1.0, -4.0]], [[1, 0], [0, 0], [0, 1]])
    s = ref.step_stats([lv])
    assert (s.tn, s.fp, s.fn, s.tp) == (4, 0, 2, 0)
    assert _result(_window([lv]))["class_iou"] == (4 / 6 + 0.0) / 2


def test_no_positives_and_none_predicted_leaves_one_class():
    lv = _level([[-2.0, -1.0], [-3.0, -0.5]], [[0, 0], [0, 0]])
    r = _result(_window([lv]))
    assert r["class_iou"] == 1.0 and math.isnan(r["regr_iou"])             # class 1 absent: the mean is class 0's alone


def test_untrainable_rows_are_not_counted():
    lv = _level([[2.0], [2.0], [-2.0]], [[1], [0], [1]], mask=[1, 0, 0])
    s = ref.step_stats([lv])
    assert (s.tn, s.fp, s.fn, s.tp) == (0, 0, 0, 1) and len(s.ious) == 1
    empty = ref.step_stats([_level([[2.0]], [[1]], mask=[0])])
    w = ref.Window()
    assert w.add(empty, 1.0, 1.0, 1.0)
    r = _result(w)
    assert math.isnan(r["class_iou"]) and math.isnan(r["regr_iou"]) and r["steps"] == 1


def test_identical_and_disjoint_boxes():
    same = _level([[3.0]], [[1]], reg_pred=[[0.3, -0.2, 0.1, 0.4]], reg_label=[[0.3, -0.2, 0.1, 0.4]])
    assert _result(_window([same]))["regr_iou"] == 1.0
    # anchors (0.2, 0.3) at the centre (0.5, 0.5): a shift of +-1 anchor height apart, unit scale: the boxes do not touch
    apart = _level([[3.0]], [[1]], reg_pred=[[1.0, 0.0, 0.0, 0.0]], reg_label=[[-1.0, 0.0, 0.0, 0.0]])
    assert _result(_window([apart]))["regr_iou"] == 0.0
    # half an anchor height apart: intersection h / 2 x w, union 3 h / 2 x w
    half = _level([[3.0]], [[1]], reg_pred=[[0.25, 0.0, 0.0, 0.0]], reg_label=[[-0.25, 0.0, 0.0, 0.0]])
    assert abs(_result(_window([half]))["regr_iou"] - 1 / 3) < 1e-6       # (the float32 anchor table: 0.2 is not exact)
    # zero regression decodes to the anchors on the cell centres (utils.py:22-44): h = 2, w = 3
    boxes = ref.decode(np.zeros((1, 2, 3, 1, 4)), ANCHORS)
    ah, aw = np.float64(ANCHORS[0, 0]), np.float64(ANCHORS[0, 1])
    for y, cy in enumerate((0.25, 0.75)):
        for x, cx in enumerate((1 / 6, 0.5, 5 / 6)):
            np.testing.assert_allclose(boxes[0, y, x, 0], [cy - ah / 2, cx - aw / 2, cy + ah / 2, cx + aw / 2], rtol=0, atol=1e-15)


@pytest.mark.parametrize("num_classes", ref.CLASS_COUNTS)
def test_reference_agrees_with_the_evaluation_metrics(num_classes):
    """One step of the device tests' inputs: the window's class_iou / regr_iou are metrics.class_iou / metrics.regr_iou of the
    same trainable labels, probabilities and decoded boxes."""
    import metrics
    s = ref.step_stats(ref.make_case(ref.SMALL_SHAPES, num_classes, "mixed"))
    assert s.tp + s.fn > 0 and s.tn + s.fp > 0 and len(s.ious) > 10
    w = ref.Window()
    assert w.add(s, 0.7, 0.3, 0.1)
    r = w.result()
    assert abs(r["class_iou"] - metrics.class_iou(s.labels, s.probs)) < 1e-15
    assert abs(r["regr_iou"] - metrics.regr_iou(s.label_boxes, s.pred_boxes)) < 1e-12
    assert 0.0 < r["regr_iou"] < 1.0
    # and the host's rule over the same totals
    got = metrics.window_result(w.sums, w.counts)
    assert got == r


def test_a_nonfinite_step_is_left_out_of_the_window():
    """Step 2 has regr_loss = inf: the means are step 1's, nonfinite_steps == 1; so for a NaN class loss and a NaN IoU."""
    import metrics
    s1 = ref.step_stats(ref.make_case(ref.SMALL_SHAPES, 3, "mixed"))
    s2 = ref.step_stats(ref.make_case(ref.SMALL_SHAPES, 3, "mixed", seed=1))
    w = ref.Window()
    assert w.add(s1, 0.75, 0.5, 0.125)
    before = (w.sums.copy(), w.counts.copy())
    assert not w.add(s2, 0.6, float("inf"), 0.125)
    r = w.result()
    assert r["steps"] == 1 and r["nonfinite_steps"] == 1
    assert (r["total_loss"], r["class_loss"], r["regr_loss"], r["regularization_loss"]) == (1.375, 0.75, 0.5, 0.125)
    assert np.array_equal(w.sums, before[0]) and np.array_equal(w.counts[2:], before[1][2:])
    assert not w.add(s2, float("nan"), 0.5, 0.125)
    # (a NaN IoU is float32's: a predicted height that overflows times a width that rounds to nothing, test_gpu_train_metrics.py;
    # float64 does not overflow there, so the list is poisoned by hand)
    assert not w.add(s2._replace(ious=s2.ious[:3] + [float("nan")] + s2.ious[3:]), 0.6, 0.5, 0.125)
    assert w.result()["nonfinite_steps"] == 3 and np.array_equal(w.sums, before[0])
    assert metrics.window_result(w.sums, w.counts) == w.result()
    empty = metrics.window_result(np.zeros(5), np.zeros(7, np.int64))
    assert all(math.isnan(empty[k]) for k in ("total_loss", "class_loss", "regr_loss", "regularization_loss", "class_iou", "regr_iou"))
    assert empty["steps"] == 0 == empty["nonfinite_steps"]


def test_float32_losses_sum_in_float64():
    w = ref.Window()
    s = ref.step_stats(ref.make_case(ref.SMALL_SHAPES, 1, "mixed"))
    vals = [(0.1, 0.2, 0.3), (1e-3, 7.0, 1e4)]
    for v in vals:
        w.add(s, *v)
    f = lambda x: np.float64(np.float32(x))
    assert w.sums[0] == ((f(0.1) + f(0.2)) + f(0.3)) + ((f(1e-3) + f(7.0)) + f(1e4)) and w.sums[1] == f(0.1) + f(1e-3)
    assert _result(w)["class_loss"] == (f(0.1) + f(1e-3)) / 2


def test_flag_parses_and_the_suffix_is_the_documented_text():
    import train
    p = train.build_parser()
    assert p.parse_args(["--dataset", "shapes"]).train_metrics is False
    assert p.parse_args(["--dataset", "shapes", "--train-metrics"]).train_metrics is True
    res = {"total_loss": 1.5, "class_loss": 1.0, "regr_loss": 0.25, "regularization_loss": 0.25, "class_iou": 0.5, "regr_iou": 0.125,
           "steps": 20, "nonfinite_steps": 0}
    assert train.train_metrics_suffix(res) == (" | mean total 1.5000 class 1.0000 regr 0.2500 reg 0.2500 class_iou 0.5000 "
                                               "regr_iou 0.1250 over 20 steps")
    assert train.train_metrics_suffix({**res, "steps": 18, "nonfinite_steps": 2}).endswith(" over 18 steps (2 non-finite left out)")


def test_train_metrics_need_a_device_arena():
    import _rn
    import metrics
    import train
    mod = torch.nn.Module()
    mod.p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(_rn.RnError, match="device arena"):
        train.Trainer(mod, device="cpu", train_metrics=True)
    with pytest.raises(_rn.RnError, match="device arena"):
        metrics.TrainMetrics("cpu")
    tr = train.Trainer(mod, device="cpu")
    assert tr.metrics is None
    with pytest.raises(ValueError, match="train_metrics=True"):
        tr.train_metrics()


def test_header_and_bindings_declare_the_entries():
    import ctypes
    import _rn
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    raw = ctypes.CDLL(_rn.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), sym
        assert sym in _rn.SYMBOLS and re.search(r"\b(int|size_t) %s\(" % sym, hdr), sym
    assert ctypes.sizeof(_rn.MetricsSeg) == 6 * 8 + 4 * 4
    assert int(re.search(r"#define RN_TRAIN_METRICS_STATE_BYTES (\d+)", hdr).group(1)) == _rn.TRAIN_METRICS_STATE_BYTES == (5 + 7) * 8
    assert (int(re.search(r"#define RN_TRAIN_METRICS_MAX_WORKSPACE_BYTES (\d+)", hdr).group(1))
            == _rn.TRAIN_METRICS_MAX_WORKSPACE_BYTES == 64 + 1024 * 64)
    for cite in ("train.py:137-161", "utils.py:62-97", "utils.py:108-117", "utils.py:183-195"):
        assert cite in hdr, cite
