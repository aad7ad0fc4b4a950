"""The running training metrics (train_metrics=True) in float64 / numpy, for the tests, written from their definition -- the
reference's build_metrics (train.py:137-161) -- and not from csrc/train_metrics.hip:

    per step, over the rows with trainable != 0 of every level:
      confusion  label positive iff label > 0.5, prediction positive iff sigmoid(logit) > 0.5, over the row's C elements
                 -> (tn, fp, fn, tp)
      box IoU    at the rows whose max_c label > 0.5: the label and the predicted regression decoded (utils.py:22-44,100-117) and
                 utils.iou (utils.py:62-97) of the two boxes -> a list of IoUs
    gate         a step is added only if class_loss, regr_loss, the regulariser and the step's IoU sum are all finite; otherwise
                 nonfinite_steps advances and nothing else
    window       totals first, ratios last: loss means = sum / steps; class_iou = mean over the classes {0, 1} with a non-zero
                 union of inter / union (tf.metrics.mean_iou); regr_iou = sum_iou / iou_rows; nan at a zero denominator

Also the inputs of the device tests (make_case), drawn here so that every test of a case sees the same arrays."""
import collections
import functools

import numpy as np

NUM_ANCHORS = 9
SMALL_SHAPES = ((2, 5, 7), (2, 3, 4), (2, 2, 3), (2, 1, 2), (2, 1, 1))     # five levels: odd, non-square, one smaller than a wave
BIG_SHAPES = ((2, 16, 16),)                                                # 4608 rows: many blocks, many partial rows
CLASS_COUNTS = (1, 3, 20)
VARIANTS = ("mixed", "untrainable", "no_foreground", "all_foreground")

Level = collections.namedtuple("Level", "logit label reg_pred reg_label mask anchors")


def decode(regression, anchors):
    """utils.regression_postprocess (utils.py:100-117 over :22-44) in float64: [n,h,w,A,4] (dy, dx, log h, log w) and the
    normalised anchor (h, w) table [A,2] -> corners [y1, x1, y2, x2]."""
    r = np.asarray(regression, np.float64)
    a = np.asarray(anchors, np.float64)
    n, h, w, na, _ = r.shape
    assert a.shape == (na, 2)
    shifts, scales = r[..., :2], np.exp(r[..., 2:])
    scaled = np.concatenate([shifts, scales], -1) * np.tile(a, (1, 2)).reshape(1, 1, 1, na, 4)          # scale_regression
    ys = np.linspace((1.0 / h) / 2, 1 - (1.0 / h) / 2, h)                                                 # :22-36
    xs = np.linspace((1.0 / w) / 2, 1 - (1.0 / w) / 2, w)
    gx, gy = np.meshgrid(xs, ys)
    pos = scaled[..., :2] + np.stack([gy, gx], -1)[None, :, :, None, :]
    half = scaled[..., 2:] / 2                                                                           # :39-44
    return np.concatenate([pos - half, pos + half], -1)


def iou(a, b):
    """utils.iou (utils.py:62-97) in float64, element-wise over [..., 4]: 0 where the intersection is inverted."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    y_top, x_left = np.maximum(a[..., 0], b[..., 0]), np.maximum(a[..., 1], b[..., 1])
    y_bottom, x_right = np.minimum(a[..., 2], b[..., 2]), np.minimum(a[..., 3], b[..., 3])
    invalid = (y_bottom < y_top) | (x_right < x_left)
    inter = (y_bottom - y_top) * (x_right - x_left)
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = inter / (area_a + area_b - inter)
    return np.where(invalid, 0.0, v)


Step = collections.namedtuple("Step", "tn fp fn tp ious label_boxes pred_boxes labels probs")


def step_stats(levels):
    """One step over a list of Level: the confusion counts, the IoU of every foreground row in level / row order, and what
    metrics.class_iou / metrics.regr_iou take for the same step (the trainable labels and probabilities, the two box lists)."""
    tn = fp = fn = tp = 0
    ious, lab_boxes, pred_boxes, labels, probs = [], [], [], [], []
    for lv in levels:
        mask = np.asarray(lv.mask).reshape(-1) != 0
        c = lv.logit.shape[-1]
        z = np.asarray(lv.logit, np.float64).reshape(-1, c)[mask]
        l = np.asarray(lv.label, np.float64).reshape(-1, c)[mask]
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-z))
        lab, pred = l > 0.5, p > 0.5
        tn += int(np.sum(~lab & ~pred)); fp += int(np.sum(~lab & pred))
        fn += int(np.sum(lab & ~pred)); tp += int(np.sum(lab & pred))
        labels.append(l.reshape(-1)); probs.append(p.reshape(-1))
        fg = l.max(-1) > 0.5 if len(l) else np.zeros(0, bool)
        with np.errstate(over="ignore", invalid="ignore"):
            tb = decode(lv.reg_label, lv.anchors).reshape(-1, 4)[mask][fg]
            pb = decode(lv.reg_pred, lv.anchors).reshape(-1, 4)[mask][fg]
            ious.extend(iou(tb, pb).tolist())
        lab_boxes.append(tb); pred_boxes.append(pb)
    return Step(tn, fp, fn, tp, ious, np.concatenate(lab_boxes), np.concatenate(pred_boxes), np.concatenate(labels),
                np.concatenate(probs))


class Window(object):
    """The window state and its rules.  sums = [total, class, regr, reg, iou], counts = [steps, nonfinite, tn, fp, fn, tp, rows]."""

    def __init__(self):
        self.sums = np.zeros(5, np.float64)
        self.counts = np.zeros(7, np.int64)

    def add(self, step, class_loss, regr_loss, reg_loss):
        """The three losses are the step's float32 scalars; every sum is a float64 sum of them."""
        cl, rl, rg = (np.float64(np.float32(v)) for v in (class_loss, regr_loss, reg_loss))
        with np.errstate(invalid="ignore", over="ignore"):
            s_iou = np.float64(0.0)
            for v in step.ious:
                s_iou += v
        if not (np.isfinite(cl) and np.isfinite(rl) and np.isfinite(rg) and np.isfinite(s_iou)):
            self.counts[1] += 1
            return False
        self.sums += [(cl + rl) + rg, cl, rl, rg, s_iou]
        self.counts += [1, 0, step.tn, step.fp, step.fn, step.tp, len(step.ious)]
        return True

    def result(self):
        steps, nonfinite, tn, fp, fn, tp, rows = (int(v) for v in self.counts)
        nan = float("nan")
        per_class = [inter / union for inter, union in ((tn, tn + fp + fn), (tp, tp + fp + fn)) if union > 0]
        return {"total_loss": self.sums[0] / steps if steps else nan, "class_loss": self.sums[1] / steps if steps else nan,
                "regr_loss": self.sums[2] / steps if steps else nan, "regularization_loss": self.sums[3] / steps if steps else nan,
                "class_iou": float(np.mean(per_class)) if per_class else nan, "regr_iou": self.sums[4] / rows if rows else nan,
                "steps": steps, "nonfinite_steps": nonfinite}


def anchor_table(level_index):
    """A normalised [9,2] anchor (h, w) table per level: three ratios x three scales around a size that doubles per level."""
    base = 0.06 * 2 ** level_index
    rows = [(base * s * np.sqrt(r), base * s / np.sqrt(r)) for r in (0.5, 1.0, 2.0) for s in (1.0, 2 ** (1 / 3), 2 ** (2 / 3))]
    return np.asarray(rows, np.float32)


@functools.lru_cache(maxsize=None)
def make_case(shapes, num_classes, variant, seed=0, pred_scale=1.0):
    """A step's levels: logits +-U[1e-3, 4], regression targets and predictions U[-1, 1], one-hot labels on about a fifth of the
    rows, about three quarters of the rows trainable; the variants replace the masks / labels.  pred_scale multiplies the
    predicted SCALES (log h, log w: the `scales` half of utils.py:110): at 100 a float32 height overflows (log h > 88.7) beside a
    width that rounds to nothing against its centre (log w < -15), inf x 0, in a few rows of a hundred -- float64 does neither."""
    assert variant in VARIANTS
    rng = np.random.default_rng([seed, num_classes, len(shapes), VARIANTS.index(variant)])
    levels = []
    for i, (n, h, w) in enumerate(shapes):
        shape = (n, h, w, NUM_ANCHORS)
        rows = int(np.prod(shape))
        mag = rng.uniform(1e-3, 4.0, shape + (num_classes,))
        logit = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
        label = np.zeros((rows, num_classes), np.float32)
        if variant == "all_foreground":
            fg = np.ones(rows, bool)
        elif variant == "no_foreground":
            fg = np.zeros(rows, bool)
        else:
            fg = rng.random(rows) < 0.2
        label[np.nonzero(fg)[0], rng.integers(0, num_classes, int(fg.sum()))] = 1.0
        mask = np.zeros(rows, np.uint8) if variant == "untrainable" else (rng.random(rows) < 0.75).astype(np.uint8)
        if variant == "all_foreground":
            mask[:] = 1
        reg_label = rng.uniform(-1.0, 1.0, shape + (4,)).astype(np.float32)
        reg_pred = (rng.uniform(-1.0, 1.0, shape + (4,)) * np.asarray([1.0, 1.0, pred_scale, pred_scale])).astype(np.float32)
        levels.append(Level(logit, label.reshape(shape + (num_classes,)), reg_pred, reg_label, mask.reshape(shape), anchor_table(i)))
    assert all(np.abs(lv.logit).min() >= 1e-3 for lv in levels)
    return tuple(levels)
