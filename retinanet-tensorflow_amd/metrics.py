"""Evaluation the reference only sketches: COCO-style mean average precision over the detections
of `utils.detect`, and the two IoU metrics of the reference's `build_metrics` (train.py:137-161): `class_iou`
(tf.metrics.mean_iou, 2 classes, of the thresholded class probabilities) and `regr_iou` (mean IoU between the
decoded ground-truth and predicted boxes at the foreground anchors).  Host-side numpy on copies of the device
results: evaluation is not on the training hot path.  `TrainMetrics` keeps the same two definitions, and the means of the
losses, as running totals on the device DURING training (csrc/train_metrics.hip; train.Trainer(train_metrics=True))."""
import numpy as np


def iou_matrix(a, b):
    """IoU of corner boxes a [K,4] x b [O,4] ([y1,x1,y2,x2]); empty / inverted intersections count 0 (utils.py:62-97)."""
    a = np.asarray(a, np.float64).reshape(-1, 1, 4)
    b = np.asarray(b, np.float64).reshape(1, -1, 4)
    tl = np.maximum(a[..., :2], b[..., :2])
    br = np.minimum(a[..., 2:], b[..., 2:])
    inter = np.prod(np.maximum(br - tl, 0.0), -1)
    area_a = np.prod(np.maximum(a[..., 2:] - a[..., :2], 0.0), -1)
    area_b = np.prod(np.maximum(b[..., 2:] - b[..., :2], 0.0), -1)
    union = area_a + area_b - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def average_precision(tp, scores, num_gt):
    """COCO 101-point interpolated AP of one (class, IoU threshold): tp flags of the detections, their scores."""
    if num_gt == 0:
        return np.nan
    order = np.argsort(-np.asarray(scores, np.float64), kind='mergesort')
    tp = np.asarray(tp, np.float64)[order]
    ctp, cfp = np.cumsum(tp), np.cumsum(1.0 - tp)
    recall = ctp / num_gt
    precision = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
    for i in range(len(precision) - 1, 0, -1):                  # precision envelope
        precision[i - 1] = max(precision[i - 1], precision[i])
    points = np.linspace(0.0, 1.0, 101)
    idx = np.searchsorted(recall, points, side='left')
    return float(np.mean([precision[i] if i < len(precision) else 0.0 for i in idx]))


def mean_average_precision(detections, ground_truth, num_classes, iou_thresholds=None):
    """detections: per image (boxes [K,4], scores [K], class_ids [K]); ground_truth: per image (boxes [O,4], class_ids [O]).
    Returns {'mAP' (IoU 0.50:0.95), 'AP50', 'AP75', 'per_class' [C] (mean over thresholds; nan = class absent)}."""
    thr = np.arange(0.5, 0.96, 0.05) if iou_thresholds is None else np.asarray(iou_thresholds, np.float64)
    ap = np.full((num_classes, len(thr)), np.nan)
    for c in range(num_classes):
        per_image, num_gt = [], 0
        for (db, ds, dc), (gb, gc) in zip(detections, ground_truth):
            dsel = np.asarray(dc) == c
            gsel = np.asarray(gc) == c
            num_gt += int(gsel.sum())
            per_image.append((np.asarray(db, np.float64).reshape(-1, 4)[dsel], np.asarray(ds, np.float64)[dsel],
                              np.asarray(gb, np.float64).reshape(-1, 4)[gsel]))
        if num_gt == 0:
            continue
        for t, th in enumerate(thr):
            tps, scs = [], []
            for db, ds, gb in per_image:
                order = np.argsort(-ds, kind='mergesort')
                ious = iou_matrix(db[order], gb) if len(gb) and len(db) else np.zeros((len(db), len(gb)))
                taken = np.zeros(len(gb), bool)
                for i in range(len(order)):
                    best, bj = th, -1
                    for j in range(len(gb)):                     # best still-free ground truth at or above the threshold
                        if not taken[j] and ious[i, j] >= best:
                            best, bj = ious[i, j], j
                    if bj >= 0:
                        taken[bj] = True
                    tps.append(1.0 if bj >= 0 else 0.0)
                    scs.append(ds[order][i])
            ap[c, t] = average_precision(tps, scs, num_gt) if len(tps) else 0.0
    def col(v):
        k = int(np.argmin(np.abs(thr - v)))
        return float(np.nanmean(ap[:, k])) if abs(thr[k] - v) < 1e-9 and np.any(~np.isnan(ap[:, k])) else float('nan')
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # classes without ground truth stay nan
        per_class = np.nanmean(ap, 1)
    return {'mAP': float(np.nanmean(ap)) if np.any(~np.isnan(ap)) else float('nan'), 'AP50': col(0.5), 'AP75': col(0.75),
            'per_class': per_class}


def detections_from_detect(out, num_images):
    """(boxes, scores, class_ids, image_ids, ...) of utils.detect -> per-image tuples for mean_average_precision."""
    boxes, scores, cls, img = (np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t) for t in out[:4])
    return [(boxes[img == i], scores[img == i], cls[img == i]) for i in range(num_images)]


def window_result(sums, counts):
    """The running metrics from a window's totals (rn_hip.h: the state of rn_train_metrics_fold): `sums` = [sum_total, sum_class,
    sum_regr, sum_reg, sum_iou], `counts` = [steps, nonfinite_steps, tn, fp, fn, tp, iou_rows].  Totals first, ratios last, as
    tf.metrics does: class_iou by the rule of `class_iou` below from the confusion counts, regr_iou = sum_iou / iou_rows; nan
    where the denominator is zero."""
    sums = [float(v) for v in sums]
    steps, nonfinite, tn, fp, fn, tp, rows = (int(v) for v in counts)
    nan = float('nan')
    ious = []
    for inter, union in ((tn, tn + fp + fn), (tp, tp + fp + fn)):      # class 0 (negative), class 1 (positive)
        if union > 0:
            ious.append(inter / union)
    mean = lambda s: s / steps if steps > 0 else nan
    return {'total_loss': mean(sums[0]), 'class_loss': mean(sums[1]), 'regr_loss': mean(sums[2]),
            'regularization_loss': mean(sums[3]),
            'class_iou': float(np.mean(ious)) if ious else nan,
            'regr_iou': sums[4] / rows if rows > 0 else nan,
            'steps': steps, 'nonfinite_steps': nonfinite}


class TrainMetrics(object):
    """The reference's streaming training metrics (build_metrics, train.py:137-161) kept on the device, inside the step:
    `update` is one launch over the tensors the loss has just read (csrc/train_metrics.hip: the confusion counts of
    sigmoid(logit) > 0.5 against the labels over the trainable anchors and the IoU of the label and predicted boxes decoded at
    the foreground anchors, as one partial row per block), `fold` one block at the end of the step that adds the step -- its
    losses included -- into the window state unless one of them is not finite.  Both are plain launches on the current stream:
    nodes of a captured step, with nothing for the host to read.  `result` is the only call that synchronises."""

    def __init__(self, device):
        import torch
        import _rn
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _rn.RnError("the training metrics are accumulated by the device's kernels: they need a device arena")
        if not hasattr(_rn.lib(), 'rn_train_metrics_pass'):
            raise _rn.RnError("%s has no rn_train_metrics_pass: rebuild it (make -C retinanet-tensorflow_amd/csrc)" % _rn.LIB_PATH)
        # doubles [sum_total, sum_class, sum_regr, sum_reg, sum_iou], int64 [steps, nonfinite_steps, tn, fp, fn, tp, iou_rows]
        self.state = torch.zeros(_rn.TRAIN_METRICS_STATE_BYTES // 8, dtype=torch.int64, device=self.device)
        # the partial rows: owned (they live from the pass to the fold: not the shared scratch arena) and allocated ONCE at the
        # largest size any shape needs -- every captured graph holds this pointer in its pass and fold nodes, and a trainer keeps
        # graphs of several input shapes alive at a time, so the buffer is never replaced
        self.partial = torch.zeros(_rn.TRAIN_METRICS_MAX_WORKSPACE_BYTES // 8, dtype=torch.int64, device=self.device)
        self._updated = False
        self._anchors = {}

    def _anchor_table(self, level, image_size):
        import utils
        key = (id(level), tuple(image_size))
        ent = self._anchors.get(key)
        if ent is None:                            # (the level is kept alive with its key)
            ent = self._anchors[key] = (utils._anchor_tensor(
                level.normalized_anchor_sizes(tuple(image_size), utils.ANCHOR_SIZE_MODE), self.device), level)
        return ent[0]

    def update(self, labels_trainable, logits_trainable, levels, image_size):
        """One launch over every level: `labels_trainable` / `logits_trainable` are the `detection_trainable` tuples
        losses.loss is given (utils.process_labels_and_logits)."""
        import torch
        import _rn
        keys = list(logits_trainable.regression.keys())
        masks = labels_trainable.trainable_masks
        segs = (_rn.MetricsSeg * len(keys))()
        keep = []
        num_classes = None
        for i, k in enumerate(keys):
            z = logits_trainable.classification.unscaled[k].detach().contiguous()
            l = labels_trainable.classification.prob[k].contiguous()
            rp = logits_trainable.regression[k].detach().contiguous()
            rl = labels_trainable.regression[k].contiguous()
            m = masks[k].contiguous()
            assert m.dtype in (torch.uint8, torch.bool) and z.dim() == 5 and z.shape == l.shape and rp.shape == rl.shape
            assert rp.shape == z.shape[:4] + (4,) and m.shape == z.shape[:4]
            n, h, w, a, c = z.shape
            assert num_classes in (None, c)
            num_classes = c
            anchors = self._anchor_table(levels[k], image_size)
            assert anchors.shape == (a, 2)
            segs[i] = _rn.MetricsSeg(_rn.f32(z), _rn.f32(l), _rn.f32(rp), _rn.f32(rl), _rn.ptr(m), _rn.f32(anchors), n, h, w, a)
            keep.append((z, l, rp, rl, m))
        L = _rn.lib()
        need = L.rn_train_metrics_workspace(segs, len(keys), num_classes)
        if need == 0:
            raise _rn.RnError("rn_train_metrics_workspace: %s" % L.rn_last_error().decode())
        assert need <= self.partial.numel() * 8, (need, self.partial.numel() * 8)     # (RN_TRAIN_METRICS_MAX_WORKSPACE_BYTES)
        self._updated = True
        _rn.check(L.rn_train_metrics_pass(segs, len(keys), num_classes, self.partial.data_ptr(), self.partial.numel() * 8,
                                          _rn.stream()), 'rn_train_metrics_pass')

    def fold(self, class_loss, regr_loss, reg_loss):
        """The end of a step: the pass's partial rows and the three device scalars into the window state (one block)."""
        import _rn
        if not self._updated:
            raise _rn.RnError("TrainMetrics.fold before any update")
        _rn.check(_rn.lib().rn_train_metrics_fold(self.partial.data_ptr(), self.partial.numel() * 8, _rn.f32(class_loss),
                                                  _rn.f32(regr_loss), _rn.f32(reg_loss), self.state.data_ptr(), _rn.stream()),
                  'rn_train_metrics_fold')

    def reset(self):
        import _rn
        _rn.check(_rn.lib().rn_train_metrics_reset(self.state.data_ptr(), _rn.stream()), 'rn_train_metrics_reset')

    def raw(self):
        """(sums [5] float64, counts [7] int64) as numpy; synchronises, one copy."""
        host = self.state.cpu().numpy()
        return host[:5].view(np.float64).copy(), host[5:].copy()

    def result(self, reset=True):
        """The window's metrics (window_result); synchronises and copies the state once.  reset=True starts a new window."""
        sums, counts = self.raw()
        if reset:
            self.reset()
        return window_result(sums, counts)


def class_iou(labels, probs, threshold=0.5):
    """tf.metrics.mean_iou(labels, sigmoid(logits) > 0.5, num_classes=2) over the trainable anchors (train.py:149-152):
    mean over the classes {0, 1} present of TP / (TP + FP + FN)."""
    l = np.asarray(labels).reshape(-1) > 0.5
    p = np.asarray(probs).reshape(-1) > threshold
    ious = []
    for v in (False, True):
        inter = np.sum((l == v) & (p == v))
        union = np.sum((l == v) | (p == v))
        if union > 0:
            ious.append(inter / union)
    return float(np.mean(ious)) if ious else float('nan')


def regr_iou(true_boxes, pred_boxes):
    """Mean IoU of matching rows (train.py:138-145,153-154: both decoded at the ground-truth foreground anchors)."""
    a = np.asarray(true_boxes, np.float64).reshape(-1, 4)
    b = np.asarray(pred_boxes, np.float64).reshape(-1, 4)
    if len(a) == 0:
        return float('nan')
    tl = np.maximum(a[:, :2], b[:, :2])
    br = np.minimum(a[:, 2:], b[:, 2:])
    inter = np.prod(np.maximum(br - tl, 0.0), -1)
    union = np.prod(np.maximum(a[:, 2:] - a[:, :2], 0), -1) + np.prod(np.maximum(b[:, 2:] - b[:, :2], 0), -1) - inter
    return float(np.mean(np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)))
