"""Detection losses (drop-in for the live path of reference losses.py:115-175 plus the focal
variant :6-15 that BASELINE's north_star names).

    class_loss, regr_loss = losses.loss(labels=labels['detection_trainable'],
                                        logits=logits['detection_trainable'])

``labels`` / ``logits`` are ``utils.Detection`` tuples of per-level dicts (P3..P7) as produced by
``utils.process_labels_and_logits``; the trainable masks ride along on the module-level
``set_trainable_masks`` / the ``trainable_masks`` argument.  One fused HIP kernel pair
(csrc/loss.hip) computes BCE + dice (or focal) and the Huber box loss over every anchor of
every level, forward and backward.

``mode`` may also be a class-loss SPEC: the reference's ``classification_loss`` (losses.py:113-141) is a list of terms its author
comments in and out; a spec names the terms to sum, each with a weight and, for the overlap terms, a smooth
(``parse_class_loss``; csrc/loss_terms.hip).

``regr_mode`` is the same for the box loss: a regression-loss SPEC sums Huber (the reference's ``regression_loss``,
losses.py:144-152, with a weight and a delta), IoU and GIoU terms over the foreground rows (``parse_regr_loss``;
csrc/regr_terms.hip).
"""
import collections
import math

import ops

LOSS_MODE = 'bce_dice'        # 'bce_dice' = live reference path; 'focal' = losses.py:6-15 + :119-122

TERM_NAMES = ('bce', 'balanced_bce', 'dice', 'jaccard', 'fixed_iou', 'focal')
# the smooths of the reference's call sites (losses.py:130, :133, :136); the other terms have none
DEFAULT_SMOOTH = {'dice': 0.0, 'jaccard': 1.0, 'fixed_iou': 1e-7}

Term = collections.namedtuple('Term', 'name weight smooth')        # smooth: None for a term that has none


class ClassLoss(tuple):
    """The parsed spec: a tuple of Term in the order given."""

    def spec(self):
        """The spec in full (every weight and smooth written out); parse_class_loss(x.spec()) == x."""
        return '+'.join('%s:%r' % (t.name, t.weight) + ('' if t.smooth is None else ':%r' % t.smooth) for t in self)

    def describe(self):
        return ' + '.join('%g * %s' % (t.weight, t.name) + ('' if t.smooth is None else '(smooth %g)' % t.smooth) for t in self)

    def struct(self):
        """The rn_loss_terms descriptor (include/rn_hip.h)."""
        import _rn
        d = _rn.LossTerms()
        for t in self:
            d.terms |= _rn.LOSS_TERM[t.name]
            setattr(d, 'w_' + t.name, t.weight)
            if t.smooth is not None:
                setattr(d, 's_' + t.name, t.smooth)
        return d


def parse_class_loss(spec):
    """SPEC = TERM[+TERM...], TERM = NAME[:WEIGHT[:SMOOTH]]; NAME one of TERM_NAMES, each at most once; WEIGHT > 0 (default 1);
    SMOOTH >= 0 only for dice, jaccard and fixed_iou (defaults 0, 1, 1e-7: the reference's call sites).  Class loss =
    sum WEIGHT * term.  E.g. 'bce+jaccard', 'balanced_bce+dice:0.5', 'bce+dice:1:1+fixed_iou:0.3:1e-7'.  jaccard(s) is
    s * fixed_iou(s) (losses.py:37-47 against :63-73), so jaccard:W:0 is identically 0.  Raises ValueError naming the token."""
    if isinstance(spec, ClassLoss):
        return spec
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError('class loss spec %r: empty' % (spec,))
    terms = []
    for token in spec.split('+'):
        def bad(why):
            return ValueError('class loss spec %r: term %r: %s' % (spec, token, why))
        fields = token.strip().split(':')
        name = fields[0].strip()
        if name not in TERM_NAMES:
            raise bad('unknown name (one of %s)' % ', '.join(TERM_NAMES))
        if any(t.name == name for t in terms):
            raise bad('given twice')
        if len(fields) > (3 if name in DEFAULT_SMOOTH else 2):
            raise bad('NAME:WEIGHT:SMOOTH at the most' if name in DEFAULT_SMOOTH else 'takes no smooth (NAME:WEIGHT)')
        try:
            weight = float(fields[1]) if len(fields) > 1 else 1.0
            smooth = float(fields[2]) if len(fields) > 2 else DEFAULT_SMOOTH.get(name)
        except ValueError:
            raise bad('weight and smooth are numbers')
        if not (math.isfinite(weight) and weight > 0.0):
            raise bad('the weight must be finite and > 0')
        if smooth is not None and not (math.isfinite(smooth) and smooth >= 0.0):
            raise bad('the smooth must be finite and >= 0')
        if name == 'jaccard' and weight * smooth > 3.4e38:
            raise bad('weight * smooth (the scale of the term) overflows float32')
        terms.append(Term(name, weight, smooth))
    return ClassLoss(terms)


REGR_TERM_NAMES = ('huber', 'iou', 'giou')

RegrTerm = collections.namedtuple('RegrTerm', 'name weight delta')        # delta: None for a term that has none


class RegrLoss(tuple):
    """The parsed regression-loss spec: a tuple of RegrTerm in the order given."""

    def spec(self):
        """The spec in full (every weight and delta written out); parse_regr_loss(x.spec()) == x."""
        return '+'.join('%s:%r' % (t.name, t.weight) + ('' if t.delta is None else ':%r' % t.delta) for t in self)

    def describe(self):
        return ' + '.join('%g * %s' % (t.weight, t.name) + ('' if t.delta is None else '(delta %g)' % t.delta) for t in self)

    def is_default(self):
        """huber with weight 1 and delta 1 alone: the regression loss of csrc/loss.hip, which then stays the one that runs."""
        return tuple(self) == (('huber', 1.0, 1.0),)

    def struct(self):
        """The rn_regr_terms descriptor (include/rn_hip.h)."""
        import _rn
        d = _rn.RegrTerms()
        for t in self:
            d.terms |= _rn.REGR_TERM[t.name]
            setattr(d, 'w_' + t.name, t.weight)
            if t.delta is not None:
                d.delta_huber = t.delta
        return d


def parse_regr_loss(spec):
    """SPEC = TERM[+TERM...], TERM = NAME[:WEIGHT] or huber[:WEIGHT[:DELTA]]; NAME one of REGR_TERM_NAMES, each at most once;
    WEIGHT > 0 (default 1); DELTA > 0 (default 1: the reference's tf.losses.huber_loss).  Regression loss = sum WEIGHT * term over
    the foreground rows: huber = sum huber_DELTA(l - p) / (4 #fg) (losses.py:144-152), iou = sum (1 - IoU) / #fg,
    giou = sum (1 - GIoU) / #fg, the boxes in anchor units.  E.g. 'giou:2', 'huber:0.5+giou:2', 'huber:1:0.11'.
    Raises ValueError naming the token."""
    if isinstance(spec, RegrLoss):
        return spec
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError('regr loss spec %r: empty' % (spec,))
    terms = []
    for token in spec.split('+'):
        def bad(why):
            return ValueError('regr loss spec %r: term %r: %s' % (spec, token, why))
        fields = token.strip().split(':')
        name = fields[0].strip()
        if name not in REGR_TERM_NAMES:
            raise bad('unknown name (one of %s)' % ', '.join(REGR_TERM_NAMES))
        if any(t.name == name for t in terms):
            raise bad('given twice')
        if len(fields) > (3 if name == 'huber' else 2):
            raise bad('NAME:WEIGHT:DELTA at the most' if name == 'huber' else 'takes no delta (NAME:WEIGHT)')
        try:
            weight = float(fields[1]) if len(fields) > 1 else 1.0
            delta = float(fields[2]) if len(fields) > 2 else (1.0 if name == 'huber' else None)
        except ValueError:
            raise bad('weight and delta are numbers')
        if not (math.isfinite(weight) and 0.0 < weight <= 3.4e38):
            raise bad('the weight must be finite and > 0')
        if delta is not None and not (math.isfinite(delta) and 0.0 < delta <= 3.4e38):
            raise bad('the delta must be finite and > 0')
        terms.append(RegrTerm(name, weight, delta))
    return RegrLoss(terms)


def loss(labels, logits, trainable_masks=None, mode=None, name='loss', return_stats=False, regr_mode=None):
    """(class_loss, regr_loss) as 0-dim tensors (losses.py:155-175).  mode: 'bce_dice', 'focal', or a class-loss spec / ClassLoss.
    regr_mode: None, or a regression-loss spec / RegrLoss; None and a spec equal to 'huber:1:1' are the Huber loss of the
    class-loss kernels, exactly as without the argument; any other spec takes the class loss from those kernels and the regression
    loss from ops.regression_terms (their Huber value is then not used)."""
    mode = mode or LOSS_MODE
    if regr_mode is not None:
        regr_mode = parse_regr_loss(regr_mode)
        if regr_mode.is_default():
            regr_mode = None
    keys = list(logits.regression.keys())
    if trainable_masks is None:
        trainable_masks = getattr(labels, 'trainable_masks', None)
    if trainable_masks is None:
        raise AssertionError('losses.loss needs trainable_masks (dict P3..P7 of [N,H,W,A] uint8/bool)')
    cls_logits = [logits.classification.unscaled[k] for k in keys]
    num_classes = cls_logits[0].shape[-1]
    # with a regression spec the class-loss kernels see the box predictions as constants: their Huber value is not used, and
    # d_reg_pred has ONE producer in the step's graph (ops.regression_terms), as it has without a spec
    class_loss, regr_loss, stats = ops.detection_loss(
        cls_logits, [logits.regression[k] if regr_mode is None else logits.regression[k].detach() for k in keys],
        [labels.classification.prob[k] for k in keys], [labels.regression[k] for k in keys],
        [trainable_masks[k] for k in keys], num_classes, mode)
    if regr_mode is not None:
        regr_loss, _ = ops.regression_terms(
            [logits.regression[k] for k in keys], [labels.regression[k] for k in keys],
            [labels.classification.prob[k] for k in keys], [trainable_masks[k] for k in keys], num_classes, regr_mode)
    if return_stats:
        return class_loss, regr_loss, stats
    return class_loss, regr_loss
