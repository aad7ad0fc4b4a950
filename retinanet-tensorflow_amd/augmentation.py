"""Horizontal-flip augmentation on the device (drop-in for reference augmentation.py:5-22).

    flipped = augmentation.flip(input)
`input` is the reference's sample dict: 'image' [H,W,3] (or a batch [N,H,W,3]), 'detection':
{'classifications': {Pk: [H,W,A,C]}, 'regressions': {Pk: [H,W,A,4]}}, 'trainable_masks': {Pk: [H,W,A]}.
Every map is reversed along its W axis and the x component (index 1) of the regression targets changes
sign.  `make_pair` builds the reference's batch of two = [sample, flip(sample)] (dataset.py:182-204).

`Policy` draws the parameters of the training-time augmentation the reference names in augment_sample (dataset.py:206-212:
random_contrast(0.8, 1.2), random_brightness(0.2), random_saturation(0.8, 1.0), left as a TODO there) plus a random crop; the
transform itself runs on the device inside the step (rn_resize_pair_u8_augment, dataset.resize_pair_u8_augment).
"""
import collections

import numpy as np
import torch

import _rn
import utils


def _flip(t, w_axis, neg_mod=0, neg_idx=0, out=None):
    t = t.contiguous()
    outer = 1
    for d in t.shape[:w_axis]:
        outer *= d
    inner = 1
    for d in t.shape[w_axis + 1:]:
        inner *= d
    esz = t.element_size()
    assert esz in (1, 4), "flip: fp32 maps or 1-byte masks"
    y = torch.empty_like(t) if out is None else out
    assert y.is_contiguous() and y.shape == t.shape and y.dtype == t.dtype
    _rn.check(_rn.lib().rn_flip_width(_rn.ptr(t), _rn.ptr(y), outer, t.shape[w_axis], inner, esz, neg_mod, neg_idx,
                                      _rn.stream()), "rn_flip_width")
    return y


def flip(input):
    batched = input['image'].dim() == 4
    ax = 2 if batched else 1
    image = _flip(input['image'], ax)
    classifications = utils.dict_map(lambda x: _flip(x, ax), input['detection']['classifications'])
    regressions = utils.dict_map(lambda x: _flip(x, ax, 4, 1), input['detection']['regressions'])
    trainable_masks = utils.dict_map(lambda x: _flip(x, ax), input['trainable_masks'])
    return {
        'image': image,
        'detection': {'classifications': classifications, 'regressions': regressions},
        'trainable_masks': trainable_masks,
    }


def make_pair(input):
    """[sample, hflip(sample)] stacked on a new leading axis (dataset.py:182-204)."""
    f = flip(input)
    stack = lambda a, b: torch.stack([a, b], 0)
    return {
        **input,
        'image': stack(input['image'], f['image']),
        'detection': {
            'classifications': utils.dict_starmap(stack, [input['detection']['classifications'], f['detection']['classifications']]),
            'regressions': utils.dict_starmap(stack, [input['detection']['regressions'], f['detection']['regressions']]),
        },
        'trainable_masks': utils.dict_starmap(stack, [input['trainable_masks'], f['trainable_masks']]),
    }


# what one sample's transform needs besides the image: the crop window in raw pixels and the three photometric scalars (fp32,
# the values the device descriptor carries)
Draw = collections.namedtuple('Draw', ['y0', 'x0', 'ch', 'cw', 'f', 'd', 'k'])


def crop_boxes(boxes, class_ids, image_hw, window):
    """Boxes [O, 4] (corners normalised to the image) under the crop window (y0, x0, ch, cw) in raw pixels: a box is kept when
    its centre lies inside the window (borders included), clipped to the window and renormalised to it; survivors keep their
    order.  Returns (boxes' [O', 4] float32, class_ids' [O'])."""
    h, w = float(image_hw[0]), float(image_hw[1])
    y0, x0, ch, cw = window
    wy0, wx0, wy1, wx1 = y0 / h, x0 / w, (y0 + ch) / h, (x0 + cw) / w
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    ids = np.asarray(class_ids).reshape(-1)
    cy, cx = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    keep = (cy >= wy0) & (cy <= wy1) & (cx >= wx0) & (cx <= wx1)
    lo = np.array([wy0, wx0, wy0, wx0])
    hi = np.array([wy1, wx1, wy1, wx1])
    out = (np.minimum(np.maximum(b[keep], lo), hi) - lo) / (hi - lo)
    return out.astype(np.float32), ids[keep]


class Policy(object):
    """Training-time augmentation parameters, drawn per sample.

        values, boxes2, class_ids2 = policy.draw(rank, ordinal, image_hw, boxes, class_ids)

    contrast (lo, hi): factor f ~ U[lo, hi];  brightness B: delta d ~ U[-B, B];  saturation (lo, hi): factor k ~ U[lo, hi]  (the
    ranges of dataset.py:206-212).  crop_min < 1 also draws a crop: side fraction s ~ U[crop_min, 1], window (max(2, round(h s)),
    max(2, round(w s))) -- the raw aspect, so the network input size stays rescale_size of the FULL image and a crop adds no
    graph shapes -- with its origin uniform over the positions that keep it inside the image.  Boxes follow crop_boxes; when
    none survives the sample keeps the full window, and its photometric draws are the ones it would have had anyway (they are
    drawn first).  The stream is np.random.default_rng([seed, rank, ordinal]): a pure function of the sample's position in the
    rank's stream, so a resumed run (the checkpoint stores samples_drawn) continues it exactly."""

    def __init__(self, contrast=(0.8, 1.2), brightness=0.2, saturation=(0.8, 1.0), crop_min=1.0, seed=0):
        self.contrast = (float(contrast[0]), float(contrast[1]))
        self.brightness = float(brightness)
        self.saturation = (float(saturation[0]), float(saturation[1]))
        self.crop_min = float(crop_min)
        self.seed = int(seed)
        if not (0.0 < self.contrast[0] <= self.contrast[1]):
            raise ValueError("Policy: contrast factors must be positive and ordered, got %r" % (self.contrast,))
        if not (0.0 <= self.saturation[0] <= self.saturation[1]):
            raise ValueError("Policy: saturation factors must be non-negative and ordered, got %r" % (self.saturation,))
        if self.brightness < 0.0:
            raise ValueError("Policy: the brightness range must be non-negative, got %r" % self.brightness)
        if not (0.0 < self.crop_min <= 1.0):
            raise ValueError("Policy: crop_min must lie in (0, 1], got %r" % self.crop_min)

    def draw(self, rank, ordinal, image_hw, boxes, class_ids):
        h, w = int(image_hw[0]), int(image_hw[1])
        rng = np.random.default_rng([self.seed, int(rank), int(ordinal)])
        f = np.float32(rng.uniform(*self.contrast))
        d = np.float32(rng.uniform(-self.brightness, self.brightness))
        k = np.float32(rng.uniform(*self.saturation))
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        class_ids = np.asarray(class_ids).reshape(-1)
        window = (0, 0, h, w)
        if self.crop_min < 1.0:
            s = rng.uniform(self.crop_min, 1.0)
            ch, cw = min(h, max(2, int(round(h * s)))), min(w, max(2, int(round(w * s))))
            y0, x0 = int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1))
            b2, ids2 = crop_boxes(boxes, class_ids, (h, w), (y0, x0, ch, cw))
            if len(ids2) > 0:                  # (no survivor: the full image, its boxes untouched)
                window, boxes, class_ids = (y0, x0, ch, cw), b2, ids2
        return Draw(window[0], window[1], window[2], window[3], f, d, k), boxes, class_ids
