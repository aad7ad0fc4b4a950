"""Anchor assignment on the device (drop-in for reference dataset.py:43-142 ``level_labels`` /
``build_labels``), batched over images.

    cls, reg, masks = build_labels(image_size, class_ids, boxes, num_obj, levels, num_classes)
    # dicts P3..P7: [N,H,W,A,C] f32 one-hot (zero where IoU<0.5), [N,H,W,A,4] f32, [N,H,W,A] u8

The tf.data input pipeline of the reference (dataset.py:145-233) maps onto: the annotation readers
(data_loaders/pascal.py, coco.py; epoch order in data_loaders/files.py), `decode_image` on the host (Pillow, an ordered
pool of decode threads), and the device side below -- rescale, normalisation, the ``[image, hflip(image)]`` batch
convention (dataset.py:182-204) and the label construction.
"""
import ctypes as C
import math

import numpy as np
import torch

import _rn
import utils

NEG_IOU_THRESHOLD = 0.4
POS_IOU_THRESHOLD = 0.5
MEAN = [0.46618041, 0.44669811, 0.40252436]
STD = [0.27940595, 0.27489075, 0.28920765]
ANCHOR_SIZE_MODE = 'trunc_int'


def level_labels(image_size, class_id, true_box, level, factor, num_classes, num_obj=None, return_argmax=False):
    """class_id [N, O] int32, true_box [N, O, 4] normalised corners, num_obj [N] (valid objects per
    image, default O) -> (classification [N,H,W,A,C], regression [N,H,W,A,4], trainable [N,H,W,A])."""
    dev = true_box.device
    n, o = true_box.shape[0], true_box.shape[1]
    true_box = true_box.contiguous().float()
    class_id = class_id.to(torch.int32).contiguous()
    if num_obj is None:
        num_obj = torch.full((n,), o, dtype=torch.int32, device=dev)
    num_obj = num_obj.to(torch.int32).contiguous()
    anchors = utils._anchor_tensor(level.normalized_anchor_sizes(image_size, ANCHOR_SIZE_MODE), dev)
    a = anchors.shape[0]
    gh, gw = int(math.ceil(image_size[0] / factor)), int(math.ceil(image_size[1] / factor))
    cls = torch.empty((n, gh, gw, a, num_classes), dtype=torch.float32, device=dev)
    reg = torch.empty((n, gh, gw, a, 4), dtype=torch.float32, device=dev)
    msk = torch.empty((n, gh, gw, a), dtype=torch.uint8, device=dev)
    arg = torch.empty((n, gh, gw, a), dtype=torch.int32, device=dev) if return_argmax else None
    _rn.check(_rn.lib().rn_anchor_assign(_rn.f32(true_box), _rn.ptr(class_id), _rn.ptr(num_obj), n, o,
                                         _rn.f32(anchors), a, gh, gw, num_classes, _rn.f32(cls), _rn.f32(reg),
                                         _rn.ptr(msk), _rn.ptr(arg), _rn.stream()), 'rn_anchor_assign')
    if return_argmax:
        return cls, reg, msk, arg
    return cls, reg, msk


def build_labels(image_size, class_ids, boxes, levels, num_classes, num_obj=None, flip_pair=False):
    """dataset.py:126-142 for a batch: every level's maps from one launch (rn_anchor_assign_levels); the per-level
    results are the ones `level_labels` gives.
    flip_pair=True: the reference's batch of two per sample (dataset.py:182-204) from the same launch -- image i is assigned
    once and fills batch slots 2i (as is) and 2i+1 (= augmentation.flip of its maps: W reversed, x shift negated), so the
    mirror image's labels are bit for bit the flipped maps, and the assignment runs once per sample."""
    dev = boxes.device
    n_src, o = boxes.shape[0], boxes.shape[1]
    n = 2 * n_src if flip_pair else n_src
    boxes = boxes.contiguous().float()
    class_ids = class_ids.to(torch.int32).contiguous()
    if num_obj is None:
        num_obj = torch.full((n_src,), o, dtype=torch.int32, device=dev)
    num_obj = num_obj.to(torch.int32).contiguous()
    names = list(levels)
    lv = (_rn.AssignLevel * len(names))()
    classifications, regressions, trainable_masks, keep = {}, {}, {}, []
    a = None
    for i, pn in enumerate(names):
        factor = 2 ** int(pn[-1])
        anchors = utils._anchor_tensor(levels[pn].normalized_anchor_sizes(image_size, ANCHOR_SIZE_MODE), dev)
        assert a in (None, anchors.shape[0]), "every level carries the same number of anchors (levels.py:32-44)"
        a = anchors.shape[0]
        gh, gw = int(math.ceil(image_size[0] / factor)), int(math.ceil(image_size[1] / factor))
        classifications[pn] = torch.empty((n, gh, gw, a, num_classes), dtype=torch.float32, device=dev)
        regressions[pn] = torch.empty((n, gh, gw, a, 4), dtype=torch.float32, device=dev)
        trainable_masks[pn] = torch.empty((n, gh, gw, a), dtype=torch.uint8, device=dev)
        keep.append(anchors)
        lv[i] = _rn.AssignLevel(anchors.data_ptr(), gh, gw, classifications[pn].data_ptr(), regressions[pn].data_ptr(),
                                trainable_masks[pn].data_ptr(), None)
    fn = _rn.lib().rn_anchor_assign_levels_pair if flip_pair else _rn.lib().rn_anchor_assign_levels
    _rn.check(fn(_rn.f32(boxes), _rn.ptr(class_ids), _rn.ptr(num_obj), n_src, o, lv, len(names), a, num_classes, _rn.stream()),
              'rn_anchor_assign_levels')
    return classifications, regressions, trainable_masks


def flip_boxes(boxes):
    """h-flip of normalised corner boxes [.., 4] = [y1, x1, y2, x2] (labels of the flipped image
    of the reference's [image, hflip] batch, dataset.py:182-204, are built from these)."""
    return torch.stack([boxes[..., 0], 1.0 - boxes[..., 3], boxes[..., 2], 1.0 - boxes[..., 1]], -1)


def rescale_size(size, scale):
    """New (h, w) of dataset.py:145-151: shorter side -> `scale`, tf.round (half to even) of size * ratio, the
    arithmetic in float32 as tf.to_float / tf.round do it."""
    size = np.asarray(size, np.float32)
    ratio = np.float32(scale) / size[int(np.argmin(size))]
    new = np.rint(size * ratio).astype(np.int32)                 # np.rint == tf.round: half to even
    return int(new[0]), int(new[1])


def rescale_image(image, scale=None, size=None, normalize=False, out=None):
    """tf.image.resize_images(image, new_size, BILINEAR, align_corners=True) (dataset.py:145-151) on the device.
    image: [H,W,C] or [N,H,W,C], uint8 (converted like tf.image.convert_image_dtype: * 1/255) or fp32.
    normalize=True also applies train.py:48-49 preprocess_image ((v - MEAN) / STD) in the same pass."""
    batched = image.dim() == 4
    x = (image if batched else image[None]).contiguous()
    n, h, w, c = x.shape
    oh, ow = size if size is not None else rescale_size((h, w), scale)
    if out is None:
        y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    else:                                          # e.g. slot 0 of the [sample, hflip] batch buffer
        y = out if batched else out[None]
        assert y.is_contiguous() and tuple(y.shape) == (n, oh, ow, c) and y.dtype == torch.float32
    assert x.dtype in (torch.uint8, torch.float32)
    mean = std = None
    if normalize:
        assert c == 3
        mean = (C.c_float * 3)(*MEAN)
        std = (C.c_float * 3)(*STD)
    _rn.check(_rn.lib().rn_resize_bilinear_normalize(_rn.ptr(x), 1 if x.dtype == torch.uint8 else 0, _rn.f32(y), n, h, w, c,
                                                     oh, ow, mean, std, _rn.stream()), 'rn_resize_bilinear_normalize')
    return y if batched else y[0]


def resize_desc(hw, size):
    """rn_resize_desc {h, w, hs, ws} of a raw (h, w) image resized to size = (oh, ow), as int32 [4] (the ratios' fp32 bits):
    hs = (h-1)/(oh-1), 0 when oh == 1, in fp32 -- the values rn_resize_bilinear_normalize computes, bit for bit."""
    h, w = int(hw[0]), int(hw[1])
    oh, ow = int(size[0]), int(size[1])
    ratios = np.array([np.float32(h - 1) / np.float32(oh - 1) if oh > 1 else 0.0,
                       np.float32(w - 1) / np.float32(ow - 1) if ow > 1 else 0.0], np.float32)
    return np.concatenate([np.array([h, w], np.int32), ratios.view(np.int32)])


def resize_pair_u8(raw, desc, size, normalize=True, out=None):
    """rn_resize_pair_u8: raw uint8 device buffer (any length; the image is its first h*w*3 bytes), desc int32 [4] device
    tensor (resize_desc) -> [2, oh, ow, 3] fp32 = [rescale_image(image, normalize), its h-flip] in one launch."""
    oh, ow = int(size[0]), int(size[1])
    pair = torch.empty((2, oh, ow, 3), dtype=torch.float32, device=raw.device) if out is None else out
    assert pair.is_contiguous() and tuple(pair.shape) == (2, oh, ow, 3) and pair.dtype == torch.float32
    assert raw.dtype == torch.uint8 and desc.dtype == torch.int32 and desc.numel() == 4
    mean = (C.c_float * 3)(*MEAN) if normalize else None
    std = (C.c_float * 3)(*STD) if normalize else None
    _rn.check(_rn.lib().rn_resize_pair_u8(_rn.ptr(raw), int(raw.numel()), _rn.ptr(desc), _rn.f32(pair), oh, ow, mean, std,
                                          _rn.stream()), 'rn_resize_pair_u8')
    return pair


def augment_desc(hw, values, size):
    """rn_augment_desc of a raw (h, w) image, augmentation.Draw `values` (crop window y0, x0, ch, cw in raw pixels; contrast f,
    brightness d, saturation k) and the output size = (oh, ow), as int32 [12] (the floats' fp32 bits): h, w, y0, x0, ch, cw,
    hs, ws, f, d, k, 0 -- hs / ws are resize_desc's ratios of the WINDOW, bit for bit."""
    ratios = resize_desc((values.ch, values.cw), size)[2:]
    fdk = np.array([values.f, values.d, values.k], np.float32).view(np.int32)
    return np.concatenate([np.array([int(hw[0]), int(hw[1]), values.y0, values.x0, values.ch, values.cw], np.int32), ratios, fdk,
                           np.zeros(1, np.int32)])


def resize_pair_u8_augment(raw, desc, size, normalize=True, out=None):
    """rn_resize_pair_u8_augment: resize_pair_u8 of the crop window with contrast, brightness and saturation applied (the
    contract is stated in csrc/preprocess.hip), every parameter read from `desc` (int32 [12] device tensor, augment_desc) at
    run time -> [2, oh, ow, 3] fp32.  Two launches; the partial channel sums live in the stream's workspace."""
    oh, ow = int(size[0]), int(size[1])
    pair = torch.empty((2, oh, ow, 3), dtype=torch.float32, device=raw.device) if out is None else out
    assert pair.is_contiguous() and tuple(pair.shape) == (2, oh, ow, 3) and pair.dtype == torch.float32
    assert raw.dtype == torch.uint8 and desc.dtype == torch.int32 and desc.numel() == 12
    mean = (C.c_float * 3)(*MEAN) if normalize else None
    std = (C.c_float * 3)(*STD) if normalize else None
    L_ = _rn.lib()
    ws = _rn.workspace(L_.rn_resize_pair_u8_augment_workspace(oh, ow), raw.device)
    _rn.check(L_.rn_resize_pair_u8_augment(_rn.ptr(raw), int(raw.numel()), _rn.ptr(desc), _rn.f32(pair), oh, ow, mean, std,
                                           ws.data_ptr(), ws.numel(), _rn.stream()), 'rn_resize_pair_u8_augment')
    return pair


def _batch_args(raw, descs, width, size, stride, out):
    """Checked (k, pairs) of the batched preprocess calls: descs [k, width] int32, raw at least k * stride bytes."""
    oh, ow = int(size[0]), int(size[1])
    stride = int(stride)
    assert raw.dtype == torch.uint8 and raw.is_contiguous() and descs.dtype == torch.int32 and descs.is_contiguous()
    assert descs.dim() == 2 and descs.shape[1] == width and descs.shape[0] >= 1
    k = int(descs.shape[0])
    assert stride >= 3 and int(raw.numel()) >= k * stride, "raw holds %d bytes, %d samples of stride %d need %d" % (
        raw.numel(), k, stride, k * stride)
    pairs = torch.empty((2 * k, oh, ow, 3), dtype=torch.float32, device=raw.device) if out is None else out
    assert pairs.is_contiguous() and tuple(pairs.shape) == (2 * k, oh, ow, 3) and pairs.dtype == torch.float32
    return k, pairs


def resize_pair_u8_batch(raw, descs, size, stride, normalize=True, out=None):
    """rn_resize_pair_u8_batch: k raw uint8 images in one device buffer, image i in raw[i * stride, (i+1) * stride) with its
    resize_desc in descs[i] (int32 [k, 4] device tensor) -> [2k, oh, ow, 3] fp32, slots 2i / 2i+1 = resize_pair_u8 of image i,
    bit for bit, in one launch."""
    k, pairs = _batch_args(raw, descs, 4, size, stride, out)
    mean = (C.c_float * 3)(*MEAN) if normalize else None
    std = (C.c_float * 3)(*STD) if normalize else None
    _rn.check(_rn.lib().rn_resize_pair_u8_batch(_rn.ptr(raw), int(stride), _rn.ptr(descs), k, _rn.f32(pairs), int(size[0]),
                                                int(size[1]), mean, std, _rn.stream()), 'rn_resize_pair_u8_batch')
    return pairs


def resize_pair_u8_augment_batch(raw, descs, size, stride, normalize=True, out=None):
    """rn_resize_pair_u8_augment_batch: resize_pair_u8_batch with the augment_desc of image i in descs[i] (int32 [k, 12] device
    tensor); slots 2i / 2i+1 = resize_pair_u8_augment of image i, bit for bit.  Two launches whatever k is; every sample's
    partial channel sums live in the stream's workspace."""
    k, pairs = _batch_args(raw, descs, 12, size, stride, out)
    oh, ow = int(size[0]), int(size[1])
    mean = (C.c_float * 3)(*MEAN) if normalize else None
    std = (C.c_float * 3)(*STD) if normalize else None
    L_ = _rn.lib()
    ws = _rn.workspace(L_.rn_resize_pair_u8_augment_batch_workspace(k, oh, ow), raw.device)
    _rn.check(L_.rn_resize_pair_u8_augment_batch(_rn.ptr(raw), int(stride), _rn.ptr(descs), k, _rn.f32(pairs), oh, ow, mean, std,
                                                 ws.data_ptr(), ws.numel(), _rn.stream()), 'rn_resize_pair_u8_augment_batch')
    return pairs


def preprocess_image(image):
    """(image - MEAN) / STD (train.py:48-49) for a float image already at its final size."""
    return rescale_image(image, size=tuple(image.shape[-3:-1]), normalize=True)


def sample_batch(image, boxes, class_ids, levels, num_classes, scale=None, num_obj=None, normalize=True):
    """One sample -> the reference's batch of two (dataset.py:154-215 after the decode): rescale_image (dataset.py:145-151) +
    preprocess_image (train.py:48-49) in ONE kernel into slot 0, its h-flip (augmentation.py:5-22) into slot 1, and the
    labels of both from ONE assignment launch (build_labels(flip_pair=True)).  Four launches, every shape static: the
    function is capturable into the train step's hipGraph (DeviceFeed.features), and it IS what build_dataset runs eagerly.
      image [H,W,3] uint8 / fp32 (device), boxes [1,O,4] normalised corners, class_ids [1,O] int32, num_obj [1] or None."""
    import augmentation
    h, w = int(image.shape[0]), int(image.shape[1])
    size = rescale_size((h, w), scale) if scale is not None else (h, w)
    pair = torch.empty((2, size[0], size[1], int(image.shape[2])), dtype=torch.float32, device=image.device)
    rescale_image(image, size=size, normalize=normalize, out=pair[0])
    augmentation._flip(pair[0], 1, out=pair[1])          # (per-element normalisation commutes with the flip: same bits)
    c, r, m = build_labels(size, class_ids, boxes, levels, num_classes, num_obj=num_obj, flip_pair=True)
    return {'image': pair, 'image_size': size, 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m}


def decode_image(path):
    """tf.image.decode_jpeg(contents, channels=3) (dataset.py:158-160) on the host: uint8 [H, W, 3].  Pillow without draft()
    (full-size decode), grey / CMYK / palette images through convert('RGB'), EXIF orientation ignored as TF ignores it, PNG
    accepted as decode_jpeg accepts it."""
    try:
        from PIL import Image
    except ImportError as e:
        raise _rn.RnError("decoding image files needs Pillow (import PIL failed: %s)" % e)
    if isinstance(path, bytes):
        path = path.decode('utf-8')
    with Image.open(path) as im:
        if im.mode != 'RGB':
            im = im.convert('RGB')
        return np.asarray(im, dtype=np.uint8).copy()


def decoded(samples, workers=4):
    """The samples of `samples`, in order, each 'image_file' one decoded into 'image' by a pool of `workers` threads (at most
    16; Pillow releases the GIL while it decodes).  Samples that already carry 'image' pass through untouched, and no pool
    is started until the first 'image_file' sample.  When the decoded size differs from the annotated 'image_size', the
    decoded size wins (the boxes are normalised by the image's own size downstream)."""
    import collections
    workers = max(1, min(16, int(workers)))

    def load(s):
        s = dict(s)
        s['image'] = decode_image(s['image_file'])
        s['image_size'] = tuple(s['image'].shape[:2])
        return s

    pool, pending = None, collections.deque()
    try:
        for s in samples:
            if 'image' in s and not pending:
                yield s
                continue
            if pool is None:
                from concurrent.futures import ThreadPoolExecutor
                pool = ThreadPoolExecutor(workers, thread_name_prefix='rn-decode')
            pending.append(pool.submit(load, s) if 'image' not in s else _done(s))
            if len(pending) >= 2 * workers:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()
    finally:
        if pool is not None:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)


def _done(value):
    from concurrent.futures import Future
    f = Future()
    f.set_result(value)
    return f


def build_dataset(data_loader, levels, scale=None, shuffle=None, augment=False, device='cuda', normalize=True, decode_workers=4,
                  first_ordinal=0):
    """Generator form of dataset.py:154-215: per sample  decode -> boxes / image_size -> rescale_image ->
    build_labels -> [sample, hflip(sample)] batch -> preprocess_image.  Everything after the host loader runs on the
    device (sample_batch).  `shuffle` is accepted for signature parity (shuffling belongs to the loader here).
    augment: False / None, or an augmentation.Policy (the reference's augment_sample, dataset.py:206-212): sample i of the
    stream is drawn at ordinal first_ordinal + i with the loader's rank and goes through resize_pair_u8_augment, its labels
    built from the transformed boxes -- what DeviceFeed(ragged=True, augment=policy) stages, eagerly.  uint8 images only.
    augment=True, the literal the reference's train_input_fn passes (train.py:190-198), stays what it has always been here and
    is in the reference, whose augment_sample is a stub: accepted, no transform.  Anything else raises a TypeError."""
    augment = _policy_or_none(augment, allow_true=True)
    dev = torch.device(device)
    for i, sample in enumerate(decoded(data_loader, decode_workers)):
        if augment:
            yield _augmented_batch(sample, augment, int(getattr(data_loader, 'rank', 0)), int(first_ordinal) + i, levels,
                                   data_loader.num_classes, scale, normalize, dev)
            continue
        image = torch.from_numpy(np.ascontiguousarray(sample['image'])).to(dev)                # uint8 or float [H,W,3]
        h, w = int(image.shape[0]), int(image.shape[1])
        boxes = np.asarray(sample['boxes'], np.float32) / np.asarray([h, w, h, w], np.float32)   # dataset.py:163
        ids = torch.from_numpy(np.asarray(sample['class_ids'], np.int32)).to(dev)[None]
        batch = sample_batch(image, torch.from_numpy(boxes).to(dev)[None], ids, levels, data_loader.num_classes, scale=scale,
                             normalize=normalize)
        batch.update(boxes=boxes, class_ids=sample['class_ids'])
        yield batch


def _policy_or_none(augment, allow_true=False):
    """None for None / False (and for True where the caller keeps the reference's literal as a no-op), the policy itself for an
    augmentation.Policy (anything with its `draw`), a TypeError otherwise."""
    if augment is None or augment is False or (allow_true and augment is True):
        return None
    if isinstance(augment, bool) or not callable(getattr(augment, 'draw', None)):
        raise TypeError("augment must be None, False or an augmentation.Policy, got %r" % (augment,))
    return augment


def _augmented_batch(sample, policy, rank, ordinal, levels, num_classes, scale, normalize, dev):
    img = np.ascontiguousarray(sample['image'])
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("build_dataset(augment=policy) transforms uint8 [H, W, 3] images (the augmentation kernel reads raw "
                         "bytes), got %s %s" % (img.dtype, img.shape))
    h, w = int(img.shape[0]), int(img.shape[1])
    boxes = np.asarray(sample['boxes'], np.float32).reshape(-1, 4) / np.asarray([h, w, h, w], np.float32)   # dataset.py:163
    values, boxes, ids = policy.draw(rank, ordinal, (h, w), boxes, np.asarray(sample['class_ids'], np.int32).reshape(-1))
    size = rescale_size((h, w), scale) if scale is not None else (h, w)
    desc = augment_desc((h, w), values, size)
    pair = resize_pair_u8_augment(torch.from_numpy(img.reshape(-1)).to(dev), torch.from_numpy(desc).to(dev), size,
                                  normalize=normalize)
    c, r, m = build_labels(size, torch.from_numpy(np.asarray(ids, np.int32)).to(dev)[None], torch.from_numpy(boxes).to(dev)[None],
                           levels, num_classes, flip_pair=True)
    return {'image': pair, 'image_size': size, 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m,
            'boxes': boxes, 'class_ids': ids, 'augment_desc': desc}


class DeviceFeed(object):
    """train_input_fn (train.py:190-202) for the hipGraph train step: a NEW sample every step without leaving the graph.

      loader thread -> pinned host slots -> async H2D on a copy stream -> STATIC device buffers (raw image, boxes, class
      ids, object count) -> `features()` = sample_batch on those buffers, captured INSIDE segment A of the step's graph.

    Protocol with train.Trainer (input_fn=feed): `stage()` before segment A is launched (the copy stream uploads the next
    sample once the previous segment A has consumed the buffers; the main stream waits for the upload), `features()` inside
    the segment, `consumed()` right after it.  The sample stream is the loader's, in order: a run through DeviceFeed sees
    exactly the samples `build_dataset` would yield.  A sample whose image size or object capacity differs from the
    buffers' gets new buffers, and `shape_key` changes -- the trainer keeps one captured graph per key.

    ragged=True (real images: many raw sizes, uint8 only): ONE pinned host slot set and ONE static device set hold the raw image
    (a flat byte buffer), its rn_resize_desc, the boxes and the ids, sized once from the loader's `max_image_pixels()` /
    `max_objects()` hints (objects rounded up to 32); without hints the capacity grows x1.5 when a sample needs more, and each
    growth is a new generation.  `features()` is rn_resize_pair_u8 (raw size read from the descriptor at run time) + the
    paired assignment, so the shape key is (oh, ow, object capacity, generation): one captured graph per NETWORK INPUT shape,
    whatever raw sizes map to it.  'image_file' samples are decoded by `decode_workers` threads (`decoded`).

    augment=policy (an augmentation.Policy; ragged mode only): the loader thread draws sample i's parameters at ordinal
    first_ordinal + i (rank: the loader's), writes the rn_augment_desc and the TRANSFORMED boxes / ids into the pinned slot, and
    `features()` is rn_resize_pair_u8_augment + the paired assignment.  Every parameter reaches the kernels through the uploaded
    descriptor, so the shape key -- and with it the set of captured graphs -- is the same as without a policy.  `last_sample`
    carries the transformed boxes and the descriptor ('augment_desc').  augment=None / False: the path above, untouched.

    samples_per_step=K (1 <= K <= 16; ragged mode only; 1 = everything above, untouched): a step trains on a GROUP -- the next
    sample of the stream plus the samples that follow it while they have the same network input size, K at most (the loader
    thread looks one sample ahead; the sample it peeked at and did not take opens the next group, and is not staged before
    that).  Nothing is dropped, reordered or duplicated: the groups, concatenated, are the loader's stream
    (FileDataset.configure(group=K) orders an epoch so that the groups are full).  The pinned slot and the static device set hold
    K samples: `raw` K * raw capacity bytes with sample i at i * raw capacity, `desc` [K, 4], `adesc` [K, 12], `boxes`
    [K, cap, 4], `ids` [K, cap], `nobj` [K]; only the used bytes of every raw image are uploaded.  `features()` of a group of j
    is rn_resize_pair_u8_batch (or _augment_batch) + ONE paired assignment over j images: `image` [2j, oh, ow, 3], sample i in
    slots 2i / 2i+1, bit for bit what K = 1 yields for it.  The shape key is (oh, ow, object capacity, generation, j): a partial
    group is a key -- a graph set -- of its own.  Sample m of the stream is still drawn at ordinal first_ordinal + m, whatever
    the grouping; `samples_staged` counts samples, `last_sample` is the list of the group's infos."""

    MAX_SAMPLES_PER_STEP = 16

    def __init__(self, data_loader, levels, scale=None, device='cuda', max_obj=32, normalize=True, prefetch=3, ragged=False,
                 decode_workers=4, augment=None, first_ordinal=0, samples_per_step=1):
        import queue
        import threading
        self.augment = _policy_or_none(augment)        # (checked before anything touches the device)
        if self.augment is not None and not ragged:
            raise ValueError("DeviceFeed(augment=policy) needs ragged=True: the augmentation kernel reads the raw uint8 image")
        self.samples_per_step = int(samples_per_step)
        if not 1 <= self.samples_per_step <= self.MAX_SAMPLES_PER_STEP:
            raise ValueError("DeviceFeed(samples_per_step=%r): 1 .. %d" % (samples_per_step, self.MAX_SAMPLES_PER_STEP))
        if self.samples_per_step > 1 and not ragged:
            raise ValueError("DeviceFeed(samples_per_step=%d) needs ragged=True: the batched preprocess kernels read raw uint8 "
                             "images" % self.samples_per_step)
        self.levels, self.scale, self.normalize = levels, scale, normalize
        self.num_classes = data_loader.num_classes
        self.device = torch.device(device)
        self.max_obj = int(max_obj)
        self.ragged = bool(ragged)
        self._rank = int(getattr(data_loader, 'rank', 0))
        self._ordinal = int(first_ordinal)
        if self.ragged:
            self._it = iter(decoded(data_loader, decode_workers))
            px = getattr(data_loader, 'max_image_pixels', None)
            ob = getattr(data_loader, 'max_objects', None)
            self._raw_cap = 3 * int(px()) if callable(px) else 0          # bytes
            self._obj_cap = max(self.max_obj, -(-int(ob()) // 32) * 32) if callable(ob) else self.max_obj
            self._generation = 0 if self._raw_cap > 0 else -1            # -1: nothing allocated yet
            self.generations = 0                                         # static device sets allocated so far
        else:
            self._it = iter(data_loader)
        self._slots = int(prefetch)
        self._free = queue.Queue()
        self._ready = queue.Queue()
        for _ in range(self._slots):
            self._free.put(None)                    # a slot is (host tensors, upload-done event); created lazily per shape
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._consumed = None                       # event: segment A of the previous step has read the static buffers
        self._static = None
        self._statics = {}                          # shape key -> static device buffers
        self.shape_key = None
        self.last_sample = None                     # host-side boxes / class ids of the staged sample (evaluation, logging)
        self.samples_staged = 0
        self._stop = False
        self._error = None
        self._thread = threading.Thread(target=self._produce, name='rn-device-feed', daemon=True)
        self._started = False

    def start(self):
        """Start the loader thread (stage() does it on first use; call it earlier to prefetch)."""
        if not self._started:
            self._started = True
            self._thread.start()

    # -- host side: loader thread
    def _produce(self):
        if self.ragged and self.samples_per_step > 1:
            return self._produce_groups()
        if self.ragged:
            return self._produce_ragged()
        try:
            for sample in self._it:
                slot = self._free.get()
                if self._stop:
                    return
                if slot is not None and slot[1] is not None:
                    slot[1].synchronize()           # the upload that last used this slot's pinned memory is done
                img = np.ascontiguousarray(sample['image'])
                ids = np.asarray(sample['class_ids'], np.int32).reshape(-1)
                h, w = int(img.shape[0]), int(img.shape[1])
                boxes = (np.asarray(sample['boxes'], np.float32).reshape(-1, 4) / np.asarray([h, w, h, w], np.float32))   # dataset.py:163
                cap = max(self.max_obj, -(-len(ids) // 32) * 32)
                host = slot[0] if slot is not None else None
                if host is None or tuple(host['image'].shape) != img.shape or host['image'].dtype != torch.from_numpy(img).dtype \
                        or host['boxes'].shape[1] != cap:
                    host = {'image': torch.empty(img.shape, dtype=torch.from_numpy(img).dtype).pin_memory(),
                            'boxes': torch.zeros((1, cap, 4), dtype=torch.float32).pin_memory(),
                            'ids': torch.zeros((1, cap), dtype=torch.int32).pin_memory(),
                            'nobj': torch.zeros((1,), dtype=torch.int32).pin_memory()}
                host['image'].numpy()[...] = img
                host['boxes'].zero_(); host['ids'].zero_()
                host['boxes'].numpy()[0, :len(ids)] = boxes
                host['ids'].numpy()[0, :len(ids)] = ids
                host['nobj'][0] = len(ids)
                self._ready.put((host, {'boxes': boxes, 'class_ids': ids, 'image_hw': (h, w)}))
            self._ready.put(None)
        except BaseException as e:                  # surfaces in stage() on the training thread
            self._error = e
            self._ready.put(None)

    def _produce_ragged(self):
        try:
            for sample in self._it:
                slot = self._free.get()
                if self._stop:
                    return
                if slot is not None and slot[1] is not None:
                    slot[1].synchronize()
                img = np.ascontiguousarray(sample['image'])
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                    raise ValueError("DeviceFeed(ragged=True) stages uint8 [H, W, 3] images, got %s %s" % (img.dtype, img.shape))
                ids = np.asarray(sample['class_ids'], np.int32).reshape(-1)
                h, w = int(img.shape[0]), int(img.shape[1])
                boxes = (np.asarray(sample['boxes'], np.float32).reshape(-1, 4) / np.asarray([h, w, h, w], np.float32))   # dataset.py:163
                if img.size > self._raw_cap or len(ids) > self._obj_cap:          # no hints, or a sample beyond them: grow
                    self._raw_cap = max(img.size, -(-self._raw_cap * 3 // 2))
                    self._obj_cap = max(self._obj_cap, -(-len(ids) // 32) * 32)
                    self._generation += 1
                oh, ow = rescale_size((h, w), self.scale) if self.scale is not None else (h, w)
                info = {}
                if self.augment is not None:
                    values, boxes, ids = self.augment.draw(self._rank, self._ordinal, (h, w), boxes, ids)
                    self._ordinal += 1
                    info['augment_desc'] = augment_desc((h, w), values, (oh, ow))
                host = slot[0] if slot is not None else None
                if host is None or host['gen'] != self._generation:
                    host = {'gen': self._generation,
                            'raw': torch.empty((self._raw_cap,), dtype=torch.uint8).pin_memory(),
                            'desc': torch.zeros((4,), dtype=torch.int32).pin_memory(),
                            'boxes': torch.zeros((1, self._obj_cap, 4), dtype=torch.float32).pin_memory(),
                            'ids': torch.zeros((1, self._obj_cap), dtype=torch.int32).pin_memory(),
                            'nobj': torch.zeros((1,), dtype=torch.int32).pin_memory()}
                    if self.augment is not None:
                        host['adesc'] = torch.zeros((12,), dtype=torch.int32).pin_memory()
                host['raw'].numpy()[:img.size] = img.reshape(-1)
                host['desc'].numpy()[:] = resize_desc((h, w), (oh, ow))
                if self.augment is not None:
                    host['adesc'].numpy()[:] = info['augment_desc']
                host['boxes'].zero_(); host['ids'].zero_()
                host['boxes'].numpy()[0, :len(ids)] = boxes
                host['ids'].numpy()[0, :len(ids)] = ids
                host['nobj'][0] = len(ids)
                host['bytes'], host['size'] = img.size, (oh, ow)
                self._ready.put((host, dict(info, boxes=boxes, class_ids=ids, image_hw=(h, w))))
            self._ready.put(None)
        except BaseException as e:
            self._error = e
            self._ready.put(None)

    def _produce_groups(self):
        """_produce_ragged for samples_per_step > 1: one pinned slot per GROUP of up to K consecutive samples of one network
        input size (see the class docstring)."""
        K = self.samples_per_step
        try:
            peeked = None                            # the sample looked at to close the previous group: it opens this one
            while True:
                group, size = [], None
                while len(group) < K:
                    if peeked is None:
                        peeked = next(self._it, None)
                        if peeked is None:
                            break
                    img = np.asarray(peeked['image'])
                    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                        raise ValueError("DeviceFeed(ragged=True) stages uint8 [H, W, 3] images, got %s %s" % (img.dtype, img.shape))
                    hw = (int(img.shape[0]), int(img.shape[1]))
                    sz = rescale_size(hw, self.scale) if self.scale is not None else hw
                    if group and sz != size:
                        break
                    group.append(peeked)
                    size, peeked = sz, None
                if not group:
                    break
                slot = self._free.get()
                if self._stop:
                    return
                if slot is not None and slot[1] is not None:
                    slot[1].synchronize()
                images = [np.ascontiguousarray(sample['image']) for sample in group]
                infos = []
                for img, sample in zip(images, group):
                    ids = np.asarray(sample['class_ids'], np.int32).reshape(-1)
                    h, w = int(img.shape[0]), int(img.shape[1])
                    boxes = (np.asarray(sample['boxes'], np.float32).reshape(-1, 4) / np.asarray([h, w, h, w], np.float32))   # dataset.py:163
                    info = {}
                    if self.augment is not None:
                        values, boxes, ids = self.augment.draw(self._rank, self._ordinal, (h, w), boxes, ids)
                        self._ordinal += 1
                        info['augment_desc'] = augment_desc((h, w), values, size)
                    infos.append(dict(info, boxes=boxes, class_ids=ids, image_hw=(h, w)))
                need_raw = max(img.size for img in images)
                need_obj = max(len(info['class_ids']) for info in infos)
                if need_raw > self._raw_cap or need_obj > self._obj_cap:          # no hints, or a sample beyond them: grow
                    self._raw_cap = max(need_raw, -(-self._raw_cap * 3 // 2))
                    self._obj_cap = max(self._obj_cap, -(-need_obj // 32) * 32)
                    self._generation += 1
                host = slot[0] if slot is not None else None
                if host is None or host['gen'] != self._generation:
                    host = {'gen': self._generation, 'stride': self._raw_cap,
                            'raw': torch.empty((K * self._raw_cap,), dtype=torch.uint8).pin_memory(),
                            'desc': torch.zeros((K, 4), dtype=torch.int32).pin_memory(),
                            'boxes': torch.zeros((K, self._obj_cap, 4), dtype=torch.float32).pin_memory(),
                            'ids': torch.zeros((K, self._obj_cap), dtype=torch.int32).pin_memory(),
                            'nobj': torch.zeros((K,), dtype=torch.int32).pin_memory()}
                    if self.augment is not None:
                        host['adesc'] = torch.zeros((K, 12), dtype=torch.int32).pin_memory()
                host['boxes'].zero_(); host['ids'].zero_(); host['nobj'].zero_()
                for i, (img, info) in enumerate(zip(images, infos)):
                    n = len(info['class_ids'])
                    host['raw'].numpy()[i * host['stride']:i * host['stride'] + img.size] = img.reshape(-1)
                    host['desc'].numpy()[i] = resize_desc(info['image_hw'], size)
                    if self.augment is not None:
                        host['adesc'].numpy()[i] = info['augment_desc']
                    host['boxes'].numpy()[i, :n] = info['boxes']
                    host['ids'].numpy()[i, :n] = info['class_ids']
                    host['nobj'][i] = n
                host['bytes'], host['size'] = [img.size for img in images], size
                self._ready.put((host, infos))
            self._ready.put(None)
        except BaseException as e:
            self._error = e
            self._ready.put(None)

    def _stage_group(self, host, cur):
        """_stage_ragged for samples_per_step > 1: the first j = len(host['bytes']) samples of the K-sample static set."""
        j = len(host['bytes'])
        key = (host['size'][0], host['size'][1], int(host['boxes'].shape[1]), host['gen'], j)
        if self._static is None or self._static['gen'] != host['gen']:
            self._static = {k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in host.items()
                            if isinstance(v, torch.Tensor)}
            self._static['gen'], self._static['stride'] = host['gen'], host['stride']
            self.generations += 1
        self.shape_key = key
        self._size, self._group = host['size'], j
        cs = self._copy_stream
        if self._consumed is not None:
            cs.wait_event(self._consumed)
        else:
            cs.wait_stream(cur)
        with torch.cuda.stream(cs):
            for i, n in enumerate(host['bytes']):
                lo = i * host['stride']
                self._static['raw'][lo:lo + n].copy_(host['raw'][lo:lo + n], non_blocking=True)
            for k in ('desc', 'boxes', 'ids', 'nobj') + (('adesc',) if 'adesc' in host else ()):
                self._static[k][:j].copy_(host[k][:j], non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        return key, done

    def _features_group(self):
        s, j = self._static, self._group
        oh, ow = self._size
        if self.augment is not None:
            pairs = resize_pair_u8_augment_batch(s['raw'], s['adesc'][:j], (oh, ow), s['stride'], normalize=self.normalize)
        else:
            pairs = resize_pair_u8_batch(s['raw'], s['desc'][:j], (oh, ow), s['stride'], normalize=self.normalize)
        c, r, m = build_labels((oh, ow), s['ids'][:j], s['boxes'][:j], self.levels, self.num_classes, num_obj=s['nobj'][:j],
                               flip_pair=True)
        return {'image': pairs, 'image_size': (oh, ow), 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m}

    def _stage_ragged(self, host, cur):
        """stage() of the ragged mode: one static set per generation (the previous one is dropped with its generation)."""
        key = (host['size'][0], host['size'][1], int(host['boxes'].shape[1]), host['gen'])
        if self._static is None or self._static['gen'] != host['gen']:
            self._static = {k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in host.items()
                            if isinstance(v, torch.Tensor)}
            self._static['gen'] = host['gen']
            self.generations += 1
        self.shape_key = key
        self._size = host['size']
        cs = self._copy_stream
        if self._consumed is not None:
            cs.wait_event(self._consumed)
        else:
            cs.wait_stream(cur)
        with torch.cuda.stream(cs):
            n = host['bytes']
            self._static['raw'][:n].copy_(host['raw'][:n], non_blocking=True)
            for k in ('desc', 'boxes', 'ids', 'nobj') + (('adesc',) if 'adesc' in host else ()):
                self._static[k].copy_(host[k], non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        return key, done

    def _features_ragged(self):
        s = self._static
        oh, ow = self._size
        if self.augment is not None:
            pair = resize_pair_u8_augment(s['raw'], s['adesc'], (oh, ow), normalize=self.normalize)
        else:
            pair = resize_pair_u8(s['raw'], s['desc'], (oh, ow), normalize=self.normalize)
        c, r, m = build_labels((oh, ow), s['ids'], s['boxes'], self.levels, self.num_classes, num_obj=s['nobj'], flip_pair=True)
        return {'image': pair, 'image_size': (oh, ow), 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m}

    def close(self):
        self._stop = True
        for _ in range(self._slots + 1):
            self._free.put(None)

    # -- device side
    def stage(self):
        """Upload the next sample into the static buffers (copy stream) and make the current stream wait for it.  Returns
        the shape key (changes when new static buffers had to be made: the caller captures a new graph for it)."""
        self.start()
        item = self._ready.get()
        if item is None:
            if self._error is not None:
                raise self._error
            raise StopIteration
        host, info = item
        cur = torch.cuda.current_stream(self.device)
        if self.ragged and self.samples_per_step > 1:
            key, done = self._stage_group(host, cur)
            self._free.put((host, done))
            self.last_sample = info                 # the list of the group's infos
            self.samples_staged += len(info)
            return key
        if self.ragged:
            key, done = self._stage_ragged(host, cur)
            self._free.put((host, done))
            self.last_sample = info
            self.samples_staged += 1
            return key
        key = (tuple(host['image'].shape), str(host['image'].dtype), int(host['boxes'].shape[1]))
        if key != self.shape_key:
            if key not in self._statics:
                self._statics[key] = {k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in host.items()}
            self._static, self.shape_key = self._statics[key], key
        cs = self._copy_stream
        if self._consumed is not None:
            cs.wait_event(self._consumed)           # the previous segment A no longer reads the buffers
        else:
            cs.wait_stream(cur)
        with torch.cuda.stream(cs):
            for k, v in host.items():
                self._static[k].copy_(v, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        cur.wait_event(done)
        self._free.put((host, done))
        self.last_sample = info
        self.samples_staged += 1
        return key

    def consumed(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._consumed = ev

    def features(self):
        """The step's features from the static buffers (inside the captured segment when the trainer runs graphs)."""
        if self.ragged and self.samples_per_step > 1:
            return self._features_group()
        if self.ragged:
            return self._features_ragged()
        s = self._static
        return sample_batch(s['image'], s['boxes'], s['ids'], self.levels, self.num_classes, scale=self.scale,
                            num_obj=s['nobj'], normalize=self.normalize)

    __call__ = features
