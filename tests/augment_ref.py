"""numpy restatement of the augmentation contract (csrc/preprocess.hip, "augmented pair"), for the tests.

r (step 1) comes from oracle.dataset_ref -- the fp32 restatement of convert_image_dtype + ResizeBilinear the device reproduces
bit for bit -- applied to a contiguous copy of the crop window; steps 2-5 are evaluated in fp64 from the fp32 values the device
descriptor holds, with m_c the fp64 channel mean of r rounded once to fp32."""
import numpy as np

from oracle import dataset_ref


def resized(image, window, size):
    """Step 1: image uint8 [H, W, 3], window (y0, x0, ch, cw), size (oh, ow) -> r fp32 [oh, ow, 3]."""
    y0, x0, ch, cw = window
    crop = np.ascontiguousarray(image[y0:y0 + ch, x0:x0 + cw])
    return dataset_ref.resize_bilinear_align_corners(crop[None], int(size[0]), int(size[1]))[0]


def transform(r, f, d, k, normalize=True):
    """Steps 2-5 in fp64 on r fp32 [oh, ow, 3]; f, d, k are taken as the fp32 values of the descriptor."""
    f, d, k = (np.float64(np.float32(v)) for v in (f, d, k))
    r64 = r.astype(np.float64)
    m = r64.reshape(-1, 3).mean(axis=0, dtype=np.float64).astype(np.float32).astype(np.float64)
    a = (r64 - m) * f + m
    b = np.clip(a + d, 0.0, 1.0)
    M, n = b.max(axis=-1, keepdims=True), b.min(axis=-1, keepdims=True)
    grey = M == n
    span = np.where(grey, 1.0, M - n)
    s = np.where(grey, b, M - (M - b) * np.minimum(k, M / span))
    if normalize:
        s = (s - dataset_ref.MEAN.astype(np.float64)) / dataset_ref.STD.astype(np.float64)
    return s


def expected_pair(image, window, f, d, k, size, normalize=True):
    """[2, oh, ow, 3] fp64: slot 0 and its h-flip."""
    s = transform(resized(image, window, size), f, d, k, normalize)
    return np.stack([s, s[:, ::-1]])
