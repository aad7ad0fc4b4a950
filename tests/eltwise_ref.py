"""References and case tables for the elementwise kernels of csrc/elementwise.hip: max / average pool, lateral + upsampled top
(and its gradient), stand-alone activations, rn_add_segs and rn_flip_width.

The references are the oracle's (oracle.tf_ops_ref: max_pool_same, avg_pool_same, upsample_nearest_align_corners, activation)
in a chosen dtype, gradients by autograd; argmax_taps restates the max pool's first-maximum rule in numpy, independently of both.
elementwise.hip has one host rule, grid_for (ceil(total / 256) blocks, at most 4096, at least 1): `blocks` models it here,
in Python -- there is no plan query for this file -- and tests/test_eltwise_cases_cpu.py uses the model to prove that the
grid-cap cases are above the cap.  tests/test_gpu_eltwise_cases.py runs the tables on the GPU."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tf_ops_ref as T

U = 2.0 ** -24          # unit roundoff of fp32
GRID_CAP, BLOCK = 4096, 256


def blocks(total):
    """A Python model of grid_for in elementwise.hip (the file's only host rule)."""
    return max(1, min(GRID_CAP, -(-total // BLOCK)))


# ------------------------------------------------------------------------------------------------------------------ pools
Pool = collections.namedtuple("Pool", "n h w c k s")
POOL_SHAPES = [(2, 16, 16, 64), (1, 7, 9, 8), (1, 1, 1, 4), (1, 2, 2, 4)]          # (1, 2, 2, 4): k > h
POOL_KS = [(3, 2), (2, 2), (3, 1), (2, 1), (3, 3)]
POOL_GRID_CAP = Pool(2, 130, 130, 128, 3, 1)
POOLS = [Pool(*shape, k, s) for shape in POOL_SHAPES for k, s in POOL_KS] + [POOL_GRID_CAP]
POOLS_F16 = [Pool(2, 16, 16, 64, 3, 2), Pool(1, 7, 9, 8, 2, 1)]
CONTINUOUS, RELU, INTEGERS = "continuous", "relu", "integers"
TIED = (RELU, INTEGERS)
RELU_SHIFT = 1.5        # relu(standard_normal - 1.5): see pool_input


def pool_id(p):
    return "%dx%dx%dx%d-k%ds%d" % p


def pool_out(p):
    return T.same_pad_1d(p.h, p.k, p.s)[0], T.same_pad_1d(p.w, p.k, p.s)[0]


@functools.lru_cache(maxsize=None)
def pool_input(p, kind):
    """-> (x [n,h,w,c], dy [n,oh,ow,c]) fp32 CPU tensors (shared: read-only).  kind: continuous (standard normal: no two cells
    equal), relu (a post-ReLU map: exact zeros) or integers in {-1, 0, 1}.  A plain relu(standard_normal) ties in a 3x3 window
    only where all nine cells are negative, 1 window in 512: the normal is shifted down by RELU_SHIFT, as after a GroupNorm
    with a negative beta, so that most windows are all zero and tie.  A 2 x 2 map has a handful of windows: the first draw in
    which a quarter of them tie is taken (a property of the input alone)."""
    assert kind in (CONTINUOUS, RELU, INTEGERS)
    rng = np.random.default_rng(5000 + sum(a * b for a, b in zip(p, (1, 3, 5, 7, 11, 13))))
    for _ in range(100):
        x = rng.standard_normal((p.n, p.h, p.w, p.c), dtype=np.float32)
        if kind == RELU:
            x = np.maximum(x - np.float32(RELU_SHIFT), np.float32(0))
        elif kind == INTEGERS:
            x = rng.integers(-1, 2, x.shape).astype(np.float32)
        if kind == CONTINUOUS or p.h * p.w == 1 or tied_fraction(x, p.k, p.s) >= 0.25:
            break
    oh, ow = pool_out(p)
    dy = rng.standard_normal((p.n, oh, ow, p.c), dtype=np.float32)
    return torch.from_numpy(x), torch.from_numpy(dy)


def window_taps(x, k, s):
    """-> [k*k, n, oh, ow, c] float64: the cells of every window in tap order kh * k + kw, padded cells -inf"""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    oh, pt, pb = T.same_pad_1d(h, k, s)
    ow, pl, pr = T.same_pad_1d(w, k, s)
    xp = np.full((n, h + pt + pb, w + pl + pr, c), -np.inf)
    xp[:, pt:pt + h, pl:pl + w] = x
    return np.stack([xp[:, a:a + (oh - 1) * s + 1:s, b:b + (ow - 1) * s + 1:s] for a in range(k) for b in range(k)])


def argmax_taps(x, k, s):
    """-> uint8 [n,oh,ow,c]: the tap index of the FIRST maximum of each window in row-major order (padded cells never win)"""
    return np.argmax(window_taps(x, k, s), axis=0).astype(np.uint8)          # (np.argmax: the first occurrence)


def tied_fraction(x, k, s):
    """The fraction of windows whose maximum occurs more than once."""
    taps = window_taps(x, k, s)
    return float(((taps == taps.max(axis=0)).sum(axis=0) >= 2).mean())


def windows_per_cell(p):
    """-> [h, w]: the number of windows that contain each cell"""
    x = torch.zeros((1, p.h, p.w, 1), dtype=torch.float64, requires_grad=True)
    _, pt, pb = T.same_pad_1d(p.h, p.k, p.s)
    _, pl, pr = T.same_pad_1d(p.w, p.k, p.s)
    y = F.avg_pool2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), p.k, p.s) * (p.k * p.k)
    return np.rint(torch.autograd.grad(y.sum(), x)[0][0, :, :, 0].numpy())


def valid_cells(p):
    """-> [oh, ow]: the un-padded cells of each window"""
    return np.isfinite(window_taps(np.zeros((1, p.h, p.w, 1)), p.k, p.s)).sum(axis=0)[0, :, :, 0]


def pool_ref(which, x, dy, k, s, dtype):
    """-> (y, dx) numpy arrays: the oracle's max / avg pool in `dtype` and its autograd for the cotangent dy"""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    y = (T.max_pool_same if which == "max" else T.avg_pool_same)(x, k, s)
    dx, = torch.autograd.grad(y, x, dy.to(dtype))
    return y.detach().numpy(), dx.numpy()


def dx_from_argmax(arg, dy, p):
    """The max pool's gradient scattered by tap index (float64): what 'the first maximum gets it' means."""
    n, oh, ow, c = dy.shape
    _, pt, _ = T.same_pad_1d(p.h, p.k, p.s)
    _, pl, _ = T.same_pad_1d(p.w, p.k, p.s)
    dx = np.zeros((n, p.h, p.w, c))
    ni, oi, oj, ci = np.meshgrid(np.arange(n), np.arange(oh), np.arange(ow), np.arange(c), indexing="ij")
    np.add.at(dx, (ni, oi * p.s - pt + arg // p.k, oj * p.s - pl + arg % p.k, ci), np.asarray(dy, dtype=np.float64))
    return dx


# ----------------------------------------------------------------------------------------------------------- upsample-add
Up = collections.namedtuple("Up", "n c th h tw w")
_SWEEP = [(th, h) for th in range(1, 9) for h in range(th, 3 * th + 3)]
UPS = ([Up(1, 4, th, h, *_SWEEP[(i + 37) % len(_SWEEP)]) for i, (th, h) in enumerate(_SWEEP)] +
       [Up(2, 8, 38, 75, 38, 75), Up(1, 4, 5, 3, 7, 4), Up(1, 4, 8, 1, 3, 2)])          # the last two shrink (h < th)
UPS_F16 = [next(u for u in UPS if (u.th, u.h) == (2, 3)), Up(2, 8, 38, 75, 38, 75), Up(1, 4, 5, 3, 7, 4)]   # (3 <- 2: a roundf tie)


def up_input(u, seed=0):
    rng = np.random.default_rng(6000 + seed)
    lat = rng.standard_normal((u.n, u.h, u.w, u.c), dtype=np.float32)
    top = rng.standard_normal((u.n, u.th, u.tw, u.c), dtype=np.float32)
    dy = rng.standard_normal((u.n, u.h, u.w, u.c), dtype=np.float32)
    return torch.from_numpy(lat), torch.from_numpy(top), torch.from_numpy(dy)


def up_ref(lat, top, dy, dtype):
    """-> (y, dtop) numpy arrays: lateral + the oracle's nearest-neighbour resize of top, and autograd's gradient of top"""
    top = top.detach().to(dtype).clone().requires_grad_(True)
    y = lat.to(dtype) + T.upsample_nearest_align_corners(top, lat.shape[1], lat.shape[2])
    dtop, = torch.autograd.grad(y, top, dy.to(dtype))
    return y.detach().numpy(), dtop.numpy()


def up_sources(u):
    """-> [th, tw]: the number of fine cells that read each coarse cell (terms of a dtop element)"""
    cy = np.bincount(T.nn_resize_index(u.h, u.th), minlength=u.th)
    cx = np.bincount(T.nn_resize_index(u.w, u.tw), minlength=u.tw)
    return np.outer(cy, cx)


def has_rounding_tie(out_size, in_size):
    """Does some dst * scale (float32, as the kernel and nn_resize_index form it) lie exactly on x.5?"""
    if out_size < 2:
        return False
    scale = np.float32(in_size - 1) / np.float32(out_size - 1)
    v = np.arange(out_size, dtype=np.float32) * scale
    return bool(np.any(v - np.floor(v) == np.float32(0.5)))


# ------------------------------------------------------------------------------------------------------------ activations
ACTS = [(0, None), (1, "relu"), (2, "elu"), (3, "relu6"), (4, "sigmoid")]          # enum rn_act
ACT_COUNTS = [1, 3, 255, 256, 257, 4096 * 256 + 5]
_f = np.float32
SPECIALS = np.array([0.0, -0.0, 6.0, np.nextafter(_f(0), _f(1)), np.nextafter(_f(0), _f(-1)), np.nextafter(_f(6), _f(7)),
                     np.nextafter(_f(6), _f(0)), 88.0, -88.0, 100.0, -100.0], dtype=np.float32)


def act_input(count):
    """-> (x, dy): the kinks (0, -0, 6), their neighbours, +-88, +-100, then 3 x standard normal; a count below the list's length
    starts the list at index `count`, so that the short counts together see the kinks too"""
    rng = np.random.default_rng(7000 + count)
    x = (3 * rng.standard_normal(count + len(SPECIALS))).astype(np.float32)
    x[:len(SPECIALS)] = np.roll(SPECIALS, -count if count < len(SPECIALS) else 0)
    dy = rng.standard_normal(count).astype(np.float32)
    return torch.from_numpy(x[:count].copy()), torch.from_numpy(dy)


def act_ref(x, dy, kind, dtype):
    x = x.detach().to(dtype).clone().requires_grad_(True)
    y = T.activation(x, kind)
    if not y.requires_grad:          # (identity of a leaf)
        y = x * 1
    dx, = torch.autograd.grad(y, x, dy.to(dtype))
    return y.detach().numpy(), dx.numpy()
