"""The tail of the training step in float64, for the tests: the detection loss with its gradients and statistics
(csrc/loss.hip) and the optimizer update with the global norm and the L2 regulariser (csrc/optimizer.hip), plus the seeded
inputs that the CPU test (test_step_tail_ref_cpu.py) and the GPU test (test_gpu_step_tail.py) share byte for byte.

Loss: oracle.losses_ref.loss on float64 tensors over the compacted trainable rows, gradients by autograd; indexing with the
mask scatters them back to full size with zeros on the masked rows.  M = #trainable rows, #fg = trainable rows whose largest
label exceeds 0.5, and per class I_c = sum l p, L_c = sum l, P_c = sum p over the trainable rows, p = sigmoid(z).

Optimizer, on the flat arena (every parameter padded to a multiple of 1024 with zeros):
    g' = grad * grad_scale + wd * w,   norm = sqrt(sum g'^2),   reg = sum 0.5 * wd * w^2,   g' *= clip / max(norm, clip)
then oracle.train_ref.apply_optimizer on float64 tensors.  The padding takes part with w = 0 and grad = 0, so what the
reference leaves there is the initial state evolved on a zero gradient."""
import collections
import functools

import numpy as np
import torch

from oracle import losses_ref, train_ref

MAX_SEG = 16          # RN_MAX_SEG
OPT_BLOCK = 1024      # RN_OPT_BLOCK
G_CLS, G_REG = 1.7, 0.6

# ------------------------------------------------------------------------------------------------------------------ loss

# 1512 rows = 94 groups of 16 and 8 more; boundaries at 37, 38, 288, 303: rows 32..47 hold segments 0, 1 and 2
SEG_ROWS = (37, 1, 250, 15, 1209)
# RN_MAX_SEG segments, unequal, one-row ones among them; 440 rows = 27 groups of 16 and 8 more
SEG_ROWS_MAX = (1, 7, 33, 1, 16, 5, 64, 1, 19, 2, 130, 1, 47, 3, 9, 101)
# the four-lane kernels run 2048 blocks x 4 waves x 2 groups x 16 rows = 262144 rows in one pass of their grid
SEG_ROWS_WRAP4 = (200000, 62144 + 389)
# the wave-per-row kernels run 2048 blocks x 4 waves x 4 rows = 32768 rows in one pass
SEG_ROWS_WRAP1 = (40000,)

C_FOUR_LANE = (4, 16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 116, 128)   # smallest and largest C of every NK
C_WAVE_PER_ROW = (1, 2, 63, 65, 129, 255, 256)

BCE_PLANT = (8.0, -8.0, 17.0, -17.0, 30.0, -30.0, 90.0, -90.0)
FOCAL_PLANT = (-90.0, -30.0, -17.0, -12.0, -8.0, 4.0, 6.0, 8.0, 12.0, 17.0, 30.0, 90.0)
FOCAL_ILL = (12.0, 17.0, 30.0, 90.0)     # 1 - p cancels against eps = 1e-7 in float32: not compared with float64
N_PLANT = 24

LossInputs = collections.namedtuple("LossInputs", "c seg_rows z lab rp rl mask planted empty_class")


def _segments(inp, a):
    out, r0 = [], 0
    for n in inp.seg_rows:
        out.append(a[r0:r0 + n])
        r0 += n
    return out


def segments(inp):
    """Per segment (z, lab, rp, rl, mask): contiguous row ranges of the full arrays."""
    return list(zip(*[_segments(inp, a) for a in (inp.z, inp.lab, inp.rp, inp.rl, inp.mask)]))


def loss_inputs(seed, c, seg_rows=SEG_ROWS, fg_rate=0.08, train_rate=0.8, plant=None):
    """Logits N(-2, 2), one-hot labels on about `fg_rate` of the rows (at least one row per class where the rows allow it, so
    that every class has a positive -- except class c // 2, left empty on purpose when c >= 3), about `train_rate` of the rows
    trainable (every foreground row is).  Box errors N(0, 1.8) on both sides of the Huber knee, none within 0.01 of zero: there the
    float32 oracle's own backward, (g q + g) - g, is rounding noise of the size of the CPU test's bound.  `plant`: a tuple of logit values written to N_PLANT positions on trainable rows, the
    first half under a label of 1 and the second under a label of 0; `planted` lists them as (row, class, value)."""
    rng = np.random.default_rng(seed)
    rows = int(sum(seg_rows))
    z = (rng.standard_normal((rows, c)) * 2 - 2).astype(np.float32)
    lab = np.zeros((rows, c), np.float32)
    empty = c // 2 if c >= 3 else None
    classes = np.array([k for k in range(c) if k != empty])
    n_fg = max(int(round(fg_rate * rows)), min(len(classes), rows // 4))
    fg_rows = rng.choice(rows, n_fg, replace=False)
    fg_cls = classes[(np.arange(n_fg) + rng.integers(0, c)) % len(classes)]
    lab[fg_rows, fg_cls] = 1.0
    rp = rng.standard_normal((rows, 4)).astype(np.float32)
    rl = (rng.standard_normal((rows, 4)) * 1.5).astype(np.float32)
    near = np.abs(rl - rp) < 0.01
    rl[near] = (rp + np.where(rl >= rp, np.float32(0.01), np.float32(-0.01)))[near]
    mask = rng.uniform(size=rows) < train_rate
    mask[fg_rows] = True
    planted = []
    if plant is not None:
        # a saturated logit under a label of 1 belongs to a class the model predicts often: the classes get logit offsets
        # from -2 to 2 and the first half goes to the upper third.  (In float32 p(1 - p) is exactly 0 at z = 17 where float64
        # has 4e-8: with every class alike that alone is 1.4e-4 of the element-wise floor, in the oracle as in any kernel.)
        offset = np.linspace(-2.0, 2.0, c).astype(np.float32)
        z += offset
        often = np.flatnonzero(offset[fg_cls] >= offset[classes][np.argsort(offset[classes])[-max(1, len(classes) // 3)]])
        half = N_PLANT // 2
        pos = rng.choice(often, half, replace=False)
        spots = [(int(fg_rows[i]), int(fg_cls[i])) for i in pos]
        bg_rows = rng.choice(np.flatnonzero(mask & (lab.max(1) == 0)), half, replace=False)
        spots += [(int(r), int(rng.integers(0, c))) for r in bg_rows]
        for i, (r, k) in enumerate(spots):
            z[r, k] = plant[i % len(plant)]
            planted.append((r, k, float(plant[i % len(plant)])))
    return LossInputs(c, tuple(seg_rows), z, lab, rp, rl, mask, tuple(planted), empty)


def _small_end(kind, c):
    """The small ends: `one_row` (one row in all, trainable and foreground), `m1` (one trainable row among many masked ones),
    `one_fg` (exactly one foreground row)."""
    if kind == "one_row":
        inp = loss_inputs(700 + c, c, seg_rows=(1,))
        lab = np.zeros_like(inp.lab)
        lab[0, c - 1] = 1.0
        return inp._replace(lab=lab, mask=np.ones(1, bool), empty_class=None)
    inp = loss_inputs(710 + c, c, seg_rows=(23, 1, 70))
    if kind == "m1":
        mask = np.zeros_like(inp.mask)
        mask[int(np.flatnonzero(inp.lab.max(1) > 0)[1])] = True
        return inp._replace(mask=mask, empty_class=None)
    assert kind == "one_fg"
    lab = np.zeros_like(inp.lab)
    lab[40, 0] = 1.0
    mask = inp.mask.copy()
    mask[40] = True
    return inp._replace(lab=lab, mask=mask, empty_class=None)


def _with_nonfinite_masked_rows(inp):
    """NaN, +inf and -inf logits on twelve rows outside the trainable mask, spread over the row range, single elements and
    whole rows: the reference removes those rows, so nothing may change.  Returns (inputs, the rows touched)."""
    z = inp.z.copy()
    masked = np.flatnonzero(~inp.mask)
    rows = masked[np.linspace(0, len(masked) - 1, 12).astype(int)]
    vals = (np.nan, np.inf, -np.inf)
    for i, r in enumerate(rows):
        z[r, i % inp.c] = vals[i % 3]
        if i % 4 == 0:
            z[r, :] = vals[(i // 4) % 3]
    return inp._replace(z=z), rows


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """The input sets by name.  `sweep-C`, `maxseg-C`, `wrap4` / `wrap1` (the grids' second pass), `plant-MODE-C` (saturated
    logits), `clean-C` / `nonfinite-C` (the masking rule: equal but for non-finite logits on masked rows), `one_row-C`, `m1-C`,
    `one_fg-C`."""
    kind, _, rest = name.partition("-")
    if kind == "sweep":
        return loss_inputs(1000 + int(rest), int(rest))
    if kind == "maxseg":
        return loss_inputs(2000 + int(rest), int(rest), seg_rows=SEG_ROWS_MAX)
    if kind == "wrap4":
        return loss_inputs(3004, 4, seg_rows=SEG_ROWS_WRAP4)
    if kind == "wrap1":
        return loss_inputs(3003, 3, seg_rows=SEG_ROWS_WRAP1)
    if kind == "plant":
        mode, c = rest.split("-")
        return loss_inputs(4000 + int(c), int(c), plant=BCE_PLANT if mode == "bce_dice" else FOCAL_PLANT)
    if kind == "clean":
        return loss_inputs(5000 + int(rest), int(rest))
    if kind == "nonfinite":
        return _with_nonfinite_masked_rows(loss_case("clean-" + rest))[0]
    if kind in ("one_row", "m1", "one_fg"):
        return _small_end(kind, int(rest))
    raise KeyError(name)


MASKING_C = (20, 3)          # four lanes per row (NK = 2, the Pascal VOC class count) and wave per row
SWEEP_CASES = tuple("sweep-%d" % c for c in C_FOUR_LANE + C_WAVE_PER_ROW)
MAXSEG_CASES = tuple("maxseg-%d" % c for c in MASKING_C)
WRAP_CASES = ("wrap4", "wrap1")
PLANT_CASES = tuple("plant-%s-%d" % (mode, c) for mode in ("bce_dice", "focal") for c in MASKING_C)
CLEAN_CASES = tuple("clean-%d" % c for c in MASKING_C)
SMALL_END_CASES = tuple("%s-%d" % (kind, c) for kind in ("one_row", "m1", "one_fg") for c in MASKING_C)


def nonfinite_rows(c):
    return _with_nonfinite_masked_rows(loss_case("clean-%d" % c))[1]


def ill_conditioned(inp, mode):
    """Boolean [rows, c]: in focal mode the planted logits of FOCAL_ILL, else nothing."""
    out = np.zeros(inp.z.shape, bool)
    for r, k, v in inp.planted:
        if mode == "focal" and v in FOCAL_ILL:
            out[r, k] = True
    return out


LossRef = collections.namedtuple("LossRef", "cls reg M nfg I L P dz dr")


def loss_ref(inp, mode, g_cls=G_CLS, g_reg=G_REG, dtype=torch.float64):
    """losses_ref.loss in `dtype` over the trainable rows and the gradient of g_cls * class loss + g_reg * regression loss
    (None: that loss takes no part) at full size, zeros on masked rows; the statistics always in float64."""
    m = torch.from_numpy(inp.mask)
    z = torch.from_numpy(inp.z).to(dtype).requires_grad_(True)
    rp = torch.from_numpy(inp.rp).to(dtype).requires_grad_(True)
    lab, rl = torch.from_numpy(inp.lab).to(dtype), torch.from_numpy(inp.rl).to(dtype)
    cl, rg = losses_ref.loss(lab[m], rl[m], z[m], rp[m], mode)
    total = 0.0
    if g_cls is not None:
        total = total + g_cls * cl
    if g_reg is not None:
        total = total + g_reg * rg
    total.backward()
    dz = z.grad.numpy() if z.grad is not None else np.zeros(inp.z.shape)
    dr = rp.grad.numpy() if rp.grad is not None else np.zeros(inp.rp.shape)
    l64 = torch.from_numpy(inp.lab).double()[m]
    p64 = torch.sigmoid(torch.from_numpy(inp.z).double()[m])
    return LossRef(cl.item(), rg.item(), int(m.sum()), int((l64.max(-1).values > 0.5).sum()) if l64.numel() else 0,
                   (l64 * p64).sum(0).numpy(), l64.sum(0).numpy(), p64.sum(0).numpy(), dz, dr)


# ------------------------------------------------------------------------------------------------------------- optimizer

OptInputs = collections.namedtuple("OptInputs", "sizes l2 offsets count w0 grads wd_elem grad_scale lr")

SMALL_SIZES = (1152, 700, 1, 1025, 3000)
SMALL_L2 = (0.3, 0.05, 1.0, None, 0.6)
# 2048 blocks x 256 threads x 4 elements = 2097152 elements in one pass of the optimizer's grid
LARGE_SIZES = (2097152 + 5 * 1024 + 7, 1500, 1024, 37)
LARGE_L2 = (0.2, 0.9, 0.07, 0.5)
CLIP_BINDS, CLIP_LOOSE = 0.5, 1e6
SMALL_SLICES = ((0, 2048), (2048, 4096), (4096, 9216))     # step_slice ranges over the small arena (9 blocks of 1024)


def optimizer_inputs(seed, sizes, l2, steps=3, grad_scale=0.5, lr=1e-2):
    """Weights N(0, 1) and per-step gradients in the arena's layout: every parameter starts on a multiple of OPT_BLOCK, zeros
    between them; `wd_elem` holds each parameter's l2 scale over its whole padded range, as train.ParamArena does.

    The gradients are drawn through g' = grad * grad_scale + wd * w0: each element's g' keeps one sign over the steps and has
    magnitude 0.25 + |N(0, 1)|.  Three steps move wd * w by 0.15 at the most, so no g' comes near zero, where float32 loses
    its relative accuracy to the cancellation (Adam then turns a sign error into a full-size update), and the momentum / Adam
    / RMSProp accumulators do not cancel to rounding noise either: the float32 oracle stays within the CPU test's bound."""
    rng = np.random.default_rng(seed)
    padded = [(s + OPT_BLOCK - 1) // OPT_BLOCK * OPT_BLOCK for s in sizes]
    count = int(sum(padded))
    w0 = np.zeros(count, np.float32)
    wd = np.zeros(count, np.float32)
    grads = [np.zeros(count, np.float32) for _ in range(steps)]
    offsets, off = [], 0
    for s, ps, scale in zip(sizes, padded, l2):
        w0[off:off + s] = rng.standard_normal(s).astype(np.float32)
        wd[off:off + ps] = scale or 0.0
        sign = np.where(rng.uniform(size=s) < 0.5, -1.0, 1.0)
        for g in grads:
            target = sign * (0.25 + np.abs(rng.standard_normal(s)))
            g[off:off + s] = ((target - np.float64(wd[off]) * w0[off:off + s]) / grad_scale).astype(np.float32)
        offsets.append(off)
        off += ps
    return OptInputs(tuple(sizes), tuple(l2), tuple(offsets), count, w0, tuple(grads), wd, grad_scale, lr)


@functools.lru_cache(maxsize=None)
def optimizer_case(name):
    if name == "small":
        return optimizer_inputs(11, SMALL_SIZES, SMALL_L2)
    if name == "large":
        return optimizer_inputs(12, LARGE_SIZES, LARGE_L2)
    raise KeyError(name)


def padding_mask(inp):
    out = np.ones(inp.count, bool)
    for off, s in zip(inp.offsets, inp.sizes):
        out[off:off + s] = False
    return out


STATE_NAMES = {"momentum": ("acc", None), "rmsprop": ("ms", "mom"), "adam": ("m", "v")}
OptStep = collections.namedtuple("OptStep", "w state1 state2 norm reg")


def optimizer_ref(inp, kind, clip=None):
    """One OptStep per gradient of `inp`, everything in float64: the weights and both state arrays after the update, the
    global norm of g' and the regulariser at the weights before it."""
    w = torch.from_numpy(inp.w0).double()
    wd = torch.from_numpy(inp.wd_elem).double()
    params, state, out = {"arena": w}, {}, []
    for step, g in enumerate(inp.grads, 1):
        gp = torch.from_numpy(g).double() * inp.grad_scale + wd * w
        norm = torch.sqrt((gp * gp).sum())
        reg = (0.5 * wd * w * w).sum()
        if clip is not None:
            gp = gp * (clip / max(norm.item(), clip))
        train_ref.apply_optimizer(kind, params, {"arena": gp}, state, inp.lr, step)
        s1, s2 = STATE_NAMES[kind]
        out.append(OptStep(w.numpy().copy(), state["arena"][s1].numpy().copy(),
                           state["arena"][s2].numpy().copy() if s2 else None, norm.item(), reg.item()))
    return out
