"""The box regression loss as a weighted sum of Huber / IoU / GIoU terms (csrc/regr_terms.hip) in torch, parameterised by dtype,
with autograd for the gradients, and the case table of its tests.

Prediction p and label l of a row are anchor-relative (ty, tx, th, tw); in anchor units

    box(t) = (ty - e^th/2, tx - e^tw/2, ty + e^th/2, tx + e^tw/2),  area(t) = e^th e^tw
    iy = max(0, min(P2, L2) - max(P0, L0)), ix likewise, I = iy ix, U = area(p) + area(l) - I, IoU = I/U
    cy = max(P2, L2) - min(P0, L0),         cx likewise, E = cy cx, GIoU = IoU - (E - U)/E

Every max / min is a torch.where on the predicate of the kernel's subgradient convention: max(P, L) is P where P >= L,
min(P, L) is P where P <= L, max(0, d) is d where d > 0.  A row is foreground (fg) when it is trainable and its largest class
label is > 0.5.  huber multiplies by the fg weight on every trainable row (a NaN there reaches the loss); the overlap terms
select the fg rows."""
import collections
import functools

import numpy as np
import torch

TERM_NAMES = ("huber", "iou", "giou")
SPECS = ("giou", "iou", "huber:2", "huber:1:0.11", "huber:0.5+iou:0.7+giou:2")
G_REG = 1.7

# the forward kernel takes FWD_BLOCKS x RPB = 2048 x 64 rows per pass, the backward BWD_BLOCKS x T = 512 x 256: both grid-stride past
WRAP_ROWS = 2048 * 64
assert WRAP_ROWS == 512 * 256

Inputs = collections.namedtuple("Inputs", "c rows lab rp rl mask planted")
RegrRef = collections.namedtuple("RegrRef", "loss nfg s_huber s_iou_l s_giou_l s_iou fg_rows dr")
Case = collections.namedtuple("Case", "name rows c seed recipe")


def terms_of(spec):
    """[(name, weight, delta or None)] of a well-formed spec (the tests' own reading of the grammar)."""
    out = []
    for token in spec.split("+"):
        f = token.split(":")
        out.append((f[0], float(f[1]) if len(f) > 1 else 1.0, (float(f[2]) if len(f) > 2 else 1.0) if f[0] == "huber" else None))
    return out


def has(spec, name):
    return any(n == name for n, _, _ in terms_of(spec))


# ------------------------------------------------------------------------------------------------------------- the formulas
def huber(err, delta):
    """tf.losses.huber_loss: 0.5 q^2 + delta (|e| - q), q = min(|e|, delta)."""
    a = err.abs()
    q = torch.clamp(a, max=delta)
    return 0.5 * q * q + delta * (a - q)


def corners(t):
    h, w = torch.exp(t[:, 2]), torch.exp(t[:, 3])
    return t[:, 0] - h / 2, t[:, 1] - w / 2, t[:, 0] + h / 2, t[:, 1] + w / 2, h * w


def _axis(plo, phi, llo, lhi):
    d = torch.where(phi <= lhi, phi, lhi) - torch.where(plo >= llo, plo, llo)
    i = torch.where(d > 0, d, torch.zeros_like(d))
    c = torch.where(phi >= lhi, phi, lhi) - torch.where(plo <= llo, plo, llo)
    return i, c


def iou_giou(p, l):
    """(IoU, GIoU) of the rows of p and l, [n, 4] each, in anchor units."""
    p0, p1, p2, p3, ap = corners(p)
    l0, l1, l2, l3, al = corners(l)
    iy, cy = _axis(p0, p2, l0, l2)
    ix, cx = _axis(p1, p3, l1, l3)
    inter = iy * ix
    union = ap + al - inter
    iou = inter / union
    enc = cy * cx
    return iou, iou - (enc - union) / enc


def regr_terms_ref(inp, spec, g_reg=G_REG, dtype=torch.float64):
    """Loss of `spec`, the sums of the statistics, fg_rows, and d(g_reg * loss)/d(reg_pred) at full size, in `dtype`."""
    m = torch.tensor(inp.mask)
    rp = torch.tensor(inp.rp).to(dtype).requires_grad_(True)
    rl = torch.tensor(inp.rl).to(dtype)
    lab = torch.tensor(inp.lab)
    fg = m & (lab.max(-1).values > 0.5) if lab.shape[0] else m
    nfg = int(fg.sum())
    zero = torch.zeros((), dtype=dtype)
    s_huber = {}
    for name, _, delta in terms_of(spec):
        if name == "huber":
            s_huber = {delta: (huber(rl[m] - rp[m], delta) * fg[m].to(dtype).unsqueeze(-1)).sum()}
    overlap = has(spec, "iou") or has(spec, "giou")
    if overlap and nfg:
        iou, giou = iou_giou(rp[fg], rl[fg])
        s_iou, s_iou_l, s_giou_l = iou.sum(), (1 - iou).sum(), (1 - giou).sum()
    else:
        s_iou = s_iou_l = s_giou_l = zero
    loss = zero
    if nfg:
        for name, w, delta in terms_of(spec):
            loss = loss + w * {"huber": lambda: s_huber[delta] / (4 * nfg), "iou": lambda: s_iou_l / nfg, "giou": lambda: s_giou_l / nfg}[name]()
    if loss.requires_grad:
        (g_reg * loss).backward()
    dr = rp.grad.numpy() if rp.grad is not None else np.zeros(inp.rp.shape)
    val = lambda t: float(t.detach()) if torch.is_tensor(t) else float(t)
    return RegrRef(val(loss), nfg, val(next(iter(s_huber.values()))) if s_huber else 0.0, val(s_iou_l), val(s_giou_l), val(s_iou),
                   fg.numpy().astype(np.uint8), dr)


# ---------------------------------------------------------------------------------------------------------------- the cases
# planted geometry, (p, l) pairs in (ty, tx, th, tw)
PLANTED = collections.OrderedDict([
    ("disjoint", ((0.0, 0.0, 0.0, 0.0), (3.0, 0.25, 0.0, 0.0))),                 # apart in y, overlapping in x
    ("disjoint_both", ((-2.0, -2.0, 0.1, -0.2), (1.5, 2.0, 0.3, 0.2))),
    ("inside", ((0.05, -0.03, -1.0, -0.9), (0.0, 0.0, 0.2, 0.3))),               # the prediction inside the label
    ("around", ((0.0, 0.0, 0.2, 0.3), (0.05, -0.03, -1.0, -0.9))),               # the label inside the prediction
    ("identical", ((0.3, -0.2, 0.2, -0.4), (0.3, -0.2, 0.2, -0.4))),             # ties in every predicate
    ("touching", ((0.0, 0.0, 0.0, 0.0), (1.0, 0.25, 0.0, 0.0))),                 # P2 == L0 == 0.5: iy == 0 exactly
    ("th_plus_10", ((0.1, 0.1, 10.0, 0.0), (0.0, 0.0, 9.5, 0.2))),
    ("th_minus_10", ((0.00001, 0.0, -10.0, -10.0), (0.0, 0.00001, -10.0, -9.8))),
])

_SMALL = [Case("r%d-c%d" % (r, c), (r,), c, 100 + 7 * r + c, "default") for r in (1, 63, 64, 65, 257) for c in (1, 3, 20, 80)]
_LEVELS = tuple(9 * hw for hw in (13 * 11, 7 * 6, 4 * 3, 2 * 2, 1 * 1))
CASE_LIST = _SMALL + [
    Case("levels-c20", _LEVELS, 20, 1, "default"), Case("levels-c3", _LEVELS, 3, 2, "default"),
    Case("r4608-c80", (4608,), 80, 3, "default"),
    Case("wrap-c20", (WRAP_ROWS + 65,), 20, 4, "default"), Case("wrap-c1", (WRAP_ROWS - 300, 365), 1, 5, "default"),
    Case("near-c20", (257,), 20, 6, "near"), Case("near-c3", (130, 127), 3, 7, "near"),
    Case("planted-c20", (65,), 20, 8, "planted"), Case("planted-c3", (30, 35), 3, 9, "planted"),
    Case("no_fg-c20", (65,), 20, 10, "no_fg"), Case("all_fg-c20", (65,), 20, 11, "all_fg"), Case("all_fg-c3", (64,), 3, 12, "all_fg"),
    Case("no_trainable-c20", (65,), 20, 13, "no_trainable"), Case("identical-c20", (65,), 20, 14, "identical"),
]
CASES = collections.OrderedDict((c.name, c) for c in CASE_LIST)
assert len(CASES) == len(CASE_LIST)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case (float32 arrays, read-only: shared between the tests)."""
    k = CASES[name]
    rng = np.random.default_rng(k.seed)
    n, c = sum(k.rows), k.c
    f = np.float32
    rl = np.concatenate([rng.normal(0, 0.5, (n, 2)), rng.normal(0, 0.4, (n, 2))], 1).astype(f)
    noise = rng.normal(0, 1.0, (n, 4))
    rp = (rl + (1e-3 if k.recipe == "near" else 0.4) * noise).astype(f)
    is_fg = rng.random(n) < 0.1
    mask = rng.random(n) < 0.8
    if k.recipe in ("default", "near", "planted"):
        is_fg[0] = mask[0] = True                       # at least one fg row, also with one row in all
        if n >= 8:                                      # and some fg-labelled rows are not trainable, on purpose
            is_fg[n - 2], mask[n - 2] = True, False
    planted = {}
    if k.recipe == "planted":
        for i, (key, (p, l)) in enumerate(PLANTED.items()):
            row = 2 * i + 1
            rp[row], rl[row] = p, l
            is_fg[row] = mask[row] = True
            planted[key] = row
    elif k.recipe == "no_fg":
        is_fg[:] = False
    elif k.recipe == "all_fg":
        is_fg[:] = mask[:] = True
    elif k.recipe == "no_trainable":
        mask[:] = False
    elif k.recipe == "identical":
        is_fg[:] = mask[:] = True
        rp = rl.copy()
    lab = np.zeros((n, c), f)
    lab[is_fg, rng.integers(0, c, int(is_fg.sum()))] = 1.0
    for a in (lab, rp, rl, mask):
        a.setflags(write=False)
    return Inputs(c, k.rows, lab, rp, rl, mask, planted)


def segments(inp):
    """[(lab, rp, rl, mask)] per segment."""
    out, start = [], 0
    for r in inp.rows:
        out.append((inp.lab[start:start + r], inp.rp[start:start + r], inp.rl[start:start + r], inp.mask[start:start + r]))
        start += r
    return out


@functools.lru_cache(maxsize=None)
def ref(name, spec, g_reg=G_REG, dtype=torch.float64):
    return regr_terms_ref(case(name), spec, g_reg, dtype)
