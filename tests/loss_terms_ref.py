"""The class loss as a weighted sum of terms (csrc/loss_terms.hip) in float64 torch with autograd, for the tests: the reference's
functions (losses.py:6-15, :37-73, :96-110, all with axis 0) written as it writes them -- every union formed the way its function
forms it, no closed-form gradient -- over the compacted trainable rows; the regression loss is oracle.losses_ref's.  Inputs are
step_tail_ref.loss_case's; the result is step_tail_ref.LossRef plus B1, B0 (per class: the cross entropy summed where the label
is 1 / is not 1).

`closed_form_f32` is the other side of the CPU test: the gradient formulas of the kernel's table evaluated in float32 numpy from
float32-rounded statistics -- what a float32 kernel can reach."""
import collections

import numpy as np
import torch

from oracle import losses_ref

TERM_NAMES = ("bce", "balanced_bce", "dice", "jaccard", "fixed_iou", "focal")
DEFAULT_SMOOTH = {"dice": 0.0, "jaccard": 1.0, "fixed_iou": 1e-7}          # the reference's call sites, losses.py:130, :133, :136

ALL_TERMS = "bce:0.7+balanced_bce:0.4+dice:0.5:0.3+jaccard:0.6:2+fixed_iou:0.3:0.01+focal:0.2"
ALL_BUT_FOCAL = ALL_TERMS.rsplit("+", 1)[0]
SINGLE_TERMS = ("bce", "balanced_bce", "dice:1:1", "jaccard", "fixed_iou")
PER_TERM_SPECS = SINGLE_TERMS + ("bce+jaccard", "balanced_bce+dice", "focal+dice:0.5")

LossTermsRef = collections.namedtuple("LossTermsRef", "cls reg M nfg I L P dz dr B1 B0")


def terms_of(spec):
    """[(name, weight, smooth or None)] of a well-formed spec (the tests' own reading of the grammar)."""
    out = []
    for token in spec.split("+"):
        f = token.split(":")
        out.append((f[0], float(f[1]) if len(f) > 1 else 1.0, float(f[2]) if len(f) > 2 else DEFAULT_SMOOTH.get(f[0])))
    return out


def has_focal(spec):
    return any(name == "focal" for name, _, _ in terms_of(spec))


def balanced_bce(labels, logits):
    """losses.py:96-110, axis 0."""
    num_positive = labels.sum(0)
    num_negative = (1 - labels).sum(0)
    weight_positive = num_negative / (num_positive + num_negative)
    weight_negative = num_positive / (num_positive + num_negative)
    ones = torch.ones_like(labels)
    weight = torch.where(labels == 1, ones * weight_positive, ones * weight_negative)
    return losses_ref.sigmoid_bce_with_logits(labels, logits) * weight


def jaccard(labels, logits, smooth):
    """losses.py:37-47, axis 0."""
    prob = torch.sigmoid(logits)
    intersection = (labels * prob).sum(0)
    union = labels.sum(0) + prob.sum(0)
    return (1 - (intersection + smooth) / (union - intersection + smooth)) * smooth


def fixed_iou(labels, logits, smooth):
    """losses.py:63-73, axis 0."""
    prob = torch.sigmoid(logits)
    intersection = (labels * prob).sum(0)
    union = labels.sum(0) + ((1 - labels) * prob).sum(0)
    return 1 - (intersection + smooth) / (union + smooth)


def class_loss(labels, logits, spec):
    """sum of weight * reduce_mean(term), as losses.py:139 sums its list; focal as :119-122."""
    total = 0.0
    for name, w, s in terms_of(spec):
        if name == "bce":
            t = losses_ref.sigmoid_bce_with_logits(labels, logits).mean()
        elif name == "balanced_bce":
            t = balanced_bce(labels, logits).mean()
        elif name == "dice":
            t = losses_ref.dice(labels, logits, smooth=s).mean()
        elif name == "jaccard":
            t = jaccard(labels, logits, s).mean()
        elif name == "fixed_iou":
            t = fixed_iou(labels, logits, s).mean()
        else:
            assert name == "focal", name
            num_fg = losses_ref.fg_mask_of(labels).to(logits.dtype).sum()
            t = losses_ref.focal_sigmoid(labels, logits).sum() / torch.clamp(num_fg, min=1.0)
        total = total + w * t
    return total


def loss_terms_ref(inp, spec, g_cls, g_reg, dtype=torch.float64):
    """Class loss of `spec` and the regression loss in `dtype` over the trainable rows, the gradient of g_cls * class loss +
    g_reg * regression loss (None: that loss takes no part) at full size with zeros on masked rows; statistics in float64."""
    m = torch.from_numpy(inp.mask)
    z = torch.from_numpy(inp.z).to(dtype).requires_grad_(True)
    rp = torch.from_numpy(inp.rp).to(dtype).requires_grad_(True)
    lab, rl = torch.from_numpy(inp.lab).to(dtype), torch.from_numpy(inp.rl).to(dtype)
    cl = class_loss(lab[m], z[m], spec)
    rg = losses_ref.regression_loss(rl[m], rp[m], losses_ref.fg_mask_of(lab[m]))
    total = 0.0
    if g_cls is not None:
        total = total + g_cls * cl
    if g_reg is not None:
        total = total + g_reg * rg
    total.backward()
    dz = z.grad.numpy() if z.grad is not None else np.zeros(inp.z.shape)
    dr = rp.grad.numpy() if rp.grad is not None else np.zeros(inp.rp.shape)
    l64, z64 = torch.from_numpy(inp.lab).double()[m], torch.from_numpy(inp.z).double()[m]
    p64 = torch.sigmoid(z64)
    bce = losses_ref.sigmoid_bce_with_logits(l64, z64)
    one = l64 == 1
    return LossTermsRef(cl.item(), rg.item(), int(m.sum()), int((l64.max(-1).values > 0.5).sum()) if l64.numel() else 0,
                        (l64 * p64).sum(0).numpy(), l64.sum(0).numpy(), p64.sum(0).numpy(), dz, dr,
                        torch.where(one, bce, torch.zeros_like(bce)).sum(0).numpy(),
                        torch.where(one, torch.zeros_like(bce), bce).sum(0).numpy())


def closed_form_f32(inp, spec, g_cls):
    """d(g_cls * class loss)/dz in float32 numpy: the per-element expressions of the kernel's table, the per-class sums taken in
    float64 and rounded to float32 once (what the finalize kernel stores), everything after that in float32."""
    f = np.float32
    m = inp.mask
    z, l = inp.z.astype(f), inp.lab.astype(f)
    p64 = 1.0 / (1.0 + np.exp(-inp.z[m].astype(np.float64)))
    l64 = inp.lab[m].astype(np.float64)
    M, C = f(m.sum()), f(inp.c)
    nfg = f((l64.max(-1) > 0.5).sum()) if l64.size else f(0)
    I, L, P = (l64 * p64).sum(0).astype(f), l64.sum(0).astype(f), p64.sum(0).astype(f)
    with np.errstate(over="ignore"):
        p = (f(1) / (f(1) + np.exp(-z))).astype(f)
    dp = p * (f(1) - p)
    g = np.zeros_like(z)
    gc = f(g_cls)
    for name, w, s in terms_of(spec):
        w = f(w)
        s = None if s is None else f(s)
        if name == "bce":
            g += gc * w * (p - l) / (M * C)
        elif name == "balanced_bce":
            g += gc * w * np.where(l == 1, (M - L) / M, L / M).astype(f) * (p - l) / (M * C)
        elif name == "dice":
            U = L + P + s
            g += -(gc * w / C) * dp * (f(2) * l * U - (f(2) * I + s)) / (U * U)
        elif name in ("jaccard", "fixed_iou"):
            D = L + P - I + s
            scale = w * s if name == "jaccard" else w
            g += -(gc * scale / C) * dp * (l * D - (I + s) * (f(1) - l)) / (D * D)
        else:
            pos = l == 1
            pt = np.where(pos, p, f(1) - p).astype(f)
            al = np.where(pos, f(0.25), f(0.75)).astype(f)
            om = f(1) - pt
            dfdpt = -al * (f(-2) * om * np.log(pt + f(1e-7)) + om * om / (pt + f(1e-7)))
            g += (gc * w / max(nfg, f(1))) * dfdpt * np.where(pos, f(1), f(-1)).astype(f) * dp
    assert g.dtype == f
    return np.where(m[:, None], g, f(0))
