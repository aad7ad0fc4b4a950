"""The guard against non-finite gradients (skip_nonfinite) in float64 / numpy, for the tests, written from its definition and not
from train.py:

    g'  = grad * grad_scale + wd * w            at the weights as they are when the gradient arrives
    n2  = sum g'^2 over the whole arena         in float64, then rounded to float32 ONCE: the float rn_norm_reg_finalize leaves
    the update is skipped  iff  float32(n2) is not finite

and a run over a list of gradients is clip_ref.clip_ref over the list with the skipped entries removed: weights, slots, average,
rates and Adam's bias correction all count APPLIED updates.  Counters after every step: (skipped in all, skipped in a row).

Inputs: the `small` arena of step_tail_ref (9 blocks: parameters of 1152, 700, 1, 1025 and 3000 elements) at its seed, drawn at
grad_scale = 0.75 and not at clip_ref.clip_case("small")'s 0.5.  The third poison below is one FINITE gradient element of 3e19
whose square must overflow a float: the criterion squares g' = grad * grad_scale + wd * w, and at grad_scale 0.5 that is 1.5e19,
whose square 2.25e38 is below FLT_MAX = 3.4e38 -- nothing would overflow and the guard would, rightly, apply the update.  At 0.75
g' = 2.25e19 and g'^2 = 5.06e38 overflows (test_guard_ref_cpu.py asserts both).  optimizer_inputs draws the gradients THROUGH g',
so the weights and every g' of the finite gradients are those of clip_case("small"), and its clip values bind / do not bind alike.

Poisoned gradients, each a copy of a finite one:
    nan        one NaN in the 1-element parameter
    inf        one +inf in the last element of the last parameter
    overflow   one finite 3e19 in the middle of the first parameter: every g' is finite, the SUM is not"""
import collections
import functools

import numpy as np

import clip_ref
import ema_ref                     # noqa: F401  (the settings clip_ref.clip_ref takes by name)
import lr_schedule_ref
import step_tail_ref

GRAD_SCALE = 0.75
POISONS = ("nan", "inf", "overflow")
OVERFLOW_VALUE = 3e19
CLIP_BINDS, CLIP_LOOSE, SCHEDULE = clip_ref.CLIP_BINDS, clip_ref.CLIP_LOOSE, clip_ref.SCHEDULE


@functools.lru_cache(maxsize=None)
def guard_case():
    """The small arena: step_tail_ref's sizes, l2 scales and seed, three finite gradients, grad_scale GRAD_SCALE."""
    return step_tail_ref.optimizer_inputs(11, step_tail_ref.SMALL_SIZES, step_tail_ref.SMALL_L2, grad_scale=GRAD_SCALE)


def poison_index(inp, which):
    if which == "nan":
        assert inp.sizes[2] == 1
        return inp.offsets[2]
    if which == "inf":
        return inp.offsets[-1] + inp.sizes[-1] - 1
    if which == "overflow":
        return inp.offsets[0] + inp.sizes[0] // 2
    raise KeyError(which)


def poisoned(inp, which, base=1):
    """A copy of the finite gradient inp.grads[base] with one element replaced."""
    g = np.array(inp.grads[base], np.float32, copy=True)
    g[poison_index(inp, which)] = {"nan": np.nan, "inf": np.inf, "overflow": OVERFLOW_VALUE}[which]
    return g


def norm_sq_float(inp, g, w, grad_scale=None):
    """float32(sum g'^2) at the weights `w`: what the device's norm pass leaves in norm_reg[0]."""
    case = inp if grad_scale is None else inp._replace(grad_scale=grad_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        n2, _ = clip_ref.norm_and_reg(case, g, w=w)
        return np.float32(n2)


def rates(inp, n):
    """The scheduled rate of each of the first n APPLIED updates (clip_ref.SCHEDULE), float64 rounded to float32 once."""
    return [float(lr_schedule_ref.lr_value(s, base=inp.lr, **SCHEDULE)) for s in range(n)]


GuardRun = collections.namedtuple("GuardRun", "run applied counters norm_sq")


def guard_ref(inp, grads, kind, clip=None, scheduled=False, setting=None):
    """GuardRun over the gradient list `grads`:
        run        clip_ref.ClipRun over the APPLIED gradients only (one OptStep per applied update; the average likewise)
        applied    per step: was its update applied?
        counters   per step: (skipped in all, skipped in a row) after it
        norm_sq    per step: float32(sum g'^2), the criterion's input"""
    kept, applied, counters, norms = [], [], [], []
    total = consecutive = 0
    w = inp.w0
    for g in grads:
        n2 = norm_sq_float(inp, g, w)
        ok = bool(np.isfinite(n2))
        norms.append(n2)
        applied.append(ok)
        if ok:
            kept.append(np.asarray(g, np.float32))
            consecutive = 0
            w = clip_ref.optimizer_steps(inp._replace(grads=tuple(kept)), kind, clip, rates(inp, len(kept)) if scheduled else None)[-1].w
        else:
            total, consecutive = total + 1, consecutive + 1
        counters.append((total, consecutive))
    case = inp._replace(grads=tuple(kept))
    run = clip_ref.clip_ref(case, kind, clip, rates(inp, len(kept)) if scheduled else None, setting) if kept else clip_ref.ClipRun([], None)
    return GuardRun(run, tuple(applied), tuple(counters), tuple(norms))
