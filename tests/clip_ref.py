"""The clipped optimizer update in float64, for the tests, written from its definition and not from train.py:

    g'   = grad * grad_scale + wd * w            (the regulariser's gradient takes part in the norm, as compute_gradients(loss) has it)
    norm = sqrt(sum g'^2),   reg = sum 0.5 * wd * w^2          (both at the weights BEFORE the update)
    g'  *= clip / max(norm, clip)                (tf.clip_by_global_norm; clip=None: no clipping)

then oracle.train_ref.apply_optimizer -- step_tail_ref.optimizer_ref's arithmetic with an optional learning rate per update (a
schedule) in the place of inp.lr, as accum_ref.optimizer_steps has it -- and ema_ref.ema_steps for the moving average.

Inputs: the small and large arenas of step_tail_ref at its seeds (11 / 12).  On them |g'| = 0.25 + |N(0, 1)| per real element, so the
norm is about 100 (small: 5878 elements) and about 1900 (large): CLIP_BINDS = 0.5 binds at every update, CLIP_LOOSE = 1e6 at none."""
import collections
import functools

import numpy as np
import torch

import ema_ref
import lr_schedule_ref
import step_tail_ref
from oracle import train_ref

CLIP_BINDS, CLIP_LOOSE = step_tail_ref.CLIP_BINDS, step_tail_ref.CLIP_LOOSE
UPDATES = 3
# the warm-up + drop schedule of test_gpu_lr_schedule.test_scheduled_optimizer_matches_tf_semantics: the rates of updates 0, 1, 2
# are base / 3, base * 2 / 3 and base
SCHEDULE = dict(kind="step", warmup_steps=2, boundaries=(3,))


@functools.lru_cache(maxsize=None)
def clip_case(name):
    """step_tail_ref.optimizer_case(name) (same seed, same sizes), three updates."""
    return step_tail_ref.optimizer_case(name)


def rates(inp, n=UPDATES):
    """The scheduled rate of each of the first n updates, float64 rounded to float32 once."""
    return [float(lr_schedule_ref.lr_value(s, base=inp.lr, **SCHEDULE)) for s in range(n)]


def clip_scale(norm, clip):
    return 1.0 if clip is None else clip / max(norm, clip)


def optimizer_steps(inp, kind, clip=None, rates=None):
    """One step_tail_ref.OptStep per gradient of `inp`, everything in float64; `rates`: one learning rate per update."""
    w = torch.from_numpy(inp.w0).double()
    wd = torch.from_numpy(inp.wd_elem).double()
    params, state, out = {"arena": w}, {}, []
    for step, g in enumerate(inp.grads, 1):
        gp = torch.from_numpy(np.asarray(g)).double() * inp.grad_scale + wd * w
        norm = torch.sqrt((gp * gp).sum())
        reg = (0.5 * wd * w * w).sum()
        if clip is not None:
            gp = gp * (clip / max(norm.item(), clip))
        lr = inp.lr if rates is None else float(rates[step - 1])
        train_ref.apply_optimizer(kind, params, {"arena": gp}, state, lr, step)
        s1, s2 = step_tail_ref.STATE_NAMES[kind]
        out.append(step_tail_ref.OptStep(w.numpy().copy(), state["arena"][s1].numpy().copy(),
                                         state["arena"][s2].numpy().copy() if s2 else None, norm.item(), reg.item()))
    return out


ClipRun = collections.namedtuple("ClipRun", "steps e")


def clip_ref(inp, kind, clip=None, rates=None, setting=None):
    """ClipRun(OptStep per update, the moving average after each update or None)."""
    steps = optimizer_steps(inp, kind, clip, rates)
    e = None
    if setting is not None:
        s = ema_ref.SETTINGS[setting] if isinstance(setting, str) else setting
        e = ema_ref.ema_steps(inp.w0, [st.w for st in steps], s.decay, s.warmup)
    return ClipRun(steps, e)


def norm_and_reg(inp, g, w=None, lo=0, hi=None):
    """(sum g'^2, reg) of the elements [lo, hi) in float64, at the weights `w` (default: the initial ones)."""
    hi = inp.count if hi is None else hi
    w = np.asarray(inp.w0 if w is None else w, np.float64)[lo:hi]
    wd = inp.wd_elem.astype(np.float64)[lo:hi]
    gp = np.asarray(g, np.float64)[lo:hi] * np.float64(inp.grad_scale) + wd * w
    return float((gp * gp).sum()), float((0.5 * wd * w * w).sum())
