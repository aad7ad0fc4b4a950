"""Gradient accumulation in float64, for the tests, written from its definition and not from train.py.  A = accumulate_steps; the
gradients of `inp` are MICRO-step gradients; an update is applied after every A-th one, from the mean of the last A:

    acc(m) = sum of grad_k * grad_scale over the micro-steps k of the current cycle up to m      (the running sum)
    G      = mean of the cycle's A gradients                                                     (float64)
    g'     = G * grad_scale + wd * w,  then the optimizer update, the global norm, the regulariser and the moving average exactly
             as step_tail_ref.optimizer_ref / ema_ref.ema_steps form them from one gradient

The last micro-step of a cycle does not store its sum (the update consumes it), so acc(m) there is acc(m - 1); a trailing partial
cycle is summed and not applied.  `rates`: one learning rate per update (a schedule) in the place of inp.lr.

Inputs: step_tail_ref.optimizer_inputs with steps = A * U + r and ema_ref's lr = 0.1, so that a missed, doubled or unaveraged
update moves a weight by far more than the tests' 1e-4.  `exact_case`: no L2, grad_scale 1, gradients k / 64 with |k| <= 65536:
every sum of up to 4 of them and the division by 2 or 4 are exact in float32, so an accumulating kernel must reproduce a plain
update on the exact means bit for bit."""
import collections
import functools

import numpy as np
import torch

import ema_ref
import step_tail_ref
from oracle import train_ref

LR = ema_ref.LR
UPDATES, REST = 2, 1            # 2A + 1 micro-steps: two full cycles and the first micro-step of a third
SEEDS = {"small": (21, step_tail_ref.SMALL_SIZES, step_tail_ref.SMALL_L2),
         "large": (22, step_tail_ref.LARGE_SIZES, step_tail_ref.LARGE_L2)}

AccumRun = collections.namedtuple("AccumRun", "acc steps e means")


@functools.lru_cache(maxsize=None)
def accum_case(name, A, updates=UPDATES, rest=REST):
    seed, sizes, l2 = SEEDS[name]
    return step_tail_ref.optimizer_inputs(seed, sizes, l2, steps=A * updates + rest, lr=LR)


@functools.lru_cache(maxsize=None)
def exact_case(A, updates=UPDATES):
    """The small arena without L2, grad_scale 1, gradients k / 64 in [-1024, 1024] (see the module docstring)."""
    sizes = step_tail_ref.SMALL_SIZES
    inp = step_tail_ref.optimizer_inputs(23, sizes, (None,) * len(sizes), steps=A * updates, grad_scale=1.0, lr=LR)
    rng = np.random.default_rng(24)
    grads = []
    for _ in range(A * updates):
        g = np.zeros(inp.count, np.float32)
        for off, s in zip(inp.offsets, inp.sizes):
            g[off:off + s] = (rng.integers(-65536, 65537, s) / 64.0).astype(np.float32)
        grads.append(g)
    return inp._replace(grads=tuple(grads))


def cycle_means(inp, A, dtype=np.float64):
    """The mean of every full block of A gradients of `inp`, in `dtype`."""
    n = len(inp.grads) // A
    return [np.mean(np.stack([np.asarray(g).astype(dtype) for g in inp.grads[u * A:(u + 1) * A]]), axis=0) for u in range(n)]


def running_sums(inp, A):
    """acc(m) for every micro-step m, float64."""
    out, acc = [], np.zeros(inp.count, np.float64)
    for m, g in enumerate(inp.grads):
        p = m % A
        if p == A - 1:
            out.append(acc.copy())                 # the applying micro-step leaves the sum as it was
            continue
        acc = (acc if p else 0.0) + np.asarray(g).astype(np.float64) * np.float64(inp.grad_scale)
        out.append(acc.copy())
    return out


def optimizer_steps(inp, kind, rates=None):
    """step_tail_ref.optimizer_ref (no clipping) with an optional learning rate per update."""
    if rates is None:
        return step_tail_ref.optimizer_ref(inp, kind)
    w = torch.from_numpy(inp.w0).double()
    wd = torch.from_numpy(inp.wd_elem).double()
    params, state, out = {"arena": w}, {}, []
    for step, (g, lr) in enumerate(zip(inp.grads, rates), 1):
        gp = torch.from_numpy(np.asarray(g)).double() * inp.grad_scale + wd * w
        norm = torch.sqrt((gp * gp).sum())
        reg = (0.5 * wd * w * w).sum()
        train_ref.apply_optimizer(kind, params, {"arena": gp}, state, float(lr), step)
        s1, s2 = step_tail_ref.STATE_NAMES[kind]
        out.append(step_tail_ref.OptStep(w.numpy().copy(), state["arena"][s1].numpy().copy(),
                                         state["arena"][s2].numpy().copy() if s2 else None, norm.item(), reg.item()))
    return out


def accum_ref(inp, kind, A, setting=None, rates=None):
    """AccumRun(acc per micro-step, OptStep per UPDATE, the moving average per update or None, the cycle means)."""
    means = cycle_means(inp, A)
    steps = optimizer_steps(inp._replace(grads=tuple(means)), kind, rates)
    e = None
    if setting is not None:
        s = ema_ref.SETTINGS[setting] if isinstance(setting, str) else setting
        e = ema_ref.ema_steps(inp.w0, [st.w for st in steps], s.decay, s.warmup)
    return AccumRun(running_sums(inp, A), steps, e, means)
