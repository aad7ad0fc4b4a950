"""An exponential moving average of the weights in float64, for the tests, written from its definition
(tf.train.ExponentialMovingAverage) and not from train.py.  With n the number of updates applied before this one and w' the
weight after this update:

    d(n) = min(D, (1 + n) / (10 + n))     with warm-up
         = D                              without
    e   <- e - (e - w') * (1 - d(n))      per element;  e starts as the initial weights (zero on the arena's padding)

The weights come from step_tail_ref.optimizer_ref on inputs drawn with lr = 0.1: an update moves a weight by about 0.1, so an
average that lags, leads or misses an update differs from the true one by far more than the tests' 1e-4.

SETTINGS: `warm` (D = 0.9999 with warm-up: the decays are 1/10, 2/11, 3/12, D never binds) and `plain` (D = 0.5 without warm-up).
`capped` (D = 0.22 with warm-up: 1/10, 2/11, then the cap, 0.22 < 3/12) stands beside them because d(n) of `plain` does not
depend on n at all: counting n wrongly cannot show there, and does under `capped`, where both branches of the min are taken.

`mistake` plants one of three errors for the sensitivity check of test_ema_ref_cpu.py: "pre_update" averages the weight before
the update, "n_off_by_one" uses d(n + 1), "dropped" leaves e alone at the second update."""
import collections
import functools

import numpy as np

import step_tail_ref

LR = 0.1
Setting = collections.namedtuple("Setting", "decay warmup")
SETTINGS = collections.OrderedDict([("warm", Setting(0.9999, True)), ("plain", Setting(0.5, False)),
                                    ("capped", Setting(0.22, True))])
MISTAKES = ("pre_update", "n_off_by_one", "dropped")
SEEDS = {"small": (11, step_tail_ref.SMALL_SIZES, step_tail_ref.SMALL_L2),
         "large": (12, step_tail_ref.LARGE_SIZES, step_tail_ref.LARGE_L2)}


def decay_value(n, decay, warmup):
    """d(n) in float64."""
    n = np.float64(n)
    if warmup:
        return np.minimum(np.float64(decay), (np.float64(1) + n) / (np.float64(10) + n))
    return np.float64(decay)


def decay_pair(n, decay, warmup):
    """[d(n), 1 - d(n)], each formed in float64 and rounded to float32 once."""
    d = decay_value(n, decay, warmup)
    return np.float32(d), np.float32(np.float64(1) - d)


@functools.lru_cache(maxsize=None)
def ema_case(name):
    seed, sizes, l2 = SEEDS[name]
    return step_tail_ref.optimizer_inputs(seed, sizes, l2, lr=LR)


def ema_steps(w0, ws, decay, warmup, mistake=None, dtype=np.float64, first_update=0):
    """One e per entry of `ws` (the weights after each update), starting from e = w0, in `dtype`."""
    e = np.asarray(w0).astype(dtype)
    prev = e.copy()
    out = []
    for i, w in enumerate(ws):
        n = first_update + i + (1 if mistake == "n_off_by_one" else 0)
        om = dtype(np.float64(1) - decay_value(n, decay, warmup))
        w = np.asarray(w).astype(dtype)
        seen = prev if mistake == "pre_update" else w
        if not (mistake == "dropped" and i == 1):
            e = e - (e - seen) * om
        prev = w
        out.append(e.copy())
    return out


EmaRun = collections.namedtuple("EmaRun", "steps e")


def ema_ref(inp, kind, setting, clip=None, mistake=None):
    """EmaRun(steps, e): step_tail_ref.optimizer_ref's OptStep per gradient of `inp` and the average after each of them."""
    s = SETTINGS[setting] if isinstance(setting, str) else setting
    steps = step_tail_ref.optimizer_ref(inp, kind, clip)
    return EmaRun(steps, ema_steps(inp.w0, [st.w for st in steps], s.decay, s.warmup, mistake))
