"""Learning-rate schedules restated in numpy from their definition (not from train.py), for the tests.

With s the number of updates already applied, W warm-up steps, f0 the warm-up factor, T the total steps, ff the final factor:

    s <  W               lr = base * (f0 + (1 - f0) * s / W)
    s >= W   constant    lr = base
             step        lr = base * decay ** (number of boundaries b with b <= s)
             cosine      lr = base * (ff + (1 - ff) * 0.5 * (1 + cos(pi * min(1, (s - W) / (T - W)))))

everything in float64, rounded to float32 once.  Adam multiplies its update by lr * sqrt(1 - 0.999^t) / (1 - 0.9^t), t = s + 1."""
import numpy as np


def lr_value(s, kind, base, warmup_steps=0, warmup_factor=1.0 / 3.0, boundaries=(), decay_factor=0.1, total_steps=None,
             final_factor=0.0):
    s = np.float64(s)
    base, f0, ff = np.float64(base), np.float64(warmup_factor), np.float64(final_factor)
    if s < warmup_steps:
        return np.float32(base * (f0 + (np.float64(1) - f0) * s / np.float64(warmup_steps)))
    if kind == "constant":
        return np.float32(base)
    if kind == "step":
        passed = int(np.count_nonzero(np.asarray(boundaries, dtype=np.int64) <= int(s)))
        return np.float32(base * np.power(np.float64(decay_factor), passed))
    if kind == "cosine":
        progress = np.minimum(np.float64(1), (s - warmup_steps) / np.float64(total_steps - warmup_steps))
        return np.float32(base * (ff + (np.float64(1) - ff) * np.float64(0.5) * (np.float64(1) + np.cos(np.pi * progress))))
    raise ValueError(kind)


def adam_rate(lr, s):
    """The scalar Adam's update is multiplied by at update s (0-based): float32 `lr` with the bias correction of t = s + 1, in float64."""
    t = np.float64(s + 1)
    return np.float32(np.float64(np.float32(lr)) * np.sqrt(np.float64(1) - np.power(np.float64(0.999), t))
                      / (np.float64(1) - np.power(np.float64(0.9), t)))


def ulp_distance(a, b):
    """Units in the last place between two finite float32 values of one sign."""
    ia = int(np.asarray(a, dtype=np.float32).view(np.int32))
    ib = int(np.asarray(b, dtype=np.float32).view(np.int32))
    return abs(ia - ib)
