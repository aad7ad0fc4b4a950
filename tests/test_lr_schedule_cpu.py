"""Learning-rate schedules without a GPU: train.LRSchedule.value against the numpy restatement (tests/lr_schedule_ref.py), the
exact edges of the formula, the flags -> schedule function of the CLI and its refusals, and the argument checks of the C entry."""
import ctypes

import numpy as np
import pytest

import lr_schedule_ref as ref

BASE = 1e-2
T = 9
# (kwargs of train.LRSchedule == kwargs of lr_schedule_ref.lr_value, `base_lr` apart)
SCHEDULES = {
    "constant": dict(kind="constant", warmup_steps=3, total_steps=T),
    "step": dict(kind="step", warmup_steps=2, boundaries=(4, 7), total_steps=T),
    "cosine": dict(kind="cosine", warmup_steps=2, total_steps=T, final_factor=0.05),
}


def _schedule(name, **over):
    import train
    kw = dict(SCHEDULES[name], base_lr=BASE)
    kw.update(over)
    return train.LRSchedule(**kw)


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_value_matches_the_restatement_within_one_ulp(name):
    """Both sides compute in float64 and round once: they can differ only where a value straddles a rounding boundary."""
    sched = _schedule(name)
    for s in range(T + 4):
        got, want = sched.value(s), ref.lr_value(s, base=BASE, **SCHEDULES[name])
        assert isinstance(got, np.float32)
        assert ref.ulp_distance(got, want) <= 1, (name, s, got, want)


def test_edges_are_exact():
    f0 = 1.0 / 3.0
    for name in SCHEDULES:
        sched = _schedule(name)
        w = sched.warmup_steps
        assert sched.value(0) == np.float32(BASE * f0), name                     # s = 0: base * f0
        assert sched.value(w) == np.float32(BASE), name                          # s = W: base
    step = _schedule("step")
    assert step.value(3) == np.float32(BASE)
    assert step.value(4) == np.float32(BASE * 0.1)                               # the boundary step itself is already decayed
    assert step.value(6) == np.float32(BASE * 0.1)
    assert step.value(7) == np.float32(BASE * 0.1 ** 2) and step.value(T + 3) == np.float32(BASE * 0.1 ** 2)
    cos = _schedule("cosine")
    for s in (T, T + 1, T + 3):
        assert cos.value(s) == np.float32(BASE * 0.05), s                        # s >= T: base * ff
    assert cos.value(T - 1) > cos.value(T)
    assert _schedule("constant").value(T + 3) == np.float32(BASE)
    # no warm-up at all: the first update already runs at the base rate
    assert _schedule("constant", warmup_steps=0).value(0) == np.float32(BASE)


def test_schedule_is_hashable_and_checks_its_arguments():
    import train
    a, b = _schedule("step"), _schedule("step")
    assert a == b and hash(a) == hash(b) and len({a, b, _schedule("cosine")}) == 2
    assert a != _schedule("step", boundaries=(4, 8))
    for bad in (dict(kind="linear"), dict(kind="cosine"), dict(kind="cosine", total_steps=2, warmup_steps=2),
                dict(kind="step", boundaries=(4, 4)), dict(kind="step", boundaries=(5, 4)), dict(kind="step", boundaries=tuple(range(1, 10))),
                dict(kind="constant", boundaries=(3,)), dict(warmup_factor=1.5), dict(kind="cosine", total_steps=5, final_factor=-0.1),
                dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            train.LRSchedule(**bad)
    d = a.struct()
    assert (d.kind, d.n_boundaries, d.warmup_steps, d.total_steps) == (1, 2, 2, T) and list(d.boundaries)[:3] == [4, 7, 0]
    assert d.base_lr == BASE and d.decay_factor == 0.1 and d.warmup_factor == 1.0 / 3.0 and d.final_factor == 0.0


def _args(*argv):
    import train
    return train.build_parser().parse_args(list(argv))


def test_schedule_from_args_defaults():
    import train
    assert train.schedule_from_args(_args(), 100, 0) is None                     # no flag: no schedule object at all
    assert train.schedule_from_args(_args("--learning-rate", "0.1", "--epochs", "3"), 100, 0) is None
    s = train.schedule_from_args(_args("--lr-schedule", "cosine", "--epochs", "3"), 100, 40)
    assert s == train.LRSchedule("cosine", 1e-2, warmup_steps=0, warmup_factor=1.0 / 3.0, total_steps=340, final_factor=0.0)
    s = train.schedule_from_args(_args("--lr-warmup-steps", "50", "--learning-rate", "0.02"), 100, 0)    # warm-up alone: constant after it
    assert (s.kind, s.base_lr, s.warmup_steps, s.warmup_factor, s.total_steps) == ("constant", 0.02, 50, 1.0 / 3.0, 100)
    s = train.schedule_from_args(_args("--lr-schedule", "step", "--lr-decay-steps", "30", "60", "--lr-decay-factor", "0.5",
                                       "--lr-warmup-factor", "0.1", "--lr-warmup-steps", "5"), 100, 0)
    assert (s.kind, s.boundaries, s.decay_factor, s.warmup_factor, s.warmup_steps) == ("step", (30, 60), 0.5, 0.1, 5)
    s = train.schedule_from_args(_args("--lr-schedule", "cosine", "--lr-total-steps", "500", "--lr-final-factor", "0.01"), 100, 0)
    assert (s.total_steps, s.final_factor) == (500, 0.01)


BAD_FLAGS = [
    ("--lr-decay-steps", "30"),                                                  # decay steps without `step`
    ("--lr-schedule", "cosine", "--lr-decay-steps", "30"),
    ("--lr-schedule", "step"),                                                   # `step` without decay steps
    ("--lr-schedule", "cosine", "--lr-total-steps", "10", "--lr-warmup-steps", "10"),     # total at the warm-up
    ("--lr-schedule", "cosine", "--lr-total-steps", "5", "--lr-warmup-steps", "10"),      # ... and below it
    ("--lr-schedule", "step", "--lr-decay-steps") + tuple(str(10 * i) for i in range(1, 10)),   # 9 boundaries
]


@pytest.mark.parametrize("argv", BAD_FLAGS)
def test_senseless_flag_combinations_are_parser_errors(argv, capsys):
    import train
    with pytest.raises(ValueError):
        train.schedule_from_args(_args(*argv), 100, 0)
    with pytest.raises(SystemExit) as e:                                         # main(): parser.error, before any device is touched
        train.main(list(argv))
    assert e.value.code == 2 and "--lr-" in capsys.readouterr().err


def test_default_total_steps_at_or_below_the_warmup_is_refused():
    import train
    with pytest.raises(ValueError, match="warmup"):                              # the run ends at update 100: a 100-step warm-up never ends
        train.schedule_from_args(_args("--lr-warmup-steps", "100"), 100, 0)
    assert train.schedule_from_args(_args("--lr-warmup-steps", "100"), 100, 1) is not None


def test_c_entry_checks_its_arguments_before_any_launch():
    """rn_step_control_eval (LR) / rn_optimizer_update (NORM + LRDEV): a bad descriptor is RN_EINVAL with a message (no device here; 8
    stands for "some non-null pointer")."""
    import _rn
    from helpers import step_control
    L = _rn.lib()
    p = ctypes.c_void_p(8)

    def lr(step_dev=p, lr_dev=p, opt_kind=0, name="cosine", **over):
        d = _schedule(name).struct()
        for k, v in over.items():
            if k == "boundaries":
                for i, b in enumerate(v):
                    d.boundaries[i] = b
            else:
                setattr(d, k, v)
        return step_control(features=_rn.CTL_F_LR, optimizer_kind=opt_kind, schedule=d, step_dev=step_dev, lr_dev=lr_dev)

    def call(name="cosine", **over):
        return lr(name=name, **over)

    assert lr(step_dev=None) == -1 and b"step_control" in L.rn_last_error()
    assert lr(lr_dev=None) == -1
    assert lr(opt_kind=3) == -1                                                              # optimizer kind
    assert call(kind=3) == -1
    assert call(total_steps=2) == -1 and b"total_steps" in L.rn_last_error()                 # T == W
    assert call(total_steps=0) == -1
    assert call("constant", total_steps=3) == -1                                             # T == W with another kind
    assert call(warmup_factor=1.25) == -1 and call(final_factor=-0.5) == -1 and call(warmup_steps=-1) == -1
    assert call("step", n_boundaries=9) == -1 and call("step", n_boundaries=-1) == -1
    assert call("step", boundaries=(7, 7)) == -1 and b"increasing" in L.rn_last_error()
    assert call("step", boundaries=(7, 4)) == -1 and call("step", boundaries=(-1, 4)) == -1
    q = ctypes.c_void_p(4096)

    def norm_lrdev(kind, w, grad, state1, state2, wd, count, lr_dev, grad_scale, advance_counter, advance_by, partial, stream):
        u = _rn.OptUpdate(kind=kind, features=_rn.OPT_F_NORM | _rn.OPT_F_LRDEV, w=w, grad=grad, state1=state1, state2=state2,
                          wd_per_block=wd, count=count, grad_scale=grad_scale, advance_counter=advance_counter,
                          advance_by=advance_by, partial=partial, lr_dev=lr_dev)
        return L.rn_optimizer_update(ctypes.byref(u), stream)
    assert norm_lrdev(0, q, q, q, None, q, 1024, None, 1.0, None, 0, q, None) == -1
    assert b"device rate" in L.rn_last_error()
    assert norm_lrdev(0, q, q, q, None, q, 1024, q, 1.0, None, 0, None, None) == -1
    assert norm_lrdev(2, q, q, q, None, q, 1024, q, 1.0, None, 0, q, None) == -1    # adam needs state2
    assert norm_lrdev(0, q, q, q, None, q, 1000, q, 1.0, None, 0, q, None) == -1    # not whole blocks
