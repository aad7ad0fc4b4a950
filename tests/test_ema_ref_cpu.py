"""The float64 reference of the weights' moving average (ema_ref.py) checked on the CPU: d(n) against hand values, the padding,
a float32 restatement, the reference's sensitivity to three planted mistakes, and the --ema-* flag errors.  No GPU."""
import numpy as np
import pytest

import ema_ref as ref
import step_tail_ref
from helpers import assert_close

TOL = 1e-4
KINDS = ("momentum", "rmsprop", "adam")


def test_decay_values_by_hand():
    # with warm-up: (1 + n) / (10 + n) until D binds
    assert ref.decay_value(0, 0.9999, True) == 0.1
    assert ref.decay_value(1, 0.9999, True) == 2.0 / 11.0
    assert ref.decay_value(8, 0.9999, True) == 0.5
    assert ref.decay_value(10 ** 6, 0.9999, True) == 0.9999          # (1e6 + 1) / (1e6 + 10) = 0.999991 > D
    assert ref.decay_value(10 ** 6, 0.999995, True) == (10 ** 6 + 1.0) / (10 ** 6 + 10.0)
    assert ref.decay_value(2, 0.22, True) == 0.22 and ref.decay_value(1, 0.22, True) == 2.0 / 11.0
    for n in (0, 1, 8, 10 ** 6):
        assert ref.decay_value(n, 0.5, False) == 0.5
    d, om = ref.decay_pair(1, 0.9999, True)
    assert d == np.float32(2.0 / 11.0) and om == np.float32(9.0 / 11.0) and d.dtype == om.dtype == np.float32
    # 1 - d is rounded from float64, not formed from the rounded d: for D = 0.9999 the two differ
    d, om = ref.decay_pair(10 ** 6, 0.9999, True)
    assert om == np.float32(1.0 - 0.9999) and om != np.float32(1.0) - d


@pytest.mark.parametrize("setting", list(ref.SETTINGS))
def test_first_average_by_hand(setting):
    """e1 = d(0) w0 + (1 - d(0)) w1, then e2 from e1: the recurrence written out."""
    s = ref.SETTINGS[setting]
    w0, w1, w2 = np.array([1.0, -2.0]), np.array([0.5, -1.0]), np.array([0.25, 4.0])
    e = ref.ema_steps(w0, [w1, w2], s.decay, s.warmup)
    d0, d1 = (0.1, 2.0 / 11.0) if s.warmup else (s.decay, s.decay)
    np.testing.assert_allclose(e[0], d0 * w0 + (1 - d0) * w1, rtol=1e-14)
    np.testing.assert_allclose(e[1], d1 * e[0] + (1 - d1) * w2, rtol=1e-14)


@pytest.mark.parametrize("setting", list(ref.SETTINGS))
@pytest.mark.parametrize("kind", KINDS)
def test_padding_stays_zero_and_float32_agrees(kind, setting):
    inp = ref.ema_case("small")
    assert inp.lr == ref.LR and inp.count == 9 * step_tail_ref.OPT_BLOCK
    run = ref.ema_ref(inp, kind, setting)
    pad = step_tail_ref.padding_mask(inp)
    assert len(run.e) == len(inp.grads) == 3
    s = ref.SETTINGS[setting]
    e32 = ref.ema_steps(inp.w0, [st.w.astype(np.float32) for st in run.steps], s.decay, s.warmup, dtype=np.float32)
    for step, (e, f) in enumerate(zip(run.e, e32), 1):
        assert not e[pad].any() and not f[pad].any()
        assert f.dtype == np.float32
        assert_close(f, e, TOL, "float32 average, %s %s step %d" % (kind, setting, step), elementwise_tol=TOL)
    # the weights move enough for the average to lag visibly behind them
    assert np.median(np.abs(run.e[2] - run.steps[2].w)[~pad]) > 1e-3


def _differs(a, b):
    """Element-wise relative difference with helpers.elementwise_rel_err's floor, per element."""
    floor = 1e-3 * np.abs(b).max()
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


@pytest.mark.parametrize("mistake", ref.MISTAKES)
@pytest.mark.parametrize("setting", list(ref.SETTINGS))
@pytest.mark.parametrize("kind", KINDS)
def test_reference_tells_planted_mistakes_apart(kind, setting, mistake):
    """Averaging the pre-update weight, n off by one, a dropped update at step 2: each must move more than half of the
    non-padding elements of e at step 3 by more than TOL.  `plain` has d(n) = D whatever n is, so a wrong n is no mistake there
    -- that is asserted as such -- and `capped` is the setting that shows it with D binding."""
    inp = ref.ema_case("small")
    true = ref.ema_ref(inp, kind, setting).e[2]
    bad = ref.ema_ref(inp, kind, setting, mistake=mistake).e[2]
    keep = ~step_tail_ref.padding_mask(inp)
    frac = float((_differs(bad, true)[keep] > TOL).mean())
    print("%s %s %s: %.3f of the elements differ by more than %.0e" % (kind, setting, mistake, frac, TOL))
    if setting == "plain" and mistake == "n_off_by_one":
        assert np.array_equal(bad, true)
        return
    assert frac > 0.5, (kind, setting, mistake, frac)


def _args(*argv):
    import train
    return train.build_parser().parse_args(list(argv))


BAD_FLAGS = [("--ema-no-warmup",), ("--ema-decay", "0"), ("--ema-decay", "1"), ("--ema-decay", "-0.5"), ("--ema-decay", "1.5"),
             ("--ema-decay", "nan")]


@pytest.mark.parametrize("argv", BAD_FLAGS)
def test_senseless_ema_flags_are_parser_errors(argv, capsys):
    import train
    assert train.ema_flag_error(_args(*argv))
    with pytest.raises(SystemExit) as e:                                         # main(): parser.error, before any device is touched
        train.main(list(argv))
    assert e.value.code == 2 and "--ema-" in capsys.readouterr().err


def test_sensible_ema_flags():
    import train
    a = _args()
    assert a.ema_decay is None and a.ema_no_warmup is False and train.ema_flag_error(a) is None
    a = _args("--ema-decay", "0.9998", "--ema-no-warmup")
    assert a.ema_decay == 0.9998 and a.ema_no_warmup is True and train.ema_flag_error(a) is None


def test_optimizer_refuses_a_decay_outside_the_open_interval():
    import torch
    import train
    mod = torch.nn.Module()
    mod.p = torch.nn.Parameter(torch.zeros(3))
    arena = train.ParamArena(mod, torch.device("cpu"))
    for bad in (0.0, 1.0, -1.0, 2.0):
        with pytest.raises(ValueError):
            train.Optimizer(arena, "momentum", 0.1, ema_decay=bad)
    opt = train.Optimizer(arena, "momentum", 0.1)
    assert opt.ema is None and opt.ema_dev is None and opt.ema_updates_dev is None
    with pytest.raises(ValueError):
        opt.ema_decay_value(0)
