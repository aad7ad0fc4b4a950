"""Gradient accumulation without a GPU: the float64 reference (accum_ref.py) against step_tail_ref.optimizer_ref, the new
entries' symbols, declarations and argument refusals (no launch), and the Optimizer / Trainer / parser errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import accum_ref as ref
import step_tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("momentum", "rmsprop", "adam")
NEW_SYMBOLS = ("rn_step_control_eval", "rn_optimizer_update")


def _same(a, b):
    for x, y in zip(a, b):
        for f, g in zip(x, y):
            assert (f is None and g is None) or np.array_equal(np.asarray(f), np.asarray(g))


@pytest.mark.parametrize("kind", KINDS)
def test_one_step_cycles_are_the_plain_reference(kind):
    """A = 1: every gradient is its own mean, and the run is step_tail_ref.optimizer_ref's, exactly."""
    inp = ref.accum_case("small", 1)
    assert len(inp.grads) == ref.UPDATES + ref.REST
    run = ref.accum_ref(inp, kind, 1)
    _same(run.steps, step_tail_ref.optimizer_ref(inp, kind))
    assert len(run.acc) == len(inp.grads) and not any(a.any() for a in run.acc)      # every micro-step applies: nothing is ever stored


@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_copies_of_one_gradient_are_one_step_on_it(kind, A):
    inp = ref.accum_case("small", 1)
    one = inp._replace(grads=inp.grads[:1])
    many = inp._replace(grads=inp.grads[:1] * A)
    run = ref.accum_ref(many, kind, A)
    assert len(run.steps) == 1 and len(run.acc) == A
    _same(run.steps, step_tail_ref.optimizer_ref(one, kind))
    g = inp.grads[0].astype(np.float64) * inp.grad_scale
    for m in range(A - 1):
        np.testing.assert_allclose(run.acc[m], (m + 1) * g, rtol=1e-15)
    assert np.array_equal(run.acc[A - 1], run.acc[A - 2])                              # the applying micro-step stores nothing


def test_reference_shape_and_sensitivity():
    """2A + 1 micro-steps give two updates; the sum restarts with the third cycle; applying a SUM instead of the mean, or the last
    gradient alone, moves most weights by more than the GPU test's 1e-4."""
    A = 3
    inp = ref.accum_case("small", A)
    assert len(inp.grads) == 2 * A + 1 and inp.lr == ref.LR
    run = ref.accum_ref(inp, "momentum", A)
    assert len(run.steps) == 2 and len(run.acc) == 7 and run.e is None
    np.testing.assert_allclose(run.acc[6], inp.grads[6].astype(np.float64) * inp.grad_scale, rtol=0)
    np.testing.assert_allclose(run.acc[4], (inp.grads[3].astype(np.float64) + inp.grads[4]) * inp.grad_scale, rtol=1e-15)
    keep = ~step_tail_ref.padding_mask(inp)
    assert not any(a[~keep].any() for a in run.acc)
    true = run.steps[0].w
    for bad in (inp._replace(grads=tuple(A * m for m in run.means)), inp._replace(grads=(inp.grads[A - 1],))):
        w = step_tail_ref.optimizer_ref(bad, "momentum")[0].w
        floor = 1e-3 * np.abs(true).max()
        frac = float(((np.abs(w - true) / np.maximum(np.abs(true), floor))[keep] > 1e-4).mean())
        assert frac > 0.5, frac
    assert len(ref.accum_ref(inp, "adam", A, setting="warm").e) == 2


def test_exact_case_is_exact_in_float32():
    for A in (2, 4):
        inp = ref.exact_case(A)
        assert len(inp.grads) == 2 * A and inp.grad_scale == 1.0 and not inp.wd_elem.any()
        m64 = ref.cycle_means(inp, A)
        acc = np.zeros(inp.count, np.float32)
        for u in range(2):
            acc[:] = 0
            for g in inp.grads[u * A:(u + 1) * A]:
                assert np.array_equal(g * 64, np.round(g * 64)) and np.abs(g).max() <= 1024
                acc = acc + g                                                           # float32 sums, in the kernel's order
            assert acc.dtype == np.float32 and np.array_equal((acc * np.float32(1.0 / A)).astype(np.float64), m64[u])


def test_new_symbols_are_exported_and_declared():
    import _rn
    raw = ctypes.CDLL(_rn.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), "librn_hip.so does not export %s" % sym
        assert sym in _rn.SYMBOLS and re.search(r"\bint %s\(" % sym, hdr), sym
    version = int(re.search(r"#define RN_API_VERSION (\d+)", hdr).group(1))
    assert version >= 413 and raw.rn_version() == version == _rn.API_VERSION


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every call below is refused by the entry's own checks, ahead of any launch: it runs on a box without a GPU, with host
    pointers that are never dereferenced."""
    import _rn
    import train
    from helpers import step_control
    L = _rn.lib()
    buf = torch.zeros(2048 + 4, dtype=torch.float32)
    base = buf.data_ptr() + (-buf.data_ptr()) % 16                   # a 16-byte aligned host address
    word = torch.zeros(1, dtype=torch.int64).data_ptr()
    pair = torch.zeros(2, dtype=torch.int32).data_ptr()
    two = torch.zeros(2, dtype=torch.float32).data_ptr()
    part = torch.zeros(8, dtype=torch.float64).data_ptr()
    sched = train.LRSchedule("constant", 0.1).struct()

    def ctl(A=2, micro_dev=word, accum_dev=pair, features=_rn.CTL_F_ACCUM, **fields):
        return step_control(features=features, accumulate_steps=A, micro_dev=micro_dev, accum_dev=accum_dev, **fields)
    for A in (0, -3):
        assert ctl(A=A) != 0
    assert ctl(micro_dev=None) != 0 and ctl(accum_dev=None) != 0
    lr = dict(features=_rn.CTL_F_ACCUM | _rn.CTL_F_LR, schedule=sched, step_dev=word, lr_dev=two)
    assert ctl(**dict(lr, accum_dev=None)) != 0                                      # the gate's word
    assert ctl(**dict(lr, step_dev=None)) != 0
    assert ctl(optimizer_kind=7, **lr) != 0                                          # (the ungated checks come along)
    ema = dict(features=_rn.CTL_F_ACCUM | _rn.CTL_F_EMA, ema_decay=0.5, ema_warmup=1, ema_updates_dev=word, ema_dev=two)
    assert ctl(**dict(ema, accum_dev=None)) != 0
    assert ctl(**dict(ema, ema_dev=None)) != 0
    assert ctl(**dict(ema, ema_decay=1.0)) != 0

    def step(acc=base, accum_dev=pair, partial=part, count=1024, inv=0.5, ema=None, ema_dev=None, state2=None, kind=0):
        f = _rn.OPT_F_NORM | _rn.OPT_F_ACCUM | (_rn.OPT_F_EMA if None not in (ema, ema_dev) else 0)
        u = _rn.OptUpdate(kind=kind, features=f, w=base, grad=base, state1=base, state2=state2, wd_per_block=two, count=count, lr=0.1,
                          grad_scale=1.0, step=1, partial=partial, ema=ema, ema_dev=ema_dev, acc=acc, inv_accum=inv, accum_dev=accum_dev)
        return L.rn_optimizer_update(ctypes.byref(u), None)
    assert step(acc=None) != 0 and step(accum_dev=None) != 0 and step(partial=None) != 0
    assert step(acc=base + 4) != 0                                                   # not 16-byte aligned
    assert b"16-byte" in L.rn_last_error()
    assert step(count=1000) != 0 and step(count=0) != 0
    for inv in (0.0, -0.5, 1.5, float("nan")):
        assert step(inv=inv) != 0
    assert b"inv_accum" in L.rn_last_error()
    assert step(ema=base) != 0 and step(ema_dev=two) != 0 and step(ema=base + 4, ema_dev=two) != 0
    assert step(kind=2) != 0 and step(kind=9, state2=base) != 0                      # Adam without state2; an unknown kind


def _arena():
    import train
    mod = torch.nn.Module()
    mod.p = torch.nn.Parameter(torch.zeros(3))
    return mod, train.ParamArena(mod, torch.device("cpu"))


def test_optimizer_and_trainer_refuse_senseless_accumulation():
    import _rn
    import train
    mod, arena = _arena()
    for bad in (0, -1, 1.5, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="accumulate_steps"):
            train.Optimizer(arena, "momentum", 0.1, accumulate_steps=bad)
    with pytest.raises(ValueError, match="grad_clip_norm"):
        train.Optimizer(arena, "momentum", 0.1, grad_clip_norm=1.0, accumulate_steps=2)
    with pytest.raises(_rn.RnError, match="device arena"):
        train.Optimizer(arena, "momentum", 0.1, accumulate_steps=2)                  # a CPU arena
    with pytest.raises(_rn.RnError, match="device arena"):
        train.Trainer(mod, device="cpu", accumulate_steps=2)
    with pytest.raises(ValueError, match="accumulate_steps"):
        train.Trainer(mod, device="cpu", accumulate_steps=0)
    with pytest.raises(ValueError, match="grad_clip_norm"):
        train.Trainer(mod, device="cpu", accumulate_steps=4, grad_clip_norm=0.5)


def test_cpu_arena_without_accumulation_is_as_before():
    import train
    mod, arena = _arena()
    for kw in ({}, {"accumulate_steps": 1}):
        opt = train.Optimizer(arena, "momentum", 0.1, **kw)
        assert opt.accumulate_steps == 1 and opt.acc is None and opt.micro_dev is None and opt.accum_dev is None
        assert [opt.count_step() for _ in range(3)] == [True] * 3 and opt.step_count == 3
    tr = train.Trainer(mod, device="cpu", accumulate_steps=1)
    assert tr.opt.acc is None and tr.opt.accumulate_steps == 1


def _args(*argv):
    import train
    return train.build_parser().parse_args(list(argv))


@pytest.mark.parametrize("argv", [("--accumulate-steps", "0"), ("--accumulate-steps", "65"), ("--accumulate-steps", "-2"),
                                  ("--accumulate-steps", "2", "--grad-clip-norm", "1.0")])
def test_senseless_accumulate_flags_are_parser_errors(argv, capsys):
    import train
    assert train.accumulate_flag_error(_args(*argv))
    with pytest.raises(SystemExit) as e:                                         # main(): parser.error, before any device is touched
        train.main(list(argv))
    assert e.value.code == 2 and "--accumulate-steps" in capsys.readouterr().err


def test_sensible_accumulate_flags_and_the_schedule_in_updates():
    import train
    a = _args()
    assert a.accumulate_steps == 1 and train.accumulate_flag_error(a) is None
    assert train.accumulate_flag_error(_args("--grad-clip-norm", "1.0")) is None
    assert train.accumulate_flag_error(_args("--accumulate-steps", "64")) is None
    # --lr-total-steps defaults to the UPDATES the run ends at: updates restored + (phase + epochs x steps per epoch) // A
    s = train.schedule_from_args(_args("--lr-schedule", "cosine", "--epochs", "3", "--accumulate-steps", "4"), 100, 10, 3)
    assert s.total_steps == 10 + (3 + 300) // 4 == 85
    s = train.schedule_from_args(_args("--lr-schedule", "cosine", "--epochs", "3", "--accumulate-steps", "4"), 100, 0)
    assert s.total_steps == 75
    s = train.schedule_from_args(_args("--lr-schedule", "cosine", "--epochs", "3"), 100, 40)
    assert s.total_steps == 340                                                  # without the flag: as before
    assert "UPDATES" in train.build_parser().format_help()
