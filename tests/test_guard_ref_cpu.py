"""The guard against non-finite gradients without a GPU: the float64 reference (guard_ref.py) against itself and against
clip_ref, the three poisons and why the case is drawn at grad_scale 0.75, the flags, the refusals that need no device, and the new
entries' symbols, declarations and argument checks (no launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clip_ref
import guard_ref as ref
import step_tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("momentum", "rmsprop", "adam")
NEW_SYMBOLS = ("rn_step_control_eval", "rn_optimizer_update")
FLT_MAX = float(np.finfo(np.float32).max)


def _same_runs(a, b):
    assert len(a.steps) == len(b.steps)
    for x, y in zip(a.steps, b.steps):
        for f, g in zip(x, y):
            assert (f is None and g is None) or np.array_equal(np.asarray(f), np.asarray(g))
    assert (a.e is None) == (b.e is None)
    if a.e is not None:
        assert len(a.e) == len(b.e) and all(np.array_equal(p, q) for p, q in zip(a.e, b.e))


def test_the_case_is_the_small_arena_and_the_poisons_are_what_they_say():
    inp = ref.guard_case()
    small = clip_ref.clip_case("small")
    assert inp.sizes == step_tail_ref.SMALL_SIZES == (1152, 700, 1, 1025, 3000) and inp.count == 9 * step_tail_ref.OPT_BLOCK
    assert inp.grad_scale == ref.GRAD_SCALE == 0.75 and len(inp.grads) == 3
    assert np.array_equal(inp.w0, small.w0) and np.array_equal(inp.wd_elem, small.wd_elem) and inp.offsets == small.offsets
    # the gradients are drawn through g': the same g' as the small case's, so its clip values bind / do not bind alike
    for g, h in zip(inp.grads, small.grads):
        np.testing.assert_allclose(g.astype(np.float64) * inp.grad_scale, h.astype(np.float64) * small.grad_scale, rtol=1e-6, atol=1e-6)
    for which in ref.POISONS:
        bad = ref.poisoned(inp, which)
        diff = np.flatnonzero(~((bad == inp.grads[1]) | (np.isnan(bad) & np.isnan(inp.grads[1]))))
        assert list(diff) == [ref.poison_index(inp, which)]
    assert ref.poison_index(inp, "nan") == inp.offsets[2] and np.isnan(ref.poisoned(inp, "nan")[inp.offsets[2]])
    assert ref.poison_index(inp, "inf") == inp.offsets[4] + 2999 and ref.poisoned(inp, "inf")[inp.offsets[4] + 2999] == np.inf
    assert ref.poison_index(inp, "overflow") == 576 and ref.poisoned(inp, "overflow")[576] == np.float32(3e19)


def test_the_criterion_classifies_the_three_poisons_as_skipped():
    """NaN, inf, and the third case: every element of the gradient -- and of g' -- is finite, and the float sum of squares is not.
    At clip_case("small")'s grad_scale of 0.5 the same 3e19 would NOT overflow (g'^2 = 2.25e38 < FLT_MAX): the reason the guard's
    case is drawn at 0.75."""
    inp = ref.guard_case()
    for g in inp.grads:
        n2 = ref.norm_sq_float(inp, g, inp.w0)
        assert np.isfinite(n2) and 50.0 < float(n2) ** 0.5 < 200.0
    assert np.isnan(ref.norm_sq_float(inp, ref.poisoned(inp, "nan"), inp.w0))
    assert ref.norm_sq_float(inp, ref.poisoned(inp, "inf"), inp.w0) == np.inf
    bad = ref.poisoned(inp, "overflow")
    assert np.isfinite(bad).all() and float(np.float32(3e19)) ** 2 > FLT_MAX
    gp = bad.astype(np.float64) * inp.grad_scale + inp.wd_elem.astype(np.float64) * inp.w0
    assert np.isfinite(gp.astype(np.float32)).all() and float((gp * gp).sum()) > FLT_MAX
    assert ref.norm_sq_float(inp, bad, inp.w0) == np.inf
    at_half = ref.norm_sq_float(inp, bad, inp.w0, grad_scale=0.5)
    assert np.isfinite(at_half) and 2.2e38 < float(at_half) < 2.3e38


@pytest.mark.parametrize("which", ref.POISONS)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_with_skips_equals_the_run_without_them(kind, which):
    """[g0, BAD, g1, BAD, BAD, g2] is [g0, g1, g2], counters (3, 0); [g0, BAD, BAD] is [g0], counters (2, 2) -- constant rate
    and scheduled (the rates count applied updates), clipped and not, with the moving average."""
    inp = ref.guard_case()
    g0, g1, g2 = inp.grads
    bad = ref.poisoned(inp, which)
    for clip in (None, ref.CLIP_BINDS):
        for scheduled in (False, True):
            want = clip_ref.clip_ref(inp, kind, clip, ref.rates(inp, 3) if scheduled else None, "warm")
            got = ref.guard_ref(inp, [g0, bad, g1, bad, bad, g2], kind, clip, scheduled, "warm")
            _same_runs(got.run, want)
            assert got.applied == (True, False, True, False, False, True)
            assert got.counters == ((0, 0), (1, 1), (1, 0), (2, 1), (3, 2), (3, 0)) and got.counters[-1] == (3, 0)
            assert all(np.isfinite(n) == a for n, a in zip(got.norm_sq, got.applied))
            short = ref.guard_ref(inp, [g0, bad, bad], kind, clip, scheduled, "warm")
            assert short.counters[-1] == (2, 2) and len(short.run.steps) == 1 and len(short.run.e) == 1
            for f, g in zip(short.run.steps[0], want.steps[0]):
                assert (f is None and g is None) or np.array_equal(np.asarray(f), np.asarray(g))
            # without a skip the guard's reference IS clip_ref
            _same_runs(ref.guard_ref(inp, list(inp.grads), kind, clip, scheduled, "warm").run, want)
    assert ref.guard_ref(inp, [bad], kind).counters == ((1, 1),) and not ref.guard_ref(inp, [bad], kind).run.steps


def test_scheduled_rates_count_applied_updates():
    """A skip does not consume a rate: the update after it takes the rate the skipped one would have had -- which moves the
    weights by far more than the GPU test's tolerance."""
    inp = ref.guard_case()
    g0, g1, _ = inp.grads
    got = ref.guard_ref(inp, [g0, ref.poisoned(inp, "nan"), g1], "adam", None, True)
    wrong = clip_ref.optimizer_steps(inp._replace(grads=(g0, g1)), "adam", None, [ref.rates(inp, 3)[0], ref.rates(inp, 3)[2]])
    keep = ~step_tail_ref.padding_mask(inp)
    moved = np.abs(got.run.steps[1].w - got.run.steps[0].w)[keep]
    off = np.abs(got.run.steps[1].w - wrong[1].w)[keep]
    assert np.median(off / moved) > 0.2


def _args(*argv):
    import train
    return train.build_parser().parse_args(list(argv))


def test_guard_flags():
    import train
    ok = (["--skip-nonfinite"], ["--skip-nonfinite", "--grad-clip-norm", "1.0"], ["--skip-nonfinite", "--lr-schedule", "cosine"],
          ["--skip-nonfinite", "--ema-decay", "0.99"], ["--skip-nonfinite", "--nonfinite-limit", "1"], [])
    for argv in ok:
        assert train.guard_flag_error(_args(*argv)) is None, argv
    err = train.guard_flag_error(_args("--accumulate-steps", "2", "--skip-nonfinite"))
    assert err and "--accumulate-steps" in err and "--skip-nonfinite" in err
    err = train.guard_flag_error(_args("--nonfinite-limit", "3"))
    assert err and "--skip-nonfinite" in err
    for n in ("0", "-2"):
        err = train.guard_flag_error(_args("--skip-nonfinite", "--nonfinite-limit", n))
        assert err and "--nonfinite-limit" in err
    a = _args()
    assert a.skip_nonfinite is False and a.nonfinite_limit is None
    help_ = " ".join(train.build_parser().format_help().split())
    assert "--skip-nonfinite" in help_ and "--nonfinite-limit" in help_


def _arena():
    import train
    mod = torch.nn.Module()
    mod.p = torch.nn.Parameter(torch.zeros(3))
    return mod, train.ParamArena(mod, torch.device("cpu"))


def test_guard_needs_a_device_arena_and_refuses_accumulation():
    import _rn
    import train
    mod, arena = _arena()
    for kind in KINDS:
        with pytest.raises(_rn.RnError, match="device arena"):
            train.Optimizer(arena, kind, 0.1, skip_nonfinite=True)
    with pytest.raises(_rn.RnError, match="device arena"):
        train.Trainer(mod, device="cpu", skip_nonfinite=True)
    with pytest.raises(ValueError, match="skip_nonfinite.*accumulate_steps"):
        train.Optimizer(arena, "momentum", 0.1, skip_nonfinite=True, accumulate_steps=2)
    with pytest.raises(ValueError, match="skip_nonfinite.*accumulate_steps"):
        train.Trainer(mod, device="cpu", skip_nonfinite=True, accumulate_steps=2)
    # off by default: nothing of the guard exists, and the count it would correct is untouched
    opt = train.Optimizer(arena, "adam", 0.1)
    assert opt.skip_nonfinite is False and opt.gate_dev is None and opt.skipped_dev is None and opt.schedule is None
    opt.step_count = 5
    assert opt.reconcile_skips() == (0, 0) and opt.step_count == 5
    assert train.Trainer(mod, device="cpu").skipped_updates() == (0, 0)
    assert train.check_nonfinite_limit(train.Trainer(mod, device="cpu"), 1) == 0


def test_the_guard_is_part_of_the_graph_key_and_adds_no_condition():
    import inspect
    import train
    assert "skip_nonfinite" in inspect.getsource(train.Trainer.step)
    src = inspect.getsource(train.Trainer._whole_step_ok)
    assert "skip" not in src and "gate" not in src and "lr_dev is not None" in src
    # (the order of the guarded step's launches: tests/test_gpu_guard.py::test_every_configuration_takes_the_one_sequence)


def test_new_symbols_are_exported_and_declared():
    import _rn
    raw = ctypes.CDLL(_rn.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), "librn_hip.so does not export %s" % sym
        assert sym in _rn.SYMBOLS and re.search(r"\bint %s\(" % sym, hdr), sym
    version = int(re.search(r"#define RN_API_VERSION (\d+)", hdr).group(1))
    assert version >= 415 and raw.rn_version() == version == _rn.API_VERSION


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every call below is refused by the entry's own checks with RN_EINVAL (-1) and a message, ahead of any launch: fake non-null
    pointers that are never dereferenced."""
    import _rn
    import train
    from helpers import step_control
    L = _rn.lib()
    q, odd2, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 2), ctypes.c_void_p(4096 + 4)

    def gate(norm_sq=q, gate_dev=q, skipped=q, features=_rn.CTL_F_GUARD, **fields):
        return step_control(features=features, norm_sq=norm_sq, gate_dev=gate_dev, skipped_dev=skipped, **fields)
    assert gate(norm_sq=None) == -1 and b"step_control" in L.rn_last_error() and b"GUARD" in L.rn_last_error()
    assert gate(gate_dev=None) == -1 and gate(skipped=None) == -1
    assert gate(norm_sq=odd2) == -1 and b"misaligned" in L.rn_last_error()
    assert gate(gate_dev=odd2) == -1 and gate(skipped=odd4) == -1 and b"misaligned" in L.rn_last_error()
    # a bit and its pointers in disagreement, either way round; the two gates together; an unknown bit; no bit at all
    lr = dict(schedule=train.LRSchedule("constant", 0.1).struct(), step_dev=q, lr_dev=q)
    ema = dict(ema_decay=0.5, ema_warmup=1, ema_updates_dev=q, ema_dev=q)
    accum = dict(accumulate_steps=2, micro_dev=q, accum_dev=q)
    for bit, fields in ((_rn.CTL_F_LR, lr), (_rn.CTL_F_EMA, ema), (_rn.CTL_F_ACCUM, accum)):
        assert gate(**fields) == -1 and b"only with it" in L.rn_last_error()                       # pointers set, bit clear
        for name in fields:
            if name.endswith("_dev"):
                assert step_control(features=bit, **dict(fields, **{name: None})) == -1 and b"only with it" in L.rn_last_error()
    assert step_control(features=_rn.CTL_F_LR, norm_sq=q, gate_dev=q, skipped_dev=q, **lr) == -1 and b"GUARD" in L.rn_last_error()
    assert gate(features=_rn.CTL_F_GUARD | _rn.CTL_F_ACCUM, **accum) == -1 and b"ACCUM goes with no GUARD" in L.rn_last_error()
    assert gate(features=_rn.CTL_F_GUARD | 16) == -1 and b"unknown feature bit" in L.rn_last_error()
    assert step_control(features=0) == -1 and b"no feature" in L.rn_last_error()
    assert L.rn_step_control_eval(None, None) == -1 and b"null descriptor" in L.rn_last_error()
    def step(kind=0, state2=None, count=1024, lr_dev=None, clip_norm=0.0, norm_sq=None, step=1, ema=None, ema_dev=None, w=q, gate_dev=q):
        f = (_rn.OPT_F_GATE | (_rn.OPT_F_CLIP if clip_norm > 0 else 0) | (_rn.OPT_F_LRDEV if lr_dev is not None else 0)
             | (_rn.OPT_F_EMA if None not in (ema, ema_dev) else 0))
        u = _rn.OptUpdate(kind=kind, features=f, w=w, grad=q, state1=q, state2=state2, wd_per_block=q, count=count, lr=0.1,
                          grad_scale=1.0, step=step, lr_dev=lr_dev, ema=ema, ema_dev=ema_dev, clip_norm=clip_norm, norm_sq=norm_sq,
                          gate_dev=gate_dev)
        return L.rn_optimizer_update(ctypes.byref(u), None)
    assert step(gate_dev=None) == -1 and b"gate_dev" in L.rn_last_error()
    assert step(gate_dev=odd2) == -1 and b"aligned" in L.rn_last_error()
    for c in (-1.0, float("nan")):
        assert step(clip_norm=c) == -1 and b"clip_norm" in L.rn_last_error()
    assert step(clip_norm=0.5) == -1 and b"norm_sq" in L.rn_last_error()
    assert step(ema=q) == -1 and b"go together" in L.rn_last_error()
    assert step(ema_dev=q) == -1 and b"go together" in L.rn_last_error()
    assert step(ema=odd4, ema_dev=q) == -1 and b"16-byte" in L.rn_last_error()
    assert step(count=1000) == -1 and b"multiple" in L.rn_last_error()
    assert step(count=0) == -1 and step(w=None) == -1
    assert step(kind=1) == -1 and b"state2" in L.rn_last_error()
    assert step(kind=2, lr_dev=q) == -1 and b"state2" in L.rn_last_error()
    assert step(kind=2, state2=q, step=0) == -1 and b"step" in L.rn_last_error()
    assert step(kind=9, state2=q) == -1 and b"kind" in L.rn_last_error()
