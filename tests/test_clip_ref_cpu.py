"""Global-norm clipping without a GPU: the float64 reference (clip_ref.py) against step_tail_ref.optimizer_ref, the clip values
and the schedule the GPU tests rely on, the new entries' symbols, declarations and argument refusals (no launch), and the errors
that stay: clipping with accumulation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as ref
import step_tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("momentum", "rmsprop", "adam")
NEW_SYMBOLS = ("rn_optimizer_update", "rn_grad_norm_partial")


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f, g in zip(x, y):
            assert (f is None and g is None) or np.array_equal(np.asarray(f), np.asarray(g))


@pytest.mark.parametrize("clip", [None, ref.CLIP_BINDS, ref.CLIP_LOOSE], ids=["none", "binds", "loose"])
@pytest.mark.parametrize("kind", KINDS)
def test_constant_rates_are_the_step_tail_reference(kind, clip):
    """Without rates, and with inp.lr handed in as the rate of every update, the run is step_tail_ref.optimizer_ref's, exactly."""
    inp = ref.clip_case("small")
    want = step_tail_ref.optimizer_ref(inp, kind, clip)
    _same(ref.optimizer_steps(inp, kind, clip), want)
    _same(ref.optimizer_steps(inp, kind, clip, rates=[inp.lr] * len(inp.grads)), want)
    run = ref.clip_ref(inp, kind, clip, setting="warm")
    _same(run.steps, want)
    assert len(run.e) == len(want) and not np.array_equal(run.e[-1], want[-1].w)


def test_the_clips_bind_and_do_not_and_the_rates_differ():
    """The small case is optimizer_case("small") (SMALL_SIZES, seed 11), three updates: CLIP_BINDS binds at every update, CLIP_LOOSE
    at none, in the clipped run and in the scheduled one; the schedule's three rates are base / 3, 2 base / 3 and base."""
    inp = ref.clip_case("small")
    assert inp is step_tail_ref.optimizer_case("small") and inp.sizes == step_tail_ref.SMALL_SIZES and len(inp.grads) == ref.UPDATES
    rates = ref.rates(inp)
    assert len(set(rates)) == 3 and rates[2] == float(np.float32(inp.lr))
    np.testing.assert_allclose(rates, [inp.lr / 3, inp.lr * 2 / 3, inp.lr], rtol=1e-6)
    for kind in KINDS:
        for r in (None, rates):
            for st in ref.optimizer_steps(inp, kind, ref.CLIP_BINDS, r):
                assert st.norm > 10 * ref.CLIP_BINDS and ref.clip_scale(st.norm, ref.CLIP_BINDS) < 0.1
            for st in ref.optimizer_steps(inp, kind, ref.CLIP_LOOSE, r):
                assert st.norm < ref.CLIP_LOOSE and ref.clip_scale(st.norm, ref.CLIP_LOOSE) == 1.0
    large = ref.clip_case("large")
    assert large.sizes == step_tail_ref.LARGE_SIZES and large.sizes[-1] % step_tail_ref.OPT_BLOCK != 0
    n2, _ = ref.norm_and_reg(large, large.grads[0])
    assert n2 ** 0.5 > ref.CLIP_BINDS


def test_reference_sensitivity():
    """A clip that binds, a rate that is scheduled, and a clip scale formed without the regulariser's gradient each move most
    weights by more than the GPU test's 1e-4 (element-wise): the comparisons there can tell them apart."""
    inp = ref.clip_case("small")
    keep = ~step_tail_ref.padding_mask(inp)
    true = ref.optimizer_steps(inp, "momentum", ref.CLIP_BINDS, ref.rates(inp))

    def frac(w, t):
        floor = 1e-3 * np.abs(t).max()
        return float(((np.abs(w - t) / np.maximum(np.abs(t), floor))[keep] > 1e-4).mean())
    # (the clipped update moves a weight by about lr * 0.5 / 100 * |g'|: small against |w| ~ 1, so the first slot carries the check)
    unclipped = ref.optimizer_steps(inp, "momentum", None, ref.rates(inp))
    assert frac(unclipped[0].state1, true[0].state1) > 0.9
    constant = ref.optimizer_steps(inp, "adam", ref.CLIP_BINDS)
    scheduled = ref.optimizer_steps(inp, "adam", ref.CLIP_BINDS, ref.rates(inp))
    assert frac(constant[0].w, scheduled[0].w) > 0.5
    # the norm of grad * grad_scale alone, the header's old formula: another clip scale
    g = inp.grads[0].astype(np.float64) * inp.grad_scale
    assert abs(np.sqrt((g * g).sum()) / true[0].norm - 1.0) > 1e-3


def test_norm_of_slices_adds_up():
    inp = ref.clip_case("small")
    whole = ref.norm_and_reg(inp, inp.grads[0])
    parts = [ref.norm_and_reg(inp, inp.grads[0], lo=lo, hi=hi) for lo, hi in step_tail_ref.SMALL_SLICES]
    np.testing.assert_allclose([sum(p[0] for p in parts), sum(p[1] for p in parts)], whole, rtol=1e-13)
    st = ref.optimizer_steps(inp, "momentum", ref.CLIP_BINDS)[0]
    np.testing.assert_allclose([whole[0] ** 0.5, whole[1]], [st.norm, st.reg], rtol=1e-13)


def test_new_symbols_are_exported_and_declared():
    import _rn
    raw = ctypes.CDLL(_rn.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), "librn_hip.so does not export %s" % sym
        assert sym in _rn.SYMBOLS and re.search(r"\bint %s\(" % sym, hdr), sym
    version = int(re.search(r"#define RN_API_VERSION (\d+)", hdr).group(1))
    assert version >= 414 and raw.rn_version() == version == _rn.API_VERSION
    # the header's formula: the clip scale multiplies the regulariser's gradient too
    assert "(grad*grad_scale + wd*w) * clip_scale" in hdr and "grad*grad_scale*clip_scale" not in hdr


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every call below is refused by the entry's own checks with RN_EINVAL (-1) and a message, ahead of any launch: it runs on a
    box without a GPU, with fake non-null pointers that are never dereferenced."""
    import _rn
    L = _rn.lib()
    q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)

    def clip(kind=0, state2=None, count=1024, lr_dev=None, clip_norm=0.5, norm_sq=q, step=1, ema=None, ema_dev=None, w=q):
        f = _rn.OPT_F_CLIP | (_rn.OPT_F_LRDEV if lr_dev is not None else 0) | (_rn.OPT_F_EMA if None not in (ema, ema_dev) else 0)
        u = _rn.OptUpdate(kind=kind, features=f, w=w, grad=q, state1=q, state2=state2, wd_per_block=q, count=count, lr=0.1,
                          grad_scale=1.0, step=step, lr_dev=lr_dev, ema=ema, ema_dev=ema_dev, clip_norm=clip_norm, norm_sq=norm_sq)
        return L.rn_optimizer_update(ctypes.byref(u), None)
    for c in (0.0, -1.0, float("nan")):
        assert clip(clip_norm=c) == -1
        assert b"clip_norm" in L.rn_last_error()
    assert clip(norm_sq=None) == -1 and b"norm_sq" in L.rn_last_error()
    assert clip(ema=q) == -1 and b"go together" in L.rn_last_error()
    assert clip(ema_dev=q) == -1 and b"go together" in L.rn_last_error()
    assert clip(ema=odd, ema_dev=q) == -1 and b"16-byte" in L.rn_last_error()
    assert clip(count=1000) == -1 and b"multiple" in L.rn_last_error()
    assert clip(count=0) == -1
    assert clip(kind=1) == -1 and b"state2" in L.rn_last_error()
    assert clip(kind=2) == -1 and b"state2" in L.rn_last_error()
    assert clip(kind=2, lr_dev=q) == -1 and b"state2" in L.rn_last_error()
    assert clip(kind=2, state2=q, step=0) == -1 and b"step" in L.rn_last_error()
    assert clip(kind=9, state2=q) == -1 and b"kind" in L.rn_last_error()
    assert clip(w=None) == -1

    def part(w=q, g=q, wd=q, count=1024, partial=q):
        return L.rn_grad_norm_partial(w, g, wd, count, 1.0, partial, None)
    assert part(w=None) == -1 and b"grad_norm_partial" in L.rn_last_error()
    assert part(g=None) == -1 and part(wd=None) == -1 and part(partial=None) == -1
    assert part(count=1000) == -1 and b"multiple" in L.rn_last_error()
    assert part(count=0) == -1 and part(count=-1024) == -1


def _arena():
    import train
    mod = torch.nn.Module()
    mod.p = torch.nn.Parameter(torch.zeros(3))
    return mod, train.ParamArena(mod, torch.device("cpu"))


def test_clipping_with_accumulation_is_still_refused():
    import train
    mod, arena = _arena()
    with pytest.raises(ValueError, match="grad_clip_norm"):
        train.Optimizer(arena, "momentum", 0.1, grad_clip_norm=1.0, accumulate_steps=2)
    with pytest.raises(ValueError, match="grad_clip_norm"):
        train.Trainer(mod, device="cpu", accumulate_steps=4, grad_clip_norm=0.5)
    args = train.build_parser().parse_args(["--accumulate-steps", "2", "--grad-clip-norm", "1.0"])
    assert train.accumulate_flag_error(args)
    # ... and clipping alone is accepted, with any optimizer, with and without a schedule
    for kind in KINDS:
        opt = train.Optimizer(arena, kind, 0.1, grad_clip_norm=1.0, schedule=train.LRSchedule("cosine", 0.1, total_steps=5))
        assert opt.clip == 1.0 and opt.accumulate_steps == 1
    assert train.Optimizer(arena, "momentum", 0.1).clip == 0.0


def test_clip_no_longer_bars_the_one_graph_step():
    """_whole_step_ok does not look at the clip any more (on a CPU device it is False for the device's sake alone), and the help
    and the docstrings say so."""
    import inspect
    import train
    src = inspect.getsource(train.Trainer._whole_step_ok)
    assert "clip" not in src and "lr_dev is not None" in src and "kind == 'momentum'" in src
    mod, _ = _arena()
    assert not train.Trainer(mod, device="cpu", grad_clip_norm=1.0)._whole_step_ok()
    help_ = " ".join(train.build_parser().format_help().split())
    assert "--grad-clip-norm" in help_ and "inside the captured step" in help_
