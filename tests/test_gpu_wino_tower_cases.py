"""The GroupNorm-folded Winograd tower (ops.wino_tower: rn_conv3x3_winograd_gn, _gn_bwd, _gn_bwd_wgrad, _gn_weights) at every
planner branch of csrc/winograd.hip's folded layers, against the fp64 evaluation of tests/wino_tower_ref.tower_ref.  The cases
and the branch each one takes: wino_tower_ref.CASES and tests/test_wino_tower_cases_cpu.py (which proves the branches on the
CPU from the library's own plan query).  Compared: every level's output, the gradient of every level's input, of every
layer's kernel / gamma / beta and of the output conv's kernel and bias, each against ITS OWN maximum (helpers.rel_err) -- no
floor shared between tensors.

Two bars per tensor:
  * the project's: outputs 1e-4 (BASELINE north_star), gradients 5e-4 (what tests/test_gpu_wino_tower.py grants a pyramid
    with a 1 x 1 level, whose GroupNorms see two values per group: the "head" cases have one);
  * one tied to the arithmetic: with e32 = rel_err(tower_ref in fp32, tower_ref in fp64) and ek = rel_err(kernel, fp64),
    ek / max(e32, 2^-23) <= RATIO_BOUND[tile].  e32 comes from the reference alone and is a DIRECT convolution; the Winograd
    transforms amplify rounding (F(4x4,3x3) more than F(2x2,3x3): its matrices hold entries up to 8), so a ratio well above 1
    is expected.  The kernels are bitwise reproducible, so the figure has no run-to-run noise.
RATIO_BOUND = {tile 2: 4, tile 4: 64}, set on 2026-10-20: per tile size twice the largest ratio of any tensor of any case of
that tile size in one run of the table on an MI355X, rounded up to a power of two (figures: profiles/wino_tower_cases_err.txt).
  F(2x2,3x3): largest ratio 1.25 (unstaged-gnw1, the gradient of the first level's input: ek 4.4e-7, e32 3.5e-7);
  F(4x4,3x3): largest ratio 21.9 (relu6, the gradient of the first layer's kernel: ek 6.1e-6, e32 2.8e-7); the ratios of that
              tile size lie between 3 and 22, largest where e32 is smallest (the 4 x 5 and 5 x 6 maps), and the twin of
              "unstaged" (the same tensors at tile 4) has 12.9 where tile 2 has 1.23.
The largest ek was 9.4e-6 for an output and 1.9e-5 for a gradient (both head-fp32: 256 channels, product mode 0): 10 and 26
times inside the project's bars."""
import numpy as np
import pytest
import torch

import wino_tower_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
RATIO_BOUND = {2: 4.0, 4: 64.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


# the switches of tests/test_gpu_x3.py
@pytest.fixture()
def product_mode():
    import _rn
    L = _rn.lib()
    before = L.rn_get_product_mode()
    yield L.rn_set_product_mode
    L.rn_set_product_mode(before)


@pytest.fixture()
def bfrag_switch():
    import _rn
    L = _rn.lib()
    before = L.rn_get_x3_bfrag()
    yield L.rn_set_x3_bfrag
    L.rn_set_x3_bfrag(before)


@pytest.fixture()
def switches(monkeypatch, product_mode, bfrag_switch):
    return monkeypatch, product_mode, bfrag_switch


def run_tower(name, dev, switches, training=True, deferred=False):
    """The case through ops.wino_tower on `dev` -> ({output name: tensor}, {gradient name: tensor}); training=False: under
    torch.no_grad(), no gradients.  deferred: the weight-gradient halves are recorded (ops.WGRAD_DEFER) and run after the
    backward pass (ops.run_deferred_wgrads), every parameter gradient written in place (ops.DIRECT_PARAM_GRADS)."""
    import ops
    case = R.CASES[name]
    monkeypatch = switches[0]
    R.configure(case, *switches)
    xs, tower, ow, ob = R.make_case(case)

    def leaf(t):
        return t.to(dev).requires_grad_(training)

    xs = [leaf(x) for x in xs]
    tower = [tuple(leaf(t) for t in layer) for layer in tower]
    ow, ob = (leaf(ow), leaf(ob)) if case.cout else (None, None)
    assert ops.wino_tower_ok(xs, tower, ow, case.groups)
    kernels = [layer[0] for layer in tower] + ([ow] if case.cout else [])
    if case.variant == "rebuild-v":
        monkeypatch.setattr(ops, "WINOGRAD_WGRAD", False)
    if case.variant == "pretransform":
        registry, _ = ops.WinoPretransform(kernels).launch()
        assert len(registry) == len(kernels)
        monkeypatch.setattr(ops, "WINO_PRE", registry)

    def forward():
        try:
            return ops.wino_tower(xs, tower, ow, ob, groups=case.groups, eps=R.EPS, act=case.act)
        finally:
            monkeypatch.setattr(ops, "WINO_PRE", {})       # (the registry holds for ONE forward pass)

    if not training:
        with torch.no_grad():
            got = forward()
        return {"y%d" % i: t for i, t in enumerate(got)}, {}
    leaves = R.leaves_of(case, xs, tower, ow, ob)
    names = R.grad_names(case)
    cot = [c.to(dev) if c is not None else None for c in R.make_cotangents(case)]
    got = forward()
    roots = [(y, c) for y, c in zip(got, cot) if c is not None]      # a level without a cotangent is no root of the backward pass
    out = {"y%d" % i: t.detach() for i, t in enumerate(got)}
    if not deferred:
        grads = torch.autograd.grad([y for y, _ in roots], leaves, [c for _, c in roots])
        return out, dict(zip(names, grads))
    params = leaves[len(xs):]
    before = (ops.DIRECT_PARAM_GRADS, ops.WGRAD_DEFER)
    try:
        ops.DIRECT_PARAM_GRADS = True
        ops.begin_direct_grad_step()
        for p in params:
            p.grad = torch.zeros_like(p)
        ops.WGRAD_DEFER = []
        torch.autograd.backward([y for y, _ in roots], [c for _, c in roots])
        records = ops.WGRAD_DEFER
        assert len(records) == len(kernels)
        for w in kernels:                                   # "this call leaves dw alone" (rn_wino_gn_bwd.defer_wgrad)
            assert not bool(w.grad.any())
        ops.run_deferred_wgrads(records)
        torch.cuda.synchronize()
    finally:
        ops.DIRECT_PARAM_GRADS, ops.WGRAD_DEFER = before
        ops.begin_direct_grad_step()
    assert all(t.grad is not None for t in leaves)
    return out, {k: t.grad for k, t in zip(names, leaves)}


def compare(name, out, grads):
    """-> [(kind "out" / "grad", tensor name, ek, e32, ratio)] for every compared tensor of the case"""
    ref64, ref32 = R.reference(name, torch.float64), R.reference(name, torch.float32)
    rows = []
    for kind, got, r64, r32 in (("out", out, ref64[0], ref32[0]), ("grad", grads, ref64[1], ref32[1])):
        assert sorted(got) == sorted(r64)
        for tname in r64:
            a = got[tname].cpu().numpy()
            assert a.shape == r64[tname].shape and np.isfinite(a).all(), tname
            ek, e32 = rel_err(a, r64[tname]), rel_err(r32[tname], r64[tname])
            rows.append((kind, tname, ek, e32, ek / max(e32, 2.0 ** -23)))
    return rows


def worst(rows, kind):
    return max((r for r in rows if r[0] == kind), key=lambda r: r[4])


def record_line(name, rows):
    """The case's line of profiles/wino_tower_cases_err.txt."""
    parts = []
    for kind in ("out", "grad"):
        _, tname, ek, e32, ratio = worst(rows, kind)
        parts.append("%-4s %-7s ek %.3e  e32 %.3e  ratio %6.2f  (max ek %.3e)" % (kind, tname, ek, e32, ratio, max(r[2] for r in rows if r[0] == kind)))
    return "%-20s tile %d | %s | %s" % (name, R.CASES[name].tile, parts[0], parts[1])


def check(name, rows):
    bound = RATIO_BOUND[R.CASES[name].tile]
    bad = ["%s %s: ek %.3e (bar %.0e), e32 %.3e, ratio %.2f (bound %s)" % (kind, tname, ek, OUT_BAR if kind == "out" else GRAD_BAR, e32, ratio, bound)
           for kind, tname, ek, e32, ratio in rows
           if ek > (OUT_BAR if kind == "out" else GRAD_BAR) or ratio > bound]
    assert not bad, "case %s: %d of %d tensors off: %s" % (name, len(bad), len(rows), "; ".join(bad))


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matches_fp64(dev, switches, name):
    rows = compare(name, *run_tower(name, dev, switches))
    print(record_line(name, rows))
    check(name, rows)


@pytest.mark.parametrize("name", ["base", "head-gnw4"])
def test_second_run_is_bit_identical(dev, switches, name):
    """"No exchange between blocks, no atomics: every sum runs over rows an earlier launch wrote" (include/rn_hip.h):
    outputs and every gradient."""
    out_a, grads_a = run_tower(name, dev, switches)
    out_b, grads_b = run_tower(name, dev, switches)
    for a, b in ((out_a, out_b), (grads_a, grads_b)):
        for tname in a:
            assert torch.equal(a[tname], b[tname]), tname


@pytest.mark.parametrize("name", ["base", "head", "unstaged", "base-rebuild-v"])
def test_deferred_weight_gradients_are_bit_identical(dev, switches, name):
    """The weight-gradient half of every layer left for later (rn_wino_gn_bwd.defer_wgrad, run by rn_conv3x3_winograd_gn_bwd_wgrad
    from the call's workspace -- base-rebuild-v: from the V the backward call rebuilt there): every dw and every other
    gradient bitwise equal to the run that finishes dw inside the backward call (README), and within the fp64 bars."""
    out_a, grads_a = run_tower(name, dev, switches)
    out_b, grads_b = run_tower(name, dev, switches, deferred=True)
    for a, b in ((out_a, out_b), (grads_a, grads_b)):
        assert sorted(a) == sorted(b)
        for tname in a:
            assert torch.equal(a[tname], b[tname]), tname
    check(name, compare(name, out_b, grads_b))


@pytest.mark.parametrize("name", ["base", "head", "relu6", "no-out"])
def test_forward_without_grad_is_bit_identical(dev, switches, name):
    """Under torch.no_grad() the node keeps nothing for a backward pass (no V, no rotated kernel transform): same outputs, bit
    for bit, as the training forward."""
    out_a, _ = run_tower(name, dev, switches)
    out_b, _ = run_tower(name, dev, switches, training=False)
    assert sorted(out_a) == sorted(out_b)
    for tname in out_a:
        assert torch.equal(out_a[tname], out_b[tname]), tname
