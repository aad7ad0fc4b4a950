"""The case table of tests/wino_tower_ref.py without a GPU: every case is one the folded tower accepts, every conv of it takes
the planner branch it was picked for (read off the host-only rn_conv3x3_winograd_gn_plan: the library loads without a device,
and the query runs the launches' own chunk_width / width_for / cfill / fill / check_fold under the same environment variables
and product switches), and the table as a whole reaches every branch listed in COVER.  A planner change that moves a case off
its branch fails here and says: pick another shape for that branch.  Three more tests check the reference itself.

What the query shows per conv (csrc/winograd.hip, run_gn_fwd / run_gn_bwd), as a Row of four sides:
  fwd_in    x  -> V   wino_gn_fwd_pre_kernel<W, LoadPlain | LoadGnAct>: always a chunk kernel
  fwd_out   M  -> y   wino_gn_output_kernel<W> where the layer emits statistic rows, else the grid-stride wino_output_kernel<W>
  bwd_in    dy -> .   wino_gn_bwd_pre_kernel<W, LoadGnBwd> where dy is the g of a folded GroupNorm, else wino_bwd_pre_kernel<W>
  bwd_out   M  -> dx  wino_gn_bwd_post_kernel<W, MODE> (and wino_gn_input_kernel<W> where V is rebuilt): always a chunk kernel
c(W, slabs[, LDS | GLOBAL]): a chunk kernel of W channels per thread, `slabs` blocks across the channels, and where its
blocks read statistic rows whether they stage them in LDS or read them from global memory; g(W): a grid-stride kernel."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import wino_tower_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

Row = collections.namedtuple("Row", "fwd_in fwd_out bwd_in bwd_out")
LDS, GLOBAL = "lds", "global"


def c(w, slabs, rows=None):
    return ("chunk", w, slabs, rows)


def g(w):
    return ("grid", w)


def tower(k, w, slabs, grid_w=1, rows=LDS, w0=None, slabs0=None):
    """The rows of k equal tower layers and an output conv: chunk width w / `slabs` on every folded side, w0 / slabs0 on the
    tower's own (not folded) input, the output conv's transforms grid-stride at grid_w."""
    w0, slabs0 = (w if w0 is None else w0), (slabs if slabs0 is None else slabs0)
    first = Row(c(w0, slabs0), c(w, slabs), c(w, slabs, rows), c(w0, slabs0))
    mid = Row(c(w, slabs, rows), c(w, slabs), c(w, slabs, rows), c(w, slabs, rows))
    last = Row(c(w, slabs, rows), g(grid_w), g(grid_w), c(w, slabs, rows))
    return [first] + [mid] * (k - 1) + [last]


# case -> ((tiles, chunks, U is the fragment image), one Row per conv)
EXPECT = {
    # 64 channels at the natural W = 2: two slabs of 32.  (2,19,13) has 5 x 4 tiles per sample (a full chunk and 4 tiles of a second),
    # (1,4,5) 2 tiles, (2,1,2) 1: 40 + 2 + 2 tiles in 4 + 1 + 2 chunks.  36 output channels: grid-stride at the natural W = 1
    "base": ((44, 7, 1), tower(2, 2, 2)),
    "base-gnw4": ((44, 7, 1), tower(2, 4, 1)),                      # one slab of 64
    "base-gnw1": ((44, 7, 1), tower(2, 1, 4)),
    "box36-w1": ((44, 7, 1), tower(2, 2, 2, grid_w=1)),
    "box36-w2": ((44, 7, 1), tower(2, 2, 2, grid_w=2)),
    "box36-w4": ((44, 7, 1), tower(2, 2, 2, grid_w=4)),
    "cls720-w1": ((44, 7, 1), tower(2, 2, 2, grid_w=1)),
    "cls720-w2": ((44, 7, 1), tower(2, 2, 2, grid_w=2)),
    "cls720-w4": ((44, 7, 1), tower(2, 2, 2, grid_w=4)),
    # one group of 64 channels: width_ok(64, 64, 2) is false, W = 4 on every folded side; the tower's input is not folded: W = 2
    "groups1": ((44, 7, 1), tower(2, 4, 1, w0=2, slabs0=2)),
    "groups64": ((42, 5, 1), tower(2, 2, 2)),
    "c128-groups8": ((44, 7, 1), tower(2, 2, 4)),
    "c128-groups4": ((44, 7, 1), tower(2, 2, 4)),
    # 256 channels: 8 slabs of 32 / 4 of 64; 4 + 1 + 1 + 1 tiles per sample, every chunk partly empty
    "head": ((14, 8, 1), tower(4, 2, 8)),
    "head-gnw4": ((14, 8, 1), tower(4, 4, 4)),
    # 64 -> 128 -> 64 -> 72: the two sides of a conv differ in slabs
    "widths": ((44, 7, 1), [Row(c(2, 2), c(2, 4), c(2, 4, LDS), c(2, 2)),
                            Row(c(2, 4, LDS), c(2, 2), c(2, 2, LDS), c(2, 4, LDS)),
                            Row(c(2, 2, LDS), g(1), g(1), c(2, 2, LDS))]),
    # the last tower conv's raw output leaves the node: its output side is grid-stride (64 channels)
    "no-out": ((44, 7, 1), [Row(c(2, 2), c(2, 2), c(2, 2, LDS), c(2, 2)),
                            Row(c(2, 2, LDS), g(1), g(1), c(2, 2, LDS))]),
    "tile2": ((290, 19, 1), tower(2, 2, 2)),                        # 17 x 16 tiles = 17 chunks, + 2 samples x 9 tiles
    # 33 x 33 tiles = 69 chunks per sample: x 16 groups per block (W = 2) = 1104 rows, x 32 (W = 4) = 2208 > 1024; x 8 (W = 1) = 552
    "unstaged": ((2187, 139, 1), tower(2, 2, 2, rows=GLOBAL)),
    "unstaged-gnw4": ((2187, 139, 1), tower(2, 4, 1, rows=GLOBAL)),
    "unstaged-gnw1": ((2187, 139, 1), tower(2, 1, 4)),
    "staged-twin": ((582, 39, 1), tower(2, 2, 2)),                  # tile 4: 17 x 17 tiles = 19 chunks per sample x 16 = 304 rows
    "relu": ((6, 3, 1), tower(2, 2, 2)),
    "relu6": ((5, 2, 1), tower(2, 2, 4)),
    "relu-3-layers": ((14, 3, 1), tower(3, 2, 2)),
    "act-none": ((44, 7, 1), tower(2, 2, 2)),
    "base-fp32": ((44, 7, 0), tower(2, 2, 2)),
    "base-x3": ((44, 7, 0), tower(2, 2, 2)),
    "head-fp32": ((14, 8, 0), tower(4, 2, 8)),
    "head-x3": ((14, 8, 0), tower(4, 2, 8)),
    "base-rebuild-v": ((44, 7, 1), tower(2, 2, 2)),
    "base-pretransform": ((44, 7, 1), tower(2, 2, 2)),
    "base-none-cotangent": ((44, 7, 1), tower(2, 2, 2)),
    "head-rebuild-v": ((14, 8, 1), tower(4, 2, 8)),
    "head-pretransform": ((14, 8, 1), tower(4, 2, 8)),
    "head-none-cotangent": ((14, 8, 1), tower(4, 2, 8)),
}
# every branch the table must reach, by the names _observe() gives them
COVER = (["%s chunk W%d" % (side, w) for side in ("fwd in", "fwd out", "bwd in", "bwd out") for w in (1, 2, 4)] +
         ["fwd grid W%d" % w for w in (1, 2, 4)] + ["bwd grid W%d" % w for w in (1, 2, 4)] +
         ["%s rows %s" % (side, how) for side in ("fwd in", "bwd in", "bwd out") for how in (LDS, GLOBAL)] +
         ["output chunked", "output grid-stride", "dy chunked", "dy plain", "U fp32", "U fragment image", "one slab", "several slabs",
          "partial chunk", "tile 2", "tile 4"])


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


def _side(call, which, grid_w):
    if not getattr(call, which + "_chunked"):
        return g(grid_w)
    rows = {1: LDS, 0: GLOBAL, -1: None}[getattr(call, which + "_staged")]
    return c(getattr(call, which + "_w"), getattr(call, which + "_slabs"), rows)


def _observe(name, monkeypatch, product_mode, bfrag_switch):
    """-> (the case as the plan query sees it, in EXPECT's form; names of the branches it takes)"""
    import _rn
    case = R.CASES[name]
    R.configure(case, monkeypatch, product_mode, bfrag_switch)
    plans = R.layer_plans(case)
    rows, names = [], {"tile %d" % case.tile}
    segs = (_rn.ConvSeg * len(case.levels))()
    for s, (n, h, w) in zip(segs, case.levels):
        s.n, s.h, s.w = n, h, w
    for p, (ci, co) in zip(plans, R.convs(case)):
        assert (p.tiles, p.chunks, p.u_frag) == (plans[0].tiles, plans[0].chunks, p.u_frag)
        assert p.chunks == _rn.lib().rn_wino_gn_rows(segs, len(case.levels), case.tile)
        # a call launches a grid-stride kernel exactly where one of its sides is not chunked, and both calls agree on the sides
        assert (p.fwd.stride_w != 0) == (not p.fwd.out_chunked) and (p.bwd.stride_w != 0) == (not p.bwd.in_chunked)
        assert p.fwd.in_chunked == p.bwd.out_chunked == 1 and p.fwd.out_chunked == p.bwd.in_chunked and p.fwd.out_staged == -1
        for call, ch in ((p.fwd, (ci, co)), (p.bwd, (co, ci))):
            for which, chans in zip(("in", "out"), ch):
                if getattr(call, which + "_chunked"):
                    assert getattr(call, which + "_w") * 16 * getattr(call, which + "_slabs") == chans
        row = Row(_side(p.fwd, "in", 0), _side(p.fwd, "out", p.fwd.stride_w), _side(p.bwd, "in", p.bwd.stride_w), _side(p.bwd, "out", 0))
        rows.append(row)
        for side, s in zip(("fwd in", "fwd out", "bwd in", "bwd out"), row):
            if s[0] == "grid":
                names.add("%s grid W%d" % (side[:3], s[1]))
            else:
                names.add("%s chunk W%d" % (side, s[1]))
                names.add("one slab" if s[2] == 1 else "several slabs")
                if s[3] is not None:
                    names.add("%s rows %s" % (side, s[3]))
        names.add("output chunked" if p.fwd.out_chunked else "output grid-stride")
        names.add("dy chunked" if p.bwd.in_chunked else "dy plain")
        names.add("U fragment image" if p.u_frag else "U fp32")
        if p.partial_chunk:
            names.add("partial chunk")
    u = {p.u_frag for p in plans}
    assert len(u) == 1
    return ((plans[0].tiles, plans[0].chunks, u.pop()), rows), names


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_is_supported_and_takes_its_branch(name, monkeypatch, product_mode, bfrag_switch):
    import ops
    case = R.CASES[name]
    xs, tw, ow, ob = R.make_case(case)
    assert R.grad_names(case) and len(R.grad_names(case)) == len(R.leaves_of(case, xs, tw, ow, ob))
    # ops.wino_tower_ok's conditions on the parameters (it also wants CUDA tensors): whole 64-channel blocks, whole groups per block
    cin = case.cin
    for w, _, _ in tw:
        gr = ops.gn_groups(w.shape[3], case.groups)
        assert w.shape[:3] == (3, 3, cin) and cin % 64 == 0 and w.shape[3] % 64 == 0 and 64 % (w.shape[3] // gr) == 0
        cin = w.shape[3]
    assert ow is None or (ow.shape[:3] == (3, 3, cin) and ow.shape[3] % 4 == 0)
    seen, _ = _observe(name, monkeypatch, product_mode, bfrag_switch)
    assert seen == EXPECT[name], "case %s left its branch: the planner now gives %s -- pick another shape for %s" % (name, seen, EXPECT[name])


def test_table_covers_every_branch(monkeypatch, product_mode, bfrag_switch):
    assert sorted(EXPECT) == sorted(R.CASES)
    names = set()
    for name in R.CASES:
        names |= _observe(name, monkeypatch, product_mode, bfrag_switch)[1]
    missing = [b for b in COVER if b not in names]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


def test_table_shapes():
    """What the planner does not decide but the cases were picked for."""
    import ops
    base, head = R.CASES["base"], R.CASES["head"]
    assert [ops.gn_groups(64, gr) for gr in (1, 32, 64)] == [1, 32, 64] and [ops.gn_groups(128, gr) for gr in (4, 8)] == [4, 8]
    assert base.levels[0][1] % 4 and base.levels[0][2] % 4                      # partial tiles on both edges
    assert min(h * w for _, h, w in R.CASES["groups64"].levels) >= 16           # one channel per group: no group of a single value
    assert head.levels[-1][1:] == (1, 1) and head.cin == 256 and len(head.widths) == 4
    assert R.CASES["no-out"].cout == 0 and R.grad_names(R.CASES["no-out"]) == ["dx0", "dx1", "dx2", "dw0", "dgamma0", "dbeta0", "dw1"]
    # the unstaged case and its twin are the same tensors at the two tiles; two samples behind a first segment
    un, twin = R.CASES["unstaged"], R.CASES["staged-twin"]
    assert R.math_key(un) == R.math_key(twin) and (un.tile, twin.tile) == (2, 4) and un.levels[1][0] == 2
    # the variants and formats share the reference of their plain case
    for name, case in R.CASES.items():
        for stem in ("base", "head"):
            if name.startswith(stem + "-") and case.variant != "none-cotangent" and not name.endswith(("gnw4", "gnw1")):
                assert R.math_key(case) == R.math_key(R.CASES[stem])
    # kinked cases stay small: a margin of 1e-4 is only reachable by a seed search while there are few pre-activations
    for name in KINK_MARGINS:
        assert sum(p.numel() for p in R.pre_activations(R.CASES[name])) <= 30000


def test_plan_query_refuses_what_the_launches_refuse(monkeypatch):
    import _rn
    L = _rn.lib()
    segs = (_rn.ConvSeg * 1)()
    segs[0].n, segs[0].h, segs[0].w = 1, 8, 8
    plan = _rn.WinoGnPlan()
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 64, 4, 32, 32, C.byref(plan)) == 0
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 64, 3, 32, 32, C.byref(plan)) == -1          # tile
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 64, 4, 32, 32, None) == -1
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 96, 64, 4, 0, 32, C.byref(plan)) == -2           # cin % 64
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 128, 128, 4, 1, 1, C.byref(plan)) == -2          # a group wider than a block
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 36, 4, 32, 32, C.byref(plan)) == -2          # 36 channels cannot be folded
    # a forced width that does not hold whole groups is ignored, as in the launches (64 channels per group need W = 4)
    monkeypatch.setenv("RN_WINO_GN_W", "2")
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 64, 4, 1, 1, C.byref(plan)) == 0
    assert (plan.fwd.in_w, plan.fwd.out_w, plan.bwd.in_w, plan.bwd.out_w) == (4, 4, 4, 4)
    assert L.rn_conv3x3_winograd_gn_plan(segs, 1, 64, 64, 4, 0, 1, C.byref(plan)) == 0
    assert (plan.fwd.in_w, plan.fwd.out_w, plan.bwd.in_w, plan.bwd.out_w) == (2, 4, 4, 2)


def test_natural_width_four_is_reached_by_a_documented_batch(monkeypatch):
    """chunk_width gives W = 4 once tiles x (C / 4) >= 256 K: at C = 256 that is 4096 tiles, which 14 images of 512^2 reach (the
    table forces that width through RN_WINO_GN_W on small maps: the same kernels)."""
    import _rn
    L = _rn.lib()
    monkeypatch.delenv("RN_WINO_GN_W", raising=False)
    widths = []
    for n in (12, 14):
        segs = (_rn.ConvSeg * 5)()
        for s, side in zip(segs, (64, 32, 16, 8, 4)):
            s.n, s.h, s.w = n, side, side
        plan = _rn.WinoGnPlan()
        assert L.rn_conv3x3_winograd_gn_plan(segs, 5, 256, 256, 4, 32, 32, C.byref(plan)) == 0
        widths.append((plan.tiles, plan.fwd.in_w, plan.fwd.out_w, plan.bwd.in_w, plan.bwd.out_w))
    assert widths == [(12 * 341, 2, 2, 2, 2), (14 * 341, 4, 4, 4, 4)]


def test_reference_is_the_oracles_chain():
    """tower_ref in fp64 == the chain test_gpu_wino_tower.test_folded_tower_matches_oracle builds out of oracle/tf_ops_ref
    (conv2d_same, group_norm, activation) on that test's parameters, to fp64 rounding: outputs and every gradient."""
    case = R._case([(2, 12, 12), (2, 6, 6), (2, 3, 3)], cout=72, seed=3)
    xs, tw, ow, ob = R.make_case(case)
    rng = np.random.default_rng(3)                                                # (that test's first draw, to show the parameters are its)
    assert np.array_equal(tw[0][0].numpy(), (rng.standard_normal((3, 3, 64, 64)) * 0.05).astype(np.float32))
    got_out, got_grads = R.run_ref(case, torch.float64)

    def leaf(t):
        return t.double().requires_grad_(True)

    xs = [leaf(x) for x in xs]
    tw = [tuple(leaf(t) for t in layer) for layer in tw]
    ow, ob = leaf(ow), leaf(ob)
    outs = []
    for x in xs:
        h = x
        for w, gam, bet in tw:
            h = T.activation(T.group_norm(T.conv2d_same(h, w, 1), gam, bet, 32), "elu")
        outs.append(T.conv2d_same(h, ow, 1, bias=ob))
    grads = torch.autograd.grad(outs, R.leaves_of(case, xs, tw, ow, ob), [c_.double() for c_ in R.make_cotangents(case)])
    for i, o in enumerate(outs):
        assert rel_err(got_out["y%d" % i], o.detach().numpy()) < 1e-13
    for name, gr in zip(R.grad_names(case), grads):
        assert rel_err(got_grads[name], gr.numpy()) < 1e-12, name


# seed -> measured margin, pinned so that a change of the generator is noticed
KINK_MARGINS = {"relu": 8.646e-4, "relu6": 6.339e-4, "relu-3-layers": 1.230e-4}


@pytest.mark.parametrize("name", list(KINK_MARGINS))
def test_no_preactivation_sits_on_a_kink(name):
    """relu / relu6: the derivative jumps at 0 (and 6), so an element within rounding of a kink may differ by O(1) between two
    correct evaluations.  The GroupNorm output is O(1) and two correct fp32 evaluations of the forward pass agree to 2e-5 of the
    maximum (tests/test_gpu_wino_tower.py): each case's seed is chosen so that, in the fp64 reference, no pre-activation is
    within KINK_MARGIN = 1e-4 of a kink -- five times that distance."""
    case = R.CASES[name]
    assert case.act in R.KINKS
    margin = R.kink_margin(case)
    assert margin > R.KINK_MARGIN, margin
    assert abs(margin / KINK_MARGINS[name] - 1) < 1e-3, margin


def test_relu6_case_uses_both_kinks():
    """gamma is scaled to about 4 so that the upper kink is in use: at least 1 % of the pre-activations lie above 6 and at
    least 1 % below 0."""
    p = torch.cat([q.flatten() for q in R.pre_activations(R.CASES["relu6"])])
    assert float((p > 6).double().mean()) >= 0.01 and float((p < 0).double().mean()) >= 0.01
    assert [name for name, case in R.CASES.items() if case.act in R.KINKS] == list(KINK_MARGINS)
