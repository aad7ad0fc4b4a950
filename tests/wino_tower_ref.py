"""The GroupNorm-folded Winograd tower (ops.wino_tower / rn_conv3x3_winograd_gn*) restated in plain torch, in any dtype, for
the tests, and the table of cases that tests/test_wino_tower_cases_cpu.py and tests/test_gpu_wino_tower_cases.py share.

`tower_ref` is written from ops.wino_tower's contract (reference retinanet.py:37-71,85-115, normalization.py:20-35), not from
the kernels: per level, with a = the level's input,

    a <- act(GN(conv3x3_same(a, w_l)))        for every layer l of the tower
    out = conv3x3_same(a, w_out) + b_out

and without an output conv the RAW product of the last layer's conv (its GroupNorm is not the node's).  The conv is a direct
3 x 3 / pad 1 convolution on NCHW views, the GroupNorm takes mean and biased variance per sample and group over (H, W, C / G)
with G = ops.gn_groups(C, groups).  Gradients come from torch.autograd in the working dtype.

A case says WHAT is computed (levels, widths, groups, activation, seed, gamma scale, which cotangent is missing) and HOW the
library is asked to compute it (tile, forced kernel widths, product format, variant); the reference depends on the first part
only (`math_key`) and is computed once per process for every distinct one.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple("Case", "levels cin widths cout groups act tile seed gamma_scale gn_w wino_w product variant")
EPS = 1e-5
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0)}
KINK_MARGIN = 1e-4
# the product kernels' operand formats: (rn_set_product_mode, rn_set_x3_bfrag)
PRODUCTS = {"x3-frag": (1, 1), "x3": (1, 0), "fp32": (0, 1)}
# rebuild-v       the forward pass keeps no V (ops.WINOGRAD_WGRAD off): the backward pass rebuilds it through the folded loader
# pretransform    U / Urot made ahead of the layers (ops.WinoPretransform -> ops.WINO_PRE)
# none-cotangent  the cotangent of the LAST level is None (the node zero-fills it; the reference uses zeros)
VARIANTS = (None, "rebuild-v", "pretransform", "none-cotangent")


def _case(levels, cin=64, widths=(64, 64), cout=36, groups=32, act="elu", tile=4, seed=0, gamma_scale=1.0, gn_w=None, wino_w=None,
          product="x3-frag", variant=None):
    assert product in PRODUCTS and variant in VARIANTS
    return Case(tuple(levels), cin, tuple(widths), cout, groups, act, tile, seed, gamma_scale, gn_w, wino_w, product, variant)


BASE = [(2, 19, 13), (1, 4, 5), (2, 1, 2)]              # 20 tiles per sample (a full chunk + 4 tiles), partial tiles on both edges
HEAD = [(2, 8, 8), (2, 4, 4), (2, 2, 2), (2, 1, 1)]     # the box subnet's width on a small pyramid, incl. the 1 x 1 level
UNSTAGED = [(1, 5, 5), (2, 66, 66)]                     # tile 2: 33^2 tiles = 69 chunks per sample; x 16 groups per block > 1024 rows
HEAD_KW = dict(cin=256, widths=(256, 256, 256, 256))

# levels (n, h, w); cin; the tower layers' output widths; the output conv's width (0: none); the groups ARGUMENT
# (ops.gn_groups resolves it per width); activation; Winograd tile; seed; forced RN_WINO_GN_W / RN_WINO_W; product format;
# variant.  What each case is for: tests/test_wino_tower_cases_cpu.py (EXPECT) names the planner branches it takes.
CASES = collections.OrderedDict([
    ("base", _case(BASE)),
    ("base-gnw4", _case(BASE, gn_w=4)),
    ("base-gnw1", _case(BASE, gn_w=1)),
    # the grid-stride output transform and the plain dy transforms of the output conv, at every width
    ("box36-w1", _case(BASE, wino_w=1)),
    ("box36-w2", _case(BASE, wino_w=2)),
    ("box36-w4", _case(BASE, wino_w=4)),
    ("cls720-w1", _case(BASE, cout=720, wino_w=1)),
    ("cls720-w2", _case(BASE, cout=720, wino_w=2)),
    ("cls720-w4", _case(BASE, cout=720, wino_w=4)),
    # 64 / 1 / 16 / 32 channels per group (groups=64: every map has at least 4 x 4 pixels, so no group has a single value)
    ("groups1", _case(BASE, groups=1)),
    ("groups64", _case(BASE[:2], groups=64)),
    ("c128-groups8", _case(BASE, cin=128, widths=(128, 128), groups=8)),
    ("c128-groups4", _case(BASE, cin=128, widths=(128, 128), groups=4)),
    ("head", _case(HEAD, **HEAD_KW)),
    ("head-gnw4", _case(HEAD, gn_w=4, **HEAD_KW)),
    ("widths", _case(BASE, widths=(128, 64), cout=72)),
    ("no-out", _case(BASE, cout=0)),
    ("tile2", _case([(1, 33, 31), (2, 6, 6)], tile=2)),
    ("unstaged", _case(UNSTAGED, tile=2)),
    ("unstaged-gnw4", _case(UNSTAGED, tile=2, gn_w=4)),
    ("unstaged-gnw1", _case(UNSTAGED, tile=2, gn_w=1)),
    ("staged-twin", _case(UNSTAGED, tile=4)),
    # relu / relu6: `seed` is chosen so that no pre-activation lies within KINK_MARGIN of a kink (test_wino_tower_cases_cpu.py)
    ("relu", _case([(1, 5, 6), (2, 3, 3)], act="relu", seed=9)),
    ("relu6", _case([(1, 6, 5), (1, 2, 2)], cin=128, widths=(128, 128), act="relu6", gamma_scale=4.0, seed=1)),
    ("relu-3-layers", _case([(2, 9, 7), (1, 4, 5)], widths=(64, 64, 64), act="relu", seed=1)),
    ("act-none", _case(BASE, act=None)),
    ("base-fp32", _case(BASE, product="fp32")),
    ("base-x3", _case(BASE, product="x3")),
    ("head-fp32", _case(HEAD, product="fp32", **HEAD_KW)),
    ("head-x3", _case(HEAD, product="x3", **HEAD_KW)),
    ("base-rebuild-v", _case(BASE, variant="rebuild-v")),
    ("base-pretransform", _case(BASE, variant="pretransform")),
    ("base-none-cotangent", _case(BASE, variant="none-cotangent")),
    ("head-rebuild-v", _case(HEAD, variant="rebuild-v", **HEAD_KW)),
    ("head-pretransform", _case(HEAD, variant="pretransform", **HEAD_KW)),
    ("head-none-cotangent", _case(HEAD, variant="none-cotangent", **HEAD_KW)),
])


def configure(case, monkeypatch, product_mode, bfrag_switch):
    """Put the library and ops into the state the case asks for; the three arguments are pytest's monkeypatch and the
    product_mode / bfrag_switch fixtures of tests/test_gpu_x3.py (which restore what they change).  The library reads
    RN_WINO_GN_W / RN_WINO_W at every call."""
    import ops
    for var, val in (("RN_WINO_GN_W", case.gn_w), ("RN_WINO_W", case.wino_w)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    monkeypatch.setattr(ops, "WINOGRAD_TILE", case.tile)
    mode, frag = PRODUCTS[case.product]
    product_mode(mode)
    bfrag_switch(frag)


def layer_plans(case):
    """rn_conv3x3_winograd_gn_plan of every conv of the case, as ops._WinoTower calls them, under the CURRENT environment
    and switches (configure() first) -> [_rn.WinoGnPlan]."""
    import ctypes as C
    import _rn
    import ops
    L = _rn.lib()
    segs = (_rn.ConvSeg * len(case.levels))()
    for s, (n, h, w) in zip(segs, case.levels):
        s.n, s.h, s.w = n, h, w
    k = len(case.widths)
    nfold = k if case.cout else k - 1
    plans = []
    for i, (ci, co) in enumerate(convs(case)):
        plan = _rn.WinoGnPlan()
        _rn.check(L.rn_conv3x3_winograd_gn_plan(segs, len(case.levels), ci, co, case.tile, ops.gn_groups(ci, case.groups) if i > 0 else 0,
                                                ops.gn_groups(co, case.groups) if i < nfold else 0, C.byref(plan)), "rn_conv3x3_winograd_gn_plan")
        plans.append(plan)
    return plans


def convs(case):
    """[(cin, cout)] of every conv of the case: the tower's layers, then the output conv if there is one."""
    chans = (case.cin,) + case.widths + ((case.cout,) if case.cout else ())
    return list(zip(chans[:-1], chans[1:]))


def math_key(case):
    """The part of a case its values depend on."""
    return case._replace(tile=0, gn_w=None, wino_w=None, product="x3-frag", variant="none-cotangent" if case.variant == "none-cotangent" else None)


def make_case(case):
    """(xs, tower, out_w, out_b) as fp32 CPU tensors from ONE numpy generator, drawn in the order and with the scales of
    test_gpu_wino_tower._params: per layer w = 0.05 N, gamma = gamma_scale (1 + 0.3 N), beta = 0.2 N; w_out = 0.05 N,
    b_out = 0.1 N; then the levels' inputs N(0, 1)."""
    rng = np.random.default_rng(case.seed)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))

    tower, c = [], case.cin
    for co in case.widths:
        w = t(rng.standard_normal((3, 3, c, co)) * 0.05)
        g = t(case.gamma_scale * (1 + 0.3 * rng.standard_normal(co)))
        b = t(0.2 * rng.standard_normal(co))
        tower.append((w, g, b))
        c = co
    ow = ob = None
    if case.cout:
        ow = t(rng.standard_normal((3, 3, c, case.cout)) * 0.05)
        ob = t(0.1 * rng.standard_normal(case.cout))
    xs = [t(rng.standard_normal((n, h, w, case.cin))) for n, h, w in case.levels]
    return xs, tower, ow, ob


def make_cotangents(case):
    """N(0, 1) cotangents of every level's output (fp32, from a generator of their own); None for the last level of a
    none-cotangent case."""
    rng = np.random.default_rng(5000 + case.seed)
    c = case.cout if case.cout else case.widths[-1]
    cot = [torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32)) for n, h, w in case.levels]
    if case.variant == "none-cotangent":
        cot[-1] = None
    return cot


def conv3x3_same(x, w, bias=None):
    """3 x 3 / stride 1 SAME convolution of NHWC x with HWIO w: F.conv2d on NCHW views, one zero pixel all round."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), bias=bias, stride=1, padding=1)
    return y.permute(0, 2, 3, 1)


def group_norm(y, gamma, beta, groups, eps=EPS):
    """Mean and BIASED variance per (sample, group) over (H, W, C / G), eps inside the root, per-channel gamma / beta."""
    n, h, w, c = y.shape
    yg = y.reshape(n, h * w, groups, c // groups)
    mean = yg.mean(dim=(1, 3), keepdim=True)
    var = ((yg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    return ((yg - mean) * torch.rsqrt(var + eps)).reshape(n, h, w, c) * gamma + beta


def act_fn(p, act):
    if act is None:
        return p
    if act == "elu":
        return torch.where(p > 0, p, torch.expm1(torch.clamp(p, max=0.0)))
    if act == "relu":
        return torch.clamp(p, min=0.0)
    if act == "relu6":
        return torch.clamp(p, min=0.0, max=6.0)
    raise ValueError(act)


def tower_ref(xs, tower, ow, ob, groups_arg, act, pre=None):
    """-> the list of the levels' outputs, in the dtype of the arguments.  pre: a list that receives every pre-activation
    GN(conv(a, w_l))."""
    import ops
    outs = []
    for x in xs:
        a = x
        for i, (w, g, b) in enumerate(tower):
            a = conv3x3_same(a, w)
            if ow is None and i == len(tower) - 1:
                break
            p = group_norm(a, g, b, ops.gn_groups(w.shape[3], groups_arg))
            if pre is not None:
                pre.append(p)
            a = act_fn(p, act)
        outs.append(conv3x3_same(a, ow, ob) if ow is not None else a)
    return outs


def grad_names(case):
    """Names of the gradients in leaf order: the levels' inputs, every layer's (w, gamma, beta), the output conv's (w, b).
    Without an output conv the last layer's GroupNorm is not part of the node: that layer has a kernel gradient only."""
    k = len(case.widths)
    names = ["dx%d" % i for i in range(len(case.levels))]
    for l in range(k):
        names += ["dw%d" % l] + (["dgamma%d" % l, "dbeta%d" % l] if (case.cout or l < k - 1) else [])
    return names + (["dw_out", "db_out"] if case.cout else [])


def leaves_of(case, xs, tower, ow, ob):
    k = len(case.widths)
    out = list(xs)
    for l, layer in enumerate(tower):
        out += list(layer) if (case.cout or l < k - 1) else [layer[0]]
    return out + ([ow, ob] if case.cout else [])


def run_ref(case, dtype):
    """The case evaluated by tower_ref in `dtype`, forward and backward under make_cotangents: ({output name: array},
    {gradient name: array}).  Outputs: "y<i>" per level; gradients: grad_names()."""
    xs, tower, ow, ob = make_case(case)

    def leaf(t):
        return t.to(dtype).requires_grad_(True)

    xs = [leaf(x) for x in xs]
    tower = [tuple(leaf(t) for t in layer) for layer in tower]
    ow, ob = (leaf(ow), leaf(ob)) if case.cout else (None, None)
    outs = tower_ref(xs, tower, ow, ob, case.groups, case.act)
    cot = [torch.zeros_like(o) if c is None else c.to(dtype) for o, c in zip(outs, make_cotangents(case))]
    grads = torch.autograd.grad(outs, leaves_of(case, xs, tower, ow, ob), cot)
    out = {"y%d" % i: o.detach().contiguous().numpy() for i, o in enumerate(outs)}
    return out, {k: g.contiguous().numpy() for k, g in zip(grad_names(case), grads)}


@functools.lru_cache(maxsize=None)
def _reference(key, dtype):
    out, grads = run_ref(key, dtype)
    for a in list(out.values()) + list(grads.values()):
        a.setflags(write=False)
    return out, grads


def reference(name, dtype):
    """run_ref of CASES[name], computed once per process for every distinct math_key and shared by the tests: treat the
    arrays as read-only."""
    return _reference(math_key(CASES[name]), dtype)


def pre_activations(case):
    """Every pre-activation of the case in the fp64 reference (a list of tensors)."""
    xs, tower, ow, ob = make_case(case)
    pre = []
    with torch.no_grad():
        tower_ref([x.double() for x in xs], [tuple(t.double() for t in layer) for layer in tower],
                  ow.double() if case.cout else None, ob.double() if case.cout else None, case.groups, case.act, pre=pre)
    return pre


def kink_margin(case):
    """Smallest distance of any pre-activation of the case (fp64 reference) from a kink of its activation."""
    return min(float((p - k).abs().min()) for p in pre_activations(case) for k in KINKS[case.act])
