"""Reference and case table for the GroupNorm kernels (csrc/group_norm.hip: rn_group_norm_fwd / rn_group_norm_bwd).

The reference is a plain torch evaluation, in a chosen dtype, of
    y = dropout(act(GN(x))) + residual                      (MobileNetV2 order)
    y = dropout(act(GN(x) + residual))                      (act_after_residual, ResNeXt order)
per segment with shared gamma / beta: two-pass statistics (mean, then the mean of the squared deviations), eps inside the
sqrt.  It returns every segment's y, the per-(sample, group) mean and rstd, and -- for fixed cotangents -- the gradients of
every x, every residual, gamma and beta.  A dropout mask cannot be reproduced on the host: the reference takes it as an
argument (the GPU test reads it off the kernel's own output, y != 0, which is why dropout cases use act None or elu and no
residual: a kept element is then not zero).

CASES names one shape per branch of the dispatch (`decide` in group_norm.hip, read through the host-only rn_group_norm_plan);
tests/test_gn_cases_cpu.py proves on the CPU that every case takes the branch it was picked for and that the table reaches
every branch, tests/test_gpu_gn_cases.py runs the table against this reference in fp64."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

EPS = 1e-5
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0)}
KINK_MARGIN = 1e-4
SWITCHES = ("RN_GN_NO_SLICE", "RN_GN_NO_ROWS", "RN_GN_NO_COOP", "RN_GN_SLICE_WC")

Case = collections.namedtuple(
    "Case", "segs c groups act res aar drop x_ld dx_ld dx_acc sync env producer offset seed gamma_scale defer")


def _case(segs, c, groups=32, act="elu", res=False, aar=False, drop=0.0, x_ld=0, dx_ld=0, dx_acc=False, sync=False, env=(),
          producer=None, offset=0.25, seed=0, gamma_scale=1.0, defer=False):
    """segs: (n, h, w) per segment.  x_ld / dx_ld: leading dimensions of the wider buffers x / dx live in (0: dense), dx_acc:
    dx += .  sync: a grid-resident sync region is passed.  env: the RN_GN_* switches set for the call.  producer:
    (rows_per_sample, per_group) of statistic rows the test computes from x and passes as rn_gn_params.stat_rows.  offset:
    mean / std of x.  defer: the backward call records its row reductions in a defer list (flushed by the test)."""
    return Case(tuple(segs), c, groups, act, res, aar, drop, x_ld, dx_ld, dx_acc, sync, tuple(env), producer, offset, seed,
                gamma_scale, defer)


NS, NR, NC = "RN_GN_NO_SLICE", "RN_GN_NO_ROWS", "RN_GN_NO_COOP"
WC4 = ("RN_GN_SLICE_WC", "4")   # tuning aid: blocks of 4 channels on a small map (the narrow slice kernel without 2 M elements)


def _env(*names):
    return tuple(n if isinstance(n, tuple) else (n, "1") for n in names)


PYRAMID = [(2, 16, 16), (2, 8, 8), (2, 4, 4), (2, 2, 2)]
CASES = collections.OrderedDict([
    # ---------------------------------------------------------------- slice-resident (two-pass statistics in registers)
    ("slice-wc8-r32", _case([(2, 36, 36)], 64)),                                     # cpg 2: four groups per block
    ("slice-r2", _case([(2, 9, 7)], 256, res=True)),
    ("slice-r4-pyramid", _case(PYRAMID, 256, act=None)),                             # smallest level: 4 pixels, R = 4
    ("slice-r8-2seg", _case([(2, 20, 20), (2, 10, 10)], 64, res=True, aar=True)),
    ("slice-r16", _case([(2, 30, 30)], 64, drop=0.25)),
    ("slice-wc64-c2048", _case([(2, 5, 6)], 2048, act=None, drop=0.25)),
    ("slice-wc9-c144", _case([(2, 9, 7)], 144, groups=16)),                          # 512 % 9 != 0: idle lanes
    ("slice-wc30-c960", _case([(2, 9, 7)], 960)),
    ("slice-wc52-c1664", _case([(2, 5, 6)], 1664)),
    ("slice-group64", _case([(2, 9, 7)], 64, groups=1)),                             # one group of 64 channels
    ("slice-relu", _case([(2, 9, 7)], 64, act="relu", seed=1)),
    ("slice-relu6-aar", _case([(2, 9, 7)], 64, act="relu6", res=True, aar=True, gamma_scale=4.0, seed=0)),
    ("slice-offset", _case([(2, 36, 36)], 64, offset=16.0)),                         # twin of slice-wc8-r32
    # ---------------------------------------------------------------- narrow slice (no sync region: the grid-resident path declines)
    ("narrow-wc4", _case([(2, 56, 56)], 32, act=None)),                              # per-channel groups
    ("narrow-wc6", _case([(2, 48, 48)], 96, res=True)),
    ("narrow-relu", _case([(2, 10, 10)], 32, act="relu", env=_env(WC4), seed=0)),
    ("narrow-relu6-aar", _case([(2, 10, 10)], 32, act="relu6", res=True, aar=True, env=_env(WC4), gamma_scale=4.0, seed=1)),
    ("narrow-offset", _case([(2, 56, 56)], 32, act=None, offset=16.0)),              # twin of narrow-wc4
    ("narrow-drop", _case([(2, 20, 20), (2, 5, 5)], 32, drop=0.25, env=_env(WC4))),
    # ---------------------------------------------------------------- grid-resident (sync region passed)
    ("coop-r4", _case([(2, 9, 7)], 256, sync=True, env=_env(NS), res=True)),         # 4 blocks
    ("coop-r4-pyramid", _case(PYRAMID, 256, act=None, sync=True, env=_env(NS))),
    ("coop-r16", _case([(2, 80, 80)], 256, sync=True)),                              # 100 blocks; the slice kernels decline (hw > 2048)
    ("coop-c96", _case([(2, 20, 18)], 96, sync=True, env=_env(NS), drop=0.25)),      # 512 % 24 != 0
    ("coop-c144", _case([(2, 20, 18)], 144, groups=16, sync=True, env=_env(NS), res=True, aar=True)),
    ("coop-groups256", _case([(2, 9, 7)], 256, groups=256, sync=True, env=_env(NS))),  # 2 x groups = the block width: one pass, no row lanes
    ("coop-groups512", _case([(2, 9, 7)], 1024, groups=512, sync=True, env=_env(NS))),  # 2 x groups = 1024: two passes in coop_group_totals
    ("coop-relu", _case([(2, 9, 7)], 64, act="relu", sync=True, env=_env(NS), seed=1)),
    ("coop-relu6-aar", _case([(2, 9, 7)], 64, act="relu6", res=True, aar=True, sync=True, env=_env(NS), gamma_scale=4.0, seed=0)),
    ("coop-offset", _case([(2, 9, 7)], 256, sync=True, env=_env(NS), res=True, offset=16.0)),   # twin of coop-r4
    ("coop-r16-offset", _case([(2, 80, 80)], 256, sync=True, offset=16.0)),                      # twin of coop-r16
    # ---------------------------------------------------------------- rows, self-made (gn_rows_partial_kernel + apply rows)
    ("rows-sw32", _case([(2, 20, 18), (2, 3, 3)], 64, env=_env(NS), res=True)),
    ("rows-sw24", _case([(2, 20, 18)], 24, groups=24, act=None, env=_env(NS))),               # slab = all of c
    ("rows-sw36", _case([(2, 20, 18)], 144, groups=16, env=_env(NS), drop=0.25)),
    ("rows-sw48", _case([(2, 20, 18)], 96, env=_env(NS), res=True, aar=True)),
    ("rows-sw60", _case([(2, 9, 7)], 960, env=_env(NS))),
    ("rows-fwd16-bwd8", _case([(2, 112, 112)], 32, env=_env(NC))),                   # per-channel groups; apply R 16 / 8
    ("rows-fwd8", _case([(2, 96, 96)], 32, act=None)),
    ("rows-x-ld", _case([(2, 20, 18)], 64, env=_env(NS), x_ld=96)),                  # channel prefix of a wider buffer
    ("rows-dx-ld", _case([(2, 20, 18)], 64, env=_env(NS), x_ld=96, dx_ld=96)),
    ("rows-dx-acc", _case([(2, 20, 18)], 64, env=_env(NS), x_ld=96, dx_ld=96, dx_acc=True, res=True)),
    ("rows-relu", _case([(2, 9, 7)], 64, act="relu", env=_env(NS), seed=1)),
    ("rows-relu6-aar", _case([(2, 9, 7)], 64, act="relu6", res=True, aar=True, env=_env(NS), gamma_scale=4.0, seed=0)),
    ("rows-offset", _case([(2, 20, 18), (2, 3, 3)], 64, env=_env(NS), res=True, offset=16.0)),   # twin of rows-sw32
    ("rows-fwd8-offset", _case([(2, 96, 96)], 32, act=None, offset=16.0)),                       # twin of rows-fwd8
    # ---------------------------------------------------------------- producer rows (computed by the test from x)
    ("prod-chan-1", _case([(2, 9, 7)], 64, producer=(1, 0), res=True)),
    ("prod-chan-5", _case([(2, 20, 18)], 144, groups=16, producer=(5, 0), act=None)),
    ("prod-chan-72", _case([(2, 96, 96)], 64, producer=(72, 0))),                    # 72 x 32 entries > 2048: 48-chunk cap, R 8
    ("prod-chan-r16", _case([(1, 112, 112)], 64, producer=(72, 0), act=None)),         # 12544 pixels > 48 x 32 x 8: R 16
    ("prod-group-1", _case([(2, 20, 18)], 96, producer=(1, 1), drop=0.25)),
    ("prod-group-7", _case([(2, 20, 18)], 256, producer=(7, 1), res=True, aar=True)),
    ("prod-relu", _case([(2, 9, 7)], 64, act="relu", producer=(3, 0), seed=1)),
    ("prod-relu6-aar", _case([(2, 9, 7)], 64, act="relu6", res=True, aar=True, producer=(3, 1), gamma_scale=4.0, seed=0)),
    ("prod-offset", _case([(2, 20, 18)], 144, groups=16, producer=(5, 0), act=None, offset=16.0)),  # twin of prod-chan-5
    # ---------------------------------------------------------------- three kernels (partial, finalize, apply)
    ("three-c2048", _case([(2, 5, 6)], 2048, env=_env(NS, NR))),                     # several channel passes
    ("three-group256", _case([(2, 9, 7), (2, 3, 3)], 256, groups=1, res=True)),      # cpg > 128: every other path declines
    ("three-sigmoid", _case([(2, 20, 18)], 96, act="sigmoid")),
    ("three-x-ld", _case([(2, 20, 18)], 64, env=_env(NR), x_ld=96, act=None)),
    ("three-dx-acc", _case([(2, 20, 18)], 64, env=_env(NR), x_ld=96, dx_ld=128, dx_acc=True, res=True, aar=True)),
    ("three-dx-ld", _case([(2, 20, 18)], 64, env=_env(NR), dx_ld=128)),
    ("three-defer", _case([(2, 20, 18), (2, 3, 3)], 96, env=_env(NS, NR), defer=True)),
    ("three-drop", _case([(2, 20, 18)], 96, env=_env(NS, NR), drop=0.25)),
    ("three-relu", _case([(2, 9, 7)], 64, act="relu", env=_env(NS, NR), seed=1)),
    ("three-relu6-aar", _case([(2, 9, 7)], 64, act="relu6", res=True, aar=True, env=_env(NS, NR), gamma_scale=4.0, seed=0)),
    ("three-offset", _case([(2, 9, 7), (2, 3, 3)], 256, groups=1, res=True, offset=16.0)),       # twin of three-group256
    ("slice-defer", _case([(2, 9, 7)], 256, res=True, defer=True)),                  # the slice rows through rn_reduce_rows
])
# the arithmetic family a case's statistics belong to (one RATIO_BOUND each)
TWO_PASS, SUM_SQ, SUM_SQ_OFFSET = "two-pass", "sum-of-squares", "sum-of-squares, offset data"
OFFSET_TWINS = {"slice-offset": "slice-wc8-r32", "narrow-offset": "narrow-wc4", "coop-offset": "coop-r4", "coop-r16-offset": "coop-r16", "rows-offset": "rows-sw32",
                "rows-fwd8-offset": "rows-fwd8", "prod-offset": "prod-chan-5", "three-offset": "three-group256"}
# one case per path for the determinism test, and the paths a dropout shape is run through for the mask comparison
ONE_PER_PATH = ["slice-r16", "narrow-drop", "coop-c96", "rows-sw36", "prod-group-1", "three-drop"]


def family(name):
    if name.startswith(("slice", "narrow")):
        return TWO_PASS
    return SUM_SQ_OFFSET if CASES[name].offset >= 8 else SUM_SQ


def cpg(case):
    return case.c // case.groups


def elements(case):
    return sum(n * h * w for n, h, w in case.segs) * case.c


def math_key(case):
    """Cases with equal keys share data and reference (dropout cases excepted: their mask comes from the run)."""
    return (case.segs, case.c, case.groups, case.act, case.res, case.aar, case.offset, case.seed, case.gamma_scale)


@functools.lru_cache(maxsize=None)
def _make(key):
    segs, c, groups, act, res, aar, offset, seed, gamma_scale = key
    rng = np.random.default_rng(1000 + seed)
    gamma = (gamma_scale * (1 + 0.3 * rng.standard_normal(c))).astype(np.float32)
    beta = (0.2 * rng.standard_normal(c)).astype(np.float32)
    xs = [((rng.standard_normal((n, h, w, c)) + offset) * 2).astype(np.float32) for n, h, w in segs]
    ress = [rng.standard_normal((n, h, w, c)).astype(np.float32) if res else None for n, h, w in segs]
    dys = [rng.standard_normal((n, h, w, c)).astype(np.float32) for n, h, w in segs]
    t = torch.from_numpy
    return ([t(x) for x in xs], [t(r) if r is not None else None for r in ress], t(gamma), t(beta), [t(d) for d in dys])


def make_case(case):
    """-> (xs, residuals (or None each), gamma, beta, cotangents): fp32 CPU tensors, NHWC.  Treat as read-only (shared)."""
    return _make(math_key(case))


def _act(z, kind):
    if kind is None:
        return z
    if kind == "elu":
        return torch.nn.functional.elu(z)
    if kind == "relu":
        return torch.relu(z)
    if kind == "relu6":
        return torch.clamp(z, 0.0, 6.0)
    if kind == "sigmoid":
        return torch.sigmoid(z)
    raise ValueError(kind)


def _normalise(x, gamma, beta, groups):
    n, h, w, c = x.shape
    xg = x.reshape(n, h * w, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)          # second pass over the deviations
    rstd = 1.0 / torch.sqrt(var + EPS)
    z = ((xg - mean) * rstd).reshape(n, h, w, c) * gamma + beta
    return z, mean.reshape(n, groups), rstd.reshape(n, groups)


def run_ref(case, dtype, masks=None):
    """-> dict of numpy arrays: y<i>, mean<i>, rstd<i>, dx<i>, dres<i> (residual cases), dgamma, dbeta.  masks: per segment
    the boolean keep mask of the dropout (required when case.drop > 0)."""
    if masks is None and not case.drop:
        return _run_ref_cached(math_key(case), dtype)
    return _run_ref(case, dtype, masks)


@functools.lru_cache(maxsize=None)
def _run_ref_cached(key, dtype):
    """Cases that share data (they differ in switches, sync, views or producer rows only) share one reference."""
    segs, c, groups, act, res, aar, offset, seed, gamma_scale = key
    return _run_ref(_case(segs, c, groups, act, res, aar, offset=offset, seed=seed, gamma_scale=gamma_scale), dtype, None)


def _run_ref(case, dtype, masks):
    xs, ress, gamma, beta, dys = make_case(case)
    assert (masks is not None) == (case.drop > 0)
    xs = [x.to(dtype).requires_grad_(True) for x in xs]
    ress = [r.to(dtype).requires_grad_(True) if r is not None else None for r in ress]
    gamma, beta = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    out, ys = {}, []
    for i, (x, r) in enumerate(zip(xs, ress)):
        z, mean, rstd = _normalise(x, gamma, beta, case.groups)
        t = _act(z + r if (case.aar and r is not None) else z, case.act)
        if case.drop:
            t = t * masks[i].to(dtype) / torch.tensor(1.0 - case.drop, dtype=dtype)
        y = t if (case.aar or r is None) else t + r
        ys.append(y)
        out["y%d" % i], out["mean%d" % i], out["rstd%d" % i] = y.detach().numpy(), mean.detach().numpy(), rstd.detach().numpy()
    leaves = xs + [r for r in ress if r is not None] + [gamma, beta]
    grads = list(torch.autograd.grad(ys, leaves, [d.to(dtype) for d in dys]))
    for i in range(len(xs)):
        out["dx%d" % i] = grads.pop(0).numpy()
    for i, r in enumerate(ress):
        if r is not None:
            out["dres%d" % i] = grads.pop(0).numpy()
    out["dgamma"], out["dbeta"] = grads[0].numpy(), grads[1].numpy()
    return out


def pre_activations(case):
    """The activation's arguments in the fp64 reference: GN(x), or GN(x) + residual with act_after_residual."""
    xs, ress, gamma, beta, _ = make_case(case)
    pre = []
    for x, r in zip(xs, ress):
        z = _normalise(x.double(), gamma.double(), beta.double(), case.groups)[0]
        pre.append(z + r.double() if (case.aar and r is not None) else z)
    return pre


def kink_margin(case):
    p = torch.cat([q.flatten() for q in pre_activations(case)])
    return min(float((p - k).abs().min()) for k in KINKS[case.act])


def producer_rows(case, xs):
    """The statistic rows a producer would have written for the case's single x, in the rn_gn_rows layout
    [n][rows_per_sample][width] pairs of fp32 (sum, sum of squares): the sample's pixels cut into rows_per_sample contiguous
    runs, width = channels (per_group 0) or groups (per_group 1).  Summed in fp64 and rounded once."""
    rps, per_group = case.producer
    x = xs[0].double()
    n, h, w, c = x.shape
    x = x.reshape(n, h * w, c)
    bounds = np.linspace(0, h * w, rps + 1).round().astype(int)
    rows = torch.zeros((n, rps, case.groups if per_group else c, 2), dtype=torch.float64)
    for r in range(rps):
        part = x[:, bounds[r]:bounds[r + 1]]
        s, q = part.sum(1), (part * part).sum(1)
        if per_group:
            s, q = s.reshape(n, case.groups, -1).sum(2), q.reshape(n, case.groups, -1).sum(2)
        rows[:, r, :, 0], rows[:, r, :, 1] = s, q
    return rows.float().contiguous()


# --------------------------------------------------------------------------------------------------------- the plan query
def configure(case, monkeypatch):
    """The RN_GN_* switches of the case (read by the library at every call) and nothing else."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env:
        monkeypatch.setenv(name, value)


_HOST_WORD = C.c_uint64(0)   # something non-NULL for the pointers the query only compares with NULL


def host_call(case, sync=None, rows_ptr=None):
    """-> (segs, nseg, params, keep-alive): the ctypes arguments of the case with NULL data pointers (sync / rows: given
    addresses, or a host word that stands for 'present')."""
    import _rn
    segs = (_rn.GnSeg * len(case.segs))()
    for s, (n, h, w) in zip(segs, case.segs):
        s.n, s.hw, s.x_ld, s.dx_ld, s.dx_accumulate = n, h * w, case.x_ld, case.dx_ld, 1 if case.dx_acc else 0
    fake = C.addressof(_HOST_WORD)
    p = _rn.GnParams(c=case.c, groups=case.groups, act=_rn.ACT[case.act], act_after_residual=1 if case.aar else 0, eps=EPS,
                     drop_rate=case.drop, drop_seed=1234, sync=(sync or fake) if case.sync else None)
    keep = None
    if case.producer:
        keep = _rn.GnRows(rows_ptr or fake, case.producer[0], case.producer[1], case.groups)
        p.stat_rows = C.addressof(keep)
    return segs, len(case.segs), p, keep


def workspace_bytes(segs, nseg, params):
    import _rn
    return _rn.lib().rn_group_norm_workspace(segs, nseg, C.byref(params))


def query(segs, nseg, params, backward, ws_bytes):
    import _rn
    plan = _rn.GnPlan()
    _rn.check(_rn.lib().rn_group_norm_plan(segs, nseg, C.byref(params), 1 if backward else 0, ws_bytes, C.byref(plan)), "rn_group_norm_plan")
    return plan


def row_of(case, plan, backward):
    """The plan in EXPECT's form: (path, width, R, blocks, how dgamma / dbeta are formed).  width: slice_wc / pixels per block
    of the grid-resident kernel / the rows paths' slab / the three kernels' names."""
    import _rn
    path = _rn.GN_PATHS[plan.path]
    grad = _rn.GN_PARAM_GRADS[plan.param_grad_deferred if case.defer else plan.param_grad] if backward else None
    if path in ("slice", "narrow_slice"):
        return (path, plan.slice_wc, plan.slice_r, plan.slice_blocks, grad)
    if path == "grid_resident":
        return (path, plan.coop_ppc, plan.coop_r, plan.coop_blocks, grad)
    if path in ("rows", "producer_rows"):
        return (path, plan.rows_sw, plan.rows_apply_r, plan.rows_apply_blocks, grad)
    kernels = tuple(_rn.GN_KERNELS[k].replace("gn_", "").replace("_kernel", "") for k in (plan.stats_kernel, plan.finalize_kernel, plan.apply_kernel))
    return (path, kernels, 0, plan.apply_blocks, grad)
