"""The case table of tests/gn_ref.py without a GPU: every case takes the branch of the GroupNorm dispatch it was picked for
(read off the host-only rn_group_norm_plan: the library loads without a device, and the query returns what `decide` in
csrc/group_norm.hip -- the one function rn_group_norm_fwd / rn_group_norm_bwd launch from -- decided under the same
environment switches), and the table as a whole reaches every branch listed in COVER.  A planner change that moves a case off
its branch fails here and says: pick another shape for that branch.  Further tests: the workspace suffices for the path taken,
the grid-resident depths that exist, RN_GN_ROWS_FIRST in a fresh process, the refusals, and the reference itself.

A row is (path, width, R, blocks, parameter gradients) for the forward and for the backward call:
  slice / narrow_slice   width = channels per block (slice_wc), R = the slice kernels' template R
  grid_resident          width = pixels per block, R = float4 values per thread (coop_r)
  rows / producer_rows   width = channel slab of the apply kernel, R = its template R, blocks = its pixel chunks (grid.x)
  three_kernels          width = (statistics, finalize, apply) kernels, blocks = apply blocks per sample"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gn_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

KERNEL, REDUCE, FINALIZE = "gn_param_grad_kernel", "rn_reduce_rows", "finalize_blocks"
GENERIC = ("partial", "finalize", "apply")
COLS = ("partial", "finalize_cols_segs", "apply")    # forward, c % 64 == 0 and whole groups per 64 channels


def both(path, width, r, blocks, grad):
    return ((path, width, r, blocks, None), (path, width, r, blocks, grad))


def sl(wc, r, blocks, grad=KERNEL):
    return both("slice", wc, r, blocks, grad)


def narrow(wc, r, blocks):
    return both("narrow_slice", wc, r, blocks, KERNEL)


def coop(ppc, r, blocks):
    return both("grid_resident", ppc, r, blocks, REDUCE)


def rows(sw, r, blocks):
    return both("rows", sw, r, blocks, REDUCE)


def prod(sw, r, blocks, bwd):
    """forward: the producer's rows; backward (which gets no rows): whatever the shape takes on its own"""
    return (("producer_rows", sw, r, blocks, None), bwd[1])


def three(fwd_kernels, blocks, grad=FINALIZE):
    return (("three_kernels", fwd_kernels, 0, blocks, None), ("three_kernels", GENERIC, 0, blocks, grad))


EXPECT = {
    # 512 / 8 = 64 pixel lanes: R = pow2(ceil(hw / 64)); blocks = samples x groups / (groups per block)
    "slice-wc8-r32": sl(8, 32, 16),
    "slice-r2": sl(8, 2, 64),
    "slice-r4-pyramid": sl(8, 4, 256),
    "slice-r8-2seg": sl(8, 8, 32),
    "slice-r16": sl(8, 16, 16),
    "slice-wc64-c2048": sl(64, 4, 64),
    "slice-wc9-c144": sl(9, 2, 32),
    "slice-wc30-c960": sl(30, 4, 64),
    "slice-wc52-c1664": sl(52, 4, 64),
    "slice-group64": sl(64, 8, 2),
    "slice-relu": sl(8, 2, 16),
    "slice-relu6-aar": sl(8, 2, 16),
    "slice-offset": sl(8, 32, 16),
    "slice-defer": sl(8, 2, 64, REDUCE),
    # 56 x 56 = 3136 pixels > 32 x 512 / 8: blocks of 8 channels do not fit, 4 do; 48 x 48 x 3-channel groups: 6
    "narrow-wc4": narrow(4, 32, 16),
    "narrow-wc6": narrow(6, 32, 32),
    "narrow-relu": narrow(4, 2, 16),
    "narrow-relu6-aar": narrow(4, 2, 16),
    "narrow-offset": narrow(4, 32, 16),
    "narrow-drop": narrow(4, 4, 32),
    # c / 4 quads across, 512 / (c / 4) pixel lanes x depth pixels per block
    "coop-r4": coop(32, 4, 4),
    "coop-r4-pyramid": coop(32, 4, 24),
    "coop-r16": coop(128, 16, 100),           # depth 4 would need 400 blocks
    "coop-c96": coop(84, 4, 10),
    "coop-c144": coop(56, 4, 14),
    "coop-groups256": coop(32, 4, 4),
    "coop-groups512": coop(8, 4, 16),         # 256 quads across: 2 pixel lanes
    "coop-relu": coop(128, 4, 2),
    "coop-relu6-aar": coop(128, 4, 2),
    "coop-offset": coop(32, 4, 4),
    "coop-r16-offset": coop(128, 16, 100),
    "rows-sw32": rows(32, 4, 3),
    "rows-sw24": rows(24, 4, 3),
    "rows-sw36": rows(36, 4, 4),
    "rows-sw48": rows(48, 4, 5),
    "rows-sw60": rows(60, 4, 1),
    # 98 chunk rows x 32 groups > 2048 entries: at most 48 pixel chunks, so the apply kernels deepen
    "rows-fwd16-bwd8": (("rows", 32, 16, 25, None), ("rows", 32, 8, 49, REDUCE)),
    "rows-fwd8": rows(32, 8, 36),
    "rows-x-ld": rows(32, 4, 3),
    "rows-dx-ld": rows(32, 4, 3),
    "rows-dx-acc": rows(32, 4, 3),
    "rows-relu": rows(32, 4, 1),
    "rows-relu6-aar": rows(32, 4, 1),
    "rows-offset": rows(32, 4, 3),
    "rows-fwd8-offset": rows(32, 8, 36),
    "prod-chan-1": prod(32, 4, 1, sl(8, 2, 16)),
    "prod-chan-5": prod(36, 4, 4, sl(9, 8, 32)),
    "prod-chan-72": prod(32, 8, 36, rows(32, 8, 36)),
    "prod-chan-r16": prod(32, 16, 25, rows(32, 8, 49)),
    "prod-group-1": prod(48, 4, 5, sl(12, 16, 16)),
    "prod-group-7": prod(32, 4, 3, sl(8, 8, 64)),
    "prod-relu": prod(32, 4, 1, sl(8, 2, 16)),
    "prod-relu6-aar": prod(32, 4, 1, sl(8, 2, 16)),
    "prod-offset": prod(36, 4, 4, sl(9, 8, 32)),
    "three-c2048": three(COLS, 15),
    "three-group256": three(GENERIC, 4),
    "three-sigmoid": three(GENERIC, 9),
    "three-x-ld": three(COLS, 6),
    "three-dx-acc": three(COLS, 6),
    "three-dx-ld": three(COLS, 6),
    "three-defer": three(GENERIC, 9, REDUCE),
    "three-drop": three(GENERIC, 9),
    "three-relu": three(COLS, 1),
    "three-relu6-aar": three(COLS, 1),
    "three-offset": three(GENERIC, 4),
}
PATHS = ("slice", "narrow_slice", "grid_resident", "rows", "three_kernels")
# every branch the table must reach, by the names _observe() gives them
COVER = (["%s %s" % (p, d) for p in PATHS for d in ("fwd", "bwd")] + ["producer_rows fwd"] +
         ["slice %s R%d" % (d, r) for d in ("fwd", "bwd") for r in (2, 4, 8, 16, 32)] +
         ["grid_resident %s R%d" % (d, r) for d in ("fwd", "bwd") for r in (4, 16)] +
         ["rows fwd R%d" % r for r in (4, 8, 16)] + ["rows bwd R%d" % r for r in (4, 8)] + ["producer_rows fwd R%d" % r for r in (4, 8, 16)] +
         ["%s act %s" % (p, a) for p in PATHS + ("producer_rows",) for a in (None, "elu", "relu", "relu6")] + ["three_kernels act sigmoid"] +
         ["%s %s" % (p, what) for p in PATHS + ("producer_rows",) for what in ("residual", "act after residual", "dropout", "offset data")] +
         ["%s several segments" % p for p in PATHS] +
         ["slice wc %d" % wc for wc in (8, 9, 30, 52, 64)] + ["narrow_slice wc 4", "narrow_slice wc 6", "slice several groups per block",
                                                              "slice one group of 64 channels", "slice segment far below R"] +
         ["rows sw %d" % sw for sw in (24, 32, 36, 48, 60)] + ["rows slab is all of c"] +
         ["grid_resident lanes do not divide the block", "grid_resident one pass over the groups without row lanes",
          "grid_resident several passes over the groups", "grid_resident <= 32 blocks", "grid_resident 100 blocks"] +
         ["producer_rows per channel", "producer_rows per group", "producer_rows 1 row", "producer_rows > 64 rows"] +
         ["%s x_ld" % p for p in ("rows", "three_kernels")] + ["%s dx_ld" % p for p in ("rows", "three_kernels")] +
         ["%s dx accumulate" % p for p in ("rows", "three_kernels")] +
         ["three_kernels several channel passes", "three_kernels group wider than 128", "three_kernels finalize", "three_kernels finalize_cols_segs"] +
         ["param grads %s" % g for g in (KERNEL, FINALIZE)] + ["param grads %s after %s" % (REDUCE, p) for p in PATHS if p != "narrow_slice"])    # (narrow: the slice launch itself)


def _observe(name, monkeypatch):
    """-> (the case as the plan query sees it, in EXPECT's form; names of the branches it takes; the two plans)"""
    case = R.CASES[name]
    R.configure(case, monkeypatch)
    segs, nseg, params, _keep = R.host_call(case)
    ws = R.workspace_bytes(segs, nseg, params)
    plans = [R.query(segs, nseg, params, b, ws) for b in (0, 1)]
    seen = tuple(R.row_of(case, p, b) for b, p in enumerate(plans))
    names = set()
    for d, (path, width, r, blocks, grad) in zip(("fwd", "bwd"), seen):
        names.add("%s %s" % (path, d))
        if path in ("slice", "grid_resident", "rows", "producer_rows"):
            names.add("%s %s R%d" % (path, d, r))
        if grad:
            names.add("param grads %s" % grad if grad != REDUCE else "param grads %s after %s" % (grad, path))
        if d == "bwd" and case.producer:
            continue                                                      # what follows describes the forward call of producer cases
        names.add("%s act %s" % (path, case.act))
        for flag, what in ((case.res and not case.aar, "residual"), (case.aar, "act after residual"), (case.drop > 0, "dropout"),
                           (case.offset >= 8, "offset data"), (len(case.segs) > 1, "several segments"), (case.x_ld, "x_ld"),
                           (case.dx_ld, "dx_ld"), (case.dx_acc, "dx accumulate")):
            if flag:
                names.add("%s %s" % (path, what))
        if path in ("slice", "narrow_slice"):
            names.add("%s wc %d" % (path, width))
            if width > R.cpg(case):
                names.add("slice several groups per block")
            if R.cpg(case) == 64:
                names.add("slice one group of 64 channels")
            if min(h * w for _, h, w in case.segs) * 4 <= r * (512 // width):
                names.add("slice segment far below R")
        if path == "rows":
            names.add("rows sw %d" % width)
            if width == case.c:
                names.add("rows slab is all of c")
        if path == "grid_resident":
            if 512 % (case.c // 4):
                names.add("grid_resident lanes do not divide the block")
            # coop_group_totals: 2 x groups (group, component) entries over the 512 threads of a block -- row lanes while they
            # are fewer, exactly one pass without row lanes at 512, a second pass (e0 = 512) only above
            if 2 * case.groups == 512:
                names.add("grid_resident one pass over the groups without row lanes")
            if 2 * case.groups > 512:
                names.add("grid_resident several passes over the groups")
            names.add("grid_resident <= 32 blocks" if blocks <= 32 else "grid_resident %d blocks" % blocks)
        if path == "producer_rows":
            names.add("producer_rows per group" if case.producer[1] else "producer_rows per channel")
            if case.producer[0] == 1:
                names.add("producer_rows 1 row")
            if case.producer[0] > 64:
                names.add("producer_rows > 64 rows")
        if path == "three_kernels":
            names.add("three_kernels %s" % width[1])
            if case.c > 1024:
                names.add("three_kernels several channel passes")
            if R.cpg(case) > 128:
                names.add("three_kernels group wider than 128")
    return seen, names, plans


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_its_branch(name, monkeypatch):
    seen, _, plans = _observe(name, monkeypatch)
    assert seen == EXPECT[name], "case %s left its branch: the planner now gives %s -- pick another shape for %s" % (name, seen, EXPECT[name])
    case = R.CASES[name]
    # the slice kernels cover a sample with blocks of slice_wc channels; the grid-resident blocks cover every segment's pixels
    for plan in plans:
        samples = sum(n for n, _, _ in case.segs)
        if plan.slice_wc:
            assert plan.slice_blocks * plan.slice_wc == samples * case.c
        if plan.coop_r:
            assert plan.coop_blocks == plan.total_chunks == sum(n * -(-h * w // plan.coop_ppc) for n, h, w in case.segs)
            assert plan.coop_ppc == (512 // (case.c // 4)) * plan.coop_r


def test_table_covers_every_branch(monkeypatch):
    assert sorted(EXPECT) == sorted(R.CASES)
    names = set()
    for name in R.CASES:
        names |= _observe(name, monkeypatch)[1]
    missing = [b for b in COVER if b not in names]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


def test_table_shapes():
    """What the planner does not decide but the cases were picked for."""
    for name, case in R.CASES.items():
        assert R.elements(case) <= 4 << 20, name
        # no degenerate groups: their gradients are ill-conditioned in any arithmetic
        assert min(h * w for _, h, w in case.segs) * R.cpg(case) >= 16, name
        if case.drop:     # the mask is read off y != 0: a kept element must not be zero, and no residual may hide it
            assert case.act in (None, "elu") and not case.res, name
            assert R.elements(case) >= 25000, name      # keep fraction within 0.01: 3.6 sigma of sqrt(0.1875 / elements)
        if case.act in R.KINKS:
            assert R.elements(case) <= 30000 and name in KINK_MARGINS, name
        if case.producer:
            assert len(case.segs) == 1 and not case.x_ld and not case.dx_ld
    assert sum(R.elements(c) <= 200000 for c in R.CASES.values()) > len(R.CASES) * 3 // 4
    for twin, plain in R.OFFSET_TWINS.items():
        a, b = R.CASES[twin], R.CASES[plain]
        assert a.offset == 16.0 and a._replace(offset=b.offset) == b, twin
    assert sorted(R.OFFSET_TWINS) == sorted(n for n, c in R.CASES.items() if c.offset >= 8)
    assert {EXPECT[n][0][0] for n in R.ONE_PER_PATH} == {"slice", "narrow_slice", "grid_resident", "rows", "producer_rows", "three_kernels"}


def _align(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("name", list(R.CASES))
def test_workspace_suffices_for_the_path_taken(name, monkeypatch):
    """The three areas of the workspace -- [2][chunks][c] partial planes, max(samples, 256) x groups coefficient pairs,
    [chunks][groups] row pairs -- at the chunk count the PLAN reports (the grid-resident path re-chunks), against the bytes
    rn_group_norm_workspace asks for; the slice kernels' per-sample rows lie in the first area.
    This restates the library's own layout in Python, so it is a consistency check between the plan's chunk counts and the
    workspace query and would pass if both were wrong alike.  What guards the kernels' writes is the GPU test: every call of
    tests/test_gpu_gn_cases.py gets a workspace of exactly the size asked for with a 64 KiB guard area behind it."""
    case = R.CASES[name]
    _, _, plans = _observe(name, monkeypatch)
    segs, nseg, params, _keep = R.host_call(case)
    ws = R.workspace_bytes(segs, nseg, params)
    samples = sum(n for n, _, _ in case.segs)
    for b, plan in enumerate(plans):
        path = R.row_of(case, plan, b)[0]
        planes = _align(plan.total_chunks * case.c * 8)
        coef = _align(max(samples, 256) * case.groups * 8)
        rows = _align(plan.total_chunks * case.groups * 8)
        assert plan.total_chunks >= (samples if path != "producer_rows" else 1)
        if path in ("slice", "narrow_slice"):
            assert 2 * samples * case.c * 4 <= planes <= ws
        elif path == "producer_rows":
            assert plan.total_chunks == case.segs[0][0] * case.producer[0]
        else:
            assert planes + coef + rows <= ws, (path, planes, coef, rows, ws)
        if path == "producer_rows":
            assert list(plan.rows_per_sample)[:nseg] == [case.producer[0]]
        if path == "rows":
            assert sum(n * r for (n, _, _), r in zip(case.segs, plan.rows_per_sample)) == plan.total_chunks


def test_grid_resident_depths(monkeypatch):
    """plan_coop takes depth 4 while the grid has at most 256 blocks and a deeper kernel while it has at most 128; since
    ceil(hw / 4L) <= 2 ceil(hw / 8L), a grid above 256 blocks at depth 4 is above 128 at depth 8: a depth-8 kernel could never be
    chosen.  A sweep of the plan query over channels, groups, samples, pixels and a second segment saw depths 4 and 16 only while
    the depth-8 arm still existed; it and its eight kernel instantiations were deleted, and the sweep pins {4, 16}."""
    import _rn
    L = _rn.lib()
    for name in R.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    plan, seen, paths = _rn.GnPlan(), set(), set()
    for c, groups in ((16, 16), (64, 32), (96, 32), (144, 16), (256, 32), (256, 256), (1024, 32), (1024, 1024)):
        for n in (1, 2, 5, 16, 39):
            for hw in list(range(1, 64, 3)) + list(range(64, 16000, 211)):
                for second in (None, (2, 9), (1, 400)):
                    segs = (_rn.GnSeg * 2)()
                    segs[0].n, segs[0].hw = n, hw
                    if second:
                        segs[1].n, segs[1].hw = second
                    nseg = 2 if second else 1
                    p = _rn.GnParams(c=c, groups=groups, act=2, eps=1e-5, sync=C.addressof(R._HOST_WORD))
                    ws = L.rn_group_norm_workspace(segs, nseg, C.byref(p))
                    for bwd in (0, 1):
                        assert L.rn_group_norm_plan(segs, nseg, C.byref(p), bwd, ws, C.byref(plan)) == 0
                        paths.add(_rn.GN_PATHS[plan.path])
                        if plan.coop_r:
                            assert plan.path == 3 and plan.coop_blocks <= (256 if plan.coop_r == 4 else 128)
                            seen.add(plan.coop_r)
    assert seen == {4, 16}
    assert paths >= {"slice", "grid_resident", "rows"}          # the sweep reaches the planner's neighbours as well


def test_rows_first_is_read_once_per_process():
    """RN_GN_ROWS_FIRST is cached in a static at the first call: a fresh child process that only runs the plan query (it never
    touches a GPU) shows the rows path in front of the grid-resident one; a second child, started with it off, shows the
    grid-resident kernel for the same call."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "import gn_ref as R\n"
              "case = R.CASES['coop-r4']\n"
              "segs, nseg, p, keep = R.host_call(case)\n"
              "ws = R.workspace_bytes(segs, nseg, p)\n"
              "print('PLAN', [R.row_of(case, R.query(segs, nseg, p, b, ws), b)[0] for b in (0, 1)])\n"
              % (here, os.path.join(os.path.dirname(here), "retinanet-tensorflow_amd")))
    env = {k: v for k, v in os.environ.items() if k not in R.SWITCHES}
    env.update(RN_GN_NO_SLICE="1")
    outs = []
    for first in ("1", "0"):
        env["RN_GN_ROWS_FIRST"] = first
        out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append([ln for ln in out.stdout.splitlines() if ln.startswith("PLAN")][0])
    assert outs == ["PLAN ['rows', 'rows']", "PLAN ['grid_resident', 'grid_resident']"]


def test_plan_query_refuses_what_the_launches_refuse():
    import _rn
    L = _rn.lib()
    segs = (_rn.GnSeg * 17)()
    for s in segs:
        s.n, s.hw = 1, 64
    plan = _rn.GnPlan()

    def q(nseg=1, backward=0, ws=None, plan_ref=C.byref(plan), **kw):
        args = dict(c=64, groups=32, act=2, eps=1e-5)
        args.update(kw)
        p = _rn.GnParams(**args)
        need = L.rn_group_norm_workspace(segs, min(max(nseg, 1), 16), C.byref(p))
        return L.rn_group_norm_plan(segs, nseg, C.byref(p), backward, need if ws is None else ws, plan_ref)

    assert q() == 0 and plan.path == 2
    assert q(plan_ref=None) == -1
    assert q(c=66, groups=33) == -2                      # c % 4
    assert q(c=4096) == -2                               # c > 2048
    assert q(c=64, groups=24) == -1                      # groups must divide c
    assert q(nseg=0) == -1 and q(nseg=17) == -1 and q(nseg=16) == 0
    assert q(backward=1, in_f16=1) == -2 and q(backward=1, out_f16=1) == -2 and q(backward=0, in_f16=1, out_f16=1) == 0
    assert plan.path == 6 and plan.stats_kernel == 2 and plan.apply_kernel == 6      # the fp16 kernels' choice is merely reported
    assert q(drop_rate=1.0) == -1
    assert q(ws=0) == -4                                 # the launches' workspace check
    assert L.rn_group_norm_plan(None, 1, None, 0, 1 << 20, C.byref(plan)) == -1
    segs[0].x_ld = 66                                    # not a multiple of 4
    assert q() == -1
    segs[0].x_ld = 96
    assert q() == 0 and plan.path == 5 and q(in_f16=1, out_f16=1) == -2              # strided views are fp32 only
    segs[0].x_ld, segs[0].hw = 0, 0
    assert q() == -1
    # (the workspace query answers 0 for a segment the launches refuse; it used to divide by zero at hw = 0)
    assert L.rn_group_norm_workspace(segs, 1, C.byref(_rn.GnParams(c=64, groups=32))) == 0


def test_reference_is_the_oracles_group_norm():
    """run_ref in fp64 == oracle/tf_ops_ref.group_norm + activation (+ residual) to fp64 rounding: outputs and every gradient;
    its statistics are the biased two-pass moments."""
    for name in ("slice-r2", "slice-r4-pyramid", "slice-wc9-c144", "three-group256"):
        case = R.CASES[name]
        xs, ress, gamma, beta, dys = R.make_case(case)
        got = R.run_ref(case, torch.float64)
        leaf = lambda t: t.double().requires_grad_(True)      # noqa: E731
        xs, gamma, beta = [leaf(x) for x in xs], leaf(gamma), leaf(beta)
        ress = [leaf(r) if r is not None else None for r in ress]
        ys = []
        for x, r in zip(xs, ress):
            y = T.activation(T.group_norm(x, gamma, beta, case.groups), case.act)
            ys.append(y + r if r is not None else y)
        grads = torch.autograd.grad(ys, xs + [gamma, beta], [d.double() for d in dys])
        for i, y in enumerate(ys):
            assert rel_err(got["y%d" % i], y.detach().numpy()) < 1e-13
            assert rel_err(got["dx%d" % i], grads[i].numpy()) < 1e-12
            n, h, w, c = xs[i].shape
            xg = xs[i].detach().numpy().reshape(n, h * w, case.groups, -1)
            assert rel_err(got["mean%d" % i], xg.mean((1, 3))) < 1e-13
            assert rel_err(got["rstd%d" % i], 1 / np.sqrt(xg.var((1, 3)) + R.EPS)) < 1e-13
        assert rel_err(got["dgamma"], grads[-2].numpy()) < 1e-12 and rel_err(got["dbeta"], grads[-1].numpy()) < 1e-12


def test_reference_orders_dropout_and_residual():
    """y = drop(act(GN(x))) + residual, against y = drop(act(GN(x) + residual)): on a hand-made mask."""
    case = R._case([(1, 4, 4)], 8, groups=2, act="elu", res=True, drop=0.25)
    xs, ress, gamma, beta, _ = R.make_case(case)
    mask = [torch.arange(128).reshape(1, 4, 4, 8) % 4 != 0]
    z = T.group_norm(xs[0].double(), gamma.double(), beta.double(), 2)
    y = R.run_ref(case, torch.float64, mask)["y0"]
    assert rel_err(y, (T.activation(z, "elu") * mask[0] / 0.75 + ress[0].double()).numpy()) < 1e-14
    y = R.run_ref(case._replace(aar=True), torch.float64, mask)["y0"]
    assert rel_err(y, (T.activation(z + ress[0].double(), "elu") * mask[0] / 0.75).numpy()) < 1e-14


def test_producer_rows_sum_to_the_statistics():
    for name in ("prod-chan-5", "prod-group-7"):
        case = R.CASES[name]
        xs = R.make_case(case)[0]
        rows = R.producer_rows(case, xs).double()
        assert rows.shape == (case.segs[0][0], case.producer[0], case.groups if case.producer[1] else case.c, 2)
        n, h, w, c = xs[0].shape
        tot = rows.sum(1).reshape(n, case.groups, -1, 2).sum(2) / (h * w * R.cpg(case))
        ref = R.run_ref(case, torch.float64)
        assert rel_err(tot[..., 0].numpy(), ref["mean0"]) < 1e-6
        assert rel_err(1 / np.sqrt(tot[..., 1].numpy() - tot[..., 0].numpy() ** 2 + R.EPS), ref["rstd0"]) < 1e-5


# seed -> measured margin, pinned so that a change of the generator is noticed
KINK_MARGINS = {"slice-relu": 2.473e-4, "slice-relu6-aar": 5.588e-4, "narrow-relu": 7.110e-4, "narrow-relu6-aar": 6.837e-4,
                "coop-relu": 2.473e-4, "coop-relu6-aar": 5.588e-4, "rows-relu": 2.473e-4, "rows-relu6-aar": 5.588e-4,
                "prod-relu": 2.473e-4, "prod-relu6-aar": 5.588e-4, "three-relu": 2.473e-4, "three-relu6-aar": 5.588e-4}


@pytest.mark.parametrize("name", list(KINK_MARGINS))
def test_no_preactivation_sits_on_a_kink(name):
    """relu / relu6: the derivative jumps at 0 (and 6), so an element within rounding of a kink may differ by O(1) between two
    correct evaluations.  The pre-activation -- GN(x), or GN(x) + residual with act_after_residual -- is O(1) (O(4) in the relu6
    cases) and two correct fp32 evaluations agree to a few 1e-6 of that: each case's seed is chosen so that, in the fp64
    reference, no pre-activation is within KINK_MARGIN = 1e-4 of a kink."""
    case = R.CASES[name]
    margin = R.kink_margin(case)
    assert margin > R.KINK_MARGIN, margin
    assert abs(margin / KINK_MARGINS[name] - 1) < 1e-3, margin


def test_relu6_cases_use_both_kinks():
    """gamma is scaled to about 4 so that the upper kink is in use: at least 1 % of the pre-activations lie above 6 and at
    least 1 % below 0."""
    for name, case in R.CASES.items():
        if case.act == "relu6":
            p = torch.cat([q.flatten() for q in R.pre_activations(case)])
            assert float((p > 6).double().mean()) >= 0.01 and float((p < 0).double().mean()) >= 0.01, name
    assert [name for name, case in R.CASES.items() if case.act in R.KINKS] == list(KINK_MARGINS)
