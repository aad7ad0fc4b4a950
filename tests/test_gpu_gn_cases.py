"""rn_group_norm_fwd / rn_group_norm_bwd at every branch of their dispatch against the fp64 reference of tests/gn_ref.py.

The entry points are driven directly (ctypes structs), so that mean / rstd, the sync region, the strided views, the producer's
rows and the workspace are in the test's hands; every case first asserts, through rn_group_norm_plan with the real pointers and
the real workspace size, that it runs the branch tests/test_gn_cases_cpu.py lists for it.  The workspace is exactly the size
rn_group_norm_workspace asks for, followed by a guard area that must stay untouched.
Strided views: rn_gn_seg gives x and dx a leading dimension (y, the residual and dy are always dense), so x's wider buffer must
come back bit-unchanged, the channels behind c of dx's buffer likewise, and every element of y, mean, rstd and dres is written
(sentinels); with dx_accumulate dx is the old content plus the gradient, without it the old content is gone.

Every y, mean, rstd, dx, dres, dgamma and dbeta is compared with the fp64 reference, each against its own maximum
(helpers.rel_err), under two bars:
  * the project's: outputs and statistics 1e-4 (BASELINE north_star), gradients 5e-4 (what tests/test_gpu_wino_tower.py grants);
  * one tied to the arithmetic: with e32 = rel_err(reference in fp32, reference in fp64) and ek = rel_err(kernel, fp64),
    ek / max(e32, 2^-23) <= RATIO_BOUND[family].  e32 comes from the reference alone.  The families differ by design: the slice
    kernels hold a sample's slice in registers and take two-pass statistics like the reference; every other path sums x and
    x^2 in fp32 per chunk and merges the chunks in fp64, which is as good while |mean| / std is small and loses
    log2((mean / std)^2) bits where it is not (the "offset" twins: mean / std = 16).
RATIO_BOUND = {two-pass: 4, sum-of-squares: 4, sum-of-squares on offset data: 1024}, set on 2026-10-20: per family twice the
largest ratio of any tensor of any case of that family in one run of the table on an MI355X, rounded up to a power of two
(figures: profiles/gn_cases_err.txt).
  two-pass:        largest ratio 1.76 (slice-wc52-c1664, the mean: ek 3.1e-7, e32 1.8e-7); the offset twins slice-offset and
                   narrow-offset: 0.17 and 1.15
  sum-of-squares:  largest ratio 1.81 (rows-sw24, the mean: ek 2.2e-7, e32 1.2e-7)
  offset data:     largest ratio 302 (rows-offset, rstd of the 3 x 3 level: ek 3.6e-5, e32 8.7e-8); grid-resident 178 (coop-offset),
                   rows at 96 x 96 86, producer rows 10.9, three kernels 8.3.  The largest error of any tensor of any case is that
                   3.6e-5: the sum-of-squares paths stay inside the 1e-4 bar at mean / std = 16 and lose about two digits to it.
The kernels are bitwise reproducible, so the figures have no run-to-run noise."""
import ctypes as C

import numpy as np
import pytest
import torch

import gn_ref as R
from helpers import rel_err
from test_gn_cases_cpu import EXPECT

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
RATIO_BOUND = {R.TWO_PASS: 4.0, R.SUM_SQ: 4.0, R.SUM_SQ_OFFSET: 1024.0}
SENTINEL = 12345.0
GUARD = 1 << 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


def _matches(row, expect):
    return row == expect if isinstance(expect, tuple) else row[0] == expect


def run_case(case, expect, dev, monkeypatch, bwd_case=None):
    """One forward and one backward call of the case -> (dict of numpy arrays named like gn_ref.run_ref's, keep masks or None).
    expect: per direction EXPECT's row, or just the path's name.  bwd_case: the backward call runs under this case's switches
    and sync instead (same tensors: the statistics one path wrote feed another path's backward)."""
    import _rn
    L = _rn.lib()
    xs, ress, gamma, beta, dys = R.make_case(case)
    c, g, nseg = case.c, case.groups, len(xs)
    gam, bet = gamma.to(dev), beta.to(dev)
    xbufs = []
    for x in xs:
        if case.x_ld:
            buf = torch.full(tuple(x.shape[:3]) + (case.x_ld,), SENTINEL, device=dev)
            buf[..., :c] = x.to(dev)
        else:
            buf = x.to(dev).contiguous()
        xbufs.append(buf)
    xkeep = [b.clone() for b in xbufs]
    rds = [r.to(dev).contiguous() if r is not None else None for r in ress]
    ys = [torch.full(tuple(x.shape), SENTINEL, device=dev) for x in xs]
    means = [torch.full((x.shape[0], g), SENTINEL, device=dev) for x in xs]
    rstds = [torch.full((x.shape[0], g), SENTINEL, device=dev) for x in xs]
    rows = R.producer_rows(case, xs).to(dev) if case.producer else None
    sync = _rn.sync_counters(dev).data_ptr()

    def call(which, backward):
        R.configure(which, monkeypatch)
        segs, _, p, keep = R.host_call(which, sync=sync, rows_ptr=rows.data_ptr() if rows is not None else None)
        for i, s in enumerate(segs):
            s.x, s.mean, s.rstd = xbufs[i].data_ptr(), means[i].data_ptr(), rstds[i].data_ptr()
            s.residual = rds[i].data_ptr() if rds[i] is not None else None
            if backward:
                s.dy, s.dx = dyd[i].data_ptr(), dxbufs[i].data_ptr()
                s.dresidual = dress[i].data_ptr() if dress[i] is not None else None
            else:
                s.y = ys[i].data_ptr()
        need = R.workspace_bytes(segs, nseg, p)
        ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        row = R.row_of(which, R.query(segs, nseg, p, backward, need), backward)
        assert _matches(row, expect[backward]), "the call takes %s, not %s" % (row, expect[backward])
        if backward:
            lst = _rn.ReduceList.make() if which.defer else None
            _rn.check(L.rn_group_norm_bwd(segs, nseg, C.byref(p), _rn.f32(gam), _rn.f32(bet), _rn.f32(dgamma), _rn.f32(dbeta), ws.data_ptr(),
                                          need, _rn.stream(), C.byref(lst) if lst is not None else None), "rn_group_norm_bwd")
            if lst is not None:
                assert lst.count == 2                                  # dbeta and dgamma wait in the list
                _rn.check(L.rn_flush_reductions(C.byref(lst), _rn.stream()), "rn_flush_reductions")
        else:
            _rn.check(L.rn_group_norm_fwd(segs, nseg, C.byref(p), _rn.f32(gam), _rn.f32(bet), ws.data_ptr(), need, _rn.stream()),
                      "rn_group_norm_fwd")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()), "the call wrote behind its workspace"
        del keep

    call(case, 0)
    out = {}
    for i in range(nseg):
        assert not bool((ys[i] == SENTINEL).any()) and not bool((means[i] == SENTINEL).any()) and not bool((rstds[i] == SENTINEL).any())
        out["y%d" % i], out["mean%d" % i], out["rstd%d" % i] = ys[i].cpu().numpy(), means[i].cpu().numpy(), rstds[i].cpu().numpy()
    masks = [(y != 0).cpu() for y in ys] if case.drop else None

    gen = torch.Generator().manual_seed(7)
    dyd = [d.to(dev).contiguous() for d in dys]
    olds = [torch.randn(tuple(x.shape[:3]) + (case.dx_ld or c,), generator=gen) if (case.dx_ld or case.dx_acc) else None for x in xs]
    dxbufs = [o.to(dev) if o is not None else torch.full(tuple(x.shape), SENTINEL, device=dev) for o, x in zip(olds, xs)]
    dress = [torch.full(tuple(x.shape), SENTINEL, device=dev) if (case.aar and r is not None) else None for x, r in zip(xs, ress)]
    dgamma, dbeta = torch.full((c,), SENTINEL, device=dev), torch.full((c,), SENTINEL, device=dev)
    call(bwd_case or case, 1)
    for i in range(nseg):
        dx = dxbufs[i].cpu()
        if olds[i] is not None:
            assert torch.equal(dx[..., c:], olds[i][..., c:]), "channels behind c of dx's buffer changed"
            if case.dx_acc:
                out["dx%d" % i] = (dx[..., :c].double() - olds[i][..., :c].double()).numpy()     # dx = old + gradient
            else:
                out["dx%d" % i] = dx[..., :c].numpy()                                            # the old content is gone
        else:
            assert not bool((dx == SENTINEL).any())
            out["dx%d" % i] = dx.numpy()
        if dress[i] is not None:
            assert not bool((dress[i] == SENTINEL).any())
            out["dres%d" % i] = dress[i].cpu().numpy()
        assert torch.equal(xbufs[i], xkeep[i]), "x's buffer changed"
    out["dgamma"], out["dbeta"] = dgamma.cpu().numpy(), dbeta.cpu().numpy()
    if case.sync or (bwd_case is not None and bwd_case.sync):
        assert _rn.barrier_timeouts() == 0
    return out, masks


def compare(case, got, masks):
    """-> [(kind, tensor, ek, e32, ratio)]; kind: 'out' (y, mean, rstd) or 'grad'.  dres is compared where the kernel writes it
    (act_after_residual: otherwise the gradient of the residual is dy itself)."""
    ref64, ref32 = R.run_ref(case, torch.float64, masks), R.run_ref(case, torch.float32, masks)
    assert sorted(k for k in ref64 if not k.startswith("dres") or case.aar) == sorted(got)
    rows = []
    for tname in sorted(got):
        ek, e32 = rel_err(got[tname], ref64[tname]), rel_err(ref32[tname], ref64[tname])
        rows.append(("out" if tname[0] in "ymr" else "grad", tname, ek, e32, ek / max(e32, 2.0 ** -23)))
    return rows


def worst(rows, kind):
    return max((r for r in rows if r[0] == kind), key=lambda r: r[4])


def record_line(name, rows):
    """The case's line of profiles/gn_cases_err.txt."""
    parts = []
    for kind in ("out", "grad"):
        _, tname, ek, e32, ratio = worst(rows, kind)
        parts.append("%-4s %-6s ek %.3e  e32 %.3e  ratio %7.2f  (max ek %.3e)" % (kind, tname, ek, e32, ratio, max(r[2] for r in rows if r[0] == kind)))
    return "%-18s %-27s | %s" % (name, R.family(name), " | ".join(parts))


def check(name, rows):
    bound = RATIO_BOUND[R.family(name)]
    bad = ["%s %s: ek %.3e (bar %.0e), e32 %.3e, ratio %.2f (bound %s)" % (kind, tname, ek, OUT_BAR if kind == "out" else GRAD_BAR, e32, ratio, bound)
           for kind, tname, ek, e32, ratio in rows
           if ek > (OUT_BAR if kind == "out" else GRAD_BAR) or ratio > bound]
    assert not bad, "%s: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matches_fp64(dev, monkeypatch, name):
    case = R.CASES[name]
    got, masks = run_case(case, EXPECT[name], dev, monkeypatch)
    if case.drop:     # over the whole case: >= 25 000 elements, so 0.01 is 3.6 standard deviations of the fraction
        kept = sum(int(m.sum()) for m in masks) / float(sum(m.numel() for m in masks))
        assert abs(kept - (1 - case.drop)) < 0.01, kept
    rows = compare(case, got, masks)
    print(record_line(name, rows))
    check(name, rows)


DROP_SHAPE = R._case([(2, 20, 18)], 96, drop=0.25)
DROP_PATHS = [("slice", DROP_SHAPE), ("narrow_slice", DROP_SHAPE._replace(env=R._env(R.WC4))),
              ("grid_resident", DROP_SHAPE._replace(env=R._env(R.NS), sync=True)), ("rows", DROP_SHAPE._replace(env=R._env(R.NS))),
              ("producer_rows", DROP_SHAPE._replace(producer=(5, 0))), ("three_kernels", DROP_SHAPE._replace(env=R._env(R.NS, R.NR)))]


def test_dropout_mask_is_the_same_on_every_path(dev, monkeypatch):
    """The mask is a function of the seed and the element index only: one shape through all six implementations (each asserted
    through the plan query) gives bit-equal masks with the right keep fraction, and gradients that use the same mask."""
    first = None
    for path, case in DROP_PATHS:
        got, masks = run_case(case, (path, "slice" if path == "producer_rows" else path), dev, monkeypatch)
        assert abs(float(masks[0].float().mean()) - 0.75) < 0.01
        if first is None:
            first = masks[0]
        assert torch.equal(first, masks[0]), path
        for kind, tname, ek, _, _ in compare(case, got, masks):      # backward used the mask the forward's y shows
            assert ek <= (OUT_BAR if kind == "out" else GRAD_BAR), (path, tname, ek)


CROSS_SHAPE = R._case([(2, 20, 18), (2, 3, 3)], 64, res=True, aar=True)
CROSS = {"slice -> three kernels": (CROSS_SHAPE, "slice", CROSS_SHAPE._replace(env=R._env(R.NS, R.NR)), "three_kernels"),
         "three kernels -> rows": (CROSS_SHAPE._replace(env=R._env(R.NS, R.NR)), "three_kernels", CROSS_SHAPE._replace(env=R._env(R.NS)), "rows")}


@pytest.mark.parametrize("which", list(CROSS))
def test_statistics_of_one_path_feed_another_paths_backward(dev, monkeypatch, which):
    fwd_case, fwd_path, bwd_case, bwd_path = CROSS[which]
    got, _ = run_case(fwd_case, (fwd_path, bwd_path), dev, monkeypatch, bwd_case=bwd_case)
    for kind, tname, ek, _, _ in compare(fwd_case, got, None):
        assert ek <= (OUT_BAR if kind == "out" else GRAD_BAR), (tname, ek)


@pytest.mark.parametrize("name", R.ONE_PER_PATH)
def test_second_run_is_bit_identical(dev, monkeypatch, name):
    """The header promises a fixed summation order on every path -- the grid-resident one included, whose blocks merge the
    exchanged sums in fp64 in row order whichever block arrives first."""
    a, ma = run_case(R.CASES[name], EXPECT[name], dev, monkeypatch)
    b, mb = run_case(R.CASES[name], EXPECT[name], dev, monkeypatch)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert all(torch.equal(p, q) for p, q in zip(ma, mb))
