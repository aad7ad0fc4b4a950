"""The detection kernels' case table (tests/detect_ref.py) reaches every branch of csrc/decode_nms.hip -- proven without a GPU.

EXPECT[case] is the plan row the case must take: (scan kernel, half, logit, q, LDS bytes per wave, scan grid, offsets blocks, emit
mode, emit grid, emit LDS bytes, segment path, segments).  tests/test_gpu_detect_cases.py asserts that rn_detect_plan with the
real arguments gives the same row before it runs the case; here the row is held against detect_ref.plan_ref, the independent
model of the host rules, and against rn_detect_plan itself (host only: no device is touched).  The sets below name every
branch; a label that loses its case fails the coverage tests."""
import ctypes as C

import numpy as np
import pytest

import detect_ref as R
from oracle import utils_ref

f32 = np.float32


def _base(scan, C_, half=0, logit=0, q=0, lds=0, n=3, seg="LDS_SCATTER", emit="HIST", grid=4):
    """a row of the base pyramid: n * 5 waves = 4 blocks (n = 3), one offsets block"""
    return (scan, half, logit, q, lds, grid, 1, emit, grid, n * C_ * 4 if emit == "HIST" else 0, seg, n * C_)


def _nms(nseg):
    return (None, 0, 0, 0, 0, 0, 0, None, 0, 0, "LDS_SCATTER", nseg)


EXPECT = {}
for _c, _q in ((4, 1), (20, 2), (36, 3), (64, 4), (80, 5), (84, 6), (100, 7), (128, 8)):
    EXPECT["scan-f32-c%d-p" % _c] = _base("Q", _c, 0, 0, _q)
    EXPECT["scan-f32-c%d-z" % _c] = _base("Q", _c, 0, 1, _q)
for _c, _q in ((8, 1), (40, 2), (128, 4), (256, 8)):
    EXPECT["scan-f16-c%d-p" % _c] = _base("Q", _c, 1, 0, _q)
    EXPECT["scan-f16-c%d-z" % _c] = _base("Q", _c, 1, 1, _q)
for _m in "pz":
    for _t, _cs in (("f32", (132, 3, 5, 130)), ("f16", (264, 12))):
        for _c in _cs:
            EXPECT["scan-%s-c%d-%s" % (_t, _c, _m)] = _base("GENERIC", _c)
    EXPECT["scan-f16-c80-" + _m] = _base("T", 80)
    EXPECT["scan-f16-c80-noT-" + _m] = _base("Q", 80, 1, int(_m == "z"), 3)
    EXPECT["scan-f16-c80-noNT-" + _m] = _base("T_PLAIN", 80)
    EXPECT["scan-lds-f32-c92-" + _m] = _base("LDS", 92, lds=23552)
    EXPECT["scan-lds-f16-c80-" + _m] = _base("LDS", 80, lds=11264)
EXPECT.update({
    "scan-mixed-storage-c16": _base("GENERIC", 16),
    "scan-mixed-logit-c16": _base("GENERIC", 16),
    "scan-lds-f32-c4-p": _base("LDS", 4, lds=1024),
    "scan-lds-f32-c80-z": _base("LDS", 80, lds=21504),
    "scan-lds-f32-c96-declined": _base("Q", 96, 0, 0, 6),
    "scan-no-lds-wins": _base("Q", 4, 0, 0, 1),
    "adv-T": _base("T", 80, n=2, grid=1),
    "adv-Q-f32": _base("Q", 36, 0, 1, 3, n=2, grid=1),
    "adv-Q-f16": _base("Q", 40, 1, 1, 2, n=2, grid=1),
    "adv-GENERIC-f32": _base("GENERIC", 5, n=2, grid=1),
    "adv-GENERIC-f16": _base("GENERIC", 12, n=2, grid=1),
    "adv-LDS": _base("LDS", 92, lds=23552, n=2, grid=1),
    "adv-mixed": _base("GENERIC", 16, n=2, grid=2),
    "det-off2-hist": ("Q", 0, 0, 1, 0, 285, 2, "HIST", 285, 16, "LDS_SCATTER", 4),
    "det-off2-strided": ("Q", 0, 0, 1, 0, 285, 2, "STRIDED", 285, 0, "LDS_SCATTER", 4),
    "det-off10-hist": ("Q", 0, 0, 1, 0, 2377, 10, "HIST", 2048, 16, "LDS_SCATTER", 4),
    "det-off10-strided": ("Q", 0, 0, 1, 0, 2377, 10, "STRIDED", 2048, 0, "LDS_SCATTER", 4),
    "det-global-scatter": _base("GENERIC", 2800, seg="GLOBAL_SCATTER", emit="STRIDED"),      # 8400 segments > EMIT_MAXSEG too
    "det-gather-second-pass": _base("GENERIC", 200),
    "det-empty": _base("Q", 4, 0, 0, 1),
    "det-overcap-hist": _base("Q", 4, 0, 0, 1),
    "det-overcap-strided": _base("Q", 4, 0, 0, 1, emit="STRIDED"),
    "nms-sort-lengths": _nms(32), "nms-cap-1": _nms(2), "nms-cap-5": _nms(2), "nms-cap-64": _nms(2), "nms-cap-1000": _nms(2),
    "nms-cap-1024": _nms(2), "nms-kept-counts": _nms(4), "nms-disjoint": _nms(4), "nms-identical": _nms(1), "nms-chains": _nms(2),
    "nms-near-thr-0.5": _nms(408), "nms-near-thr-0.3": _nms(408), "nms-near-thr-0.75": _nms(408), "nms-near-thr-0": _nms(340),
    "nms-near-thr-1": _nms(408), "nms-degenerate": _nms(3), "nms-ties": _nms(6), "nms-many": _nms(6),
})

# every branch of the host rules: (scan kernel, half, logit, q or the catch-all's reason) ...
PLAN_LABELS = {("Q", 0, lg, q) for lg in (0, 1) for q in range(1, 9)} | {("Q", 1, lg, q) for lg in (0, 1) for q in (1, 2, 3, 4, 8)} | \
    {("T", h, lg, 0) for h in (1,) for lg in (0, 1)} | {("T_PLAIN", 1, lg, 0) for lg in (0, 1)} | \
    {("LDS", h, lg, 0) for h in (0, 1) for lg in (0, 1)} | {("GENERIC", "remainder"), ("GENERIC", "q>8"), ("GENERIC", "mixed")} | \
    {"HIST", "STRIDED", "STRIDED:nseg", "offsets:1", "offsets:2", "offsets:>=10", "emit-grid:capped", "emit-grid:uncapped",
     "LDS_SCATTER", "GLOBAL_SCATTER", "chunks%4!=0", "lds:declined", "lds:switched-off"}
# ... and of the device code that depends on the data
DEVICE_LABELS = {"scatter:few", "scatter:many", "scatter:global", "sort:lds", "sort:global", "nms:early-exit", "nms:identical",
                 "cap:mid-batch", "kept:15", "kept:16", "kept:17", "kept:>64", "gather:passes=1", "gather:passes=2",
                 "nms:batches=0", "nms:batches=1", "nms:batches=2", "nms:batches=>2"} | \
    {"sort:%d" % m for m in R.SORT_LENGTHS} | {"cap:%d" % m for m in (1, 5, 64, 1000, 1024)}


def plan_labels(case):
    p = R.plan_ref(case)
    if case.entry == "nms_classwise":
        return {p["segments"]}
    lv = case.levels[0]
    out = {p["emit"], p["segments"], "offsets:%s" % (p["offsets_blocks"] if p["offsets_blocks"] < 10 else ">=10"),
           "emit-grid:capped" if p["scan_grid"] > 2048 else "emit-grid:uncapped"}
    out.add(("GENERIC", p["reason"]) if p["scan"] == "GENERIC" else (p["scan"], int(lv.half), int(lv.logit), p["q"]))
    if p["scan"] == "Q" and (case.C // (8 if lv.half else 4)) % 4:
        out.add("chunks%4!=0")            # the clamped, duplicated chunk min(sub + 4 q, CV - 1) is taken
    if p["emit"] == "STRIDED" and p["nseg"] > 8192:
        out.add("STRIDED:nseg")
    env = dict(case.env)
    if "RN_SCAN_LDS" in env and p["scan"] != "LDS":
        out.add("lds:switched-off" if "RN_SCAN_NO_LDS" in env else "lds:declined")
    return out


def test_the_table_and_expect_name_the_same_cases():
    assert sorted(EXPECT) == sorted(R.CASES)


@pytest.mark.parametrize("name", list(R.CASES))
def test_plan_model_gives_the_expected_row(name):
    assert R.plan_row(R.plan_ref(R.CASES[name])) == EXPECT[name]


def product_plan(case, levels=None, cap=None, max_per_class=None):
    """rn_detect_plan for the case -> (status, row, workspace bytes); levels: a filled _rn.DetLevel array (default: shapes only)"""
    import _rn
    L = _rn.lib()
    par = _rn.DetParams(case.n, case.C, max_per_class or case.max_per_class, case.score_thr, case.iou_thr, cap or R.capacity(case))
    pl = _rn.DetPlan()
    if case.entry == "nms_classwise":
        st = L.rn_detect_plan(None, 0, C.byref(par), C.byref(pl))
    else:
        if levels is None:
            levels = (_rn.DetLevel * len(case.levels))()
            for i, l in enumerate(case.levels):
                levels[i].rows_per_image, levels[i].prob_f16, levels[i].prob_is_logit = l.rows, int(l.half), int(l.logit)
        st = L.rn_detect_plan(levels, len(case.levels), C.byref(par), C.byref(pl))
    row = (_rn.DET_SCANS[pl.scan], pl.scan_half, pl.scan_logit, pl.scan_q, pl.scan_lds_per_wave, pl.scan_grid, pl.offsets_blocks,
           _rn.DET_EMITS[pl.emit_mode], pl.emit_grid, pl.emit_lds_bytes, _rn.DET_SEGMENTS.get(pl.segments), pl.nseg)
    return st, row, pl.workspace_bytes


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items() if not c.process])
def test_the_products_plan_entry_agrees_on_the_host(name, monkeypatch):
    """(the cases whose switch is read once per process are asserted in their child process on the GPU)"""
    case = R.CASES[name]
    for k in ("RN_SCAN_LDS", "RN_SCAN_NO_LDS", "RN_SCAN_T", "RN_SCAN_NT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    st, row, ws = product_plan(case)
    assert st == 0 and row == EXPECT[name] and ws == R.plan_ref(case)["workspace"]


def test_plan_entry_refusals():
    import _rn
    case = R.CASES["det-empty"]
    assert product_plan(case, max_per_class=1025)[0] == -2                     # RN_EUNSUPPORTED
    assert _rn.lib().rn_detect_plan(None, 0, None, None) == -1                 # RN_EINVAL


def test_every_host_branch_has_a_case():
    seen = set()
    for case in R.CASES.values():
        seen |= plan_labels(case)
    assert PLAN_LABELS - seen == set(), sorted(map(str, PLAN_LABELS - seen))


@pytest.fixture(scope="module")
def branches():
    return {name: R.device_branches(case, R.make_case_cached(case), R.run_ref_cached(case)) for name, case in R.CASES.items()}


def test_every_device_branch_has_a_case(branches):
    seen = set().union(*branches.values())
    assert DEVICE_LABELS - seen == set(), sorted(DEVICE_LABELS - seen)
    assert "sort:16385" in branches["nms-sort-lengths"] and "sort:0" in branches["nms-sort-lengths"]     # one call, empty segments between
    assert {"sort:%d" % m for m in R.SORT_LENGTHS} <= branches["nms-sort-lengths"]
    assert {"scatter:many", "sort:global"} <= branches["nms-many"]
    assert "scatter:global" in branches["det-global-scatter"] and "gather:passes=2" in branches["det-gather-second-pass"]
    assert "nms:identical" in branches["nms-identical"] and "nms:early-exit" in branches["nms-identical"]
    assert {"kept:15", "kept:16", "kept:17", "kept:>64"} <= branches["nms-kept-counts"]
    assert any("cap:mid-batch" in branches["nms-cap-%d" % m] for m in (5, 64, 1000, 1024))
    for m in (1, 5, 64, 1000, 1024):
        assert "cap:%d" % m in branches["nms-cap-%d" % m]


def test_conditions_on_the_reference_alone():
    for name, case in R.CASES.items():
        ref = R.run_ref_cached(case)
        cand, kept = int(ref["counts"][0]), int(ref["counts"][1])
        assert (kept > 0) == (name != "det-empty"), name
        assert int(ref["counts"][2:].sum()) == (kept if case.entry != "boxes_decode" else 0)
        # a suppression wherever an NMS runs on boxes that can overlap (an IoU above 1.0 does not exist)
        no_nms = case.entry == "boxes_decode" or case.recipe == "adversarial" or name in ("det-empty", "nms-disjoint", "nms-near-thr-1")
        assert kept < cand if not no_nms else kept <= cand, name
        if name.startswith("det-overcap"):
            assert cand > R.capacity(case)
        elif case.entry != "nms_classwise":
            assert cand <= R.capacity(case), name


def test_chains_keep_every_other_box_and_dead_boxes_kill_nothing():
    ref = R.run_ref_cached(R.CASES["nms-chains"])
    assert np.array_equal(ref["anchor"], np.concatenate([np.arange(0, 40, 2), 40 + np.arange(0, 200, 2)]))


def test_the_zero_tie_is_won_by_the_lower_index():
    case = R.CASES["nms-ties"]
    inp, ref = R.make_case_cached(case), R.run_ref_cached(case)
    s = inp["scores"]
    for k in range(0, 40, 2):
        assert np.signbit(s[k]) and s[k] == 0 and not np.signbit(s[k + 1]) and s[k + 1] == 0
        assert k in ref["anchor"] and k + 1 not in ref["anchor"]
    assert (s < 0).sum() > 100 and len(np.unique(s)) <= 5


def test_smallest_cases_agree_with_the_scalar_nms():
    for name in ("scan-f32-c4-p", "scan-f32-c36-z", "nms-kept-counts", "nms-chains", "nms-degenerate", "nms-ties", "nms-near-thr-0.5",
                 "nms-near-thr-0", "nms-identical"):
        case = R.CASES[name]
        a, b = R.run_ref_cached(case), R.run_ref(case, R.make_case_cached(case), nms=utils_ref.nms_indices)
        for k in ("boxes", "scores", "class", "image", "anchor", "counts"):
            assert np.array_equal(a[k], b[k]), (name, k)


def test_boxes_decode_thr_is_the_oracles_at_its_threshold():
    case = R.CASES["scan-f32-c20-p"]
    inp = R.make_case_cached(case)
    got, rows = R.boxes_decode_thr(inp["probs"][0][1], inp["boxes"][0][1], 0.5)
    want = utils_ref.boxes_decode(inp["probs"][0][1], inp["boxes"][0][1])
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(rows) == len(want.scores) > 0


def test_logit_gap_of_distinct_candidate_scores():
    """distinct candidate logits differ by at least 4e-6 in probability: the device's 1e-6 cannot reorder or tie them"""
    for name, case in R.CASES.items():
        if case.recipe == "adversarial" or not any(l.logit for l in case.levels):
            continue
        inp = R.make_case_cached(case)
        z = np.concatenate([p.astype(np.float64).max(-1).ravel() for l, p in zip(case.levels, inp["probs"]) if l.logit])
        z = np.unique(z[z > 0])
        assert len(z) >= 1 and np.abs(z).max() <= 8 and np.all(z * 64 == np.round(z * 64)), name
    grid = np.arange(1, 513) / 64.0                       # every positive logit a case may hold
    assert np.diff(R.sigmoid64(grid)).min() >= 4e-6


def test_near_threshold_pairs_sit_inside_the_band_and_on_the_threshold():
    for thr in (0.5, 0.3, 0.75, 1.0):
        A, B = R.near_thr_pairs(thr)
        iou = (B[:, 3].astype(np.float64) * B[:, 2]) / (A[:, 3].astype(np.float64) * A[:, 2])      # B inside A, exact in fp64
        t = float(f32(thr))
        rel = iou / t - 1.0
        on, below, above = int((rel == 0).sum()), int(((rel < 0) & (rel > -2.0 ** -20)).sum()), int(((rel > 0) & (rel < 2.0 ** -20)).sum())
        assert on >= 1 and below >= 8 and (above >= 8 or thr == 1.0), (thr, on, below, above)
    A, B = R.near_thr_pairs(0.5)
    assert int(((B[:, 3] * 2 == A[:, 3]) & (B[:, 2] == A[:, 2])).sum()) >= 8          # IoU exactly 0.5, dyadic and scaled sides
    A, B = R.near_thr_pairs(0.0)
    inter, _, _ = R.inter_union_f32(A, B)
    assert (inter == 0).sum() >= 1 and ((inter > 0) & (inter < 1e-6)).sum() >= 1


THRS = (0.5, 0.3, 0.75, 0.0, 1.0)


def test_fast_predicate_equals_the_exact_one_near_the_threshold():
    for thr in THRS:
        A, B = R.near_thr_pairs(thr)
        for t in THRS:
            assert np.array_equal(R.suppresses_fast_f32(A, B, t), R.suppresses_f32(A, B, t)), (thr, t)
            assert np.array_equal(R.suppresses_fast_f32(B, A, t), R.suppresses_f32(B, A, t)), (thr, t)


def test_fast_predicate_equals_the_exact_one_on_random_pairs():
    rng = np.random.default_rng(5)
    n = 1000000
    scale = (10.0 ** rng.uniform(-21, 1, (n, 1))).astype(f32)          # down to areas that are float32 subnormals
    a = (rng.uniform(0, 1, (n, 4)).astype(f32) * scale).astype(f32)
    b = (a + (rng.normal(0, 0.2, (n, 4)).astype(f32) * scale).astype(f32)).astype(f32)
    _, _, _, _, area = R._norm(a)
    assert ((area > 0) & (area < 1.1754944e-38)).sum() > 1000
    for t in THRS:
        exact = R.suppresses_f32(a, b, t)
        assert np.array_equal(R.suppresses_fast_f32(a, b, t), exact), t
        assert 0 < exact.sum() < n or t == 1.0


def test_fast_predicate_equals_the_exact_one_on_denormal_units():
    """inter = i and u = j denormal units (2^-149), every combination up to 64: products with the threshold round to whole units"""
    unit = np.float64(2.0) ** -149
    i, j = np.meshgrid(np.arange(65), np.arange(1, 65), indexing="ij")
    inter, u = (i * unit).astype(f32), (j * unit).astype(f32)
    assert inter[1, 0] > 0
    for t in THRS + (0.1, 0.45, 0.6, 0.9):
        assert np.array_equal(R.decide_fast_f32(inter, u, t), R.decide_f32(inter, u, t)), t


def test_lds_scan_row_of_a_chunk_is_exact():
    """r = int((g + 0.5f) * (1 / CV)) == g // CV for every chunk count the planner admits ((CV | 1) * 16 * 64 <= 24 KB) and
    every chunk g of a wave's 64 rows"""
    admitted = [cv for cv in range(1, 200) if (cv | 1) * 16 * 64 <= 24 * 1024]
    assert admitted == list(range(1, 24))
    for cv in admitted:
        g = np.arange(64 * cv)
        assert np.array_equal(R.lds_row_of_chunk(g, cv), g // cv), cv


def test_adversarial_rows_hold_what_they_claim():
    for half in (False, True):
        rows = R.adversarial_rows(40, half)
        st = np.float16 if half else f32
        assert np.array_equal(rows, rows.astype(st).astype(np.float64))                       # exact in the storage type
        top = np.sort(rows, -1)[:, ::-1]
        assert ((top[:, 0] > 16) & (top[:, 1] > 16)).any() and (top[:, 0] == top[:, 1]).any() and (rows == -80).all(-1).any()
        one_ulp = top[:, 1] == np.nextafter(top[:, 0].astype(st), st(-np.inf)).astype(np.float64)
        assert one_ulp.sum() >= 8
        first = rows.argmax(-1)
        later = np.array([np.flatnonzero(r >= r.max() - 1e-3)[0] for r in rows])
        assert (later < first).any()              # a near-maximum in front of the maximum: the shortcut must look at it
