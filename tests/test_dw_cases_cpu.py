"""The case table of tests/dw_ref.py without a GPU: every case takes the branch of the depthwise host decision it was picked
for (read off the host-only rn_depthwise_plan: the library loads without a device, and the query returns what `decide` in
csrc/depthwise.hip -- the one function every rn_depthwise_* entry point launches from -- decided), and the table as a whole
reaches every value of the plan's enums, both grid caps and every layout edge listed in COVER.  A planner change that moves a
case off its branch fails here and says: pick another shape for that branch.  Further tests: the refusals (each beside the
nearest shape that is accepted, so that the bound itself is pinned) and the reference against its loop form.

A row is ((forward kernel, blocks), (dgrad variant, blocks), (weight-gradient chunks, pixels per chunk, workspace bytes) or
None, the fused backward's blocks, (statistics R, pixels per block, rows per sample, blocks) or None)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dw_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

GENERIC = (("generic", 1), ("generic", 1), None, 0, None)     # wgrad / bwd refuse k != 3, and so does the statistics kernel
EXPECT = {
    # 256 threads = (pixel, channel quad) each; chunks of about 2048 elements; statistics: 512 / (c / 4) pixel lanes x R
    "k3-s1-odd": (("k3", 16), ("k3", 16), (8, 64, 9216), 24, (4, 256, 1, 2)),
    "k3-s2-even": (("k3", 18), ("k3_parity", 72), (9, 15, 46656), 81, (4, 56, 2, 4)),
    "k3-s2-odd": (("k3", 4), ("k3_parity", 12), (2, 20, 6912), 14, (4, 84, 1, 2)),
    "k3-s3": (("k3", 1), ("k3", 1), (1, 12, 288), 2, (4, 1024, 1, 1)),
    "c4-1x1": (("k3", 1), ("k3", 1), (1, 2, 144), 2, (4, 2048, 1, 2)),
    "c4-row": (("k3", 1), ("k3_parity", 1), (1, 3, 144), 2, (4, 2048, 1, 1)),
    "c1024": (("k3", 30), ("k3", 30), (15, 2, 552960), 45, (4, 8, 4, 4)),
    "k5-s1": GENERIC,
    "k5-s2": GENERIC,
    "k1": GENERIC,
    "k2-s1": GENERIC,
    # 2 x 132 x 132 x 64 quads = 8712 blocks > 8192; 34848 pixels x 256 / 2048 = 4356 > 4096 chunks: 9 pixels each, 3872 chunks
    "grid-cap": (("k3", 8192), ("k3", 8192), (3872, 9, 35684352), 12064, (4, 32, 545, 1090)),
    "stats-r4-ragged": (("k3", 180), ("k3", 180), (87, 22, 300672), 267, (4, 84, 12, 24)),      # 957 pixels = 11 x 84 + 33
    "stats-r4-s2": (("k3", 18), ("k3_parity", 72), (9, 15, 46656), 81, (4, 56, 2, 4)),
    # two pixel lanes: 9216 / 8 = 1152 rows > 1024 -> R 8; 18496 / 16 = 1156 > 1024 -> R 16
    "stats-r8": (("k3", 8192), ("k3", 8192), (3072, 3, 113246208), 11264, (8, 16, 576, 576)),
    "stats-r16": (("k3", 8192), ("k3", 8192), (3700, 5, 136396800), 11892, (16, 32, 578, 578)),
}
# SAME geometry (oh, ow, pad before rows, pad before columns) of the cases picked for it
GEOMETRY = {"k3-s2-even": (8, 8, 0, 0), "k3-s2-odd": (5, 4, 1, 1), "k3-s3": (4, 3, 1, 0), "c4-1x1": (1, 1, 1, 1), "c4-row": (1, 3, 1, 1),
            "k5-s1": (9, 7, 2, 2), "k5-s2": (5, 5, 1, 2), "k1": (4, 5, 0, 0), "k2-s1": (5, 4, 0, 0)}
COVER = (["fwd %s" % k for k in ("k3", "generic")] + ["dgrad %s" % k for k in ("k3_parity", "k3", "generic")] +
         ["wgrad runs", "wgrad refuses", "stats declines"] + ["stats R%d" % r for r in (4, 8, 16)] +
         ["fwd grid cap", "dgrad grid cap", "wgrad chunk cap", "dgrad k3 stride 1", "dgrad k3 stride 3", "parity pad before 0", "parity pad before 1",
          "one quad", "one pixel", "one row", "wgrad one pixel lane", "stats two pixel lanes", "quads divide neither 256 nor 512",
          "ragged dgrad grid above 8", "ragged wgrad grid above 8", "ragged fwd grid above 8", "ragged stats grid above 8",
          "stats ragged last chunk", "stats at stride 2", "stats several rows per sample", "generic even kernel", "generic k 1", "generic stride 2",
          "several samples", "several grid-stride rounds"])


def _observe(name):
    case = R.CASES[name]
    st, plan = R.query(case)
    assert st == 0
    row = R.row_of(plan)
    (fwd, fwd_blocks), (dgrad, dgrad_blocks), wgrad, _, stats = row
    oh, ow = R.out_hw(case)
    quads = case.c // 4
    names = {"fwd %s" % fwd, "dgrad %s" % dgrad, "wgrad runs" if wgrad else "wgrad refuses"}
    names.add("stats R%d" % stats[0] if stats else "stats declines")
    if case.n * oh * ow * quads > 8192 * 256 and fwd_blocks == 8192:
        names.add("fwd grid cap")
    if case.n * case.h * case.w * quads > 8192 * 256 and dgrad_blocks == 8192:
        names.add("dgrad grid cap")
    if case.n * case.h * case.w * quads > 2 * 8192 * 256:
        names.add("several grid-stride rounds")
    if wgrad and -(-case.n * oh * ow * case.c // 2048) > 4096 and wgrad[1] == -(-case.n * oh * ow // 4096):
        names.add("wgrad chunk cap")
    if dgrad == "k3":
        names.add("dgrad k3 stride %d" % case.s)
    if dgrad == "k3_parity":
        names.add("parity pad before %d" % plan.pad_t)
    for flag, what in ((quads == 1, "one quad"), (case.h * case.w == 1, "one pixel"), (case.h == 1 and case.w > 1, "one row"),
                       (wgrad and 256 // quads == 1, "wgrad one pixel lane"), (stats and 512 // quads == 2, "stats two pixel lanes"),
                       (256 % quads and 512 % quads, "quads divide neither 256 nor 512"),
                       (dgrad_blocks > 8 and dgrad_blocks % 8, "ragged dgrad grid above 8"), (fwd_blocks > 8 and fwd_blocks % 8, "ragged fwd grid above 8"),
                       (wgrad and wgrad[0] > 8 and wgrad[0] % 8, "ragged wgrad grid above 8"), (stats and stats[3] > 8 and stats[3] % 8, "ragged stats grid above 8"),
                       (stats and (oh * ow) % stats[1] and stats[2] > 1, "stats ragged last chunk"), (stats and case.s == 2, "stats at stride 2"),
                       (stats and stats[2] > 1, "stats several rows per sample"), (fwd == "generic" and case.k % 2 == 0, "generic even kernel"),
                       (fwd == "generic" and case.k == 1, "generic k 1"), (fwd == "generic" and case.s == 2, "generic stride 2"),
                       (case.n > 1, "several samples")):
        if flag:
            names.add(what)
    return row, names, plan


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_its_branch(name):
    import _rn
    row, _, plan = _observe(name)
    assert row == EXPECT[name], "case %s left its branch: the planner now gives %s -- pick another shape for %s" % (name, row, EXPECT[name])
    case = R.CASES[name]
    oh, ow = R.out_hw(case)
    assert (plan.oh, plan.ow) == (oh, ow)
    assert (plan.pad_t, plan.pad_l) == (T.same_pad_1d(case.h, case.k, case.s)[1], T.same_pad_1d(case.w, case.k, case.s)[1])
    if name in GEOMETRY:
        assert (plan.oh, plan.ow, plan.pad_t, plan.pad_l) == GEOMETRY[name]
    L = _rn.lib()
    args = (case.n, case.h, case.w, case.c, case.k, case.s)
    # the stand-alone queries answer what the plan reports
    assert L.rn_depthwise_wgrad_workspace(*args) == plan.wgrad_workspace_bytes
    lay = _rn.GnRows()
    nbytes = L.rn_depthwise_stats_rows(*args, case.groups, C.byref(lay))
    if plan.stats_r:
        assert nbytes == plan.stats_blocks * case.groups * 8 and plan.stats_blocks == case.n * plan.stats_rows_per_sample
        assert (lay.rows_per_sample, lay.per_group, lay.groups) == (plan.stats_rows_per_sample, 1, case.groups)
        assert plan.stats_ppc == (512 // (case.c // 4)) * plan.stats_r and plan.stats_rows_per_sample == -(-oh * ow // plan.stats_ppc)
        assert L.rn_group_norm_rows_ok(case.c, case.groups, plan.stats_rows_per_sample, 1) == 1
    else:
        assert nbytes == 0
    if plan.wgrad_ok:
        assert plan.wgrad_chunks == -(-case.n * oh * ow // plan.wgrad_ppc) <= 4096          # the chunks cover the output pixels
        assert plan.wgrad_workspace_bytes == plan.wgrad_chunks * 9 * case.c * 4
        assert plan.bwd_blocks == plan.dgrad_blocks + plan.wgrad_chunks
    # a plan without a GroupNorm behind it differs in the statistics only
    st, bare = R.query(case, groups=0)
    assert st == 0 and R.row_of(bare)[:4] == EXPECT[name][:4] and bare.stats_r == 0


def test_table_covers_every_branch():
    assert sorted(EXPECT) == sorted(R.CASES)
    names = set()
    for name in R.CASES:
        names |= _observe(name)[1]
    missing = [b for b in COVER if b not in names]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


def test_table_shapes():
    for name, case in R.CASES.items():
        oh, ow = R.out_hw(case)
        assert R.elements(case) * 4 <= 80 << 20, name
        assert (R.elements(case) > 1 << 20) == (name in R.LARGE), name
    assert EXPECT[R.DEFER_CASE][2] is not None


def _plan(*args):
    import _rn
    plan = _rn.DwPlan()
    return _rn.lib().rn_depthwise_plan(*args, C.byref(plan)), plan


def _declines(n, h, w, c, k, s, groups):
    import _rn
    st, plan = _plan(n, h, w, c, k, s, groups)
    assert st == 0
    rows = _rn.lib().rn_depthwise_stats_rows(n, h, w, c, k, s, groups, None)
    assert (plan.stats_r == 0) == (rows == 0)
    return plan.stats_r == 0


def test_statistics_refusals():
    """Every bound of the statistics kernel, beside the nearest shape on its other side: the plan says R = 0 and
    rn_depthwise_stats_rows returns 0 exactly where the kernel's index arithmetic or the GroupNorm's merge gives out."""
    assert _declines(1, 1, 4100, 4, 3, 1, 4) and _declines(1, 1, 4097, 4, 3, 1, 4) and not _declines(1, 1, 4096, 4, 3, 1, 4)         # ow > 4096
    assert _declines(1, 1024, 1024, 4, 3, 1, 4) and not _declines(1, 1023, 1024, 4, 3, 1, 4)                                          # oh ow = 2^20
    assert _declines(1, 512, 512, 64, 3, 1, 1) and not _declines(1, 511, 512, 64, 3, 1, 1)                                            # oh ow cpg = 2^24
    assert _declines(1, 9, 7, 96, 3, 1, 36) and not _declines(1, 9, 7, 96, 3, 1, 32)                                                  # c % groups
    assert _declines(1, 9, 7, 96, 5, 1, 32) and _declines(1, 9, 7, 96, 1, 1, 32)                                                      # k != 3
    assert _declines(1, 9, 7, 96, 3, 1, 0)
    # a rows layout the GroupNorm refuses to merge: one group of 256 channels (slab wider than 128)
    import _rn
    assert _rn.lib().rn_group_norm_rows_ok(256, 1, 1, 1) == 0 and _rn.lib().rn_group_norm_rows_ok(256, 2, 1, 1) == 1
    assert _declines(1, 9, 7, 256, 3, 1, 1) and not _declines(1, 9, 7, 256, 3, 1, 2)
    # the launch refuses the same shapes before it touches a pointer's target (the host word stands for device memory)
    word = C.c_uint64(0)
    p = C.addressof(word)
    rows = _rn.GnRows(p, 1, 1, 32)
    assert _rn.lib().rn_depthwise_fwd_stats(p, p, p, 1, 9, 7, 96, 5, 1, C.byref(rows), None) == -2
    rows = _rn.GnRows(p, 1, 1, 36)
    assert _rn.lib().rn_depthwise_fwd_stats(p, p, p, 1, 9, 7, 96, 3, 1, C.byref(rows), None) == -2
    rows = _rn.GnRows(p, 2, 1, 32)                       # a layout other than the one rn_depthwise_stats_rows reports
    assert _rn.lib().rn_depthwise_fwd_stats(p, p, p, 1, 9, 7, 96, 3, 1, C.byref(rows), None) == -2
    rows = _rn.GnRows(p, 1, 0, 32)
    assert _rn.lib().rn_depthwise_fwd_stats(p, p, p, 1, 9, 7, 96, 3, 1, C.byref(rows), None) == -2
    assert _rn.lib().rn_depthwise_fwd_stats(p, p, p, 1, 9, 7, 96, 3, 1, None, None) == -1


def test_argument_refusals():
    import _rn
    L = _rn.lib()
    assert _plan(1, 9, 7, 96, 3, 1, 32)[0] == 0
    assert L.rn_depthwise_plan(1, 9, 7, 96, 3, 1, 32, None) == -1
    for bad in ((0, 9, 7, 96, 3, 1), (1, 0, 7, 96, 3, 1), (1, 9, 0, 96, 3, 1), (1, 9, 7, 0, 3, 1), (1, 9, 7, 96, 0, 1), (1, 9, 7, 96, 3, 0)):
        st, plan = _plan(*bad, 32)
        assert st == -1 and R.row_of(plan)[2:] == (None, 0, None) and plan.fwd_blocks == 0
    word = C.c_uint64(0)
    p = C.addressof(word)
    for bad in ((1, 9, 7, 98, 3, 1), (1, 9, 7, 1028, 3, 1), (1, 9, 7, 2048, 3, 1),                    # c % 4, c > 1024
                (1, 16384, 8192, 4, 3, 1), (2, 8192, 8192, 4, 3, 1), (1, 1024, 512, 1024, 3, 1)):     # 2^29 elements
        st, plan = _plan(*bad, 1)
        assert st == -2 and plan.fwd_blocks == 0, bad
        assert L.rn_depthwise_wgrad_workspace(*bad) == 0 and L.rn_depthwise_stats_rows(*bad, 1, None) == 0
        # every launch refuses alike, before it looks at a pointer
        assert L.rn_depthwise_fwd(p, p, p, *bad, None) == -2 and L.rn_depthwise_dgrad(p, p, p, *bad, None) == -2
        assert L.rn_depthwise_wgrad(p, p, p, *bad, p, 1 << 40, None, None) == -2
        assert L.rn_depthwise_bwd(p, p, p, p, p, *bad, p, 1 << 40, None, None) == -2
    assert _plan(1, 9, 7, 1024, 3, 1, 32)[0] == 0 and _plan(1, 16384, 8191, 4, 3, 1, 4)[0] == 0    # the nearest accepted shapes
    # k != 3: the weight gradient and the fused backward refuse (after the null check, before the workspace check)
    for k in (1, 2, 5):
        assert L.rn_depthwise_wgrad(p, p, p, 1, 9, 7, 8, k, 1, p, 0, None, None) == -2
        assert L.rn_depthwise_bwd(p, p, p, p, p, 1, 9, 7, 8, k, 1, p, 0, None, None) == -2
    assert L.rn_depthwise_wgrad(p, p, p, 1, 9, 7, 8, 3, 1, p, 0, None, None) == -4                   # (3x3: the workspace check)
    assert L.rn_depthwise_bwd(p, p, p, p, p, 1, 9, 7, 8, 3, 1, p, 0, None, None) == -4
    assert L.rn_depthwise_fwd(None, p, p, 1, 9, 7, 8, 3, 1, None) == -1


@pytest.mark.parametrize("shape", [(2, 5, 4, 4, 3, 2), (1, 4, 5, 4, 2, 1), (1, 6, 5, 4, 5, 2), (1, 7, 4, 4, 3, 3)])
def test_reference_is_its_loop_form(shape):
    """reference (padding + F.conv2d + autograd) in fp64 against loops over (output pixel, tap): y, dx and dw to fp64 rounding,
    at an odd and an even kernel, strides 1 to 3; and against the oracle's depthwise conv."""
    case = R._case(*shape)
    x, w, dy = R.make_case(case, seed=1)
    a, b = R.reference(x, w, dy, case.s, torch.float64), R.reference_loops(x, w, dy, case.s)
    for k in ("y", "dx", "dw"):
        assert a[k].shape == b[k].shape and rel_err(a[k], b[k]) < 1e-14, k
    assert rel_err(a["y"], T.depthwise_conv2d_same(x.double(), w.double().unsqueeze(3), case.s).numpy()) < 1e-15
    # the tap count of the bound is the loop's count
    taps = np.zeros((case.h, case.w))
    oh, pt, _ = T.same_pad_1d(case.h, case.k, case.s)
    ow, pl, _ = T.same_pad_1d(case.w, case.k, case.s)
    for i in range(oh):
        for j in range(ow):
            for p in range(case.k):
                for q in range(case.k):
                    if 0 <= i * case.s + p - pt < case.h and 0 <= j * case.s + q - pl < case.w:
                        taps[i * case.s + p - pt, j * case.s + q - pl] += 1
    assert np.array_equal(R.valid_taps(case), taps)


def test_statistic_rows_sum_to_the_moments():
    case = R.CASES["stats-r4-ragged"]
    y = R.small_case_data("stats-r4-ragged")[1]["y"]
    rows = R.stat_rows(y, case.groups, 84)
    assert rows.shape == (2, 12, 32, 2)
    yg = y.reshape(2, -1, 32, 3)
    assert rel_err(rows.sum(1)[..., 0], yg.sum((1, 3))) < 1e-13 and rel_err(rows.sum(1)[..., 1], (yg ** 2).sum((1, 3))) < 1e-13
    assert rel_err(rows[1, 11, 5, 0], yg[1, 11 * 84:, 5].sum()) < 1e-13                    # the ragged last chunk: 33 pixels
    # the bound's two parts: rounding of the sums (pixels x channels per group terms) and what the fp32 y passes on
    yb = np.full_like(y, 1e-6)
    b = R.stat_bounds(y, yb, case.groups, 84)
    for r, pixels in ((0, 84), (11, 33)):
        part = yg[:, r * 84:(r + 1) * 84]
        assert rel_err(b[:, r, :, 0], (pixels * 3 + 1) * R.U * np.abs(part).sum((1, 3)) + pixels * 3 * 1e-6) < 1e-12
        assert rel_err(b[:, r, :, 1], (pixels * 3 + 1) * R.U * (part ** 2).sum((1, 3)) + (2 * np.abs(part) * 1e-6 + 1e-12).sum((1, 3))) < 1e-12
