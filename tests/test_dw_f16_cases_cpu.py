"""The case table of tests/dw_f16_ref.py without a GPU: every case takes the kernel variant it was picked for (read off the
host-only rn_depthwise_f16_plan: the library loads without a device, and the query is the launch decision of
csrc/depthwise_f16.hip stopped before the launch), and the table as a whole reaches every template instantiation
(stride x strip width x input fold x statistics), strips one / two / four rows tall (whole and ragged at the bottom), one and
several chunks per sample, and strip counts below, at and one above a chunk.  Further: every refusal (fake pointers, no launch), rn_depthwise_f16_rows
against the plan, the reference's SAME padding against oracle.tf_ops_ref, and the header's declarations.

Rows (dw_f16_ref.row_of): (kernel, pixels per thread, pixel lanes, rows per thread, strips per sample, strips per chunk,
rows per sample, blocks, input fold, statistics)."""
import os
import re

import numpy as np
import pytest
import torch

import dw_f16_ref as R
import f16_conv_ref
from oracle import tf_ops_ref as T

EXPECT = {
    "c8-1x1": ('s1', 1, 256, 1, 1, 256, 1, 1, 0, 0),
    "c8-1x1-fold": ('s1', 1, 256, 1, 1, 256, 1, 3, 1, 0),
    "c24-2x3": ('s1', 1, 85, 1, 6, 85, 1, 3, 1, 1),
    "c24-2x1-s2": ('s2', 1, 85, 1, 1, 85, 1, 1, 1, 1),
    "c32-5x2-s2": ('s2', 1, 64, 1, 3, 64, 1, 3, 0, 0),
    "c32-5x2-s2-fold": ('s2', 1, 64, 1, 3, 64, 1, 1, 1, 0),
    "c96-3x1-s2": ('s2', 1, 21, 1, 2, 21, 1, 1, 0, 1),
    "c96-3x3": ('s1', 1, 21, 1, 9, 21, 1, 1, 0, 1),
    "c24-2x3-s2": ('s2', 2, 85, 1, 1, 85, 1, 1, 1, 1),
    "c960-5x7-s2": ('s2', 2, 2, 1, 6, 2, 3, 3, 1, 1),
    "c24-5x7": ('s1', 4, 85, 1, 10, 85, 1, 1, 1, 1),
    "c32-9x12": ('s1', 4, 64, 2, 15, 64, 1, 3, 1, 1),
    "c32-9x12-s2": ('s2', 2, 64, 1, 15, 64, 1, 1, 0, 0),
    "c96-16x16": ('s1', 4, 21, 2, 32, 21, 2, 2, 1, 1),
    "c96-16x16-s2": ('s2', 2, 21, 2, 16, 21, 1, 3, 1, 1),
    "c144-33x17": ('s1', 4, 14, 4, 45, 14, 4, 4, 1, 1),
    "c144-33x17-s2": ('s2', 2, 14, 2, 45, 14, 4, 12, 1, 1),
    "c144-33x17-nostats": ('s1', 4, 14, 4, 45, 14, 4, 4, 1, 0),
    "c960-5x7": ('s1', 4, 2, 1, 10, 2, 5, 5, 1, 1),
    "c960-16x16-s2": ('s2', 2, 2, 2, 16, 2, 8, 24, 1, 1),
    "c96-3x3-s2": ('s2', 2, 21, 1, 2, 21, 1, 1, 0, 1),
    "c32-5x6-s2": ('s2', 2, 64, 1, 6, 64, 1, 3, 0, 0),
    "c32-9x12-plain": ('s1', 4, 64, 2, 15, 64, 1, 1, 0, 0),
    "c96-16x16-s2-nostats": ('s2', 2, 21, 2, 16, 21, 1, 1, 1, 0),
    "c144-33x17-s2-plain": ('s2', 2, 14, 2, 45, 14, 4, 4, 0, 1),
    "c8-64x65": ('s1', 4, 256, 4, 272, 256, 2, 2, 1, 1),
    "chunk-below": ('s1', 4, 2, 1, 1, 2, 1, 1, 0, 1),
    "chunk-at": ('s1', 4, 2, 1, 2, 2, 1, 3, 1, 1),
    "chunk-above": ('s1', 4, 2, 1, 3, 2, 2, 2, 0, 1),
}


def test_table_and_expectations_name_the_same_cases():
    assert list(R.CASES) == list(EXPECT)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_its_variant(name):
    case = R.CASES[name]
    plan = R.query(R.descriptor(case))
    assert R.row_of(plan) == EXPECT[name], "%s: the plan moved; pick another shape for this row" % name
    # the geometry and the derived fields
    oh, pt, _ = T.same_pad_1d(case.h, 3, case.stride)
    ow, pl, _ = T.same_pad_1d(case.w, 3, case.stride)
    assert (plan.oh, plan.ow, plan.pad_t, plan.pad_l) == (oh, ow, pt, pl)
    wide = 4 if case.stride == 1 else 2
    assert plan.pixels_per_thread == (wide if ow >= wide else 1)
    assert plan.rows_per_thread == (4 if oh >= 32 else 2 if oh >= 8 else 1)
    assert plan.pixel_lanes == 256 // (case.c // 8)
    assert plan.strips_per_sample == -(-oh // plan.rows_per_thread) * -(-ow // plan.pixels_per_thread)
    assert plan.strips_per_chunk == plan.pixel_lanes
    assert plan.pixels_per_chunk == plan.strips_per_chunk * plan.pixels_per_thread * plan.rows_per_thread
    assert plan.rows_per_sample == -(-plan.strips_per_sample // plan.strips_per_chunk)
    assert plan.blocks == case.n * plan.rows_per_sample
    assert (plan.fold, plan.stats) == (int(case.fold), int(case.stats))
    import _rn
    assert _rn.lib().rn_depthwise_f16_rows(case.n, case.h, case.w, case.c, case.stride) == plan.rows_per_sample


def test_table_reaches_every_variant():
    rows = list(EXPECT.values())
    variants = {(r[0], r[1], r[8], r[9]) for r in rows}
    assert variants == {(k, p, f, s) for k, ps in (('s1', (1, 4)), ('s2', (1, 2))) for p in ps for f in (0, 1) for s in (0, 1)}
    assert {r[3] for r in rows} == {1, 2, 4}                       # rows per thread ...
    ragged = {r[3] for n, r in EXPECT.items() if -(-R.CASES[n].h // R.CASES[n].stride) % r[3]}
    assert ragged == {2, 4}                                        # ... with a last strip that is not whole
    assert any(r[6] > 1 for r in rows) and any(r[6] == 1 for r in rows)
    assert any(256 % (R.CASES[n].c // 8) for n in EXPECT)          # idle threads in a block
    below, at, above = EXPECT["chunk-below"], EXPECT["chunk-at"], EXPECT["chunk-above"]
    assert below[4] < below[5] and below[6] == 1
    assert at[4] == at[5] and at[6] == 1
    assert above[4] == above[5] + 1 and above[6] == 2
    cases = R.CASES.values()
    assert {c.c for c in cases} >= {8, 24, 32, 96, 144, 960}
    assert {(c.h, c.w) for c in cases} >= {(1, 1), (2, 3), (5, 7), (9, 12), (16, 16), (33, 17)}
    assert {c.n for c in cases} >= {1, 3}
    assert {c.act for c in cases if c.fold} == set(R.ACTS) and any(not c.fold for c in cases)
    assert {c.c // c.groups for c in cases if c.fold} >= {1, 3, 6, 30}
    s2 = [c for c in cases if c.stride == 2]
    assert {(c.h % 2, c.w % 2) for c in s2} >= {(0, 0), (1, 1), (0, 1), (1, 0)}


@pytest.mark.parametrize("name", list(R.REFUSALS))
def test_refusal(name):
    over, status = R.REFUSALS[name]
    R.query(R.descriptor(R.REFUSAL_BASE), 0)
    plan = R.query(R.descriptor(R.REFUSAL_BASE, **over), status)
    assert R.row_of(plan) == (None, 0, 0, 0, 0, 0, 0, 0, 0, 0)      # a refused call's plan is zeroed
    import _rn
    assert _rn.lib().rn_last_error().decode().startswith("depthwise f16")


def test_refusals_of_the_entry_points_without_a_descriptor():
    import ctypes as C
    import _rn
    L = _rn.lib()
    plan = _rn.DwF16Plan()
    assert L.rn_depthwise_f16_plan(None, C.byref(plan)) == R.EINVAL
    assert L.rn_depthwise_f16_plan(C.byref(R.descriptor(R.REFUSAL_BASE)), None) == R.EINVAL
    assert L.rn_depthwise_fwd_f16(None, None) == R.EINVAL
    # the launch entry refuses before it launches: no device is touched here
    for name, (over, status) in R.REFUSALS.items():
        assert L.rn_depthwise_fwd_f16(C.byref(R.descriptor(R.REFUSAL_BASE, **over)), None) == status, name
    assert L.rn_depthwise_f16_rows(2, 9, 12, 12, 1) == 0 and L.rn_depthwise_f16_rows(2, 9, 12, 96, 3) == 0


@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 1), (1, 6, 9, 16, 2), (3, 7, 4, 8, 2)])
def test_reference_padding_is_the_oracles(shape):
    n, h, w, c, stride = shape
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, h, w, c))
    k = rng.standard_normal((3, 3, c))
    want = T.depthwise_conv2d_same(torch.from_numpy(x), torch.from_numpy(k).reshape(3, 3, c, 1), stride).numpy()
    got = R.dwconv(x, k, stride)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_fold_operand_generalises_the_convs_reference():
    """fold_operand_g with f16_conv_ref's four groups and its two activations is f16_conv_ref.fold_operand"""
    rng = np.random.default_rng(9)
    x = R.flush16(2.0 * rng.standard_normal((2, 3, 5, 16), dtype=np.float32) + 0.3)
    g = f16_conv_ref.IN_GROUPS
    gn = ((0.3 + 0.1 * rng.standard_normal((2, g))).astype(np.float32), (0.5 + 0.1 * rng.random((2, g))).astype(np.float32),
          (1.0 + 0.3 * rng.standard_normal(16)).astype(np.float32), (0.5 + 0.2 * rng.standard_normal(16)).astype(np.float32))
    for kind in ("relu", "elu"):
        for dtype in (np.float32, np.float64):
            for fused in (False, True):
                assert np.array_equal(R.fold_operand_g(x, gn, g, kind, dtype, fused), R.fold_operand(x, gn, kind, dtype, fused))


def test_reference_zero_padding_after_the_activation_shows():
    """with beta != 0 a reference that padded BEFORE the activation differs at the borders and nowhere else"""
    case = R.CASES["c24-5x7"]
    x, w, gn = R.make_case(case)
    ref = R.run_ref(case)
    padded_first = np.zeros((case.n, case.h + 2, case.w + 2, case.c), np.float16)
    padded_first[:, 1:-1, 1:-1] = x
    a = R.fold_operand_g(padded_first, gn, case.groups, case.act, np.float64).astype(np.float64)
    k = torch.from_numpy(w.astype(np.float64)).reshape(3, 3, 1, case.c)
    wrong = torch.nn.functional.conv2d(torch.from_numpy(a).permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), groups=case.c).permute(0, 2, 3, 1).numpy()
    d = np.abs(wrong - ref.y64) > R.element_bound(ref)
    assert d[:, 0].any() and d[:, -1].any() and d[:, :, 0].any() and d[:, :, -1].any() and not d[:, 1:-1, 1:-1].any()


def test_header_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rn_hip.h")).read()
    for decl in (r"int rn_depthwise_f16_rows\(int n, int h, int w, int c, int stride\);",
                 r"int rn_depthwise_fwd_f16\(const rn_dw_f16\* d, rn_stream_t stream\);",
                 r"int rn_depthwise_f16_plan\(const rn_dw_f16\* d, rn_dw_f16_plan\* plan\);",
                 r"typedef struct rn_dw_f16 \{", r"\} rn_dw_f16_plan;"):
        assert re.search(decl, hdr), decl
    comment = hdr[hdr.index("fp16 inference depthwise 3x3"):hdr.index("typedef struct rn_dw_f16 {")]
    assert "mobilenet_v2.py:15-38" in comment and "normalization.py" in comment        # the reference call sites
    import _rn
    for name in ("rn_depthwise_f16_rows", "rn_depthwise_fwd_f16", "rn_depthwise_f16_plan"):
        assert name in _rn.SYMBOLS and hasattr(_rn.lib(), name)
