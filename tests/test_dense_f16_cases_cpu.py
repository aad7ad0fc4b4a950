"""The tables of tests/dense_f16_ref.py without a GPU, read off the host-only rn_dense_f16_plan (the launch decision of
csrc/dense_f16.hip stopped before the launch; the library loads without a device): rows is a function of hw alone, every call of
every table takes the launch its row says, the fifth table has three rows per sample with a ragged last one, every refusal returns
its status and launches nothing (fake pointers, NULL stream), the header declares the entries, and the identity the pool-first
transition rests on holds in fp64.

Rows (dense_f16_ref.plan_row): (op, vector width, chunk, rows, octets per block, lanes, grid x, y, z, threads); op 1 put, 2 finalize,
3 norm."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dense_f16_ref as R
from oracle import tf_ops_ref as T

_HOST_WORDS = (C.c_uint64 * 4)()
FAKE = (C.addressof(_HOST_WORDS) + 15) & ~15       # 16-byte aligned, never followed: every call below is refused before a launch

# per table: put of the block's input, put of a growth slice (the first), finalize and norm of the LAST layer's prefix
EXPECT = {
    "t16x16": [(1, 8, 256, 1, 8, 32, 1, 2, 1, 256), (1, 8, 256, 1, 4, 64, 1, 2, 1, 256), (2, 1, 256, 1, 0, 0, 32, 2, 1, 256), (3, 8, 256, 1, 0, 0, 5, 2, 1, 256)],
    "t19x25": [(1, 8, 256, 2, 8, 32, 2, 2, 1, 256), (1, 8, 256, 2, 4, 64, 2, 2, 1, 256), (2, 1, 256, 2, 0, 0, 32, 2, 1, 256), (3, 8, 256, 2, 0, 0, 8, 2, 1, 256)],
    "t8x8": [(1, 8, 256, 1, 32, 8, 1, 1, 4, 256), (1, 8, 256, 1, 4, 64, 1, 1, 1, 256), (2, 1, 256, 1, 0, 0, 32, 1, 1, 256), (3, 8, 256, 1, 0, 0, 8, 1, 1, 256)],
    "t5x7": [(1, 8, 256, 1, 16, 16, 1, 3, 1, 256), (1, 8, 256, 1, 4, 64, 1, 3, 1, 256), (2, 1, 256, 1, 0, 0, 32, 3, 1, 256), (3, 8, 256, 1, 0, 0, 1, 3, 1, 256)],
    "t23x25": [(1, 8, 256, 3, 8, 32, 3, 1, 1, 256), (1, 8, 256, 3, 4, 64, 3, 1, 1, 256), (2, 1, 256, 3, 0, 0, 32, 1, 1, 256), (3, 8, 256, 3, 0, 0, 7, 1, 1, 256)],
}


def _rows_of_table(name):
    t = R.TABLES[name]
    hw, ld = t.h * t.w, R.table_ld(t)
    last = R.prefixes(t)[-2]
    return [R.plan_row(R.plan("put", t.n, hw, t.c_in, ld)), R.plan_row(R.plan("put", t.n, hw, R.GROWTH, ld, t.c_in)),
            R.plan_row(R.plan("finalize", t.n, hw, last, ld, 0, R.GROUPS)), R.plan_row(R.plan("norm", t.n, hw, last, ld, 0, R.GROUPS))]


def test_tables_and_expectations_name_the_same_cases():
    assert list(R.TABLES) == list(EXPECT)
    assert [tuple(R.TABLES[k]) for k in R.TABLES] == [(2, 16, 16, 64, 4), (2, 19, 25, 64, 3), (1, 8, 8, 992, 2), (3, 5, 7, 128, 2), (1, 23, 25, 64, 2)]
    assert set(R.BLOCK_TABLES) == set(list(R.TABLES)[:4])


@pytest.mark.parametrize("name", list(R.TABLES))
def test_table_takes_its_launches(name):
    assert _rows_of_table(name) == EXPECT[name], "%s: the plan moved" % name
    t = R.TABLES[name]
    hw, ld = t.h * t.w, R.table_ld(t)
    import _rn
    rows = _rn.lib().rn_dense_f16_rows(hw)
    for i, c in enumerate(R.prefixes(t)):
        # every slice and every prefix of the block: one row count, one chunk length; the derived fields
        for p in ([R.plan("put", t.n, hw, R.GROWTH, ld, c)] if i < t.depth else []) + [R.plan("finalize", t.n, hw, c, ld, 0, R.GROUPS),
                                                                                       R.plan("norm", t.n, hw, c, ld, 0, R.GROUPS)]:
            assert p.rows == rows == -(-hw // p.chunk) and p.threads == 256
        assert c % R.GROUPS == 0
    p = R.plan("put", t.n, hw, t.c_in, ld)
    assert p.octets_per_block * p.lanes == p.threads and p.octets_per_block <= 32 and p.grid_z == -(-(t.c_in // 8) // p.octets_per_block)
    assert (p.grid_x, p.grid_y) == (rows, t.n) and p.vec == 8


def test_tables_reach_what_they_were_picked_for():
    group_sizes = {name: [c // R.GROUPS for c in R.prefixes(R.TABLES[name])] for name in R.TABLES}
    assert group_sizes["t16x16"] == [2, 3, 4, 5, 6] and group_sizes["t8x8"] == [31, 32, 33] and R.table_ld(R.TABLES["t8x8"]) == 1056
    chunk = R.plan("put", 1, 1, 8, 8).chunk
    hw = {name: R.TABLES[name].h * R.TABLES[name].w for name in R.TABLES}
    assert hw["t19x25"] == 475 and hw["t19x25"] % chunk and hw["t19x25"] > chunk           # a ragged last chunk
    assert hw["t5x7"] < chunk and R.TABLES["t5x7"].n == 3                                   # fewer pixels than one chunk
    p = R.plan("put", 1, hw["t23x25"], R.GROWTH, R.table_ld(R.TABLES["t23x25"]), 64)
    assert p.rows >= 3 and hw["t23x25"] % p.chunk and p.rows == -(-hw["t23x25"] // p.chunk)   # three rows, the last one ragged
    assert any(R.TABLES[n].c_in // 8 > 32 for n in R.TABLES)                                # a put spanning several octet blocks ...
    assert 992 // 8 % 32                                                                    # ... with idle threads in the last one


@pytest.mark.parametrize("hw", [1, 35, 64, 255, 256, 257, 475, 575, 4096, 25600])
def test_rows_is_a_function_of_hw_alone(hw):
    import _rn
    rows = _rn.lib().rn_dense_f16_rows(hw)
    chunk = R.plan("put", 1, hw, 8, 8).chunk
    assert rows == -(-hw // chunk)
    seen = set()
    for n in (1, 3):
        for c, ld, coff in ((8, 8, 0), (32, 96, 64), (992, 1056, 0), (64, 192, 128)):
            seen.add(R.plan("put", n, hw, c, ld, coff).rows)
            if coff == 0:
                seen.add(R.plan("finalize", n, hw, c, ld, 0, 8).rows)
                seen.add(R.plan("norm", n, hw, c, ld, 0, 8).rows)
    assert seen == {rows}
    assert _rn.lib().rn_dense_f16_rows(0) == 0 and _rn.lib().rn_dense_f16_rows(-3) == 0


REFUSALS = [
    # (op, n, hw, c, ld, coff, groups, status)
    ("put c % 8", ("put", 2, 64, 12, 96, 0, 1), R.EUNSUPPORTED),
    ("put ld < coff + c", ("put", 2, 64, 32, 96, 72, 1), R.EINVAL),
    ("put ld % 8", ("put", 2, 64, 32, 100, 64, 1), R.EUNSUPPORTED),
    ("put coff % 8", ("put", 2, 64, 32, 96, 4, 1), R.EUNSUPPORTED),
    ("put n = 0", ("put", 0, 64, 32, 96, 0, 1), R.EINVAL),
    ("put hw = 0", ("put", 2, 0, 32, 96, 0, 1), R.EINVAL),
    ("put coff < 0", ("put", 2, 64, 32, 96, -8, 1), R.EINVAL),
    ("finalize c % 8", ("finalize", 2, 64, 36, 96, 0, 4), R.EUNSUPPORTED),
    ("finalize ld < c", ("finalize", 2, 64, 128, 96, 0, 32), R.EINVAL),
    ("finalize ld % 8", ("finalize", 2, 64, 64, 100, 0, 32), R.EUNSUPPORTED),
    ("finalize groups", ("finalize", 2, 64, 64, 96, 0, 5), R.EINVAL),
    ("finalize coff", ("finalize", 2, 64, 32, 96, 32, 32), R.EINVAL),
    ("norm c % 8", ("norm", 2, 64, 36, 96, 0, 4), R.EUNSUPPORTED),
    ("norm ld < c", ("norm", 2, 64, 128, 96, 0, 32), R.EINVAL),
    ("norm ld % 8", ("norm", 2, 64, 64, 100, 0, 32), R.EUNSUPPORTED),
    ("norm groups", ("norm", 2, 64, 64, 96, 0, 0), R.EINVAL),
    ("norm c > 2048", ("norm", 2, 64, 2080, 2112, 0, 32), R.EUNSUPPORTED),
]


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_refusal(name):
    import _rn
    L = _rn.lib()
    (op, n, hw, c, ld, coff, groups), status = [(r[1], r[2]) for r in REFUSALS if r[0] == name][0]
    p = R.plan(op, n, hw, c, ld, coff, groups, status)
    assert R.plan_row(p) == (0,) * 10                                # a refused call's plan is zeroed
    assert L.rn_last_error().decode().startswith("dense f16")
    # the launch entry refuses with the same status before it launches: fake pointers, no device is touched
    if op == "put":
        got = L.rn_dense_f16_put(FAKE, FAKE, FAKE, n, hw, c, ld, coff, None)
    elif coff != 0:
        return                                                       # (finalize / norm have no coff argument)
    elif op == "finalize":
        got = L.rn_dense_f16_finalize(FAKE, n, hw, c, ld, groups, 1e-5, FAKE, FAKE, None)
    else:
        got = L.rn_dense_f16_norm(FAKE, FAKE, n, hw, c, ld, groups, FAKE, FAKE, FAKE, FAKE, 2, None)
    assert got == status


def test_refusals_of_null_pointers_and_unknown_values():
    import _rn
    L = _rn.lib()
    ok = (2, 64, 32, 96)
    assert L.rn_dense_f16_plan(1, *ok, 64, 1, None) == R.EINVAL
    assert L.rn_dense_f16_plan(0, *ok, 64, 1, C.byref(_rn.DenseF16Plan())) == R.EINVAL
    assert L.rn_dense_f16_plan(4, *ok, 64, 1, C.byref(_rn.DenseF16Plan())) == R.EINVAL
    for ptrs in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None), (FAKE + 8, FAKE, FAKE), (FAKE, FAKE + 2, FAKE), (FAKE, FAKE, FAKE + 4)):
        assert L.rn_dense_f16_put(*ptrs, *ok, 64, None) == R.EINVAL
    for ptrs in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert L.rn_dense_f16_finalize(ptrs[0], 2, 64, 64, 96, 32, 1e-5, ptrs[1], ptrs[2], None) == R.EINVAL
    for i in range(6):
        ptrs = [FAKE] * 6
        ptrs[i] = None
        assert L.rn_dense_f16_norm(ptrs[0], ptrs[1], 2, 64, 64, 96, 32, *ptrs[2:], 2, None) == R.EINVAL
    assert L.rn_dense_f16_norm(FAKE, FAKE, 2, 64, 64, 96, 32, FAKE, FAKE, FAKE, FAKE, 7, None) == R.EINVAL      # unknown activation


def test_avgpool_refusals():
    import _rn
    L = _rn.lib()
    gn = (FAKE, FAKE, FAKE, FAKE, 8, 0)
    none = (None, None, None, None, 0, 0)
    for k, s in ((3, 2), (2, 1), (1, 1), (2, 3), (3, 3)):
        assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 32, k, s, *none, None) == R.EUNSUPPORTED
        assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 32, k, s, *gn, None) == R.EUNSUPPORTED
    assert L.rn_last_error().decode().startswith("avgpool gn fwd f16")
    assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 12, 2, 2, *none, None) == R.EUNSUPPORTED          # c % 8
    assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 2056, 2, 2, *gn, None) == R.EUNSUPPORTED          # c > 2048 behind a GroupNorm
    assert L.rn_avgpool_gn_fwd_f16(None, FAKE, 2, 8, 8, 32, 2, 2, *none, None) == R.EINVAL
    assert L.rn_avgpool_gn_fwd_f16(FAKE, None, 2, 8, 8, 32, 2, 2, *none, None) == R.EINVAL
    assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 0, 8, 8, 32, 2, 2, *none, None) == R.EINVAL
    assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 32, 2, 2, FAKE, None, FAKE, FAKE, 8, 0, None) == R.EINVAL     # a GroupNorm given partly
    assert L.rn_avgpool_gn_fwd_f16(FAKE, FAKE, 2, 8, 8, 32, 2, 2, FAKE, FAKE, FAKE, FAKE, 5, 0, None) == R.EINVAL     # groups do not divide c


def test_pool_first_identity_in_fp64():
    """avgpool(conv1x1(GN(x))) == conv1x1(avgpool(GN(x))) on a 5 x 7 map: both axes odd, so the edge windows average 2 cells and the
    corner window 1 -- the pool's weights sum to 1 in every window, which is all the identity needs"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, 64, generator=g, dtype=torch.float64)
    gamma, beta = 1 + 0.3 * torch.randn(64, generator=g, dtype=torch.float64), 0.2 * torch.randn(64, generator=g, dtype=torch.float64)
    w = torch.randn(1, 1, 64, 32, generator=g, dtype=torch.float64) / 8
    gn = T.group_norm(x, gamma, beta, 32, 1e-5)
    conv_first = T.avg_pool_same(T.conv2d_same(gn, w, 1), 2, 2)
    pool_first = T.conv2d_same(T.avg_pool_same(gn, 2, 2), w, 1)
    assert conv_first.shape == pool_first.shape == (2, 3, 4, 32)
    assert float((conv_first - pool_first).abs().max()) <= 1e-13 * float(conv_first.abs().max())
    # ... and the reference pool of this file is the oracle's
    got, cnt = R.avg_pool_np(gn.numpy())
    assert np.abs(got - T.avg_pool_same(gn, 2, 2).numpy()).max() <= 1e-13
    assert sorted(set(cnt.reshape(-1).tolist())) == [1.0, 2.0, 4.0]


def test_pool_shapes_are_the_issues():
    assert [v[:4] for v in R.POOL_SHAPES.values()] == [(2, 16, 16, 64), (1, 5, 7, 32), (3, 19, 25, 8), (1, 1, 1, 64), (1, 2, 3, 40), (2, 6, 6, 96)]
    assert R.POOL_SHAPES["2x6x6x96"][4] == 32 and 96 // 32 == 3


def test_header_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rn_hip.h")).read()
    for decl in (r"int rn_dense_f16_rows\(int hw\);",
                 r"int rn_dense_f16_put\(const void\* src, void\* buf, float\* partial, int n, int hw, int c, int ld, int coff, rn_stream_t stream\);",
                 r"int rn_dense_f16_finalize\(const float\* partial, int n, int hw, int c, int ld, int groups, float eps, float\* mean, float\* rstd,",
                 r"int rn_dense_f16_norm\(const void\* buf, void\* y, int n, int hw, int c, int ld, int groups, const float\* mean, const float\* rstd,",
                 r"int rn_dense_f16_plan\(int op, int n, int hw, int c, int ld, int coff, int groups, rn_dense_plan\* plan\);",
                 r"int rn_avgpool_gn_fwd_f16\(const void\* x, void\* y, int n, int h, int w, int c, int k, int stride, const float\* mean, const float\* rstd,"):
        assert re.search(decl, hdr), decl
    comment = hdr[hdr.index("fp16 inference dense block"):hdr.index("int rn_dense_f16_rows(int hw);")]
    assert "densenet.py:117-121" in comment and "normalization.py" in comment          # the reference call sites
    import _rn
    for name in ("rn_dense_f16_rows", "rn_dense_f16_put", "rn_dense_f16_finalize", "rn_dense_f16_norm", "rn_dense_f16_plan", "rn_avgpool_gn_fwd_f16"):
        assert name in _rn.SYMBOLS and hasattr(_rn.lib(), name)
    assert C.sizeof(_rn.DenseF16Plan) == 40
