"""The fp16 inference DenseNet kernels (csrc/dense_f16.hip) against fp64 of the same stored fp16 values, on the tables and with the
bounds of tests/dense_f16_ref.py (derived there; tests/test_dense_f16_cases_cpu.py proves which launch every call takes).

  * rn_avgpool_gn_fwd_f16, plain and behind a GroupNorm (no activation, ELU): every output element within pool_bound; the folded
    mode bit-equal to rn_group_norm_apply_f16 followed by the plain pool;
  * rn_dense_f16_put slice by slice into a sentinel-filled buffer and table: the slice bit-equal to its source, every other byte of
    both unchanged, the table's rows within the fp32-sum bound; rn_dense_f16_finalize of every prefix within stat_bounds;
    rn_dense_f16_norm of every prefix within norm_bound (ELU for the layers' prefixes, no activation for the whole buffer: the
    transition's GroupNorm).
`pytest -s` prints each case's worst ratio to its bound (DENSE_F16 lines; profiles/dense_f16_err.txt)."""
import numpy as np
import pytest
import torch

import dense_f16_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("mode", R.POOL_MODES)
@pytest.mark.parametrize("name", list(R.POOL_SHAPES))
def test_avg_pool(dev, name, mode):
    import _rn, ops_f16
    n, h, w, c, groups = R.POOL_SHAPES[name]
    x, gn = R.pool_case(name)
    ref = R.pool_ref(name, mode)
    xd = _t(x, dev)
    if mode == "plain":
        got = ops_f16.avg_pool(xd)
    else:
        act = None if mode == "gn-none" else "elu"
        mean, rstd, gamma, beta = [_t(a, dev) for a in gn]
        got = ops_f16.avg_pool_norm(ops_f16.Pending(xd, mean, rstd, gamma, beta, groups, act))
        applied = torch.empty_like(xd)
        _rn.check(_rn.lib().rn_group_norm_apply_f16(_rn.f16(xd), None, _rn.f16(applied), n, h * w, c, groups, _rn.f32(mean), _rn.f32(rstd),
                                                    _rn.f32(gamma), _rn.f32(beta), _rn.ACT[act], 0, _rn.stream()), "rn_group_norm_apply_f16")
        assert torch.equal(got, ops_f16.avg_pool(applied)), "folded pool != apply pass + plain pool"
    assert got.dtype == torch.float16 and tuple(got.shape) == ref.y64.shape == (n, -(-h // 2), -(-w // 2), c)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.y64)
    ratio = float((err / ref.bound).max())
    print("DENSE_F16 pool %-11s %-8s worst element %.3f of its bound" % (name, mode, ratio))
    assert ratio <= 1.0


SENT16 = 0x5A5A          # the int16 pattern of untouched buffer halfs
SENT32 = -777.25         # the value of untouched table floats


@pytest.mark.parametrize("name", list(R.TABLES))
def test_put_finalize_norm(dev, name):
    import _rn
    L = _rn.lib()
    t = R.TABLES[name]
    n, hw, ld = t.n, t.h * t.w, R.table_ld(t)
    slices, params = R.table_data(name)
    chunk = R.plan("put", n, hw, t.c_in, ld).chunk
    rows = L.rn_dense_f16_rows(hw)
    buf = torch.full((n, hw, ld), SENT16, dtype=torch.int16, device=dev).view(torch.float16)
    table = torch.full((2, n, rows, ld), SENT32, dtype=torch.float32, device=dev)
    want_buf = np.full((n, hw, ld), SENT16, np.int16)
    want_tab = np.full((2, n, rows, ld), SENT32, np.float64)
    tol_tab = np.zeros((2, n, rows, ld))
    p = min(chunk, hw)
    g = (p - 1) * R.U / (1.0 - (p - 1) * R.U)
    coff, worst = 0, {"row": 0.0, "mean": 0.0, "rstd": 0.0, "norm": 0.0}
    for i, sl in enumerate(slices):
        c = sl.shape[2]
        src = _t(sl, dev)
        _rn.check(L.rn_dense_f16_put(_rn.f16(src), _rn.f16(buf), _rn.f32(table), n, hw, c, ld, coff, _rn.stream()), "rn_dense_f16_put")
        want_buf[:, :, coff:coff + c] = sl.view(np.int16)
        s1, s2, sa = R.row_sums(sl, chunk)
        want_tab[0, :, :, coff:coff + c], want_tab[1, :, :, coff:coff + c] = s1, s2
        tol_tab[0, :, :, coff:coff + c], tol_tab[1, :, :, coff:coff + c] = g * sa, g * s2
        coff += c
        # the slice is bit-equal to its source, every other byte of the buffer is what it was
        assert np.array_equal(buf.view(torch.int16).cpu().numpy(), want_buf), "slice %d: buffer bytes" % i
        got_tab = table.cpu().numpy().astype(np.float64)
        assert np.array_equal(got_tab[:, :, :, coff:], want_tab[:, :, :, coff:]), "slice %d: table entries outside the slices written" % i
        d = np.abs(got_tab[:, :, :, :coff] - want_tab[:, :, :, :coff])
        assert (d <= tol_tab[:, :, :, :coff]).all(), "slice %d: table rows" % i
        worst["row"] = max(worst["row"], float((d / np.maximum(tol_tab[:, :, :, :coff], 1e-300)).max()))
        # the prefix [0, coff): statistics and the normalised operand
        prefix = np.concatenate(slices[:i + 1], 2)
        st = R.stat_bounds(prefix, R.GROUPS, chunk)
        mean = torch.empty((n, R.GROUPS), dtype=torch.float32, device=dev)
        rstd = torch.empty((n, R.GROUPS), dtype=torch.float32, device=dev)
        _rn.check(L.rn_dense_f16_finalize(_rn.f32(table), n, hw, coff, ld, R.GROUPS, R.EPS, _rn.f32(mean), _rn.f32(rstd), _rn.stream()),
                  "rn_dense_f16_finalize")
        rm = float((np.abs(mean.cpu().numpy().astype(np.float64) - st.mean) / st.dm).max())
        rr = float((np.abs(rstd.cpu().numpy().astype(np.float64) - st.rstd) / st.dr).max())
        assert rm <= 1.0 and rr <= 1.0, "prefix %d: mean %.3f / rstd %.3f of the bound" % (coff, rm, rr)
        worst["mean"], worst["rstd"] = max(worst["mean"], rm), max(worst["rstd"], rr)
        gamma, beta = params[i]
        gamma_d, beta_d = _t(gamma, dev), _t(beta, dev)          # (named: the device copies must outlive the launch)
        kind = "elu" if i < t.depth else None
        a = torch.full((n, hw, coff), SENT16, dtype=torch.int16, device=dev).view(torch.float16)
        _rn.check(L.rn_dense_f16_norm(_rn.f16(buf), _rn.f16(a), n, hw, coff, ld, R.GROUPS, _rn.f32(mean), _rn.f32(rstd), _rn.f32(gamma_d),
                                      _rn.f32(beta_d), _rn.ACT[kind], _rn.stream()), "rn_dense_f16_norm")
        a64, bound = R.norm_ref(prefix, st, gamma, beta, R.GROUPS, kind)
        rn_ = float((np.abs(a.cpu().numpy().astype(np.float64) - a64) / bound).max())
        assert rn_ <= 1.0, "prefix %d: norm %.3f of the bound" % (coff, rn_)
        worst["norm"] = max(worst["norm"], rn_)
        assert np.array_equal(buf.view(torch.int16).cpu().numpy(), want_buf)          # norm reads the buffer only
    assert coff == ld
    print("DENSE_F16 table %-7s worst ratio to the bound: table row %.3f  mean %.3f  rstd %.3f  norm %.3f" % (
        name, worst["row"], worst["mean"], worst["rstd"], worst["norm"]))


def test_sums_of_a_finished_tensor_in_place(dev):
    """DenseBuffer.of: put with src == buf (ld == c, coff == 0) stores nothing to the tensor and gives the table of a copy"""
    import ops_f16
    sl = R.table_data("t19x25")[0][0]
    t = R.TABLES["t19x25"]
    x = _t(sl, dev).reshape(t.n, t.h, t.w, t.c_in)
    keep = x.clone()
    d = ops_f16.DenseBuffer.of(x)
    assert d.buf.data_ptr() == x.data_ptr() and torch.equal(x, keep)
    other = ops_f16.DenseBuffer(t.n, t.h, t.w, t.c_in, dev)
    other.put(keep)
    assert torch.equal(d.table, other.table) and torch.equal(other.buf, keep)
