"""The inputs and the float64 reference of the step-tail tests (tests/step_tail_ref.py), without a GPU.

(1) On every input set of test_gpu_step_tail.py -- of the two large grid-wrap sets only the smaller -- the float64 reference agrees
with the committed float32 oracle (oracle/losses_ref.py, oracle/train_ref.py) on every element the GPU test compares: element-wise
relative error (helpers.elementwise_rel_err, floor_frac 1e-3) at most 5e-5, scalars within 1e-6.  The inputs are well conditioned,
so a GPU failure points at the kernel and not at the formula.
(2) The inputs reach what they are meant to reach: a 16-row group over three segments, ragged totals, a positive in every class
but the one left empty, planted logits where the generator says, a weight-decay term that matters, one clip that binds and one
that does not, both grids past their first pass."""
import numpy as np
import pytest
import torch

import step_tail_ref as ref
from helpers import elementwise_rel_err
from oracle import train_ref

EW_TOL = 5e-5
SCALAR_TOL = 1e-6
MODES = ("bce_dice", "focal")


def _scalar_err(a, b):
    return abs(a - b) / max(abs(b), 1e-30) if b != 0.0 else abs(a)


def _loss_cases():
    out = []
    for name in ref.SWEEP_CASES + ref.MAXSEG_CASES + ("wrap1",) + ref.CLEAN_CASES + ref.SMALL_END_CASES:
        out += [(name, mode) for mode in MODES]
    out += [(name, name.split("-")[1]) for name in ref.PLANT_CASES]
    return out


@pytest.mark.parametrize("name,mode", _loss_cases(), ids=lambda v: str(v))
def test_loss_reference_agrees_with_the_float32_oracle(name, mode):
    """(the planted focal logits of FOCAL_ILL are left out of dz, and that set's class loss is not compared: float32 and float64
    differ there by the formula's own 1 - p cancellation against eps; the GPU test compares that scalar with float32 instead)"""
    inp = ref.loss_case(name)
    r64 = ref.loss_ref(inp, mode)
    r32 = ref.loss_ref(inp, mode, dtype=torch.float32)
    keep = ~ref.ill_conditioned(inp, mode)
    ill_set = mode == "focal" and not keep.all()
    e_dz = elementwise_rel_err(np.where(keep, r32.dz, 0.0), np.where(keep, r64.dz, 0.0))
    e_dr = elementwise_rel_err(r32.dr, r64.dr)
    e_cls, e_reg = _scalar_err(r32.cls, r64.cls), _scalar_err(r32.reg, r64.reg)
    print("%s %s: dz %.2e dr %.2e class loss %.2e regr loss %.2e" % (name, mode, e_dz, e_dr, e_cls, e_reg))
    assert e_dz <= EW_TOL and e_dr <= EW_TOL, (e_dz, e_dr)
    assert e_reg <= SCALAR_TOL and (ill_set or e_cls <= SCALAR_TOL), (e_cls, e_reg)
    assert (r32.M, r32.nfg) == (r64.M, r64.nfg) == (int(inp.mask.sum()), int((inp.lab.max(1)[inp.mask] > 0.5).sum()))
    assert not r64.dz[~inp.mask].any() and not r64.dr[~inp.mask].any()


@pytest.mark.parametrize("c", ref.MASKING_C)
@pytest.mark.parametrize("mode", MODES)
def test_reference_removes_masked_rows(c, mode):
    """boolean_mask: non-finite logits on masked rows change nothing, bit for bit, and those rows get zero gradients."""
    clean, dirty = ref.loss_ref(ref.loss_case("clean-%d" % c), mode), ref.loss_ref(ref.loss_case("nonfinite-%d" % c), mode)
    for a, b in zip(clean, dirty):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    inp, rows = ref.loss_case("nonfinite-%d" % c), ref.nonfinite_rows(c)
    assert len(rows) == 12 and not inp.mask[rows].any()
    bad = inp.z[rows]
    assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any()
    assert np.isfinite(inp.z[inp.mask]).all() and np.isfinite(np.delete(inp.z, rows, 0)).all()


def _segment_of_row(seg_rows):
    return np.repeat(np.arange(len(seg_rows)), seg_rows)


def test_loss_inputs_reach_the_edges():
    # a 16-row group over three segments, a one-row segment, a ragged last group
    for seg_rows in (ref.SEG_ROWS, ref.SEG_ROWS_MAX):
        seg = _segment_of_row(seg_rows)
        spans = [len(np.unique(seg[g:g + 16])) for g in range(0, len(seg), 16)]
        assert max(spans) >= 3 and 1 in seg_rows and len(seg) % 16 != 0 and 0 not in seg_rows
        assert any(b % 16 for b in np.cumsum(seg_rows)[:-1])
    assert len(ref.SEG_ROWS_MAX) == ref.MAX_SEG and len(set(ref.SEG_ROWS_MAX)) > 8
    # both grids go round again, and only part of the four-lane grid's waves do
    rows4 = sum(ref.SEG_ROWS_WRAP4)
    assert rows4 % 16 != 0 and 262144 < rows4 < 262144 + 2048 * 128 and len(set(ref.SEG_ROWS_WRAP4)) == 2
    assert ref.loss_case("wrap4").c == 4 and ref.loss_case("wrap1").c == 3 and sum(ref.SEG_ROWS_WRAP1) > 2048 * 16
    # every NK of the four-lane dispatch (quads per lane = ceil(C / 16)), its smallest and its largest C
    assert sorted({(c // 4 + 3) // 4 for c in ref.C_FOUR_LANE}) == list(range(1, 9))
    for nk in range(1, 9):
        assert {16 * nk - 12, 16 * nk} <= set(ref.C_FOUR_LANE)
    assert all(c % 4 or c > 128 for c in ref.C_WAVE_PER_ROW)
    for name in ref.SWEEP_CASES + ref.MAXSEG_CASES + ref.WRAP_CASES + ref.CLEAN_CASES + ref.PLANT_CASES:
        inp = ref.loss_case(name)
        positives = inp.lab[inp.mask].sum(0)
        for k in range(inp.c):
            assert (positives[k] == 0) == (k == inp.empty_class), (name, k)
        assert set(np.unique(inp.lab)) <= {0.0, 1.0} and inp.lab.sum(1).max() == 1.0
        fg = inp.lab.max(1) > 0.5
        assert inp.mask[fg].all() and 0.6 < inp.mask.mean() < 0.95
        if name.startswith("sweep") and inp.c <= 128:
            assert 0.05 < fg.mean() < 0.12
    # the small ends
    for c in ref.MASKING_C:
        one = ref.loss_case("one_row-%d" % c)
        assert one.z.shape == (1, c) and one.mask.all() and one.lab.max() == 1.0
        m1 = ref.loss_case("m1-%d" % c)
        assert m1.mask.sum() == 1 and len(m1.mask) > 90
        fg1 = ref.loss_case("one_fg-%d" % c)
        assert ((fg1.lab.max(1) > 0.5) & fg1.mask).sum() == 1 and fg1.mask.sum() > 50


@pytest.mark.parametrize("name", ref.PLANT_CASES)
def test_planted_logits_are_where_the_generator_says(name):
    inp, mode = ref.loss_case(name), name.split("-")[1]
    values = ref.BCE_PLANT if mode == "bce_dice" else ref.FOCAL_PLANT
    assert len(inp.planted) == ref.N_PLANT == len({(r, k) for r, k, _ in inp.planted})
    assert {v for _, _, v in inp.planted} == set(values)
    under_one = [inp.lab[r, k] == 1.0 for r, k, _ in inp.planted]
    assert sum(under_one) == ref.N_PLANT // 2
    for r, k, v in inp.planted:
        assert inp.mask[r] and inp.z[r, k] == np.float32(v)
    # every value under both labels
    assert {v for (_, _, v), one in zip(inp.planted, under_one) if one} == set(values)
    assert {v for (_, _, v), one in zip(inp.planted, under_one) if not one} == set(values)
    ill = ref.ill_conditioned(inp, mode)
    assert ill.sum() == (0 if mode == "bce_dice" else 8) and ill.sum() <= 12


# ------------------------------------------------------------------------------------------------------------- optimizer

def _optimizer_float32(inp, kind, clip):
    """The committed float32 oracle: train_ref.clip_by_global_norm and train_ref.apply_optimizer on g' formed in float32."""
    w, wd = torch.from_numpy(inp.w0.copy()), torch.from_numpy(inp.wd_elem)
    params, state, out = {"arena": w}, {}, []
    for step, g in enumerate(inp.grads, 1):
        gp = torch.from_numpy(g) * inp.grad_scale + wd * w
        reg = (0.5 * wd * w * w).sum().item()
        if clip is None:
            gn = torch.sqrt((gp.double() ** 2).sum()).float()      # (the norm as clip_by_global_norm forms it)
        else:
            (gp,), gn = train_ref.clip_by_global_norm([gp], clip)
        train_ref.apply_optimizer(kind, params, {"arena": gp}, state, inp.lr, step)
        s1, s2 = ref.STATE_NAMES[kind]
        out.append(ref.OptStep(w.numpy().copy(), state["arena"][s1].numpy().copy(),
                               state["arena"][s2].numpy().copy() if s2 else None, gn.item(), reg))
    return out


OPT_CASES = [("small", kind, clip) for kind in ("momentum", "rmsprop", "adam") for clip in (None, ref.CLIP_BINDS, ref.CLIP_LOOSE)] + \
            [("large", kind, clip) for kind in ("momentum", "adam") for clip in (None, ref.CLIP_BINDS)]


@pytest.mark.parametrize("name,kind,clip", OPT_CASES, ids=lambda v: str(v))
def test_optimizer_reference_agrees_with_the_float32_oracle(name, kind, clip):
    inp = ref.optimizer_case(name)
    pad = ref.padding_mask(inp)
    worst = {}
    for step, (a, b) in enumerate(zip(_optimizer_float32(inp, kind, clip), ref.optimizer_ref(inp, kind, clip)), 1):
        for what, x, y in (("weights", a.w, b.w), ("state1", a.state1, b.state1), ("state2", a.state2, b.state2)):
            if y is not None:
                worst[what] = max(worst.get(what, 0.0), elementwise_rel_err(x, y))
        assert _scalar_err(a.norm, b.norm) <= SCALAR_TOL and _scalar_err(a.reg, b.reg) <= SCALAR_TOL, (a.norm, b.norm, a.reg, b.reg)
        # the padding: zero weights, the initial state evolved on a zero gradient
        assert not b.w[pad].any()
        if kind == "rmsprop":
            assert np.allclose(b.state1[pad], 0.9 ** step, rtol=1e-14, atol=0) and not b.state2[pad].any()
        else:
            assert not b.state1[pad].any() and (b.state2 is None or not b.state2[pad].any())
    print("%s %s clip %s: %s" % (name, kind, clip, " ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= EW_TOL, worst


@pytest.mark.parametrize("name", ["small", "large"])
def test_optimizer_inputs_reach_the_edges(name):
    inp = ref.optimizer_case(name)
    real = ~ref.padding_mask(inp)
    assert any(s % ref.OPT_BLOCK for s in inp.sizes) and inp.count % ref.OPT_BLOCK == 0 and (~real).any()
    assert len(set(inp.l2)) == len(inp.l2)
    # the decay term is at least a tenth of |g'| on at least a quarter of the elements
    for g in inp.grads:
        gp = g.astype(np.float64) * inp.grad_scale + inp.wd_elem.astype(np.float64) * inp.w0
        share = np.abs(inp.wd_elem.astype(np.float64) * inp.w0)[real] >= 0.1 * np.abs(gp)[real]
        assert share.mean() >= 0.25, share.mean()
    # one clip binds and one does not, at every step
    for step in ref.optimizer_ref(inp, "momentum"):
        assert ref.CLIP_BINDS < step.norm < ref.CLIP_LOOSE
    if name == "small":
        assert len(inp.sizes) >= 5 and None in inp.l2 and sum(s % ref.OPT_BLOCK != 0 for s in inp.sizes) >= 4
        assert all(0.05 <= s <= 1.0 for s in inp.l2 if s is not None)
        assert ref.SMALL_SLICES[0][0] == 0 and ref.SMALL_SLICES[-1][1] == inp.count and len(ref.SMALL_SLICES) == 3
        assert all(a[1] == b[0] and b[0] % ref.OPT_BLOCK == 0 for a, b in zip(ref.SMALL_SLICES, ref.SMALL_SLICES[1:]))
    else:
        # more than 2048 blocks of 256 threads x 4 elements: the grid cap binds, part of the grid goes round again, and
        # every decayed parameter after the first lies past the first pass
        assert inp.count // 4 > 2048 * 256 and inp.count // 4 < 2 * 2048 * 256
        assert inp.sizes[0] == 2097152 + 5 * 1024 + 7 and all(o >= 2097152 for o in inp.offsets[1:])
        assert all(s is not None for s in inp.l2)



def test_update_descriptor_refuses_features_and_fields_that_do_not_agree():
    """rn_optimizer_update picks its kernel from `features`, and a field that does not agree with them is refused with RN_EINVAL
    (-1) and a message ahead of any launch: fake non-null pointers that are never dereferenced, no device needed."""
    import ctypes
    import _rn
    L = _rn.lib()
    q = ctypes.c_void_p(4096)
    N, CLIP, A, G = _rn.OPT_F_NORM, _rn.OPT_F_CLIP, _rn.OPT_F_ACCUM, _rn.OPT_F_GATE
    fields = {N: dict(partial=q), CLIP: dict(clip_norm=0.5, norm_sq=q), A: dict(acc=q, inv_accum=0.5, accum_dev=q), G: dict(gate_dev=q)}

    def update(features, **over):
        """Every field of every set feature is filled as the header asks, then `over`: only the combination can be at fault."""
        kw = dict(kind=0, features=features, w=q, grad=q, state1=q, wd_per_block=q, count=1024, lr=0.1, grad_scale=1.0, step=1)
        for bit, f in fields.items():
            if features & bit:
                kw.update(f)
        kw.update(over)
        u = _rn.OptUpdate(**kw)
        return L.rn_optimizer_update(ctypes.byref(u), None), L.rn_last_error()

    rc = L.rn_optimizer_update(None, None)
    assert rc == -1 and b"descriptor" in L.rn_last_error()
    for bad in (64, 1 << 31, N | 128):
        rc, msg = update(bad)
        assert rc == -1 and b"feature bit" in msg, bad
    for features, word in ((N | CLIP, b"NORM"), (G | N, b"NORM"), (G | A, b"ACCUM"), (A, b"ACCUM"), (N | A | CLIP, b"CLIP"),
                           (N | A | G, b"GATE")):
        rc, msg = update(features)
        assert rc == -1 and word in msg and b"neither" in msg, (features, msg)
    # a field of a feature that is clear: a pointer set by mistake does not pass, and does not select a kernel
    rc, msg = update(0, partial=q)
    assert rc == -1 and b"partial" in msg
    rc, msg = update(0, gate_dev=q)
    assert rc == -1 and b"gate_dev" in msg
    rc, msg = update(0, clip_norm=-1.0)
    assert rc == -1 and b"clip_norm" in msg
    rc, msg = update(0, norm_sq=q)
    assert rc == -1 and b"norm_sq" in msg
    rc, msg = update(0, lr_dev=q)
    assert rc == -1 and b"device rate" in msg
    rc, msg = update(N, acc=q, accum_dev=q, inv_accum=0.5)
    assert rc == -1 and b"ACCUM" in msg
