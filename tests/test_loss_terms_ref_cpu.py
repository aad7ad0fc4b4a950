"""The class loss as a weighted sum of terms, without a GPU: the spec grammar (losses.parse_class_loss), the --class-loss flag,
the descriptor validation of rn_loss_terms_fwd / rn_loss_terms_bwd (they refuse before any launch, so the library answers on a
CPU), the float64 reference of loss_terms_ref.py against oracle.losses_ref where the two overlap, jaccard = s * fixed_iou, and
that the GPU test's bar (TOL = 1e-4, element-wise) is within reach of float32: the closed-form gradients evaluated in float32
numpy against the float64 autograd reference on the GPU test's cases."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import loss_terms_ref as ref
import step_tail_ref
from helpers import assert_close, elementwise_rel_err

TOL = 1e-4
G_CLS, G_REG = step_tail_ref.G_CLS, step_tail_ref.G_REG


# ------------------------------------------------------------------------------------------------------------ the grammar
def test_spec_defaults_and_examples():
    import losses
    p = losses.parse_class_loss
    assert p("bce+jaccard") == (("bce", 1.0, None), ("jaccard", 1.0, 1.0))
    assert p("balanced_bce+dice:0.5") == (("balanced_bce", 1.0, None), ("dice", 0.5, 0.0))
    assert p("bce+dice:1:1+fixed_iou:0.3:1e-7") == (("bce", 1.0, None), ("dice", 1.0, 1.0), ("fixed_iou", 0.3, 1e-7))
    assert p("fixed_iou") == (("fixed_iou", 1.0, 1e-7),) and p("focal:2") == (("focal", 2.0, None),)
    assert p(" bce + dice ") == p("bce+dice")
    assert p("jaccard:1:0") == (("jaccard", 1.0, 0.0),)            # identically zero, as in the reference: allowed
    assert [t.name for t in p("+".join(reversed(losses.TERM_NAMES)))] == list(reversed(losses.TERM_NAMES))
    assert losses.TERM_NAMES == ref.TERM_NAMES and losses.DEFAULT_SMOOTH == ref.DEFAULT_SMOOTH
    for spec in (ref.ALL_TERMS,) + ref.PER_TERM_SPECS:                # the tests' own reading of the grammar agrees
        assert [tuple(t) for t in p(spec)] == ref.terms_of(spec)


@pytest.mark.parametrize("spec", [ref.ALL_TERMS, "bce+jaccard", "dice:0.1:1e-30", "focal:3.0000001", "fixed_iou:1:0"])
def test_spec_round_trip(spec):
    import losses
    parsed = losses.parse_class_loss(spec)
    assert losses.parse_class_loss(parsed.spec()) == parsed
    assert isinstance(parsed.describe(), str) and all(t.name in parsed.describe() for t in parsed)


@pytest.mark.parametrize("spec,token,why", [
    ("bce+huber", "huber", "unknown name"), ("bce+dice+bce:2", "bce:2", "twice"), ("bce:1:1", "bce:1:1", "no smooth"),
    ("focal:1:0", "focal:1:0", "no smooth"), ("balanced_bce:1:2", "balanced_bce:1:2", "no smooth"),
    ("dice:1:1:1", "dice:1:1:1", "at the most"), ("dice:x", "dice:x", "numbers"), ("dice:1:y", "dice:1:y", "numbers"),
    ("bce:0", "bce:0", "weight"), ("bce:-1", "bce:-1", "weight"), ("bce:inf", "bce:inf", "weight"), ("bce:nan", "bce:nan", "weight"),
    ("dice:1:-0.5", "dice:1:-0.5", "smooth"), ("jaccard:1:inf", "jaccard:1:inf", "smooth"), ("dice:1:nan", "dice:1:nan", "smooth"),
    ("bce+", "", "unknown name"), ("+bce", "", "unknown name"), ("bce++dice", "", "unknown name"), ("BCE", "BCE", "unknown name"),
    ("dice:", "dice:", "numbers"), ("bce+jaccard:1e30:1e30", "jaccard:1e30:1e30", "overflows"),
])
def test_spec_errors_name_the_token(spec, token, why):
    import losses
    with pytest.raises(ValueError) as e:
        losses.parse_class_loss(spec)
    assert repr(token) in str(e.value) and why in str(e.value), str(e.value)


def test_spec_refuses_nothing_at_all():
    import losses
    for bad in ("", "   ", None, 3):
        with pytest.raises(ValueError, match="empty"):
            losses.parse_class_loss(bad)


def test_class_loss_flag_error():
    import train
    parser = train.build_parser()
    base = ["--dataset", "shapes"]
    assert parser.parse_args(base).class_loss is None and parser.parse_args(base).loss == "bce_dice"
    assert train.class_loss_flag_error(parser.parse_args(base)) is None
    assert train.class_loss_flag_error(parser.parse_args(base + ["--loss", "focal"])) is None
    assert train.class_loss_flag_error(parser.parse_args(base + ["--class-loss", "bce+jaccard"])) is None
    assert train.class_loss_flag_error(parser.parse_args(base + ["--class-loss", "bce+jaccard", "--loss", "bce_dice"])) is None
    err = train.class_loss_flag_error(parser.parse_args(base + ["--class-loss", "bce+jaccard", "--loss", "focal"]))
    assert "--class-loss" in err and "--loss focal" in err
    err = train.class_loss_flag_error(parser.parse_args(base + ["--class-loss", "bce+iou"]))
    assert err.startswith("--class-loss") and "'iou'" in err
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--loss", "bce+jaccard"])             # --loss keeps its two choices
    assert train.class_loss_flag_error(argparse.Namespace(class_loss=None, loss="focal")) is None


def test_trainer_validates_the_spec_at_construction():
    import layers, levels, losses, retinanet, train
    lv = levels.build_levels()
    net = retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0)
    with pytest.raises(ValueError, match="'hinge'"):
        train.Trainer(net, lv, device=torch.device("cpu"), use_graph=False, loss_mode="bce+hinge")
    tr = train.Trainer(net, lv, device=torch.device("cpu"), use_graph=False, loss_mode="balanced_bce+jaccard")
    assert tr.loss_mode == losses.parse_class_loss("balanced_bce+jaccard")
    assert train.Trainer(net, lv, device=torch.device("cpu"), use_graph=False, loss_mode="focal").loss_mode == "focal"
    assert train.Trainer(net, lv, device=torch.device("cpu"), use_graph=False, loss_mode=None).loss_mode is None    # losses.LOSS_MODE, as before


# ------------------------------------------------------------------------------------------------- the library's refusals
def _desc(**kw):
    import _rn
    return _rn.LossTerms(**kw)


def _fwd(desc, segs=None, nseg=1, c=4):
    import _rn
    L = _rn.lib()
    return L.rn_loss_terms_fwd(segs, nseg, c, ctypes.byref(desc) if desc is not None else None, None, None, None, None, 0, None)


def _bwd(desc, segs=None, nseg=1, c=4):
    import _rn
    L = _rn.lib()
    return L.rn_loss_terms_bwd(segs, nseg, c, ctypes.byref(desc) if desc is not None else None, None, None, None, None)


BAD_DESCRIPTORS = [
    (None, "null descriptor"),
    (dict(terms=0), "no term set"),
    (dict(terms=64, w_bce=1.0), "unknown term bits 0x40"),
    (dict(terms=1 | 128, w_bce=1.0), "unknown term bits 0x80"),
    (dict(terms=1, w_bce=0.0), "weight of bce must be finite and > 0"),
    (dict(terms=2, w_balanced_bce=-1.0), "weight of balanced_bce must be finite and > 0"),
    (dict(terms=4, w_dice=float("inf")), "weight of dice must be finite and > 0"),
    (dict(terms=8, w_jaccard=float("nan"), s_jaccard=1.0), "weight of jaccard must be finite and > 0"),
    (dict(terms=16, w_fixed_iou=1.0, s_fixed_iou=-1e-7), "smooth of fixed_iou must be finite and >= 0"),
    (dict(terms=4, w_dice=1.0, s_dice=float("inf")), "smooth of dice must be finite and >= 0"),
    (dict(terms=8, w_jaccard=1.0, s_jaccard=float("nan")), "smooth of jaccard must be finite and >= 0"),
    (dict(terms=8, w_jaccard=1e30, s_jaccard=1e30), "weight * smooth of jaccard overflows"),
    (dict(terms=1, w_bce=1.0, w_focal=0.5), "weight of the clear term focal must be 0"),
    (dict(terms=32, w_focal=1.0, w_dice=1.0), "weight of the clear term dice must be 0"),
    (dict(terms=1, w_bce=1.0, s_dice=1.0), "smooth of the clear term dice must be 0"),
    (dict(terms=1 | 4, w_bce=1.0, w_dice=1.0, s_fixed_iou=1e-7), "smooth of the clear term fixed_iou must be 0"),
]


@pytest.mark.parametrize("fields,message", BAD_DESCRIPTORS, ids=[m for _, m in BAD_DESCRIPTORS])
def test_library_refuses_bad_descriptors(fields, message):
    """RN_EINVAL with its message from both entries, before the segments are looked at (they are null here) and before any launch."""
    import _rn
    L = _rn.lib()
    desc = None if fields is None else _desc(**fields)
    for call in (_fwd, _bwd):
        assert call(desc) == -1
        assert message in L.rn_last_error().decode(), L.rn_last_error()
    assert L.rn_loss_terms_workspace(None, 1, 4, ctypes.byref(desc) if desc is not None else None) == 0


def test_library_checks_segments_and_classes_after_the_descriptor():
    """The segment and C checks of rn_loss_fwd: for the general kernels and for the two descriptors that run the existing ones."""
    import _rn
    L = _rn.lib()
    general = _desc(terms=1 | 8, w_bce=1.0, w_jaccard=1.0, s_jaccard=1.0)
    legacy = _desc(terms=1 | 4, w_bce=1.0, w_dice=1.0)
    segs = (_rn.LossSeg * 1)()
    for desc in (general, legacy):
        for call in (_fwd, _bwd):
            assert call(desc, None, 1) == -1 and b"bad segments" in L.rn_last_error()
            assert call(desc, segs, 0) == -1 and b"bad segments" in L.rn_last_error()
            assert call(desc, segs, _rn.MAX_SEG + 1) == -1 and b"bad segments" in L.rn_last_error()
            assert call(desc, segs, 1, 257) == -2 and b"num_classes 257" in L.rn_last_error()           # RN_EUNSUPPORTED
            assert call(desc, segs, 1, 0) == -2
            assert call(desc, segs, 1, 4) == -1 and b"null pointer in segment 0" in L.rn_last_error()
    assert L.rn_loss_terms_stats_floats(20) == _rn.LOSS_STATS_HEADER + 5 * 20
    # the two existing modes' descriptors need the existing workspace, every other one its own (wider with balanced_bce)
    assert L.rn_loss_terms_workspace(segs, 1, 20, ctypes.byref(legacy)) == L.rn_loss_workspace(segs, 1, 20)
    plain = L.rn_loss_terms_workspace(segs, 1, 20, ctypes.byref(general))
    wide = L.rn_loss_terms_workspace(segs, 1, 20, ctypes.byref(_desc(terms=2, w_balanced_bce=1.0)))
    assert plain == L.rn_loss_workspace(segs, 1, 20) and wide > plain


def test_descriptor_of_a_spec():
    import _rn, losses
    d = losses.parse_class_loss("bce:0.5+jaccard:2:3+focal").struct()
    assert d.terms == _rn.LOSS_TERM["bce"] | _rn.LOSS_TERM["jaccard"] | _rn.LOSS_TERM["focal"] == 1 | 8 | 32
    assert (d.w_bce, d.w_jaccard, d.s_jaccard, d.w_focal) == (0.5, 2.0, 3.0, 1.0)
    assert (d.w_balanced_bce, d.w_dice, d.w_fixed_iou, d.s_dice, d.s_fixed_iou) == (0.0,) * 5
    assert ctypes.sizeof(_rn.LossTerms) == 40


# ----------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
@pytest.mark.parametrize("spec,mode", [("bce+dice", "bce_dice"), ("focal", "focal")])
def test_reference_equals_the_oracle_where_they_overlap(spec, mode, c):
    inp = step_tail_ref.loss_case("sweep-%d" % c)
    a, b = ref.loss_terms_ref(inp, spec, G_CLS, G_REG), step_tail_ref.loss_ref(inp, mode)
    assert (a.cls, a.reg, a.M, a.nfg) == (b.cls, b.reg, b.M, b.nfg)
    for x, y in ((a.I, b.I), (a.L, b.L), (a.P, b.P), (a.dz, b.dz), (a.dr, b.dr)):
        assert np.array_equal(x, y)
    m = torch.from_numpy(inp.mask)
    from oracle import losses_ref
    bce = losses_ref.sigmoid_bce_with_logits(torch.from_numpy(inp.lab).double()[m], torch.from_numpy(inp.z).double()[m])
    assert abs((a.B1.sum() + a.B0.sum()) / bce.sum().item() - 1.0) < 1e-12


@pytest.mark.parametrize("s", [0.0, 1e-7, 0.5, 1.0, 3.0])
@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
def test_jaccard_is_smooth_times_fixed_iou(c, s):
    """L + sum (1 - l) p = L + P - I: one function up to the factor s, in value and in gradient."""
    inp = step_tail_ref.loss_case("sweep-%d" % c)
    j = ref.loss_terms_ref(inp, "jaccard:1:%r" % s, G_CLS, None)
    f = ref.loss_terms_ref(inp, "fixed_iou:1:%r" % s, G_CLS, None)
    assert abs(j.cls - s * f.cls) <= 1e-14 * max(abs(f.cls), 1.0)
    assert np.abs(j.dz - s * f.dz).max() <= 1e-14 * max(np.abs(f.dz).max(), 1.0)
    if s == 0.0:
        assert j.cls == 0.0 and not j.dz.any()


# ------------------------------------------------------------------------------------ the bar is within reach of float32
BAR_CASES = (tuple("sweep-%d" % c for c in (1, 2, 3, 4, 20, 65, 80, 128, 256)) + step_tail_ref.MAXSEG_CASES +
             step_tail_ref.SMALL_END_CASES + ("plant-bce_dice-3", "plant-bce_dice-20"))


@pytest.mark.parametrize("name", BAR_CASES)
def test_float32_closed_form_reaches_the_bar(name):
    """Every term but focal on every case, planted saturated logits included; all six on the cases without planted logits
    (focal at a saturated logit under the other family's plant is off by O(1) in float32: test_gpu_step_tail's
    test_loss_saturated_logits has the reason)."""
    inp = step_tail_ref.loss_case(name)
    for spec in (ref.ALL_BUT_FOCAL,) + (() if name.startswith("plant") else (ref.ALL_TERMS,)):
        want = ref.loss_terms_ref(inp, spec, G_CLS, None).dz
        got = ref.closed_form_f32(inp, spec, G_CLS)
        print("%s %s: element-wise %.3e" % (name, "all six" if spec == ref.ALL_TERMS else "focal-free", elementwise_rel_err(got, want)))
        assert_close(got, want, TOL, "%s float32 closed form" % name, elementwise_tol=TOL)


@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
def test_float32_closed_form_reaches_the_bar_on_planted_focal(c):
    name = "plant-focal-%d" % c
    inp = step_tail_ref.loss_case(name)
    keep = ~step_tail_ref.ill_conditioned(inp, "focal")
    for spec in (ref.ALL_TERMS, "focal+dice:0.5"):
        want = np.where(keep, ref.loss_terms_ref(inp, spec, G_CLS, None).dz, 0.0)
        got = np.where(keep, ref.closed_form_f32(inp, spec, G_CLS), 0.0)
        print("%s %s: element-wise %.3e" % (name, spec, elementwise_rel_err(got, want)))
        assert_close(got, want, TOL, "%s float32 closed form" % name, elementwise_tol=TOL)
