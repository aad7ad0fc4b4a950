"""The box regression loss as a weighted sum of terms, without a GPU: the spec grammar (losses.parse_regr_loss), the --regr-loss
flag, the descriptor validation of rn_regr_terms_fwd / rn_regr_terms_bwd (they refuse before any launch, so the library answers
on a CPU), and the float64 reference of regr_terms_ref.py itself: the invariance of the anchor-unit IoU under the decode of
oracle.utils_ref.regression_postprocess, its gradients against central differences, huber:1:1 against oracle.losses_ref, and the
ranges of the two overlap measures."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import regr_terms_ref as ref
from oracle import losses_ref, utils_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the grammar
def test_spec_defaults_and_examples():
    import losses
    p = losses.parse_regr_loss
    assert p("huber") == (("huber", 1.0, 1.0),) and p("huber:2") == (("huber", 2.0, 1.0),)
    assert p("huber:1:0.11") == (("huber", 1.0, 0.11),)
    assert p("giou:2") == (("giou", 2.0, None),) and p("iou") == (("iou", 1.0, None),)
    assert p("huber:0.5+giou:2") == (("huber", 0.5, 1.0), ("giou", 2.0, None))
    assert p(" giou + huber ") == p("giou+huber")
    assert losses.REGR_TERM_NAMES == ref.TERM_NAMES
    for spec in ref.SPECS:                                            # the tests' own reading of the grammar agrees
        assert [tuple(t) for t in p(spec)] == ref.terms_of(spec)
    assert p("huber").is_default() and p("huber:1:1").is_default() and p("huber:1.0:1.0").is_default()
    for spec in ("huber:2", "huber:1:0.5", "giou", "huber+giou"):
        assert not p(spec).is_default()
    assert p(p("giou")) is not None and isinstance(p("giou"), losses.RegrLoss)


@pytest.mark.parametrize("spec", ref.SPECS + ("huber", "iou:3.0000001+huber:1e-3:1e-30"))
def test_spec_round_trip(spec):
    import losses
    parsed = losses.parse_regr_loss(spec)
    assert losses.parse_regr_loss(parsed.spec()) == parsed
    assert isinstance(parsed.describe(), str) and all(t.name in parsed.describe() for t in parsed)


@pytest.mark.parametrize("spec,token,why", [
    ("huber+diou", "diou", "unknown name"), ("ciou", "ciou", "unknown name"), ("GIoU", "GIoU", "unknown name"),
    ("giou+", "", "unknown name"), ("+giou", "", "unknown name"),
    ("giou+iou+giou:2", "giou:2", "twice"), ("huber+huber", "huber", "twice"),
    ("giou:0", "giou:0", "weight"), ("iou:-1", "iou:-1", "weight"), ("huber:inf", "huber:inf", "weight"), ("giou:nan", "giou:nan", "weight"),
    ("giou:x", "giou:x", "numbers"), ("giou:", "giou:", "numbers"), ("huber:1:y", "huber:1:y", "numbers"),
    ("huber:1:0", "huber:1:0", "delta"), ("huber:1:-0.5", "huber:1:-0.5", "delta"), ("huber:1:inf", "huber:1:inf", "delta"),
    ("huber:1:nan", "huber:1:nan", "delta"),
    ("giou:1:1", "giou:1:1", "no delta"), ("iou:1:0.5", "iou:1:0.5", "no delta"), ("huber:1:1:1", "huber:1:1:1", "at the most"),
])
def test_spec_errors_name_the_token(spec, token, why):
    import losses
    with pytest.raises(ValueError) as e:
        losses.parse_regr_loss(spec)
    assert repr(token) in str(e.value) and why in str(e.value) and str(e.value).startswith("regr loss spec"), str(e.value)


def test_spec_refuses_nothing_at_all():
    import losses
    for bad in ("", "   ", None, 3):
        with pytest.raises(ValueError, match="empty"):
            losses.parse_regr_loss(bad)


def test_regr_loss_flag_error():
    import train
    parser = train.build_parser()
    base = ["--dataset", "shapes"]
    assert parser.parse_args(base).regr_loss is None
    assert train.regr_loss_flag_error(parser.parse_args(base)) is None
    for spec in ("giou:2", "huber", "huber:0.5+giou:2"):
        assert train.regr_loss_flag_error(parser.parse_args(base + ["--regr-loss", spec])) is None
    assert train.regr_loss_flag_error(parser.parse_args(base + ["--regr-loss", "giou", "--loss", "focal"])) is None
    assert train.regr_loss_flag_error(parser.parse_args(base + ["--regr-loss", "giou", "--class-loss", "bce+jaccard"])) is None
    err = train.regr_loss_flag_error(parser.parse_args(base + ["--regr-loss", "huber+diou"]))
    assert err.startswith("--regr-loss: ") and "'diou'" in err
    err = train.regr_loss_flag_error(parser.parse_args(base + ["--regr-loss", "huber:1:0"]))
    assert err.startswith("--regr-loss: ") and "'huber:1:0'" in err and "delta" in err
    assert train.regr_loss_flag_error(argparse.Namespace(regr_loss=None)) is None


def test_bad_spec_exits_through_the_parser_before_any_device_work(capsys, monkeypatch):
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    with pytest.raises(SystemExit) as e:
        train.main(["--dataset", "shapes", "--regr-loss", "giou+diou"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--regr-loss: regr loss spec 'giou+diou': term 'diou': unknown name" in err


def test_trainer_validates_the_spec_at_construction():
    import layers, levels, losses, retinanet, train
    lv = levels.build_levels()
    net = retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="'ciou'"):
        train.Trainer(net, lv, device=cpu, use_graph=False, regr_loss="huber+ciou")
    assert train.Trainer(net, lv, device=cpu, use_graph=False).regr_loss is None
    assert train.Trainer(net, lv, device=cpu, use_graph=False, regr_loss=None).regr_loss is None
    tr = train.Trainer(net, lv, device=cpu, use_graph=False, regr_loss="huber")
    assert tr.regr_loss == losses.parse_regr_loss("huber:1:1") and tr.regr_loss.is_default()
    tr = train.Trainer(net, lv, device=cpu, use_graph=False, regr_loss="huber:0.5+giou:2")
    assert tr.regr_loss == (("huber", 0.5, 1.0), ("giou", 2.0, None))


def test_losses_loss_takes_todays_route_for_none_and_huber(monkeypatch):
    """regr_mode None and 'huber' (weight 1, delta 1) call ops.detection_loss alone and return its two losses; another spec also
    calls ops.regression_terms and returns ITS regression loss."""
    import losses, ops, utils
    calls = []
    monkeypatch.setattr(ops, "detection_loss", lambda *a: calls.append("detection_loss") or ("cls", "huber_of_loss_hip", "stats"))
    monkeypatch.setattr(ops, "regression_terms", lambda *a: calls.append(("regression_terms", a[-1])) or ("regr_of_terms", "stats"))
    t = {"P3": torch.zeros(2, 4)}
    logits = utils.Detection(classification=utils.Classification(unscaled=t, prob=t), regression=t, regression_postprocessed=None)
    kw = dict(labels=logits, logits=logits, trainable_masks=t)
    for regr_mode in (None, "huber", "huber:1:1", losses.parse_regr_loss("huber:1.0")):
        del calls[:]
        assert losses.loss(regr_mode=regr_mode, **kw) == ("cls", "huber_of_loss_hip") and calls == ["detection_loss"]
    del calls[:]
    assert losses.loss(**kw) == ("cls", "huber_of_loss_hip") and calls == ["detection_loss"]
    assert losses.loss(regr_mode="giou:2", **kw) == ("cls", "regr_of_terms")
    assert calls == ["detection_loss", "detection_loss", ("regression_terms", (("giou", 2.0, None),))]
    with pytest.raises(ValueError, match="'diou'"):
        losses.loss(regr_mode="diou", **kw)


# ------------------------------------------------------------------------------------------------- the library's refusals
def _desc(**kw):
    import _rn
    return _rn.RegrTerms(**kw)


def _fwd(desc, segs=None, nseg=1, c=4):
    import _rn
    return _rn.lib().rn_regr_terms_fwd(segs, nseg, c, ctypes.byref(desc) if desc is not None else None, None, None, None, None, 0, None)


def _bwd(desc, segs=None, nseg=1, c=4):
    import _rn
    return _rn.lib().rn_regr_terms_bwd(segs, nseg, ctypes.byref(desc) if desc is not None else None, None, None, None, None)


BAD_DESCRIPTORS = [
    (None, "null descriptor"),
    (dict(terms=0), "no term set"),
    (dict(terms=8, w_huber=1.0), "unknown term bits 0x8"),
    (dict(terms=2 | 64, w_iou=1.0), "unknown term bits 0x40"),
    (dict(terms=1, w_huber=0.0, delta_huber=1.0), "w_huber must be finite and > 0"),
    (dict(terms=2, w_iou=-1.0), "w_iou must be finite and > 0"),
    (dict(terms=4, w_giou=float("inf")), "w_giou must be finite and > 0"),
    (dict(terms=4, w_giou=float("nan")), "w_giou must be finite and > 0"),
    (dict(terms=1, w_huber=1.0, delta_huber=0.0), "delta_huber must be finite and > 0"),
    (dict(terms=1, w_huber=1.0, delta_huber=float("nan")), "delta_huber must be finite and > 0"),
    (dict(terms=1, w_huber=1.0, delta_huber=float("inf")), "delta_huber must be finite and > 0"),
    (dict(terms=2, w_iou=1.0, w_giou=0.5), "w_giou of the clear term must be 0"),
    (dict(terms=4, w_giou=1.0, w_huber=1.0), "w_huber of the clear term must be 0"),
    (dict(terms=4, w_giou=1.0, delta_huber=1.0), "delta_huber of the clear term must be 0"),
]


@pytest.mark.parametrize("fields,message", BAD_DESCRIPTORS, ids=[m for _, m in BAD_DESCRIPTORS])
def test_library_refuses_bad_descriptors(fields, message):
    """RN_EINVAL with a message that names the field, from both entries, before the segments are looked at (they are null here)."""
    import _rn
    L = _rn.lib()
    desc = None if fields is None else _desc(**fields)
    for call in (_fwd, _bwd):
        assert call(desc) == -1
        assert message in L.rn_last_error().decode(), L.rn_last_error()
    assert L.rn_regr_terms_workspace(None, 1, 4, ctypes.byref(desc) if desc is not None else None) == 0


def test_library_checks_segments_after_the_descriptor():
    import _rn
    L = _rn.lib()
    good = _desc(terms=1 | 4, w_huber=1.0, delta_huber=1.0, w_giou=2.0)
    segs = (_rn.LossSeg * 1)()
    for call in (_fwd, _bwd):
        assert call(good, segs, 0) == -1 and b"nseg 0" in L.rn_last_error()
        assert call(good, segs, _rn.MAX_SEG + 1) == -1 and b"nseg 17" in L.rn_last_error()
        assert call(good, None, 1) == -1 and b"null segs" in L.rn_last_error()
        assert call(good, segs, 1) == -1 and b"in segment 0" in L.rn_last_error()
    assert L.rn_regr_terms_workspace(segs, 1, 20, ctypes.byref(good)) > 0


def test_descriptor_of_a_spec():
    import _rn, losses
    d = losses.parse_regr_loss("huber:0.5:0.11+giou:2").struct()
    assert d.terms == _rn.REGR_TERM["huber"] | _rn.REGR_TERM["giou"] == 1 | 4
    assert (d.w_huber, d.w_giou, d.w_iou) == (0.5, 2.0, 0.0) and d.delta_huber == np.float32(0.11)
    d = losses.parse_regr_loss("iou:3").struct()
    assert (d.terms, d.w_iou, d.w_huber, d.w_giou, d.delta_huber) == (2, 3.0, 0.0, 0.0, 0.0)
    assert ctypes.sizeof(_rn.RegrTerms) == 20 and _rn.REGR_STATS_FLOATS == 8


def test_header_declares_the_entries_and_the_bindings_list_them():
    import _rn
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    for name in ("rn_regr_terms_workspace", "rn_regr_terms_fwd", "rn_regr_terms_bwd"):
        assert re.search(r"\b%s\(" % name, text) and name in _rn.SYMBOLS
        assert hasattr(_rn.lib(), name)
    assert "enum rn_regr_term { RN_RT_HUBER = 1, RN_RT_IOU = 2, RN_RT_GIOU = 4 };" in text
    assert re.search(r"#define RN_REGR_STATS_FLOATS 8\b", text)
    assert int(re.search(r"#define RN_API_VERSION (\d+)", text).group(1)) == _rn.API_VERSION == _rn.lib().rn_version()
    assert "DIoU" in text and "CIoU" in text


# ----------------------------------------------------------------------------------------------------- the reference itself
def _random_pairs(n, seed, noise=0.4):
    rng = np.random.default_rng(seed)
    l = np.concatenate([rng.normal(0, 0.5, (n, 2)), rng.normal(0, 0.4, (n, 2))], 1)
    return l + noise * rng.normal(0, 1, (n, 4)), l


def test_anchor_unit_iou_is_the_iou_of_the_decoded_boxes():
    """Both boxes of a row share anchor and cell, so the decode (centre = t * anchor + cell, size = exp(t) * anchor) is one
    translation and one positive per-axis scaling, and IoU / GIoU do not see it: 4608 rows = [8, 8, 8, 9] anchors with random
    anisotropic anchor sizes.  In float64 with the decode written out: 1e-12.  Against oracle.utils_ref's regression_postprocess +
    iou, which compute in float32 on image coordinates in [0, 1]: a corner carries up to 1 ulp(1) = 1.2e-7 against box sides from
    0.01 up, 1.2e-5 relative per side and four sides in an area ratio -- 1e-4 absolute on an IoU <= 1; invalid intersections are 0
    on both sides."""
    n, h, w, a = 8, 8, 8, 9
    rng = np.random.default_rng(5)
    anchors = rng.uniform(0.05, 0.5, (a, 2))
    p, l = _random_pairs(n * h * w * a, 6)
    p32, l32 = p.astype(np.float32), l.astype(np.float32)
    iou, giou = ref.iou_giou(torch.from_numpy(p32).double(), torch.from_numpy(l32).double())
    disjoint = (iou == 0).numpy()
    assert 0.03 < disjoint.mean() < 0.25, disjoint.mean()
    # float64, written out
    cells = np.stack(np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij"), -1)[None, :, :, None, :]

    def decode(t):
        t = t.astype(np.float64).reshape(n, h, w, a, 4)
        centre, size = t[..., :2] * anchors + cells, np.exp(t[..., 2:]) * anchors
        return np.concatenate([centre - size / 2, centre + size / 2], -1).reshape(-1, 4)
    bp, bl = decode(p32), decode(l32)
    iy = np.maximum(0, np.minimum(bp[:, 2], bl[:, 2]) - np.maximum(bp[:, 0], bl[:, 0]))
    ix = np.maximum(0, np.minimum(bp[:, 3], bl[:, 3]) - np.maximum(bp[:, 1], bl[:, 1]))
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = area(bp) + area(bl) - iy * ix
    enc = (np.maximum(bp[:, 2], bl[:, 2]) - np.minimum(bp[:, 0], bl[:, 0])) * (np.maximum(bp[:, 3], bl[:, 3]) - np.minimum(bp[:, 1], bl[:, 1]))
    assert np.abs(iy * ix / union - iou.numpy()).max() <= 1e-12
    assert np.abs(iy * ix / union - (enc - union) / enc - giou.numpy()).max() <= 1e-12
    # the oracle
    shape = (n, h, w, a, 4)
    op, ol = utils_ref.regression_postprocess(p32.reshape(shape), anchors), utils_ref.regression_postprocess(l32.reshape(shape), anchors)
    got = utils_ref.iou(op, ol).reshape(-1).astype(np.float64)
    assert (got[disjoint] == 0).all()
    err = np.abs(got - iou.numpy()).max()
    print("anchor-unit IoU against the oracle's decoded float32 IoU: %.3e" % err)
    assert err <= 1e-4


@pytest.mark.parametrize("spec", ref.SPECS)
def test_reference_gradients_against_central_differences(spec):
    """Rows without ties, step 1e-6 in float64: the truncation term is O(step^2) and rounding 1e-16 / 1e-6, so 1e-7 of the largest
    gradient is ample; a row whose difference straddles a kink of max / min / Huber is left out (its two one-sided slopes differ)."""
    p, l = _random_pairs(48, 11)
    lab = np.zeros((48, 3), np.float32)
    lab[np.arange(48), np.arange(48) % 3] = 1.0
    inp = ref.Inputs(3, (48,), lab, p, l, np.ones(48, bool), {})
    base = ref.regr_terms_ref(inp, spec, 1.0)
    step, worst = 1e-6, 0.0

    def side(t):                                        # the predicates a step must not flip
        t0, t1, t2, t3, _ = [x.numpy() for x in ref.corners(torch.from_numpy(t))]
        l0, l1, l2, l3, _ = [x.numpy() for x in ref.corners(torch.from_numpy(l))]
        return np.stack([t0 > l0, t1 > l1, t2 > l2, t3 > l3, t2 > l0, t3 > l1, l2 > t0, l3 > t1] +
                        [np.abs(t - l)[:, k] > d for k in range(4) for d in (1.0, 0.11)], 1)
    for k in range(4):
        hi, lo = p.copy(), p.copy()
        hi[:, k] += step
        lo[:, k] -= step
        keep = (side(hi) == side(lo)).all(1)
        assert keep.sum() >= 40
        for row in np.flatnonzero(keep):                # the loss is a sum over rows: one row at a time
            a, b = p.copy(), p.copy()
            a[row, k] += step
            b[row, k] -= step
            num = (ref.regr_terms_ref(inp._replace(rp=a), spec, 1.0).loss - ref.regr_terms_ref(inp._replace(rp=b), spec, 1.0).loss) / (2 * step)
            worst = max(worst, abs(num - base.dr[row, k]))
    scale = np.abs(base.dr).max()
    print("%s: central differences against autograd %.3e (largest gradient %.3e)" % (spec, worst, scale))
    assert worst <= 1e-7 * scale


def test_huber_1_1_is_the_oracles_regression_loss():
    for name in ("levels-c20", "r257-c3", "no_fg-c20", "all_fg-c3"):
        inp = ref.case(name)
        m = torch.tensor(inp.mask)
        rp = torch.tensor(inp.rp).double().requires_grad_(True)
        lab, rl = torch.tensor(inp.lab).double(), torch.tensor(inp.rl).double()
        want = losses_ref.regression_loss(rl[m], rp[m], losses_ref.fg_mask_of(lab[m]))
        got = ref.regr_terms_ref(inp, "huber:1:1", 1.0)
        assert abs(got.loss - want.item()) <= 1e-14 * max(1.0, abs(want.item()))
        if want.requires_grad and got.nfg:
            want.backward()
            assert np.abs(rp.grad.numpy() - got.dr).max() <= 1e-15
        assert got.nfg == int(losses_ref.fg_mask_of(lab[m]).sum())


def test_ranges_of_the_overlap_measures():
    for noise, seed in ((0.4, 1), (2.0, 2), (1e-3, 3)):
        p, l = _random_pairs(4096, seed, noise)
        iou, giou = ref.iou_giou(torch.from_numpy(p), torch.from_numpy(l))
        assert ((1 - iou) >= 0).all() and ((1 - iou) <= 1).all()
        assert (giou >= -1).all() and (giou <= 1).all() and (giou <= iou + 1e-15).all()
    one = torch.tensor([[0.3, -0.2, 0.2, -0.4]], dtype=torch.float64)
    iou, giou = ref.iou_giou(one, one.clone())
    assert abs(iou.item() - 1) <= 1e-15 and abs(giou.item() - 1) <= 1e-15


def test_case_table_covers_what_it_must():
    """Both label paths (C % 4 == 0 and not), the small ends, the grid wrap, every planted geometry, the degenerate masks."""
    assert {c.c for c in ref.CASE_LIST} == {1, 3, 20, 80}
    assert {1, 63, 64, 65, 257} <= {c.rows[0] for c in ref.CASE_LIST if len(c.rows) == 1}
    assert any(len(c.rows) == 5 and all(r % 64 for r in c.rows) and c.rows[-1] == 9 for c in ref.CASE_LIST)    # ragged pyramid levels
    for name in ("wrap-c20", "wrap-c1"):
        assert sum(ref.CASES[name].rows) > ref.WRAP_ROWS
    text = open(os.path.join(ROOT, "retinanet-tensorflow_amd", "csrc", "regr_terms.hip")).read()
    const = lambda n: int(re.search(r"constexpr int %s = ([^;]+);" % n, text).group(1).replace("T / 64", "4").replace("RPW * WAVES", "64"))
    assert const("FWD_BLOCKS") * const("RPB") == ref.WRAP_ROWS == const("BWD_BLOCKS") * const("T")
    inp = ref.case("planted-c20")
    want = ref.ref("planted-c20", "giou", 1.0)
    iou, _ = ref.iou_giou(torch.tensor(inp.rp).double(), torch.tensor(inp.rl).double())
    for key in ("disjoint", "disjoint_both", "touching"):
        assert iou[inp.planted[key]] == 0 and want.fg_rows[inp.planted[key]] == 1
    assert iou[inp.planted["identical"]] == 1
    assert ref.ref("no_fg-c20", "giou").nfg == 0 and ref.ref("no_trainable-c20", "giou").nfg == 0
    assert ref.ref("all_fg-c20", "giou").nfg == 65
    d = ref.case("levels-c20")
    assert ((d.lab.max(1) > 0.5) & ~d.mask).any()          # fg-labelled rows outside the trainable mask
