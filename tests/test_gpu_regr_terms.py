"""The box regression loss as a weighted sum of Huber / IoU / GIoU terms on the MI355X (-m gpu): csrc/regr_terms.hip through
ops.regression_terms against the float64 autograd reference of tests/regr_terms_ref.py on every case of its table -- loss, the
sums of the statistics, fg_rows exactly, d_reg_pred element by element --, the exact-value, masking and reproducibility
properties, the route through losses.loss, the one-graph training step and the command line.

The bar: assert_close(got, want, 1e-4, elementwise_tol=1e-4), as tests/test_gpu_loss_terms.py.  A quantity of a case may exceed
1e-4 element-wise only while the float32 torch evaluation of the SAME reference formulas on the same input exceeds 2.5e-5 on that
quantity; its bar is then 4 x that float32 figure (the factor the GroupNorm and Winograd case tests give a kernel over the fp32
reference).  Every use of that rule is printed, counted in RELAXED and marked in profiles/regr_terms_err.txt, which the module
writes when it ends with every case's figures.  Identical boxes are compared absolutely (|loss| <= 1e-6): float64 leaves 1e-16
there and a relative figure says nothing."""
import collections
import os

import numpy as np
import pytest
import torch

import regr_terms_ref as ref
import test_gpu_train_metrics as tm
from helpers import assert_close, elementwise_rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
F32_FLOOR = 2.5e-5
G_REG = ref.G_REG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = collections.OrderedDict()        # (case, spec) -> {quantity: (error, bar)}
RELAXED = []                               # (case, spec, quantity, error, float32 figure): where the 4 x float32 bar was used


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    yield torch.device("cuda:0")
    lines = ["regression-loss terms (csrc/regr_terms.hip) against float64, element-wise relative error (tests/helpers.py) per case and spec;",
             "bar 1e-4, or 4 x the float32 torch evaluation of the reference where that exceeds 2.5e-5 (marked *; used %d times)" % len(RELAXED),
             "", "%-18s %-26s %-11s %-11s %-11s %-11s %-11s %-11s" % ("case", "spec", "loss", "sum huber", "sum 1-IoU", "sum 1-GIoU", "sum IoU", "d_reg_pred")]
    for (name, spec), q in FIGURES.items():
        cells = ["%.2e%s" % (q[k][0], "*" if q[k][1] > TOL else " ") if k in q else "-" for k in ("loss", "s_huber", "s_iou_l", "s_giou_l", "s_iou", "dr")]
        lines.append("%-18s %-26s %-11s %-11s %-11s %-11s %-11s %-11s" % tuple([name, spec] + cells))
    for r in RELAXED:
        lines.append("* %s %s %s: %.3e against float64, float32 torch %.3e -> bar %.3e" % (r + (4 * r[4],)))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    if len(FIGURES) >= len(ref.CASE_LIST) * len(ref.SPECS):          # the whole table ran
        with open(os.path.join(ROOT, "profiles", "regr_terms_err.txt"), "w") as f:
            f.write(text)


def _t(a, dev, grad=False):
    return torch.tensor(np.ascontiguousarray(a), device=dev).requires_grad_(grad)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


Got = collections.namedtuple("Got", "loss stats fg_rows dr")


def _run(dev, inp, spec, g_reg=G_REG):
    """ops.regression_terms and its backward on the segments of `inp`."""
    import ops
    segs = ref.segments(inp)
    rg = [_t(s[1], dev, True) for s in segs]
    loss, stats = ops.regression_terms(rg, [_t(s[2], dev) for s in segs], [_t(s[0], dev) for s in segs],
                                       [_t(s[3].astype(np.uint8), dev) for s in segs], inp.c, spec)
    assert not stats.requires_grad and loss.requires_grad
    fg_rows = loss.grad_fn.saved_tensors[1].cpu().numpy()
    (g_reg * loss).backward()
    torch.cuda.synchronize()
    return Got(loss.item(), stats.cpu().numpy(), fg_rows, np.concatenate([t.grad.cpu().numpy() for t in rg]))


def _close(name, spec, key, got, want, f32_of):
    """The bar of the module docstring on one quantity; f32_of(): the float32 torch figure, evaluated only when needed."""
    e = elementwise_rel_err(got, want)
    bar = TOL
    if e > TOL:
        f = f32_of()
        if f > F32_FLOOR:
            bar = 4.0 * f
            RELAXED.append((name, spec, key, e, f))
            print("%s %s %s: %.3e > 1e-4 while float32 torch shows %.3e: bar %.3e" % (name, spec, key, e, f, bar))
    FIGURES.setdefault((name, spec), {})[key] = (e, bar)
    print("%s %s %s: element-wise %.3e (bar %.1e)" % (name, spec, key, e, bar))
    assert_close(got, want, bar, "%s %s %s" % (name, spec, key), elementwise_tol=bar)
    return e


def _close_or_zero(got, want, what):
    """giou alone at identical boxes has gradient 0 (test_exact_values_on_planted_geometry): float64 leaves 1e-17 there, and the
    comparison is absolute, against 1e-6 of the per-row factor g_reg * weight / #fg <= G_REG here."""
    if np.abs(want).max() <= 1e-12:
        assert np.abs(got).max() <= 1e-6 * G_REG, (what, np.abs(got).max())
    else:
        assert_close(got, want, TOL, what, elementwise_tol=TOL)


def _check(dev, name, spec):
    inp = ref.case(name)
    got, want = _run(dev, inp, spec), ref.ref(name, spec)
    f32 = {}

    def f32_of(key):
        def f():
            if not f32:
                f32["r"] = ref.regr_terms_ref(inp, spec, G_REG, torch.float32)
            return elementwise_rel_err(getattr(f32["r"], key), getattr(want, key))
        return f
    assert got.stats.shape == (8,) and got.stats[0] == np.float32(got.loss) and not got.stats[6:].any()
    assert np.array_equal(got.fg_rows, want.fg_rows) and got.fg_rows.dtype == np.uint8
    assert got.stats[1] == want.nfg
    identical = ref.CASES[name].recipe == "identical"
    overlap = ref.has(spec, "iou") or ref.has(spec, "giou")
    if identical and overlap:
        assert abs(got.loss) <= 1e-6 and abs(got.stats[3]) <= 1e-6 * want.nfg and abs(got.stats[4]) <= 1e-6 * want.nfg, (got.loss, got.stats)
        FIGURES.setdefault((name, spec), {})
    else:
        _close(name, spec, "loss", got.loss, want.loss, f32_of("loss"))
        for key, idx in (("s_huber", 2), ("s_iou_l", 3), ("s_giou_l", 4)):
            _close(name, spec, key, got.stats[idx], getattr(want, key), f32_of(key))
    _close(name, spec, "s_iou", got.stats[5], want.s_iou, f32_of("s_iou"))
    if not ref.has(spec, "huber"):
        assert got.stats[2] == 0
    if not overlap:
        assert not got.stats[3:6].any()
    if identical and np.abs(want.dr).max() <= 1e-12:
        _close_or_zero(got.dr, want.dr, "%s %s dr" % (name, spec))
    else:
        _close(name, spec, "dr", got.dr, want.dr, f32_of("dr"))
    assert not got.dr[want.fg_rows == 0].any()                     # exact zeros on rows that are not fg, every element written
    assert np.isfinite(got.dr).all()
    return got, want


# --------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("name", list(ref.CASES))
def test_case_table(dev, name):
    for spec in ref.SPECS:
        _check(dev, name, spec)


def test_exact_values_on_planted_geometry(dev):
    inp = ref.case("planted-c20")
    rows = [inp.planted[k] for k in ("disjoint", "disjoint_both", "touching")]
    iou, giou = _run(dev, inp, "iou"), _run(dev, inp, "giou")
    assert iou.fg_rows[rows].all() and not iou.dr[rows].any()                # disjoint: IoU has no slope ...
    assert (np.abs(giou.dr[rows]).max(1) > 0).all()                          # ... GIoU has one
    want = ref.ref("planted-c20", "giou")
    for r in rows:
        assert_close(giou.dr[r], want.dr[r], TOL, "giou gradient of a disjoint row", elementwise_tol=TOL)
    # identical boxes inside a mixed case: the gradient of the convention (every predicate true).  IoU: growing the prediction
    # grows I and area(p) alike, d(1 - IoU)/d(th) = -1; GIoU: the enclosure grows as well, (E - U)/E adds +1, the sum is 0
    r = inp.planted["identical"]
    k = G_REG / want.nfg
    w = ref.ref("planted-c20", "iou").dr[r]
    assert np.abs(w - [0, 0, -k, -k]).max() <= 1e-15
    assert iou.dr[r][0] == 0 and iou.dr[r][1] == 0
    assert_close(iou.dr[r], w, TOL, "iou gradient at identical boxes", elementwise_tol=TOL)
    assert np.abs(want.dr[r]).max() <= 1e-15 and giou.dr[r][0] == 0 and giou.dr[r][1] == 0
    assert np.abs(giou.dr[r]).max() <= 1e-6 * k, giou.dr[r]


def test_identical_boxes(dev):
    inp = ref.case("identical-c20")
    for spec in ("iou", "giou", "huber:0.5+iou:0.7+giou:2"):
        got, want = _run(dev, inp, spec), ref.ref("identical-c20", spec)
        assert abs(got.loss) <= 1e-6, got.loss
        assert abs(got.stats[5] - want.nfg) <= 1e-6 * want.nfg
        _close_or_zero(got.dr, want.dr, "%s gradient at identical boxes" % spec)


def test_no_foreground_and_no_trainable_row(dev):
    for name in ("no_fg-c20", "no_trainable-c20"):
        for spec in ref.SPECS:
            got = _run(dev, ref.case(name), spec)
            assert got.loss == 0 and not got.stats.any() and not got.fg_rows.any() and not got.dr.any()
            assert np.array_equal(_bits(got.dr), np.zeros_like(_bits(got.dr)))


# ----------------------------------------------------------------------------------------------------------------- masking
def _planted_nan(kind):
    """levels-c20 with one row's regression label set to NaN (and, on the background row, exp(th) of the prediction overflowing)."""
    inp = ref.case("levels-c20")
    fg_label = inp.lab.max(1) > 0.5
    row = {"non_trainable": np.flatnonzero(~inp.mask & fg_label)[0], "background": np.flatnonzero(inp.mask & ~fg_label)[3],
           "fg": np.flatnonzero(inp.mask & fg_label)[2]}[kind]
    rl, rp = inp.rl.copy(), inp.rp.copy()
    rl[row] = np.nan
    if kind != "fg":
        rp[row, 2] = 100.0            # exp overflows in float32
    return inp._replace(rl=rl, rp=rp), row


@pytest.mark.parametrize("spec", ref.SPECS)
def test_masking_with_planted_nans(dev, spec):
    clean = _run(dev, ref.case("levels-c20"), spec)
    assert np.isfinite(clean.loss)
    dirty, row = _planted_nan("non_trainable")                     # never read into a sum: no bit changes
    got = _run(dev, dirty, spec)
    assert np.array_equal(_bits(got.stats), _bits(clean.stats)) and np.array_equal(_bits(got.dr), _bits(clean.dr))
    assert np.array_equal(got.fg_rows, clean.fg_rows) and not got.dr[row].any()
    dirty, row = _planted_nan("background")                        # trainable, not fg: the overlap terms select, huber multiplies
    got = _run(dev, dirty, spec)
    assert not got.dr[row].any() and np.array_equal(got.fg_rows, clean.fg_rows)
    if ref.has(spec, "huber"):
        assert np.isnan(got.loss)
    else:
        assert np.array_equal(_bits(got.stats), _bits(clean.stats)) and np.array_equal(_bits(got.dr), _bits(clean.dr))
    dirty, row = _planted_nan("fg")
    assert np.isnan(_run(dev, dirty, spec).loss)


# ------------------------------------------------------------------------------------- against the existing Huber kernels
@pytest.mark.parametrize("name", ["levels-c20", "levels-c3", "r257-c80", "no_fg-c20"])
def test_huber_1_1_through_the_new_kernels_is_the_existing_regression_loss(dev, name):
    """ops.regression_terms always runs csrc/regr_terms.hip (the choice of route is losses.loss's): 'huber:1:1' there against
    rn_loss_fwd's stats[1] and rn_loss_bwd's d_reg_pred."""
    import ops
    inp = ref.case(name)
    segs = ref.segments(inp)
    rg = [_t(s[1], dev, True) for s in segs]
    rng = np.random.default_rng(0)
    z = [_t(rng.standard_normal(s[0].shape).astype(np.float32), dev) for s in segs]
    _, regr, stats = ops.detection_loss(z, rg, [_t(s[0], dev) for s in segs], [_t(s[2], dev) for s in segs],
                                        [_t(s[3].astype(np.uint8), dev) for s in segs], inp.c, "bce_dice")
    (G_REG * regr).backward()
    want_dr = np.concatenate([t.grad.cpu().numpy() for t in rg])
    got = _run(dev, inp, "huber:1:1")
    print("%s: huber:1:1 %.9g against rn_loss_fwd %.9g" % (name, got.loss, stats[1].item()))
    assert_close(got.loss, stats[1].item(), TOL, "huber:1:1 against rn_loss_fwd", elementwise_tol=TOL)
    assert got.stats[1] == stats[3].item()
    assert_close(got.dr, want_dr, TOL, "huber:1:1 d_reg_pred against rn_loss_bwd", elementwise_tol=TOL)


def _detection(inp, dev, grad):
    import utils
    keys = ["P%d" % (3 + i) for i in range(len(inp.rows))]
    segs = ref.segments(inp)
    rng = np.random.default_rng(1)
    z = {k: _t(rng.standard_normal(s[0].shape).astype(np.float32), dev, grad) for k, s in zip(keys, segs)}
    rp = {k: _t(s[1], dev, grad) for k, s in zip(keys, segs)}
    lab = {k: _t(s[0], dev) for k, s in zip(keys, segs)}
    rl = {k: _t(s[2], dev) for k, s in zip(keys, segs)}
    masks = {k: _t(s[3].astype(np.uint8), dev) for k, s in zip(keys, segs)}
    logits = utils.Detection(classification=utils.Classification(unscaled=z, prob=None), regression=rp, regression_postprocessed=None)
    labels = utils.Detection(classification=utils.Classification(unscaled=None, prob=lab), regression=rl, regression_postprocessed=None)
    return labels, logits, masks


def _through_losses(dev, regr_mode, mode="bce_dice", **kw):
    import losses
    labels, logits, masks = _detection(ref.case("levels-c20"), dev, True)
    cl, rl = losses.loss(labels, logits, trainable_masks=masks, mode=mode, regr_mode=regr_mode, **kw)
    (cl + G_REG * rl).backward()
    torch.cuda.synchronize()
    dz = np.concatenate([t.grad.cpu().numpy() for t in logits.classification.unscaled.values()])
    dr = np.concatenate([t.grad.cpu().numpy() for t in logits.regression.values()])
    return cl.item(), rl.item(), dz, dr


def test_none_and_huber_through_losses_loss_are_the_same_bits(dev):
    import losses
    labels, logits, masks = _detection(ref.case("levels-c20"), dev, True)
    cl, rl = losses.loss(labels, logits, trainable_masks=masks)           # the call as it was before the argument existed
    (cl + G_REG * rl).backward()
    base = (cl.item(), rl.item(), np.concatenate([t.grad.cpu().numpy() for t in logits.classification.unscaled.values()]),
            np.concatenate([t.grad.cpu().numpy() for t in logits.regression.values()]))
    for regr_mode in (None, "huber", "huber:1:1", losses.parse_regr_loss("huber")):
        got = _through_losses(dev, regr_mode)
        assert np.float32(got[0]).tobytes() == np.float32(base[0]).tobytes() and np.float32(got[1]).tobytes() == np.float32(base[1]).tobytes()
        assert np.array_equal(_bits(got[2]), _bits(base[2])) and np.array_equal(_bits(got[3]), _bits(base[3]))


@pytest.mark.parametrize("mode", ["bce_dice", "focal", "bce+jaccard"])
def test_spec_through_losses_loss(dev, mode):
    """Another spec: the class loss and its gradient keep the bits of the default route in every class-loss mode, the regression loss
    and d_reg_pred are those of the new kernels (the class-loss kernels see the box predictions detached)."""
    spec = "huber:0.5+giou:2"
    base, got = _through_losses(dev, None, mode), _through_losses(dev, spec, mode)
    want = ref.ref("levels-c20", spec)
    assert np.float32(got[0]).tobytes() == np.float32(base[0]).tobytes() and np.array_equal(_bits(got[2]), _bits(base[2]))
    assert_close(got[1], want.loss, TOL, "regr loss of %s through losses.loss" % spec, elementwise_tol=TOL)
    assert_close(got[3], want.dr, TOL, "d_reg_pred of %s through losses.loss" % spec, elementwise_tol=TOL)
    direct = _run(dev, ref.case("levels-c20"), spec)
    assert np.float32(got[1]).tobytes() == np.float32(direct.loss).tobytes()


@pytest.mark.parametrize("name", ["levels-c20", "levels-c3", "wrap-c20"])
def test_bitwise_reproducible(dev, name):
    spec = "huber:0.5+iou:0.7+giou:2"
    a, b = _run(dev, ref.case(name), spec), _run(dev, ref.case(name), spec)
    assert np.float32(a.loss).tobytes() == np.float32(b.loss).tobytes()
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------------------ in the step
STEP_SPEC = "huber:0.5+giou:2"
feats = tm.feats          # (the module-scoped fixture with that trainer's inputs)


def _same_run(a, b):
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    for k in ("weights", "state1", "state2", "drop_counter"):
        assert tm._same(a["state"][k], b["state"][k]), k


@pytest.mark.parametrize("train_metrics", [False, True])
def test_spec_in_the_step_is_one_graph_and_equals_eager(dev, feats, train_metrics):
    """Four scheduled-Adam steps (tests/test_gpu_train_metrics.py's trainer) with regr_loss='huber:0.5+giou:2': ONE graph, captured
    once, bit-identical to eager launches in losses, weights and both optimizer slots; with the training metrics the window's
    regr_loss mean is the float64 mean of the steps' own regression losses, which are not the Huber ones."""
    import losses, metrics
    g = tm._run(dev, feats, True, train_metrics, regr_loss=STEP_SPEC)
    e = tm._run(dev, feats, False, train_metrics, regr_loss=STEP_SPEC)
    tr = g["trainer"]
    assert tr.regr_loss == losses.parse_regr_loss(STEP_SPEC)
    assert tr._graphs[5] and len(tr._graph_cache) == 1 and tr.recaptures == 0
    _same_run(g, e)
    assert all(np.isfinite(l).all() for l in g["losses"])
    huber = tm._run(dev, feats, True, False)
    assert huber["losses"][0][0] == g["losses"][0][0] and huber["losses"][0][1] != g["losses"][0][1]     # same first class loss, another box loss
    if train_metrics:
        sums, counts = g["raw"]
        assert counts[0] == tm.STEPS and counts[1] == 0
        want = sum(np.float64(l[1]) for l in g["losses"])
        assert sums[2] == want
        assert metrics.window_result(sums, counts)["regr_loss"] == want / tm.STEPS
        assert np.array_equal(g["raw"][0].view(np.uint64), e["raw"][0].view(np.uint64))


def test_no_spec_and_huber_are_the_same_trainer(dev, feats):
    _same_run(tm._run(dev, feats, True, False), tm._run(dev, feats, True, False, regr_loss="huber"))


def test_cli_trains_with_a_regr_loss_spec(capsys):
    import train
    argv = ["--dataset", "shapes", "--epochs", "5", "--steps-per-epoch", "4", "--scale", "128", "--backbone", "mobilenet_v2",
            "--regr-loss", "giou:2"]                            # (the losses are printed every 20th step)
    assert train.main(argv) == 20
    out = capsys.readouterr().out.splitlines()
    assert [l for l in out if l.startswith("regr loss:")] == ["regr loss: 2 * giou"]
    assert not [l for l in out if l.startswith("class loss:")]
    lines = [l for l in out if "class_loss" in l]
    assert len(lines) == 1
    for key in ("class_loss ", "regr_loss "):
        assert np.isfinite(float(lines[-1].split(key)[1].split()[0]))
    with pytest.raises(SystemExit) as e:
        train.main(argv[:-1] + ["giou:2+ciou"])
    assert e.value.code == 2 and "--regr-loss: regr loss spec 'giou:2+ciou': term 'ciou': unknown name" in capsys.readouterr().err
