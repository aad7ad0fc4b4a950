"""The class loss as a weighted sum of terms on the MI355X (-m gpu): csrc/loss_terms.hip through ops.detection_loss(mode=SPEC)
against the float64 autograd reference of tests/loss_terms_ref.py, element by element, on the inputs of step_tail_ref.loss_case:
every quads-per-lane instantiation of the four-lane kernels and the wave-per-row kernels, RN_MAX_SEG segments, the small ends,
both grids past their first pass, saturated logits, non-finite logits on masked rows; the two descriptors that must run the
existing kernels bit for bit; the spec inside the one-graph training step and on the command line.

The bar: assert_close(..., TOL, what, elementwise_tol=TOL) with TOL = 1e-4, as tests/test_gpu_step_tail.py.  On the planted
(saturated-logit) inputs alone it is max(TOL, 2 x the element-wise error the existing bce_dice mode shows on the same inputs in
the same run): there the distance to float64 is the device expf's against the float64 exp, which both kernel families share.
The worst element-wise error of every family is printed when the module ends (-s shows it).

Run as a program (RN_LOSS_TERMS_GENERAL=1 set by the parent test) it checks the general kernels on the two descriptors the
library otherwise hands to the existing ones."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "retinanet-tensorflow_amd"), os.path.join(_root, "tests")]

import loss_terms_ref as ref
import step_tail_ref
import test_gpu_ema as ema_tests
from helpers import assert_close, elementwise_rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
G_CLS, G_REG = step_tail_ref.G_CLS, step_tail_ref.G_REG
WORST = collections.OrderedDict()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    import _rn
    _rn.lib()          # fails loudly if librn_hip.so is missing
    yield torch.device("cuda:0")
    print("\nworst element-wise relative error against float64, by family (bar %.0e; planted: see the module docstring):" % TOL)
    for family, e in WORST.items():
        print("  %-28s %.3e" % (family, e))


def _t(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def _close(family, got, want, what, tol=TOL):
    e = elementwise_rel_err(got, want)
    WORST[family] = max(WORST.get(family, 0.0), e)
    print("%s [%s]: element-wise %.3e (bar %.1e)" % (what, family, e, tol))
    assert_close(got, want, tol, what, elementwise_tol=tol)
    return e


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


LossGot = collections.namedtuple("LossGot", "cls reg stats dz dr")


def _run(dev, inp, mode, g_cls=G_CLS, g_reg=G_REG):
    """ops.detection_loss and its backward on the segments of `inp`; mode: a spec, or 'bce_dice' / 'focal'."""
    import ops
    segs = step_tail_ref.segments(inp)
    zg = [_t(s[0], dev, True) for s in segs]
    rg = [_t(s[2], dev, True) for s in segs]
    cl, rl, stats = ops.detection_loss(zg, rg, [_t(s[1], dev) for s in segs], [_t(s[3], dev) for s in segs],
                                       [_t(s[4].astype(np.uint8), dev) for s in segs], inp.c, mode)
    total = 0.0
    if g_cls is not None:
        total = total + g_cls * cl
    if g_reg is not None:
        total = total + g_reg * rl
    total.backward()
    torch.cuda.synchronize()
    return LossGot(cl.item(), rl.item(), stats.cpu().numpy(), np.concatenate([t.grad.cpu().numpy() for t in zg]),
                   np.concatenate([t.grad.cpu().numpy() for t in rg]))


@functools.lru_cache(maxsize=None)
def _ref(name, spec, g_cls=G_CLS, g_reg=G_REG, dtype=torch.float64):
    return ref.loss_terms_ref(step_tail_ref.loss_case(name), spec, g_cls, g_reg, dtype)


def _check(inp, spec, got, want, tag, tol=TOL, keep=None, cls_want=None):
    """Everything the general kernels return against the reference.  `keep`: the elements of dz that are compared; `cls_want`:
    another expected class loss than the float64 one."""
    import _rn
    H, C = _rn.LOSS_STATS_HEADER, inp.c
    assert got.stats.shape == (H + 5 * C,)
    _close("class loss", got.cls, want.cls if cls_want is None else cls_want, "%s class loss" % tag, tol)
    _close("regr loss", got.reg, want.reg, "%s regr loss" % tag, tol)
    assert got.stats[0] == np.float32(got.cls) and got.stats[1] == np.float32(got.reg)
    assert got.stats[2] == want.M and got.stats[3] == want.nfg, (got.stats[:4], want.M, want.nfg)
    per_class = got.stats[H:H + 3 * C].reshape(C, 3)
    for col, (what, w) in enumerate((("I", want.I), ("L", want.L), ("P", want.P))):
        _close("I / L / P", per_class[:, col], w, "%s per-class %s" % (tag, what), tol)
    b1, b0 = got.stats[H + 3 * C:H + 4 * C], got.stats[H + 4 * C:]
    if any(name == "balanced_bce" for name, _, _ in ref.terms_of(spec)):
        _close("B1 / B0", b1, want.B1, "%s per-class B1" % tag, tol)
        _close("B1 / B0", b0, want.B0, "%s per-class B0" % tag, tol)
    else:
        assert not b1.any() and not b0.any()
    dz, dz_want = (got.dz, want.dz) if keep is None else (np.where(keep, got.dz, 0.0), np.where(keep, want.dz, 0.0))
    _close("dz, planted saturated logits" if tag.startswith("plant") else "dz", dz, dz_want, "%s d cls logits" % tag, tol)
    _close("dr", got.dr, want.dr, "%s d reg" % tag, tol)
    # rows outside the trainable mask: exactly zero (the buffers come from torch.empty: every element was written)
    assert not got.dz[~inp.mask].any() and not got.dr[~inp.mask].any()
    assert np.isfinite(got.dz).all() and np.isfinite(got.dr).all()


@functools.lru_cache(maxsize=None)
def _planted_bar(dev, name):
    """max(TOL, 2 x the worst element-wise error of the EXISTING bce_dice mode on these inputs, in this run)."""
    import _rn
    inp = step_tail_ref.loss_case(name)
    got, want = _run(dev, inp, "bce_dice"), step_tail_ref.loss_ref(inp, "bce_dice")
    per_class = got.stats[_rn.LOSS_STATS_HEADER:].reshape(inp.c, 3)
    pairs = [(got.cls, want.cls), (got.reg, want.reg), (got.dz, want.dz), (got.dr, want.dr)]
    pairs += [(per_class[:, i], w) for i, w in enumerate((want.I, want.L, want.P))]
    e = max(elementwise_rel_err(a, b) for a, b in pairs)
    print("existing bce_dice mode on %s: element-wise %.3e -> bar %.3e" % (name, e, max(TOL, 2.0 * e)))
    return max(TOL, 2.0 * e)


def _check_case(dev, name, spec):
    inp = step_tail_ref.loss_case(name)
    got, want = _run(dev, inp, spec), _ref(name, spec)
    tag = "%s %s" % (name, spec)
    if not name.startswith("plant"):
        return _check(inp, spec, got, want, tag)
    tol = _planted_bar(dev, name)
    if not ref.has_focal(spec):
        return _check(inp, spec, got, want, tag, tol)
    # focal at 12, 17, 30, 90 loses 1 - p against eps = 1e-7 in float32 (test_gpu_step_tail.test_loss_saturated_logits): those
    # elements are finite and of the right sign, and the class loss is compared with the float32 reference
    ill = step_tail_ref.ill_conditioned(inp, "focal")
    assert 0 < ill.sum() <= 12
    _check(inp, spec, got, want, tag, tol, keep=~ill, cls_want=_ref(name, spec, dtype=torch.float32).cls)
    assert np.isfinite(got.cls) and np.isfinite(got.dz[ill]).all()


# ------------------------------------------------------------------------------------------------------- general kernels
@pytest.mark.parametrize("name", step_tail_ref.SWEEP_CASES)
def test_dispatch_sweep_all_terms(dev, name):
    """All six terms at unequal weights and non-default smooths over C = 16 NK - 12 and 16 NK for every NK of the four-lane
    kernels and the wave-per-row kernels on both sides of their 64-class lanes; 1512 rows in five ragged segments."""
    _check_case(dev, name, ref.ALL_TERMS)


def _per_term_cases(c, spec):
    family = "focal" if ref.has_focal(spec) else "bce_dice"
    return ["sweep-%d" % c, "maxseg-%d" % c] + ["%s-%d" % (k, c) for k in ("one_row", "m1", "one_fg")] + ["plant-%s-%d" % (family, c)]


@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
@pytest.mark.parametrize("spec", ref.PER_TERM_SPECS)
def test_per_term(dev, spec, c):
    """Each new term alone and three mixtures, per kernel layout: the sweep inputs, RN_MAX_SEG segments, one row in all, one
    trainable row, one foreground row, and the planted saturated logits of the spec's family."""
    for name in _per_term_cases(c, spec):
        _check_case(dev, name, spec)


@pytest.mark.parametrize("name", step_tail_ref.WRAP_CASES)
def test_grid_wrap_all_terms(dev, name):
    _check_case(dev, name, ref.ALL_TERMS)


@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
def test_masked_rows_never_reach_a_sum(dev, c):
    """NaN, +inf and -inf logits on rows outside the trainable mask change nothing, bit for bit, and those rows get exactly 0."""
    clean, dirty = step_tail_ref.loss_case("clean-%d" % c), step_tail_ref.loss_case("nonfinite-%d" % c)
    rows = step_tail_ref.nonfinite_rows(c)
    a, b = _run(dev, clean, ref.ALL_TERMS), _run(dev, dirty, ref.ALL_TERMS)
    _check(clean, ref.ALL_TERMS, a, _ref("clean-%d" % c, ref.ALL_TERMS), "clean-%d" % c)
    assert (a.cls, a.reg) == (b.cls, b.reg), (a.cls, b.cls, a.reg, b.reg)
    assert np.array_equal(_bits(a.stats), _bits(b.stats))
    assert np.array_equal(_bits(a.dz), _bits(b.dz)) and np.array_equal(_bits(a.dr), _bits(b.dr))
    assert not b.dz[rows].any() and not b.dr[rows].any()


@pytest.mark.parametrize("name", ["clean-20", "clean-3", "wrap4"])
def test_bitwise_reproducible(dev, name):
    inp = step_tail_ref.loss_case(name)
    a, b = _run(dev, inp, ref.ALL_TERMS), _run(dev, inp, ref.ALL_TERMS)
    assert np.float32(a.cls).tobytes() == np.float32(b.cls).tobytes() and np.float32(a.reg).tobytes() == np.float32(b.reg).tobytes()
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("c", step_tail_ref.MASKING_C)
def test_backward_of_one_loss_alone(dev, c):
    name = "sweep-%d" % c
    inp = step_tail_ref.loss_case(name)
    got, want = _run(dev, inp, ref.ALL_TERMS, g_reg=None), _ref(name, ref.ALL_TERMS, G_CLS, None)
    assert not got.dr.any() and not want.dr.any()
    _check(inp, ref.ALL_TERMS, got, want, name + " class loss alone")
    got, want = _run(dev, inp, ref.ALL_TERMS, g_cls=None), _ref(name, ref.ALL_TERMS, None, G_REG)
    assert not got.dz.any() and not want.dz.any()
    _check(inp, ref.ALL_TERMS, got, want, name + " regr loss alone")


# ------------------------------------------------------------------------------------- the existing kernels by dispatch
LEGACY = (("bce+dice", "bce_dice"), ("focal:1", "focal"))      # ('focal' itself is the mode's name: the existing route)


@pytest.mark.parametrize("name", ["sweep-20", "sweep-3", "plant-bce_dice-20"])
@pytest.mark.parametrize("spec,mode", LEGACY)
def test_default_recipes_run_the_existing_kernels(dev, spec, mode, name):
    """{bce 1, dice 1:0} and {focal 1} through the spec route: losses, statistics [0, 8 + 3C) and both gradients carry the bits of
    mode='bce_dice' / 'focal'."""
    import _rn
    inp = step_tail_ref.loss_case(name)
    a, b = _run(dev, inp, spec), _run(dev, inp, mode)
    n = _rn.LOSS_STATS_HEADER + 3 * inp.c
    assert a.stats.shape == (n + 2 * inp.c,) and b.stats.shape == (n,)
    assert np.float32(a.cls).tobytes() == np.float32(b.cls).tobytes() and np.float32(a.reg).tobytes() == np.float32(b.reg).tobytes()
    assert np.array_equal(_bits(a.stats[:n]), _bits(b.stats))
    assert np.array_equal(_bits(a.dz), _bits(b.dz)) and np.array_equal(_bits(a.dr), _bits(b.dr))
    spelled_out = _run(dev, inp, "dice:1:0+bce:1" if mode == "bce_dice" else "focal:1.0")
    assert np.array_equal(_bits(spelled_out.dz), _bits(b.dz))


def _forced_general_child():
    """RN_LOSS_TERMS_GENERAL=1: the general kernels on the two default recipes, within the bar of float64 (I / L / P included, which
    the existing focal kernels of the four-lane layout leave at zero)."""
    assert os.environ.get("RN_LOSS_TERMS_GENERAL") == "1"
    dev = torch.device("cuda:0")
    for spec, _ in LEGACY:
        for name in ("sweep-20", "sweep-3"):
            _check_case(dev, name, spec)
    got = _run(dev, step_tail_ref.loss_case("sweep-20"), "focal:1")
    assert got.stats[8:8 + 60].any()
    print("FORCED GENERAL OK")


def test_forced_general_kernels_on_the_default_recipes(dev):
    env = dict(os.environ, RN_LOSS_TERMS_GENERAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FORCED GENERAL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    # and without the switch the existing focal kernels ran: they do not form the per-class sums at C = 20
    assert not _run(dev, step_tail_ref.loss_case("sweep-20"), "focal:1").stats[8:8 + 60].any()


# ------------------------------------------------------------------------------------------------------------ in the step
STEP_SPEC = "balanced_bce+jaccard"
STEPS = 8


def _build(dev, use_graph):
    """test_gpu_ema.py's small net and trainer (Adam on a schedule: the one-graph step with both slots, no moving average), its
    loss switched to the spec before the first step."""
    import losses
    net, tr = ema_tests._build(dev, use_graph, "adam", scheduled=True, ema=False)
    tr.loss_mode = losses.parse_class_loss(STEP_SPEC)
    return net, tr


feats = ema_tests.feats          # (the module-scoped fixture with that trainer's inputs)


def test_spec_in_the_step_is_one_graph_and_equals_eager(dev, feats, monkeypatch):
    """Eight Adam steps with loss_mode='balanced_bce+jaccard': ONE graph, captured once, bit-identical to eager launches in
    weights, both slots and the dropout counter; the first step's class loss against float64 on that step's logits and labels."""
    import losses
    _, tg = _build(dev, True)
    _, te = _build(dev, False)
    assert tg.loss_mode == losses.parse_class_loss(STEP_SPEC)
    seen = []
    real = losses.loss

    def spy(labels, logits, **kw):
        if not seen:
            keys = list(logits.regression.keys())
            masks = kw.get("trainable_masks") or labels.trainable_masks
            seen.append([np.concatenate([d[k].detach().cpu().numpy().reshape(-1, n) for k in keys]) for d, n in (
                (logits.classification.unscaled, 4), (labels.classification.prob, 4), (logits.regression, 4), (labels.regression, 4))]
                + [np.concatenate([masks[k].cpu().numpy().reshape(-1) for k in keys]).astype(bool)])
        return real(labels, logits, **kw)
    monkeypatch.setattr(losses, "loss", spy)
    first = te.step(feats)["class_loss"].item()
    monkeypatch.setattr(losses, "loss", real)
    for i in range(STEPS):
        tg.step(feats)
        if i:
            te.step(feats)
    torch.cuda.synchronize()
    assert tg._graphs[5] and len(tg._graph_cache) == 1 and tg.recaptures == 0
    assert torch.equal(tg.arena.weights, te.arena.weights)
    assert torch.equal(tg.opt.state1, te.opt.state1) and torch.equal(tg.opt.state2, te.opt.state2)
    assert torch.equal(tg.drop_counter, te.drop_counter) and tg.drop_counter.item() != 0
    z, lab, rp, rl, mask = seen[0]
    inp = step_tail_ref.LossInputs(4, (len(mask),), z, lab, rp, rl, mask, (), None)
    want = ref.loss_terms_ref(inp, STEP_SPEC, 1.0, 1.0)
    assert want.M > 0 and want.nfg > 0
    _close("class loss in the step", first, want.cls, "first step's class loss")


def test_cli_trains_with_a_class_loss_spec(tmp_path, capsys):
    import train
    argv = ["--dataset", "shapes", "--epochs", "1", "--steps-per-epoch", "20", "--scale", "128", "--backbone", "mobilenet_v2",
            "--dropout", "0.1", "--class-loss", "bce+jaccard"]
    assert train.main(argv) == 20
    out = capsys.readouterr().out.splitlines()
    assert [l for l in out if l.startswith("class loss:")] == ["class loss: 1 * bce + 1 * jaccard(smooth 1)"]
    lines = [l for l in out if "class_loss" in l]
    assert len(lines) == 1
    for key in ("class_loss ", "regr_loss "):
        assert np.isfinite(float(lines[0].split(key)[1].split()[0]))
    with pytest.raises(SystemExit) as e:
        train.main(argv + ["--loss", "focal"])
    assert e.value.code == 2 and "--class-loss with --loss focal" in capsys.readouterr().err


if __name__ == "__main__":
    _forced_general_child()
