"""ONE bottleneck (case 20: two) through ops_mb.mb_chain -- the call mobilenet_v2.MobileNetV2.call makes, with hand-built
ops_mb.Block / ops_mb.Norm lists -- at every planner branch of csrc/mbconv.hip, against the fp64 evaluation of
tests/mbchain_ref.chain_ref.  The cases and the branch each one takes: mbchain_ref.CASES and tests/test_mbchain_cases_cpu.py
(which proves the branches on the CPU).  Compared: every tap and the raw tail output, the gradient of x, of the nine tensors
of every block and of the tail kernel, each against ITS OWN maximum (helpers.rel_err) -- no floor shared between tensors.

Two bars per tensor:
  * the project's: outputs 1e-4 (BASELINE north_star), gradients 5e-4;
  * one tied to the arithmetic: with e32 = rel_err(chain_ref in fp32, chain_ref in fp64) and ek = rel_err(kernel, fp64),
    ek / max(e32, 2^-23) <= RATIO_BOUND.  The kernels sum in fp32 in another order than torch does (MFMA K-tiles, split-K inside
    a block, fp64-merged statistic rows, per-block weight-gradient partial sums), so a ratio of a few is expected; they are
    bitwise reproducible, so it has no run-to-run noise.  e32 comes from the reference alone.
RATIO_BOUND = 4, set on 2026-10-19 from one run of the table on an MI355X (figures: profiles/mbchain_cases_err.txt): the
largest ratio of any tensor of any case was 1.50 (case 9, the gradient of gamma2); twice that, rounded up to a power of two.
The largest ek was 4.9e-7 for an output and 1.8e-6 for a gradient: 200 and 270 times inside the project's bars."""
import numpy as np
import pytest
import torch

import mbchain_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR = 1e-4, 5e-4
RATIO_BOUND = 4.0
RUNS = [(cid, False) for cid in R.CASES] + [(20, True)]       # (case, the tail kernel is the constant identity of a stage cut)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_chain(cid, tail_identity, dev, training=True, rate=None):
    """The case through ops_mb.mb_chain on `dev` -> ({output name: tensor}, {gradient name: tensor}); training=False: under
    torch.no_grad(), no gradients.  rate: the rate the Norms carry (default: the case's)."""
    import ops_mb
    case = R.CASES[cid]
    x, blocks, tail_w = R.make_case(case, tail_identity)
    rate = case.rate if rate is None else rate

    def leaf(t):
        return t.to(dev).requires_grad_(training)

    def norm(nm, act):
        return ops_mb.Norm(leaf(nm.gamma), leaf(nm.beta), nm.groups_arg, nm.eps, act, rate, nm.seed)

    xd = leaf(x)
    gb = [ops_mb.Block(leaf(b.w1), norm(b.n1, case.act), leaf(b.wd), norm(b.n2, case.act), leaf(b.w3), norm(b.n3, None), b.stride, b.residual)
          for b in blocks]
    tw = tail_w.to(dev) if tail_identity else leaf(tail_w)
    leaves = [xd] + [t for b in gb for t in (b.w1, b.n1.gamma, b.n1.beta, b.wd, b.n2.gamma, b.n2.beta, b.w3, b.n3.gamma, b.n3.beta)]
    if not tail_identity:
        leaves.append(tw)
    seed_dev = torch.tensor([case.counter], dtype=torch.int64, device=dev) if case.counter else None
    taps = sorted(case.taps)
    if not training:
        with torch.no_grad():
            got, tail = ops_mb.mb_chain(xd, gb, tw, taps, training=False, seed_dev=seed_dev, tail_const=tail_identity)
        return dict([("tap%d" % i, t) for i, t in zip(taps, got)] + [("tail", tail)]), {}
    got, tail = ops_mb.mb_chain(xd, gb, tw, taps, training=True, seed_dev=seed_dev, tail_const=tail_identity)
    cot = [c.to(dev) for c in R.make_cotangents(case, tail_w.shape[3])]
    torch.autograd.backward(list(got) + [tail], cot)
    names = R.grad_names(len(gb), not tail_identity)
    assert all(t.grad is not None for t in leaves), [n for n, t in zip(names, leaves) if t.grad is None]
    out = dict([("tap%d" % i, t.detach()) for i, t in zip(taps, got)] + [("tail", tail.detach())])
    return out, {k: t.grad for k, t in zip(names, leaves)}


def measure(cid, tail_identity, dev):
    """-> [(kind "out" / "grad", tensor name, ek, e32, ratio)] for every compared tensor of the case"""
    out, grads = run_chain(cid, tail_identity, dev)
    ref64 = R.reference(cid, torch.float64, tail_identity)
    ref32 = R.reference(cid, torch.float32, tail_identity)
    rows = []
    for kind, got, r64, r32 in (("out", out, ref64[0], ref32[0]), ("grad", grads, ref64[1], ref32[1])):
        assert sorted(got) == sorted(r64)
        for name in r64:
            g = got[name].cpu().numpy()
            assert g.shape == r64[name].shape and np.isfinite(g).all(), name
            ek, e32 = rel_err(g, r64[name]), rel_err(r32[name], r64[name])
            rows.append((kind, name, ek, e32, ek / max(e32, 2.0 ** -23)))
    return rows


def worst(rows, kind):
    return max((r for r in rows if r[0] == kind), key=lambda r: r[4])


@pytest.mark.parametrize("cid,tail_identity", RUNS, ids=["%d%s" % (c, "-const-tail" if t else "") for c, t in RUNS])
def test_case_matches_fp64(dev, cid, tail_identity):
    rows = measure(cid, tail_identity, dev)
    for kind in ("out", "grad"):
        print("case %d%s worst %s ratio: %s ek %.3e e32 %.3e ratio %.2f" % ((cid, " const tail" if tail_identity else "", kind) + worst(rows, kind)[1:]))
    bad = ["%s %s: ek %.3e (bar %.0e), e32 %.3e, ratio %.2f (bound %s)" % (kind, name, ek, OUT_BAR if kind == "out" else GRAD_BAR, e32, ratio, RATIO_BOUND)
           for kind, name, ek, e32, ratio in rows
           if ek > (OUT_BAR if kind == "out" else GRAD_BAR) or ratio > RATIO_BOUND]
    assert not bad, "case %d: %d of %d tensors off: %s" % (cid, len(bad), len(rows), "; ".join(bad))


@pytest.mark.parametrize("cid", [1, 10])
def test_second_run_is_bit_identical(dev, cid):
    """"No atomics; results are bitwise reproducible" (include/rn_hip.h): outputs and every gradient."""
    out_a, grads_a = run_chain(cid, False, dev)
    out_b, grads_b = run_chain(cid, False, dev)
    for a, b in ((out_a, out_b), (grads_a, grads_b)):
        for name in a:
            assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("cid,tail_identity", [(3, False), (20, False), (20, True)], ids=["3", "20", "20-const-tail"])
def test_inference_ignores_the_dropout_rate(dev, cid, tail_identity):
    """training=False under torch.no_grad(): taps and tail equal the dropout-off reference although the Norms carry rate 0.2."""
    out, _ = run_chain(cid, tail_identity, dev, training=False, rate=0.2)
    ref64, _ = R.reference(cid, torch.float64, tail_identity, False)
    ref32, _ = R.reference(cid, torch.float32, tail_identity, False)
    assert sorted(out) == sorted(ref64)
    for name in ref64:
        ek, e32 = rel_err(out[name].cpu().numpy(), ref64[name]), rel_err(ref32[name], ref64[name])
        ratio = ek / max(e32, 2.0 ** -23)
        print("case %d inference %s: ek %.3e e32 %.3e ratio %.2f" % (cid, name, ek, e32, ratio))
        assert ek <= OUT_BAR and ratio <= RATIO_BOUND, (name, ek, e32, ratio)
