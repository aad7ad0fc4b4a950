"""The MobileNetV2 bottleneck chain (ops_mb.mb_chain) restated in plain torch, in any dtype, for the tests, and the table of
cases that tests/test_mbchain_cases_cpu.py and tests/test_gpu_mbchain_cases.py share.

`chain_ref` is written from mb_chain's contract (reference mobilenet_v2.py:41-94, normalization.py:20-35), not from the
kernels, out of the oracle's ops (oracle/tf_ops_ref.py).  Per block, with a = the block's input:

    z1  = drop(act(GN(a w1)))
    z2  = drop(act(GN(dw3x3(z1, stride))))
    out = drop(GN(z2 w3)) [+ a]

and after the last block the RAW product out w_tail (the GroupNorm of the conv that follows the chain is not the chain's).
`drop` keeps element e of the tensor it acts on iff oracle.dropout_ref.uniform01(norm.seed + counter, e) >= rate and scales
by the kernels' fp32 1.f / (1.f - rate), promoted to the working dtype.  Gradients come from torch.autograd in that dtype.

A block is anything with the attributes of ops_mb.Block (w1, n1, wd, n2, w3, n3, stride, residual; a norm: gamma, beta,
groups_arg, eps, rate, seed): the `Block` / `Norm` tuples below on the CPU, ops_mb's own classes on the GPU.
"""
import collections
import functools

import numpy as np
import torch

from oracle import dropout_ref
from oracle import tf_ops_ref as T

Norm = collections.namedtuple("Norm", "gamma beta groups_arg eps rate seed")
Block = collections.namedtuple("Block", "w1 n1 wd n2 w3 n3 stride residual")
Spec = collections.namedtuple("Spec", "cin wide cout stride residual")
Case = collections.namedtuple("Case", "n h w specs act rate counter taps tail seed")
PARAM_NAMES = ("w1", "gamma1", "beta1", "wd", "gamma2", "beta2", "w3", "gamma3", "beta3")
EPS = 1e-5


def _case(n, h, w, *specs, act="elu", rate=0.0, counter=0, taps=None, tail=32, seed=0):
    specs = tuple(Spec(*s) for s in specs)
    return Case(n, h, w, specs, act, rate, counter, (len(specs) - 1,) if taps is None else tuple(taps), tail, seed)


# n, h, w, (cin, wide, cout, stride, residual) per block.  The tail kernel maps the last cout to `tail` channels (32: the
# width of MobileNetV2's output_conv).  `taps`: the blocks whose output leaves the chain; the last one unless said otherwise --
# cases 2, 7, 13 and 16 have none, so the backward pass without a tap gradient runs too.  What each case is for:
# tests/test_mbchain_cases_cpu.py (EXPECT) names the planner branches, tests/test_gpu_mbchain_cases.py the kernels.
CASES = collections.OrderedDict([
    (1, _case(2, 8, 8, (160, 960, 160, 1, True))),
    (2, _case(1, 16, 16, (160, 960, 320, 1, False), taps=())),
    (3, _case(2, 12, 16, (32, 192, 32, 1, True))),
    (4, _case(1, 64, 3, (32, 192, 64, 1, False))),
    (5, _case(1, 128, 5, (32, 192, 64, 2, False))),
    (6, _case(1, 5, 128, (32, 192, 64, 2, False))),
    (7, _case(1, 66, 64, (24, 144, 32, 1, False), taps=())),
    (8, _case(2, 24, 32, (20, 120, 28, 1, False))),
    (9, _case(1, 16, 16, (36, 216, 44, 2, False))),
    (10, _case(1, 128, 128, (24, 144, 24, 1, True))),
    (11, _case(2, 128, 128, (24, 144, 24, 1, True), rate=0.2, counter=3)),
    (12, _case(2, 128, 128, (16, 96, 16, 1, True))),
    (13, _case(1, 128, 128, (24, 144, 32, 2, False), taps=())),
    (14, _case(2, 64, 256, (16, 96, 24, 2, False))),
    (15, _case(1, 128, 128, (32, 32, 16, 1, False))),
    (16, _case(1, 128, 128, (12, 92, 20, 1, False), taps=())),
    (17, _case(1, 256, 256, (24, 144, 24, 1, True))),
    # relu6 / relu: `seed` is chosen so that no pre-activation lies within KINK_MARGIN of a kink (test_mbchain_cases_cpu.py)
    (18, _case(2, 12, 16, (32, 192, 32, 1, True), act="relu6", seed=2)),
    (19, _case(2, 12, 16, (32, 192, 32, 1, True), act="relu", rate=0.2, seed=22)),
    (20, _case(2, 16, 16, (32, 192, 64, 2, False), (64, 384, 64, 1, True), taps=(0, 1))),
])
KINK_MARGIN = 1e-5
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0)}


def out_hw(case):
    """(h, w) of every block's input, then of the chain's output."""
    h, w, dims = case.h, case.w, []
    for s in case.specs:
        dims.append((h, w))
        h, w = T.same_pad_1d(h, 3, s.stride)[0], T.same_pad_1d(w, 3, s.stride)[0]
    return dims + [(h, w)]


def make_case(case, tail_identity=False):
    """(x, blocks, tail_w) of a case as fp32 CPU tensors: drawn in fp64 from one seeded generator and rounded once.  Kernels
    N(0, 1) / sqrt(fan in), gamma = 1 + 0.2 N, beta = 0.1 N (as test_gpu_mbchain._backbone), x = N(0, 1).  Dropout seeds are
    1000 + 10 block + k for norm k.  tail_identity: the tail kernel is the identity (the stage cut's constant)."""
    g = torch.Generator().manual_seed(1000 + case.seed)

    def randn(*shape):
        return torch.randn(shape, generator=g, dtype=torch.float64)

    def norm(c, seed):
        return Norm((1 + 0.2 * randn(c)).float(), (0.1 * randn(c)).float(), 32, EPS, case.rate, seed)

    x = randn(case.n, case.h, case.w, case.specs[0].cin).float()
    blocks = []
    for i, s in enumerate(case.specs):
        w1 = (randn(1, 1, s.cin, s.wide) / np.sqrt(s.cin)).float()
        n1 = norm(s.wide, 1000 + 10 * i + 1)
        wd = (randn(3, 3, s.wide, 1) / 3.0).float()
        n2 = norm(s.wide, 1000 + 10 * i + 2)
        w3 = (randn(1, 1, s.wide, s.cout) / np.sqrt(s.wide)).float()
        n3 = norm(s.cout, 1000 + 10 * i + 3)
        blocks.append(Block(w1, n1, wd, n2, w3, n3, s.stride, s.residual))
    c = case.specs[-1].cout
    tail_w = (randn(1, 1, c, case.tail) / np.sqrt(c)).float()
    if tail_identity:
        tail_w = torch.eye(c, dtype=torch.float32).reshape(1, 1, c, c).contiguous()
    return x, blocks, tail_w


def make_cotangents(case, tail_cout):
    """N(0, 1) cotangents of every tap and of the tail output (fp32, from a generator of their own)."""
    g = torch.Generator().manual_seed(5000 + case.seed)
    dims = out_hw(case)
    cot = [torch.randn((case.n,) + dims[i + 1] + (case.specs[i].cout,), generator=g, dtype=torch.float64).float() for i in sorted(case.taps)]
    cot.append(torch.randn((case.n,) + dims[-1] + (tail_cout,), generator=g, dtype=torch.float64).float())
    return cot


def keep_masks(x_shape, blocks, counter=0):
    """Per block the three keep masks (float32 0 / 1 tensors, None where the rate is 0) of the tensors its Norms act on."""
    n, h, w, _ = x_shape
    masks = []
    for b in blocks:
        oh, ow = T.same_pad_1d(h, 3, b.stride)[0], T.same_pad_1d(w, 3, b.stride)[0]
        shapes = ((n, h, w, b.w1.shape[3]), (n, oh, ow, b.w1.shape[3]), (n, oh, ow, b.w3.shape[3]))
        masks.append(tuple(torch.from_numpy(dropout_ref.keep_mask(nm.seed + counter, s, nm.rate).astype(np.float32)) if nm.rate > 0.0 else None
                           for nm, s in zip((b.n1, b.n2, b.n3), shapes)))
        h, w = oh, ow
    return masks


def chain_ref(x, blocks, tail_w, act, dtype, masks=None, pre=None):
    """-> (list of every block's output, raw tail product), computed in `dtype`.  Tensors of another dtype are converted (a
    tensor already in `dtype` is used as it is, so a leaf stays a leaf).  masks: keep_masks(...) or None (no dropout, whatever
    rate the Norms carry).  pre: a list that receives the two pre-activations GN(a w1), GN(dw(z1)) of every block."""
    def cv(t):
        return t if t.dtype == dtype else t.to(dtype)

    def gn(y, nm):
        return T.group_norm(y, cv(nm.gamma), cv(nm.beta), nm.groups_arg, nm.eps)

    def drop(y, nm, keep):
        if keep is None:
            return y
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(nm.rate))      # the kernels' fp32 keep scale
        return y * (keep.to(dtype) * float(scale))

    a = cv(x)
    outs = []
    for i, b in enumerate(blocks):
        m = masks[i] if masks is not None else (None, None, None)
        p1 = gn(T.conv2d_same(a, cv(b.w1), 1), b.n1)
        z1 = drop(T.activation(p1, act), b.n1, m[0])
        p2 = gn(T.depthwise_conv2d_same(z1, cv(b.wd), b.stride), b.n2)
        z2 = drop(T.activation(p2, act), b.n2, m[1])
        out = drop(gn(T.conv2d_same(z2, cv(b.w3), 1), b.n3), b.n3, m[2])
        if pre is not None:
            pre += [p1, p2]
        if b.residual:
            out = out + a
        outs.append(out)
        a = out
    return outs, T.conv2d_same(a, cv(tail_w), 1)


def grad_names(nblocks, with_tail=True):
    names = ["x"] + ["b%d.%s" % (i, p) for i in range(nblocks) for p in PARAM_NAMES]
    return names + (["tail_w"] if with_tail else [])


def run_ref(case, dtype, tail_identity=False, dropout=True):
    """The case evaluated by chain_ref in `dtype`, forward and backward under make_cotangents: ({output name: array},
    {gradient name: array}).  Outputs: "tap<i>" and "tail"; gradients: grad_names().  A constant (identity) tail kernel has no
    gradient."""
    x, blocks, tail_w = make_case(case, tail_identity)
    masks = keep_masks(x.shape, blocks, case.counter) if (dropout and case.rate > 0.0) else None

    def leaf(t):
        return t.to(dtype).requires_grad_(True)

    xl = leaf(x)
    lb = [Block(leaf(b.w1), b.n1._replace(gamma=leaf(b.n1.gamma), beta=leaf(b.n1.beta)),
                leaf(b.wd), b.n2._replace(gamma=leaf(b.n2.gamma), beta=leaf(b.n2.beta)),
                leaf(b.w3), b.n3._replace(gamma=leaf(b.n3.gamma), beta=leaf(b.n3.beta)), b.stride, b.residual) for b in blocks]
    tl = tail_w.to(dtype) if tail_identity else leaf(tail_w)
    outs, tail = chain_ref(xl, lb, tl, case.act, dtype, masks)
    taps = sorted(case.taps)
    cot = make_cotangents(case, tail_w.shape[3])
    leaves = [xl] + [t for b in lb for t in (b.w1, b.n1.gamma, b.n1.beta, b.wd, b.n2.gamma, b.n2.beta, b.w3, b.n3.gamma, b.n3.beta)]
    if not tail_identity:
        leaves.append(tl)
    loss = sum((o * c.to(dtype)).sum() for o, c in zip([outs[i] for i in taps] + [tail], cot))
    grads = torch.autograd.grad(loss, leaves)
    out = {"tap%d" % i: outs[i].detach().numpy() for i in taps}
    out["tail"] = tail.detach().numpy()
    return out, {k: g.numpy() for k, g in zip(grad_names(len(blocks), not tail_identity), grads)}


@functools.lru_cache(maxsize=None)
def reference(cid, dtype, tail_identity=False, dropout=True):
    """run_ref of CASES[cid], computed once per process and shared by the tests: treat the arrays as read-only."""
    out, grads = run_ref(CASES[cid], dtype, tail_identity, dropout)
    for a in list(out.values()) + list(grads.values()):
        a.setflags(write=False)
    return out, grads


def kink_margin(case):
    """Smallest distance of any pre-activation of the case (fp64 reference) from a kink of its activation."""
    x, blocks, tail_w = make_case(case)
    pre = []
    with torch.no_grad():
        chain_ref(x, blocks, tail_w, case.act, torch.float64, keep_masks(x.shape, blocks, case.counter) if case.rate > 0.0 else None, pre=pre)
    return min(float((p - k).abs().min()) for p in pre for k in KINKS[case.act])
