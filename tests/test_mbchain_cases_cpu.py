"""The case table of tests/mbchain_ref.py without a GPU: every case is one the chain accepts, takes the planner branch it was
picked for (read off the host-only rn_mb_*_rows / *_workspace queries: the library loads without a device), and the table as
a whole covers every branch listed in COVER.  A planner change that moves a case off its branch fails here and says: pick
another shape for that branch.  Two more tests check the reference itself.

What the queries show:
  pointwise forward    (bm, bn) = (pixels per sample / rows per sample, the layout's bn): the tile of pw_cfg
  pointwise backward   ("one-pass", ceil(cin / 16), ceil(cout / 16)): mb_pw_bwd_big_kernel -- one row AND one weight-gradient
                       split per block, one N-tile of 16 ceil(cin / 16) channels; else ("tile", dpb, splits per sample) with
                       dpb = the layout's bn = the data-gradient tile of pw_bwd_cfg, splits = workspace / (4 n cin cout)
  depthwise            rows per sample = blocks per (sample, slab) of dw_plan / dw_bwd_plan
What they do not show stands in the comment beside each case, derived once by reading dw_slab / dw_plan / dw_bwd_plan /
dw_tiles_per_block (mb_common.h, mbconv.hip): forward tile th x tw and tiles per block tpb; backward tile, tpb and the loads
per thread npa / npd that pick the prefetching instantiation.  `slab` (channels per depthwise block) is derived the same way;
the test only checks that it is a legal slab (whole groups, whole quads, divides the channels)."""
import collections
import ctypes as C

import pytest
import torch

import mbchain_ref as R
from oracle import model_ref
from oracle import tf_ops_ref as T

E = collections.namedtuple("E", "fwd1 dwf fwd3 bwd3 dwb bwd1 slab")
BIG, TILE = "one-pass", "tile"
# case -> one E per block
EXPECT = {
    # dw fwd 4x4 tpb 1; bwd 4x4 tpb 1 npa 3 npd 3 (plain).  fwd1 K = 160: 4 wave groups, fwd3 K = 960: 8.  bwd1 reduces over 960: {32,8,64,2}
    1: [E((32, 32), 4, (32, 32), (TILE, 32, 1), 4, (TILE, 32, 1), 60)],
    # dw as case 1.  bwd3 reduces over 320: {32,4,64,1}, two weight-gradient splits
    2: [E((32, 32), 16, (32, 32), (TILE, 32, 2), 16, (TILE, 32, 1), 60)],
    # dw fwd 4x4 tpb 1; bwd 4x4 tpb 1 npa 2 npd 2.  hw = 192 is no multiple of 128: one split per sample
    3: [E((64, 64), 12, (32, 32), (TILE, 64, 1), 12, (TILE, 32, 1), 48)],
    # dw fwd th 4 tw 3 (the map's width); bwd 4x4 over a 3-wide map, tpb 1
    4: [E((64, 64), 16, (32, 32), (TILE, 64, 1), 16, (TILE, 32, 1), 48)],
    # stride 2, pad_l = 1: dw fwd th 4 tw 3 on the 64x3 output; bwd 4x4 on 128x5 (64 tiles), npa 2 npd 1
    5: [E((64, 64), 16, (32, 32), (TILE, 64, 1), 64, (TILE, 32, 5), 48)],
    # stride 2, pad_t = 1: dw fwd th 3 tw 4 on the 3x64 output
    6: [E((64, 64), 16, (32, 32), (TILE, 64, 1), 64, (TILE, 32, 5), 48)],
    # hw = 4224 > 4096: 128x64 tiles, 33 rows.  dw fwd and bwd th 4 tw 8 (17 tile rows, the last one half full), tpb 1, npa 3 npd 3.
    # bwd3 has 198 data-gradient blocks: {64,1,64,1}
    7: [E((128, 64), 136, (128, 64), (TILE, 64, 33), 136, (TILE, 32, 33), 36)],
    # groups 20 / 30 / 28; dw 4x4 tpb 1, npa 2 npd 2
    8: [E((64, 64), 48, (32, 32), (TILE, 64, 6), 48, (TILE, 32, 6), 40)],
    # groups 18 / 27 / 22; stride 2: dw fwd 4x4 on 8x8 (patch 9x9), bwd 4x4 npa 3 npd 2
    9: [E((64, 64), 4, (32, 32), (TILE, 64, 1), 16, (TILE, 32, 2), 72)],
    # dw fwd 8x8 tpb 2 (prefetching forward); bwd 8x8 tpb 2 npa 4 npd 4: <ELU,true,1,4,4,true>.  bwd3 (144 -> 24 below 256^2): tile
    # kernel, 256 rows = rn_mb_rows_max(), 768 data-gradient blocks
    10: [E((128, 64), 128, (128, 32), (TILE, 64, 128), 128, (BIG, 2, 9), 36)],
    # as 10 with n = 2: tpb 4; bwd3 has 1536 data-gradient blocks (> 1024: weight-gradient blocks first)
    11: [E((128, 64), 64, (128, 32), (TILE, 64, 64), 64, (BIG, 2, 9), 36)],
    # 48-channel slab: dw bwd 8x8 tpb 2 npa 5 npd 5: <ELU,true,1,5,5,true>; fwd 8x8 tpb 2
    12: [E((128, 64), 128, (128, 32), (TILE, 64, 64), 128, (BIG, 1, 6), 48)],
    # stride 2: dw fwd th 4 tw 8 tpb 1; bwd 8x8 tpb 2 npa 4 npd 2: <ELU,true,2,4,2,true>
    13: [E((128, 64), 128, (32, 32), (TILE, 64, 32), 128, (BIG, 2, 9), 36)],
    # stride 2, 48-channel slab: dw bwd 8x8 tpb 2 npa 5 npd 2: <ELU,true,2,5,2,true>
    14: [E((128, 64), 128, (64, 64), (TILE, 64, 32), 128, (BIG, 1, 6), 48)],
    # expansion 1, one slab: dw th 4 tw 8 tpb 1 (512 rows: compacted), bwd npa 2 npd 2
    15: [E((128, 32), 512, (128, 32), (BIG, 2, 1), 512, (BIG, 2, 2), 32)],
    # one 92-channel slab: dw th 4 tw 8 tpb 1; bwd npa 6 npd 6 (above every prefetching instantiation, and tpb 1): <ELU,false>
    16: [E((128, 64), 512, (128, 32), (BIG, 6, 2), 512, (BIG, 1, 6), 92)],
    # 256^2: 512 forward rows (compacted); dw 8x8 tpb 8; bwd3 is the one-pass (9,2) kernel
    17: [E((128, 64), 128, (128, 32), (BIG, 9, 2), 128, (BIG, 2, 9), 36)],
    # the shape of case 3 (the activation does not enter the planners)
    18: [E((64, 64), 12, (32, 32), (TILE, 64, 1), 12, (TILE, 32, 1), 48)],
    19: [E((64, 64), 12, (32, 32), (TILE, 64, 1), 12, (TILE, 32, 1), 48)],
    # block A stride 2 (dw fwd 4x4 on 8x8, bwd 4x4 on 16x16 npa 2 npd 1); block B 8 slabs of 48, 4x4
    20: [E((64, 64), 4, (32, 32), (TILE, 64, 1), 16, (TILE, 32, 2), 48),
         E((64, 64), 4, (32, 32), (TILE, 64, 1), 4, (TILE, 32, 1), 48)],
}
# every branch the table must reach, by the names _observe() gives them
COVER = (["fwd 64x64", "fwd 128x32", "fwd 128x64", "fwd 32x32 K<481", "fwd 32x32 K>=481",
          "bwd {64,1,64,1}", "bwd {32,4,64,1}", "bwd {32,8,64,2}", "wgrad one split", "wgrad several splits",
          "rows == max", "rows > max", "one slab", "several slabs"] +
         ["bwd one-pass (%d,%d)" % p for p in ((2, 2), (1, 6), (2, 9), (2, 1), (6, 2), (9, 2))])


def _lib():
    import _rn
    return _rn, _rn.lib()


def _layout(query, *args):
    _rn, _ = _lib()
    lay = _rn.MbRows()
    assert query(*args, C.byref(lay)), "no layout for %s" % (args,)
    return lay


def _fwd(n, hw, cin, cout, groups):
    _, L = _lib()
    lay = _layout(L.rn_mb_pointwise_rows, n, hw, cin, cout, groups)
    return (hw // lay.rows_per_sample, lay.bn), lay.rows_per_sample


def _bwd(n, hw, cin, cout, groups):
    _, L = _lib()
    lay = _layout(L.rn_mb_pointwise_bwd_rows, n, hw, cin, cout, groups)
    ws = L.rn_mb_pointwise_bwd_workspace(n, hw, cin, cout)
    assert ws and ws % (4 * n * cin * cout) == 0
    splits = ws // (4 * n * cin * cout)
    nti = -(-cin // 16)
    if lay.bn == 16 * nti and splits == lay.rows_per_sample:
        return (BIG, nti, -(-cout // 16)), lay.rows_per_sample
    assert lay.bn in (32, 64) and lay.rows_per_sample == hw // lay.bn
    return (TILE, lay.bn, splits), lay.rows_per_sample


def _observe(cid):
    """-> (one E per block as the queries see it, names of the branches the case takes)"""
    import ops
    _, L = _lib()
    case = R.CASES[cid]
    seen, names = [], set()
    rmax = L.rn_mb_rows_max()
    for spec, (h, w), (oh, ow), want in zip(case.specs, R.out_hw(case), R.out_hw(case)[1:], EXPECT[cid]):
        n = case.n
        g0, g1, g3 = ops.gn_groups(spec.cin, 32), ops.gn_groups(spec.wide, 32), ops.gn_groups(spec.cout, 32)
        fwd1, r1 = _fwd(n, h * w, spec.cin, spec.wide, g1)
        fwd3, r3 = _fwd(n, oh * ow, spec.wide, spec.cout, g3)
        dwf = _layout(L.rn_mb_depthwise_rows, n, h, w, spec.wide, spec.stride, g1).rows_per_sample
        dwb = _layout(L.rn_mb_depthwise_bwd_rows, n, h, w, spec.wide, spec.stride, g1).rows_per_sample
        bwd3, q3 = _bwd(n, oh * ow, spec.wide, spec.cout, g1)
        bwd1, q1 = _bwd(n, h * w, spec.cin, spec.wide, g0)
        # the slab is not visible to the queries: only that the stated one is legal
        cpg = spec.wide // g1
        assert spec.wide % want.slab == 0 and want.slab % cpg == 0 and want.slab % 4 == 0 and want.slab <= 128
        seen.append(E(fwd1, dwf, fwd3, bwd3, dwb, bwd1, want.slab))
        for (bm, bn), k in ((fwd1, spec.cin), (fwd3, spec.wide)):
            names.add("fwd %dx%d" % (bm, bn) + ((" K<481" if k < 481 else " K>=481") if bm == 32 else ""))
        for b, reduce_over in ((bwd3, spec.cout), (bwd1, spec.wide)):
            if b[0] == BIG:
                names.add("bwd one-pass (%d,%d)" % b[1:])
            else:
                # pw_bwd_cfg: 64-pixel tiles are {64,1,64,1}; 32-pixel tiles split K in 8 from 16 K-tiles (481 channels) on, else in 4
                names.add("bwd {64,1,64,1}" if b[1] == 64 else ("bwd {32,8,64,2}" if reduce_over >= 481 else "bwd {32,4,64,1}"))
                names.add("wgrad one split" if b[2] == 1 else "wgrad several splits")
        for r in (r1, r3, dwf, dwb, q3, q1):
            if r >= rmax:
                names.add("rows == max" if r == rmax else "rows > max")
        names.add("one slab" if want.slab == spec.wide else "several slabs")
    return seen, names


def _blocks(case):
    return R.make_case(case)[1]


@pytest.mark.parametrize("cid", list(R.CASES))
def test_case_is_supported_and_takes_its_branch(cid):
    import ops_mb
    case = R.CASES[cid]
    assert ops_mb.chain_supported((case.n, case.h, case.w, case.specs[0].cin), _blocks(case))
    seen, _ = _observe(cid)
    assert seen == EXPECT[cid], "case %d left its branch: the planners now give %s -- pick another shape for %s" % (cid, seen, EXPECT[cid])


def test_table_covers_every_branch():
    assert sorted(EXPECT) == sorted(R.CASES)
    names = set()
    for cid in R.CASES:
        names |= _observe(cid)[1]
    missing = [b for b in COVER if b not in names]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


def test_table_shapes():
    """What the planners do not decide but the cases were picked for: the odd-side stride-2 paddings, the group counts."""
    import ops
    assert T.same_pad_1d(5, 3, 2) == (3, 1, 1) and T.same_pad_1d(128, 3, 2) == (64, 0, 1)      # (pad before the data only on the odd side)
    assert [R.out_hw(R.CASES[c])[-1] for c in (5, 6)] == [(64, 3), (3, 64)]
    assert [tuple(ops.gn_groups(c, 32) for c in R.CASES[k].specs[0][:3]) for k in (8, 9, 16)] == [(20, 30, 28), (18, 27, 22), (12, 23, 20)]
    for case in R.CASES.values():
        assert all(h * w % 64 == 0 for h, w in R.out_hw(case))


@pytest.mark.parametrize("name,before", [("bottleneck_3_2", "bottleneck_3_1"), ("bottleneck_4_1", "bottleneck_3_3")])
def test_chain_ref_is_the_oracles_bottleneck_bit_for_bit(name, before, monkeypatch):
    """chain_ref in fp32 with production parameters == the slice of oracle.model_ref.mobilenet_v2_forward that runs `name`
    (3_2: stride 1 with its residual; 4_1: stride 2), and its raw tail product, normalised, == the block behind the slice."""
    names = [b[0] for b in model_ref.MOBILENET_V2_BLOCKS]
    upto = names.index(name) + 1
    params = model_ref.init_params("mobilenet_v2", num_classes=3, seed=4)
    g = torch.Generator().manual_seed(5)
    for k in params:
        if k.endswith(".gamma"):
            params[k] = 1 + 0.2 * torch.randn(params[k].shape, generator=g)
        elif k.endswith(".beta"):
            params[k] = 0.1 * torch.randn(params[k].shape, generator=g)
    cout = model_ref.MOBILENET_V2_BLOCKS[upto - 1][1]
    params["backbone.output_conv.conv.weight"] = torch.randn((1, 1, cout, 32), generator=g) / cout ** 0.5     # (the backbone cut behind `name`)
    monkeypatch.setattr(model_ref, "MOBILENET_V2_BLOCKS", model_ref.MOBILENET_V2_BLOCKS[:upto])
    monkeypatch.setattr(model_ref, "MOBILENET_V2_TAPS", {before: "in", name: "out"})
    image = torch.randn((2, 64, 48, 3), generator=g)
    with torch.no_grad():
        want = model_ref.mobilenet_v2_forward(params, image)
        p = "backbone.%s." % name

        def norm(part):
            return R.Norm(params[p + part + ".norm.gamma"], params[p + part + ".norm.beta"], 32, R.EPS, 0.0, 0)

        stride = model_ref.MOBILENET_V2_BLOCKS[upto - 1][3]
        block = R.Block(params[p + "expand_conv.conv.weight"], norm("expand_conv"), params[p + "depthwise_conv.conv.weight"], norm("depthwise_conv"),
                        params[p + "linear_conv.conv.weight"], norm("linear_conv"), stride, stride == 1 and want["in"].shape[3] == cout)
        outs, tail = R.chain_ref(want["in"], [block], params["backbone.output_conv.conv.weight"], "elu", torch.float32)
        assert block.residual == (name == "bottleneck_3_2")
        assert torch.equal(outs[0], want["out"])
        c5 = T.activation(T.group_norm(tail, params["backbone.output_conv.norm.gamma"], params["backbone.output_conv.norm.beta"]), "elu")
        assert torch.equal(c5, want["C5"])


@pytest.mark.parametrize("cid", [18, 19])
def test_no_preactivation_sits_on_a_kink(cid):
    """relu / relu6: the derivative jumps at 0 (and 6), so an element within rounding of a kink may differ by O(1) between two
    correct evaluations.  The case's seed is chosen so that, in the fp64 reference, none is within KINK_MARGIN; the measured
    margins (case 18 seed 2: 1.92e-5, case 19 seed 22: 2.30e-5) are pinned so that a change of the generator is noticed."""
    margin = R.kink_margin(R.CASES[cid])
    assert margin > R.KINK_MARGIN, margin
    assert abs(margin - {18: 1.923e-5, 19: 2.296e-5}[cid]) < 2e-8, margin
