"""fp16 inference of the DenseNet backbones: the dense block on one fp16 buffer (densenet.DenseNet_Block._call_f16,
ops_f16.dense_block, the RN_F16_DENSE_BLOCK switch), the pool-first transition (densenet.TransitionLayer._call_f16), the whole
DenseNet-121-FPN net, DenseNet-169, and train.evaluate(dtype='f16').

Block: the one-buffer path against the concat path (ops_f16.DENSE_BLOCK = False) at assert_close 2e-3 -- the bar of
tests/test_gpu_mb_f16.py for "the same fp32 arithmetic on the same fp16 values" --, relative L2 against the block's own fp32
forward below 1e-2 (the same precedent), and a forward captured with torch.cuda.graph equal to the eager one bit for bit.

Whole net, relative L2 per output against the product's own fp32 forward.  The bar is not chosen: the yardstick is the fp16-STORAGE
MODEL (tests/dense_f16_ref.py: oracle.backbones_ref + model_ref in fp64, plain, against the same with the backbone's dropout hook
rounding every hooked activation -- the output of every 1 x 1, 3 x 3 and transition conv -- to fp16), computed on the CPU for this
net and this image (`python tests/dense_f16_ref.py`):

    C3 4.582e-04   C4 5.908e-04   C5 5.420e-04   P3 6.442e-04   P4 7.337e-04   P5 7.354e-04   (P6 7.013e-04   P7 7.599e-04)

BAR = 8 x MODEL, the reasoning of tests/test_gpu_mb_f16.py: 4 x for two stored sites where the model has one (the product rounds the
normalised operand as well as the raw conv output), 2 x for statistics formed from the stored values.  P6 / P7 (2 x 2 and 1 x 1
maps) keep that file's separate 1e-1.  Measured on the MI355X: see MEASURED below and profiles/dense_f16_err.txt."""
import numpy as np
import pytest
import torch

import dense_f16_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu

MODEL = {"C3": 4.582e-04, "C4": 5.908e-04, "C5": 5.420e-04, "P3": 6.442e-04, "P4": 7.337e-04, "P5": 7.354e-04}
BAR = {k: 8.0 * v for k, v in MODEL.items()}
SMALL_MAP_BAR = 1e-1        # P6, P7
# MEASURED on the MI355X (relative L2 against the product's fp32 forward; RN_F16_DENSE_BLOCK = 1 | 0; profiles/dense_f16_err.txt):
#   C3 1.313e-03 | 1.315e-03   C4 1.516e-03 | 1.514e-03   C5 1.371e-03 | 1.364e-03
#   P3 3.437e-03 | 3.442e-03   P4 3.468e-03 | 3.481e-03   P5 3.546e-03 | 3.534e-03   P6 3.649e-03 | 3.670e-03   P7 4.806e-03 | 4.776e-03
# i.e. 2.5 - 2.9 x the model's figure on C3 - C5 and 4.7 - 5.3 x on P3 - P5, against the 8 x granted; both block paths alike.


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _perturb(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("gamma"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("beta"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return g


@pytest.mark.parametrize("name", R.BLOCK_TABLES)
def test_block_one_buffer_equals_concat_path(dev, monkeypatch, name):
    import densenet, layers, ops_f16
    t = R.TABLES[name]
    torch.manual_seed(21)
    blk = densenet.DenseNet_Block(R.GROWTH, depth=t.depth, bottleneck=True, activation=layers.elu, dropout_rate=0.0,
                                  kernel_initializer=layers.VarianceScaling(factor=2.0), kernel_regularizer=None, in_channels=t.c_in)
    g = _perturb(blk, 22)
    blk.to(dev)
    x = torch.randn(t.n, t.h, t.w, t.c_in, generator=g).to(dev)
    xh = ops_f16.to_half(x)
    can_fold = name in ("t16x16", "t8x8")          # 475 and 35 pixels per sample are no whole number of m-tiles: conv2d + group_norm_act
    with torch.no_grad():
        ref32 = blk(x, training=False)
        layers.set_inference_dtype('f16')
        try:
            assert ops_f16.DENSE_BLOCK and ops_f16.FOLD
            f0 = blk.composite_functions[0].layers
            assert (ops_f16.conv2d_norm(xh, f0[2].weight, f0[4], 'elu') is not None) == can_fold
            d = blk._call_f16(xh)
            assert isinstance(d, ops_f16.DenseBuffer) and d.filled == d.ld == R.table_ld(t)
            one = blk(xh, training=False)
            assert torch.equal(one, d.buf)
            assert torch.equal(blk(x, training=False), one)              # an fp32 input is cast first
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                captured = blk(xh, training=False)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, one), "graph replay != eager"
            monkeypatch.setattr(ops_f16, "DENSE_BLOCK", False)
            assert blk._call_f16(xh) is None
            concat = blk(xh, training=False)
        finally:
            layers.set_inference_dtype('f32')
        again32 = blk(x, training=False)
    assert torch.equal(again32, ref32)
    assert one.dtype == concat.dtype == torch.float16 and one.shape == concat.shape == ref32.shape
    assert torch.equal(one[..., :t.c_in], xh)                            # the block's input is the buffer's first slice
    e = assert_close(one.float().cpu().numpy(), concat.float().cpu().numpy(), 2e-3, "one-buffer vs concat fp16 block " + name)
    err = float((one.float() - ref32).norm() / ref32.norm())
    err0 = float((concat.float() - ref32).norm() / ref32.norm())
    print("DENSE_F16_BLOCK %-7s one-buffer vs concat max-norm %.3e; rel L2 vs fp32: one-buffer %.3e  concat %.3e" % (name, e, err, err0))
    assert err < 1e-2, "one-buffer fp16 block vs fp32: rel L2 %.3e" % err


@pytest.mark.parametrize("shape", [(2, 16, 16, 256), (2, 19, 25, 128)])
def test_transition_pool_first(dev, shape):
    import densenet, layers, ops_f16
    n, h, w, c = shape
    torch.manual_seed(31)
    tr = densenet.TransitionLayer(input_filters=c, compression_factor=0.5, dropout_rate=0.0,
                                  kernel_initializer=layers.VarianceScaling(factor=2.0), kernel_regularizer=None)
    g = _perturb(tr, 32)
    tr.to(dev)
    x = (1.5 * torch.randn(n, h, w, c, generator=g) + 0.3).to(dev)
    xh = ops_f16.to_half(x)
    with torch.no_grad():
        ref32 = tr(x, training=False)
        layers.set_inference_dtype('f16')
        try:
            got = tr(xh, training=False)
            direct = tr._call_f16(xh)
            d = ops_f16.DenseBuffer(n, h, w, c, dev)
            d.put(xh)
            from_buffer = tr._call_f16(d)
        finally:
            layers.set_inference_dtype('f32')
    assert direct is not None and torch.equal(got, direct) and torch.equal(got, from_buffer)
    assert got.dtype == torch.float16 and got.shape == ref32.shape == (n, -(-h // 2), -(-w // 2), c // 2)
    err = float((got.float() - ref32).norm() / ref32.norm())
    print("DENSE_F16_TRANSITION %s rel L2 vs fp32 %.3e" % (shape, err))
    assert err < 1e-2


@pytest.mark.parametrize("switch", [1, 0])
def test_densenet_fpn_fp16_inference_matches_fp32(dev, monkeypatch, switch):
    import layers, ops_f16
    monkeypatch.setattr(ops_f16, "DENSE_BLOCK", bool(switch))
    taken, real = [], ops_f16.dense_block
    monkeypatch.setattr(ops_f16, "dense_block", lambda *a, **k: (taken.append(real(*a, **k)), taken[-1])[1])
    net = R.build_net().to(dev)
    x = R.image().to(dev)
    with torch.no_grad():
        ref32 = net(x, training=False)
        feats32 = net.base.backbone(x, training=False)
        layers.set_inference_dtype('f16')
        try:
            out16 = net(x, training=False)
            feats16 = net.base.backbone(x, training=False)
            layers.set_inference_dtype('f16', outputs='f32')
            out16_f32 = net(x, training=False)
        finally:
            layers.set_inference_dtype('f32')
        again32 = net(x, training=False)
    assert not layers.INFERENCE_F16
    # switch 1: each of the three fp16 forwards ran its four blocks on one buffer (no silent fall-back); switch 0: none did
    assert len(taken) == (12 if switch else 0) and all(isinstance(d, ops_f16.DenseBuffer) for d in taken)
    del taken[:]
    for k in ("C3", "C4", "C5"):
        assert feats16[k].dtype == torch.float16 and feats16[k].shape == feats32[k].shape and feats32[k].dtype == torch.float32
    for k in R.LEVELS:
        for head in ("classifications", "regressions"):
            assert out16[head][k].dtype == torch.float16 and out16[head][k].shape == ref32[head][k].shape
            assert out16_f32[head][k].dtype == torch.float32 and out16_f32[head][k].shape == ref32[head][k].shape
            assert torch.equal(again32[head][k], ref32[head][k])          # the fp32 path is what it was
    err = R.output_errors(feats16, out16, feats32, ref32)
    for k, e in err.items():
        print("DENSE_F16_ERR switch %d %-3s rel L2 %.3e  model %s  bar %.3e" % (
            switch, k, e, ("%.3e" % MODEL[k]) if k in MODEL else "    -    ", BAR.get(k, SMALL_MAP_BAR)))
    bad = {k: e for k, e in err.items() if not e <= BAR.get(k, SMALL_MAP_BAR)}
    assert not bad, "relative L2 above the bar: %s" % bad


def test_densenet_169_fp16_runs(dev):
    """64 x 64: block 4 grows to 1664 channels on a 2 x 2 map (prefixes up to 1632, group sizes up to 51)"""
    import layers
    net = R.build_net('densenet_169').to(dev)
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    with torch.no_grad():
        ref32 = net(x, training=False)
        feats32 = net.base.backbone(x, training=False)
        layers.set_inference_dtype('f16')
        try:
            out16 = net(x, training=False)
            feats16 = net.base.backbone(x, training=False)
        finally:
            layers.set_inference_dtype('f32')
    assert feats32["C5"].shape == (2, 2, 2, 1664)
    for k in ("C3", "C4", "C5"):
        assert feats16[k].dtype == torch.float16 and feats16[k].shape == feats32[k].shape and bool(torch.isfinite(feats16[k].float()).all())
    for k in R.LEVELS:
        for head in ("classifications", "regressions"):
            assert out16[head][k].shape == ref32[head][k].shape and bool(torch.isfinite(out16[head][k].float()).all())


def test_evaluate_fp16_densenet(dev):
    import layers, levels as levels_mod, retinanet, train
    from data_loaders.shapes import Shapes
    lv = levels_mod.build_levels()
    torch.manual_seed(1)
    net = retinanet.RetinaNet('densenet_121', lv, 3, layers.elu, 0.0).to(dev)
    res16 = train.evaluate(net, Shapes(None, image_size=(128, 128), seed=12345), lv, 4, scale=128, device=dev, dtype='f16')
    assert not layers.INFERENCE_F16 and not layers.F16_OUTPUTS_F32
    assert res16['images'] == 4
    assert all(np.isfinite(float(res16[k])) for k in ('mAP', 'class_iou', 'regr_iou'))

    def broken(image, training):
        assert layers.INFERENCE_F16
        raise RuntimeError("forward failed")

    with pytest.raises(RuntimeError, match="forward failed"):
        train.evaluate(broken, Shapes(None, image_size=(128, 128), seed=12345), lv, 4, scale=128, device=dev, dtype='f16')
    assert not layers.INFERENCE_F16 and not layers.F16_OUTPUTS_F32
