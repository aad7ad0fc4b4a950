"""fp16 inference of the MobileNetV2 backbone (mobilenet_v2.Bottleneck._call_f16_folded, MobileNetV2._call_f16, the
RN_F16_MB_BACKBONE switch) and train.evaluate(dtype='f16').

Bottleneck: folded (GroupNorms applied on the next conv's operand load, csrc/depthwise_f16.hip in the middle) against layer by
layer (ops_f16.FOLD = False) at assert_close 2e-3, the bar of test_resnext_bottleneck_fp16_folded_equals_layer_by_layer for the same
comparison: the same fp32 arithmetic on the same fp16 values.

Whole net, relative L2 per output against the product's own fp32 forward.  The bar is not chosen: the yardstick is the fp16-STORAGE
MODEL (tests/mb_f16_ref.py: oracle.model_ref in fp64, plain, against the same with every stored backbone activation rounded to
fp16), computed on the CPU for this net and this image:

    C3 9.443e-04   C4 1.510e-03   C5 2.073e-03   P3 1.632e-03   P4 2.023e-03   P5 2.383e-03   (P6 2.349e-03   P7 2.580e-03)

The product may reach 4 x the model's figure -- it rounds the raw conv output as well as the normalised activation, two sites
where the model has one -- and a further 2 x for its differently formed statistics (of the fp16-stored conv output, not of the
exact one): BAR = 8 x MODEL.  P6 / P7 (2 x 2 and 1 x 1 maps: GroupNorm over a handful of values) get the ResNeXt test's separate 1e-1.
Measured on the MI355X (profiles/mb_f16_err.txt): see MEASURED below."""
import numpy as np
import pytest
import torch

import mb_f16_ref as M
from helpers import assert_close

pytestmark = pytest.mark.gpu

MODEL = {"C3": 9.443e-04, "C4": 1.510e-03, "C5": 2.073e-03, "P3": 1.632e-03, "P4": 2.023e-03, "P5": 2.383e-03}
BAR = {k: 8.0 * v for k, v in MODEL.items()}
SMALL_MAP_BAR = 1e-1        # P6, P7
# MEASURED on the MI355X (relative L2 against the product's fp32 forward; RN_F16_MB_BACKBONE = 1 | 0; profiles/mb_f16_err.txt):
#   C3 1.567e-03 | 2.082e-04   C4 2.543e-03 | 2.085e-04   C5 3.555e-03 | 2.028e-04
#   P3 4.047e-03 | 3.012e-03   P4 4.628e-03 | 3.031e-03   P5 5.117e-03 | 3.076e-03   P6 5.369e-03 | 3.426e-03   P7 6.027e-03 | 4.275e-03
# i.e. the fp16 backbone stands at 1.7 x (C3 - C5) and 2.1 - 2.5 x (P3 - P5) the model's figure, against the 8 x granted.


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


@pytest.mark.parametrize("h,w,cin,filters,stride,t", [(32, 32, 32, 16, 1, 1), (32, 32, 24, 32, 2, 6), (16, 16, 64, 64, 1, 6), (16, 16, 160, 320, 1, 6),
                                                      (19, 25, 32, 32, 1, 6)])
def test_bottleneck_fp16_folded_equals_layer_by_layer(dev, h, w, cin, filters, stride, t):
    """(19 x 25: 475 pixels per sample are no whole number of m-tiles -- the 1 x 1 convs cannot fold and take conv + three-kernel
    GroupNorm; the depthwise conv folds at every shape)"""
    import layers, mobilenet_v2, ops_f16
    torch.manual_seed(11)
    blk = mobilenet_v2.Bottleneck(filters, strides=stride, expansion_factor=t, activation=layers.elu, dropout_rate=0.0,
                                  kernel_initializer=layers.VarianceScaling(factor=2.0), kernel_regularizer=None, in_channels=cin)
    g = _perturb(blk, 12)
    blk.to(dev)
    x = torch.randn(2, h, w, cin, generator=g).to(dev)
    xh = ops_f16.to_half(x)
    can_fold = (h, w) != (19, 25)
    with torch.no_grad():
        ref32 = blk(x, training=False)
        layers.set_inference_dtype('f16')
        try:
            assert ops_f16.FOLD
            conv1, norm1 = blk.expand_conv.layers[0], blk.expand_conv.layers[1]
            assert (ops_f16.conv2d_norm(xh, conv1.weight, norm1, 'elu') is not None) == can_fold
            folded = blk._call_f16_folded(xh)
            via_call = blk(xh, training=False)
            ops_f16.FOLD = False
            plain = blk(xh, training=False)
        finally:
            ops_f16.FOLD = True
            layers.set_inference_dtype('f32')
    assert folded.dtype == torch.float16 and folded.shape == plain.shape == ref32.shape
    assert torch.equal(folded, via_call)
    assert_close(folded.float().cpu().numpy(), plain.float().cpu().numpy(), 2e-3, "folded vs layer-by-layer fp16 bottleneck")
    err = float((folded.float() - ref32).norm() / ref32.norm())
    assert err < 1e-2, "folded fp16 bottleneck vs fp32: rel L2 %.3e" % err


def test_pending_travels_between_blocks_without_a_residual(dev):
    """keep_pending: a block without a residual hands its Pending to the next block; materialising in between gives the same bits"""
    import layers, mobilenet_v2, ops_f16
    torch.manual_seed(3)
    mk = lambda cin, f, s: mobilenet_v2.Bottleneck(f, strides=s, expansion_factor=6, activation=layers.elu, dropout_rate=0.0,
                                                   kernel_initializer=layers.VarianceScaling(factor=2.0), kernel_regularizer=None, in_channels=cin)
    a, b = mk(16, 24, 2), mk(24, 32, 2)
    _perturb(a, 1), _perturb(b, 2)
    a.to(dev), b.to(dev)
    xh = ops_f16.to_half(torch.randn(2, 64, 64, 16).to(dev))
    with torch.no_grad():
        p = a._call_f16_folded(xh, keep_pending=True)
        assert isinstance(p, ops_f16.Pending)
        assert torch.equal(b._call_f16_folded(p), b._call_f16_folded(p.materialise()))
        assert torch.equal(p.materialise(), a._call_f16_folded(xh))


@pytest.mark.parametrize("switch", [1, 0])
def test_mobilenet_fpn_fp16_inference_matches_fp32(dev, monkeypatch, switch):
    import layers, mobilenet_v2
    monkeypatch.setattr(mobilenet_v2, "F16_BACKBONE", bool(switch))
    net = M.build_net().to(dev)
    x = M.image().to(dev)
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
    for k in ("C3", "C4", "C5"):
        assert feats16[k].dtype == torch.float16 and feats16[k].shape == feats32[k].shape and feats32[k].dtype == torch.float32
    for k in M.LEVELS:
        for head in ("classifications", "regressions"):
            assert out16[head][k].dtype == torch.float16 and out16[head][k].shape == ref32[head][k].shape
            assert out16_f32[head][k].dtype == torch.float32 and out16_f32[head][k].shape == ref32[head][k].shape
            assert torch.equal(again32[head][k], ref32[head][k])          # the fp32 path is what it was
    err = M.output_errors(feats16, out16, feats32, ref32)
    for k, e in err.items():
        print("MB_F16_ERR switch %d %-3s rel L2 %.3e  model %s  bar %.3e" % (
            switch, k, e, ("%.3e" % MODEL[k]) if k in MODEL else "    -    ", BAR.get(k, SMALL_MAP_BAR)))
    bad = {k: e for k, e in err.items() if not e <= BAR.get(k, SMALL_MAP_BAR)}
    assert not bad, "relative L2 above the bar: %s" % bad


@pytest.mark.parametrize("switch", [1, 0])
def test_evaluate_fp16(dev, monkeypatch, switch):
    """(128 x 128: the maps from 8 x 8 down are no whole number of m-tiles -- with the fp16 backbone their 1 x 1 convs take the layer-by-layer
    fallback inside the folded path)"""
    import layers, levels as levels_mod, mobilenet_v2, retinanet, train
    monkeypatch.setattr(mobilenet_v2, "F16_BACKBONE", bool(switch))
    from data_loaders.shapes import Shapes
    lv = levels_mod.build_levels()
    torch.manual_seed(1)
    net = retinanet.RetinaNet('mobilenet_v2', lv, 3, layers.elu, 0.0).to(dev)
    res32 = train.evaluate(net, Shapes(None, image_size=(128, 128), seed=12345), lv, 4, scale=128, device=dev)
    res16 = train.evaluate(net, Shapes(None, image_size=(128, 128), seed=12345), lv, 4, scale=128, device=dev, dtype='f16')
    assert not layers.INFERENCE_F16 and not layers.F16_OUTPUTS_F32
    assert set(res16) == set(res32) and res16['images'] == res32['images'] == 4
    assert all(np.isfinite(float(res16[k])) for k in ('mAP', 'class_iou', 'regr_iou'))

    def broken(image, training):
        assert layers.INFERENCE_F16
        raise RuntimeError("forward failed")

    with pytest.raises(RuntimeError, match="forward failed"):
        train.evaluate(broken, Shapes(None, image_size=(128, 128), seed=12345), lv, 4, scale=128, device=dev, dtype='f16')
    assert not layers.INFERENCE_F16 and not layers.F16_OUTPUTS_F32
