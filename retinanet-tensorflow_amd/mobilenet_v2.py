"""MobileNetV2 bottom-up network (drop-in for reference mobilenet_v2.py:15-223), GroupNorm
variant, NHWC fp32 on gfx950 kernels.

    net = MobileNetV2(activation=layers.elu, dropout_rate=0.2)
    feats = net(image, training=True)      # {'C1'..'C5'}, strides 2..32

Block table (filters, expansion, stride) and the taps follow mobilenet_v2.py:120-223:
stem 3x3/2 -> 32; 17 inverted-residual bottlenecks (expand 1x1 -> depthwise 3x3 -> linear 1x1,
each + GroupNorm, dropout; residual iff shapes match, :91-92); final 1x1 -> 32 channels (:178-185,
SURVEY Q8).  Each [conv, Normalization, activation, Dropout] run is conv kernel + ONE fused
GroupNorm kernel (the residual add rides in the same kernel).
"""
import os

import torch

import layers as L
import ops
import ops_mb
from model import Model, Sequential
from normalization import Normalization

# stage -> (filters, expansion, [strides of its blocks])
_STAGES = (
    (1, 16, 1, (1,)),
    (2, 24, 6, (2, 1)),
    (3, 32, 6, (2, 1, 1)),
    (4, 64, 6, (2, 1, 1, 1)),
    (5, 96, 6, (1, 1, 1)),
    (6, 160, 6, (2, 1, 1)),
    (7, 320, 6, (1,)),
)
_TAP_AFTER = {'bottleneck_1_1': 'C1', 'bottleneck_2_2': 'C2', 'bottleneck_3_3': 'C3', 'bottleneck_5_3': 'C4'}

# The bottlenecks as ONE autograd node over the rn_mb_* kernels (ops_mb.mb_chain): every GroupNorm applied by its consumer,
# 3 launches per bottleneck forward and 3 backward instead of 6 + 7.  It starts at the first bottleneck from which on every
# layer's shape qualifies (maps whose statistic rows a consumer block can merge: <= 128 x 128 at the headline size); the
# bottlenecks in front of it run layer by layer.  RN_MB_CHAIN=0: layer by layer everywhere.
MB_CHAIN = os.environ.get("RN_MB_CHAIN", "1") == "1"
# Maps of more than this many pixels per sample stay on the layer-by-layer path; 0 = no limit (the default since the
# depthwise kernels walk several tiles per block on big maps: 427 vs 423 images/s with the 256 x 256 maps in the chain; their
# statistic rows go through rn_mb_compact_rows first).  RN_MB_CHAIN_MAX_HW=16384: the round-3 first version (chain from
# bottleneck_2_2 on).
MB_CHAIN_MAX_HW = int(os.environ.get("RN_MB_CHAIN_MAX_HW", 0))
STAGE_CUT_AFTER = 'bottleneck_3_3'      # (the C3 tap: everything above it is 95 % of the backbone's gradient bytes and runs on maps <= 32 x 32)
# fp16 inference (layers.set_inference_dtype('f16')).  1: the backbone itself runs in fp16 -- every bottleneck's GroupNorms folded
# into the convs around them (Bottleneck._call_f16_folded; csrc/depthwise_f16.hip is the depthwise conv).  0 (the default: measured
# faster, 1069 - 1076 vs 955 - 956 images/s at 1024 x 1024 batch 16, profiles/mb_f16_inference.txt): the backbone runs in fp32
# through the fused chain above and only C3, C4, C5 are cast to fp16 for the FPN and the heads.
F16_BACKBONE = os.environ.get("RN_F16_MB_BACKBONE", "0") == "1"


def _f16_conv_norm(x, conv, norm, act, residual=None):
    """1 x 1 / stem conv -> GroupNorm -> act on the fp16 path.  x: fp16 tensor or ops_f16.Pending.  A Pending where the conv can
    fold (ops_f16.conv2d_norm); else the finished fp16 tensor from conv + three-kernel GroupNorm, `residual` added."""
    import ops_f16
    p = ops_f16.conv2d_norm(x, conv.weight, norm, act, conv.strides, conv.groups) if ops_f16.FOLD else None
    if p is not None:
        return p
    t = x.materialise() if isinstance(x, ops_f16.Pending) else x
    return ops_f16.group_norm_act(ops_f16.conv2d(t, conv.weight, None, conv.strides, conv.groups), norm.gamma, norm.beta, norm.groups,
                                  norm.eps, act, residual)


class DepthwiseConv2D(L.DepthwiseConv2D):
    pass


class Bottleneck(Model):
    def __init__(self, filters, strides, expansion_factor, activation, dropout_rate, kernel_initializer,
                 kernel_regularizer, name='bottleneck', in_channels=None):
        super().__init__(name=name)
        self._cfg = (filters, strides, expansion_factor, L.get_activation(activation), dropout_rate,
                     kernel_initializer, kernel_regularizer)
        self.expand_conv = self.depthwise_conv = self.linear_conv = None
        if in_channels is not None:
            self.build(in_channels)

    def build(self, in_channels):
        filters, strides, t, act, rate, init, reg = self._cfg
        wide = in_channels * t

        def pointwise(cout, cin):
            return L.Conv2D(cout, 1, use_bias=False, kernel_initializer=init, kernel_regularizer=reg, in_channels=cin)

        self.expand_conv = Sequential([pointwise(wide, in_channels), Normalization(channels=wide), act, L.Dropout(rate)])
        self.depthwise_conv = Sequential([
            DepthwiseConv2D(3, strides=strides, padding='same', use_bias=False, kernel_initializer=init,
                            kernel_regularizer=reg, in_channels=wide),
            Normalization(channels=wide), act, L.Dropout(rate)])
        self.linear_conv = Sequential([pointwise(filters, wide), Normalization(channels=filters), L.Dropout(rate)])
        self._same_shape = (strides == 1 and filters == in_channels)

    def call(self, input, training):
        if self.expand_conv is None:
            self.build(input.shape[3])
            self.to(input.device)
        identity = None
        if input.dtype == torch.float16 and not training:
            import ops_f16
            if ops_f16.FOLD:
                return self._call_f16_folded(input)
        if self._same_shape and input.dtype == torch.float16:       # fp16 inference, layer by layer: no gradients to sum
            identity = input
        elif self._same_shape:      # the input feeds the expand conv and the residual: their gradients are summed by our kernel
            input, identity = ops.fanout(input, 2)
        mid = self.depthwise_conv(self.expand_conv(input, training), training)
        return self.linear_conv(mid, training, residual=identity)

    def _call_f16_folded(self, input, keep_pending=False):
        """fp16 inference with the block's three GroupNorms folded into its convs (the pattern of
        resnet.ResNeXt_Bottleneck._call_f16_folded): the expand conv's epilogue emits the statistics of its output, the depthwise
        conv applies that GroupNorm + activation on its operand load and emits its own statistics (ops_f16.depthwise_norm), the
        linear conv does the same.  `input`: an fp16 tensor, or the Pending output of the block in front (a block without a
        residual).  The block's output is materialised once -- with the residual in the same pass -- unless `keep_pending` and
        there is no residual: then the Pending goes to the next block's expand conv.  A 1 x 1 conv whose map is not a whole number
        of m-tiles runs conv + GroupNorm layer by layer (_f16_conv_norm); the depthwise conv folds at every shape."""
        import ops_f16
        conv1, norm1, act1, _ = self.expand_conv.layers
        dw, norm2, act2, _ = self.depthwise_conv.layers
        conv3, norm3, _ = self.linear_conv.layers
        if self._same_shape and isinstance(input, ops_f16.Pending):
            input = input.materialise()                 # read twice: by the expand conv and as the residual
        identity = input if self._same_shape else None
        a1 = _f16_conv_norm(input, conv1, norm1, L.activation_name(act1))
        p2 = ops_f16.depthwise_norm(a1, dw.weight, norm2, L.activation_name(act2), dw.strides)
        a3 = _f16_conv_norm(p2, conv3, norm3, None, residual=identity)
        if isinstance(a3, ops_f16.Pending) and not (keep_pending and identity is None):
            return a3.materialise(residual=identity)
        return a3


class MobileNetV2(Model):
    def __init__(self, activation, dropout_rate, name='mobilenet_v2'):
        super().__init__(name=name)
        act = L.relu6 if activation is None else L.get_activation(activation)
        init = L.VarianceScaling(factor=2.0)
        reg = L.L2Regularizer(scale=4e-5)

        def conv_block(cout, k, stride, cin):
            return Sequential([
                L.Conv2D(cout, k, strides=stride, padding='same', use_bias=False, kernel_initializer=init,
                         kernel_regularizer=reg, in_channels=cin),
                Normalization(channels=cout), act, L.Dropout(dropout_rate)])

        self.input_conv = conv_block(32, 3, 2, 3)
        self.block_names = []
        channels = 32
        for stage, filters, t, strides in _STAGES:
            for i, s in enumerate(strides):
                name = 'bottleneck_%d_%d' % (stage, i + 1)
                setattr(self, name, Bottleneck(filters, strides=s, expansion_factor=t, activation=act,
                                               dropout_rate=dropout_rate, kernel_initializer=init,
                                               kernel_regularizer=reg, name=name, in_channels=channels))
                self.block_names.append(name)
                channels = filters
        self.output_conv = conv_block(32, 1, 1, channels)
        self.out_channels = {'C3': 32, 'C4': 96, 'C5': 32}
        # train.Trainer installs a callable here while a collective is active (see resnet.ResNeXt.stage_cut): the backward pass
        # of the chain then runs in two parts, cut behind STAGE_CUT_AFTER, and the upper part's 7.3 MB of gradients (95 % of the
        # backbone's) are all-reduced underneath the lower part's backward pass on the large maps.  The cut costs one identity
        # 1x1 conv forward and backward on the C3 map (the chain kernels apply a GroupNorm in their CONSUMER: the first half
        # needs one) -- about 25 us per step, so it is taken only where there is a collective to hide.
        self.stage_cut = None
        self.stage_cut_needs_collective = True

    def _chain_blocks(self, first):
        blocks = []
        for name in self.block_names[first:]:
            b = getattr(self, name)
            conv1, norm1, act1, drop1 = b.expand_conv.layers
            dw, norm2, act2, drop2 = b.depthwise_conv.layers
            conv3, norm3, drop3 = b.linear_conv.layers
            blocks.append(ops_mb.Block(
                conv1.weight, ops_mb.Norm(norm1.gamma, norm1.beta, norm1.groups, norm1.eps, L.activation_name(act1), drop1.rate, drop1.seed),
                dw.weight, ops_mb.Norm(norm2.gamma, norm2.beta, norm2.groups, norm2.eps, L.activation_name(act2), drop2.rate, drop2.seed),
                conv3.weight, ops_mb.Norm(norm3.gamma, norm3.beta, norm3.groups, norm3.eps, None, drop3.rate, drop3.seed),
                dw.strides, b._same_shape))
        return blocks

    def _identity(self, c, device):
        """[1, 1, c, c] identity kernel (a constant, not a parameter) for the stage cut's pass-through conv."""
        cache = self.__dict__.setdefault('_eye_cache', {})
        key = (c, str(device))
        if key not in cache:
            cache[key] = torch.eye(c, dtype=torch.float32, device=device).reshape(1, 1, c, c).contiguous()
        return cache[key]

    def _chain_start(self, x, training):
        """Index of the first bottleneck the fused chain runs (None: no chain) for the stem output x."""
        if not (MB_CHAIN and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32) or (L.INFERENCE_F16 and not training):
            return None
        key = tuple(x.shape)
        cache = self.__dict__.setdefault('_chain_cache', {})
        if key not in cache:
            n, h, w, c = key
            shapes = []
            for name in self.block_names:
                b = getattr(self, name)
                shapes.append((n, h, w, c))
                s = b.depthwise_conv.layers[0].strides
                h, w, c = -(-h // s), -(-w // s), b.linear_conv.layers[0].filters
            start = None
            for i in range(len(self.block_names) - 1):
                if MB_CHAIN_MAX_HW and shapes[i][1] * shapes[i][2] > MB_CHAIN_MAX_HW:
                    continue
                if ops_mb.chain_supported(shapes[i], self._chain_blocks(i)):
                    start = i
                    break
            cache[key] = start
        return cache[key]

    def _call_f16(self, image):
        """The backbone in fp16 (F16_BACKBONE): stem on the 4-channel fp16 image, then every bottleneck folded; a Pending travels
        from a block to the next one's expand conv unless the block has a residual or its output is a tap of the pyramid.  C1
        (which no caller of an inference pass reads) is not materialised: the key is present, as in resnet.ResNeXt.call.
        ops_f16.FOLD off: every layer on its own (conv / depthwise, then the three-kernel GroupNorm)."""
        import ops_f16
        out = {}
        x = ops_f16.image_to_half4(image)
        if not ops_f16.FOLD:
            x = self.input_conv(x, False)
            for name in self.block_names:
                x = getattr(self, name)(x, False)
                if name in _TAP_AFTER:
                    out[_TAP_AFTER[name]] = x
            out['C5'] = self.output_conv(x, False)
            return out
        conv_s, norm_s, act_s, _ = self.input_conv.layers
        x = _f16_conv_norm(x, conv_s, norm_s, L.activation_name(act_s))
        for name in self.block_names:
            tap = _TAP_AFTER.get(name)
            x = getattr(self, name)._call_f16_folded(x, keep_pending=tap not in ('C3', 'C4'))
            if tap is not None:
                out[tap] = None if isinstance(x, ops_f16.Pending) else x
        conv_o, norm_o, act_o, _ = self.output_conv.layers
        c5 = _f16_conv_norm(x, conv_o, norm_o, L.activation_name(act_o))
        out['C5'] = c5.materialise() if isinstance(c5, ops_f16.Pending) else c5
        return out

    def call(self, input, training):
        if L.INFERENCE_F16 and not training and torch.is_tensor(input) and input.is_cuda and input.dtype == torch.float32:
            if F16_BACKBONE:
                return self._call_f16(input)
            # the backbone in fp32 (the fused chain), its taps cast for the fp16 FPN and heads
            import ops_f16
            L.INFERENCE_F16 = False
            try:
                out = self.call(input, training)
            finally:
                L.INFERENCE_F16 = True
            for k in ('C3', 'C4', 'C5'):
                out[k] = ops_f16.to_half(out[k])
            return out
        out = {}
        input = self.input_conv(input, training)
        start = self._chain_start(input, training)
        cut_at = self.block_names[self.block_names.index(STAGE_CUT_AFTER) + 1]
        for name in (self.block_names if start is None else self.block_names[:start]):
            if name == cut_at and self.stage_cut is not None and training and torch.is_grad_enabled():
                input = self.stage_cut(getattr(self, name), input, tuple(out.keys()))      # (layer by layer: the cut costs nothing)
            input = getattr(self, name)(input, training)
            if name in _TAP_AFTER:      # a tap feeds the next block and (C3, C4) the pyramid
                out[_TAP_AFTER[name]], input = ops.fanout(input, 2)
        conv_o, norm_o, act_o, drop_o = self.output_conv.layers
        if start is None:
            out['C5'] = self.output_conv(input, training)
            return out
        names = self.block_names[start:]
        blocks = self._chain_blocks(start)
        seed_dev = L.Dropout.seed_device_counter
        if (self.stage_cut is not None and training and torch.is_grad_enabled() and STAGE_CUT_AFTER in names[:-1]):
            k = names.index(STAGE_CUT_AFTER) + 1          # first half: names[:k], ends with the identity conv; second half: names[k:]
            c_mid = blocks[k - 1].w3.shape[3]
            eye = self._identity(c_mid, input.device)
            tap_a = [i for i, name in enumerate(names[:k]) if name in _TAP_AFTER]
            taps, y_mid = ops_mb.mb_chain(input, blocks[:k], eye, tap_a, training=training, seed_dev=seed_dev, tail_const=True)
            for i, t in zip(tap_a, taps):
                out[_TAP_AFTER[names[i]]] = t
            x_mid = self.stage_cut(getattr(self, names[k]), y_mid, tuple(out.keys()))
            input, blocks, names = x_mid, blocks[k:], names[k:]
        tap_after = [i for i, name in enumerate(names) if name in _TAP_AFTER]
        taps, y_tail = ops_mb.mb_chain(input, blocks, conv_o.weight, tap_after, training=training, seed_dev=seed_dev)
        for i, t in zip(tap_after, taps):
            out[_TAP_AFTER[names[i]]] = t
        # the output block's own GroupNorm + activation + dropout (its 1x1 conv ran as the chain's tail)
        out['C5'] = norm_o.fused(y_tail, training, act=L.activation_name(act_o), dropout=drop_o)
        return out
