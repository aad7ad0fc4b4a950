"""The network of tests/test_gpu_mb_f16.py and its yardstick: the fp16-STORAGE MODEL of the MobileNetV2-FPN RetinaNet.

build_net() is the product net with the test's seeds (gamma / beta perturbed as in the ResNeXt fp16 test).  model_figures() runs
oracle.model_ref on the same parameters in fp64 twice -- plain, and with the backbone's `dropout(site, x)` hook rounding every
stored activation to fp16 -- and returns the relative L2 distance of the two per output: C3, C4, C5, and P3 .. P7 logits (mean
removed) / box deltas.  That is what storing the backbone's activations in fp16 costs THIS net with exact arithmetic everywhere
else; the test grants the product a multiple of it.

    python tests/mb_f16_ref.py          prints the figures (CPU, about a minute); they are quoted in tests/test_gpu_mb_f16.py"""
import os
import sys

import torch

NUM_CLASSES = 80
IMAGE_SHAPE = (2, 256, 256, 3)
LEVELS = ("P3", "P4", "P5", "P6", "P7")


def build_net():
    import layers, levels, retinanet
    torch.manual_seed(5)
    net = retinanet.RetinaNet('mobilenet_v2', levels.build_levels(), NUM_CLASSES, layers.elu, 0.0)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("gamma"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("beta"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return net


def image():
    return torch.randn(IMAGE_SHAPE, generator=torch.Generator().manual_seed(7))


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def output_errors(feats, out, feats_ref, out_ref):
    """relative L2 per output of one forward against another: {'C3': .., 'P3': max(logits with the mean removed, box deltas), ..}"""
    err = {k: rel_l2(feats[k].float(), feats_ref[k]) for k in ("C3", "C4", "C5")}
    for k in LEVELS:
        a, b = out["classifications"][k].double().cpu(), out_ref["classifications"][k].double().cpu()
        err[k] = max(rel_l2(a - a.mean(), b - b.mean()), rel_l2(out["regressions"][k], out_ref["regressions"][k]))
    return err


def model_figures():
    from helpers import to_oracle_name
    from oracle import model_ref
    net = build_net()
    params = {to_oracle_name(k): v.detach().double() for k, v in net.named_parameters()}
    x = image().double()

    def store_f16(site, t):
        return t.half().double()

    with torch.no_grad():
        feats64 = model_ref.mobilenet_v2_forward(params, x, "elu")
        out64 = model_ref.retinanet_forward(params, x, NUM_CLASSES, act="elu")
        feats16 = model_ref.mobilenet_v2_forward(params, x, "elu", dropout=store_f16)
        out16 = model_ref.retinanet_forward(params, x, NUM_CLASSES, act="elu", dropout=store_f16)
    return output_errors(feats16, out16, feats64, out64)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "retinanet-tensorflow_amd"), os.path.join(root, "tests")]
    for k, v in model_figures().items():
        print("MB_F16_MODEL %-3s rel L2 %.3e" % (k, v))
