"""The fp16 depthwise kernel (csrc/depthwise_f16.hip) alone on the depthwise layers of MobileNetV2 at a 512 x 512 input, batch 2,
as the folded backbone calls it (input fold + statistics): device-event time per launch against its memory bound -- one read of
x and one write of y at the 6.29 TB/s a float4 copy achieves on the MI355X.  Maps of a few MB stay in the caches between
launches; the figure is what the layer costs inside a forward pass, not an HBM measurement.
    python tools/dw_f16_bench.py [input size] [batch] [launches]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "retinanet-tensorflow_amd")):
    sys.path.insert(0, p)
import torch

COPY_BW = 6.29e12


def layers_of(size):
    """(name, map size, channels, stride) of every depthwise conv, from the block table"""
    import mobilenet_v2
    out, hw, c = [], -(-size // 2), 32
    for stage, filters, t, strides in mobilenet_v2._STAGES:
        for i, s in enumerate(strides):
            out.append(("bottleneck_%d_%d" % (stage, i + 1), hw, c * t, s))
            hw, c = -(-hw // s), filters
    return out


def main(size=512, batch=2, launches=50):
    import ops_f16
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    total_us = total_bound = 0.0
    for name, hw, c, s in layers_of(size):
        g = ops_f16.gn_groups(c, 32)
        raw = torch.randn(batch, hw, hw, c, device=dev).half()
        w = torch.randn(3, 3, c, 1, device=dev) / 3

        class Norm(object):
            gamma, beta, groups, eps = torch.ones(c, device=dev), torch.zeros(c, device=dev), 32, 1e-5

        p = ops_f16.Pending(raw, torch.zeros(batch, g, device=dev), torch.ones(batch, g, device=dev), Norm.gamma, Norm.beta, g, "elu")
        for _ in range(10):
            y, _, _ = ops_f16._depthwise_call(p, w, s, True)
        # the launches replayed from one hipGraph: the host's enqueue time (longer than the kernel on the small maps) stays out
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(launches):
                ops_f16._depthwise_call(p, w, s, True)
        graph.replay()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(5):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / (5 * launches)
        del graph
        bound = (raw.numel() + y.numel()) * 2 / COPY_BW * 1e6
        total_us += us
        total_bound += bound
        print(json.dumps({"layer": name, "map": hw, "c": c, "stride": s, "MB": round((raw.numel() + y.numel()) * 2 / 1e6, 2),
                          "us_per_launch": round(us, 2), "bound_us": round(bound, 2), "share_of_bound": round(bound / us, 3)}), flush=True)
    print(json.dumps({"layers": "all 17", "us": round(total_us, 1), "bound_us": round(total_bound, 1)}), flush=True)


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
