"""Kernel time of the regression-loss terms (csrc/regr_terms.hip) at the headline loss shape (512 x 512, batch 2, 80 classes, the
rows of the five levels of levels.build_levels: 98 208 rows), forward (reduce + finalize: two launches) and backward (one launch),
for 'huber:2', 'giou' and 'huber+iou+giou', each as a ratio to rn_loss_fwd / rn_loss_bwd (mode bce_dice) IN THE SAME PROCESS:

    python tools/regr_terms_cost.py --out profiles/regr_terms_cost.txt

The library entries are called directly on pre-allocated buffers.  Each figure: device events around one replay of a graph of
--launches calls (kernel time, not the host's launch rate), after a warm-up replay; --rounds rounds, the configurations
interleaved inside a round, median and range over the rounds.

What to expect: the forward reads the class labels once more to find the foreground rows -- rows x C x 4 B = 31 MB, about 9 us at
the 3.6 TB/s the metrics pass reached -- plus 33 B per row of boxes, mask and fg_rows; the backward is one pass over [rows, 4]:
1 B (fg_rows) + 16 B (store) per row and 32 B more on a foreground row, 1.7 MB, which is launch latency rather than bandwidth."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('bce_dice', 'huber:2', 'giou', 'huber+iou+giou')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, 'retinanet-tensorflow_amd')):
        sys.path.insert(0, p)
    import torch
    import bench
    import _rn, levels, losses, ops
    if not torch.cuda.is_available():
        raise _rn.RnError("the cost of the loss kernels is measured on an MI355X: there is nothing to time without one")
    dev = torch.device('cuda:0')
    L = _rn.lib()
    lv = levels.build_levels()
    g = torch.Generator(device=dev).manual_seed(0)
    n, c = bench.BATCH, bench.NUM_CLASSES
    z, lab, rp, rl, msk = [], [], [], [], []
    for i, k in enumerate(lv):
        s = bench.IMAGE_SIZE // (8 << i)
        rows = n * s * s * lv.num_anchors
        z.append(torch.randn((rows, c), device=dev, generator=g) * 2 - 2)
        fg = torch.rand((rows,), device=dev, generator=g) < 0.05
        l = torch.zeros((rows, c), device=dev)
        l[fg, torch.randint(0, c, (int(fg.sum()),), device=dev, generator=g)] = 1.0
        lab.append(l)
        rl.append(torch.randn((rows, 4), device=dev, generator=g) * 0.4)
        rp.append(rl[-1] + torch.randn((rows, 4), device=dev, generator=g) * 0.4)
        msk.append(((torch.rand((rows,), device=dev, generator=g) < 0.9) | fg).to(torch.uint8))
    dz, dr = [torch.empty_like(t) for t in z], [torch.empty_like(t) for t in rp]
    segs = ops._loss_segs(z, lab, rp, rl, msk, dz, dr)
    nseg = len(z)
    rows = sum(int(m.numel()) for m in msk)
    stats = torch.zeros((_rn.LOSS_STATS_HEADER + 3 * c,), device=dev)
    rstats = torch.zeros((_rn.REGR_STATS_FLOATS,), device=dev)
    fg_rows = torch.zeros((rows,), dtype=torch.uint8, device=dev)
    one = torch.ones((1,), device=dev)
    cls, reg = torch.zeros((), device=dev), torch.zeros((), device=dev)

    def calls(cfg):
        if cfg in _rn.LOSS_MODE:
            mode = _rn.LOSS_MODE[cfg]
            ws = _rn.workspace(L.rn_loss_workspace(segs, nseg, c), dev)
            return (lambda: _rn.check(L.rn_loss_fwd(segs, nseg, c, mode, _rn.f32(stats), _rn.f32(cls), _rn.f32(reg), ws.data_ptr(),
                                                    ws.numel(), _rn.stream()), 'rn_loss_fwd'),
                    lambda: _rn.check(L.rn_loss_bwd(segs, nseg, c, mode, _rn.f32(stats), _rn.f32(one), _rn.f32(one), _rn.stream()),
                                      'rn_loss_bwd'))
        desc = losses.parse_regr_loss(cfg).struct()
        ws = _rn.workspace(max(L.rn_regr_terms_workspace(segs, nseg, c, ctypes.byref(desc)), L.rn_loss_workspace(segs, nseg, c)), dev)
        return (lambda: _rn.check(L.rn_regr_terms_fwd(segs, nseg, c, ctypes.byref(desc), _rn.f32(rstats), _rn.f32(reg), _rn.ptr(fg_rows),
                                                      ws.data_ptr(), ws.numel(), _rn.stream()), 'rn_regr_terms_fwd'),
                lambda: _rn.check(L.rn_regr_terms_bwd(segs, nseg, ctypes.byref(desc), _rn.f32(rstats), _rn.ptr(fg_rows), _rn.f32(one),
                                                      _rn.stream()), 'rn_regr_terms_bwd'))

    graphs = {}
    for cfg in CONFIGS:
        for which, fn in zip(('fwd', 'bwd'), calls(cfg)):
            fn()                                            # (the forward first: the backward reads its statistics)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(a.launches):
                    fn()
            gr.replay()
            graphs[cfg, which] = gr
    torch.cuda.synchronize()
    us = {key: [] for key in graphs}
    for r in range(a.rounds):
        for key in (list(graphs) if r % 2 == 0 else list(graphs)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[key].replay()
            e1.record()
            torch.cuda.synchronize()
            us[key].append(1000.0 * e0.elapsed_time(e1) / a.launches)
    med = {key: statistics.median(v) for key, v in us.items()}
    nfg = int(fg_rows.sum().item())
    fwd_mb, bwd_mb = (rows * c * 4 + rows * 2 + nfg * 32) / 1e6, (rows * 17 + nfg * 32) / 1e6
    lines = ['regression-loss terms at %d rows x %d classes in %d segments (%d foreground rows), us per call: median (min - max) of %d '
             'rounds, each one replay of a graph of %d calls; ratio to rn_loss_fwd / rn_loss_bwd (bce_dice) in the same process'
             % (rows, c, nseg, nfg, a.rounds, a.launches),
             'bytes a call must move: forward %.1f MB (the class labels once more: %.1f us at 3.6 TB/s), backward %.1f MB (%.1f us)'
             % (fwd_mb, fwd_mb / 3.6, bwd_mb, bwd_mb / 3.6), '']
    lines.append('%-34s %-28s %-7s %-28s %-7s' % ('configuration', 'forward', 'ratio', 'backward', 'ratio'))
    for cfg in CONFIGS:
        name = {'bce_dice': "rn_loss_fwd / rn_loss_bwd (bce_dice)", 'huber:2': 'huber:2 (no expf)'}.get(cfg, cfg)
        cells = []
        for which in ('fwd', 'bwd'):
            v = us[cfg, which]
            cells += ['%.2f (%.2f - %.2f)' % (med[cfg, which], min(v), max(v)), '%.3f' % (med[cfg, which] / med['bce_dice', which])]
        lines.append('%-34s %-28s %-7s %-28s %-7s' % tuple([name] + cells))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
