"""Kernel time of the detection loss at the headline shape (512 x 512, batch 2, 80 classes, the rows of the five levels of
levels.build_levels) for the two existing modes and for class-loss specs (csrc/loss_terms.hip), forward (reduce + sum + finalize:
three launches) and backward (one launch), each as a ratio to the existing bce_dice mode IN THE SAME PROCESS:

    python tools/loss_terms_cost.py --out profiles/loss_terms_cost.txt

The library entries are called directly on pre-allocated buffers.  Each figure: device events around one replay of a graph of
--launches calls (kernel time, not the host's launch rate), after a warm-up replay; --rounds rounds, the configurations
interleaved inside a round, median and range over the rounds.  RN_LOSS_TERMS_GENERAL=1 is set for the whole process so that
'bce+dice' runs the general kernels (the existing modes are measured through rn_loss_fwd / rn_loss_bwd, which the switch does
not touch): that row is what the dispatch rule saves."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('bce_dice', 'focal', 'bce+dice', 'bce+jaccard', 'balanced_bce+dice',
           'bce:0.7+balanced_bce:0.4+dice:0.5:0.3+jaccard:0.6:2+fixed_iou:0.3:0.01+focal:0.2')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    os.environ['RN_LOSS_TERMS_GENERAL'] = '1'              # read by the library at its first rn_loss_terms_* call
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
        rp.append(torch.randn((rows, 4), device=dev, generator=g))
        rl.append(torch.randn((rows, 4), device=dev, generator=g))
        msk.append(((torch.rand((rows,), device=dev, generator=g) < 0.9) | fg).to(torch.uint8))
    dz, dr = [torch.empty_like(t) for t in z], [torch.empty_like(t) for t in rp]
    segs = ops._loss_segs(z, lab, rp, rl, msk, dz, dr)
    nseg = len(z)
    stats = torch.zeros((L.rn_loss_terms_stats_floats(c),), device=dev)
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
        desc = losses.parse_class_loss(cfg).struct()
        ws = _rn.workspace(L.rn_loss_terms_workspace(segs, nseg, c, ctypes.byref(desc)), dev)
        return (lambda: _rn.check(L.rn_loss_terms_fwd(segs, nseg, c, ctypes.byref(desc), _rn.f32(stats), _rn.f32(cls), _rn.f32(reg),
                                                      ws.data_ptr(), ws.numel(), _rn.stream()), 'rn_loss_terms_fwd'),
                lambda: _rn.check(L.rn_loss_terms_bwd(segs, nseg, c, ctypes.byref(desc), _rn.f32(stats), _rn.f32(one), _rn.f32(one),
                                                      _rn.stream()), 'rn_loss_terms_bwd'))

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
    rows = sum(int(m.numel()) for m in msk)
    med = {key: statistics.median(v) for key, v in us.items()}
    lines = ['detection loss kernels at %d rows x %d classes (%.1f MB of logits and labels), us per call: median (min - max) of %d '
             'rounds, each one replay of a graph of %d calls; ratio to the existing bce_dice mode in the same process'
             % (rows, c, rows * c * 8 / 1e6, a.rounds, a.launches), '']
    lines.append('%-32s %-28s %-7s %-28s %-7s' % ('configuration', 'forward (3 launches)', 'ratio', 'backward', 'ratio'))
    for cfg in CONFIGS:
        name = {'bce_dice': "mode 'bce_dice' (existing)", 'focal': "mode 'focal' (existing)", 'bce+dice': 'bce+dice, general kernels forced',
                CONFIGS[-1]: 'all six terms'}.get(cfg, cfg)
        cells = []
        for which in ('fwd', 'bwd'):
            v = us[cfg, which]
            cells += ['%.2f (%.2f - %.2f)' % (med[cfg, which], min(v), max(v)), '%.3f' % (med[cfg, which] / med['bce_dice', which])]
        lines.append('%-32s %-28s %-7s %-28s %-7s' % tuple([name] + cells))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
