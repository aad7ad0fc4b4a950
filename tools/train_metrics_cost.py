"""ms/step of the headline training step (MobileNetV2-FPN, 512 x 512, batch 2, focal loss, dropout 0.2, momentum at a constant rate:
bench.py's workload and timing loop) with and without the running training metrics, against the parent commit's library:

    (p)   RN_LIB_PATH=PARENT/librn_hip.so python tools/train_metrics_cost.py      the parent's kernels under this commit's host
                                                                                  code (the entries were added without an ABI
                                                                                  bump, so the parent's library loads)
    (off) python tools/train_metrics_cost.py                                      this commit, Trainer(train_metrics=False)
    (on)  python tools/train_metrics_cost.py --metrics                            this commit, Trainer(train_metrics=True)
    (k)   python tools/train_metrics_cost.py --kernels                            the pass and the fold alone, on tensors of the
                                                                                  headline shapes: device events around 200 launches

One measurement per process; prints one JSON line.  The driver (--rounds N) runs them interleaved, in the order of the list, each
in a fresh child process with a time limit of its own, stops at the first child that fails, and writes the table:

    python tools/train_metrics_cost.py --rounds 6 --alternate --parent-lib PARENT/librn_hip.so --out profiles/train_metrics_cost.txt

(--alternate: every second round in the reverse order, so that a run's position inside a round does not side with one build)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    for p in (ROOT, os.path.join(ROOT, 'retinanet-tensorflow_amd')):
        sys.path.insert(0, p)
    import torch
    import bench                                       # workload constants, make_batch
    import _rn, dataset, layers, levels, retinanet, train
    dev, _, _, _ = train.init_distributed()
    torch.manual_seed(0)
    lv = levels.build_levels()
    net = retinanet.RetinaNet('mobilenet_v2', lv, bench.NUM_CLASSES, layers.elu, 0.2).to(dev)
    image, boxes, cls, nobj = bench.make_batch(0, dev)

    def features():
        c, r, m = dataset.build_labels((bench.IMAGE_SIZE, bench.IMAGE_SIZE), cls, boxes, lv, bench.NUM_CLASSES, num_obj=nobj, flip_pair=True)
        return {'image': image, 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m}
    features.concurrent = True

    kw = {'train_metrics': True} if a.metrics else {}
    tr = train.Trainer(net, lv, optimizer='momentum', learning_rate=1e-2, loss_mode='focal', device=dev, use_graph=True,
                       input_fn=features, **kw)
    tr.check_interval = 0
    for _ in range(a.warmup):
        tr.step()
    if a.metrics:
        tr.train_metrics()                             # the window covers the timed steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.step()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / a.steps
    res = {'lib': os.path.relpath(_rn.LIB_PATH, ROOT), 'metrics': bool(a.metrics), 'steps': a.steps, 'ms_per_step': round(ms, 4),
           'images_per_s': round(bench.BATCH * 1000.0 / ms, 1), 'one_graph': bool(tr._graphs[5]), 'graph_sets': len(tr._graph_cache),
           'recaptures': tr.recaptures, 'class_loss': round(float(out['class_loss'].item()), 6),
           'last_norm': round(float(tr.opt.norm_reg[0].item()) ** 0.5, 4)}
    if a.metrics:
        w = tr.train_metrics()
        res['window'] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in w.items()}
    print(json.dumps(res), flush=True)


def kernels(a):
    """The pass and the fold alone at the headline shapes (random logits, a fifth of the rows trainable foreground)."""
    for p in (ROOT, os.path.join(ROOT, 'retinanet-tensorflow_amd')):
        sys.path.insert(0, p)
    import torch
    import bench
    import levels, metrics, utils
    dev = torch.device('cuda:0')
    lv = levels.build_levels()
    g = torch.Generator(device=dev).manual_seed(0)
    n, c = bench.BATCH, bench.NUM_CLASSES
    cls_l, cls_z, reg_l, reg_p, msk = {}, {}, {}, {}, {}
    for i, k in enumerate(lv):
        s = bench.IMAGE_SIZE // (8 << i)
        shape = (n, s, s, lv.num_anchors)
        cls_z[k] = torch.randn(shape + (c,), device=dev, generator=g)
        fg = torch.rand(shape, device=dev, generator=g) < 0.2
        cls_l[k] = torch.zeros(shape + (c,), device=dev)
        cls_l[k][..., 0] = fg.float()
        reg_l[k] = torch.rand(shape + (4,), device=dev, generator=g) - 0.5
        reg_p[k] = torch.rand(shape + (4,), device=dev, generator=g) - 0.5
        msk[k] = torch.ones(shape, dtype=torch.uint8, device=dev)
    lab = utils.DetectionTrainable(utils.Classification(None, cls_l), reg_l, None, msk)
    log = utils.DetectionTrainable(utils.Classification(cls_z, None), reg_p, None, msk)
    tm = metrics.TrainMetrics(dev)
    one = torch.ones((), device=dev)
    size = (bench.IMAGE_SIZE, bench.IMAGE_SIZE)
    out = {}
    for name, fn in (('pass', lambda: tm.update(lab, log, lv, size)), ('fold', lambda: tm.fold(one, one, one))):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g_ = torch.cuda.CUDAGraph()                    # 200 launches as one graph: kernel time, not the host's launch rate
        with torch.cuda.graph(g_):
            for _ in range(200):
                fn()
        g_.replay()
        torch.cuda.synchronize()
        e0.record()
        g_.replay()
        e1.record()
        torch.cuda.synchronize()
        out[name + '_us'] = round(1000.0 * e0.elapsed_time(e1) / 200, 2)
    rows = sum(int(v.numel()) for v in msk.values())
    out.update(rows=rows, classes=c, bytes_read=rows * (2 * c * 4 + 1) + int(0.2 * rows) * 32)
    print(json.dumps(out), flush=True)


def drive(a):
    py = sys.executable
    me = os.path.abspath(__file__)
    configs = {'p': ([], {'RN_LIB_PATH': os.path.abspath(a.parent_lib)}), 'off': ([], {}), 'on': (['--metrics'], {})}
    order = a.order.split(',')
    assert sorted(order) == sorted(configs), a.order
    configs = [(name,) + configs[name] for name in order]                  # (the table's columns stay p, off, on)
    rows = []
    for r in range(a.rounds):
        row = {}
        for name, args, env in (configs[::-1] if (a.alternate and r % 2) else configs):
            p = subprocess.run([py, me, '--steps', str(a.steps), '--warmup', str(a.warmup)] + args, env={**os.environ, **env},
                               stdout=subprocess.PIPE, universal_newlines=True, timeout=240)
            if p.returncode != 0:
                print('round %d (%s): exit status %d: stopping' % (r + 1, name, p.returncode), flush=True)
                return 1
            res = json.loads(p.stdout.strip().splitlines()[-1])
            assert res['one_graph'] and res['graph_sets'] == 1 and res['recaptures'] == 0, res
            print(r + 1, name, json.dumps(res), flush=True)
            row[name] = res
        rows.append(row)
    p = subprocess.run([py, me, '--kernels'], stdout=subprocess.PIPE, universal_newlines=True, timeout=240)
    if p.returncode != 0:
        print('--kernels: exit status %d' % p.returncode, flush=True)
        return 1
    kern = json.loads(p.stdout.strip().splitlines()[-1])
    ms = {k: [row[k]['ms_per_step'] for row in rows] for k in ('p', 'off', 'on')}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    lo, hi = min(ms['p']), max(ms['p'])
    lines = ['round   (p)       (off)     (on)        ms per step, %d warm-up + %d timed steps, one process per figure, run in the order %s'
             % (a.warmup, a.steps, a.order + (' in odd rounds, reversed in even ones' if a.alternate else ''))]
    for i in range(a.rounds):
        lines.append('  %d     %.4f    %.4f    %.4f' % (i + 1, ms['p'][i], ms['off'][i], ms['on'][i]))
    lines.append('mean    %.4f    %.4f    %.4f' % (mean['p'], mean['off'], mean['on']))
    lines.append('')
    lines.append("repeat spread of the parent's own figure: %.2f %% (%.4f - %.4f)" % (100.0 * (hi - lo) / lo, lo, hi))
    inside = [lo <= v <= hi for v in ms['off']]
    lines.append("(off) inside the parent's range in %d of %d rounds; per round against (p): %s; means %+.2f %%" % (
        sum(inside), a.rounds, ', '.join('%+.2f %%' % (100.0 * (o - q) / q) for o, q in zip(ms['off'], ms['p'])),
        100.0 * (mean['off'] - mean['p']) / mean['p']))
    lines.append("(on) per round against (off): %s; means %+.2f %% = %+.1f us" % (
        ', '.join('%+.2f %%' % (100.0 * (o - q) / q) for o, q in zip(ms['on'], ms['off'])),
        100.0 * (mean['on'] - mean['off']) / mean['off'], 1000.0 * (mean['on'] - mean['off'])))
    lines.append("the kernels alone (device events around a graph of 200 launches): pass %.2f us over %d rows x %d classes "
                 "(%.1f MB read: %.0f GB/s), fold %.2f us" % (kern['pass_us'], kern['rows'], kern['classes'], kern['bytes_read'] / 1e6,
                                                             kern['bytes_read'] / kern['pass_us'] / 1e3, kern['fold_us']))
    lines.append("class_loss / last gradient norm at the end of every run: %s" % sorted(
        set((row[k]['class_loss'], row[k]['last_norm']) for row in rows for k in row)))
    lines.append("window of the last (on) run: %s" % json.dumps(rows[-1]['on']['window']))
    text = '\n'.join(lines) + '\n'
    print(text, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--metrics', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=0)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--order', default='p,off,on', help='with --rounds: the order of the three runs inside a round')
    ap.add_argument('--alternate', action='store_true', help='with --rounds: every second round runs in the reverse order')
    a = ap.parse_args()
    if a.rounds:
        if not a.parent_lib:
            ap.error('--rounds needs --parent-lib PATH (the parent commit\'s librn_hip.so)')
        sys.exit(drive(a))
    if a.kernels:
        kernels(a)
    else:
        measure(a)


if __name__ == '__main__':
    main()
