"""ms/step of the headline training step (MobileNetV2-FPN, 512 x 512, batch 2, focal loss, dropout 0.2: bench.py's workload and
timing loop), momentum at a constant rate, with and without the guard against non-finite gradients:

    --mode plain          no clipping: the one-graph step as it has always been
    --mode clip           Trainer(grad_clip_norm=C), default C = 1.0
    --guard               Trainer(skip_nonfinite=True) on top of either (not with --tree of a commit from before the guard):
                          clipped, the one-thread control launch (rn_step_control_eval) between the norm's finalize and the update;
                          unclipped, the norm pass of its own (8 B per parameter) that the fused update otherwise spares

One measurement per process; prints one JSON line.  --tree DIR imports the package (and its librn_hip.so) from another checkout
of this repository, e.g. the parent commit, so that two commits are compared on one box in interleaved runs:

    for i in 1 2 3; do
      for mode in plain clip; do
        python tools/guard_cost.py --mode $mode --tree /tmp/parent
        python tools/guard_cost.py --mode $mode
        python tools/guard_cost.py --mode $mode --guard
      done
    done
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['plain', 'clip'], required=True)
    ap.add_argument('--guard', action='store_true')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--clip', type=float, default=1.0)
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    for p in (root, os.path.join(root, 'retinanet-tensorflow_amd')):
        sys.path.insert(0, p)
    import torch
    import bench                                       # the tree's own: workload constants, make_batch
    import dataset, layers, levels, retinanet, train
    assert os.path.abspath(train.__file__).startswith(root), train.__file__
    dev, _, _, _ = train.init_distributed()
    torch.manual_seed(0)
    lv = levels.build_levels()
    net = retinanet.RetinaNet('mobilenet_v2', lv, bench.NUM_CLASSES, layers.elu, 0.2).to(dev)
    image, boxes, cls, nobj = bench.make_batch(0, dev)

    def features():
        c, r, m = dataset.build_labels((bench.IMAGE_SIZE, bench.IMAGE_SIZE), cls, boxes, lv, bench.NUM_CLASSES, num_obj=nobj, flip_pair=True)
        return {'image': image, 'detection': {'classifications': c, 'regressions': r}, 'trainable_masks': m}
    features.concurrent = True

    kw = {'grad_clip_norm': a.clip} if a.mode == 'clip' else {}
    if a.guard:
        kw['skip_nonfinite'] = True
    tr = train.Trainer(net, lv, optimizer='momentum', learning_rate=1e-2, loss_mode='focal', device=dev, use_graph=True,
                       input_fn=features, **kw)
    tr.check_interval = 0
    for _ in range(a.warmup):
        tr.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.step()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / a.steps
    norm = float(tr.opt.norm_reg[0].item()) ** 0.5       # (the last step's)
    skipped = tr.skipped_updates() if a.guard else (0, 0)
    print(json.dumps({'mode': a.mode, 'guard': bool(a.guard), 'clip': a.clip if a.mode == 'clip' else None,
                      'tree': os.path.basename(root), 'steps': a.steps, 'updates': tr.opt.step_count, 'skipped': skipped[0],
                      'ms_per_step': round(ms, 4), 'images_per_s': round(bench.BATCH * 1000.0 / ms, 1),
                      'one_graph': bool(tr._graphs[5]), 'graph_sets': len(tr._graph_cache), 'recaptures': tr.recaptures,
                      'arena_mb': round(tr.arena.count * 4 / 1e6, 1), 'last_norm': round(norm, 4),
                      'class_loss': round(float(out['class_loss'].item()), 6)}), flush=True)


if __name__ == '__main__':
    main()
