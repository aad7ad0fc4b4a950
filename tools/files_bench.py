"""Real-image training throughput: writes a VOC-format tree of shapes-rendered JPEGs at Pascal VOC's common raw sizes (plus a tail
of other sizes) into DIR, trains through train.main with --shape-runs 0 and 8, and prints one JSON line per measurement:
images/s (two per step: [image, hflip]), recaptures per 100 steps, the host decode rate of one worker, and the in-memory
shapes stream at the same --scale.  The training times are wall time of train.main's loop, graph captures included.

    python tools/files_bench.py DIR [--images 96] [--steps 200] [--scale 512] [--decode-workers 4] [--shape-runs 0 8] [--augment [S]]
                                [--samples-per-step K]

--augment [S]: the file runs train with --augment (and --augment-crop S when S is given): the cost of the augmentation kernels and of
the loader thread's draws shows as the difference to a run without it.
--samples-per-step K: the file runs train with --samples-per-step K (K > 1: 2K images per step, the loader orders by groups and
--shape-runs only labels the line); images/s counts the staged samples, so lines of different K compare directly.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'retinanet-tensorflow_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

# (h, w): VOC's most common raw sizes first, then a tail of others
COMMON = [(375, 500), (500, 375), (333, 500), (500, 500)]
TAIL = [(281, 500), (366, 500), (500, 333), (400, 500), (480, 640), (334, 500), (500, 400), (375, 499)]


def write_dataset(root, n):
    import files_fixtures as ff
    sizes = [COMMON[i % 4] if i % 5 != 4 else TAIL[(i // 5) % len(TAIL)] for i in range(n)]
    names = ff.write_voc(root, ff.render(sizes, seed=1), quality=90)
    return sizes, names


def run(argv):
    import train
    train.main(argv)
    r = dict(train.LAST_RUN)
    r['images_per_s'] = round(2 * r['samples'] / r['seconds'], 1)
    r['recaptures_per_100_steps'] = round(100.0 * r['recaptures'] / max(1, r['steps']), 2)
    r['seconds'] = round(r['seconds'], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('dir')
    ap.add_argument('--images', type=int, default=96)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--scale', type=int, default=512)
    ap.add_argument('--decode-workers', type=int, default=4)
    ap.add_argument('--backbone', default='mobilenet_v2')
    ap.add_argument('--shape-runs', type=int, nargs='+', default=[0, 8])
    ap.add_argument('--augment', type=float, nargs='?', const=1.0, default=None, metavar='S')
    ap.add_argument('--samples-per-step', type=int, default=1, metavar='K')
    ap.add_argument('--no-shapes', action='store_true', help='skip the in-memory shapes stream')
    a = ap.parse_args()
    import dataset
    sizes, names = write_dataset(a.dir, a.images)
    files = [os.path.join(a.dir, 'JPEGImages', n + '.jpg') for n in names]
    t = time.perf_counter()
    for f in files:
        dataset.decode_image(f)
    dt = time.perf_counter() - t
    print(json.dumps({'what': 'decode', 'images': len(files), 'images_per_s_per_worker': round(len(files) / dt, 1),
                      'network_sizes': len({dataset.rescale_size(s, a.scale) for s in sizes})}), flush=True)
    common = ['--scale', str(a.scale), '--steps-per-epoch', str(a.steps), '--backbone', a.backbone, '--dropout', '0.0']
    aug = []
    if a.augment is not None:
        aug = ['--augment'] + (['--augment-crop', str(a.augment)] if a.augment < 1.0 else [])
    group = ['--samples-per-step', str(a.samples_per_step)] if a.samples_per_step != 1 else []
    for k in a.shape_runs:
        r = run(['--dataset', 'pascal', a.dir, 'trainval', '--shape-runs', str(k), '--decode-workers', str(a.decode_workers)] + common + aug
                + group)
        print(json.dumps(dict(what='pascal', shape_runs=k, augment=a.augment, samples_per_step=a.samples_per_step, **r)), flush=True)
    if not a.no_shapes:
        r = run(['--dataset', 'shapes'] + common)
        print(json.dumps(dict(what='shapes', **r)), flush=True)


if __name__ == '__main__':
    main()
