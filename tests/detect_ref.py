"""The reference side of the detection kernels' case table (csrc/decode_nms.hip): plain numpy, no torch, no GPU.

  CASES            named cases: entry point, batch, class count, levels, thresholds, capacity rule, switches, input recipe
  make_case        deterministic inputs of a case
  plan_ref         an independent model of the host-side choices rn_detect_plan reports (written from the rules the kernel
                   file documents: which scan kernel, the grids, the emit mode, the segment path, the workspace)
  run_ref          the oracle: oracle/utils_ref.py's boxes_decode (with the case's score threshold), merge_boxes_decoded and,
                   per (image, class), nms_indices_vectorised with the case's max_output_size / iou_threshold -- extended to
                   return every survivor's image and flat anchor row, and counts[]
  device_branches  the data-dependent branches a case takes on the device (scatter half, sort in LDS / global memory, NMS
                   batches, the cap inside a batch, early exit, gather passes), computed from the reference alone
  suppresses_f32 / suppresses_fast_f32   float32 models of the two device predicates, every operation a separate float32 step

Number formats.  Probabilities lie on the grid k / 1024 and logits on k / 64 with |z| <= 8: both exact in fp16, so a case means
the same numbers in either storage type.  Distinct candidate logits then differ by >= sigmoid'(8) / 64 = 5.2e-6 in probability,
more than twice the 1e-6 granted to the hardware exponential: the order of the device's scores is the order of the fp64
sigmoid rounded to fp32, and equal logits give equal device scores, so classes, boxes, images, anchors and order are exact."""
import functools
import zlib
from dataclasses import dataclass, replace

import numpy as np

from oracle import utils_ref

f32 = np.float32
BAND = f32(9.5367431640625e-07)      # 2^-20: suppresses_fast's relative band around inter == thr * u
FLT_MIN = f32(1.17549435e-38)        # a threshold below it (0.0): the exact quotient always decides


@dataclass(frozen=True)
class Level:
    h: int
    w: int
    A: int
    half: bool = False        # prob stored as fp16
    logit: bool = False       # prob holds logits
    half_reg: bool = False    # raw regression stored as fp16 (entry detect_raw)

    @property
    def rows(self):
        return self.h * self.w * self.A


@dataclass(frozen=True)
class Case:
    entry: str                # "detect" (decoded boxes) | "detect_raw" | "boxes_decode" | "nms_classwise"
    n: int
    C: int
    levels: tuple = ()
    score_thr: float = 0.5
    iou_thr: float = 0.5
    max_per_class: int = 1000
    cap: object = "rows"      # "rows": n * rows per image; "rows/16"; or a number
    env: tuple = ()           # ((name, value), ...)
    process: bool = False     # a switch read once per process: the case runs in a fresh child
    recipe: str = "hot"
    hot: float = 0.08
    hot_classes: tuple = ()   # () = (0, C // 2, C - 1)
    seed: int = 0


BASE = (Level(3, 5, 9), Level(1, 1, 9), Level(1, 1, 9))       # 135 + 9 + 9 rows, 3 + 1 + 1 waves per image


def _lv(levels, **kw):
    return tuple(replace(l, **kw) for l in levels)


def _build_cases():
    c = {}
    # ---- scan families on the base pyramid, n = 3: every class count in probability ("p") and logit ("z") mode
    for half, cs in ((False, (4, 20, 36, 64, 80, 84, 100, 128, 132, 3, 5, 130)), (True, (8, 40, 128, 256, 80, 264, 12))):
        for C in cs:
            for mode in "pz":
                entry = {4: "detect_raw", 80: "detect_raw", 20: "boxes_decode", 40: "boxes_decode"}.get(C, "detect")
                c["scan-%s-c%d-%s" % ("f16" if half else "f32", C, mode)] = Case(
                    entry, 3, C, _lv(BASE, half=half, logit=mode == "z", half_reg=half and entry == "detect_raw"),
                    hot=0.2 if entry == "detect_raw" else 0.08)
    for mode in "pz":       # RN_SCAN_T / RN_SCAN_NT are read once per process
        lv = _lv(BASE, half=True, logit=mode == "z")
        c["scan-f16-c80-noT-" + mode] = Case("detect", 3, 80, lv, env=(("RN_SCAN_T", "0"),), process=True)
        c["scan-f16-c80-noNT-" + mode] = Case("detect", 3, 80, lv, env=(("RN_SCAN_NT", "0"),), process=True)
    c["scan-mixed-storage-c16"] = Case("detect", 3, 16, (BASE[0], replace(BASE[1], half=True), BASE[2]))
    c["scan-mixed-logit-c16"] = Case("detect", 3, 16, (BASE[0], BASE[1], replace(BASE[2], logit=True)))
    lds = (("RN_SCAN_LDS", "1"),)
    c["scan-lds-f32-c4-p"] = Case("detect", 3, 4, BASE, env=lds)
    c["scan-lds-f32-c80-z"] = Case("detect", 3, 80, _lv(BASE, logit=True), env=lds)
    c["scan-lds-f32-c92-p"] = Case("detect", 3, 92, BASE, env=lds)
    c["scan-lds-f32-c92-z"] = Case("detect", 3, 92, _lv(BASE, logit=True), env=lds)
    c["scan-lds-f32-c96-declined"] = Case("detect", 3, 96, BASE, env=lds)
    c["scan-lds-f16-c80-p"] = Case("detect", 3, 80, _lv(BASE, half=True), env=lds)
    c["scan-lds-f16-c80-z"] = Case("detect", 3, 80, _lv(BASE, half=True, logit=True), env=lds)
    c["scan-no-lds-wins"] = Case("detect", 3, 4, BASE, env=lds + (("RN_SCAN_NO_LDS", "1"),))
    # ---- adversarial logit rows, once per scan family (expected: the stand-alone sigmoid kernel + the probability-mode call)
    adv = (Level(1, 70, 1, logit=True),)
    c["adv-T"] = Case("detect", 2, 80, _lv(adv, half=True), score_thr=0.0, recipe="adversarial")
    c["adv-Q-f32"] = Case("detect", 2, 36, adv, score_thr=0.0, recipe="adversarial")
    c["adv-Q-f16"] = Case("detect", 2, 40, _lv(adv, half=True), score_thr=0.0, recipe="adversarial")
    c["adv-GENERIC-f32"] = Case("detect", 2, 5, adv, score_thr=0.0, recipe="adversarial")
    c["adv-GENERIC-f16"] = Case("detect", 2, 12, _lv(adv, half=True), score_thr=0.0, recipe="adversarial")
    c["adv-LDS"] = Case("detect", 2, 92, adv, score_thr=0.0, recipe="adversarial", env=lds)
    c["adv-mixed"] = Case("detect", 2, 16, (adv[0], replace(adv[0], half=True)), score_thr=0.0, recipe="adversarial")
    # ---- offsets and emit: 1140 waves = 2 offsets blocks; 9507 waves = 10 blocks, begin > 8 * 1024, the emit grid capped
    for tag, g in (("off2", 90), ("off10", 260)):
        for mode, cap in (("hist", "rows"), ("strided", "rows/16")):
            c["det-%s-%s" % (tag, mode)] = Case("detect", 1, 4, (Level(g, g, 9),), cap=cap, recipe="sparse", hot=0.01)
    c["det-global-scatter"] = Case("detect", 3, 2800, BASE, max_per_class=8, hot=0.3)
    c["det-gather-second-pass"] = Case("detect", 3, 200, BASE, hot=0.3)
    c["det-empty"] = Case("detect", 3, 4, BASE, hot=0.0)
    c["det-overcap-hist"] = Case("detect", 3, 4, BASE, cap=60, hot=0.5)
    c["det-overcap-strided"] = Case("detect", 3, 4, BASE, cap=40, hot=0.5)
    # ---- sort, NMS and gather through rn_nms_classwise
    c["nms-sort-lengths"] = Case("nms_classwise", 1, 32, recipe="sort_lengths")
    for m in (1, 5, 64, 1000, 1024):
        c["nms-cap-%d" % m] = Case("nms_classwise", 1, 2, max_per_class=m, recipe="lattice")
    c["nms-kept-counts"] = Case("nms_classwise", 1, 4, recipe="kept_counts")
    c["nms-disjoint"] = Case("nms_classwise", 2, 2, recipe="disjoint")
    c["nms-identical"] = Case("nms_classwise", 1, 1, recipe="identical")
    c["nms-chains"] = Case("nms_classwise", 1, 2, recipe="chains")
    for t in (0.5, 0.3, 0.75, 0.0, 1.0):
        c["nms-near-thr-%g" % t] = Case("nms_classwise", 1, 0, iou_thr=t, recipe="near_thr")     # C = the number of pairs
    c["nms-degenerate"] = Case("nms_classwise", 1, 3, recipe="degenerate")
    c["nms-ties"] = Case("nms_classwise", 2, 3, recipe="ties")
    c["nms-many"] = Case("nms_classwise", 2, 3, recipe="many")
    out = {}
    for name, case in c.items():
        if case.recipe == "near_thr":
            case = replace(case, C=len(near_thr_pairs(case.iou_thr)[0]))
        out[name] = replace(case, seed=zlib.crc32(name.encode()) & 0xFFFF)
    return out


SORT_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 8191, 8192, 8193, 16385)
NMS_MANY = 270000


# ------------------------------------------------------------------ inputs
def rows_per_image(case):
    return sum(l.rows for l in case.levels)


def capacity(case):
    if case.entry == "nms_classwise":
        return max(int(make_case_cached(case)["count"]), 1)
    total = case.n * rows_per_image(case)
    return total if case.cap == "rows" else total // 16 if case.cap == "rows/16" else int(case.cap)


def _cluster_boxes(rng, shape, clusters=3, smallest=0.1):
    """boxes around a few centres, so that suppression happens"""
    centres = rng.uniform(0.2, 0.8, (clusters, 2))
    ctr = centres[rng.integers(0, clusters, shape)] + rng.normal(0, 0.02, shape + (2,))
    sz = rng.uniform(smallest, 0.3, shape + (2,))
    return np.concatenate([ctr - sz / 2, ctr + sz / 2], -1).astype(f32)


def _anchor_sizes(A):
    k = np.arange(A)
    return np.stack([0.08 + 0.03 * (k % 3), 0.06 + 0.02 * (k // 3)], -1).astype(f32)


def _hot_level(case, lv, rng):
    """[n, rows, C] in the storage type: cold rows below the threshold, hot rows with one class above it -- a third of them
    with the same value in a second class (the first index must win)."""
    n, C = case.n, case.C
    hot_classes = np.array(case.hot_classes or sorted({0, C // 2, C - 1}))
    if lv.logit:
        v = -rng.integers(1, 513, (n, lv.rows, C)).astype(np.float64) / 64
    else:
        v = rng.integers(0, 461, (n, lv.rows, C)).astype(np.float64) / 1024
    sel = np.argwhere(rng.uniform(size=(n, lv.rows)) < case.hot)
    for j, (i, r) in enumerate(sel):
        val = rng.integers(1, 513) / 64 if lv.logit else (513 + rng.integers(0, 500)) / 1024
        cls = hot_classes[rng.integers(0, len(hot_classes))]
        v[i, r, cls] = val
        if j % 3 == 0:
            v[i, r, hot_classes[rng.integers(0, len(hot_classes))]] = val
    return v.astype(np.float16 if lv.half else f32)


def adversarial_rows(C, half):
    """Rows of logits [R, C] (float64 holding values exact in the storage type) that strain the max-logit shortcut: the pairs
    sit at the ends of the row, in neighbouring chunks and in the last chunk."""
    st = np.float16 if half else f32
    pred = lambda x: float(np.nextafter(st(x), st(-np.inf)))
    places = [(0, C - 1), (1, C // 2), (C // 2, C - 1), (C - 2, C - 1)]
    rows = []

    def row(fill, *items):
        for lo, hi in places:
            r = np.full(C, float(st(fill)))
            idx = [lo, hi] + [k for k in (2, C // 3, C - 3) if k not in (lo, hi) and 0 <= k < C]
            for k, val in zip(idx, items):
                r[k] = float(st(val))
            rows.append(r)
    row(-3.0, 20.0, 17.0, 30.0, 18.0)             # saturated: the first index wins whatever the logits
    row(-3.0, 2.5, 2.5)                           # equal logits
    row(-1.0, pred(3.0), 3.0)                     # one ulp apart in the storage type, the smaller one first
    row(-1.0, 3.0, pred(3.0))
    row(-80.0, -80.0, -80.0)                      # a row of -80
    row(-3.0, 16.6, 16.7)
    row(-3.0, 16.7, 16.6)
    row(-3.0, pred(12.0), 12.0)
    row(0.0, pred(pred(0.5)), pred(0.5), 0.5)     # adjacent values around a binade edge
    row(5.99, 6.0, pred(6.0), 5.999)              # the whole row close to the maximum
    return np.array(rows)


def _adversarial_level(case, lv, k):
    rows = adversarial_rows(case.C, lv.half)
    idx = (np.arange(case.n * lv.rows) * 7 + 3 * k) % len(rows)      # every row more than once, out of step with the waves
    return rows[idx].reshape(case.n, lv.rows, case.C).astype(np.float16 if lv.half else f32)


def _disjoint_boxes(count):
    """count tiny boxes on a lattice, none touching another"""
    k = np.arange(count)
    y, x = (k // 64).astype(f32) / f32(64), (k % 64).astype(f32) / f32(64)
    return np.stack([y, x, y + f32(0.01), x + f32(0.01)], -1).astype(f32)


def near_thr_pairs(thr):
    """-> (A [P, 4], B [P, 4]): B lies inside A, so IoU = area B / area A.  Family 1: B = A's lower half, IoU exactly 0.5, and
    its neighbours; family 2: IoU = 1/3 (1 +- k ulp); family 3: the same around the case's own threshold (B = [0, 0, s, thr s]
    with s = 1 has IoU == thr exactly)."""
    A, B = [], []
    for s in (1.0, 0.5, 0.75, 3.0, 1.0 / 3.0, 0.1, 1e-3, 100.7):
        s = f32(s)
        for frac in (f32(0.5), f32(1.0) / f32(3.0), f32(thr)):
            t0 = f32(s * frac)
            for k in range(-8, 9):
                t = t0
                for _ in range(abs(k)):
                    t = np.nextafter(t, f32(np.inf) if k > 0 else f32(-np.inf))
                if t <= 0:
                    continue
                A.append([0, 0, s, s])
                B.append([0, 0, s, t])
    if thr == 0.0:      # touching and barely overlapping boxes: IoU > 0 iff the intersection is positive
        for d in (0.0, 1e-7, -1e-7, 1e-30):
            A.append([0, 0, 1, 1])
            B.append([0, f32(1.0) - f32(d), 1, 2])
    return np.array(A, f32), np.array(B, f32)


def _nms_inputs(case, rng):
    """-> boxes [K, 4], scores [K], class_ids [K], image_ids [K]"""
    r = case.recipe
    n, C = case.n, case.C
    if r == "sort_lengths":      # class 2 k holds SORT_LENGTHS[k] candidates (odd classes stay empty), in shuffled order
        cls = rng.permutation(np.repeat(np.arange(0, 32, 2), SORT_LENGTHS))
        K = len(cls)
        return _cluster_boxes(rng, (K,), 40), (rng.integers(1, 4096, K) / 4096).astype(f32), cls, np.zeros(K, np.int64)
    if r == "lattice":           # ~1500 per class on disjoint cells, a fifth of them near-copies of another one
        K = 3000
        b = _disjoint_boxes(K)
        dup = rng.uniform(size=K) < 0.2
        src = rng.integers(0, K, K)
        b[dup] = b[src[dup]] + f32(2 ** -11)
        cls = np.arange(K) % 2
        cls[dup] = cls[src[dup]]
        return b, rng.permutation((np.arange(K) + 1) / f32(4096)).astype(f32), cls, np.zeros(K, np.int64)
    if r == "kept_counts":       # class 0 / 1 / 2: the first 64 by score keep exactly 15 / 16 / 17, more follow; class 3: > 64 kept
        bs, cs = [], []
        for c_, k in enumerate((15, 16, 17)):
            cell = _disjoint_boxes(128)
            i = np.arange(64 + 40)
            pick = np.where(i < k, i, np.where(i < 64, i % k, np.where(i % 2 == 0, 20 + i // 2, i % k)))
            bs.append(cell[pick]); cs.append(np.full(len(i), c_))
        bs.append(_disjoint_boxes(140)); cs.append(np.full(140, 3))
        b, cls = np.concatenate(bs), np.concatenate(cs)
        K = len(cls)
        return b, (f32(1) - np.arange(K).astype(f32) / f32(4096)).astype(f32), cls, np.zeros(K, np.int64)
    if r == "disjoint":
        K = 200
        return _disjoint_boxes(K), rng.uniform(-1, 1, K).astype(f32), np.arange(K) % C, (np.arange(K) // 2) % n
    if r == "identical":
        K = 300
        return np.tile(np.array([[0.1, 0.2, 0.5, 0.7]], f32), (K, 1)), rng.permutation(np.arange(K) / f32(512)).astype(f32), \
            np.zeros(K, np.int64), np.zeros(K, np.int64)
    if r == "chains":            # box k = box 0 shifted by 0.3 k: k kills k + 1 (IoU 0.54), spares k + 2 (IoU 0.25); dead boxes kill nothing
        K = 200
        x = (np.arange(K) * f32(0.3)).astype(f32)
        b = np.stack([np.zeros(K, f32), x, np.ones(K, f32), x + f32(1)], -1).astype(f32)
        s = (f32(1) - np.arange(K).astype(f32) / f32(256)).astype(f32)
        b, s = np.concatenate([b[:40], b]), np.concatenate([s[:40], s])     # class 0: inside one batch; class 1: across batches
        return b, s, np.concatenate([np.zeros(40, np.int64), np.ones(K, np.int64)]), np.zeros(K + 40, np.int64)
    if r == "near_thr":          # pair p is class p: A (higher score) then B
        A, B = near_thr_pairs(case.iou_thr)
        P = len(A)
        b = np.stack([A, B], 1).reshape(-1, 4)
        return b, np.tile(np.array([0.9, 0.8], f32), P), np.repeat(np.arange(P), 2), np.zeros(2 * P, np.int64)
    if r == "degenerate":
        tiny = f32(1e-20)
        b = np.array([[0.3, 0.3, 0.3, 0.3], [0.3, 0.3, 0.3, 0.3],            # zero area: never suppressed, suppress nothing
                      [0.1, 0.1, 0.4, 0.4], [0.4, 0.4, 0.1, 0.1],            # inverted corners: the same box
                      [0.4, 0.1, 0.1, 0.4], [0.12, 0.1, 0.4, 0.4],
                      [0, 0, tiny, tiny], [0, 0, tiny, tiny],                # area 1e-40, a float32 subnormal: positive, IoU 1
                      [0, 0, tiny, 1], [0, 0, tiny, 0.7], [0, 0, tiny, 0.4],
                      [0.5, 0.5, 0.5, 0.9], [0.5, 0.5, 0.9, 0.5]], f32)     # zero height / width
        b = np.tile(b, (3, 1))
        K = len(b)
        return b, (f32(1) - np.arange(K).astype(f32) / f32(64)).astype(f32), np.arange(K) // 13, np.zeros(K, np.int64)
    if r == "ties":              # many equal scores, negative scores, and -0.0 in front of +0.0
        K = 600
        b = _cluster_boxes(rng, (K,), 6)
        s = rng.choice(np.array([0.75, 0.5, -0.25, -1.5, 0.0, -0.0], f32), K).astype(f32)
        cls, img = rng.integers(0, C, K), rng.integers(0, n, K)
        for k in range(0, 40, 2):    # overlapping pairs in one segment: -0.0 at the lower index, +0.0 behind it
            b[k] = b[k + 1] = _disjoint_boxes(64)[k]
            s[k], s[k + 1] = f32(-0.0), f32(0.0)
            cls[k] = cls[k + 1] = 0
            img[k] = img[k + 1] = 0
        return b, s, cls, img
    if r == "many":
        K = NMS_MANY
        return _cluster_boxes(rng, (K,), 24), rng.uniform(0, 1, K).astype(f32), rng.integers(0, C, K), rng.integers(0, n, K)
    raise ValueError(r)


def make_case(case):
    """Deterministic inputs.  Detection entries: probs [n, rows, C] per level in the storage type, and boxes [n, rows, 4]
    (float32) or regs [n, h, w, A, 4] + anchors [A, 2] per level.  nms_classwise: boxes, scores, class_ids, image_ids, count."""
    rng = np.random.default_rng(case.seed)
    if case.entry == "nms_classwise":
        b, s, cls, img = _nms_inputs(case, rng)
        return {"boxes": np.ascontiguousarray(b, f32), "scores": np.ascontiguousarray(s, f32), "class_ids": cls.astype(np.int32),
                "image_ids": img.astype(np.int32), "count": len(s)}
    out = {"probs": [], "boxes": [], "regs": [], "anchors": []}
    for k, lv in enumerate(case.levels):
        if case.recipe == "adversarial":
            out["probs"].append(_adversarial_level(case, lv, k))
        else:
            out["probs"].append(_hot_level(case, lv, rng))
        if case.entry == "detect_raw":
            reg = rng.integers(-40, 41, (case.n, lv.h, lv.w, lv.A, 4)) / 128.0      # exact in fp16
            out["regs"].append(reg.astype(np.float16 if lv.half_reg else f32))
            out["anchors"].append(_anchor_sizes(lv.A))
        elif case.recipe == "adversarial":
            out["boxes"].append(np.tile(_disjoint_boxes(lv.rows)[None], (case.n, 1, 1)))
        else:
            out["boxes"].append(_cluster_boxes(rng, (case.n, lv.rows), 40) if case.recipe == "sparse" else
                                _cluster_boxes(rng, (case.n, lv.rows), 2, 0.22))
    return out


@functools.lru_cache(maxsize=None)
def make_case_cached(case):
    return make_case(case)


# ------------------------------------------------------------------ the host-side rules
def _align(x, a=256):
    return (x + a - 1) // a * a


def workspace_ref(n, C, rows, waves, cap, max_per_class):
    """Every array of the workspace starts on a 256-byte boundary: per row score and class (4 + 4), per wave count, offset
    (4 + 4) and mask (8), per candidate key (8), sorted value (4), box (16), score, class, image (4 each), anchor (8), per
    segment count, fill, start (+ 1 entry), keep, offset (4 each) and max_per_class kept indices (4 each)."""
    nrows, nw, nseg = n * rows, n * waves, n * C
    sizes = [nrows * 4] * 2 + [nw * 4] * 2 + [nw * 8] + [cap * 8, cap * 4, cap * 16, cap * 4, cap * 4, cap * 4, cap * 8] + \
        [nseg * 4] * 2 + [(nseg + 1) * 4] + [nseg * 4] * 2 + [nseg * max_per_class * 4]
    return sum(_align(s) for s in sizes)


def plan_ref(case):
    """-> dict of what rn_detect_plan reports, plus "reason" where the catch-all scan kernel is taken."""
    n, C = case.n, case.C
    nseg = n * C
    seg = "LDS_SCATTER" if nseg <= 8192 else "GLOBAL_SCATTER"
    cap = capacity(case)
    p = dict(scan=None, half=0, logit=0, q=0, lds_per_wave=0, scan_grid=0, offsets_blocks=0, emit=None, emit_grid=0, emit_lds=0,
             segments=seg, nseg=nseg, reason=None)
    if case.entry == "nms_classwise":        # sized as one level of 64 rows: no scan, offsets or emit pass runs
        p["workspace"] = workspace_ref(n, C, 64, 1, cap, case.max_per_class)
        return p
    env = dict(case.env)
    waves = sum((l.rows + 63) // 64 for l in case.levels)
    rows = rows_per_image(case)
    nw = n * waves
    p["workspace"] = workspace_ref(n, C, rows, waves, cap, case.max_per_class)
    p["scan_grid"] = (nw + 3) // 4                       # one wave per 64 rows of a level, four waves per block
    p["offsets_blocks"] = (nw + 1023) // 1024
    hist = nseg <= 8192 and cap * 8 >= n * rows          # a capacity of an eighth of the rows or more: counts through LDS
    p["emit"], p["emit_lds"] = ("HIST", nseg * 4) if hist else ("STRIDED", 0)
    p["emit_grid"] = min(p["scan_grid"], 2048)
    # the scan: 16-byte chunks of V = 4 (fp32) or 8 (fp16) classes
    first = case.levels[0]
    uniform = all(l.half == first.half and l.logit == first.logit for l in case.levels)
    V = 8 if first.half else 4
    q = (C // V + 3) // 4 if C % V == 0 else 0           # chunks per lane when four lanes share a row
    lds_bytes = [64 * ((C // (8 if l.half else 4)) | 1) * 16 for l in case.levels]      # 64 rows, odd stride in chunks
    lds = "RN_SCAN_LDS" in env and "RN_SCAN_NO_LDS" not in env and \
        all(C % (8 if l.half else 4) == 0 for l in case.levels) and max(lds_bytes) <= 24 * 1024
    if lds:
        p["scan"], p["lds_per_wave"] = "LDS", max(lds_bytes)
    elif uniform and first.half and C == 80 and env.get("RN_SCAN_T") != "0":
        p["scan"] = "T_PLAIN" if env.get("RN_SCAN_NT") == "0" else "T"
    elif uniform and 1 <= q <= 8:
        p["scan"], p["half"], p["logit"], p["q"] = "Q", int(first.half), int(first.logit), q
    else:
        p["scan"] = "GENERIC"
        p["reason"] = "mixed" if not uniform else "remainder" if C % V else "q>8"
    return p


PLAN_FIELDS = ("scan", "half", "logit", "q", "lds_per_wave", "scan_grid", "offsets_blocks", "emit", "emit_grid", "emit_lds", "segments", "nseg")


def plan_row(p):
    return tuple(p[k] for k in PLAN_FIELDS)


# ------------------------------------------------------------------ the oracle
def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def level_scores(lv, prob):
    """float32 class scores of one level as the pipeline defines them: the stored value, or the sigmoid of the stored logit
    (fp64, rounded once)"""
    v = prob.astype(np.float64)
    return (sigmoid64(v) if lv.logit else v).astype(f32)


def boxes_decode_thr(classifications, regressions, thr):
    """utils_ref.boxes_decode with the threshold as a parameter, also returning the rows it kept"""
    classifications = np.asarray(classifications, dtype=f32)
    cmax = classifications.max(-1)
    ids = classifications.argmax(-1).astype(np.int64)
    fg = cmax > f32(thr)
    return utils_ref.BoxesDecoded(np.asarray(regressions, dtype=f32)[fg], cmax[fg], ids[fg]), np.flatnonzero(fg)


def decode_boxes_ref(inputs, case):
    """entry detect_raw: the oracle's decoded boxes per level [n, rows, 4]"""
    return [utils_ref.regression_postprocess(r.astype(f32), a).reshape(case.n, -1, 4) for r, a in zip(inputs["regs"], inputs["anchors"])]


def candidates_ref(case, inputs, boxes=None):
    """-> boxes [K, 4], scores, class, image, anchor (flat row inside the image, levels concatenated) in the emit order: image,
    level, row.  boxes: per level [n, rows, 4] (default: the inputs' own, or the oracle's decode of the raw regressions)."""
    if boxes is None:
        boxes = inputs["boxes"] if case.entry != "detect_raw" else decode_boxes_ref(inputs, case)
    scores = [level_scores(lv, p) for lv, p in zip(case.levels, inputs["probs"])]
    ob, os_, oc, oi, oa = [], [], [], [], []
    for i in range(case.n):
        parts, off = [], 0
        for lv, s, b in zip(case.levels, scores, boxes):
            dec, rows = boxes_decode_thr(s[i], b[i], case.score_thr)
            parts.append(dec)
            oa.append(rows + off)
            off += lv.rows
        m = utils_ref.merge_boxes_decoded(parts)
        ob.append(m.boxes); os_.append(m.scores); oc.append(m.class_ids); oi.append(np.full(len(m.scores), i, np.int64))
    return np.concatenate(ob).reshape(-1, 4), np.concatenate(os_), np.concatenate(oc), np.concatenate(oi), np.concatenate(oa)


def _segments(n, C, cls, img):
    """-> (order, bounds): candidates grouped by segment image * C + class, in index order inside a segment"""
    seg = img.astype(np.int64) * C + cls.astype(np.int64)
    order = np.argsort(seg, kind="stable")
    bounds = np.searchsorted(seg[order], np.arange(n * C + 1))
    return order, bounds


def nms_ref(case, boxes, scores, cls, img, index, nms=utils_ref.nms_indices_vectorised):
    """Class-wise NMS per image over candidate arrays -> dict of the survivors' arrays in (image, class, score descending,
    index ascending) order, `counts`, and per segment (length, sorted positions of the kept)."""
    n, C = case.n, case.C
    order, bounds = _segments(n, C, cls, img)
    keep_all, segs = [], []
    per_image = np.zeros(n, np.int64)
    for k in range(n * C):
        idx = order[bounds[k]:bounds[k + 1]]
        if len(idx) == 0:
            segs.append((0, np.zeros(0, np.int64)))
            continue
        kept = nms(boxes[idx], scores[idx], case.max_per_class, case.iou_thr)
        rank = np.empty(len(idx), np.int64)
        rank[np.argsort(-scores[idx].astype(np.float64), kind="stable")] = np.arange(len(idx))
        segs.append((len(idx), rank[kept]))
        keep_all.append(idx[kept])
        per_image[k // C] += len(kept)
    keep = np.concatenate(keep_all) if keep_all else np.zeros(0, np.int64)
    counts = np.concatenate([[len(scores), len(keep)], per_image]).astype(np.int64)
    return {"boxes": boxes[keep], "scores": scores[keep], "class": cls[keep].astype(np.int32), "image": img[keep].astype(np.int32),
            "anchor": index[keep].astype(np.int64), "counts": counts, "segments": segs}


def run_ref(case, inputs, boxes=None, nms=utils_ref.nms_indices_vectorised):
    """The oracle's result of the case (see nms_ref).  entry boxes_decode: the candidates themselves, counts[1] = counts[0]."""
    if case.entry == "nms_classwise":
        K = inputs["count"]
        return nms_ref(case, inputs["boxes"], inputs["scores"], inputs["class_ids"].astype(np.int64), inputs["image_ids"].astype(np.int64),
                       np.arange(K), nms)
    b, s, c, i, a = candidates_ref(case, inputs, boxes)
    if case.entry == "boxes_decode":
        return {"boxes": b, "scores": s, "class": c.astype(np.int32), "image": i.astype(np.int32), "anchor": a.astype(np.int64),
                "counts": np.array([len(s), len(s)] + [0] * case.n, np.int64), "segments": []}
    return nms_ref(case, b, s, c, i, a, nms)


@functools.lru_cache(maxsize=None)
def run_ref_cached(case):
    return run_ref(case, make_case_cached(case))


# ------------------------------------------------------------------ data-dependent branches
def device_branches(case, inputs, ref=None):
    """The labels of the branches the device code takes on this case, from the reference alone."""
    ref = ref or run_ref(case, inputs)
    labels = set()
    nseg = case.n * case.C
    ncand = min(int(ref["counts"][0]), capacity(case))
    if case.entry == "boxes_decode":
        return labels
    if nseg <= 8192:       # 256 blocks share the candidates: fewer than 4 * 256 each -> one global atomic per candidate
        labels.add("scatter:few" if (ncand + 255) // 256 < 1024 else "scatter:many")
    else:
        labels.add("scatter:global")
    for m, kept_pos in ref["segments"]:
        labels.add("sort:%d" % m)
        if m:
            labels.add("sort:lds" if m <= 8192 else "sort:global")
            labels.add("sort:p2=%d" % (1 << max(m - 1, 0).bit_length()))
        nk = len(kept_pos)
        if nk == case.max_per_class and m:
            last = int(kept_pos.max())
            labels.add("cap:%d" % case.max_per_class)
            if last % 64 != 63 and last != m - 1:
                labels.add("cap:mid-batch")
            batches = last // 64 + 1
        else:
            batches = (m + 63) // 64
        labels.add("nms:batches=%s" % (batches if batches <= 2 else ">2"))
        for b in range(1, batches):      # the kept list a later batch is tested against, four boxes per step with clamped indices
            nkb = int((kept_pos < 64 * b).sum())
            labels.add("kept:%d" % nkb if nkb in (15, 16, 17) else "kept:>64" if nkb > 64 else "kept:other")
        if nk:      # a later batch that adds nothing: every candidate of it dies against the kept list (the early exit)
            hit = np.zeros(max(batches, 1), bool)
            hit[kept_pos // 64] = True
            if batches > 1 and not hit[1:].all():
                labels.add("nms:early-exit")
        if nk == 1 and m > 64:
            labels.add("nms:identical")
    labels.add("gather:passes=%d" % max((nseg - 1 + 511) // 512, 1))
    return labels


# ------------------------------------------------------------------ the two device predicates in float32
def _norm(b):
    b = np.asarray(b, f32)
    ymin, ymax = np.minimum(b[..., 0], b[..., 2]), np.maximum(b[..., 0], b[..., 2])
    xmin, xmax = np.minimum(b[..., 1], b[..., 3]), np.maximum(b[..., 1], b[..., 3])
    area = ((ymax - ymin).astype(f32) * (xmax - xmin).astype(f32)).astype(f32)
    return ymin, xmin, ymax, xmax, area


def inter_union_f32(bi, bj):
    """-> (inter, u, valid): the float32 intermediate values both predicates start from"""
    yi0, xi0, yi1, xi1, ai = _norm(bi)
    yj0, xj0, yj1, xj1, aj = _norm(bj)
    iy = np.maximum((np.minimum(yi1, yj1) - np.maximum(yi0, yj0)).astype(f32), f32(0))
    ix = np.maximum((np.minimum(xi1, xj1) - np.maximum(xi0, xj0)).astype(f32), f32(0))
    inter = (iy * ix).astype(f32)
    u = ((ai + aj).astype(f32) - inter).astype(f32)
    return inter, u, (ai > 0) & (aj > 0)


def decide_f32(inter, u, thr):
    """`suppresses` after the area test: inter / u > thr"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(inter, f32) / np.asarray(u, f32)).astype(f32) > f32(thr)


def decide_fast_f32(inter, u, thr):
    """`suppresses_fast` after the area test: inter > thr u; the exact quotient inside the 2^-20 band, and always for a
    threshold that is zero or subnormal (inter > 0 can hold where inter / u rounds to zero)"""
    inter, u = np.asarray(inter, f32), np.asarray(u, f32)
    t = (f32(thr) * u).astype(f32)
    r = inter > t
    band = (np.abs((inter - t).astype(f32)) <= (BAND * np.abs(t)).astype(f32)) | (f32(thr) < FLT_MIN)
    return np.where(band, decide_f32(inter, u, thr), r)


def suppresses_f32(bi, bj, thr):
    inter, u, valid = inter_union_f32(bi, bj)
    return valid & decide_f32(inter, u, thr)


def suppresses_fast_f32(bi, bj, thr):
    inter, u, valid = inter_union_f32(bi, bj)
    return valid & decide_fast_f32(inter, u, thr)


def lds_row_of_chunk(g, cv):
    """the LDS scan's row of chunk g: int((g + 0.5f) * (1 / CV)) in float32"""
    inv = f32(1) / f32(cv)
    return (((np.asarray(g).astype(f32) + f32(0.5)).astype(f32)) * inv).astype(f32).astype(np.int64)


CASES = _build_cases()
