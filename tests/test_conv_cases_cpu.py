"""The case table of tests/conv_ref.py without a GPU: every call of every case takes the branch of the convolution dispatch it
was picked for (read off the host-only rn_conv2d_plan: the library loads without a device, and the query runs the very
functions rn_conv2d_fwd / _fwd_stats / _dgrad / _wgrad / _bwd launch from, stopped before the first launch, under the same
environment switches), and the table as a whole reaches every branch listed in COVER.  A planner change that moves a case off
its branch fails here and says: pick another shape for that branch.  Further tests: the workspace functions return exactly
what the planned path takes, the once-per-process switches (each in a fresh process), the refusals, and the reference itself.

The rows are conv_ref.row_of's:
  fp32:     ('fp32', tile shape 0..3, load variant, nsplit, K tiles per split-K range | pixels per weight-gradient split, blocks)
            + (phase pseudo-segments, those without taps) for the data gradient
            + (a split runs in windows, straight into dw, the row reduction) for the weight gradient
  x3_1x1:   ('x3_1x1', m-tile rows) + (slabs, the row reduction) for the weight gradient
  x3_patch: ('x3_patch', m-tile rows, samples per piece, patch-matrix bytes) + likewise
  stem: ('stem', blocks);  direct_grouped: ('direct_grouped',) + (the row reduction,);  fwd_stats: + (rows per sample,)
  bwd:      ('merged_bwd', blocks, dgrad row, wgrad row) or ('two_calls', why, dgrad row, wgrad row)
  ('refused',) + the row the forward call would take: rn_conv2d_stats_rows returns 0, the call RN_EUNSUPPORTED"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4

EXPECT = {
    "f32-cfg0-scalar": {
        "fwd": ('fp32', 0, 'scalar', 1, 0, 3),
        "dgrad": ('fp32', 0, 'scalar', 1, 0, 3, 0, 0),
        "wgrad": ('fp32', 0, 'scalar', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg0-vec4": {
        "fwd": ('fp32', 0, 'vec4', 1, 0, 3),
        "dgrad": ('fp32', 0, 'vec4', 1, 0, 3, 0, 0),
        "wgrad": ('fp32', 0, 'vec4', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg0-tap": {
        "fwd": ('fp32', 0, 'vec4_tap', 1, 0, 3),
        "dgrad": ('fp32', 0, 'vec4_tap', 4, 5, 12, 0, 0),
        "wgrad": ('fp32', 0, 'vec4', 5, 64, 15, 0, 0, 'launched'),
    },
    "f32-cfg1-scalar": {
        "fwd": ('fp32', 1, 'scalar', 1, 0, 3),
        "dgrad": ('fp32', 1, 'scalar', 1, 0, 3, 0, 0),
        "wgrad": ('fp32', 1, 'scalar', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg1-vec4": {
        "fwd": ('fp32', 1, 'vec4', 1, 0, 3),
        "dgrad": ('fp32', 1, 'vec4', 1, 0, 3, 0, 0),
        "wgrad": ('fp32', 1, 'vec4', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg1-tap": {
        "fwd": ('fp32', 1, 'vec4_tap', 1, 0, 3),
        "dgrad": ('fp32', 1, 'vec4_tap', 4, 5, 12, 0, 0),
        "wgrad": ('fp32', 1, 'vec4', 5, 64, 15, 0, 0, 'launched'),
    },
    "f32-cfg2-scalar": {
        "fwd": ('fp32', 2, 'scalar', 1, 0, 5),
        "dgrad": ('fp32', 2, 'scalar', 1, 0, 5, 0, 0),
        "wgrad": ('fp32', 2, 'scalar', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg3-scalar": {
        "fwd": ('fp32', 3, 'scalar', 1, 0, 3),
        "dgrad": ('fp32', 3, 'scalar', 1, 0, 3, 0, 0),
        "wgrad": ('fp32', 3, 'scalar', 5, 64, 5, 0, 0, 'launched'),
    },
    "f32-cfg3-tap": {
        "fwd": ('fp32', 3, 'vec4_tap', 1, 0, 6),
        "dgrad": ('fp32', 3, 'vec4_tap', 4, 5, 12, 0, 0),
        "wgrad": ('fp32', 3, 'vec4', 5, 64, 30, 0, 0, 'launched'),
    },
    "dense-cfg0": {
        "fwd": ('fp32', 0, 'vec4', 1, 0, 200),
        "dgrad": ('fp32', 2, 'vec4_tap', 8, 36, 400, 0, 0),
        "wgrad": ('fp32', 0, 'vec4', 50, 64, 400, 0, 0, 'launched'),
    },
    "dense-cfg1-dgrad-cfg3": {
        "fwd": ('fp32', 1, 'vec4', 1, 0, 1200),
        "dgrad": ('fp32', 3, 'vec4_tap', 1, 0, 150, 0, 0),
        "wgrad": ('fp32', 0, 'vec4', 150, 128, 600, 0, 0, 'launched'),
    },
    "group-w64": {
        "fwd": ('fp32', 2, 'vec4_tap', 1, 0, 4),
        "dgrad": ('fp32', 3, 'vec4_tap', 1, 0, 2, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 2, 64, 20, 0, 0, 'launched'),
    },
    "group-w96": {
        "fwd": ('fp32', 2, 'vec4', 1, 0, 8),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 8, 0, 0),
        "wgrad": ('fp32', 3, 'vec4', 2, 64, 72, 0, 0, 'launched'),
    },
    "splitk": {
        "fwd": ('fp32', 2, 'vec4', 6, 5, 6),
        "dgrad": ('fp32', 2, 'vec4_tap', 4, 5, 8, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 1, 64, 15, 0, 1, None),
    },
    "splitk-none": {
        "fwd": ('fp32', 2, 'vec4', 1, 0, 1),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 2, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 1, 64, 15, 0, 1, None),
    },
    "splitk-short": {
        "fwd": ('fp32', 2, 'vec4', 1, 0, 1),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 2, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 1, 64, 15, 0, 1, None),
    },
    "splitk-off": {
        "fwd": ('fp32', 2, 'vec4', 1, 0, 1),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 2, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 1, 64, 15, 0, 1, None),
    },
    "splitk-80-tiles": {
        "fwd": ('fp32', 2, 'vec4_tap', 4, 5, 320),
        "dgrad": ('fp32', 2, 'vec4_tap', 4, 5, 320, 0, 0),
    },
    "splitk-s2": {
        "fwd": ('fp32', 2, 'vec4_tap', 18, 4, 72),
        "dgrad": ('fp32', 2, 'vec4_tap', 18, 4, 144, 0, 0),
        "wgrad": ('fp32', 0, 'vec4', 1, 64, 36, 0, 1, None),
    },
    "pyramid5": {
        "fwd": ('fp32', 2, 'vec4_tap', 1, 0, 13),
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 13, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 13, 64, 117, 0, 0, 'launched'),
        "bwd": ('two_calls', 'shape', ('fp32', 2, 'vec4', 1, 0, 13, 0, 0), ('fp32', 2, 'vec4', 13, 64, 117, 0, 0, 'launched')),
    },
    "pyramid4-bwd": {
        "bwd": ('merged_bwd', 120, ('fp32', 2, 'vec4_tap', 1, 0, 12, 0, 0), ('fp32', 2, 'vec4', 12, 64, 108, 0, 0, 'launched')),
    },
    "pyramid4-bwd-vec": {
        "bwd": ('merged_bwd', 36, ('fp32', 2, 'vec4', 1, 0, 12, 0, 0), ('fp32', 1, 'vec4', 12, 64, 24, 0, 0, 'launched')),
    },
    "stem": {
        "fwd": ('stem', 2),
        "fwd_stats": ('stem', 2, 1),
    },
    "stem-off": {
        "fwd": ('fp32', 2, 'scalar', 1, 0, 7),
    },
    "x3-1x1-m128": {
        "fwd": ('x3_1x1', 128),
        "dgrad": ('x3_1x1', 64),
        "wgrad": ('x3_1x1', 64, 16, 'launched'),
        "fwd_stats": ('x3_1x1', 128, 40),
    },
    "x3-1x1-m64": {
        "fwd": ('x3_1x1', 64),
        "dgrad": ('x3_1x1', 64),
        "wgrad": ('x3_1x1', 64, 16, 'launched'),
        "bwd": ('two_calls', 'x3_1x1', ('x3_1x1', 64), ('x3_1x1', 64, 16, 'launched')),
        "fwd_stats": ('x3_1x1', 64, 16),
    },
    "x3-1x1-slice": {
        "fwd": ('x3_1x1', 64),
        "dgrad": ('x3_1x1', 64),
        "wgrad": ('x3_1x1', 64, 16, 'launched'),
    },
    "x3-1x1-mode0": {
        "fwd": ('fp32', 2, 'vec4_tap', 1, 0, 96),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 32, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 32, 64, 96, 0, 0, 'launched'),
    },
    "x3-1x1-under": {
        "fwd": ('fp32', 2, 'vec4_tap', 1, 0, 93),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 31, 0, 0),
        "wgrad": ('fp32', 2, 'vec4', 31, 64, 93, 0, 0, 'launched'),
    },
    "patch": {
        "fwd": ('x3_patch', 64, 2, 14017536),
        "dgrad": ('x3_patch', 64, 0, 14017536),
        "wgrad": ('x3_patch', 64, 0, 14017536, 8, 'launched'),
        "bwd": ('two_calls', 'x3_patch', ('x3_patch', 64, 0, 14017536), ('x3_patch', 64, 0, 14017536, 8, 'launched')),
    },
    "patch-none": {
        "fwd": ('fp32', 2, 'vec4_tap', 1, 0, 384),
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 376, 4, 0),
    },
    "patch-stats": {
        "fwd_stats": ('x3_patch', 64, 3, 14155776, 16),
    },
    "gconv-cg4": {
        "fwd": ('direct_grouped',),
        "dgrad": ('direct_grouped',),
        "wgrad": ('direct_grouped', 'launched'),
        "bwd": ('two_calls', 'direct_grouped', ('direct_grouped',), ('direct_grouped', 'launched')),
    },
    "gconv-cg8": {
        "fwd": ('direct_grouped',),
        "dgrad": ('direct_grouped',),
        "wgrad": ('direct_grouped', 'launched'),
    },
    "gconv-cg16": {
        "fwd": ('direct_grouped',),
        "dgrad": ('direct_grouped',),
        "wgrad": ('direct_grouped', 'launched'),
    },
    "gconv-cg32": {
        "fwd": ('direct_grouped',),
        "dgrad": ('direct_grouped',),
        "wgrad": ('direct_grouped', 'launched'),
    },
    "gconv-under": {
        "fwd": ('fp32', 3, 'vec4', 1, 0, 512),
        "dgrad": ('fp32', 3, 'vec4', 1, 0, 512, 0, 0),
        "wgrad": ('fp32', 3, 'vec4', 21, 96, 672, 0, 0, 'launched'),
    },
    "phase-3x3-odd": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 68, 4, 0),
        "bwd": ('two_calls', 'shape', ('fp32', 2, 'vec4', 1, 0, 68, 4, 0), ('fp32', 3, 'vec4', 18, 64, 36, 0, 0, 'launched')),
    },
    "phase-3x3-even": {
        "dgrad": ('fp32', 2, 'vec4_tap', 1, 0, 68, 4, 0),
    },
    "phase-1x1": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 68, 4, 3),
    },
    "phase-7x7": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 68, 4, 0),
    },
    "phase-h1": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 66, 2, 0),
    },
    "phase-2seg": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 72, 8, 0),
    },
    "phase-slice": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 68, 4, 0),
    },
    "phase-off-3x3": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 67, 0, 0),
    },
    "phase-off-1x1": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 67, 0, 0),
    },
    "phase-off-h1": {
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 66, 0, 0),
    },
    "slice-f32": {
        "fwd": ('fp32', 2, 'vec4', 1, 0, 5),
        "dgrad": ('fp32', 2, 'vec4', 1, 0, 5, 0, 0),
        "wgrad": ('fp32', 3, 'vec4', 5, 64, 5, 0, 0, 'launched'),
    },
    "wg-window-1k": {
        "wgrad": ('fp32', 3, 'vec4', 1, 1056, 2, 1, 1, None),
    },
    "wg-window-2k": {
        "wgrad": ('fp32', 3, 'vec4', 1, 2080, 2, 1, 1, None),
    },
    "wg-window-own": {
        "wgrad": ('fp32', 1, 'vec4', 2, 1056, 792, 1, 0, 'launched'),
    },
    "wg-acc-1": {
        "wgrad": ('fp32', 3, 'vec4', 1, 128, 2, 0, 0, 'launched'),
    },
    "wg-acc-n": {
        "wgrad": ('fp32', 3, 'vec4', 17, 64, 34, 0, 0, 'launched'),
    },
    "wg-defer": {
        "wgrad": ('fp32', 3, 'vec4', 17, 64, 34, 0, 0, 'deferred'),
        "bwd": ('merged_bwd', 51, ('fp32', 2, 'vec4', 1, 0, 17, 0, 0), ('fp32', 3, 'vec4', 17, 64, 34, 0, 0, 'deferred')),
    },
    "bwd-merged-tap": {
        "bwd": ('merged_bwd', 30, ('fp32', 2, 'vec4_tap', 1, 0, 5, 0, 0), ('fp32', 2, 'vec4', 5, 64, 25, 0, 0, 'launched')),
    },
    "bwd-merged-vec": {
        "bwd": ('merged_bwd', 10, ('fp32', 2, 'vec4', 1, 0, 5, 0, 0), ('fp32', 3, 'vec4', 5, 64, 5, 0, 0, 'launched')),
    },
    "bwd-scalar": {
        "bwd": ('two_calls', 'shape', ('fp32', 2, 'scalar', 1, 0, 5, 0, 0), ('fp32', 2, 'scalar', 5, 64, 5, 0, 0, 'launched')),
    },
    "stats-f32": {
        "fwd_stats": ('fp32', 2, 'vec4', 1, 0, 8, 4),
    },
    "stats-refused-ragged": {
        "fwd_stats": ('refused', 'fp32', 2, 'vec4', 1, 0, 5, 0),
    },
    "stats-refused-bias": {
        "fwd_stats": ('refused', 'fp32', 2, 'vec4', 1, 0, 8, 0),
    },
    "stats-refused-splitk": {
        "fwd_stats": ('refused', 'fp32', 2, 'vec4_tap', 9, 4, 9, 0),
    },
}
GEMM_EXPECT = {
    "gemm-kn": ('fp32', 2, 'vec4', 1, 0, 15, 5),
    "gemm-nk": ('fp32', 2, 'vec4', 1, 0, 15, 0, 0, 5),
    "gemm-kn-tap": ('fp32', 2, 'vec4_tap', 1, 0, 9, 3),
    "gemm-nk-x3": ('x3_1x1', 64, 5),
}

CFGS, LOADS = range(4), ("scalar", "vec4", "vec4_tap")
# every branch the table must reach, by the names _observe() gives them
COVER = (["fp32 %s cfg%d %s" % (op, c, l) for op in ("fwd", "dgrad") for c in CFGS for l in LOADS] +
         ["fp32 wgrad cfg%d %s" % (c, l) for c in CFGS for l in ("scalar", "vec4")] +
         ["cfg3 by group width", "cfg2 by group width"] + ["cfg%d by choose_cfg" % c for c in CFGS] +
         ["split-K %s" % op for op in ("fwd", "dgrad")] + ["split-K ranges of unequal length", "split-K with a K tail", "split-K stride 2", "split-K on 64 .. 95 tiles",
                                                          "split-K refused: NULL workspace", "split-K refused: one byte short", "split-K off"] +
         ["five segments down to 1 x 1 %s" % op for op in ("fwd", "dgrad")] + ["grouped fp32, groups wider than 64 %s" % op for op in ("fwd", "dgrad")] +
         ["batched fp32 product kn with a K tail", "batched fp32 product nk with a K tail", "batched fp32 product tap-uniform",
          "batched split-bf16 product"] +
         ["stem", "stem shape just off: fp32 scalar"] +
         ["x3_1x1 fwd m128", "x3_1x1 fwd m64"] + ["x3_1x1 %s" % op for op in ("dgrad", "wgrad")] +
         ["x3_1x1 %s channel slice" % op for op in ("fwd", "dgrad", "wgrad")] + ["1x1 in product mode 0 %s" % op for op in ("fwd", "dgrad", "wgrad")] +
         ["1x1 just under 96 tiles"] +
         ["x3_patch %s" % op for op in ("fwd", "dgrad", "wgrad")] + ["patch matrix declined without a workspace %s" % op for op in ("fwd", "dgrad")] +
         ["direct_grouped %s cg%d" % (op, cg) for op in ("fwd", "dgrad", "wgrad") for cg in (4, 8, 16, 32)] + ["grouped 3x3 just under the direct kernels' line"] +
         ["phases 3x3", "phases 1x1: three without taps", "phases 7x7", "phases odd map", "phases even map", "phases h == 1: two phases",
          "phases two segments", "phases channel slice", "RN_NO_PHASE_DGRAD 3x3", "RN_NO_PHASE_DGRAD 1x1", "RN_NO_PHASE_DGRAD h == 1"] +
         ["fp32 channel slice %s" % op for op in ("fwd", "dgrad", "wgrad")] +
         ["wgrad several ragged splits", "wgrad segments start mid-table", "wgrad 2 windows", "wgrad 3 windows", "wgrad windows, unforced", "wgrad straight into dw",
          "wgrad accumulate, one split", "wgrad accumulate, several splits", "wgrad deferred", "merged bwd deferred", "bias grad deferred"] +
         ["merged bwd 1 segment vec4_tap", "merged bwd 1 segment vec4", "merged bwd 4 segments vec4_tap", "merged bwd 4 segments vec4"] +
         ["bwd in two calls: %s" % why for why in ("x3_1x1", "direct_grouped", "x3_patch", "shape: scalar loads", "shape: more than 4 segments",
                                                   "shape: phase decomposition")] +
         ["stats fp32", "stats stem", "stats x3_1x1 m128", "stats x3_1x1 m64", "stats x3_patch", "stats refused: ragged map", "stats refused: bias",
          "stats refused: split-K"] +
         ["bias grad one segment", "bias grad several segments", "bias grad cout % 4 != 0"])


def _plan_rows(name, monkeypatch):
    """-> {op: (row in EXPECT's form, bytes the workspace function returns)} for the case's ops (bias_grad has no plan)"""
    case = R.CASES[name]
    R.configure(case, monkeypatch)
    segs, nseg, geom = R.host_call(case)
    rows = {}
    for op in case.ops:
        if op == "bias_grad":
            continue
        need = R.workspace_need(case, op, segs, nseg, geom)
        given, null = R.workspace_given(case, op, need)
        refused = EXPECT.get(name, {}).get(op, ("",))[0] == "refused"
        plan = R.query(case, op, segs, nseg, geom, given, None if null else R.FAKE, status=EUNSUPPORTED if refused else 0)
        rows[op] = ((("refused",) if refused else ()) + R.row_of(plan, op), need)
    return rows


def _observe(name, monkeypatch):
    """names of the branches the case takes"""
    case = R.CASES[name]
    forced = dict(case.env)
    names = set()
    nseg, pixels = len(case.segs), sum(n * h * w for n, h, w in case.segs)
    cin_g, cout_g = case.cin // case.groups, case.cout // case.groups
    for op, (row, need) in _plan_rows(name, monkeypatch).items():
        if op == "bwd":
            d, w = row[2], row[3]
            if row[0] == "merged_bwd":
                names.add("merged bwd %d segment%s %s" % (nseg, "s" if nseg > 1 else "", d[2]))
                if w[-1] == "deferred":
                    names = names - {"merged bwd 1 segment vec4"} | {"merged bwd deferred"}
            else:
                why = row[1]
                if why == "shape":
                    why += ": " + ("more than 4 segments" if nseg > 4 else "phase decomposition" if d[6] else "scalar loads" if d[2] == "scalar" else "other")
                names.add("bwd in two calls: %s" % why)
            continue
        if op == "fwd_stats":
            if row[0] == "refused":
                names.add("stats refused: %s" % ("bias" if case.bias else "split-K" if row[4] > 1 else "ragged map"))
            else:
                names.add("stats %s" % (row[0] if row[0] != "x3_1x1" else "x3_1x1 m%d" % row[1]))
            continue
        path = row[0]
        if path == "fp32":
            _, cfg, load, nsplit, ksplit, blocks = row[:6]
            names.add("fp32 %s cfg%d %s" % (op, cfg, load))
            width = cout_g if op == "fwd" else cin_g
            if op in ("fwd", "dgrad"):
                if "RN_CONV_CFG" not in forced:
                    names.add("cfg%d by group width" % cfg if (case.groups > 1 and width <= 64) else "cfg%d by choose_cfg" % cfg)
                if case.groups > 1 and width > 64:
                    names.add("grouped fp32, groups wider than 64 %s" % op)
                if nseg == 5 and min(h * w for _, h, w in case.segs) == 1:
                    names.add("five segments down to 1 x 1 %s" % op)
                ktot = case.k * case.k * (case.cin if op == "fwd" else case.cout)
                if nsplit > 1:
                    names.add("split-K %s" % op)
                    if -(-ktot // 32) % ksplit:
                        names.add("split-K ranges of unequal length")
                    if ktot % 32:
                        names.add("split-K with a K tail")
                    if case.stride == 2:
                        names.add("split-K stride 2")
                    if 64 <= blocks // nsplit < 96:
                        names.add("split-K on 64 .. 95 tiles")
                elif need and case.k == 3 and case.stride == 1 and case.ws != "exact":
                    names.add("split-K refused: %s" % ("NULL workspace" if case.ws == "none" else "one byte short"))
                elif "RN_NO_SPLITK" in forced:
                    names.add("split-K off")
                if case.x_ld and not (op == "dgrad" and row[6]):
                    names.add("fp32 channel slice %s" % op)
                if case.cin == 3 and case.stride == 2 and op == "fwd":
                    names.add("stem shape just off: fp32 scalar")
                if case.k == 1 and case.stride == 1 and case.groups == 1 and nseg == 1 and not case.bias:
                    names.add("1x1 in product mode 0 %s" % op if case.mode == 0 else "1x1 just under 96 tiles")
                if need and case.ws == "none" and case.stride == 2 and case.cout >= 512:
                    names.add("patch matrix declined without a workspace %s" % op)
                if case.groups > 1 and case.k == 3 and case.cin == case.cout and cin_g in (4, 8, 16, 32):
                    names.add("grouped 3x3 just under the direct kernels' line")
            if op == "dgrad":
                phases, empty = row[6], row[7]
                h, w = case.segs[0][1:]
                if phases:
                    names.add("phases %s" % ("1x1: three without taps" if empty == 3 else "%dx%d" % (case.k, case.k)))
                    names.add("phases h == 1: two phases" if h == 1 else ("phases odd map" if h % 2 and w % 2 else "phases even map"))
                    if nseg > 1:
                        names.add("phases two segments")
                    if case.x_ld:
                        names.add("phases channel slice")
                elif "RN_NO_PHASE_DGRAD" in forced:
                    names.add("RN_NO_PHASE_DGRAD %s" % ("h == 1" if h == 1 else "%dx%d" % (case.k, case.k)))
            if op == "wgrad":
                windows, direct, reduce = row[6:9]
                if case.k == 1 and case.mode == 0:
                    names.add("1x1 in product mode 0 wgrad")
                if case.x_ld:
                    names.add("fp32 channel slice wgrad")
                if nseg == 1 and nsplit > 1 and pixels % ksplit and pixels % 32 and not case.accumulate and not case.defer:
                    names.add("wgrad several ragged splits")
                if nseg > 1 and nsplit > nseg:
                    names.add("wgrad segments start mid-table")
                if windows:
                    names.add("wgrad %d windows" % -(-min(pixels, ksplit) // R.WG_MAXPIX) if "RN_WGRAD_SPLITS" in forced else "wgrad windows, unforced")
                if direct:
                    names.add("wgrad straight into dw")
                if case.accumulate:
                    names.add("wgrad accumulate, %s" % ("one split" if nsplit == 1 else "several splits"))
                if reduce == "deferred":
                    names.add("wgrad deferred")
        elif path == "x3_1x1":
            names.add("x3_1x1 fwd m%d" % row[1] if op == "fwd" else "x3_1x1 %s" % op)
            if case.x_ld:
                names.add("x3_1x1 %s channel slice" % op)
        elif path == "x3_patch":
            names.add("x3_patch %s" % op)
        elif path == "direct_grouped":
            names.add("direct_grouped %s cg%d" % (op, cin_g))
        else:
            names.add(path)
    if "bias_grad" in case.ops:
        names.add("bias grad deferred" if case.defer else ("bias grad one segment" if nseg == 1 else "bias grad several segments"))
        if case.cout % 4:
            names.add("bias grad cout % 4 != 0")
    return names


def _observe_gemm(name):
    row = R.gemm_row(name)
    m, k, n, nb, b_nk, mode = R.GEMMS[name]
    if row[0] != "fp32":
        return {"batched split-bf16 product"}
    if k % 32 == 0:
        return {"batched fp32 product tap-uniform"}
    return {"batched fp32 product %s with a K tail" % ("nk" if b_nk else "kn")}


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_its_branch(monkeypatch, name):
    assert set(EXPECT[name]) == set(op for op in R.CASES[name].ops if op != "bias_grad")
    for op, (row, _) in _plan_rows(name, monkeypatch).items():
        assert row == EXPECT[name][op], ("%s %s now takes %s, not %s: the planner changed -- pick another shape for that branch"
                                         % (name, op, row, EXPECT[name][op]))


@pytest.mark.parametrize("name", list(R.GEMMS))
def test_batched_product_takes_its_branch(name):
    import _rn
    try:
        assert R.gemm_row(name) == GEMM_EXPECT[name], "the planner changed -- pick another shape for that branch"
    finally:
        _rn.lib().rn_set_product_mode(1)


def _all_names(monkeypatch):
    import _rn
    per_case = {name: _observe(name, monkeypatch) for name in R.CASES}
    per_case.update({name: _observe_gemm(name) for name in R.GEMMS})
    _rn.lib().rn_set_product_mode(1)
    return per_case


def test_table_reaches_every_branch(monkeypatch):
    assert len(set(COVER)) == len(COVER)
    seen = set().union(*_all_names(monkeypatch).values())
    missing = [b for b in COVER if b not in seen]
    assert not missing, "no case of the table reaches: %s" % missing


def test_every_case_is_needed(monkeypatch):
    """Each case is the only one that reaches some branch of COVER: removing it makes test_table_reaches_every_branch name the
    branch that lost its case."""
    per_case = _all_names(monkeypatch)
    idle = [name for name, mine in per_case.items()
            if not any(b in COVER and all(b not in other for o, other in per_case.items() if o != name) for b in mine)]
    assert not idle, "cases that pin no branch of their own: %s" % idle


@pytest.mark.parametrize("name", list(R.CASES))
def test_workspace_suffices_for_the_path(monkeypatch, name):
    """With rn_conv2d_*_workspace bytes every call succeeds and decides as with unlimited scratch; with one byte less the forward
    and the data gradient give up their split-K / patch matrix (for them the size is exact).  The weight gradient's size is the
    largest of the paths either product mode may take: it refuses less than its own path needs (test_refusals)."""
    import _rn
    case = R.CASES[name]._replace(ws="exact")
    R.configure(case, monkeypatch)
    segs, nseg, geom = R.host_call(case)
    for op in case.ops:
        if op in ("bias_grad", "fwd_stats"):
            continue
        need = R.workspace_need(case, op, segs, nseg, geom)
        exact = R.row_of(R.query(case, op, segs, nseg, geom, need), op)
        assert exact == R.row_of(R.query(case, op, segs, nseg, geom, 1 << 40), op)
        if op in ("wgrad", "bwd"):
            assert need > 0
        elif need:
            assert R.row_of(R.query(case, op, segs, nseg, geom, need - 1), op) != exact, op
    assert _rn.lib().rn_conv2d_bias_grad_workspace(case.cout) == 256 * case.cout * 4


CHILD = r"""
import ctypes as C, os, sys
sys.path[:0] = %r
import conv_ref as R, _rn
class Env:
    def delenv(self, n, raising=False): os.environ.pop(n, None)
    def setenv(self, n, v): os.environ[n] = v
R.PROCESS_SWITCHES = ()
name, op = sys.argv[1:3]
case = R.CASES.get(name) or R.EXTRA[name]
R.configure(case, Env())
segs, nseg, geom = R.host_call(case)
need = R.workspace_need(case, op, segs, nseg, geom)
print(repr(R.row_of(R.query(case, op, segs, nseg, geom, need), op)))
"""
# switch, value, case, op -> the row in a process started with the switch (the table's rows hold without it)
PROCESS_ROWS = {
    "RN_STEM_DIRECT": ('0', 'stem', 'fwd', ('fp32', 2, 'scalar', 1, 0, 8)),
    "RN_X3_CONV1X1": ('0', 'x3-1x1-m64', 'fwd', ('fp32', 2, 'vec4_tap', 1, 0, 96)),
    "RN_X3_IM2COL": ('0', 'patch', 'fwd', ('fp32', 2, 'vec4_tap', 1, 0, 384)),
    "RN_GCONV_DIRECT": ('0', 'gconv-cg8', 'fwd', ('fp32', 3, 'vec4', 1, 0, 704)),
    "RN_NO_MERGED_BWD": ('1', 'bwd-merged-tap', 'bwd', ('two_calls', 'switch', ('fp32', 2, 'vec4_tap', 1, 0, 5, 0, 0), ('fp32', 2, 'vec4', 5, 64, 25, 0, 0, 'launched'))),
    "RN_X3_IM2COL_PIECE_MB": ('16', 'patch-pieces', 'fwd', ('x3_patch', 64, 3, 14155776)),
}


@pytest.mark.parametrize("switch", list(R.PROCESS_SWITCHES))
def test_once_per_process_switch(switch):
    value, name, op, row = PROCESS_ROWS[switch]
    assert name in R.EXTRA or EXPECT[name][op] != row
    env = dict(os.environ)
    env[switch] = value
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [os.path.dirname(here), os.path.join(os.path.dirname(here), "retinanet-tensorflow_amd"), here]
    out = subprocess.run([sys.executable, "-c", CHILD % (paths,), name, op], env=env, check=True, capture_output=True, text=True).stdout
    assert eval(out.strip().splitlines()[-1]) == row, (switch, out)


def test_refusals(monkeypatch):
    import _rn
    L = _rn.lib()
    base = R.EXTRA["refusals"]
    R.configure(base, monkeypatch)

    def status(case=base, op="fwd", nseg=None, plan=True, edit=None, dw=R.FAKE, ws=R.FAKE, ws_bytes=1 << 30, opcode=None):
        segs, n, geom = R.host_call(case)
        if edit:
            edit(segs, geom)
        p = _rn.ConvPlan()
        return L.rn_conv2d_plan(segs, n if nseg is None else nseg, C.byref(geom), _rn.CONV_OPS[op] if opcode is None else opcode, 0, 0, 0, dw, ws,
                                ws_bytes, C.byref(p) if plan else None)

    assert status() == 0
    assert status(plan=False) == EINVAL and status(opcode=9) == EINVAL
    assert status(nseg=0) == EINVAL and status(nseg=_rn.MAX_SEG + 1) == EINVAL
    for field in ("kh", "kw", "stride", "cin"):
        assert status(edit=lambda s, g, f=field: setattr(g, f, 0)) == EINVAL, field
    assert status(edit=lambda s, g: setattr(g, "groups", -1)) == EINVAL
    assert status(edit=lambda s, g: setattr(g, "groups", 3)) == EINVAL                           # cin 16
    assert status(edit=lambda s, g: (setattr(g, "groups", 4), setattr(s[0], "cout", 50))) == EINVAL
    for field in ("n", "h", "w", "cout"):
        assert status(edit=lambda s, g, f=field: setattr(s[0], f, 0)) == EINVAL, field
    for ld, off in ((24, 12), (18, 0), (32, 2), (32, -4)):                                       # too narrow, not multiples of 4, negative
        assert status(edit=lambda s, g, a=ld, b=off: (setattr(s[0], "x_ld", a), setattr(s[0], "x_coff", b))) == EINVAL, (ld, off)
    assert status(edit=lambda s, g: (setattr(s[0], "x_ld", 32), setattr(s[0], "x_coff", 16))) == 0
    assert status(edit=lambda s, g: (setattr(s[0], "h", 8192), setattr(s[0], "w", 8192))) == EUNSUPPORTED     # x: 2 x 2^26 x 16 x 4 bytes
    assert status(edit=lambda s, g: (setattr(s[0], "n", 1), setattr(s[0], "h", 32768), setattr(s[0], "w", 1))) == EUNSUPPORTED
    for op, field in (("fwd", "x"), ("fwd", "wgt"), ("fwd", "y"), ("dgrad", "dy"), ("dgrad", "dx"), ("wgrad", "x"), ("wgrad", "dy")):
        assert status(op=op, edit=lambda s, g, f=field: setattr(s[0], f, None)) == EINVAL, (op, field)
    assert status(op="wgrad", dw=None) == EINVAL and status(op="wgrad", ws=None) == EINVAL
    assert status(op="wgrad", ws_bytes=16) == EWORKSPACE and status(op="bwd", ws_bytes=16) == EWORKSPACE
    assert status(op="fwd", ws=None, ws_bytes=0) == 0                                            # never an error for the forward call
    two = base._replace(segs=((2, 9, 7), (2, 5, 5)))
    assert status(case=two, op="wgrad", edit=lambda s, g: setattr(s[1], "cout", 32)) == EINVAL   # one kernel tensor


SMALL_REFS = [((2, 5, 4), 3, 4, 3, 1, 1), ((1, 7, 5), 4, 6, 3, 2, 1), ((2, 6, 8), 4, 6, 3, 2, 2), ((1, 5, 7), 2, 3, 1, 2, 1),
              ((1, 9, 9), 2, 2, 7, 2, 1), ((1, 1, 6), 3, 2, 3, 2, 1), ((2, 4, 5), 6, 9, 3, 1, 3)]


@pytest.mark.parametrize("shape,cin,cout,k,stride,groups", SMALL_REFS)
def test_reference_against_a_loop_convolution(shape, cin, cout, k, stride, groups):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape + (cin,), generator=gen, dtype=torch.float64)
    w = torch.randn(k, k, cin // groups, cout, generator=gen, dtype=torch.float64)
    b = torch.randn(cout, generator=gen, dtype=torch.float64)
    y = R.conv_same(x, w, stride, groups, b).numpy()
    assert rel_err(y, R.conv_same_naive(x.numpy(), w.numpy(), stride, groups, b.numpy())) < 1e-13
    if groups == 1:
        assert rel_err(y, T.conv2d_same(x, w, stride, b).numpy()) < 1e-13
        assert rel_err(y, T.conv2d_same_naive(x.numpy(), w.numpy(), stride, b.numpy())) < 1e-13
    for n, s in ((shape[1], stride), (shape[2], stride)):
        import _rn
        assert R.same_pad(n, k, s)[:2] == _rn.same_pad(n, k, s) and R.same_pad(n, k, s) == T.same_pad_1d(n, k, s)


def test_reference_gradients_and_rows():
    """autograd's gradients against the definition on a tiny case; the statistic rows against a loop"""
    case = R._case([(1, 5, 4), (2, 3, 3)], 4, 6, stride=2, seed=5)
    xs, w, _, dys, _ = R.make_case(case)
    ref = R.run_ref(case, torch.float64)
    eps = 1e-6
    wd = w.double()
    for idx in ((0, 0, 0, 0), (2, 1, 3, 5), (1, 2, 2, 1)):
        wp, wm = wd.clone(), wd.clone()
        wp[idx] += eps
        wm[idx] -= eps
        f = lambda ww: sum(float((R.conv_same(x.double(), ww, 2) * d.double()).sum()) for x, d in zip(xs, dys))
        assert abs((f(wp) - f(wm)) / (2 * eps) - ref["dw"][idx]) < 1e-6 * max(1.0, abs(ref["dw"][idx]))
    assert rel_err(ref["dbias"], sum(d.double().sum((0, 1, 2)) for d in dys).numpy()) < 1e-14
    y = torch.randn(2, 4, 6, 5, dtype=torch.float64)
    rows = R.stat_rows(y, 3)
    flat = y.reshape(2, 24, 5)
    for n in range(2):
        for r in range(3):
            part = flat[n, r * 8:(r + 1) * 8]
            assert np.allclose(rows[n * 3 + r, :, 0], part.sum(0).numpy()) and np.allclose(rows[n * 3 + r, :, 1], (part * part).sum(0).numpy())


def test_plan_structs_match_the_header():
    import _rn
    assert C.sizeof(_rn.ConvPlanCall) == 80 and C.sizeof(_rn.ConvPlan) == 248
