"""The case table of tests/f16_conv_ref.py without a GPU: every case takes the branch of the fp16 convolution's dispatch it was
picked for (read off the host-only rn_conv2d_f16_plan: the library loads without a device, and the query is conv_f16_impl
itself, stopped before the first launch, under the same environment switches), and the table as a whole reaches every branch
listed in COVER.  A dispatch change that moves a case off its branch fails here and says: pick another shape for that branch.
Further tests: the once-per-process switches (each group in a fresh process), the refusals, rn_conv2d_f16_fold_rows /
rn_conv2d_f16_stats_tiles against the plan, ops_f16.sg_kernel_takes against the plan, and the reference itself.

The rows are f16_conv_ref.row_of's:
  implicit GEMM: ('igemm', tile 0..5, gather 4 | 8, tap-uniform, F (0, 2 statistics, 3 input fold + statistics, 7 with ReLU),
                  pipe (0 plain, 1 both operands through LDS, 2 weight fragments), epilogue, non-temporal loads,
                  fragment copy proven, blocks, K tiles, rows per sample, (tiles per sample of every segment))
  super-group:   ('sg', stride, FIN (0, 1 any activation, 2 ReLU), statistics, blocks, rows per sample)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import f16_conv_ref as R
from helpers import rel_err
from oracle import tf_ops_ref as T

EINVAL, EUNSUPPORTED = -1, -2

EXPECT = {
    "cfg0-vec4": ('igemm', 0, 4, 0, 0, 0, 'staged', 0, 0, 9, 2, 0, (0,)),
    "cfg0-vec8": ('igemm', 0, 8, 0, 0, 0, 'scalar_f32', 0, 0, 9, 4, 0, (0,)),
    "cfg0-tap": ('igemm', 0, 8, 1, 0, 0, 'staged', 0, 1, 9, 9, 0, (0,)),
    "cfg1-vec4": ('igemm', 1, 4, 0, 0, 0, 'staged', 0, 0, 15, 2, 0, (0,)),
    "cfg1-vec8": ('igemm', 1, 8, 0, 0, 0, 'scalar_f32', 0, 0, 15, 4, 0, (0,)),
    "cfg1-tap": ('igemm', 1, 8, 1, 0, 0, 'staged', 0, 1, 15, 9, 0, (0,)),
    "cfg2-vec4": ('igemm', 2, 4, 0, 0, 0, 'staged', 0, 0, 25, 2, 0, (0,)),
    "cfg2-vec8": ('igemm', 2, 8, 0, 0, 0, 'scalar_f32', 0, 0, 25, 4, 0, (0,)),
    "cfg2-tap": ('igemm', 2, 8, 1, 0, 0, 'staged', 0, 1, 25, 9, 0, (0,)),
    "cfg3-vec4": ('igemm', 3, 4, 0, 0, 0, 'staged', 0, 0, 27, 2, 0, (0,)),
    "cfg3-vec8": ('igemm', 3, 8, 0, 0, 0, 'scalar_f32', 0, 0, 27, 4, 0, (0,)),
    "cfg3-tap": ('igemm', 3, 8, 1, 0, 0, 'staged', 0, 1, 27, 9, 0, (0,)),
    "cfg4-vec4": ('igemm', 4, 4, 0, 0, 0, 'staged', 0, 0, 6, 2, 0, (0,)),
    "cfg4-vec8": ('igemm', 4, 8, 0, 0, 0, 'scalar_f32', 0, 0, 6, 4, 0, (0,)),
    "cfg4-tap": ('igemm', 4, 8, 1, 0, 0, 'staged', 0, 1, 6, 9, 0, (0,)),
    "cfg5-vec4": ('igemm', 5, 4, 0, 0, 0, 'staged', 0, 0, 4, 2, 0, (0,)),
    "cfg5-vec8": ('igemm', 5, 8, 0, 0, 0, 'scalar_f32', 0, 0, 4, 4, 0, (0,)),
    "cfg5-tap": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 4, 9, 0, (0,)),
    "scalar16-cfg3": ('igemm', 3, 8, 0, 0, 0, 'scalar_f16', 0, 0, 6, 4, 0, (0,)),
    "scalar16-cfg5": ('igemm', 5, 8, 0, 0, 0, 'scalar_f16', 0, 0, 2, 4, 0, (0,)),
    "stride2": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 10, 4, 0, (0,)),
    "k1": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 25, 1, 0, (0,)),
    "stem": ('igemm', 2, 4, 0, 2, 0, 'staged', 0, 0, 8, 4, 4, (4,)),
    "auto-0": ('igemm', 0, 8, 0, 0, 0, 'staged', 0, 0, 208, 1, 0, (0,)),
    "auto-1": ('igemm', 1, 8, 0, 0, 0, 'staged', 0, 0, 1168, 1, 0, (0,)),
    "auto-2": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 5, 4, 0, (0,)),
    "auto-3": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 0, 146, 1, 0, (0,)),
    "group-w24": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 0, 2, 4, 0, (0,)),
    "group-w48": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 4, 4, 0, (0,)),
    "group-w96": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 8, 11, 0, (0,)),
    "auto-5": ('igemm', 5, 8, 1, 0, 2, 'staged', 1, 1, 512, 2, 256, (256,)),
    "auto-5-miss-big": ('igemm', 0, 8, 1, 0, 0, 'staged', 0, 1, 2044, 2, 1022, (1022,)),
    "auto-5-miss-k128": ('igemm', 0, 8, 1, 0, 0, 'staged', 0, 1, 2048, 1, 512, (512,)),
    "auto-5-miss-k512": ('igemm', 1, 8, 1, 0, 0, 'staged', 0, 1, 5120, 2, 512, (512,)),
    "auto-5-miss-vec4": ('igemm', 0, 4, 0, 0, 0, 'staged', 0, 0, 2048, 3, 512, (512,)),
    "pipe2-k1": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 4, 1, 0, (0,)),
    "pipe2-k2": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 4, 2, 0, (0,)),
    "pipe2-k3": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 4, 3, 0, (0,)),
    "pipe2-one-n-tile": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 2, 2, 0, (0,)),
    "pipe2-stats": ('igemm', 5, 8, 1, 2, 2, 'staged', 0, 1, 4, 9, 1, (1,)),
    "pipe1-short": ('igemm', 5, 8, 1, 0, 1, 'staged', 0, 0, 4, 9, 0, (0,)),
    "pipe1-short-stats": ('igemm', 5, 8, 1, 2, 1, 'staged', 0, 0, 4, 9, 1, (1,)),
    "fin7-plain-short": ('igemm', 5, 8, 1, 7, 0, 'staged', 0, 0, 4, 2, 1, (1,)),
    "fin7-pipe-k2": ('igemm', 5, 8, 1, 7, 2, 'staged', 0, 1, 4, 2, 1, (1,)),
    "fin7-pipe-k5": ('igemm', 5, 8, 1, 7, 2, 'staged', 0, 1, 4, 5, 1, (1,)),
    "fin7-pipe-2048": ('igemm', 5, 8, 1, 7, 2, 'staged', 0, 1, 2, 32, 1, (1,)),
    "fin3-elu": ('igemm', 5, 8, 1, 3, 0, 'staged', 0, 1, 4, 2, 1, (1,)),
    "fin7-3x3": ('igemm', 5, 8, 1, 7, 0, 'staged', 0, 1, 4, 9, 1, (1,)),
    "fin7-3x3-cfg2": ('igemm', 2, 8, 1, 7, 0, 'staged', 0, 1, 4, 9, 1, (1,)),
    "fin3-3x3-cin96": ('igemm', 2, 8, 0, 3, 0, 'staged', 0, 1, 16, 14, 4, (4,)),
    "slice-plain": ('igemm', 2, 8, 1, 0, 0, 'staged', 0, 1, 25, 9, 0, (0,)),
    "slice-pipe": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 4, 9, 0, (0,)),
    "multi-plain": ('igemm', 2, 8, 0, 0, 0, 'staged', 0, 0, 28, 4, 0, (0, 0, 0)),
    "multi-stats": ('igemm', 2, 8, 1, 2, 0, 'staged', 0, 1, 22, 9, 0, (4, 1, 0)),
    "multi-stats-cfg5": ('igemm', 5, 8, 1, 2, 2, 'staged', 0, 1, 22, 9, 0, (4, 1, 0)),
    "multi-stats-vec4": ('igemm', 2, 4, 0, 2, 0, 'staged', 0, 0, 20, 2, 0, (4, 1)),
    "sg1-plain": ('sg', 1, 0, 0, 24, 6),
    "sg1-stats": ('sg', 1, 0, 1, 24, 6),
    "sg1-elu": ('sg', 1, 1, 1, 24, 6),
    "sg1-relu": ('sg', 1, 2, 1, 24, 6),
    "sg2-plain": ('sg', 2, 0, 0, 32, 8),
    "sg2-stats": ('sg', 2, 0, 1, 32, 8),
    "sg2-elu": ('sg', 2, 1, 1, 32, 8),
    "sg2-relu": ('sg', 2, 2, 1, 32, 8),
    "sg1-cg4": ('sg', 1, 0, 1, 24, 6),
    "sg1-cg8": ('sg', 1, 0, 1, 24, 6),
    "sg1-cg16": ('sg', 1, 0, 1, 24, 6),
    "sg-miss-map": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 1, 24, 5, 6, (0,)),
    "sg-miss-bias": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 1, 48, 5, 12, (0,)),
    "sg-miss-f32": ('igemm', 3, 8, 0, 0, 0, 'scalar_f32', 0, 1, 48, 5, 0, (0,)),
    "sg-miss-short": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 0, 48, 5, 12, (0,)),
    "sg-miss-slice": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 1, 48, 5, 12, (0,)),
}

FORCED = [(c, l) for c in range(6) for l in ("vec4", "vec8", "tap")]
# every branch the table must reach, by the names _observe() gives them
COVER = (["igemm forced tile %d %s" % cl for cl in FORCED] +
         ["epilogue staged", "epilogue scalar_f16", "epilogue scalar_f32", "bias, staged epilogue", "bias, scalar epilogue",
          "stride 2", "1x1, ragged tiles both ways, one K tile with a tail", "stem 7x7/2: vec4 with statistics (F 2)"] +
         ["cost model -> tile %d" % c for c in range(4)] +
         ["grouped, cout/G <= 32 -> tile 3", "grouped, cout/G 33..64 -> tile 2", "grouped, cout/G > 64: cost model"] +
         ["automatic tile 5", "automatic non-temporal loads", "tile 5 missed: big = 511", "tile 5 missed: K < 128", "tile 5 missed: K < 512",
          "tile 5 missed: cin % 8"] +
         ["pipe 2, %d K tiles" % k for k in (1, 2, 3, 9)] +
         ["pipe 1: wgt_bytes covers Wt only", "pipe 1 with statistics: wgt_bytes covers Wt only", "pipe 2 with statistics",
          "plain F 7: no fragment copy", "pipelined F 7, 2 K tiles", "pipelined F 7, 5 K tiles", "pipelined F 7, cin 2048: 32 K tiles",
          "plain F 3 (ELU fold)", "plain F 7 in front of a 3x3", "plain F 7 at the 64-row tile", "input fold, not tap-uniform"] +
         ["channel slice, plain loop", "channel slice, pipelined"] +
         ["segments with different cout", "segment statistics, the last straddles samples, automatic tile",
          "segment statistics, the last straddles samples, tile 5", "segment statistics, vec4"] +
         ["sg stride %d %s" % (s, v) for s in (1, 2) for v in ("plain", "statistics", "FIN 1", "FIN 2")] +
         ["sg %d channels per group" % g for g in (4, 8, 16)] +
         ["sg missed: %s" % w for w in ("map", "bias", "fp32 output", "wgt_bytes", "channel slice")])


def _row(name, monkeypatch):
    R.configure(R.CASES[name], monkeypatch)
    return R.plan_row(R.CASES[name])


def _observe(name, monkeypatch):
    """names of the branches the case takes"""
    case, row = R.CASES[name], _row(name, monkeypatch)
    names, nseg = set(), len(case.segs)
    cin_g, cout_g = case.cin // case.groups, case.cout[0] // case.groups
    sg_shaped = case.groups > 1 and case.k == 3 and cin_g == cout_g and cin_g in (4, 8, 16, 32) and case.cout[0] % 32 == 0
    if row[0] == "sg":
        _, stride, fin, stats, _, _ = row
        if cin_g == 32:
            names.add("sg stride %d %s" % (stride, "FIN %d" % fin if fin else "statistics" if stats else "plain"))
        else:
            names.add("sg %d channels per group" % cin_g)
        return names
    _, cfg, vec, tapu, f, pipe, epi, a_nt, frag, blocks, k_tiles, rps, tps = row
    load = "tap" if tapu else "vec%d" % vec
    plain = not (case.fold or case.stats or case.x_ld or nseg > 1 or case.wgt != "full" or case.groups > 1)
    if sg_shaped:
        why = ("bias" if case.bias else "fp32 output" if case.out_f32 else "wgt_bytes" if case.wgt != "full" else "channel slice" if case.x_ld
               else "map")
        # the plan says so: the same call without that one property is the super-group kernel's
        undo = {"bias": dict(bias=False), "fp32 output": dict(out_f32=False), "wgt_bytes": dict(wgt="full"), "channel slice": dict(x_ld=0, x_coff=0),
                "map": dict(segs=tuple(R.SG_MAP[1]))}[why]
        if R.plan_row(case._replace(**undo))[0] == "sg":
            names.add("sg missed: %s" % why)
        return names
    if case.cfg is not None and plain and case.k == 3 and case.cout[0] == 264:
        names.add("igemm forced tile %d %s" % (cfg, load))
    if plain:
        names.add("epilogue %s" % epi)
        if case.bias:
            names.add("bias, %s epilogue" % ("staged" if epi == "staged" else "scalar"))
        if case.stride == 2:
            names.add("stride 2")
        m = sum(n * int(np.prod(R.out_hw(case, h, w))) for n, h, w in case.segs)
        if case.k == 1 and case.cfg is None and cfg != 5 and k_tiles == 1 and R.k_products(case) % 64 and m % R.BM[cfg] and case.cout[0] % R.BN[cfg]:
            names.add("1x1, ragged tiles both ways, one K tile with a tail")
    if case.k == 7 and case.stride == 2 and case.cin == 4 and (vec, f) == (4, 2):
        names.add("stem 7x7/2: vec4 with statistics (F 2)")
    if case.cfg is None and plain:
        big = sum(-(-n * np.prod(R.out_hw(case, h, w)) // 256) * -(-co // 256) for (n, h, w), co in zip(case.segs, case.cout))
        K = R.k_products(case)
        if cfg == 5:
            names.add("automatic tile 5")
            if a_nt:
                names.add("automatic non-temporal loads")
        elif case.k == 1 and big == 511:
            names.add("tile 5 missed: big = 511")
        elif big >= 512 and case.cin % 8:
            names.add("tile 5 missed: cin % 8")
        elif big >= 512 and K < 128:
            names.add("tile 5 missed: K < 128")
        elif big >= 512 and K < 512:
            names.add("tile 5 missed: K < 512")
        else:
            names.add("cost model -> tile %d" % cfg)
    if case.groups > 1 and case.cfg is None:
        names.add("grouped, cout/G <= 32 -> tile 3" if (cout_g <= 32 and cfg == 3) else "grouped, cout/G 33..64 -> tile 2" if (33 <= cout_g <= 64 and cfg == 2)
                  else "grouped, cout/G > 64: cost model" if cout_g > 64 else "grouped: ?")
    if cfg == 5 and not case.x_ld and nseg == 1:
        if pipe == 2 and f == 0 and case.wgt == "full":
            names.add("pipe 2, %d K tiles" % k_tiles)
        if pipe == 2 and f == 2:
            names.add("pipe 2 with statistics")
        if pipe == 1 and case.wgt == "wt" and not frag:
            names.add("pipe 1 with statistics: wgt_bytes covers Wt only" if f == 2 else "pipe 1: wgt_bytes covers Wt only")
        if f == 7 and pipe == 0 and case.k == 1 and not frag:
            names.add("plain F 7: no fragment copy")
        if f == 7 and pipe == 2:
            names.add("pipelined F 7, cin 2048: 32 K tiles" if case.cin == 2048 else "pipelined F 7, %d K tiles" % k_tiles)
        if f == 3 and pipe == 0:
            names.add("plain F 3 (ELU fold)")
        if f == 7 and pipe == 0 and case.k == 3:
            names.add("plain F 7 in front of a 3x3")
    if f == 7 and cfg == 2:
        names.add("plain F 7 at the 64-row tile")
    if f in (3, 7) and not tapu:
        names.add("input fold, not tap-uniform")
    if case.x_ld:
        names.add("channel slice, %s" % ("pipelined" if pipe else "plain loop"))
    if nseg > 1:
        if not case.stats and len(set(case.cout)) > 1:
            names.add("segments with different cout")
        if f == 2 and vec == 4:
            names.add("segment statistics, vec4")
        elif f == 2 and tps[-1] == 0 and all(tps[:-1]):
            names.add("segment statistics, the last straddles samples, %s" % ("tile 5" if case.cfg == 5 and pipe else "automatic tile"))
    return names


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_its_branch(monkeypatch, name):
    row = _row(name, monkeypatch)
    assert row == EXPECT[name], ("%s now takes %s, not %s: the dispatch changed -- pick another shape for that branch" % (name, row, EXPECT[name]))


def test_table_reaches_every_branch(monkeypatch):
    assert len(set(COVER)) == len(COVER) and set(EXPECT) == set(R.CASES)
    per_case = {name: _observe(name, monkeypatch) for name in R.CASES}
    seen = set().union(*per_case.values())
    missing = [b for b in COVER if b not in seen]
    assert not missing, "no case of the table reaches: %s" % missing
    idle = [name for name, mine in per_case.items() if not mine & set(COVER)]
    assert not idle, "cases that reach no branch of COVER: %s" % idle


@pytest.mark.parametrize("name", list(R.CASES))
def test_fold_rows_and_stats_tiles_read_the_plan(monkeypatch, name):
    """rn_conv2d_f16_fold_rows and rn_conv2d_f16_stats_tiles are readers of the plan of the plain fp16-output call."""
    import _rn
    L = _rn.lib()
    case = R.CASES[name]
    R.configure(case, monkeypatch)
    call = R.HostCall(case)
    plan = call.query_plain()
    assert L.rn_conv2d_f16_fold_rows(call.segs, call.nseg, C.byref(call.geom)) == plan.rows_per_sample
    tiles = (C.c_int32 * call.nseg)(*([-7] * call.nseg))
    e = L.rn_conv2d_f16_stats_tiles(call.segs, call.nseg, C.byref(call.geom), tiles)
    if _rn.F16_KERNELS[plan.kernel] == "igemm" and plan.multi_stats:
        assert e == 0 and list(tiles) == list(plan.tiles_per_sample[:call.nseg])
        assert all(t == (np.prod(R.out_hw(case, h, w)) // R.BM[plan.cfg] if np.prod(R.out_hw(case, h, w)) % R.BM[plan.cfg] == 0 else 0)
                   for t, (_, h, w) in zip(tiles, case.segs))
    else:
        assert e == EUNSUPPORTED and list(tiles) == [-7] * call.nseg
    if case.stats == 1 and not case.out_f32:
        assert plan.rows_per_sample > 0 and call.query().rows_per_sample == plan.rows_per_sample


CHILD = r"""
import os, sys
sys.path[:0] = %r
import f16_conv_ref as R
class Env:
    def delenv(self, n, raising=False): os.environ.pop(n, None)
    def setenv(self, n, v): os.environ[n] = v
R.PROCESS_SWITCHES = ()
for name in sys.argv[1:]:
    R.configure(R.CASES[name], Env())
    print(repr((name, R.plan_row(R.CASES[name]))))
"""
# the once-per-process switches, in three fresh processes: (environment, {case: its row there}); the table's rows hold without them
PROCESS_ROWS = {
    "pipe0-sg0": ({"RN_F16_PIPE": "0", "RN_F16_SG": "0"}, {
        "cfg5-tap": ('igemm', 5, 8, 1, 0, 0, 'staged', 0, 1, 4, 9, 0, (0,)),
        "pipe2-stats": ('igemm', 5, 8, 1, 2, 0, 'staged', 0, 1, 4, 9, 1, (1,)),
        "fin7-pipe-k2": ('igemm', 5, 8, 1, 7, 0, 'staged', 0, 1, 4, 2, 1, (1,)),
        "sg1-plain": ('igemm', 3, 8, 0, 0, 0, 'staged', 0, 1, 48, 5, 12, (0,)),
        "sg2-relu": ('igemm', 3, 8, 0, 7, 0, 'staged', 0, 1, 32, 5, 8, (0,)),
    }),
    "pipe1-nt1": ({"RN_F16_PIPE": "1", "RN_F16_NT": "1"}, {
        "cfg5-tap": ('igemm', 5, 8, 1, 0, 1, 'staged', 0, 1, 4, 9, 0, (0,)),
        "pipe2-stats": ('igemm', 5, 8, 1, 2, 1, 'staged', 0, 1, 4, 9, 1, (1,)),
        "pipe2-one-n-tile": ('igemm', 5, 8, 1, 0, 1, 'staged', 1, 1, 2, 2, 0, (0,)),
        "fin7-pipe-k2": ('igemm', 5, 8, 1, 7, 0, 'staged', 0, 1, 4, 2, 1, (1,)),
    }),
    "nt0-mink64": ({"RN_F16_NT": "0", "RN_F16_PIPE_MIN_K": "64"}, {
        "auto-5": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 512, 2, 256, (256,)),
        "auto-5-miss-k128": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 512, 1, 256, (256,)),
        "auto-5-miss-k512": ('igemm', 5, 8, 1, 0, 2, 'staged', 0, 1, 1024, 2, 256, (256,)),
    }),
}


def child_paths():
    here = os.path.dirname(os.path.abspath(__file__))
    return [os.path.dirname(here), os.path.join(os.path.dirname(here), "retinanet-tensorflow_amd"), here]


@pytest.mark.parametrize("group", list(PROCESS_ROWS))
def test_once_per_process_switches(group):
    env, rows = PROCESS_ROWS[group]
    assert set(env) <= set(R.PROCESS_SWITCHES) and all(EXPECT[name] != row for name, row in rows.items())
    out = subprocess.run([sys.executable, "-c", CHILD % (child_paths(),)] + list(rows), env=dict(os.environ, **env), check=True, capture_output=True,
                         text=True).stdout
    got = dict(eval(line) for line in out.strip().splitlines())
    assert got == rows, (group, got)


def test_every_process_switch_has_a_row():
    assert set().union(*(set(env) for env, _ in PROCESS_ROWS.values())) == set(R.PROCESS_SWITCHES)


@pytest.mark.parametrize("what", list(R.REFUSALS))
def test_refusals(monkeypatch, what):
    import _rn
    case, tweak, status = R.REFUSALS[what]
    R.configure(case, monkeypatch)
    call = R.HostCall(case, tiles=[1] * len(case.segs), tweak=tweak)
    plan = _rn.F16Plan()
    e = _rn.lib().rn_conv2d_f16_plan(call.segs, call.nseg, C.byref(call.geom), 1 if case.out_f32 else 0, call.fold_ref(), C.byref(plan))
    assert e == status, (what, e, _rn.lib().rn_last_error().decode())


def test_bad_arguments(monkeypatch):
    import _rn
    L = _rn.lib()
    base = R._case(R.WHOLE, 64, 72)
    R.configure(base, monkeypatch)

    def status(edit=None, nseg=None, plan=True):
        call = R.HostCall(base)
        if edit:
            edit(call.segs, call.geom)
        p = _rn.F16Plan()
        return L.rn_conv2d_f16_plan(call.segs, call.nseg if nseg is None else nseg, C.byref(call.geom), 0, None, C.byref(p) if plan else None)

    assert status() == 0 and status(plan=False) == EINVAL
    assert status(nseg=0) == EINVAL and status(nseg=_rn.MAX_SEG + 1) == EINVAL
    for field in ("kh", "kw", "stride", "cin"):
        assert status(edit=lambda s, g, f=field: setattr(g, f, 0)) == EINVAL, field
    assert status(edit=lambda s, g: setattr(g, "groups", 3)) == EINVAL                                   # cin 64
    assert status(edit=lambda s, g: (setattr(g, "groups", 4), setattr(s[0], "cout", 50))) == EINVAL
    for field in ("n", "h", "w", "cout", "x", "wgt", "y"):
        assert status(edit=lambda s, g, f=field: setattr(s[0], f, 0)) == EINVAL, field
    assert status(edit=lambda s, g: (setattr(s[0], "h", 8192), setattr(s[0], "w", 8192))) == EUNSUPPORTED  # x: 2 x 2^26 x 64 x 2 bytes


SG_GRID = [(h, w, stride, cg, c) for h in (16, 24, 32, 48, 64) for w in (16, 24, 32, 48, 64) for stride in (1, 2, 3) for cg in (4, 8, 16, 32, 64)
           for c in (64, 128)]


def test_sg_kernel_takes_agrees_with_the_plan(monkeypatch):
    """ops_f16.sg_kernel_takes repeats the C condition in Python: the two agree over a grid of shapes, on the geometry
    ops_f16.conv2d_norm passes after packed_weight's merge of narrow groups into 32-channel super-groups."""
    import _rn
    import ops_f16
    monkeypatch.delenv("RN_CONV_CFG", raising=False)
    assert "RN_F16_SG" not in os.environ and ops_f16.SG_KERNEL
    L = _rn.lib()
    n_sg, wrong = 0, []
    for h, w, stride, cg, c in SG_GRID:
        groups = c // cg
        wt = torch.empty(3, 3, cg, c, device="meta")
        # packed_weight: groups narrower than 32 channels are merged into super-groups of 32
        if groups > 1 and cg < ops_f16.SUPER_GROUP and ops_f16.SUPER_GROUP % cg == 0 and c % ops_f16.SUPER_GROUP == 0:
            cin_g, g2 = ops_f16.SUPER_GROUP, c // ops_f16.SUPER_GROUP
        else:
            cin_g, g2 = cg, groups
        seg = (_rn.ConvSeg * 1)()
        s = seg[0]
        s.x = s.wgt = s.y = R.FAKE
        s.n, s.h, s.w, s.cout = 2, h, w, c
        s.wgt_bytes = int(L.rn_pack_weights_f16_bytes(3, 3, cin_g, c))
        geom = _rn.ConvGeom(3, 3, stride, cin_g * g2, g2)
        plan = _rn.F16Plan()
        _rn.check(L.rn_conv2d_f16_plan(seg, 1, C.byref(geom), 0, None, C.byref(plan)), "rn_conv2d_f16_plan")
        c_says = _rn.F16_KERNELS[plan.kernel] == "sg"
        py_says = bool(ops_f16.sg_kernel_takes((2, h, w, c), wt, stride, groups))
        n_sg += c_says
        if c_says != py_says:
            wrong.append((h, w, stride, cg, c, c_says, py_says))
    assert not wrong, "ops_f16.sg_kernel_takes and conv_f16_impl disagree (h, w, stride, channels per group, C, C says, Python says): %s" % wrong
    assert 0 < n_sg < len(SG_GRID)


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name", ["stride2", "group-w48"])
def test_reference_against_torch_fp64(name):
    case = R.CASES[name]
    xs, ws, bs, _ = R.make_case(case)
    ref = R.run_ref(case)[0]
    x, w = torch.from_numpy(xs[0].astype(np.float64)), torch.from_numpy(ws[0].astype(np.float64))
    _, pt, pb = T.same_pad_1d(x.shape[1], case.k, case.stride)
    _, pl, pr = T.same_pad_1d(x.shape[2], case.k, case.stride)
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=case.stride,
                                   groups=case.groups).permute(0, 2, 3, 1).numpy()
    assert y.shape == ref.y64.shape and rel_err(ref.y64, y) < 1e-14
    if case.groups == 1:
        assert rel_err(ref.y64, T.conv2d_same(x, w, case.stride).numpy()) < 1e-14
    assert rel_err(ref.y32, ref.y64) < 1e-5 and np.all(ref.S >= np.abs(ref.y64) - 1e-12)
    # operands: fp16 values without subnormals, the kernel tensor exactly representable in fp16
    assert xs[0].dtype == np.float16 and not np.any((xs[0] != 0) & (np.abs(xs[0]) < 2.0 ** -14))
    assert np.array_equal(ws[0], ws[0].astype(np.float16).astype(np.float32)) and not np.any((ws[0] != 0) & (np.abs(ws[0]) < 2.0 ** -14))


@pytest.mark.parametrize("name", ["fin7-3x3-cfg2", "fin3-3x3-cin96"])
def test_fold_operand_against_group_norm(name):
    """The fold operand is act(GroupNorm(x)) rounded to fp16: against oracle/tf_ops_ref.group_norm + activation in fp64 (the
    statistics handed to the fold are x's own, so the two agree up to their fp32 rounding: a few fp16 spacings at most, none
    for most elements), and beta is centred at 0.5."""
    case = R.CASES[name]
    xs, _, _, gn = R.make_case(case)
    x = torch.from_numpy(xs[0].astype(np.float64))
    z = T.activation(T.group_norm(x, torch.from_numpy(gn[2]).double(), torch.from_numpy(gn[3]).double(), R.IN_GROUPS, R.EPS), case.fold).numpy()
    want = z.astype(np.float16)
    for dtype, fused in ((np.float64, False), (np.float32, False), (np.float32, True)):
        got = R.fold_operand(xs[0], gn, case.fold, dtype, fused)
        assert got.dtype == np.float16 and got.shape == want.shape
        off = np.abs(got.astype(np.float64) - want.astype(np.float64)) / R.fp16_ulp(z)
        assert off.max() <= 2.0 and (off > 0).mean() < 0.02, (off.max(), (off > 0).mean())
    assert abs(float(gn[3].mean()) - 0.5) < 0.1
    ref = R.run_ref(case)[0]
    assert np.all(ref.slack >= 0) and ref.slack.max() < 0.05 * ref.S.max()      # (a double rounding is rare: one element in thousands)


def test_fp16_spacing_and_statistic_rows():
    for v, u in ((1.0, 2.0 ** -10), (1.5, 2.0 ** -10), (2.0, 2.0 ** -9), (0.999, 2.0 ** -11), (2.0 ** -14, 2.0 ** -24), (1e-7, 2.0 ** -24), (0.0, 2.0 ** -24)):
        assert R.fp16_ulp(v) == u, v
        if v > 0:
            assert float(np.nextafter(np.float16(v), np.float16(np.inf))) - float(np.float16(v)) == u
    y = np.random.default_rng(0).standard_normal((2, 4, 6, 5))
    s1, s2, sa = R.stat_rows(y, 8)
    flat = y.reshape(2, 24, 5)
    for n in range(2):
        for r in range(3):
            part = flat[n, r * 8:(r + 1) * 8]
            assert np.allclose(s1[n * 3 + r], part.sum(0)) and np.allclose(s2[n * 3 + r], (part * part).sum(0)) and np.allclose(sa[n * 3 + r], np.abs(part).sum(0))


def test_plan_struct_matches_the_header():
    import _rn
    assert C.sizeof(_rn.F16Plan) == 4 * (14 + _rn.MAX_SEG)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rn_hip.h")).read()
    body = hdr[hdr.index("typedef struct rn_f16_plan {"):hdr.index("} rn_f16_plan;")]
    import re
    fields = re.findall(r"int32_t (\w+)(?:\[RN_MAX_SEG\])?;", body)
    assert fields == [f[0] for f in _rn.F16Plan._fields_]
