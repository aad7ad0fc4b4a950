"""rn_detect / rn_boxes_decode / rn_nms_classwise at every branch of their dispatch against the oracle (tests/detect_ref.py).

The entry points are driven directly (ctypes structs).  Every case first asserts, through rn_detect_plan with the real pointers,
that it runs the branch tests/test_detect_cases_cpu.py lists for it and that the plan's workspace figure is rn_detect_workspace's.
The workspace is exactly that many bytes followed by a guard area; the outputs are `capacity` rows followed by a guard; both
guards must come back untouched and the inputs bit-unchanged.  counts[], boxes, classes, images and anchors equal the oracle's
exactly; scores are bit-equal in probability mode and within 1e-6 (what tests/test_gpu_fullsize.py grants the hardware
exponential) where a level holds logits.  Rows in [counts[1], capacity) keep the sentinel, and a second call on the same buffers
gives the same bytes (the scatter's order is arbitrary, the result is not).

The logit cases print `DETECT_ERR <case> <largest |score - fp64 sigmoid|>` (pytest -s): the lines of profiles/detect_cases_err.txt.

RN_SCAN_T / RN_SCAN_NT are read once per process: their cases run in one fresh child process per switch."""
import ctypes as C
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import detect_ref as R
from test_detect_cases_cpu import EXPECT

pytestmark = pytest.mark.gpu

SCORE_BAR = 1e-6
FSENT, ISENT = 12345.0, -7
GUARD_ROWS, GUARD_BYTES = 257, 1 << 16
RN_EUNSUPPORTED, RN_EWORKSPACE = -2, -4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import _rn
    _rn.lib()
    return torch.device("cuda:0")


class Call:
    """The device side of one case: inputs, the level structs, sentinel-filled outputs with guard rows, the workspace."""

    def __init__(self, case, inputs, dev):
        import _rn
        self.case, self.dev, self.L = case, dev, _rn.lib()
        self.cap = cap = int(inputs.get("capacity", 0)) or R.capacity(case)
        self.par = _rn.DetParams(case.n, case.C, case.max_per_class, case.score_thr, case.iou_thr, cap)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.inputs, self.levels = [], None
        if case.entry == "nms_classwise":
            self.inputs = [t(inputs["boxes"]), t(inputs["scores"]), t(inputs["class_ids"]), t(inputs["image_ids"]),
                           torch.tensor([inputs["count"]], dtype=torch.int64, device=dev)]
        else:
            self.levels = (_rn.DetLevel * len(case.levels))()
            for i, lv in enumerate(case.levels):
                p = t(inputs["probs"][i])
                assert p.dtype == (torch.float16 if lv.half else torch.float32) and tuple(p.shape) == (case.n, lv.rows, case.C)
                self.inputs.append(p)
                s = self.levels[i]
                s.prob, s.prob_f16, s.prob_is_logit, s.rows_per_image = p.data_ptr(), int(lv.half), int(lv.logit), lv.rows
                if case.entry == "detect_raw":
                    reg, anc = t(inputs["regs"][i]), t(inputs["anchors"][i])
                    self.inputs += [reg, anc]
                    s.boxes, s.regression, s.regression_f16, s.anchor_sizes = None, reg.data_ptr(), int(lv.half_reg), anc.data_ptr()
                    s.grid_h, s.grid_w, s.num_anchors = lv.h, lv.w, lv.A
                else:
                    b = t(inputs["boxes"][i])
                    assert b.dtype == torch.float32 and tuple(b.shape) == (case.n, lv.rows, 4)
                    self.inputs.append(b)
                    s.boxes = b.data_ptr()
        self.keep = [x.clone() for x in self.inputs]
        rows = cap + GUARD_ROWS
        self.out = {"boxes": torch.full((rows, 4), FSENT, device=dev), "scores": torch.full((rows,), FSENT, device=dev),
                    "class": torch.full((rows,), ISENT, dtype=torch.int32, device=dev),
                    "image": torch.full((rows,), ISENT, dtype=torch.int32, device=dev),
                    "anchor": torch.full((rows,), ISENT, dtype=torch.int64, device=dev),
                    "counts": torch.full((2 + case.n + GUARD_ROWS,), ISENT, dtype=torch.int64, device=dev)}

    def plan(self):
        import _rn
        pl = _rn.DetPlan()
        nl = 0 if self.levels is None else len(self.levels)
        st = self.L.rn_detect_plan(self.levels, nl, C.byref(self.par), C.byref(pl))
        row = (_rn.DET_SCANS[pl.scan], pl.scan_half, pl.scan_logit, pl.scan_q, pl.scan_lds_per_wave, pl.scan_grid, pl.offsets_blocks,
               _rn.DET_EMITS[pl.emit_mode], pl.emit_grid, pl.emit_lds_bytes, _rn.DET_SEGMENTS.get(pl.segments), pl.nseg)
        return st, row, int(pl.workspace_bytes)

    def workspace_bytes(self):
        if self.levels is None:
            return int(self.L.rn_nms_classwise_workspace(C.byref(self.par)))
        return int(self.L.rn_detect_workspace(self.levels, len(self.levels), C.byref(self.par)))

    def launch(self, ws, ws_bytes):
        """-> the entry point's status (synchronised)"""
        import _rn
        o = self.out
        outs = [o["boxes"].data_ptr(), o["scores"].data_ptr(), o["class"].data_ptr(), o["image"].data_ptr(), o["anchor"].data_ptr(),
                o["counts"].data_ptr()]
        if self.levels is None:
            st = self.L.rn_nms_classwise(*[x.data_ptr() for x in self.inputs], C.byref(self.par), *outs, ws.data_ptr(), ws_bytes, _rn.stream())
        else:
            fn = self.L.rn_boxes_decode if self.case.entry == "boxes_decode" else self.L.rn_detect
            st = fn(self.levels, len(self.levels), C.byref(self.par), *outs, ws.data_ptr(), ws_bytes, _rn.stream())
        torch.cuda.synchronize()
        return st

    def untouched(self):
        return all(bool((v == (FSENT if v.dtype == torch.float32 else ISENT)).all()) for v in self.out.values())

    def check_guards(self, ws, need):
        assert bool((ws[need:] == 0xA5).all()), "the call wrote behind its workspace"
        for k, v in self.out.items():
            tail = v[2 + self.case.n:] if k == "counts" else v[self.cap:]
            assert bool((tail == (FSENT if v.dtype == torch.float32 else ISENT)).all()), "the call wrote behind the capacity of " + k
        for a, b in zip(self.inputs, self.keep):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input changed"


def run_case(case, inputs, dev, expect=None):
    """One call (and a second one on the same buffers) -> dict of numpy arrays: the first counts[1] rows of every output, `counts`.
    expect: the plan row the call must take (None: not asserted)."""
    import _rn
    call = Call(case, inputs, dev)
    st, row, plan_ws = call.plan()
    need = call.workspace_bytes()
    assert st == 0 and plan_ws == need > 0
    if expect is not None:
        assert row == expect, "the call takes %s, not %s" % (row, expect)
    if case.entry != "nms_classwise":
        assert need == R.plan_ref(case)["workspace"] or "capacity" in inputs
    ws = torch.full((need + GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=dev)
    _rn.check(call.launch(ws, need), case.entry)
    call.check_guards(ws, need)
    first = {k: v.clone() for k, v in call.out.items()}
    counts = first["counts"][:2 + case.n].cpu().numpy()
    over = counts[0] > call.cap
    if not over:
        kept = int(counts[1])
        assert 0 <= kept <= call.cap
        for k, v in first.items():           # rows the call does not own keep the sentinel
            if k != "counts":
                assert bool((v[kept:call.cap] == (FSENT if v.dtype == torch.float32 else ISENT)).all()), "rows behind counts[1] of %s were written" % k
        _rn.check(call.launch(ws, need), case.entry)
        call.check_guards(ws, need)
        for k, v in call.out.items():
            assert torch.equal(v.view(torch.uint8), first[k].view(torch.uint8)), "the second call gave other bytes in " + k
    else:
        kept = 0
    got = {k: v[:kept].cpu().numpy() for k, v in first.items() if k != "counts"}
    got["counts"] = counts
    return got


def device_decode(case, inputs, dev):
    """entry detect_raw: the boxes of every row through rn_decode_boxes (the identity the header states: the emit pass decodes a
    candidate with the same arithmetic, same bits), per level [n, rows, 4]; held against the oracle's decode here"""
    import _rn
    out = []
    for lv, reg, anc in zip(case.levels, inputs["regs"], inputs["anchors"]):
        r = torch.from_numpy(reg.astype(np.float32)).to(dev)
        a = torch.from_numpy(anc).to(dev)
        b = torch.empty_like(r)
        _rn.check(_rn.lib().rn_decode_boxes(r.data_ptr(), a.data_ptr(), b.data_ptr(), case.n, lv.h, lv.w, lv.A, _rn.stream()), "rn_decode_boxes")
        out.append(b.cpu().numpy().reshape(case.n, lv.rows, 4))
    for b, want in zip(out, R.decode_boxes_ref(inputs, case)):
        assert np.allclose(b, want, rtol=1e-5, atol=1e-6)
    return out


def survivor_logits(case, inputs, image, anchor):
    """fp64 row maximum of the stored values behind every survivor, and whether its level holds logits"""
    z, is_logit = np.zeros(len(anchor)), np.zeros(len(anchor), bool)
    offs = np.cumsum([0] + [lv.rows for lv in case.levels])
    for k, (i, a) in enumerate(zip(image, anchor)):
        l = int(np.searchsorted(offs, a, side="right") - 1)
        z[k] = inputs["probs"][l][i, a - offs[l]].astype(np.float64).max()
        is_logit[k] = case.levels[l].logit
    return z, is_logit


def check_case(name, dev):
    case = R.CASES[name]
    inputs = R.make_case_cached(case)
    got = run_case(case, inputs, dev, EXPECT[name])
    if case.entry == "detect_raw":
        ref = R.run_ref(case, inputs, boxes=device_decode(case, inputs, dev))
    else:
        ref = R.run_ref_cached(case)
    if name.startswith("det-overcap"):       # the contract: the true count is reported, the call succeeds, nothing behind the capacity is written
        assert got["counts"][0] == ref["counts"][0] > R.capacity(case)
        return
    assert np.array_equal(got["counts"], ref["counts"]), (got["counts"], ref["counts"])
    for k in ("class", "image", "anchor", "boxes"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    logit = any(lv.logit for lv in case.levels)
    if not logit:
        assert np.array_equal(got["scores"].view(np.uint32), ref["scores"].view(np.uint32))      # (bits: -0.0 stays -0.0)
    else:
        assert np.abs(got["scores"].astype(np.float64) - ref["scores"].astype(np.float64)).max() <= SCORE_BAR
        z, is_logit = survivor_logits(case, inputs, got["image"], got["anchor"])
        assert np.array_equal(got["scores"][~is_logit], ref["scores"][~is_logit])
        err = np.abs(got["scores"].astype(np.float64) - R.sigmoid64(z))[is_logit].max()
        print("DETECT_ERR %-28s %.3e" % (name, err))
        assert err <= SCORE_BAR


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items() if not c.process and c.recipe != "adversarial"])
def test_case_matches_the_oracle(dev, monkeypatch, name):
    for k in ("RN_SCAN_LDS", "RN_SCAN_NO_LDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in R.CASES[name].env:
        monkeypatch.setenv(k, v)
    check_case(name, dev)


def test_emit_modes_agree(dev):
    """the two walks of the emit pass on the same input: the same survivors"""
    for tag in ("off2", "off10"):
        h, s = R.CASES["det-%s-hist" % tag], R.CASES["det-%s-strided" % tag]
        inputs = R.make_case_cached(h)
        a = run_case(h, inputs, dev, EXPECT["det-%s-hist" % tag])
        b = run_case(s, inputs, dev, EXPECT["det-%s-strided" % tag])
        assert a["counts"][1] > 0
        for k in a:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items() if c.recipe == "adversarial"])
def test_adversarial_logit_rows(dev, monkeypatch, name):
    """The max-logit shortcut of every scan family on rows built to break it.  Expected: the product's stand-alone sigmoid
    kernel followed by the same call in probability mode (the identity include/rn_hip.h states; that scan is pinned to the oracle
    by the other cases), bit for bit.  Against fp64: the chosen class's logit lies within the documented margin
    5e-7 (1 + e^m) + 1e-6 |m| of the row maximum m (or both lie above 16), and the score within 1e-6 of sigmoid(m)."""
    import _rn
    case = R.CASES[name]
    for k in ("RN_SCAN_LDS", "RN_SCAN_NO_LDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    inputs = R.make_case_cached(case)
    got = run_case(case, inputs, dev, EXPECT[name])
    probs = []
    for z in inputs["probs"]:
        x = torch.from_numpy(z.astype(np.float32)).to(dev)
        y = torch.empty_like(x)
        _rn.check(_rn.lib().rn_act_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _rn.ACT["sigmoid"], _rn.stream()), "rn_act_fwd")
        probs.append(y.cpu().numpy())
    for k, _ in case.env:
        monkeypatch.delenv(k, raising=False)
    plain = replace(case, levels=tuple(replace(lv, half=False, logit=False) for lv in case.levels), env=())
    want = run_case(plain, dict(inputs, probs=probs), dev)
    rows = case.n * R.rows_per_image(case)
    assert got["counts"][0] == rows and got["counts"][1] > rows // 2           # threshold 0: every row is a candidate
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    z, _ = survivor_logits(case, inputs, got["image"], got["anchor"])
    offs = np.cumsum([0] + [lv.rows for lv in case.levels])
    chosen = np.array([inputs["probs"][int(np.searchsorted(offs, a, side="right") - 1)][i, a - offs[int(np.searchsorted(offs, a, side="right") - 1)], c]
                       for i, a, c in zip(got["image"], got["anchor"], got["class"])], np.float64)
    margin = 5e-7 * (1 + np.exp(z)) + 1e-6 * np.abs(z)
    assert np.all((chosen >= z - margin) | ((chosen > 16) & (z > 16)))
    err = np.abs(got["scores"].astype(np.float64) - R.sigmoid64(z)).max()
    print("DETECT_ERR %-28s %.3e" % (name, err))
    assert err <= SCORE_BAR


def _child(names):
    dev = torch.device("cuda:0")
    for name in names:
        check_case(name, dev)
        print("CHILD_OK " + name)


@pytest.mark.parametrize("switch", ["RN_SCAN_T", "RN_SCAN_NT"])
def test_switches_read_once_per_process(dev, switch):
    names = [k for k, c in R.CASES.items() if c.process and dict(c.env).get(switch) == "0"]
    assert len(names) == 2
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [os.path.dirname(here), os.path.join(os.path.dirname(here), "retinanet-tensorflow_amd"), here]
    code = "import sys; sys.path[:0] = %r; import test_gpu_detect_cases as G; G._child(%r)" % (paths, names)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for name in names:
        assert "CHILD_OK " + name in r.stdout


def test_refusals_launch_nothing(dev):
    """max_per_class above the NMS kernel's kept list: RN_EUNSUPPORTED; a workspace one byte short: RN_EWORKSPACE; in both the
    outputs and the workspace still hold their sentinels"""
    case = R.CASES["scan-f32-c36-p"]
    inputs = R.make_case_cached(case)
    call = Call(replace(case, max_per_class=1025), inputs, dev)
    assert call.plan()[0] == RN_EUNSUPPORTED and call.workspace_bytes() == 0
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=dev)
    assert call.launch(ws, ws.numel()) == RN_EUNSUPPORTED
    assert call.untouched() and bool((ws == 0xA5).all())
    call = Call(case, inputs, dev)
    need = call.workspace_bytes()
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    assert call.launch(ws, need - 1) == RN_EWORKSPACE
    assert call.untouched() and bool((ws == 0xA5).all())
    nms = R.CASES["nms-chains"]
    call = Call(replace(nms, max_per_class=1025), R.make_case_cached(nms), dev)
    assert call.launch(ws, ws.numel()) == RN_EUNSUPPORTED and call.untouched()
    call = Call(nms, R.make_case_cached(nms), dev)
    assert call.launch(ws, call.workspace_bytes() - 1) == RN_EWORKSPACE and call.untouched()
