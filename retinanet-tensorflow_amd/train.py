"""Training step for the RetinaNet hot path (step semantics of reference train.py:111-134,
206-243, 261-273) -- the Estimator / CLI / summary plumbing around it is out of scope.

  model_fn composition   train.py:206-243  ->  Trainer.forward_backward(): net -> process_labels_and_logits
                                               -> losses.loss -> (+ L2 regulariser, folded into the
                                               optimizer kernel as wd*w, value from rn_grad_norm_l2reg)
  build_train_step       train.py:111-134  ->  Trainer.apply(): fused optimizer kernel on one flat arena
  MirroredStrategy       train.py:261-267  ->  one process per GPU; gradients averaged with ONE RCCL
                                               all-reduce per bucket over xGMI (torch.distributed 'nccl')

MI355X-first design: all parameters, gradients and optimizer slots live in three flat fp32
arenas (one allocation each, per-parameter padding to 1024 elements) so that the optimizer is a
single kernel, the gradient all-reduce is a few large contiguous messages sized for per-link
xGMI bandwidth, and the whole step (forward, loss, backward, optimizer) can be captured into one
hipGraph -- the launch-bound small kernels of the pyramid's coarse levels then cost no host time.
"""
import collections
import contextlib
import ctypes
import gc
import math
import os
import sys
import time

import numpy as np
import torch

import _rn
import layers as L
import losses
import ops
import utils
from levels import build_levels

OPT_BLOCK = _rn.OPT_BLOCK
FUSED_OPT_NORM = os.environ.get("RN_FUSED_OPT_NORM", "1") == "1"     # (tuning aids; both parity-neutral)


class ParamArena(object):
    """Flat fp32 storage for every parameter of `model` (and its gradients).

    Each parameter is re-pointed to a view of `self.weights`; `param.grad` is a view of
    `self.grads`.  Every parameter starts on a 1024-element boundary so the optimizer / norm
    kernels can look the L2 scale up per block."""

    def __init__(self, model, device):
        params = [p for p in model.parameters() if p.requires_grad]
        sizes = [p.numel() for p in params]
        padded = [(s + OPT_BLOCK - 1) // OPT_BLOCK * OPT_BLOCK for s in sizes]
        self.count = int(sum(padded))
        self.num_params = int(sum(sizes))
        self.weights = torch.zeros(self.count, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.count, dtype=torch.float32, device=device)
        wd = np.zeros(self.count // OPT_BLOCK, dtype=np.float32)
        self.offsets = []
        off = 0
        for p, s, ps in zip(params, sizes, padded):
            view = self.weights[off:off + s].view(p.shape)
            view.copy_(p.data.to(device))
            scale = float(getattr(p, 'l2_scale', 0.0))
            p.data = view
            p.grad = self.grads[off:off + s].view(p.shape)
            wd[off // OPT_BLOCK:(off + ps) // OPT_BLOCK] = scale
            self.offsets.append((off, s))
            off += ps
        self.params = params
        self.wd_per_block = torch.from_numpy(wd).to(device)

    def zero_grad(self):
        if self.grads.is_cuda:          # our own kernel: no PyTorch kernel inside the step
            _rn.check(_rn.lib().rn_zero(_rn.f32(self.grads), self.grads.numel(), _rn.stream()), "rn_zero")
        else:
            self.grads.zero_()


class LRSchedule(object):
    """The learning rate as a function of s, the number of updates already applied (the reference trains at one constant rate;
    its TODO list: "try other scheduling schemes").  W = warmup_steps, f0 = warmup_factor, T = total_steps, ff = final_factor:

        s <  W             base * (f0 + (1 - f0) * s / W)
        s >= W  constant   base
                step       base * decay_factor ** #{boundaries b <= s}
                cosine     base * (ff + (1 - ff) * 0.5 * (1 + cos(pi * min(1, (s - W) / (T - W)))))

    in float64, rounded to float32 once.  rn_step_control_eval evaluates the same descriptor on the device (struct()), where a
    replayed graph advances it by itself; value(s) is the host's copy of the formula (launch arguments of a CPU arena's update,
    logging, tests).  Immutable and hashable: it is part of the one-graph step's cache key."""

    KINDS = ('constant', 'step', 'cosine')
    MAX_BOUNDARIES = _rn.LR_MAX_BOUNDARIES

    def __init__(self, kind='constant', base_lr=1e-2, warmup_steps=0, warmup_factor=1.0 / 3.0, boundaries=(), decay_factor=0.1,
                 total_steps=None, final_factor=0.0):
        if kind not in self.KINDS:
            raise ValueError("lr schedule: kind %r is none of %s" % (kind, ', '.join(self.KINDS)))
        boundaries = tuple(int(b) for b in boundaries)
        warmup_steps = int(warmup_steps)
        total_steps = None if total_steps is None else int(total_steps)
        if warmup_steps < 0:
            raise ValueError("lr schedule: warmup_steps %d < 0" % warmup_steps)
        if not (0.0 <= warmup_factor <= 1.0 and 0.0 <= final_factor <= 1.0):
            raise ValueError("lr schedule: warmup_factor %g and final_factor %g must lie in [0, 1]" % (warmup_factor, final_factor))
        if len(boundaries) > self.MAX_BOUNDARIES:
            raise ValueError("lr schedule: %d boundaries, at most %d" % (len(boundaries), self.MAX_BOUNDARIES))
        if any(b < 0 for b in boundaries) or any(b <= a for a, b in zip(boundaries, boundaries[1:])):
            raise ValueError("lr schedule: boundaries %s are not non-negative and strictly increasing" % (boundaries,))
        if boundaries and kind != 'step':
            raise ValueError("lr schedule: boundaries belong to kind 'step' (got %r)" % kind)
        if kind == 'cosine' and total_steps is None:
            raise ValueError("lr schedule: kind 'cosine' needs total_steps")
        if total_steps is not None and total_steps <= warmup_steps:
            raise ValueError("lr schedule: total_steps %d is not above warmup_steps %d" % (total_steps, warmup_steps))
        self._key = (kind, float(base_lr), warmup_steps, float(warmup_factor), boundaries, float(decay_factor), total_steps,
                     float(final_factor))

    kind = property(lambda self: self._key[0])
    base_lr = property(lambda self: self._key[1])
    warmup_steps = property(lambda self: self._key[2])
    warmup_factor = property(lambda self: self._key[3])
    boundaries = property(lambda self: self._key[4])
    decay_factor = property(lambda self: self._key[5])
    total_steps = property(lambda self: self._key[6])
    final_factor = property(lambda self: self._key[7])

    def __hash__(self):
        return hash(self._key)

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self._key == other._key

    def __ne__(self, other):
        return not self == other

    def __repr__(self):
        return "LRSchedule(kind=%r, base_lr=%r, warmup_steps=%r, warmup_factor=%r, boundaries=%r, decay_factor=%r, " \
               "total_steps=%r, final_factor=%r)" % self._key

    def value(self, s):
        kind, base, W, f0, bounds, decay, T, ff = self._key
        s = int(s)
        if s < W:
            lr = base * (f0 + (1.0 - f0) * s / W)
        elif kind == 'step':
            lr = base * decay ** sum(1 for b in bounds if b <= s)
        elif kind == 'cosine':
            lr = base * (ff + (1.0 - ff) * 0.5 * (1.0 + math.cos(math.pi * min(1.0, (s - W) / float(T - W)))))
        else:
            lr = base
        return np.float32(lr)

    def struct(self):
        """rn_lr_schedule of include/rn_hip.h: the `schedule` field of rn_step_control."""
        kind, base, W, f0, bounds, decay, T, ff = self._key
        d = _rn.LrSchedule(kind=self.KINDS.index(kind), n_boundaries=len(bounds), base_lr=base, warmup_factor=f0,
                           final_factor=ff, decay_factor=decay, warmup_steps=W, total_steps=T or 0)
        for i, b in enumerate(bounds):
            d.boundaries[i] = b
        return d


class Optimizer(object):
    """tf.train.MomentumOptimizer(lr, 0.9) | RMSPropOptimizer(lr, 0.9, 0.9) | AdamOptimizer(lr) (train.py:114-119) + optional
    tf.clip_by_global_norm (train.py:127-132) on the flat arena.  Every configuration takes ONE sequence per call of step():

        count_step     the host's count of updates
        norm ahead     rn_grad_norm_partial + rn_norm_reg_finalize -> norm_reg, where the norm is an INPUT of what follows:
                       grad_clip_norm (RN_OPT_F_CLIP) and skip_nonfinite (RN_OPT_F_GATE); one more pass over w and g
        control        ONE rn_step_control_eval, built once here (`_control`; None: no launch): every device word the update reads
        update         rn_optimizer_update with `_features`, over the arena or per slice (step_slice)
        finalize       rn_norm_reg_finalize -> norm_reg, where the update formed the norm beside itself (RN_OPT_F_NORM)

    begin_step is the first three, step_slice the update, finish_step the rest.  Nothing in it allocates, synchronises or reads a
    device value, and on a device arena no launch argument changes from step to step -- but Adam's / RMSProp's rate without a
    schedule (Trainer._whole_step_ok) -- so the sequence is recorded into the one-graph step as it is launched eagerly.

    What the control launch keeps, each behind its constructor argument (formulas: include/rn_hip.h, rn_step_control):
      `schedule` (LRSchedule)  lr_dev = [lr(s), the rate the update multiplies by: Adam's bias correction included] from the step
        word step_dev, which it advances.  `lr` stays the base rate; current_lr() is the host's copy.
      `ema_decay` D in (0, 1), `ema_warmup`  ema_dev = [d(n), 1 - d(n)] from the average's own word ema_updates_dev; the update keeps
        `ema`, tf.train.ExponentialMovingAverage of the weights, in the same pass.
      `accumulate_steps` A > 1 (no clipping, no guard)  accum_dev = [p, p == A - 1] from the micro-step word micro_dev.  step() is a
        MICRO-step: the update sums the gradient into `acc` (+4 B per parameter) and applies the mean on every A-th one.  On a
        micro-step that only sums, norm_reg keeps the last update's values; the dropout counter advances every micro-step.
      `skip_nonfinite`  gate_dev = [0, norm_reg[0] finite] and skipped_dev = [updates skipped in all, in a row].  A skipped update
        leaves w, the slots, ema and every word of the schedule and the average bit-untouched; the dropout counter advances and
        norm_reg shows the offending norm.  With several ranks the norm is the reduced gradient's: all ranks decide alike.
    Schedule and average run behind the phase's or the guard's gate, so step_count, step_dev, ema_updates_dev and Adam's bias
    correction count APPLIED updates.  The host never reads a device word inside a step: under the guard step_count runs ahead by
    the skips it has not seen until reconcile_skips() (which synchronises) subtracts them.  Guarded Adam / RMSProp given no
    schedule get LRSchedule('constant', learning_rate), so that the bias correction counts on the device.

    A CPU arena or RN_FUSED_OPT_NORM=0 is the same sequence with the norm ahead from rn_grad_norm_l2reg (its own workspace and
    summation order) and the rate a launch argument evaluated on the host: no schedule part in the control launch."""

    def __init__(self, arena, kind='momentum', learning_rate=1e-2, grad_clip_norm=None, schedule=None, ema_decay=None,
                 ema_warmup=True, accumulate_steps=1, skip_nonfinite=False):
        assert kind in ['momentum', 'adam', 'rmsprop']
        self.arena, self.kind, self.lr = arena, kind, float(learning_rate)
        self.clip = float(grad_clip_norm) if grad_clip_norm is not None else 0.0
        dev = arena.weights.device
        if isinstance(accumulate_steps, bool) or not isinstance(accumulate_steps, (int, np.integer)) or accumulate_steps < 1:
            raise ValueError("accumulate_steps %r is not an integer >= 1" % (accumulate_steps,))
        self.accumulate_steps = int(accumulate_steps)
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.skip_nonfinite and self.accumulate_steps > 1:
            raise ValueError("skip_nonfinite with accumulate_steps > 1: a poisoned micro-step would need a decision per cycle, which "
                             "is not implemented")
        if self.skip_nonfinite and (dev.type != 'cuda' or not FUSED_OPT_NORM):
            raise _rn.RnError("skip_nonfinite gates the device's update kernel on the device's norm: it needs a device arena and "
                              "RN_FUSED_OPT_NORM=1")
        if self.skip_nonfinite and schedule is None and kind != 'momentum':
            # the bias correction (and with it the rate the update multiplies by) must count APPLIED updates: from the device
            schedule = LRSchedule('constant', self.lr)
        if self.accumulate_steps > 1 and self.clip > 0.0:
            raise ValueError("accumulate_steps > 1 with grad_clip_norm: the clipped update takes the norm as an input, and clipping "
                             "an accumulated gradient is not implemented")
        if self.accumulate_steps > 1 and (dev.type != 'cuda' or not FUSED_OPT_NORM):
            raise _rn.RnError("gradient accumulation is kept by the device's fused update kernel: it needs a device arena and "
                              "RN_FUSED_OPT_NORM=1")
        self.schedule = schedule
        if schedule is not None:
            assert isinstance(schedule, LRSchedule)
            self.lr = schedule.base_lr
        # allocated HERE like _partial below (a lazy zero-fill inside a step would not be ordered against a side stream's slice)
        self.step_dev = self.lr_dev = None
        if schedule is not None and dev.type == 'cuda':
            self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)        # (the kernel's uint64: same bits)
            self.lr_dev = torch.zeros(2, dtype=torch.float32, device=dev)
        # the moving average and its two device words: HERE as well, for the same reason (e starts as the weights as they are now)
        self.ema_decay, self.ema_warmup = (None if ema_decay is None else float(ema_decay)), bool(ema_warmup)
        self.ema = self.ema_updates_dev = self.ema_dev = None
        if self.ema_decay is not None:
            if not 0.0 < self.ema_decay < 1.0:
                raise ValueError("ema_decay %r is not inside (0, 1)" % (ema_decay,))
            if dev.type != 'cuda':
                raise _rn.RnError("the moving average of the weights is kept by the device's update kernel: it needs a device arena")
            self.ema = arena.weights.clone()
            self.ema_updates_dev = torch.zeros(1, dtype=torch.int64, device=dev)    # (the kernel's uint64: same bits)
            self.ema_dev = torch.zeros(2, dtype=torch.float32, device=dev)
        self.state1 = torch.ones_like(arena.weights) if kind == 'rmsprop' else torch.zeros_like(arena.weights)
        self.state2 = torch.zeros_like(arena.weights) if kind != 'momentum' else None
        self.norm_reg = torch.zeros(2, dtype=torch.float32, device=dev)   # [sum g'^2, L2 reg loss]
        # (sum g'^2, regulariser) pairs of the slices of a step: allocated HERE, not lazily in begin_step -- a first-step zero-fill
        # on the main stream would not be ordered against a side stream's slice update that writes its pairs
        self._pairs = 0
        self._partial = None
        if dev.type == 'cuda':
            n = 4 * int(_rn.lib().rn_optimizer_norm_pairs(arena.count)) + 16
            self._partial = torch.zeros(2 * n, dtype=torch.float64, device=dev)
        # the sum of a cycle's gradients and the two device words of its phase: HERE as well, for the same reason
        self.acc = self.micro_dev = self.accum_dev = None
        self._phase = 0                 # the host's mirror of micro_dev % A: micro-steps of the current cycle already summed
        if self.accumulate_steps > 1:
            self.acc = torch.zeros_like(arena.weights)
            self.micro_dev = torch.zeros(1, dtype=torch.int64, device=dev)          # (the kernel's uint64: same bits)
            self.accum_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        # the guard's gate and its two counters: HERE as well, for the same reason
        self.gate_dev = self.skipped_dev = None
        self._skips_seen = 0            # skipped updates the host's step_count has been corrected for (reconcile_skips)
        if self.skip_nonfinite:
            self.gate_dev = torch.zeros(2, dtype=torch.int32, device=dev)
            self.skipped_dev = torch.zeros(2, dtype=torch.int64, device=dev)        # (the kernel's uint64 pair: same bits)
        # the path is fixed by now (step): behind the gate | the norm beside the update | the norm ahead of it (clipped, or not fused)
        fused = self._fused = dev.type == 'cuda' and FUSED_OPT_NORM
        self._features = ((_rn.OPT_F_GATE if self.skip_nonfinite else _rn.OPT_F_NORM if fused and self.clip <= 0.0 else 0)
                          | (_rn.OPT_F_CLIP if self.clip > 0.0 else 0)
                          | (_rn.OPT_F_LRDEV if fused and self.lr_dev is not None else 0)   # (not fused: the host evaluates the schedule)
                          | (_rn.OPT_F_EMA if self.ema is not None else 0) | (_rn.OPT_F_ACCUM if self.acc is not None else 0))
        # ... and so is the control launch: nothing in its descriptor changes from step to step (None: nothing to launch)
        c = _rn.StepControl(optimizer_kind=_rn.OPT[kind])
        if self.acc is not None:
            c.features |= _rn.CTL_F_ACCUM
            c.accumulate_steps, c.micro_dev, c.accum_dev = self.accumulate_steps, self.micro_dev.data_ptr(), self.accum_dev.data_ptr()
        if self.skip_nonfinite:
            c.features |= _rn.CTL_F_GUARD
            c.norm_sq, c.gate_dev, c.skipped_dev = _rn.f32(self.norm_reg), self.gate_dev.data_ptr(), self.skipped_dev.data_ptr()
        if self._features & _rn.OPT_F_LRDEV:
            c.features |= _rn.CTL_F_LR
            c.schedule, c.step_dev, c.lr_dev = schedule.struct(), self.step_dev.data_ptr(), _rn.f32(self.lr_dev)
        if self.ema is not None:
            c.features |= _rn.CTL_F_EMA
            c.ema_decay, c.ema_warmup = self.ema_decay, int(self.ema_warmup)
            c.ema_updates_dev, c.ema_dev = self.ema_updates_dev.data_ptr(), _rn.f32(self.ema_dev)
        self._control = c if c.features else None
        self._control_event = None      # behind the control launch: what a slice on a side stream waits for
        self.step_count = 0

    def _update(self, lo, hi, grad_scale, advance_counter, partial=None, stream=None):
        """rn_optimizer_update over [lo, hi) of the arena with this optimizer's features; only the fields of set features are filled.
        `lr` / `step` are what begin_step left: this update's rate from the host and its 1-based number (Adam's bias correction),
        both read only without RN_OPT_F_LRDEV."""
        a, f = self.arena, self._features
        u = _rn.OptUpdate(kind=_rn.OPT[self.kind], features=f, w=a.weights[lo:].data_ptr(), grad=a.grads[lo:].data_ptr(),
                          state1=self.state1[lo:].data_ptr(), state2=self.state2[lo:].data_ptr() if self.state2 is not None else None,
                          wd_per_block=a.wd_per_block[lo // OPT_BLOCK:].data_ptr(), count=hi - lo,
                          lr=self._host_lr, grad_scale=grad_scale, step=self._update_no,
                          advance_counter=advance_counter.data_ptr() if advance_counter is not None else None,
                          advance_by=ops.DROPOUT_COUNTER_STEP)
        if f & _rn.OPT_F_NORM:
            u.partial = partial.data_ptr()
        if f & _rn.OPT_F_LRDEV:
            u.lr_dev = _rn.f32(self.lr_dev)
        if f & _rn.OPT_F_EMA:
            u.ema, u.ema_dev = self.ema[lo:].data_ptr(), _rn.f32(self.ema_dev)
        if f & _rn.OPT_F_CLIP:
            u.clip_norm, u.norm_sq = self.clip, _rn.f32(self.norm_reg)
        if f & _rn.OPT_F_ACCUM:
            u.acc, u.inv_accum, u.accum_dev = self.acc[lo:].data_ptr(), 1.0 / self.accumulate_steps, self.accum_dev.data_ptr()
        if f & _rn.OPT_F_GATE:
            u.gate_dev = self.gate_dev.data_ptr()
        _rn.check(_rn.lib().rn_optimizer_update(ctypes.byref(u), stream if stream is not None else _rn.stream()), 'rn_optimizer_update')

    def count_step(self):
        """The host's side of one (micro-)step: step_count counts UPDATES, so with accumulate_steps = A it moves on every A-th call.
        Returns whether this call's step applies an update.  begin_step calls it; a replayed graph's owner calls it per replay."""
        if self.acc is None:
            self.step_count += 1
            return True
        applying = self._phase == self.accumulate_steps - 1
        self._phase = (self._phase + 1) % self.accumulate_steps
        if applying:
            self.step_count += 1
        return applying

    def step(self, grad_scale=1.0, advance_counter=None):
        """The sequence of the class docstring over the whole arena.  `advance_counter`: the device word the dropout masks hash;
        bumped by the update kernel itself."""
        self.begin_step(grad_scale)
        self.step_slice(0, self.arena.count, grad_scale, advance_counter)
        self.finish_step()

    def reconcile_skips(self):
        """(updates skipped in all, updates skipped in a row) from the device -- this SYNCHRONISES -- and step_count brought back to
        "updates applied": the skips the host had not seen yet are subtracted.  (0, 0) without the guard, and no synchronisation."""
        if self.skipped_dev is None:
            return 0, 0
        total, consecutive = (int(v) for v in self.skipped_dev.tolist())
        self.step_count -= total - self._skips_seen
        self._skips_seen = total
        return total, consecutive

    def set_skipped(self, total):
        """Updates skipped so far (a restored checkpoint): the device's counter and what the host has accounted for; the run of
        consecutive skips starts again at 0."""
        if self.skipped_dev is not None:
            self.skipped_dev[0] = int(total)
            self.skipped_dev[1] = 0
            self._skips_seen = int(total)

    # -- the three pieces of the sequence.  Trainer-side callers drive them directly to update the arena in slices (RN_OPT_F_NORM
    # only): the heads + FPN slice on a side stream while the backbone's backward pass still runs, the rest after it; every slice's
    # launch leaves its share of (sum g'^2, regulariser)
    def begin_step(self, grad_scale=1.0):
        """count_step, the norm where it is formed ahead of the update (`grad_scale` is read only there), the control launch."""
        a, L_ = self.arena, _rn.lib()
        self._host_lr = self.current_lr()           # this update's rate where it is a launch argument: before the count moves
        applying = self.count_step()                # (under the guard reconcile_skips takes the skipped ones out again)
        # (the update this micro-step's cycle ends in, 1-based: Adam's bias correction where the rate is a launch argument)
        self._update_no = self.step_count if applying else self.step_count + 1
        self._pairs = 0
        if not self._fused:
            # a CPU arena or RN_FUSED_OPT_NORM=0: the norm pass sizes its own workspace
            ws = _rn.workspace(L_.rn_optimizer_workspace(a.count), a.weights.device)
            _rn.check(L_.rn_grad_norm_l2reg(_rn.f32(a.weights), _rn.f32(a.grads), _rn.f32(a.wd_per_block), a.count,
                                            grad_scale, _rn.f32(self.norm_reg), ws.data_ptr(), ws.numel(), _rn.stream()),
                      'rn_grad_norm_l2reg')
        elif not self._features & _rn.OPT_F_NORM:
            self._pairs = int(L_.rn_optimizer_norm_pairs(a.count))
            assert 2 * self._pairs <= self._partial.numel()
            _rn.check(L_.rn_grad_norm_partial(_rn.f32(a.weights), _rn.f32(a.grads), _rn.f32(a.wd_per_block), a.count, grad_scale,
                                              self._partial.data_ptr(), _rn.stream()), 'rn_grad_norm_partial')
            _rn.check(L_.rn_norm_reg_finalize(self._partial.data_ptr(), self._pairs, _rn.f32(self.norm_reg), _rn.stream()),
                      'rn_norm_reg_finalize')
        if self._control is not None:
            # on the main stream ahead of every slice; the kernel advances the words it reads itself
            _rn.check(L_.rn_step_control_eval(ctypes.byref(self._control), _rn.stream()), 'rn_step_control_eval')
            if self._features & _rn.OPT_F_NORM:
                self._control_event = torch.cuda.Event()
                self._control_event.record()

    def step_slice(self, lo, hi, grad_scale, advance_counter=None, stream=None):
        a = self.arena
        assert 0 <= lo < hi <= a.count and lo % OPT_BLOCK == 0 and hi % OPT_BLOCK == 0
        part = None
        if self._features & _rn.OPT_F_NORM:
            npairs = int(_rn.lib().rn_optimizer_norm_pairs(hi - lo))
            assert 2 * (self._pairs + npairs) <= self._partial.numel()
            part = self._partial[2 * self._pairs:]
            self._pairs += npairs
        else:
            assert (lo, hi) == (0, a.count), "slices form the norm beside the update: not with clipping, the guard or a CPU arena"
        if self._control_event is not None and stream is not None:
            # a slice on another stream reads lr_dev / ema_dev / accum_dev too: behind the control launch, not the whole main stream
            other = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(getattr(stream, 'value', stream)))
            other.wait_event(self._control_event)
            stream = ctypes.c_void_p(other.cuda_stream)
        self._update(lo, hi, grad_scale, advance_counter, partial=part, stream=stream)

    def finish_step(self):
        if self._features & _rn.OPT_F_NORM:
            _rn.check(_rn.lib().rn_norm_reg_finalize(self._partial.data_ptr(), self._pairs, _rn.f32(self.norm_reg), _rn.stream()),
                      'rn_norm_reg_finalize')
        import ops_f16
        ops_f16.weights_changed()      # fp16-packed copies of the kernels (inference path) are stale now

    def current_lr(self):
        """The rate of the NEXT update, from the host's step count (no device synchronisation)."""
        return self.lr if self.schedule is None else float(self.schedule.value(self.step_count))

    def set_step_count(self, n):
        """Updates applied so far (a restored checkpoint): the host's count and the device word the schedule kernel reads."""
        self.step_count = int(n)
        if self.step_dev is not None:
            self.step_dev.fill_(self.step_count)
        if self.ema_updates_dev is not None:
            self.ema_updates_dev.fill_(self.step_count)

    def set_accum_micro(self, n):
        """Micro-steps taken so far (a restored checkpoint): the device word the control launch reads and the host's phase."""
        if self.acc is not None:
            self.micro_dev.fill_(int(n))
            self._phase = int(n) % self.accumulate_steps

    def ema_decay_value(self, n):
        """d(n), the decay of the update that follows n applied ones, in float64: the host's copy of what the control launch forms."""
        if self.ema_decay is None:
            raise ValueError("this optimizer keeps no moving average (ema_decay=None)")
        n = int(n)
        return min(self.ema_decay, (1.0 + n) / (10.0 + n)) if self.ema_warmup else self.ema_decay

    @property
    def regularization_loss(self):
        """sum_w scale * ||w||^2 / 2 at the weights used for the last gradient (train.py:221)."""
        return self.norm_reg[1]


class GradientAllReduce(object):
    """MirroredStrategy's cross-replica gradient sum (train.py:261-267) as RCCL all-reduces of
    contiguous arena slices.  xGMI is point-to-point (7 links x ~153 GB/s), ring collectives are
    per-link bound, so a region goes out as FEW LARGE buckets (default 64 MB: the whole 40 MB arena of the
    headline config would be ONE message) rather than one message per tensor; the 1/world_size average is
    folded into the optimizer kernel.

    launch(start, end) enqueues the (asynchronous) all-reduce of grads[start:end] behind the work already
    queued on the current stream and returns at once: the collective runs on the process group's own
    stream while the current stream goes on with the next backward segment; wait() joins."""

    def __init__(self, arena, process_group=None, bucket_bytes=64 << 20, force=False):
        import torch.distributed as dist
        self.dist, self.group, self.arena = dist, process_group, arena
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        # force: issue the collectives even with one rank (self-tests of the RCCL path on a 1-GPU box)
        self.active = self.world > 1 or (bool(force) and dist.is_initialized())
        self.per = max(OPT_BLOCK, (int(bucket_bytes) // 4) // OPT_BLOCK * OPT_BLOCK)
        # a backend without device collectives (gloo: debugging, tests with several processes on one GPU) gets the
        # bucket through host memory, synchronously; the production backend ('nccl' = RCCL) reduces in place in HBM
        self.host_staged = bool(self.active and arena.grads.is_cuda and dist.get_backend(process_group) != 'nccl')
        self.buckets = self.buckets_of(0, arena.count)
        self._works = []
        self.launched = []          # (start, end) of every bucket issued since the last wait(): for tests
        self._capturable = None     # decided once, by doing it: probe_capturable()

    def buckets_of(self, start, end):
        return [(s, min(s + self.per, end)) for s in range(start, end, self.per)]

    @property
    def capturable(self):
        """May launch() / wait() be recorded into a hipGraph (the collectives as nodes of the step's graph)?"""
        return bool(self._capturable)

    def probe_capturable(self, device):
        """Decide -- by doing it, on every rank, with a known answer -- whether this backend's all-reduce can be CAPTURED into a
        hipGraph and replayed: rank r contributes r + 1, a replay must leave world (world + 1) / 2 everywhere, twice (a second
        replay must not reduce the first one's result again).  An exception or a wrong sum on ANY rank (MIN over ranks, eager
        collective) selects the eager collectives between captured segments on EVERY rank.  RN_DP_CAPTURE=0 skips the probe
        (never capture), =1 / auto (default) runs it."""
        if self._capturable is not None:
            return self._capturable
        self._capturable = False
        if (not self.active or self.host_staged or device.type != 'cuda' or os.environ.get("RN_DP_CAPTURE", "auto") == "0"):
            return False
        ok, why = 1.0, ""
        try:
            cur = torch.cuda.current_stream(device)
            buf = torch.full((OPT_BLOCK,), float(self.rank + 1), dtype=torch.float32, device=device)
            self.dist.all_reduce(buf, op=self.dist.ReduceOp.SUM, group=self.group)     # eager first: the communicator connects outside any capture
            torch.cuda.synchronize(device)
            g = torch.cuda.CUDAGraph()
            with _no_gc_while_capturing(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                w = self.dist.all_reduce(buf, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
                w.wait()
            want = float(self.world * (self.world + 1) // 2)
            for _ in range(2):
                buf.fill_(float(self.rank + 1))
                g.replay()
                cur.synchronize()
                if not bool((buf == want).all().item()):
                    ok, why = 0.0, "replayed all-reduce gave %r, expected %r" % (float(buf[0].item()), want)
            del g
        except Exception as e:       # noqa: BLE001 -- any failure means "do not capture", never "abort the run"
            ok, why = 0.0, "%s: %s" % (type(e).__name__, e)
        t = torch.tensor([ok], dtype=torch.float32, device=device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN, group=self.group)
        self._capturable = bool(t.item() == 1.0)
        if not self._capturable and self.rank == 0:
            print("[trainer] collectives are not captured into the step's graph (%s): eager collectives between captured segments"
                  % (why or "another rank's probe failed"), file=sys.stderr, flush=True)
        return self._capturable

    def launch(self, start=0, end=None):
        end = self.arena.count if end is None else end
        if not self.active or end <= start:
            return
        # last bucket first: within a region the later layers' gradients were produced first
        for s, e in reversed(self.buckets_of(start, end)):
            if self.host_staged:
                host = self.arena.grads[s:e].cpu()
                self.dist.all_reduce(host, op=self.dist.ReduceOp.SUM, group=self.group)
                self.arena.grads[s:e].copy_(host)
                self.launched.append((s, e))
                continue
            self._works.append(self.dist.all_reduce(self.arena.grads[s:e], op=self.dist.ReduceOp.SUM, group=self.group,
                                                    async_op=True))
            self.launched.append((s, e))

    def wait(self):
        for w in self._works:
            w.wait()
        del self._works[:]
        return 1.0 / self.world

    def wait_on_current_stream(self):
        """Make the CURRENT stream wait for every collective issued so far (Work.wait() orders the stream, not the host) without
        forgetting them: wait() on the main stream later still covers them."""
        for w in self._works:
            w.wait()

    def __call__(self):
        self.launch(0, self.arena.count)
        return self.wait()


# The captured graphs of one input shape (Trainer._graphs; callers outside this file read the first six by position).
#   whole = False (_capture): `first` is segment A and `parts` / `ranges` one graph and one arena slice per part of segment B;
#     deferred_in_part0: the tower weight gradients are forked and joined inside parts[0], the subnets' slice is complete behind it
#   whole = True (_capture_whole): `first` is the whole step; `ranges` the parts' slices, kept for reporting; `schedule` the
#     slices in the order the recorded step reduces them
StepGraphs = collections.namedtuple('StepGraphs', 'first parts ranges out static whole deferred_in_part0 schedule')


class Trainer(object):
    """One data-parallel replica.  `step(features)` = forward + loss + backward + gradient
    all-reduce + optimizer.

    Backward runs in TWO segments (`overlap=True`): (A) forward, loss and the backward pass of the heads + FPN --
    82 % of the gradient bytes of the headline config, complete first -- then (B) the backward pass of the
    backbone.  The all-reduce of region A's slice of the gradient arena is launched between the two and runs on
    RCCL's stream underneath segment B; only the (small) backbone slice is reduced after it.  The cut is made
    with detached leaves at the backbone taps the FPN reads (RetinaNetBase.backward_cut), so the arithmetic is
    unchanged.  With use_graph=True each segment is one hipGraph (shared memory pool, always replayed A then
    B); the collectives stay eager launches between the replays."""

    def __init__(self, net, levels=None, optimizer='momentum', learning_rate=1e-2, grad_clip_norm=None,
                 loss_mode='bce_dice', device='cuda', use_graph=False, process_group=None,
                 direct_param_grads=True, wgrad_side_stream=False, defer_reductions=True, overlap=True,
                 force_collective=False, input_fn=None, check_interval=50, capture_collectives=None, lr_schedule=None,
                 ema_decay=None, ema_warmup=True, accumulate_steps=1, skip_nonfinite=False, train_metrics=False, regr_loss=None):
        self.net, self.levels = net, levels or build_levels()
        self.device = torch.device(device)
        if self.device.type == 'cuda':
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            # the kernels are launched on the CURRENT device's current stream with raw pointers
            assert torch.cuda.current_device() == self.device.index, \
                "call torch.cuda.set_device(%d) before building the Trainer" % self.device.index
        # (without an lr_schedule Adam's bias-corrected learning rate is a fresh launch argument every step: its update -- and
        # RMSProp's -- is then launched per step, outside the captured segments, also with use_graph=True)
        # loss_mode: 'bce_dice' / 'focal' (None: losses.LOSS_MODE), or a class-loss spec (losses.parse_class_loss: a weighted sum of the reference's terms),
        # parsed here so that a bad one fails before anything is built; the loss stays two nodes of the step's graph either way
        self.loss_mode = loss_mode if (loss_mode is None or loss_mode in _rn.LOSS_MODE) else losses.parse_class_loss(loss_mode)
        # regr_loss: None (the Huber loss of the class-loss kernels), or a regression-loss spec (losses.parse_regr_loss: a weighted sum
        # of Huber, IoU and GIoU terms), parsed here as well; a spec other than 'huber:1:1' adds three nodes to the step's graph
        self.regr_loss = None if regr_loss is None else losses.parse_regr_loss(regr_loss)
        self.arena = ParamArena(net, self.device)
        # lr_schedule (LRSchedule): the rate lives on the device and advances inside the step (Optimizer docstring); None: the
        # constant `learning_rate`, a launch argument
        # ema_decay: the update kernel also keeps a moving average of the weights (Optimizer docstring; ema_weights() runs the net
        # on it).  Its decay is read from the device like a scheduled rate: no host scalar, so nothing about the one-graph step or
        # its cache key changes
        # accumulate_steps A: step() is a micro-step, every A-th one applies the mean of the last A gradients (Optimizer docstring).
        # Phase and gate live on the device as well: the step stays ONE graph, captured once and replayed for every phase; A is part
        # of its cache key.  With several ranks every micro-step's gradient is all-reduced (1 / world applied as it is summed)
        # skip_nonfinite: the update of a step whose global gradient norm is not finite does not happen (Optimizer docstring).  Gate
        # and counters live on the device: the step stays ONE graph, the guard is part of its cache key, and Adam / RMSProp at a
        # constant rate read it from the device then, so they qualify for the one-graph step as with an lr_schedule
        self.opt = Optimizer(self.arena, optimizer, learning_rate, grad_clip_norm, schedule=lr_schedule, ema_decay=ema_decay,
                             ema_warmup=ema_warmup, accumulate_steps=accumulate_steps, skip_nonfinite=skip_nonfinite)
        # train_metrics: the reference's streaming training metrics (build_metrics, train.py:137-161: loss means, class_iou,
        # regr_iou) as running totals on the device (metrics.TrainMetrics).  One pass behind the loss over the tensors it has just
        # read and one block behind the update: two more nodes of the SAME graph(s), or two eager launches; the host reads them only
        # in train_metrics().  They observe: weights, slots and the dropout counter are bit for bit those of a run without them.
        # Every micro-step of accumulate_steps counts as a step; the state is rank-local and not stored in checkpoints
        self.metrics = None
        if train_metrics:
            import metrics as _metrics
            self.metrics = _metrics.TrainMetrics(self.device)        # (raises on a CPU arena)
        self.allreduce = GradientAllReduce(self.arena, process_group, force=force_collective)
        self.use_graph = use_graph
        self.input_fn = input_fn       # optional: features = input_fn(), run INSIDE segment A (e.g. device-side label assignment)
        self.defer_reductions = (bool(defer_reductions) and bool(direct_param_grads) and
                                 os.environ.get("RN_DEFER_REDUCTIONS", "1") == "1")
        # kernels write parameter gradients straight into the arena (every parameter of this network is used by exactly one
        # op call per step; ops._grad_slot refuses a second write); see ops.DIRECT_PARAM_GRADS.  These switches and the dropout
        # counter are process-wide in ops / layers: they are set only while THIS trainer's segments run (_scoped) and restored
        # afterwards, so trainers and plain autograd users in one process do not see each other's settings
        self.direct_param_grads = bool(direct_param_grads)
        # ... which would let the weight-gradient kernels run on a side stream under the dgrad / GroupNorm chain;
        # measured on MI355X: 162 vs 170 img/s (fork/join edges + CU contention cost more than the overlap buys), so off
        self.wgrad_side_stream = bool(direct_param_grads) and bool(wgrad_side_stream)
        # backward segments: arena offset where the FPN's parameters start (arena order = registration order =
        # backbone, fpn, classification_subnet, regression_subnet)
        self.cut_offset = 0
        base = getattr(net, 'base', None)
        if overlap and base is not None and hasattr(base, 'backward_cut') and hasattr(base, 'fpn'):
            first = next(iter(base.fpn.parameters()), None)
            for p, (off, _) in zip(self.arena.params, self.arena.offsets):
                if p is first:
                    self.cut_offset = off
        # (the hook itself -- base.backward_cut -- is installed only while one of this trainer's segments runs: _scoped)
        self._cut_base = base if self.cut_offset else None
        self._cut_src = self._cut_leaves = None
        # ... and the backbone's own backward pass in one part per stage where the backbone offers the cut points (`stage_cut`:
        # ResNeXt / DenseNet, whose 200 / 50 MB of backbone gradients would otherwise all wait for the last backward kernel):
        # part j's slice of the gradient arena is reduced underneath the parts that follow it
        bb = getattr(base, 'backbone', None) if self._cut_base is not None else None
        self._stage_bb = bb if (bb is not None and hasattr(bb, 'stage_cut') and os.environ.get("RN_STAGE_CUTS", "1") == "1") else None
        # (a backbone whose cut costs kernels -- MobileNetV2's chain -- takes it only where a collective is there to hide)
        if self._stage_bb is not None and getattr(bb, 'stage_cut_needs_collective', False) and not self.allreduce.active:
            self._stage_bb = None
        self._stage_cuts = []          # per step: (arena offset, source tensor, detached leaf, names of the taps made before it)
        self._param_offset = {id(p): off for p, (off, _) in zip(self.arena.params, self.arena.offsets)}
        self._parts = []               # per step: (roots, grads-of-leaves getter, arena range) of segment B's parts
        # The head towers' WEIGHT gradients (half of their backward products) beside the backbone's backward pass instead of inside
        # the heads' (ops.WGRAD_DEFER): segment A records them, segment B launches them on a side stream before its own kernels.
        # With several ranks the step keeps them there (round 6): the slice that is complete when segment A ends -- the FPN's,
        # [cut_offset, heads_offset) -- is all-reduced at once, the subnets' slice [heads_offset, count) BEHIND the deferred products
        # on their stream (the collective waits for that stream, not for the backbone's backward pass).  A forked stream must be
        # joined inside the graph that forked it, so with one graph PER PART and eager collectives between them (the fallback when
        # the collectives cannot be captured) the products are forked AND joined inside the first part's graph and the subnets'
        # slice is reduced right behind that part, under the parts that follow.  RN_DEFER_WGRAD=0: off everywhere.
        self.heads_offset = self.arena.count
        if base is not None and hasattr(base, 'classification_subnet'):
            first = next(iter(base.classification_subnet.parameters()), None)
            self.heads_offset = self._param_offset.get(id(first), self.arena.count)
        # One captured graph per step needs nothing between its parts -- or collectives that can themselves be recorded into the
        # graph (GradientAllReduce.probe_capturable decides that by doing it, identically on every rank).
        self.whole_step_graph = os.environ.get("RN_WHOLE_STEP_GRAPH", "1") == "1"
        if capture_collectives is False:          # (A/B aid and fallback: eager collectives between one graph per part)
            self.allreduce._capturable = False
        if self.allreduce.active and use_graph and self.whole_step_graph and self.device.type == 'cuda':
            self.allreduce.probe_capturable(self.device)
        self.defer_wgrad = os.environ.get("RN_DEFER_WGRAD", "1") == "1" and self.device.type == 'cuda' and self.direct_param_grads
        # OPT-IN (RN_WINO_PRE=1; measured SLOWER, kept as the record of the experiment): the Winograd kernel transforms of the head
        # towers' 10 convs once per step on a side stream beside the backbone's forward pass, instead of inside every layer's first
        # launch (ops.WinoPretransform).  Same kernels, same values -- the weights do not change between the optimizer's update and
        # the forward pass that follows -- and the layers' launches lose their kernel-transform blocks (upper bound with the
        # transforms skipped altogether: 491 -> 497 - 502 images/s), but ten more launches beside the backbone's latency-bound
        # chain cost more than that: 471 - 485 against 488 - 494 images/s (profiles/r06_ab_runs.txt).
        self.wino_pre = os.environ.get("RN_WINO_PRE", "0") == "1" and self.device.type == 'cuda'
        self._wino_pre = None
        self._deferred_wgrads = []
        self._deferred_running = []
        self._graphs = None
        # input shape key (dataset.DeviceFeed.shape_key; None without a feed) -> captured segments, least recently used first.
        # Every entry owns its graphs' private activation pool and static buffers, so the cache is BOUNDED (RN_GRAPH_CACHE, default 4
        # shapes; a ragged DeviceFeed keys by network input shape, so raw image sizes do not count); a key beyond the bound evicts
        # the least recently used set
        # (its next appearance re-captures: two warm-up passes + capture, logged).
        self._graph_cache = collections.OrderedDict()
        self.graph_cache_max = max(1, int(os.environ.get("RN_GRAPH_CACHE", "4")))
        # The whole step -- segment A, the collectives, every part of segment B, the update -- is ONE captured graph wherever
        # nothing has to happen on the host between its parts: the ~80 us a step the GPU idles at the graph boundaries and in
        # front of an eagerly launched update (profiles/r05_bench_step_timeline.txt: "idle stretches") disappear.  The update's
        # host-side scalars are constants of such a graph: momentum SGD only (no step-dependent scalar), and a changed learning
        # rate or clip value captures again (both are part of the cache key; the clip SCALE is formed on the device from the
        # norm, with or without a schedule).  With an lr_schedule the update has no such scalar -- rate and Adam's bias correction are read from the device -- so RMSProp and Adam qualify too and the schedule,
        # not a rate, is part of the key.  RN_WHOLE_STEP_GRAPH=0: one graph per part.
        self.schedule = []             # the gradient slices of the last recorded / eager step, in the order their all-reduce was issued
        self._last_lr, self._lr_changes = None, 0
        self.recaptures = 0
        self._static = None
        # the device word every fused dropout hashes (bumped by the optimizer kernel); replicas start it at different values
        # so that they draw different masks (each tower of the reference's MirroredStrategy has its own dropout stream)
        self.drop_rank_offset = self.allreduce.rank * 0x632BE59BD9B4E019 % (1 << 62)      # (checkpoints store counter - offset)
        self.drop_counter = torch.full((1,), self.drop_rank_offset, dtype=torch.int64, device=self.device)
        self._one = torch.ones((), dtype=torch.float32, device=self.device)
        self.check_interval = int(check_interval)
        self.steps_done = 0
        self.timing = None             # set to {} to collect 'allreduce_exposed_ms' (events around the final wait)
        self.last = {}

    @contextlib.contextmanager
    def _scoped(self):
        """This trainer's process-wide switches (direct parameter gradients, weight-gradient side stream, dropout counter) for
        the duration of one of its segments."""
        saved = (ops.DIRECT_PARAM_GRADS, ops.WGRAD_SIDE_STREAM, L.Dropout.seed_device_counter)
        ops.DIRECT_PARAM_GRADS, ops.WGRAD_SIDE_STREAM = self.direct_param_grads, self.wgrad_side_stream
        L.Dropout.seed_device_counter = self.drop_counter
        base = self._cut_base
        saved_cut = base.backward_cut if base is not None else None
        saved_stage = self._stage_bb.stage_cut if self._stage_bb is not None else None
        if base is not None:        # plain autograd users of the same net (and other trainers) never see this trainer's cut
            base.backward_cut = self._cut
        if self._stage_bb is not None:
            self._stage_bb.stage_cut = self._stage_cut
        try:
            yield
        finally:
            ops.DIRECT_PARAM_GRADS, ops.WGRAD_SIDE_STREAM, L.Dropout.seed_device_counter = saved
            if base is not None:
                base.backward_cut = saved_cut
            if self._stage_bb is not None:
                self._stage_bb.stage_cut = saved_stage

    # -- replica-local work (capturable)
    def _cut(self, taps):
        """RetinaNetBase.backward_cut: the FPN reads detached leaves; segment B feeds their gradients back."""
        keys = [k for k in ('C3', 'C4', 'C5') if k in taps]
        self._cut_keys = keys
        self._cut_src = [taps[k] for k in keys]
        self._cut_leaves = [t.detach().requires_grad_(True) for t in self._cut_src]
        return {**taps, **dict(zip(keys, self._cut_leaves))}

    def _stage_cut(self, module, x, taps_before=()):
        """<backbone>.stage_cut: the stage that starts with `module` reads a detached leaf (see __init__)."""
        first = next(iter(module.parameters()), None)
        off = self._param_offset.get(id(first)) if first is not None else None
        if off is None or not x.requires_grad or not (0 < off < self.cut_offset):
            return x
        leaf = x.detach().requires_grad_(True)
        self._stage_cuts.append((off, x, leaf, frozenset(taps_before)))
        return leaf

    def _plan_parts(self):
        """Segment B as parts, last stage first: [(roots, leaves whose .grad seeds them, (start, end) of the arena slice complete after it)]."""
        keys, srcs, leaves = self._cut_keys, self._cut_src, self._cut_leaves
        cuts = sorted(self._stage_cuts, key=lambda c: c[0])
        parts, done, hi = [], set(), self.cut_offset
        nxt = None                                     # (source, leaf) of the cut above the part being built
        for off, x, leaf, before in reversed(cuts):
            idx = [i for i, k in enumerate(keys) if k not in before and k not in done]
            done.update(keys[i] for i in idx)
            roots = [srcs[i] for i in idx] + ([nxt[0]] if nxt is not None else [])
            seeds = [leaves[i] for i in idx] + ([nxt[1]] if nxt is not None else [])
            parts.append((roots, seeds, (off, hi)))
            nxt, hi = (x, leaf), off
        idx = [i for i, k in enumerate(keys) if k not in done]
        roots = [srcs[i] for i in idx] + ([nxt[0]] if nxt is not None else [])
        seeds = [leaves[i] for i in idx] + ([nxt[1]] if nxt is not None else [])
        parts.append((roots, seeds, (0, hi)))
        return parts

    def _backward(self, roots, grads, skip_join=()):
        defer = self.defer_reductions and self.device.type == 'cuda' and ops.DIRECT_PARAM_GRADS
        if defer:                                  # ~130 gradient row reductions -> one launch per segment
            import retinanet
            extra = [retinanet.side_stream(self.device)] if retinanet.HEADS_TWO_STREAMS else []
            if ops.WGRAD_SIDE_STREAM:
                extra.append(_rn.side_stream(self.device, 0))
            if os.environ.get("RN_DEFER_SIDE", "1") != "1":
                extra = []
            ops.begin_deferred_reductions(extra)
        try:
            torch.autograd.backward(roots, grads)
        finally:
            if defer:
                ops.end_deferred_reductions()
        # weight-gradient kernels may run on side streams and write straight into the arena: join them before
        # anything (the collective, the optimizer) reads it
        if self.device.type == 'cuda':
            _rn.join_side_streams(self.device, skip=skip_join)

    def segment_a(self, features=None):
        """forward + loss + backward of the heads and the FPN (the whole backward pass when there is no cut)."""
        with self._scoped():
            label_stream = None
            zeroed = False
            if features is None:
                # input_fn builds the step's labels on the device (anchor assignment); only the loss reads them: their
                # kernels run on a side stream underneath the backbone's forward pass (the image itself -- written before
                # the step, not by input_fn -- is read at once).  OPT-IN (input_fn.concurrent = True): an input_fn that also
                # creates / uploads / preprocesses the IMAGE must stay on the main stream, or the backbone would read the image
                # with no ordering against the side stream that writes it.
                if self.device.type == 'cuda' and getattr(self.input_fn, 'concurrent', False):
                    label_stream = _rn.side_stream(self.device, 2)
                    label_stream.wait_stream(torch.cuda.current_stream())
                    main_stream = torch.cuda.current_stream()
                    with torch.cuda.stream(label_stream):
                        features = self.input_fn()
                        # (the gradient arena is cleared here too, underneath the backbone's forward pass, instead of between the
                        # loss and its gradient: nothing reads or writes it before the join in front of the loss)
                        self.arena.zero_grad()
                        zeroed = True
                    _for_each_tensor(features, lambda t: t.record_stream(main_stream) if t.is_cuda else None)   # (allocated on the side stream, read on this one)
                else:
                    features = self.input_fn()
            self._cut_src = self._cut_leaves = None
            self._stage_cuts = []
            self._parts = []
            ops.begin_direct_grad_step()       # a parameter's gradient slot may be written once per step from here on
            pre_ev = self._fork_kernel_transforms()
            try:
                logits = {'detection': self.net(features['image'], training=True)}
            finally:
                ops.WINO_PRE = {}
            if pre_ev is not None:             # (joined even if no layer read them: a captured side stream must rejoin)
                torch.cuda.current_stream().wait_event(pre_ev)
            if label_stream is not None:
                torch.cuda.current_stream().wait_stream(label_stream)
            inp, logits = utils.process_labels_and_logits(labels=features, logits=logits, levels=self.levels)
            class_loss, regr_loss = losses.loss(labels=inp['detection_trainable'], logits=logits['detection_trainable'],
                                                mode=self.loss_mode, regr_mode=self.regr_loss)
            if self.metrics is not None:       # on this stream, before the backward pass: every tensor it reads is alive and ordered
                self.metrics.update(inp['detection_trainable'], logits['detection_trainable'], self.levels,
                                    tuple(features['image'].shape[1:3]))
            # kernels that write a parameter's gradient directly overwrite it; gradients that reach a parameter
            # through autograd (e.g. the concatenated head kernels) are accumulated -> the arena starts at zero
            if not zeroed:
                self.arena.zero_grad()
            # d(class_loss + regr_loss): both roots seeded with the same pre-allocated 1 (no add / fill kernels in the step)
            ops.WGRAD_DEFER = [] if self.defer_wgrad else None
            try:
                self._backward([class_loss, regr_loss], [self._one, self._one])
            finally:
                self._deferred_wgrads, ops.WGRAD_DEFER = (ops.WGRAD_DEFER or []), None
            if self._cut_src is not None:
                self._parts = self._plan_parts()
                self._cut_src = self._cut_leaves = None
                self._stage_cuts = []
            if self._deferred_wgrads and not self._parts:       # no segment B to hide them under: finish them here
                ops.run_deferred_wgrads(self._deferred_wgrads)
                self._deferred_wgrads = []
            return class_loss.detach(), regr_loss.detach()

    PRE_STREAM = 8                     # _rn.side_stream index of the tower kernels' transforms

    def _fork_kernel_transforms(self):
        """Launch the head towers' kernel transforms on their side stream (behind everything queued so far: the optimizer's update of
        the previous step) and publish the buffers for this forward pass (ops.WINO_PRE).  Returns the event behind them, or None."""
        if not self.wino_pre or not (ops.WINO_GN_FOLD and ops.WINOGRAD):
            return None
        if self._wino_pre is None:
            if torch.cuda.is_current_stream_capturing():
                return None                    # (built by the eager steps in front of a capture; never allocate inside one)
            base = getattr(self.net, 'base', self.net)
            subnets = [getattr(base, n, None) for n in ('classification_subnet', 'regression_subnet')]
            kernels = [w for sn in subnets if sn is not None and hasattr(sn, 'tower_kernels') for w in sn.tower_kernels()]
            if not kernels:
                return None
            self._wino_pre = ops.WinoPretransform(kernels)
        side = _rn.side_stream(self.device, self.PRE_STREAM)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.WINO_PRE, ev = self._wino_pre.launch()
        return ev

    def num_parts(self):
        """Parts of segment B planned by the last segment_a (1 without stage cuts, 0 without any cut)."""
        return len(self._parts)

    WGRAD_STREAM = 7                   # _rn.side_stream index of the deferred weight-gradient products

    def segment_b(self, part=None, join_wgrads=True, after_wgrads=None):
        """backward of the backbone from the gradients segment A left at the cut: every part (part=None), or part j of
        num_parts() (last stage first).  Returns the (start, end) arena slice that is complete after it.

        The first call of a step forks the deferred tower weight gradients (segment A's records) onto their side stream;
        `after_wgrads()` runs on that stream behind them (the all-reduce of their slice); `join_wgrads=False` leaves the stream
        un-joined when the call returns -- the caller joins it (_join_wgrads) before anything reads those gradients."""
        if not self._parts:
            return None
        rng = None
        if self._deferred_wgrads:             # the towers' weight-gradient halves: forked off here
            self._fork_wgrads(after_wgrads)
        skip = () if join_wgrads else (self.WGRAD_STREAM,)
        for j in (range(len(self._parts)) if part is None else [part]):
            roots, seeds, rng = self._parts[j]
            with self._scoped():
                self._backward(roots, [l.grad for l in seeds], skip_join=skip)
        if part is None:
            self._parts = []
            return (0, self.cut_offset)
        return rng

    def _fork_wgrads(self, after=None):
        if self.device.type == 'cuda':
            wside = _rn.side_stream(self.device, self.WGRAD_STREAM)
            wside.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(wside):
                ops.run_deferred_wgrads(self._deferred_wgrads)
                if after is not None:
                    after()
        else:                                 # (no streams: tests of the schedule on CPU)
            ops.run_deferred_wgrads(self._deferred_wgrads)
            if after is not None:
                after()
        self._deferred_running = self._deferred_wgrads      # (their workspaces stay allocated until the next step replaces this)
        self._deferred_wgrads = []

    def _join_wgrads(self):
        if self.device.type == 'cuda':
            torch.cuda.current_stream().wait_stream(_rn.side_stream(self.device, self.WGRAD_STREAM))

    def forward_backward(self, features=None, advance_dropout=True):
        """Both segments, no collective, no update.  The dropout counter is bumped here (one tiny launch); step() leaves
        that to the optimizer kernel."""
        out = self.segment_a(features)
        self.segment_b()
        if advance_dropout and self.device.type == 'cuda':
            ops.advance_dropout_counter(self.drop_counter)
        return out

    def _run_step(self, features=None, timed=False, replay=None):
        """The device work of ONE step in issue order -- the same sequence whether it is launched eagerly, recorded into one graph
        or replayed from one graph per part, with one rank or many (MirroredStrategy's per-tower step + cross-tower sum,
        train.py:111-134, 261-267):

            segment A (assignment, forward, loss, backward of the heads and the FPN; tower weight gradients recorded, not run)
            all-reduce  [cut_offset, heads_offset)      the FPN's slice             } under segment B
            fork: deferred tower weight gradients  ->  all-reduce [heads_offset, count) behind them
            for every part j of the backbone's backward pass, last stage first:  part j  ->  all-reduce of its slice
            join, wait for the collectives, optimizer update (1 / world folded in; bumps the dropout counter); with
            grad_clip_norm the norm pass runs here too, behind the wait: the norm of the REDUCED gradient times 1 / world

        `replay` (the StepGraphs of _capture): segment A and the parts are replays of their graphs, not launches.  A forked stream
        must be joined inside the graph that forked it, so part 0's graph holds the deferred products whole and the subnets' slice
        is reduced right behind that replay; launched, it is reduced on the products' own stream, by segment_b's callback.
        `schedule` -- the order the slices' collectives are issued in -- is the same either way.
        Without deferred products the first collective covers [cut_offset, count).  With one rank launch() / wait() do nothing."""
        ar = self.allreduce
        del self.schedule[:]

        def reduce(lo, hi):
            if hi > lo:
                self.schedule.append((lo, hi))
                ar.launch(lo, hi)

        if replay is None:
            class_loss, regr_loss = self.segment_a(features)
            n = self.num_parts()
            deferred = bool(self._deferred_wgrads) and n > 0

            def run_part(j, after):
                return self.segment_b(j, join_wgrads=False, after_wgrads=after)
        else:
            replay.first.replay()
            class_loss, regr_loss = replay.out
            n, deferred = len(replay.parts), replay.deferred_in_part0

            def run_part(j, after):
                replay.parts[j].replay()
                if j == 0 and after is not None:
                    after()
                return replay.ranges[j]

        top = self.heads_offset if (deferred and ar.active) else self.arena.count
        reduce(self.cut_offset, top)                       # heads + FPN (or the FPN alone): under the backbone's backward pass
        after = (lambda: reduce(top, self.arena.count)) if top < self.arena.count else None
        for j in range(n if n else (1 if self.cut_offset else 0)):
            rng = run_part(j, after) if n else None
            reduce(*(rng or (0, self.cut_offset)))         # this part's slice: under the parts that follow
        self._parts = []
        if deferred and replay is None:
            self._join_wgrads()
        if timed and self.timing is not None and self.device.type == 'cuda':
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            grad_scale = ar.wait()
            e1.record()
            self.timing.setdefault('exposed_events', []).append((e0, e1))
        else:
            grad_scale = ar.wait()
        self.opt.step(grad_scale, self.drop_counter)       # also bumps the dropout counter: fresh masks next step
        self._fold_metrics(class_loss, regr_loss)
        return class_loss, regr_loss

    def _fold_metrics(self, class_loss, regr_loss):
        """Behind the update, where norm_reg[1] -- the regulariser the log shows -- is final: the step into the metrics' window."""
        if self.metrics is not None:
            self.metrics.fold(class_loss, regr_loss, self.opt.regularization_loss)

    def _warm_up(self):
        # warm-up on a side stream (allocator + workspace sizing), then capture; ONE warm-up stream per trainer: every shape
        # key re-captures, and per-stream state elsewhere (_rn.sync_counters) is keyed by the stream handle
        s = getattr(self, "_warm_stream", None)
        if s is None:
            s = self._warm_stream = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            counter = self.drop_counter.clone()
            for _ in range(2):
                self.forward_backward(self._static, advance_dropout=False)
            self.drop_counter.copy_(counter)       # the warm-up passes do not count: replay i draws the masks eager step i draws
        torch.cuda.current_stream().wait_stream(s)

    def _capture(self, features):
        """One graph for segment A and one per part of segment B; collectives and the update are eager launches between / after
        the replays (several ranks whose collectives cannot be captured; RN_WHOLE_STEP_GRAPH=0; Adam / RMSProp at a constant rate,
        whose update takes a step-dependent launch argument).  Clipping does not bring a step here: the eager update of this path is
        the very sequence -- Optimizer.step() -- that _capture_whole records."""
        # the captured segments read PRIVATE copies of the features: a caller may hand in other tensors (or reuse these) on
        # later steps -- step() copies them into the static buffers -- and must never find its own tensors overwritten
        self._static = _clone_tree(features)
        self._warm_up()
        dot = os.environ.get("RN_GRAPH_DOT")       # tuning aid: the captured segment A as a DOT file (nodes = kernels, edges = dependencies)
        ga = torch.cuda.CUDAGraph(keep_graph=True) if dot else torch.cuda.CUDAGraph()
        # thread_local: RCCL's watchdog thread may poll events while the capture is open
        with _no_gc_while_capturing(), torch.cuda.graph(ga, capture_error_mode="thread_local"):
            self._graph_out = self.segment_a(self._static)
        if dot:
            hip = ctypes.CDLL("libamdhip64.so")
            hip.hipGraphDebugDotPrint.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint]
            err = hip.hipGraphDebugDotPrint(ctypes.c_void_p(ga.raw_cuda_graph()), dot.encode(), 0)
            print("hipGraphDebugDotPrint ->", err, dot, flush=True)
            ga.instantiate()
        had_deferred = bool(self._deferred_wgrads) and self.num_parts() > 0      # (forked and joined inside the first part's graph)
        gbs, ranges = [], []
        for j in range(self.num_parts()):          # one graph per part of segment B: the collectives go between the replays
            gb = torch.cuda.CUDAGraph()
            with _no_gc_while_capturing(), torch.cuda.graph(gb, pool=ga.pool(), capture_error_mode="thread_local"):
                ranges.append(self.segment_b(j))   # (deferred weight gradients, if any, are forked AND joined inside the first part)
            gbs.append(gb)
        self._parts = []
        self._graphs = StepGraphs(ga, gbs, ranges, self._graph_out, self._static, False, had_deferred, None)

    def _whole_step_ok(self):
        ar = self.allreduce
        return (self.whole_step_graph and self.use_graph and self.device.type == 'cuda'
                and (not ar.active or (getattr(ar, 'capturable', False) and not getattr(ar, 'host_staged', False)))
                and (self.opt.kind == 'momentum' or self.opt.lr_dev is not None) and FUSED_OPT_NORM)

    def _capture_whole(self, features):
        """_run_step as ONE graph (see __init__: whole_step_graph): with several ranks the collectives are nodes of it."""
        self._static = _clone_tree(features)
        self._warm_up()
        g = torch.cuda.CUDAGraph()
        count, phase = self.opt.step_count, self.opt._phase
        with _no_gc_while_capturing(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._graph_out = self._run_step(self._static)
        self.opt.step_count, self.opt._phase = count, phase      # (recorded, not run: replays count their own steps)
        ranges = [r for r in self.schedule if r[1] <= self.cut_offset]
        # (the parts' arena ranges are kept for reporting; no graph per part)
        self._graphs = StepGraphs(g, [], ranges, self._graph_out, self._static, True, False, list(self.schedule))

    def step(self, features=None):
        # a feed (dataset.DeviceFeed: input_fn with stage / consumed) puts a NEW sample into its static device buffers before
        # every step -- the captured segment reads them, so the graph path trains on fresh data like the reference's
        # train_input_fn (train.py:190-202); one set of captured segments per input shape
        feed = self.input_fn if (features is None and hasattr(self.input_fn, 'stage')) else None
        key = feed.stage() if feed is not None else None
        whole = self._whole_step_ok()
        scheduled = self.opt.lr_dev is not None       # the rate is read from the device: no constant of the graph changes
        if whole and not scheduled:
            # the one-graph step bakes the learning rate into the captured update: a rate that keeps changing (a schedule, a warm-up)
            # would capture again every step -- two warm-up passes + a capture each time, churning the graph cache.  After the third
            # distinct rate the trainer keeps to one graph per part with the update launched eagerly (its scalars are launch arguments).
            if self.opt.lr != self._last_lr:
                self._last_lr, self._lr_changes = self.opt.lr, self._lr_changes + 1
                if self._lr_changes == 4:
                    print("[trainer] the learning rate keeps changing: the update leaves the captured step (one graph per part from here on)",
                          file=sys.stderr, flush=True)
            if self._lr_changes > 3:
                whole = False
        if whole:
            key = (key, 'whole', self.opt.schedule if scheduled else self.opt.lr, self.opt.clip, id(self.allreduce), self.opt.accumulate_steps,
                   self.opt.skip_nonfinite)
        if self.use_graph:
            if self._graphs is None:
                self._graph_cache.clear()
            cached = self._graph_cache.get(key)
            if cached is None:
                if self._graph_cache:
                    self.recaptures += 1
                    print("[trainer] new graph key %s (input shape / learning rate / collective): capturing another graph set "
                          "(%d cached, bound %d)" % (key, len(self._graph_cache), self.graph_cache_max), file=sys.stderr, flush=True)
                while len(self._graph_cache) >= self.graph_cache_max:
                    self._graph_cache.popitem(last=False)             # least recently used: its pool is freed with it
                if whole:
                    self._capture_whole(features)
                else:
                    self._capture(features)
                self._graph_cache[key] = self._graphs
            else:
                self._graph_cache.move_to_end(key)
                self._graphs = cached
                self._graph_out, self._static = cached.out, cached.static
                if features is not None:
                    _copy_tree(self._static, features)
            g = self._graphs
            if g.whole:
                # the whole step was that one replay: what is left is the update's host-side bookkeeping
                g.first.replay()
                class_loss, regr_loss = g.out
                self.schedule[:] = g.schedule
                self.opt.count_step()               # (updates, not replays: every accumulate_steps-th replay applied one)
                import ops_f16
                ops_f16.weights_changed()
            else:
                class_loss, regr_loss = self._run_step(timed=True, replay=g)
        else:
            class_loss, regr_loss = self._run_step(features, timed=True)
        if feed is not None:
            feed.consumed()
        self.steps_done += 1
        # (only the opt-in waiting kernels -- the grid-resident GroupNorm -- can flag anything; checked after the first steps
        # too, not only every check_interval: a poisoned update must not be trained on for long.  The same check on every
        # path, the one-graph step included.)
        if (self.check_interval and ops.GN_GRID_RESIDENT
                and (self.steps_done in (1, 2, 4, 8) or self.steps_done % self.check_interval == 0)):
            self.check_device_errors()
        self.last = {'class_loss': class_loss, 'regr_loss': regr_loss,
                     'regularization_loss': self.opt.regularization_loss}
        return self.last

    def train_metrics(self, reset=True):
        """The running metrics over the steps since the last reset (metrics.TrainMetrics.result: total_loss, class_loss, regr_loss,
        regularization_loss, class_iou, regr_iou, steps, nonfinite_steps).  Synchronises; reset=True starts a new window."""
        if self.metrics is None:
            raise ValueError("this trainer keeps no training metrics: build it with train_metrics=True (--train-metrics)")
        return self.metrics.result(reset=reset)

    def skipped_updates(self):
        """(updates the guard skipped in all, updates skipped in a row up to now) -- (0, 0) without skip_nonfinite.  Synchronises,
        and brings opt.step_count back to "updates applied" (Optimizer.reconcile_skips)."""
        return self.opt.reconcile_skips()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the net runs on the moving average: the contents of arena.weights and opt.ema are swapped on the
        device (the net's parameters are views of the arena), and swapped back on the way out, also after an exception.  Do not
        train inside it."""
        import ops_f16
        if self.opt.ema is None:
            raise ValueError("this trainer keeps no moving average of the weights: build it with ema_decay=D (--ema-decay D)")
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise _rn.RnError("ema_weights() swaps the weights on the device: not while a stream is capturing")

        def swap():
            with torch.no_grad():
                tmp = self.arena.weights.clone()
                self.arena.weights.copy_(self.opt.ema)
                self.opt.ema.copy_(tmp)
            ops_f16.weights_changed()
        swap()
        try:
            yield self.net
        finally:
            swap()

    def allreduce_exposed_ms(self):
        """Mean time the compute stream waited for collectives after the last backward kernel (needs timing = {})."""
        ev = (self.timing or {}).get('exposed_events', [])
        if not ev:
            return 0.0
        torch.cuda.synchronize()
        return float(sum(a.elapsed_time(b) for a, b in ev) / len(ev))

    def check_device_errors(self):
        """Raise if any kernel of this process has flagged an error on the device (synchronises).  One opt-in kernel family
        waits for co-resident blocks and can time out: the grid-resident GroupNorm (ops.GN_GRID_RESIDENT); it is switched off
        when it has flagged."""
        n_gn = _rn.barrier_timeouts()
        if self.allreduce.active:       # every rank must take the same decision, or the others hang in the next all-reduce
            t = torch.tensor([float(n_gn)], device=self.device)
            self.allreduce.dist.all_reduce(t, op=self.allreduce.dist.ReduceOp.MAX, group=self.allreduce.group)
            n_gn = int(t[0].item())
        if n_gn:
            ops.GN_GRID_RESIDENT = False        # the launch-ordered kernels from here on (on every rank: the count is a maximum over ranks)
            _rn.reset_barrier_timeouts()
            self._graphs = None                 # the captured graphs contain the waiting kernels: capture again ...
            self._graph_cache.clear()           # ... for every input shape
            raise _rn.RnError("timed out on some rank: %d GroupNorm exchange wait(s) (ops.GN_GRID_RESIDENT is now False): the updates "
                              "since the last check are invalid -- reload the last checkpoint and continue" % n_gn)


def _for_each_tensor(tree, fn):
    if torch.is_tensor(tree):
        fn(tree)
    elif isinstance(tree, dict):
        for v in tree.values():
            _for_each_tensor(v, fn)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            _for_each_tensor(v, fn)


@contextlib.contextmanager
def _no_gc_while_capturing():
    """Around an open stream capture.  torch.cuda.graph no longer collects garbage before it begins a capture, and Python's
    cyclic collector runs whenever its allocation counters say so: in the middle of a capture it may free an earlier Trainer's
    graph set (graphs, their memory pool, events) -- device calls a capture does not allow; the process aborts inside the
    collector.  So: collect before the capture opens, where those calls are harmless and the memory is of use, and keep the
    collector off until the capture has ended.  (Objects whose last reference goes are freed as ever.)"""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def _clone_tree(tree):
    if torch.is_tensor(tree):
        return tree.clone()
    if isinstance(tree, dict):
        return {k: _clone_tree(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_clone_tree(v) for v in tree)
    return tree


def _copy_tree(dst, src):
    if torch.is_tensor(dst):
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)
    elif isinstance(dst, dict):
        for k in dst:
            _copy_tree(dst[k], src[k])
    elif isinstance(dst, (list, tuple)):
        for d, s in zip(dst, src):
            _copy_tree(d, s)


# ------------------------------------------------------------------------------------------------ CLI
# Minimal driver with the reference's flags (train.py:88-108).  --dataset pascal ROOT SUBSET / coco ANN IMAGES read the
# annotation files (data_loaders/pascal.py, coco.py; JPEG decode with Pillow on the host); 'shapes' is a synthetic stand-in
# following data_loaders/shapes.py:133-176 (1-4 filled squares, half-size in [20, S/4], 3 classes), rendered with numpy.
def evaluate(net, data_loader, levels, num_images, scale=None, device='cuda', score_threshold=0.5, dtype='f32'):
    """Inference + decode + class-wise NMS (train.py:68-85) over `num_images` samples of the loader, scored with
    COCO-style mAP and the reference's two IoU metrics (train.py:137-161); see metrics.py.
    dtype 'f16': the forward passes run in fp16 storage (layers.set_inference_dtype; logits and box deltas leave the net in fp32);
    the setting in force before the call is restored afterwards, also when the call raises."""
    if dtype != 'f32':
        import layers
        assert dtype == 'f16', dtype
        before = (layers.INFERENCE_F16, layers.F16_OUTPUTS_F32)
        layers.set_inference_dtype('f16', outputs='f32')
        try:
            return evaluate(net, data_loader, levels, num_images, scale, device, score_threshold)
        finally:
            layers.INFERENCE_F16, layers.F16_OUTPUTS_F32 = before
    import dataset
    import metrics
    dets, gts, ciou, riou = [], [], [], []
    it = dataset.build_dataset(data_loader, levels, scale=scale, device=device)
    with torch.no_grad():
        for _ in range(num_images):
            try:
                b = next(it)
            except StopIteration:
                break
            image = b['image'][:1]                                                 # the un-flipped half
            out = net(image, training=False)
            size = (int(image.shape[1]), int(image.shape[2]))
            anchors = {k: levels[k].normalized_anchor_sizes(size) for k in levels}
            probs = {k: ops.activation(v, 'sigmoid') for k, v in out['classifications'].items()}
            dec = {k: utils.regression_postprocess(out['regressions'][k], anchors[k]) for k in levels}
            d = utils.detect(probs, dec, data_loader.num_classes, score_threshold=score_threshold)[0]
            dets.append((d.boxes.cpu().numpy(), d.scores.cpu().numpy(), d.class_ids.cpu().numpy()))
            gts.append((np.asarray(b['boxes'], np.float32), np.asarray(b['class_ids'])))
            for k in levels:                                                       # build_metrics inputs, per level
                m = b['trainable_masks'][k][:1].cpu().numpy().astype(bool)
                lab = b['detection']['classifications'][k][:1].cpu().numpy()
                ciou.append((lab[m], probs[k].cpu().numpy()[m]))
                fg = lab.max(-1) > 0.5
                true_boxes = utils.regression_postprocess(b['detection']['regressions'][k][:1], anchors[k]).cpu().numpy()
                riou.append((true_boxes[fg], dec[k].cpu().numpy()[fg]))
    res = metrics.mean_average_precision(dets, gts, data_loader.num_classes)
    res['class_iou'] = metrics.class_iou(np.concatenate([a.reshape(-1) for a, _ in ciou]), np.concatenate([p.reshape(-1) for _, p in ciou]))
    res['regr_iou'] = metrics.regr_iou(np.concatenate([a for a, _ in riou]), np.concatenate([p for _, p in riou]))
    res['images'] = len(dets)
    return res


def build_parser():
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--learning-rate', type=float, default=1e-2)
    parser.add_argument('--dropout', type=float, default=0.2)
    parser.add_argument('--dataset', type=str, nargs='+', default=['shapes'],
                        help='shapes [PATH NUM SIZE] | pascal ROOT SUBSET | coco ANN_JSON IMAGES_DIR')
    parser.add_argument('--epochs', type=int, default=1)
    parser.add_argument('--scale', type=int, default=256)
    parser.add_argument('--experiment', type=str, default=None, help='directory for checkpoints (model.safetensors)')
    parser.add_argument('--grad-clip-norm', type=float, metavar='C',
                        help='scale the gradient (the L2 regulariser\'s part included) by C / max(its global norm, C); norm and scale '
                             'are formed on the device, so the update stays inside the captured step; not with --accumulate-steps')
    parser.add_argument('--backbone', type=str, choices=['resnet_50', 'densenet_121', 'densenet_169', 'mobilenet_v2'],
                        default='mobilenet_v2')
    parser.add_argument('--optimizer', type=str, choices=['momentum', 'adam', 'rmsprop'], default='momentum')
    parser.add_argument('--loss', type=str, choices=['bce_dice', 'focal'], default='bce_dice')
    parser.add_argument('--class-loss', type=str, default=None, metavar='SPEC',
                        help='the class loss as a weighted sum of the terms of the reference\'s classification_loss: '
                             'NAME[:WEIGHT[:SMOOTH]] joined by +, NAME one of %s, SMOOTH for dice / jaccard / fixed_iou only '
                             '(defaults 0 / 1 / 1e-7), e.g. bce+jaccard or balanced_bce+dice:0.5; not with --loss focal'
                             % ', '.join(losses.TERM_NAMES))
    parser.add_argument('--regr-loss', type=str, default=None, metavar='SPEC',
                        help='the box regression loss as a weighted sum of terms over the foreground anchors: huber[:WEIGHT[:DELTA]] '
                             '(the reference\'s regression_loss; DELTA defaults to 1), iou[:WEIGHT] and giou[:WEIGHT] (1 - IoU and '
                             '1 - GIoU of the predicted and the label box), joined by +, e.g. giou:2 or huber:0.5+giou:2; '
                             'left out: huber alone, as before')
    parser.add_argument('--steps-per-epoch', type=int, default=None,
                        help='default: 100 for shapes, NUM for shapes PATH NUM SIZE, one pass of the shard for a file dataset')
    parser.add_argument('--shape-runs', type=int, default=None,
                        help='file datasets: runs of <= K samples of one network input size (default 8; 0 = plain shuffle)')
    parser.add_argument('--decode-workers', type=int, default=4, help='threads decoding the image files (at most 16)')
    parser.add_argument('--eval-images', type=int, default=0, help='after training: mAP / IoU metrics over this many samples')
    parser.add_argument('--eval-fp16', action='store_true',
                        help='with --eval-images: evaluate once more with fp16 inference and print an `eval (fp16):` line')
    parser.add_argument('--eval-dataset', type=str, nargs='+', default=None,
                        help='TYPE ARGS... as --dataset; required with --eval-images for a file dataset')
    parser.add_argument('--augment', action='store_true',
                        help='file datasets: random contrast (0.8, 1.2), brightness 0.2, saturation (0.8, 1.0) per training sample '
                             '(dataset.py:206-212), on the device inside the step; the evaluation loader never augments')
    parser.add_argument('--augment-crop', type=float, default=None, metavar='S',
                        help='with --augment: also a random crop of side fraction U[S, 1] (0 < S <= 1), boxes clipped to it')
    parser.add_argument('--augment-seed', type=int, default=None, metavar='N', help='with --augment: seed of the draws (default 0)')
    parser.add_argument('--samples-per-step', type=int, default=1, metavar='K',
                        help='file datasets: train on up to K samples of one network input size per step (a batch of 2K images: '
                             'every sample and its h-flip; 1 <= K <= 16, default 1)')
    parser.add_argument('--no-graph', action='store_true', help='launch every kernel eagerly instead of replaying the captured step')
    # learning-rate schedule (LRSchedule); none of these flags: the constant --learning-rate, as before
    parser.add_argument('--lr-schedule', type=str, choices=list(LRSchedule.KINDS), default=None,
                        help='rate after the warm-up: constant | step (x --lr-decay-factor at every --lr-decay-steps) | cosine '
                             '(down to --lr-final-factor x the rate at --lr-total-steps)')
    parser.add_argument('--lr-warmup-steps', type=int, default=None, metavar='N',
                        help='linear warm-up from --lr-warmup-factor x the rate to the rate over the first N updates (default 0; '
                             'updates, not steps, with --accumulate-steps)')
    parser.add_argument('--lr-warmup-factor', type=float, default=None, metavar='F', help='default 1/3')
    parser.add_argument('--lr-decay-steps', type=int, nargs='+', default=None, metavar='A',
                        help='with --lr-schedule step: update counts (at most %d, increasing) at which the rate drops' % LRSchedule.MAX_BOUNDARIES)
    parser.add_argument('--lr-decay-factor', type=float, default=None, metavar='G', help='default 0.1')
    parser.add_argument('--lr-total-steps', type=int, default=None, metavar='T',
                        help='update count at which the cosine reaches its floor (default: the update count the run ends at: restored '
                             'step + epochs x steps per epoch; with --accumulate-steps A the updates restored + (steps into the '
                             'restored cycle + epochs x steps per epoch) // A)')
    parser.add_argument('--lr-final-factor', type=float, default=None, metavar='F', help='default 0')
    # moving average of the weights (Optimizer docstring); without --ema-decay: none, as before
    parser.add_argument('--ema-decay', type=float, default=None, metavar='D',
                        help='keep an exponential moving average of the weights inside the step (0 < D < 1, e.g. 0.9998); it is '
                             'stored in the checkpoint and evaluated beside the raw weights')
    parser.add_argument('--ema-no-warmup', action='store_true',
                        help='with --ema-decay: the decay is D from the first update on instead of min(D, (1 + n) / (10 + n))')
    # gradient accumulation (Optimizer docstring); without --accumulate-steps: an update per step, as before
    parser.add_argument('--accumulate-steps', type=int, default=1, metavar='A',
                        help='apply an update on every A-th step, from the mean of the last A gradients (1 <= A <= 64, default 1: an '
                             'effective batch A times larger at +4 B per parameter); not with --grad-clip-norm (clipping an accumulated '
                             'gradient is not implemented; clipping alone stays inside the captured step).  --lr-warmup-steps, '
                             '--lr-decay-steps and --lr-total-steps then count UPDATES, not steps')
    # guard against non-finite gradients (Optimizer docstring); without --skip-nonfinite: none, as before
    parser.add_argument('--skip-nonfinite', action='store_true',
                        help='skip the update of a step whose global gradient norm is not finite (a NaN or inf gradient, or a sum '
                             'of squares that overflows): weights, optimizer slots, schedule and moving average stay as they '
                             'are, decided on the device inside the captured step; the log line shows the count; not with '
                             '--accumulate-steps')
    parser.add_argument('--nonfinite-limit', type=int, default=None, metavar='N',
                        help='with --skip-nonfinite: end the run with an error when N updates in a row have been skipped, as seen '
                             'at a log line or a checkpoint (default: no limit)')
    # running training metrics (metrics.TrainMetrics); without --train-metrics: none, as before
    parser.add_argument('--train-metrics', action='store_true',
                        help='keep the means of the losses, class_iou and regr_iou over the steps between two log lines on the '
                             'device, inside the captured step, and append them to the log line (steps with a non-finite loss or '
                             'box IoU are left out and counted)')
    return parser


def train_metrics_suffix(res):
    """What --train-metrics appends to the log line: the window's means (Trainer.train_metrics())."""
    return (' | mean total %.4f class %.4f regr %.4f reg %.4f class_iou %.4f regr_iou %.4f over %d steps' % (
        res['total_loss'], res['class_loss'], res['regr_loss'], res['regularization_loss'], res['class_iou'], res['regr_iou'],
        res['steps']) + (' (%d non-finite left out)' % res['nonfinite_steps'] if res['nonfinite_steps'] > 0 else ''))


def regr_loss_flag_error(args):
    """What is wrong with --regr-loss as given (checked before any dataset or device is touched), or None."""
    if getattr(args, 'regr_loss', None) is None:
        return None
    try:
        losses.parse_regr_loss(args.regr_loss)
    except ValueError as e:
        return '--regr-loss: %s' % e
    return None


def class_loss_flag_error(args):
    """What is wrong with --class-loss as given (checked before any dataset or device is touched), or None."""
    if args.class_loss is None:
        return None
    if args.loss != 'bce_dice':
        return '--class-loss with --loss %s: the spec names every term of the class loss, leave --loss out' % args.loss
    try:
        losses.parse_class_loss(args.class_loss)
    except ValueError as e:
        return '--class-loss: %s' % e
    return None


def accumulate_flag_error(args):
    """What is wrong with --accumulate-steps as given (checked before any dataset or device is touched), or None."""
    if not 1 <= args.accumulate_steps <= 64:
        return '--accumulate-steps A: 1 <= A <= 64 (got %d)' % args.accumulate_steps
    if args.accumulate_steps > 1 and args.grad_clip_norm is not None:
        return '--accumulate-steps with --grad-clip-norm: clipping an accumulated gradient is not implemented'
    return None


def guard_flag_error(args):
    """What is wrong with --skip-nonfinite / --nonfinite-limit as given (checked before any dataset or device is touched), or None."""
    if args.nonfinite_limit is not None and not args.skip_nonfinite:
        return '--nonfinite-limit needs --skip-nonfinite'
    if args.nonfinite_limit is not None and args.nonfinite_limit < 1:
        return '--nonfinite-limit N: N >= 1 (got %d)' % args.nonfinite_limit
    if args.skip_nonfinite and args.accumulate_steps > 1:
        return '--accumulate-steps with --skip-nonfinite: a poisoned micro-step would need a decision per cycle, which is not implemented'
    return None


def check_nonfinite_limit(trainer, limit):
    """The guard's counters at a point where the training loop synchronises anyway (its log line, a checkpoint; on every rank: all
    of them see the same counts).  Reconciles the host's update count (Trainer.skipped_updates), returns the updates skipped in all,
    and raises when `limit` (--nonfinite-limit; None: no limit) or more updates in a row have been skipped."""
    total, consecutive = trainer.skipped_updates()
    if limit is not None and consecutive >= limit:
        raise _rn.RnError("--nonfinite-limit %d: the last %d updates in a row were skipped for a non-finite gradient norm (%d "
                          "skipped in all): the run ends here" % (limit, consecutive, total))
    return total


def ema_flag_error(args):
    """What is wrong with the --ema-* flags as given (checked before any dataset or device is touched), or None."""
    if args.ema_no_warmup and args.ema_decay is None:
        return '--ema-no-warmup needs --ema-decay'
    if args.ema_decay is not None and not 0.0 < args.ema_decay < 1.0:
        return '--ema-decay D: 0 < D < 1 (got %g)' % args.ema_decay
    return None


LR_FLAGS = ('lr_schedule', 'lr_warmup_steps', 'lr_warmup_factor', 'lr_decay_steps', 'lr_decay_factor', 'lr_total_steps',
            'lr_final_factor')


def lr_flag_error(args):
    """What is wrong with the --lr-* flags as given (checked before any dataset or device is touched), or None."""
    kind = args.lr_schedule or 'constant'
    if args.lr_decay_steps is not None and kind != 'step':
        return '--lr-decay-steps needs --lr-schedule step'
    if args.lr_decay_factor is not None and kind != 'step':
        return '--lr-decay-factor needs --lr-schedule step'
    if args.lr_final_factor is not None and kind != 'cosine':
        return '--lr-final-factor needs --lr-schedule cosine'
    if kind == 'step' and not args.lr_decay_steps:
        return '--lr-schedule step needs --lr-decay-steps A B ...'
    if args.lr_decay_steps is not None and len(args.lr_decay_steps) > LRSchedule.MAX_BOUNDARIES:
        return '--lr-decay-steps: at most %d steps (got %d)' % (LRSchedule.MAX_BOUNDARIES, len(args.lr_decay_steps))
    if args.lr_total_steps is not None and args.lr_total_steps <= (args.lr_warmup_steps or 0):
        return '--lr-total-steps %d is not above --lr-warmup-steps %d' % (args.lr_total_steps, args.lr_warmup_steps or 0)
    return None


def schedule_from_args(args, steps_per_epoch, restored_step, phase=0):
    """The LRSchedule the --lr-* flags describe, or None when none of them is given (the constant-rate path, unchanged).  Pure:
    no device, no files.  --lr-total-steps defaults to the update count this run ends at: with --accumulate-steps A,
    `restored_step` is the number of UPDATES restored and `phase` the micro-steps of the restored, unfinished cycle.  Raises
    ValueError (main: parser.error) for combinations that make no sense."""
    if all(getattr(args, f) is None for f in LR_FLAGS):
        return None
    err = lr_flag_error(args)
    if err:
        raise ValueError(err)
    warmup = args.lr_warmup_steps or 0
    A = int(getattr(args, 'accumulate_steps', 1))
    total = (args.lr_total_steps if args.lr_total_steps is not None
             else int(restored_step) + (int(phase) + args.epochs * int(steps_per_epoch)) // A)
    if total <= warmup:
        raise ValueError('the run ends at update %d, not above --lr-warmup-steps %d (see --lr-total-steps)' % (total, warmup))
    return LRSchedule(kind=args.lr_schedule or 'constant', base_lr=args.learning_rate, warmup_steps=warmup,
                      warmup_factor=1.0 / 3.0 if args.lr_warmup_factor is None else args.lr_warmup_factor,
                      boundaries=tuple(args.lr_decay_steps or ()),
                      decay_factor=0.1 if args.lr_decay_factor is None else args.lr_decay_factor,
                      total_steps=total, final_factor=0.0 if args.lr_final_factor is None else args.lr_final_factor)


def init_distributed(backend=None):
    """One process per GPU, like the reference picks MirroredStrategy from the number of GPUs (train.py:261-267):
    rank / world size / device come from the launcher's environment (python -m torch.distributed.run, or
    bench.py --gpus N which starts that itself).  Returns (device, rank, world, process_group_initialised).
    Must run before anything else touches the GPU: it selects the device every kernel launch then uses."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise _rn.RnError("training needs an MI355X: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    started = False
    if 'WORLD_SIZE' in os.environ and 'RANK' in os.environ:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if not dist.is_initialized():
            dist.init_process_group(backend or 'nccl', rank=rank, world_size=world,
                                    **({'device_id': dev} if (backend or 'nccl') == 'nccl' else {}))
            started = True
    return dev, rank, world, started


def broadcast_initial_state(trainer, src=0):
    """Replicas must start from identical variables (MirroredStrategy creates them once and mirrors them)."""
    import torch.distributed as dist
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(trainer.arena.weights, src=src)
        dist.broadcast(trainer.opt.state1, src=src)
        if trainer.opt.state2 is not None:
            dist.broadcast(trainer.opt.state2, src=src)
        if trainer.opt.ema is not None:
            dist.broadcast(trainer.opt.ema, src=src)
        if trainer.opt.acc is not None:
            dist.broadcast(trainer.opt.acc, src=src)


LAST_RUN = {}


def main(argv=None):
    import checkpoint
    import dataset
    import retinanet
    parser = build_parser()
    args = parser.parse_args(argv)
    kind, dargs = args.dataset[0], args.dataset[1:]
    files = kind in ('pascal', 'coco')
    if kind not in ('shapes', 'pascal', 'coco') or len(dargs) != {'shapes': 3 if dargs else 0}.get(kind, 2):
        parser.error('--dataset: shapes [PATH NUM SIZE] | pascal ROOT SUBSET | coco ANN_JSON IMAGES_DIR (got %s)' % ' '.join(args.dataset))
    if files and args.eval_images and not args.eval_dataset:
        parser.error('--eval-images with a file dataset needs --eval-dataset TYPE ARGS...')
    if (args.augment or args.augment_crop is not None or args.augment_seed is not None) and not files:
        parser.error('--augment transforms raw uint8 image files: it needs --dataset pascal ... or coco ...')
    if (args.augment_crop is not None or args.augment_seed is not None) and not args.augment:
        parser.error('--augment-crop / --augment-seed need --augment')
    if args.augment_crop is not None and not (0.0 < args.augment_crop <= 1.0):
        parser.error('--augment-crop S: 0 < S <= 1 (got %g)' % args.augment_crop)
    if lr_flag_error(args):
        parser.error(lr_flag_error(args))
    if ema_flag_error(args):
        parser.error(ema_flag_error(args))
    if accumulate_flag_error(args):
        parser.error(accumulate_flag_error(args))
    if guard_flag_error(args):
        parser.error(guard_flag_error(args))
    if class_loss_flag_error(args):
        parser.error(class_loss_flag_error(args))
    if regr_loss_flag_error(args):
        parser.error(regr_loss_flag_error(args))
    K = args.samples_per_step
    if K != 1 and not files:
        parser.error('--samples-per-step groups raw uint8 image files: it needs --dataset pascal ... or coco ...')
    if not 1 <= K <= 16:
        parser.error('--samples-per-step K: 1 <= K <= 16 (got %d)' % K)
    dev, rank, world, started = init_distributed()
    from data_loaders.shapes import Shapes
    # every replica draws its own samples (dataset.py:182-204: a replica's batch is [sample, hflip(sample)])
    if files:
        from data_loaders.inferred import Inferred
        # one epoch = a permutation seeded by (0, epoch), sample i to rank i % world, runs of one network input size
        # (--samples-per-step K > 1: full groups of K samples of one size instead of the runs, data_loaders/files.py)
        loader = Inferred(kind, dargs).configure(seed=0, rank=rank, world=world, scale=args.scale, repeat=True,
                                                 shape_runs=8 if args.shape_runs is None else args.shape_runs,
                                                 **({'group': K} if K > 1 else {}))
        if K > 1:
            # a step is a group, and ranks form different numbers of groups from their shards: every rank computes every rank's
            # count for epoch 0 (no I/O) and all run the smallest -- unequal step counts would leave a rank waiting in a collective
            steps_per_epoch = args.steps_per_epoch or max(1, min(loader.epoch_steps(0, r) for r in range(world)))
        else:
            steps_per_epoch = args.steps_per_epoch or max(1, len(loader.records) // world)    # every rank runs the same steps
        if rank == 0:
            print('%s: %d images (%d skipped: no valid box), %d steps per epoch' % (kind, len(loader.records), loader.skipped,
                                                                                  steps_per_epoch), flush=True)
            if K > 1:
                print('%d images per step: %d samples of one input size and their h-flips (fewer where a group is partial)'
                      % (2 * K, K), flush=True)
    elif dargs:
        loader = Shapes(dargs[0], image_size=(int(dargs[2]), int(dargs[2])), seed=rank)
        steps_per_epoch = args.steps_per_epoch or int(dargs[1])
    else:
        loader = Shapes(None, image_size=(args.scale + args.scale // 4, args.scale), seed=rank)   # rescale_image brings it to --scale
        steps_per_epoch = args.steps_per_epoch or 100
    levels = build_levels()
    torch.manual_seed(0)                                                           # same initial weights on every rank
    net = retinanet.RetinaNet(backbone=args.backbone, levels=levels, num_classes=loader.num_classes, activation=L.elu,
                              dropout_rate=args.dropout).to(dev)
    # train_input_fn (train.py:190-202) = dataset.DeviceFeed: loader thread -> pinned host memory -> asynchronous upload ->
    # static device buffers; rescale, normalisation, the h-flip and the anchor assignment of every NEW sample run inside the
    # captured step (one hipGraph per backward segment, replayed per step; --no-graph launches the same kernels eagerly).
    # File datasets: ragged staging, one graph set per network input shape whatever the raw image sizes (DeviceFeed docstring).
    # --augment: the sample's crop window and photometric scalars are drawn on the loader thread as a function of (seed, rank,
    # position in the stream) and reach the kernels through a descriptor uploaded with the sample: the same graphs serve every draw
    drawn0 = 0
    path = None if args.experiment is None else os.path.join(args.experiment, 'model.safetensors')
    if path is not None and os.path.exists(path):
        drawn0 = int(checkpoint.load_extra(path).get('samples_drawn', 0))
    # (first_ordinal = samples_drawn holds because every staged sample is one sample of the loader's stream: the file readers drop
    # invalid records once, up front, so Inferred skips nothing while iterating -- checked where the checkpoint is written)
    skipped0 = getattr(loader, 'skipped', 0)
    group_kw = {'samples_per_step': K} if K > 1 else {}
    if files and args.augment:
        import augmentation
        policy = augmentation.Policy(crop_min=1.0 if args.augment_crop is None else args.augment_crop, seed=args.augment_seed or 0)
        feed = dataset.DeviceFeed(loader, levels, scale=args.scale, device=dev, ragged=True, decode_workers=args.decode_workers,
                                  augment=policy, first_ordinal=drawn0, **group_kw)
    elif files:
        feed = dataset.DeviceFeed(loader, levels, scale=args.scale, device=dev, ragged=True, decode_workers=args.decode_workers,
                                  **group_kw)
    else:
        feed = dataset.DeviceFeed(loader, levels, scale=args.scale, device=dev)
    restored = checkpoint.saved_step(path) if (path is not None and os.path.exists(path)) else 0
    A, phase = args.accumulate_steps, 0
    if A > 1 and path is not None and os.path.exists(path):
        # the schedule counts updates: those the file holds, and the run resumes `phase` micro-steps into a cycle
        restored, phase = checkpoint.saved_updates(path, A)
    elif args.skip_nonfinite and path is not None and os.path.exists(path):
        restored = checkpoint.saved_updates(path, 1)[0]                           # updates applied: steps less the skipped ones
    try:
        lr_schedule = schedule_from_args(args, steps_per_epoch, restored, phase)
    except ValueError as e:
        parser.error(str(e))
    trainer = Trainer(net, levels, optimizer=args.optimizer, learning_rate=args.learning_rate,
                      grad_clip_norm=args.grad_clip_norm, loss_mode=args.class_loss or args.loss, device=dev, use_graph=not args.no_graph,
                      input_fn=feed, **({'lr_schedule': lr_schedule} if lr_schedule is not None else {}),
                      **({'ema_decay': args.ema_decay, 'ema_warmup': not args.ema_no_warmup} if args.ema_decay is not None else {}),
                      **({'accumulate_steps': A} if A > 1 else {}), **({'skip_nonfinite': True} if args.skip_nonfinite else {}),
                      **({'train_metrics': True} if args.train_metrics else {}),
                      **({'regr_loss': args.regr_loss} if args.regr_loss is not None else {}))
    if args.class_loss is not None and rank == 0:
        print('class loss: %s' % trainer.loss_mode.describe(), flush=True)
    if args.regr_loss is not None and rank == 0:
        print('regr loss: %s' % trainer.regr_loss.describe(), flush=True)

    def skipped():
        return check_nonfinite_limit(trainer, args.nonfinite_limit)
    step = 0
    if path is not None and os.path.exists(path):
        step = checkpoint.load(path, net, trainer)                                 # every rank reads the same file
        # like the reference (train.py:271-273: `for epoch in range(args.epochs): estimator.train(...)` on a restored global
        # step) a rerun trains args.epochs MORE epochs; what is carried over besides the weights: the step count, the
        # optimizer slots, the dropout counter and the position in the sample stream (counted in samples, not steps: drawn0
        # above, which is also the ordinal the augmentation draws continue from)
        if rank == 0:
            print('restored step', step)
    loader.skip(drawn0)                                                            # (before the feed's thread draws: it starts lazily)
    broadcast_initial_state(trainer)
    feed.start()
    t0 = time.perf_counter()
    try:
        for epoch in range(args.epochs):
            for _ in range(steps_per_epoch):
                out = trainer.step()                                               # batch = [image, hflip] of a new sample
                step += 1
                skips = skipped() if (args.skip_nonfinite and step % 20 == 0) else 0
                if step % 20 == 0 and rank == 0:
                    print('epoch %d step %d class_loss %.4f regr_loss %.4f reg %.4f lr %.3g' % (
                        epoch, step, out['class_loss'].item(), out['regr_loss'].item(), out['regularization_loss'].item(),
                        trainer.opt.current_lr())                                  # (the rate of the NEXT update: host-side, no sync)
                          + (' update %d' % trainer.opt.step_count if A > 1 else '')
                          + (' skipped %d' % skips if skips > 0 else '')
                          + (train_metrics_suffix(trainer.train_metrics()) if args.train_metrics else ''), flush=True)
            trainer.check_device_errors()
            if args.skip_nonfinite:
                skipped()
            if args.augment and getattr(loader, 'skipped', 0) != skipped0:
                raise _rn.RnError("the loader skipped samples while iterating: the augmentation's ordinals no longer equal the "
                                  "stream position a checkpoint stores (samples_drawn)")
            if path is not None and rank == 0:                                     # replicas are identical: rank 0 writes
                checkpoint.save(path, net, trainer, step=step,
                                extra={'epochs_done': epoch + 1, 'samples_drawn': drawn0 + feed.samples_staged})
    finally:
        feed.close()
    # what the run did, for measuring tools (tools/files_bench.py): wall time of the training loop (captures, checkpoints included)
    skipped_total = trainer.skipped_updates()[0]                                  # (reconciles: `updates` below counts applied ones)
    LAST_RUN.update(steps=step, seconds=time.perf_counter() - t0, samples=feed.samples_staged, recaptures=trainer.recaptures,
                    graph_sets=len(trainer._graph_cache), updates=trainer.opt.step_count, skipped=skipped_total)
    if args.eval_images and rank == 0:
        if args.eval_dataset:
            from data_loaders.inferred import Inferred
            eval_loader = Inferred(args.eval_dataset[0], args.eval_dataset[1:])
        else:
            eval_loader = Shapes(None, image_size=(args.scale + args.scale // 4, args.scale), seed=12345)
        res = evaluate(net, eval_loader, levels, args.eval_images, scale=args.scale, device=dev)
        print('eval: mAP %.4f AP50 %.4f AP75 %.4f class_iou %.4f regr_iou %.4f over %d images' % (
            res['mAP'], res['AP50'], res['AP75'], res['class_iou'], res['regr_iou'], res['images']), flush=True)
        if trainer.opt.ema is not None:
            if args.eval_dataset:
                eval_loader = Inferred(args.eval_dataset[0], args.eval_dataset[1:])        # (a fresh loader: the same samples again)
            else:
                eval_loader = Shapes(None, image_size=(args.scale + args.scale // 4, args.scale), seed=12345)
            with trainer.ema_weights():
                res = evaluate(net, eval_loader, levels, args.eval_images, scale=args.scale, device=dev)
            print('eval (ema): mAP %.4f AP50 %.4f AP75 %.4f class_iou %.4f regr_iou %.4f over %d images' % (
                res['mAP'], res['AP50'], res['AP75'], res['class_iou'], res['regr_iou'], res['images']), flush=True)
        if args.eval_fp16:
            if args.eval_dataset:
                eval_loader = Inferred(args.eval_dataset[0], args.eval_dataset[1:])        # (a fresh loader: the same samples again)
            else:
                eval_loader = Shapes(None, image_size=(args.scale + args.scale // 4, args.scale), seed=12345)
            res = evaluate(net, eval_loader, levels, args.eval_images, scale=args.scale, device=dev, dtype='f16')
            print('eval (fp16): mAP %.4f AP50 %.4f AP75 %.4f class_iou %.4f regr_iou %.4f over %d images' % (
                res['mAP'], res['AP50'], res['AP75'], res['class_iou'], res['regr_iou'], res['images']), flush=True)
    if started:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return step


if __name__ == '__main__':
    main()
