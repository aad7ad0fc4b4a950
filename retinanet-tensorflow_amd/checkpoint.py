"""Checkpoint I/O: weights + optimizer slots in one safetensors file, keyed by the
model's parameter names (the reference delegates this to tf.estimator, train.py:263-273: model_dir +
save_checkpoints_steps; no custom format exists to be compatible with)."""
import json
import os
import sys

import torch
from safetensors import safe_open
from safetensors.torch import save_file


def save(path, net, trainer=None, step=0, extra=None):
    """Weights under "model/<name>"; optimizer slots PER PARAMETER under "optimizer/state{1,2}/<name>" (independent of the
    arena's layout); the dropout step counter, so that a resumed run does not replay the masks of step 0.  A trainer that keeps a
    moving average of the weights adds it PER PARAMETER under "ema/<name>" with metadata ema_decay / ema_warmup / ema_updates
    ("model/<name>" stays the raw weights: resuming needs them); readers that know nothing of these keys ignore them.  A trainer
    that accumulates gradients (accumulate_steps A > 1) adds the cycle's running sum PER PARAMETER under "accum/<name>" with metadata
    accum_steps = A and accum_micro = micro-steps taken, so a checkpoint written in the middle of a cycle resumes exactly.  `step`
    counts micro-steps (the position in the sample stream depends on it), step_count counts updates.  A trainer with the guard
    against non-finite gradients (skip_nonfinite) is reconciled first (Optimizer.reconcile_skips: this synchronises), so the
    step_count stored is that of the updates APPLIED, and metadata nonfinite_skipped holds the updates skipped in all."""
    tensors = {"model/" + k: v.detach().cpu().contiguous().clone() for k, v in net.named_parameters()}
    meta = {"step": str(int(step)), "format": "retinanet-amd-v2"}
    if trainer is not None:
        names = {id(p): k for k, p in net.named_parameters()}
        for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
            name = names[id(p)]
            tensors["optimizer/state1/" + name] = trainer.opt.state1[off:off + size].detach().cpu().clone().view(p.shape)
            if trainer.opt.state2 is not None:
                tensors["optimizer/state2/" + name] = trainer.opt.state2[off:off + size].detach().cpu().clone().view(p.shape)
        # (stored without this replica's offset: every rank adds its own back on load, replicas keep distinct dropout streams)
        tensors["trainer/drop_counter"] = trainer.drop_counter.detach().cpu().clone() - int(getattr(trainer, "drop_rank_offset", 0))
        if getattr(trainer.opt, "skipped_dev", None) is not None:
            meta.update(nonfinite_skipped=str(trainer.opt.reconcile_skips()[0]))        # (ahead of step_count below: it corrects it)
        meta.update(optimizer=trainer.opt.kind, step_count=str(trainer.opt.step_count))
        if getattr(trainer.opt, "ema", None) is not None:
            for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
                tensors["ema/" + names[id(p)]] = trainer.opt.ema[off:off + size].detach().cpu().clone().view(p.shape)
            meta.update(ema_decay=repr(trainer.opt.ema_decay), ema_warmup=str(int(trainer.opt.ema_warmup)),
                        ema_updates=str(int(trainer.opt.ema_updates_dev.item())))
        if getattr(trainer.opt, "acc", None) is not None:
            for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
                tensors["accum/" + names[id(p)]] = trainer.opt.acc[off:off + size].detach().cpu().clone().view(p.shape)
            meta.update(accum_steps=str(trainer.opt.accumulate_steps), accum_micro=str(int(trainer.opt.micro_dev.item())))
    if extra:
        meta["extra"] = json.dumps(extra)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    save_file(tensors, tmp, metadata=meta)
    os.replace(tmp, path)


def load_extra(path):
    """The `extra` dict a checkpoint was saved with (train.py main(): epochs done, samples drawn per rank); {} if none."""
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    return json.loads(meta["extra"]) if "extra" in meta else {}


def saved_step(path):
    """The step a checkpoint was saved at (what load() returns), without reading a tensor."""
    with safe_open(path, framework="pt") as f:
        return int((f.metadata() or {}).get("step", 0))


def saved_updates(path, accumulate_steps):
    """(updates applied, micro-steps into the unfinished cycle) as a run with `accumulate_steps` resumes from this checkpoint,
    without reading a tensor: the phase is 0 unless the file was written with the same accumulate_steps (see load)."""
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    same = int(meta.get("accum_steps", 1)) == int(accumulate_steps) and "accum_micro" in meta
    return int(meta.get("step_count", 0)), (int(meta["accum_micro"]) % int(accumulate_steps) if same else 0)


_seeded_note = [False]
_fresh_cycle_note = [False]


def load(path, net, trainer=None, use_ema=False):
    """Restores in place (the parameters keep pointing into the trainer's arena).  Returns the saved step.
    Missing keys and shape mismatches raise a ValueError that names the parameter.

    A trainer that keeps a moving average gets "ema/<name>" and the update word back; from a file without any "ema/" key (a run
    that kept none) the average is seeded with the loaded weights and the word with step_count, said once on stderr.  A trainer
    that keeps none ignores the keys.  A trainer that accumulates gradients (accumulate_steps A > 1) gets "accum/<name>" and the
    micro-step word back when the file was written with the same A; from any other file (no "accum/" key, or another accum_steps)
    it starts a fresh cycle -- phase 0, the sum cleared -- said once on stderr.  A trainer with A = 1 ignores the keys.
    A trainer with the guard against non-finite gradients gets its skip count back from nonfinite_skipped (a file without the key:
    0) -- the device's counter and what the host has accounted for; step_count, the schedule's position and the average's word
    are those of the updates applied.  A trainer without the guard ignores the key.
    use_ema=True (trainer=None): the net is given the AVERAGES instead of the raw weights, for inference; a file without them
    raises a ValueError."""
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
        keys = set(f.keys())
        fmt = meta.get("format")
        if fmt != "retinanet-amd-v2":       # checked BEFORE any weight is overwritten in place
            raise ValueError("checkpoint %s has format %r; this build reads 'retinanet-amd-v2' (per-parameter optimizer slots)" % (path, fmt))
        if trainer is not None and meta.get("optimizer") is not None:
            if meta.get("optimizer") != trainer.opt.kind:
                raise ValueError("checkpoint optimizer %s != %s" % (meta.get("optimizer"), trainer.opt.kind))
            need = ["optimizer/state1/"] + (["optimizer/state2/"] if trainer.opt.state2 is not None else [])
            for k, _ in net.named_parameters():
                for pre in need:
                    if pre + k not in keys:
                        raise ValueError("checkpoint %s has no tensor %r" % (path, pre + k))
        has_ema = any(k.startswith("ema/") for k in keys)
        if use_ema:
            if trainer is not None:
                raise ValueError("checkpoint.load(use_ema=True) puts the averages into a net for inference: pass no trainer")
            if not has_ema:
                raise ValueError("checkpoint %s holds no moving average of the weights (no 'ema/' tensors): it was written "
                                 "without --ema-decay" % path)
        want_ema = trainer is not None and getattr(trainer.opt, "ema", None) is not None
        want_acc = trainer is not None and getattr(trainer.opt, "acc", None) is not None
        has_acc = (want_acc and any(k.startswith("accum/") for k in keys) and "accum_micro" in meta
                   and int(meta.get("accum_steps", 1)) == trainer.opt.accumulate_steps)
        prefixes = ["ema/" if use_ema else "model/"] + (["ema/"] if want_ema and has_ema else []) + (["accum/"] if has_acc else [])
        for k, p in net.named_parameters():
            for pre in prefixes:
                if pre + k not in keys:
                    raise ValueError("checkpoint %s has no tensor %r" % (path, pre + k))
                shape = tuple(f.get_slice(pre + k).get_shape())
                if shape != tuple(p.shape):
                    raise ValueError("checkpoint %s: %r has shape %s, the model expects %s" % (path, pre + k, shape, tuple(p.shape)))

        def get(key, like):
            if key not in keys:
                raise ValueError("checkpoint %s has no tensor %r" % (path, key))
            t = f.get_tensor(key)
            if tuple(t.shape) != tuple(like.shape):
                raise ValueError("checkpoint %s: %r has shape %s, the model expects %s" % (path, key, tuple(t.shape), tuple(like.shape)))
            return t

        with torch.no_grad():
            for k, p in net.named_parameters():
                p.copy_(get(("ema/" if use_ema else "model/") + k, p).to(p.device))
            if trainer is not None and meta.get("optimizer") is not None:
                if meta.get("optimizer") != trainer.opt.kind:
                    raise ValueError("checkpoint optimizer %s != %s" % (meta.get("optimizer"), trainer.opt.kind))
                names = {id(p): k for k, p in net.named_parameters()}
                for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
                    name = names[id(p)]
                    trainer.opt.state1[off:off + size].copy_(get("optimizer/state1/" + name, p).reshape(-1).to(trainer.opt.state1.device))
                    if trainer.opt.state2 is not None:
                        trainer.opt.state2[off:off + size].copy_(get("optimizer/state2/" + name, p).reshape(-1).to(trainer.opt.state2.device))
                if "trainer/drop_counter" in keys:
                    trainer.drop_counter.copy_((f.get_tensor("trainer/drop_counter") + int(getattr(trainer, "drop_rank_offset", 0)))
                                               .to(trainer.drop_counter.device))
                # (also the device step word of a learning-rate schedule: a resumed run continues the schedule where it stopped)
                trainer.opt.set_step_count(int(meta.get("step_count", 0)))
            if trainer is not None and getattr(trainer.opt, "skipped_dev", None) is not None:
                trainer.opt.set_skipped(int(meta.get("nonfinite_skipped", 0)))
            if want_ema:
                opt = trainer.opt
                if has_ema:
                    names = {id(p): k for k, p in net.named_parameters()}
                    for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
                        opt.ema[off:off + size].copy_(get("ema/" + names[id(p)], p).reshape(-1).to(opt.ema.device))
                    opt.ema_updates_dev.fill_(int(meta.get("ema_updates", meta.get("step_count", 0))))
                else:
                    # written by a run that kept no average: it starts here, at the loaded weights
                    opt.ema.copy_(trainer.arena.weights)
                    opt.ema_updates_dev.fill_(int(meta.get("step_count", 0)))
                    if not _seeded_note[0]:
                        _seeded_note[0] = True
                        print("[checkpoint] %s holds no moving average of the weights: it starts from the loaded weights, at update %d"
                              % (path, int(meta.get("step_count", 0))), file=sys.stderr, flush=True)
            if want_acc:
                opt = trainer.opt
                if has_acc:
                    names = {id(p): k for k, p in net.named_parameters()}
                    for p, (off, size) in zip(trainer.arena.params, trainer.arena.offsets):
                        opt.acc[off:off + size].copy_(get("accum/" + names[id(p)], p).reshape(-1).to(opt.acc.device))
                    opt.set_accum_micro(int(meta["accum_micro"]))
                else:
                    # written without accumulation, or with another accumulate_steps: its partial sum (if any) means nothing here
                    opt.acc.zero_()
                    opt.set_accum_micro(0)
                    if not _fresh_cycle_note[0]:
                        _fresh_cycle_note[0] = True
                        print("[checkpoint] %s holds no gradient sum for accumulate_steps %d (written with %s): the accumulation "
                              "starts a fresh cycle, at phase 0" % (path, opt.accumulate_steps, meta.get("accum_steps", "1")),
                              file=sys.stderr, flush=True)
    import ops_f16
    ops_f16.weights_changed()
    return int(meta.get("step", 0))
