"""The training loop and its command line: what the reference's ``train.py`` does through mmcv's EpochBasedRunner.

  python -m demf_amd.train --data-root R --ann-file sunrgbd_infos_train.pkl --work-dir W
                           [--val-ann-file sunrgbd_infos_val.pkl] [--load-from C] [--resume-from C] [--no-validate]
                           [--no-graphs] [--batch-size 16] [--epochs 36] [--seed 0] [--workers 4] [--log-interval 50]
                           [--accumulate 1] [--autoscale-lr] [--model {demf,votenet}]
                           [--feature-cache DIR [--feature-cache-dtype {fp32,bf16}]] [--gpus N]

``fit`` feeds a dataset through ``SceneLoader(mode="train")``, the frozen image stream and ``engine.Trainer`` (one
captured hipGraph per batch shape, ``StepCache``).  Losses, gradient norm and learning rate are logged through the
device-side step meter (``meter.StepMeter``): the loop enqueues one copy of the meter's ring per log interval and
never waits for the GPU between log points.  Checkpoints are written per epoch, as mmcv's CheckpointHook does, in
a layout ``infer.load_checkpoint`` and the reference's tools read; ``resume_from`` continues with the next epoch
(mmcv's resume granularity).  Validation is ``infer.run_test`` + ``dataset.evaluate``.

``--accumulate 8`` forms the step of the reference's 8 ranks x 16 scenes from 8 forward + backward passes on one GPU
(gradient accumulation, ``engine.Trainer(accumulate=W)``): iterations, log lines and the meter then count OPTIMIZER
steps.

``--gpus N`` is the reference's tools/dist_train.sh: N ranks of this module, one GPU each (``ranks.launch``; under a
launcher that set ``RANK``, ``main`` joins the process group instead).  ``fit`` then gives every rank its share of
each epoch's permutation (``pipeline.shard_chunks``: optimizer step k consumes the chunks a single process with
``accumulate = N`` consumes in its group k), ``engine.Trainer`` keeps the replicas identical (rank-0 broadcast, SUM
all-reduce of the flat gradient buffer), the log's loss terms are the mean over ranks (``StepMeter.snapshot`` merges
the ranks' rings), rank 0 alone writes ``train.log.json`` and the checkpoints, and validation runs sharded
(``infer.run_test``) after rank 0's BatchNorm statistics have been broadcast.  Without a process group nothing of
this runs: single process, one GPU, the files and log lines of before.
"""
import argparse
import functools
import glob
import json
import math
import os
import re
import sys
import time

import torch

# The reference's values, where it sets them:
DEFAULTS = dict(
    batch_size=16,           # configs/_base_/datasets/sunrgbd-3d-10class.py:75  samples_per_gpu=16
    workers=4,               # configs/_base_/datasets/sunrgbd-3d-10class.py:76  workers_per_gpu=4
    repeat=5,                # configs/_base_/datasets/sunrgbd-3d-10class.py:77-86  RepeatDataset(times=5)
    lr=0.008,                # configs/_base_/schedules/schedule_3x.py:4-5  AdamW lr=0.008
    weight_decay=0.01,       # configs/_base_/schedules/schedule_3x.py:5  weight_decay=0.01
    max_grad_norm=10,        # configs/_base_/schedules/schedule_3x.py:6  grad_clip max_norm=10, norm_type=2
    lr_steps=(24, 32),       # configs/_base_/schedules/schedule_3x.py:7  policy='step', step=[24, 32]
    gamma=0.1,               # (mmcv StepLrUpdaterHook's default, which schedule_3x.py:7 leaves in place)
    max_epochs=36,           # configs/_base_/schedules/schedule_3x.py:9  EpochBasedRunner max_epochs=36
    ckpt_interval=1,         # configs/_base_/default_runtime.py:1, configs/demf/demf_votenet.py:280  interval=1
    max_keep_ckpts=1,        # configs/demf/demf_votenet.py:280  checkpoint_config max_keep_ckpts=1
    log_interval=50,         # configs/_base_/default_runtime.py:6-7  log_config interval=50
    eval_interval=36,        # configs/demf/demf_votenet.py:275-278  evaluation interval=36
    seed=0,
    accumulate=1,            # (tools/dist_train.sh:4 trains on 8 GPUs: --accumulate 8 is that step on one)
)
REFERENCE_WORLD = 8          # train.py:51-53: --autoscale-lr scales lr by len(gpu_ids) / 8


def lr_factor(epoch, lr_steps=DEFAULTS["lr_steps"], gamma=DEFAULTS["gamma"]):
    """mmcv StepLrUpdaterHook by epoch (0-based, as ``runner.epoch``): gamma ** (milestones reached).  The same
    expression as ``engine.Trainer.set_epoch``."""
    return gamma ** sum(1 for s in lr_steps if epoch >= s)


def loader_epoch(epoch, rep, repeat):
    """The ``SceneLoader.epoch`` of pass ``rep`` (0 .. repeat-1) of runner epoch ``epoch`` (0-based): every pass of
    the run has its own number, so a resumed run draws the permutations and augmentations the first one would."""
    if not 0 <= rep < repeat:
        raise ValueError(f"pass {rep} of {repeat}")
    return int(epoch) * int(repeat) + int(rep)


def accumulation_plan(batches_per_pass, repeat, accumulate):
    """One runner epoch is ``repeat`` passes of ``batches_per_pass`` batches; groups of ``accumulate`` batches run
    across the passes and a group left incomplete at the end of the epoch is abandoned.
    -> (optimizer steps per runner epoch, batches discarded at its end)."""
    if batches_per_pass < 0 or repeat < 1 or accumulate < 1:
        raise ValueError("accumulation_plan: batches_per_pass >= 0, repeat >= 1 and accumulate >= 1")
    total = int(batches_per_pass) * int(repeat)
    return total // int(accumulate), total % int(accumulate)


def check_resume_accumulate(meta, accumulate, path="the checkpoint"):
    """A resumed run keeps the checkpoint's ``accumulate`` (its ``iter`` and the meter's ``t`` count optimizer steps
    of that size); a file written before the field existed reads as 1."""
    was = int(meta.get("accumulate", 1))
    if was != int(accumulate):
        raise ValueError("resume_from %s was trained with accumulate = %d, this run asks for accumulate = %d"
                         % (path, was, int(accumulate)))
    return was


def check_resume_world(meta, world, path="the checkpoint"):
    """A resumed run keeps the checkpoint's ``world`` (the ranks' shards and the number of iterations per epoch
    depend on it); the field is written only when it is above 1, and an absent one reads as 1."""
    was = int(meta.get("world", 1))
    if was != int(world):
        raise ValueError("resume_from %s was trained with world = %d ranks, this run has world = %d"
                         % (path, was, int(world)))
    return was


def autoscale_lr(lr, accumulate=1, world=1):
    """The reference's ``--autoscale-lr`` (train.py:51-53: lr x len(gpu_ids) / 8, the linear scaling rule) with the
    number of 16-scene batches per optimizer step in the place of the GPU count: lr x (accumulate x world) / 8."""
    return float(lr) * (int(accumulate) * int(world)) / REFERENCE_WORLD


def format_log(rows, epoch, it, base_lr, seconds_per_iter, names=None):
    """One ``mode: "train"`` log line from the meter rows of an interval: ``epoch`` (1-based) and ``iter`` (global,
    1-based) of the interval's last step, ``lr`` of the first parameter group, the mean of every loss term, of
    ``loss`` (the meter's ``_total``) and of ``grad_norm`` over the rows, ``time`` per iteration."""
    if not rows:
        raise ValueError("a log line needs at least one meter row")
    skip = ("t", "lr_factor", "grad_norm", "clip", "nonfinite", "_total")
    names = [k for k in rows[0] if k not in skip] if names is None else [k for k in names if k != "_total"]
    line = dict(mode="train", epoch=int(epoch), iter=int(it), lr=float(base_lr) * rows[-1]["lr_factor"])
    n = len(rows)
    for k in names:
        line[k] = math.fsum(r[k] for r in rows) / n
    line["loss"] = math.fsum(r["_total"] for r in rows) / n
    line["grad_norm"] = math.fsum(r["grad_norm"] for r in rows) / n
    line["time"] = float(seconds_per_iter)
    return line


def check_finite(rows, iters_per_epoch):
    """Stop the run at the first metered step with a non-finite loss term or gradient norm."""
    for r in rows:
        if r["nonfinite"]:
            it = r["t"] + 1
            raise FloatingPointError("non-finite %s at epoch %d, iteration %d (optimizer step %d)"
                                     % (", ".join(r["nonfinite"]), r["t"] // max(iters_per_epoch, 1) + 1, it, r["t"]))


# ---- checkpoints --------------------------------------------------------------------------------------------------
def _to_cpu(v):
    if torch.is_tensor(v):
        return v.detach().cpu()
    if isinstance(v, dict):
        return {k: _to_cpu(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_to_cpu(x) for x in v)
    return v


def make_checkpoint(model, trainer, meter, meta):
    """{"meta", "state_dict", "trainer", "meter"}: ``state_dict`` is the model's, under the key mmcv uses, so that
    ``infer.load_checkpoint`` and the reference's tools read the file; ``trainer`` is ``Trainer.state_dict()``
    without its copy of the model.  Tensors, numbers, strings and containers only (``torch.load(weights_only=True)``)."""
    tsd = dict(trainer.state_dict())
    tsd.pop("model")
    return _to_cpu(dict(meta=dict(meta), state_dict=dict(model.state_dict()), trainer=tsd,
                        meter=None if meter is None else meter.state_dict()))


def restore_checkpoint(ckpt, model, trainer, meter=None):
    """Model, optimizer (moments, step count, lr factor), dropout counter and meter position -> ``meta``."""
    trainer.load_state_dict(dict(ckpt["trainer"], model=ckpt["state_dict"]))
    if meter is not None and ckpt.get("meter") is not None:
        meter.load_state_dict(ckpt["meter"])
    return ckpt["meta"]


def _atomic_save(obj, path):
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)                       # (a reader sees the old file or the whole new one)


def save_checkpoint(work_dir, epoch, ckpt, max_keep_ckpts=DEFAULTS["max_keep_ckpts"]):
    """``epoch_{epoch}.pth`` (written under a temporary name and renamed), then ``latest.pth`` the same way, then
    every ``epoch_*.pth`` but the newest ``max_keep_ckpts`` is deleted (``max_keep_ckpts`` <= 0 keeps all)."""
    os.makedirs(work_dir, exist_ok=True)
    path = os.path.join(work_dir, f"epoch_{int(epoch)}.pth")
    _atomic_save(ckpt, path)
    _atomic_save(ckpt, os.path.join(work_dir, "latest.pth"))
    if max_keep_ckpts > 0:
        found = []
        for p in glob.glob(os.path.join(work_dir, "epoch_*.pth")):
            m = re.fullmatch(r"epoch_(\d+)\.pth", os.path.basename(p))
            if m:
                found.append((int(m.group(1)), p))
        for _, p in sorted(found)[:-max_keep_ckpts]:
            os.remove(p)
    return path


def load_checkpoint_file(path):
    return torch.load(path, map_location="cpu", weights_only=True)


# ---- the loop -----------------------------------------------------------------------------------------------------
def _lookahead(it):
    """(item, next item or None) pairs."""
    it = iter(it)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, nxt
        cur = nxt
    yield cur, None


class _Log:
    """``path`` None: a rank that keeps no log (every rank but 0) - lines are dropped."""

    def __init__(self, path, echo=True):
        self.f = None if path is None else open(path, "a")
        self.echo = echo

    def write(self, line):
        if self.f is None:
            return
        text = json.dumps(line)
        self.f.write(text + "\n")
        self.f.flush()
        if self.echo:
            print(text, flush=True)

    def close(self):
        if self.f is not None:
            self.f.close()


def model_loss_names(model):
    """The scalars the step meter records for ``model``, in the order of its columns: the loss terms its head has
    (``modules.VoteNet``'s CAVoteHead has no ``center_loss``), the vote loss and their sum."""
    from .meter import loss_names
    head = getattr(model, "bbox_head", None)
    terms = getattr(head, "LOSS_NAMES", None)
    return loss_names() if terms is None else tuple(terms) + ("vote_loss", "_total")


def validate(model, val_set, batch_size, workers, num_points, img_scale, seed=0):
    """One validation pass: ``infer.run_test`` into a fresh store, ``val_set.evaluate``; the model goes back to
    ``train()`` (for ``DeMFVoteNet`` that keeps the image branch in eval).  Under ranks: rank 0's buffers (the
    BatchNorm statistics, which every rank has updated from its own batches) go to every rank first, the pass runs
    sharded, rank 0 evaluates the merged store and its dict is broadcast - every rank returns the same."""
    from . import infer, ranks
    try:
        ranks.broadcast_buffers(model)
        store = infer.run_test(model, val_set, batch_size=batch_size, workers=workers, num_points=num_points,
                               img_scale=img_scale, seed=seed)
        return ranks.broadcast_object(val_set.evaluate(store) if ranks.rank() == 0 else None)
    finally:
        model.train()


def fit(model, train_set, work_dir, *, val_set=None, batch_size=DEFAULTS["batch_size"],
        max_epochs=DEFAULTS["max_epochs"], repeat=DEFAULTS["repeat"], lr=DEFAULTS["lr"],
        weight_decay=DEFAULTS["weight_decay"], max_grad_norm=DEFAULTS["max_grad_norm"],
        lr_steps=DEFAULTS["lr_steps"], gamma=DEFAULTS["gamma"], log_interval=DEFAULTS["log_interval"],
        ckpt_interval=DEFAULTS["ckpt_interval"], max_keep_ckpts=DEFAULTS["max_keep_ckpts"],
        eval_interval=DEFAULTS["eval_interval"], seed=DEFAULTS["seed"], workers=DEFAULTS["workers"], graphs=True,
        resume_from=None, load_from=None, num_points=20000, img_scale=(1333, 800), on_step=None, echo=True,
        val_batch_size=None, accumulate=DEFAULTS["accumulate"], feature_cache=None):
    """Train ``model`` (a ``DeMFVoteNet``: frozen image stream + hot path; or a model without ``extract_img_feat``,
    ``modules.VoteNet``: from points alone - the loader then reads, decodes and uploads no image) on ``train_set`` for
    ``max_epochs`` runner epochs of ``repeat`` passes each.  -> dict(trainer, meter, stepper, epoch, iter, val).

    ``on_step(info)``: called after every micro-step has been enqueued, ``info = dict(epoch, iter, indices, loss,
    micro)`` with the 1-based epoch and global iteration, the batch's dataset indices, the batch's loss as a DEVICE
    tensor (reading it synchronises; the loop itself does not) and the micro-step's position in its group.

    ``accumulate`` = W > 1: every optimizer step is formed from W consecutive batches (``engine.Trainer``);
    ``iter``, the meter's ``t``, ``log_interval`` and the log lines count optimizer steps, groups run across the
    ``repeat`` passes of a runner epoch, and the fewer than W batches left over at its end are abandoned
    (``accumulation_plan``; the epoch's last log line carries ``discarded``), so that checkpoints, learning-rate
    changes and validation fall on step boundaries.

    ``feature_cache`` (a ``featcache.FeatureCache`` of ``train_set`` for this model's image branch): the loader opens
    no image file (``SceneLoader(with_img=False, image_shapes=cache.ori_shapes)``) and every batch's image features
    are ``feature_cache.assemble(batch.indices, batch["img_metas"])``; ``model.extract_img_feat`` is not called in
    the training loop.  Validation still computes the stream: a validation scene is seen once per pass.

    In a process group of W > 1 ranks (``engine.init_distributed``) this is one rank of a data-parallel run: the
    loader yields the rank's share, ``on_step`` sees the rank's indices, every rank returns the same ``val``, and the
    log and the checkpoints are rank 0's (module docstring)."""
    from . import engine, infer, ranks
    from .meter import StepMeter
    from .modules import DeMFHotPath
    from .pipeline import SceneLoader
    if batch_size < 1 or max_epochs < 0 or repeat < 1 or log_interval < 1 or ckpt_interval < 1 or eval_interval < 1:
        raise ValueError("batch_size, repeat, log_interval, ckpt_interval and eval_interval must be positive")
    if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
        raise ValueError("accumulate must be a positive integer, got %r" % (accumulate,))
    with_img = hasattr(model, "extract_img_feat")
    if feature_cache is not None:
        if not with_img:
            raise ValueError("feature_cache: the model has no image branch")
        if feature_cache.model is not model or len(feature_cache) != len(train_set):
            raise ValueError("feature_cache was built for another model or for a dataset of another size")
        if tuple(feature_cache.img_scale) != tuple(img_scale):
            raise ValueError("feature_cache holds img_scale %s, the run asks for %s"
                             % (tuple(feature_cache.img_scale), tuple(img_scale)))
    world, rank = ranks.world(), ranks.rank()
    os.makedirs(work_dir, exist_ok=True)
    torch.manual_seed(seed)                       # (the Trainer seeds the dropout counter from it and from the rank)
    model.cuda().train()
    if load_from is not None:
        # weights only (mmcv's load_from): through the model's load_state_dict, which for DeMFVoteNet applies the
        # stage-1 image-branch key remap; a stage-1 file holds the image branch alone, so not strict
        bad = model.load_state_dict(infer._model_state(load_checkpoint_file(load_from)), strict=False)
        if echo and rank == 0:
            print(f"load_from {load_from}: {len(bad.missing_keys)} missing, {len(bad.unexpected_keys)} unexpected keys",
                  flush=True)
    # the runner computes the frozen image features itself and drives the hot path's forward_train
    trainer = engine.Trainer(model, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                             forward=functools.partial(DeMFHotPath.forward_train, model) if with_img else None,
                             accumulate=accumulate)
    names = model_loss_names(model)
    meter = StepMeter(names, ring_rows=max(128, 2 * log_interval))
    trainer.attach_meter(meter)
    epoch0, it = 0, 0
    if resume_from is not None:
        ckpt = load_checkpoint_file(resume_from)
        check_resume_accumulate(ckpt["meta"], accumulate, resume_from)
        check_resume_world(ckpt["meta"], world, resume_from)
        meta = restore_checkpoint(ckpt, model, trainer, meter)
        epoch0, it = int(meta["epoch"]), int(meta["iter"])
        if rank > 0 and trainer.fused:
            # the file holds rank 0's dropout counter [seed, step]: this rank keeps its own seed (engine.Trainer:
            # seed + 7919 * rank) at the checkpoint's step
            from . import fused
            dev = trainer.flat.flat.device
            s0, k0 = fused.get_rng_state(dev)
            fused.set_rng_state(dev, [(s0 + 7919 * rank) & 0x7FFFFFFFFFFFFFFF, k0])
    if feature_cache is not None and (load_from is not None or resume_from is not None):
        feature_cache.verify()                    # (the weights just loaded must be the ones the cache was built from)
    stepper = trainer.bucketed() if graphs else None
    loader = SceneLoader(train_set, batch_size, "train", seed=seed, img_scale=img_scale, num_points=num_points,
                         workers=workers, with_img=with_img and feature_cache is None,
                         image_shapes=None if feature_cache is None else feature_cache.ori_shapes,
                         rank=rank, world=world)
    ipe, dropped = accumulation_plan(len(loader), repeat, accumulate)      # iterations per runner epoch
    log = _Log(os.path.join(work_dir, "train.log.json") if rank == 0 else None, echo)
    rows, marks = [], []                          # meter rows not logged yet; (last t, epoch, iter, s/iter) per interval

    def drain(wait):
        got = meter.collect(wait=wait)
        check_finite(got, ipe)
        rows.extend(got)
        while marks and rows and rows[-1]["t"] >= marks[0][0]:
            last_t, e, i, dt, extra = marks.pop(0)
            k = sum(1 for r in rows if r["t"] <= last_t)
            log.write(dict(format_log(rows[:k], e, i, lr, dt, names), **extra))
            del rows[:k]

    val = None
    try:
        for epoch in range(epoch0, max_epochs):
            trainer.set_epoch(epoch, lr_steps, gamma)
            since, t_mark = 0, time.perf_counter()
            it_end = it + ipe                     # the epoch's last optimizer step

            def mark():
                nonlocal since, t_mark
                now = time.perf_counter()
                if world > 1:
                    trainer.flush()               # (an overlapped collective's update, and its meter row, are owed)
                meter.snapshot()
                # (with accumulate > 1 the epoch's last line says how many batches its open group loses)
                extra = dict(discarded=dropped) if accumulate > 1 and it == it_end else {}
                marks.append((it - 1, epoch + 1, it, (now - t_mark) / since, extra))
                since, t_mark = 0, now

            for rep in range(repeat):
                loader.epoch = loader_epoch(epoch, rep, repeat)
                for batch, nxt in _lookahead(loader):
                    step_batch = dict(points=batch["points"], gt_bboxes_3d=batch["gt_bboxes_3d"],
                                      gt_labels_3d=batch["gt_labels_3d"])
                    if feature_cache is not None:
                        step_batch.update(img_features=feature_cache.assemble(batch.indices, batch["img_metas"]),
                                          img_metas=batch["img_metas"])
                    elif with_img:
                        step_batch.update(img_features=model.extract_img_feat(batch["img"], batch["img_metas"]),
                                          img_metas=batch["img_metas"])
                    micro = trainer.micro
                    if stepper is not None:
                        loss = stepper.step(step_batch, next_points=None if nxt is None else nxt["points"])
                    else:
                        loss = trainer.step(step_batch)
                    stepped = trainer.micro == 0  # (the group's last micro-step: an optimizer step has been enqueued)
                    if on_step is not None:
                        on_step(dict(epoch=epoch + 1, iter=it + 1, indices=tuple(batch.indices), loss=loss,
                                     micro=micro))
                    if stepped:
                        it += 1
                        since += 1
                        if since >= log_interval:
                            mark()
                    drain(False)
            if trainer.micro:
                trainer.reset_accumulation()      # the epoch's incomplete group (``dropped`` batches) is abandoned
            if since:
                mark()                            # the tail of the epoch
            drain(True)
            done = epoch + 1
            if done % ckpt_interval == 0 or done == max_epochs:
                meta = dict(epoch=done, iter=it, seed=int(seed), repeat=int(repeat), batch_size=int(batch_size),
                            lr=float(lr), lr_steps=[int(s) for s in lr_steps], gamma=float(gamma),
                            max_epochs=int(max_epochs), accumulate=int(accumulate))
                if world > 1:
                    meta["world"] = int(world)
                if rank == 0:
                    save_checkpoint(work_dir, done, make_checkpoint(model, trainer, meter, meta), max_keep_ckpts)
                ranks.barrier()                   # (no rank runs ahead of a file another run may resume from)
            if val_set is not None and (done % eval_interval == 0 or done == max_epochs):
                trainer.flush()
                val = validate(model, val_set, val_batch_size or batch_size, workers, num_points, img_scale, seed)
                log.write(dict(mode="val", epoch=done, iter=it, **val))
    finally:
        log.close()
    return dict(trainer=trainer, meter=meter, stepper=stepper, epoch=max(epoch0, max_epochs), iter=it, val=val)


# ---- command line -------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m demf_amd.train", description=__doc__.split("\n")[0])
    p.add_argument("--data-root", required=True)
    p.add_argument("--ann-file", required=True, help="training infos file, absolute or relative to --data-root")
    p.add_argument("--work-dir", required=True, help="checkpoints and train.log.json go here")
    p.add_argument("--val-ann-file", default=None, help="validation infos file (none: no validation)")
    p.add_argument("--load-from", default=None, help="weights to start from (for example a stage-1 image checkpoint)")
    p.add_argument("--resume-from", default=None, help="a checkpoint of this runner: continue with its next epoch")
    p.add_argument("--no-validate", action="store_true")
    p.add_argument("--no-graphs", action="store_true", help="eager steps instead of captured hipGraphs")
    p.add_argument("--batch-size", type=int, default=DEFAULTS["batch_size"])
    p.add_argument("--epochs", type=int, default=DEFAULTS["max_epochs"])
    p.add_argument("--seed", type=int, default=DEFAULTS["seed"])
    p.add_argument("--workers", type=int, default=DEFAULTS["workers"],
                   help="loader threads PER PROCESS: with --gpus N the job runs N times as many (a job that is given "
                        "16 CPUs in all has 2 per rank at N = 8)")
    p.add_argument("--gpus", type=int, default=None,
                   help="run as N data-parallel ranks, one GPU each (started here unless a launcher already set RANK)")
    p.add_argument("--log-interval", type=int, default=DEFAULTS["log_interval"])
    p.add_argument("--accumulate", type=int, default=DEFAULTS["accumulate"],
                   help="batches per optimizer step (8: the reference's 8-GPU step on one GPU)")
    p.add_argument("--autoscale-lr", action="store_true",
                   help="the reference's linear scaling rule: lr x (accumulate x ranks) / 8")
    p.add_argument("--model", choices=("demf", "votenet"), default="demf",
                   help="demf: DeMFVoteNet (configs/demf/demf_votenet.py); votenet: the points-only class-agnostic "
                        "baseline (configs/baseline/votenet.py), trained without reading an image")
    p.add_argument("--feature-cache", default=None, metavar="DIR",
                   help="train from cached image tokens: load the frozen image-feature cache in DIR, or build and "
                        "save it there; the loop then decodes no image and does not run the image stream")
    p.add_argument("--feature-cache-dtype", choices=("fp32", "bf16"), default=None,
                   help="storage of a cache that has to be built (default fp32)")
    args = p.parse_args(argv)
    if args.feature_cache_dtype is not None and args.feature_cache is None:
        p.error("--feature-cache-dtype needs --feature-cache")
    if args.feature_cache is not None and args.model != "demf":
        p.error("--feature-cache needs a model with an image branch (--model demf)")
    if args.batch_size < 1 or args.workers < 1 or args.log_interval < 1 or args.accumulate < 1:
        p.error("--batch-size, --workers, --log-interval and --accumulate must be positive")
    if args.epochs < 0:
        p.error("--epochs must not be negative")
    if args.gpus is not None and args.gpus < 1:
        p.error("--gpus must be positive")
    if args.load_from and args.resume_from:
        p.error("--load-from and --resume-from exclude each other (a resumed run takes its weights from the checkpoint)")
    return args


def open_feature_cache(directory, model, train_set, dtype=None, load_from=None, resume_from=None,
                       img_scale=(1333, 800), echo=True):
    """The ``--feature-cache DIR`` of the command line: the weights the run starts from go into ``model`` first (the
    cache is a function of the image branch; ``fit`` loads them again, which changes nothing), then a valid cache in
    ``directory`` is loaded - one of ``dtype`` if that is given -, otherwise one is built and saved there."""
    from . import featcache, infer
    model.cuda()
    if load_from is not None:
        model.load_state_dict(infer._model_state(load_checkpoint_file(load_from)), strict=False)
    elif resume_from is not None:
        model.load_state_dict(load_checkpoint_file(resume_from)["state_dict"], strict=False)
    why = "no cache there"
    if os.path.exists(os.path.join(directory, featcache.INDEX_FILE)):
        try:
            cache = featcache.FeatureCache.load(directory, model, train_set)
            if (dtype is None or cache.dtype == dtype) and tuple(cache.img_scale) == tuple(img_scale):
                if echo:
                    print(f"feature cache {directory}: loaded {len(cache)} scenes, {cache.nbytes} bytes, {cache.dtype}",
                          flush=True)
                return cache
            why = f"it holds {cache.dtype} at img_scale {tuple(cache.img_scale)}"
            del cache
        except (ValueError, OSError) as e:
            why = str(e)
    if echo:
        print(f"feature cache {directory}: building ({why})", flush=True)
    cache = featcache.FeatureCache.build(model, train_set, img_scale=img_scale, dtype=dtype or "fp32")
    cache.save(directory)
    return cache


def main(argv=None, model=None, **fit_kwargs):
    """-> what ``fit`` returns.  ``model``: the detector to train instead of the full-size ``DeMFVoteNet()``;
    ``fit_kwargs`` go to ``fit`` (``num_points``, ``img_scale``, schedule overrides, ``on_step``)."""
    args = parse_args(argv)
    from . import ranks
    if "RANK" in os.environ:
        from . import engine
        ranks.check_gpus(args.gpus)
        engine.init_distributed()
    elif args.gpus is not None and args.gpus > 1:
        if model is not None or fit_kwargs:
            raise ValueError("--gpus starts new processes: a model or fit arguments given in this one cannot follow")
        return ranks.launch("demf_amd.train", sys.argv[1:] if argv is None else list(argv), args.gpus)
    from .dataset import SUNRGBDDataset
    train_set = SUNRGBDDataset(args.data_root, args.ann_file)
    val_set = None
    if args.val_ann_file and not args.no_validate:
        val_set = SUNRGBDDataset(args.data_root, args.val_ann_file, test_mode=True)
    if model is None:
        from .modules import DeMFVoteNet, VoteNet
        model = VoteNet() if args.model == "votenet" else DeMFVoteNet()
    kw = dict(val_set=val_set, batch_size=args.batch_size, max_epochs=args.epochs, seed=args.seed,
              workers=args.workers, log_interval=args.log_interval, graphs=not args.no_graphs,
              resume_from=args.resume_from, load_from=args.load_from, accumulate=args.accumulate)
    if args.autoscale_lr:
        kw["lr"] = autoscale_lr(DEFAULTS["lr"], args.accumulate, ranks.world())
    kw.update(fit_kwargs)
    if args.feature_cache is not None:
        # rank 0 opens first, building and saving the cache if it has to; the others load what it left (every rank
        # holds the whole cache: the permutation is global)
        opened = functools.partial(open_feature_cache, args.feature_cache, model, train_set, args.feature_cache_dtype,
                                   load_from=kw.get("load_from"), resume_from=kw.get("resume_from"),
                                   img_scale=kw.get("img_scale", (1333, 800)))
        if ranks.world() > 1:
            # (without --load-from / --resume-from every rank has drawn its own weights: the cache is a function of
            # the image branch, so the replicas are made identical here already, not only by the Trainer)
            ranks.broadcast_buffers(model.cuda(), parameters=True)
        if ranks.rank() == 0:
            kw["feature_cache"] = opened()
        ranks.barrier()
        if ranks.rank() != 0:
            kw["feature_cache"] = opened(echo=False)
    return fit(model, train_set, args.work_dir, **kw)


if __name__ == "__main__":
    _ret = main(sys.argv[1:])
    sys.exit(_ret if isinstance(_ret, int) else 0)
