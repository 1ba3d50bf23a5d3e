"""The collective glue of a multi-rank run: what ``train.fit``, ``infer.run_test`` and ``meter.StepMeter`` do with
the process group ``engine.init_distributed`` made.  Without a process group (or with one rank) every function here
is the identity, so a single process runs what it ran before this module existed.

  world(), rank()          the process group's, (1, 0) without one
  gather_stacked(t)        every rank's ``t`` stacked rank-major, the same (W, *t.shape) tensor on every rank
  merge_stores(store, n)   the ranks' DetectionStores -> one store in rank order (ops.store_concat), on every rank
  merge_rings(ring)        the ranks' step-meter rings -> one ring of means (ops.meter_merge), on every rank
  broadcast_buffers(m)     rank 0's buffers (BatchNorm statistics) into every rank, as mmcv's DistEvalHook does
  broadcast_object(o)      rank 0's picklable object on every rank
  launch_command(...)      the ``python -m torch.distributed.run`` line of ``--gpus N``;  launch(...) starts it

The merges themselves are HIP kernels without communication (csrc/ranks.hip); a function here runs ONE collective per
array in front of them and nothing else on the host.
"""
import os
import subprocess
import sys

import torch
import torch.distributed as dist

from . import ops


def world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def barrier():
    if world() > 1:
        dist.barrier()


def gather_stacked(t):
    """``t`` (a contiguous device tensor of 4-byte elements, the same shape on every rank) of every rank ->
    (W, *t.shape), rank-major, identical on every rank.  NCCL / RCCL gathers into the tensor; any other backend
    (gloo: no gather of device tensors into one tensor) runs a SUM all-reduce of a zero-filled (W, ...) int32 view in
    which each rank fills its own slab - x + 0 + ... + 0 in integers is exact, so the result is the same bits."""
    W, r = world(), rank()
    if not t.is_contiguous():
        raise ValueError("gather_stacked takes a contiguous tensor")
    if W == 1:
        return t.unsqueeze(0).clone()
    if dist.get_backend() == "nccl":
        out = torch.empty((W,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t)
        return out
    if t.element_size() != 4:
        raise TypeError(f"gather_stacked: 4-byte elements expected, got {t.dtype}")
    words = torch.zeros((W,) + tuple(t.shape), dtype=torch.int32, device=t.device)
    words[r].copy_(t.view(torch.int32))
    dist.all_reduce(words, op=dist.ReduceOp.SUM)
    return words.view(t.dtype)


def rows_per_scene(model, tta=None):
    """The most rows one scene can hold in a store ``model`` appends to, from its configuration alone (the head's
    ``packed_shape``; with ``tta`` the merge's ``max_num``): what ``DetectionStore.reserve`` is told at the first
    append, known on the host of every rank without communication."""
    head = getattr(model, "pts_bbox_head", None)
    if head is None:
        head = model.bbox_head
    K, C, per_class = head.packed_shape()
    rows = K * C if per_class else K
    if tta is not None and tta.max_num is not None:
        rows = int(tta.max_num)
    return int(rows)


def merge_stores(store, counts):
    """The stores of the W ranks (the same capacity on every rank; rank r appended ``counts[r]`` scenes) -> a new
    ``DetectionStore`` holding all scenes in rank order, the same on every rank.  Five collectives, one launch, no
    host sync beyond what the backend's collective does."""
    from .detections import DetectionStore
    counts = [int(c) for c in counts]
    W = world()
    if len(counts) != W:
        raise ValueError(f"merge_stores: {len(counts)} counts for {W} ranks")
    if counts[rank()] != len(store):
        raise ValueError(f"merge_stores: this rank's store holds {len(store)} scenes, counts says {counts[rank()]}")
    if store.boxes is None:
        raise ValueError("merge_stores: the store has no rows allocated (make it with max_rows)")
    arrays = [gather_stacked(a) for a in (store.scene_off, store.state, store.boxes, store.scores, store.labels)]
    total = sum(counts)
    out = DetectionStore(max(total, 1), max_rows=min(W * store.max_rows, (1 << 31) - 1), device=store.device)
    ops.store_concat(counts, *arrays, out.boxes, out.scores, out.labels, out.scene_off, out.state)
    out._scenes = total
    return out


def merge_rings(ring):
    """This rank's step-meter ring (rows, 16) int32 -> the ring of means over ranks, the same on every rank."""
    return ops.meter_merge(gather_stacked(ring))


def broadcast_buffers(model, parameters=False):
    """Rank 0's buffers into every rank, in place (BatchNorm running statistics differ between ranks after training:
    each rank normalised its own batches).  ``parameters``: the parameters too (what ``engine.Trainer`` does when it
    is made)."""
    if world() > 1:
        if parameters:
            for p in model.parameters():
                dist.broadcast(p.data, src=0)
        for b in model.buffers():
            dist.broadcast(b.data, src=0)


def broadcast_object(obj):
    """Rank 0's ``obj`` on every rank."""
    if world() == 1:
        return obj
    box = [obj if rank() == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return box[0]


def check_gpus(gpus):
    """``--gpus N`` inside a launched rank: N must be the process group's size."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if gpus is not None and int(gpus) != ws:
        raise SystemExit(f"--gpus {gpus} under a launcher with WORLD_SIZE={ws}")


def launch_command(module, argv, gpus, port=None):
    """The command line that runs ``python -m module argv`` as ``gpus`` ranks on this node."""
    if int(gpus) < 1:
        raise ValueError(f"gpus must be positive, got {gpus}")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(gpus)),
           "--master-addr", "127.0.0.1"]
    if port is not None:
        cmd += ["--master-port", str(int(port))]
    return cmd + ["-m", str(module)] + [str(a) for a in argv]


def launch(module, argv, gpus, port=None):
    """Start the ranks as child processes and wait for them (nothing replaces this process, and it has not touched
    the GPU).  -> the launcher's exit status."""
    if port is None and os.environ.get("MASTER_PORT"):
        port = int(os.environ["MASTER_PORT"])
    return subprocess.run(launch_command(module, argv, gpus, port)).returncode
