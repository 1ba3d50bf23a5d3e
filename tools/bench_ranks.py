"""Time the rank merges (csrc/ranks.hip) on one GPU.

    python tools/bench_ranks.py [--reps 20] [--out profiles/ranks_bench.json]

store_concat  W = 8 ranks, the validation set's 5 050 scenes (632 per rank, the last rank 626), every rank's store at
              its worst-case capacity (K = 256 candidates x C = 10 classes = 2 560 rows per scene) and a realistic
              fill (0 .. 80 rows per scene, seeded).  The launch is sized for the capacity; the rows that exist decide
              the traffic.  Next to it: one device-to-device copy of the bytes the merge moves (the filled rows' 36
              bytes each plus the scene offsets), measured in the same run.
meter_merge   W = 8 rings of 128 rows (64 KiB in, 8 KiB out), next to a device-to-device copy of the 64 KiB.

Device events around the work, three warm-up rounds, best and median of --reps repetitions.  The arrays are made in
place: no process group, no communication - a validation pass runs the first once, a log interval the second once.
There is no pass bar; the numbers are reported.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, SCENES, ROWS_PER_SCENE, MAX_FILL, RING_ROWS = 8, 5050, 2560, 80, 128


def _events(fn, reps):
    import torch
    ms = []
    for i in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
    return dict(ms_best=round(min(ms), 4), ms_median=round(statistics.median(ms), 4), reps=reps)


def bench_store_concat(reps):
    import numpy as np
    import torch
    from demf_amd import ops
    from demf_amd.detections import DetectionStore
    rng = np.random.default_rng(0)
    q = -(-SCENES // W)
    counts = [max(0, min(SCENES, (r + 1) * q) - r * q) for r in range(W)]
    R = q * ROWS_PER_SCENE
    off = np.zeros((W, q + 1), np.int32)
    for r in range(W):
        off[r, 1:counts[r] + 1] = np.cumsum(rng.integers(0, MAX_FILL + 1, size=counts[r]))
    rows = [int(off[r, counts[r]]) for r in range(W)]
    state = np.array([[n, 0] for n in rows], np.int32)
    dev = "cuda"
    src = [torch.from_numpy(off).to(dev), torch.from_numpy(state).to(dev),
           torch.randn((W, R, 7), device=dev), torch.rand((W, R), device=dev),
           torch.randint(0, 10, (W, R), dtype=torch.int32, device=dev)]
    out = DetectionStore(SCENES, max_rows=W * R, device=dev)
    run = lambda: ops.store_concat(counts, *src, out.boxes, out.scores, out.labels, out.scene_off, out.state)  # noqa: E731
    run()
    out._scenes = SCENES
    host_off, total = out.host_index()
    assert total == sum(rows) and host_off[-1] == total
    merge = _events(run, reps)
    moved = total * 36 + (SCENES + 1) * 4
    a = torch.empty(moved, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    copy = _events(lambda: b.copy_(a), reps)
    return dict(W=W, scenes=SCENES, scenes_per_rank=q, rows_capacity_per_rank=R, rows_filled=total,
                bytes_moved=moved, capacity_bytes=W * R * 36, store_concat=merge, d2d_copy_same_bytes=copy)


def bench_meter_merge(reps):
    import numpy as np
    import torch
    from demf_amd import meter, ops
    rings = np.stack([meter.empty_ring(RING_ROWS) for _ in range(W)])
    for r in range(W):
        rings[r, :, :2] = np.arange(RING_ROWS, dtype=np.int64).view(np.int32).reshape(RING_ROWS, 2)
    rings.view(np.float32)[:, :, 3:] = np.random.default_rng(1).random((W, RING_ROWS, 13), dtype=np.float32)
    rings[:, :, 2] = 0
    dev_rings = torch.from_numpy(rings).cuda()
    out = torch.empty((RING_ROWS, 16), dtype=torch.int32, device="cuda")
    merge = _events(lambda: ops.meter_merge(dev_rings, out), reps)
    rows, nxt = meter.decode_ring(out.cpu().numpy(), meter.loss_names(), 0)
    assert nxt == RING_ROWS and len(rows) == RING_ROWS
    twin = torch.empty_like(dev_rings)
    copy = _events(lambda: twin.copy_(dev_rings), reps)
    return dict(W=W, rows=RING_ROWS, bytes_in=int(dev_rings.numel() * 4), bytes_out=int(out.numel() * 4),
                meter_merge=merge, d2d_copy_same_bytes=copy)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranks_bench.json"))
    args = p.parse_args(argv)
    import torch
    result = dict(device=torch.cuda.get_device_name(0), store_concat=bench_store_concat(args.reps),
                  meter_merge=bench_meter_merge(args.reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
