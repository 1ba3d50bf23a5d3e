"""Time the training step of the points-only VoteNet baseline next to the DeMF hot path's, in one process on one GPU.

    python tools/bench_baseline.py [--batch 8 16] [--windows 7] [--window-steps 200] [--out FILE]

What is timed is the step ``bench.py`` times, for both models the same way: ``engine.Trainer.capture`` - forward + loss +
backward + gradient pack + norm + clip + AdamW as ONE hipGraph, the next batch's index pre-pass launched in front of it
on a side stream - at the reference's sizes (20 000 points, 256 proposals; DeMF with its 18 609 image tokens), in two
loops: ``new`` = 4 distinct HBM-resident batches cycled through ``replay.load()`` (target padding, static-buffer copies
and, for DeMF, the token conversion and the meta refresh are inside the timed step), ``resident`` = one batch replayed.
If the baseline's step is not the faster one, something fell onto a slow kernel form.

Protocol: both steps are captured and warmed first; then windows of ``--window-steps`` steps each, the models and the two
loops alternating window by window, every window timed by device events around it; reported are the median and the
minimum / maximum over the windows, in ms per step.  One JSON line on stdout (and in ``--out``).

    python tools/bench_baseline.py --trace-passes 30

runs no timing: 30 eager training passes and 30 test passes (eval forward + get_bboxes_packed) of the baseline at
B = 8, the workload ``profiles/baseline_kernel_stats.txt`` was traced on -

    rocprofv3 --kernel-trace --stats -d OUT -o votenet -- python tools/bench_baseline.py --trace-passes 30
    python tools/bench_baseline.py --kernel-table OUT/votenet_results.db > profiles/baseline_kernel_stats.txt"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_GT = 16


def _seed_weights(module, seed):
    """Deterministic, well-conditioned weights (fan-in scaled matrices, BatchNorm scales near 1)."""
    import math

    import torch
    g = torch.Generator().manual_seed(seed)
    out = {}
    sd = module.state_dict()
    for k in sorted(sd):
        v = sd[k]
        if k.endswith(("num_batches_tracked", "running_mean")):
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            out[k] = torch.ones_like(v)
        elif v.dim() >= 2:
            out[k] = torch.randn(v.shape, generator=g) / math.sqrt(v[0].numel())
        elif k.endswith("weight"):
            out[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    module.load_state_dict(out)


def _batches(B, n, with_img):
    import torch

    from demf_amd.config import BATCH_INPUT_SHAPE, PYRAMID_SHAPES
    from demf_amd.synthetic import make_scene_batch
    out = []
    for seed in range(1, n + 1):
        raw = make_scene_batch(B, 20000, PYRAMID_SHAPES if with_img else ((2, 2),), BATCH_INPUT_SHAPE if with_img else (32, 32),
                               256 if with_img else 4, seed=seed, n_gt=8)
        b = dict(points=torch.from_numpy(raw["points"]).cuda(),
                 gt_bboxes_3d=[torch.from_numpy(x).cuda() for x in raw["gt_boxes"]],
                 gt_labels_3d=[torch.from_numpy(x).cuda() for x in raw["gt_labels"]])
        if with_img:
            b.update(img_features=[torch.from_numpy(f).cuda() for f in raw["img_features"]], img_metas=raw["img_metas"])
        out.append(b)
    return out


def build(B, seed=1):
    """-> {name: (replay, batches)}: the captured training step of each model and its four batches."""
    from demf_amd import engine
    from demf_amd.config import DeMFCfg, VoteNetCfg
    from demf_amd.modules import DeMFHotPath, VoteNet
    out = {}
    for name, model, with_img in (("votenet", VoteNet(VoteNetCfg()), False), ("demf_hot_path", DeMFHotPath(DeMFCfg()), True)):
        _seed_weights(model, seed)
        model.cuda().train()
        batches = _batches(B, 4, with_img)
        trainer = engine.Trainer(model, lr=1e-4)
        out[name] = (trainer.capture(batches[0], max_gt=MAX_GT), batches)
    return out


def time_windows(steps_by_name, windows, steps):
    """Alternating windows of ``steps`` steps -> {(name, loop): [ms per step, one per window]}."""
    import torch
    loops = {}
    for name, (replay, batches) in steps_by_name.items():
        def new(k, replay=replay, batches=batches):
            replay.load(batches[k % len(batches)])
            return replay(next_points=batches[(k + 1) % len(batches)]["points"])

        def resident(k, replay=replay, batches=batches):
            return replay(next_points=batches[0]["points"])
        loops[(name, "new")], loops[(name, "resident")] = new, resident
    last = {}
    for key, fn in loops.items():                   # every loop warm before the first timed window
        for k in range(12):
            last[key] = fn(k)
        if key[1] == "new":
            steps_by_name[key[0]][0].load(steps_by_name[key[0]][1][0])
    torch.cuda.synchronize()
    times = {k: [] for k in loops}
    for _ in range(windows):
        for key, fn in loops.items():
            if key[1] == "resident":
                steps_by_name[key[0]][0].load(steps_by_name[key[0]][1][0])
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for k in range(steps):
                last[key] = fn(k)
            t1.record()
            torch.cuda.synchronize()
            times[key].append(t0.elapsed_time(t1) / steps)
    return times, {k: float(v) for k, v in last.items()}


def trace_passes(n, B=8):
    """The workload of the kernel trace: n eager training passes, then n test passes of the baseline."""
    import torch

    from demf_amd.config import VoteNetCfg
    from demf_amd.modules import VoteNet
    model = VoteNet(VoteNetCfg())
    _seed_weights(model, 1)
    model.cuda().train()
    batch = _batches(B, 1, False)[0]
    params = [p for p in model.parameters() if p.requires_grad]
    for _ in range(n):
        losses = model.forward_train(batch["points"], None, batch["gt_bboxes_3d"], batch["gt_labels_3d"])
        torch.autograd.grad(losses["_total"], params, allow_unused=True)
    model.eval()
    for _ in range(n):
        model.bbox_head.get_bboxes_packed(batch["points"], model.forward_head(batch["points"]), None)
    torch.cuda.synchronize()
    print("traced %d training and %d test passes, last loss %.4f" % (n, n, float(losses["_total"].detach())))


def kernel_table(db_path):
    """The per-kernel table of a rocprofv3 results database (its ``kernels`` view) on stdout."""
    import re
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels "
                      "group by name order by sum(duration) desc").fetchall()
    total = sum(r[2] for r in rows)
    fmt = lambda r: "%-72s %5d %10.1f %8.2f %8.2f %8.2f %5.1f%%" % (                      # noqa: E731
        re.sub(r"\(.*", "", r[0])[-70:], r[1], r[2] / 1e3, r[3] / 1e3, r[4] / 1e3, r[5] / 1e3, 100 * r[2] / total)
    print("# rocprofv3 --kernel-trace, VoteNet baseline at the reference's sizes, B = 8, eager: 30 x (forward + loss + "
          "backward), then 30 x (eval forward + get_bboxes_packed)")
    print("# name, calls, total us, mean us, min us, max us, share of all kernel time")
    for r in rows[:25]:
        print(fmt(r))
    print("# the new kernels")
    for r in rows:
        if "ca_" in r[0]:
            print(fmt(r))
    print("# all kernel time: %.1f us over %d kernel names" % (total / 1e3, len(rows)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-passes", type=int, default=0, help="run the kernel trace's workload instead of timing")
    ap.add_argument("--kernel-table", default=None, help="print the per-kernel table of a rocprofv3 results database")
    args = ap.parse_args(argv)
    if args.kernel_table:
        return kernel_table(args.kernel_table)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_baseline needs a HIP device: a time taken elsewhere says nothing")
    if args.trace_passes:
        return trace_passes(args.trace_passes)
    result = dict(what="engine.Trainer.capture: fwd + loss + bwd + pack + clip + AdamW as one hipGraph, pre-pass of the next "
                       "batch in front; new = 4 batches cycled through replay.load(), resident = one batch; ms per step",
                  device=torch.cuda.get_device_name(0), windows=args.windows, window_steps=args.window_steps, batch={})
    for B in args.batch:
        steps = build(B)
        times, last = time_windows(steps, args.windows, args.window_steps)
        row = {}
        for (name, loop), t in times.items():
            assert last[(name, loop)] == last[(name, loop)], (name, loop)      # a finite loss at the end of the loop
            row.setdefault(name, {})[loop] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4),
                                                  max_ms=round(max(t), 4), last_loss=last[(name, loop)])
        for loop in ("new", "resident"):
            row["votenet_over_demf_" + loop] = round(row["votenet"][loop]["median_ms"] /
                                                     row["demf_hot_path"][loop]["median_ms"], 4)
        result["batch"][str(B)] = row
        del steps
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    slow = [B for B, r in result["batch"].items() if max(r["votenet_over_demf_new"], r["votenet_over_demf_resident"]) >= 1.0]
    if slow:
        raise SystemExit("the baseline's step is not faster than the DeMF hot path's at B = %s: look for a slow kernel form"
                         % slow)


if __name__ == "__main__":
    main()
