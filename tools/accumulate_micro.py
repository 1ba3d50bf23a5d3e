"""Cost of gradient accumulation on the captured full-size training step (the bench configuration, synthetic
batches): one W = 8 group (seven 'accumulate' replays + one 'last' replay, engine.Trainer(accumulate=8)) against
eight plain steps of an accumulate=1 trainer - the step as it was before accumulation existed - in one process.

  python tools/accumulate_micro.py [--rounds 6] [--groups 12] [--batch 8] [--accumulate 8] [--out FILE.json]
  python tools/accumulate_micro.py --profile-groups 2        # a few groups only, for a kernel trace

Both trainers carry a step meter, as the runner's always does.  The unit timed is what one optimizer step of the
W = 8 trainer consumes: W batches - device events around the W replays of a group, and around W plain steps.  A round
is ``groups`` such units of one variant, the variants alternate after a warm-up, and the spread reported is the range
of the rounds' medians.  Prints one JSON line (and writes it to ``--out``).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--groups", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--accumulate", type=int, default=8)
    ap.add_argument("--profile-groups", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W = a.accumulate

    import bench
    from demf_amd import engine, meter
    from demf_amd.config import DeMFCfg
    from demf_amd.modules import DeMFHotPath
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    batches = [bench.make_batch(a.batch, seed=1000 + 7919 * i, device=dev)[0] for i in range(2)]

    def build(accumulate):
        torch.manual_seed(0)
        model = DeMFHotPath(DeMFCfg()).to(dev).train()
        tr = engine.Trainer(model, accumulate=accumulate)
        m = meter.StepMeter(meter.loss_names(), ring_rows=max(128, a.groups * W + 8))
        tr.attach_meter(m)
        return tr, m

    plain_tr, plain_m = build(1)
    plain = plain_tr.capture(batches[0], max_gt=8)
    acc_tr, acc_m = build(W)
    first = acc_tr.capture(batches[0], max_gt=8, role="accumulate")
    last = acc_tr.capture(batches[0], max_gt=8, role="last", geo_pipe=first.geo)
    assert plain.update_in_graph and last.update_in_graph and (first.role, last.role) == ("accumulate", "last")
    rows = dict(plain=[], group=[])

    def run(name, units, timed):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(units)]
        torch.cuda.synchronize()
        k = 0
        for s, e in ev:
            s.record()
            for micro in range(W):
                replay = plain if name == "plain" else (last if micro == W - 1 else first)
                replay.load(batches[k % 2])
                replay(next_points=batches[(k + 1) % 2]["points"])
                k += 1
            e.record()
        torch.cuda.synchronize()
        mt = plain_m if name == "plain" else acc_m
        mt.snapshot()
        rows[name].extend(mt.collect(wait=True))
        return [s.elapsed_time(e) for s, e in ev] if timed else None

    if a.profile_groups:
        run("group", a.profile_groups, False)
        print(json.dumps(dict(profiled_groups=a.profile_groups, rows=len(rows["group"]))))
        return
    for name in ("plain", "group"):                         # warm-up
        run(name, 3, False)
    dev_ms = dict(plain=[], group=[])
    for _ in range(a.rounds):
        for name in ("plain", "group"):
            dev_ms[name].append(run(name, a.groups, True))
    out = dict(batch=a.batch, accumulate=W, rounds=a.rounds, units_per_round=a.groups,
               unit="%d batches: one W = %d group / %d plain steps" % (W, W, W),
               plain_rows=len(rows["plain"]), group_rows=len(rows["group"]),
               all_rows_finite=all(not r["nonfinite"] for r in rows["plain"] + rows["group"]),
               optimizer_steps=dict(plain=plain_tr.opt.t, group=acc_tr.opt.t))
    for name in ("plain", "group"):
        med = [statistics.median(r) for r in dev_ms[name]]
        out[name] = dict(device_ms_median=statistics.median(sum(dev_ms[name], [])),
                         device_ms_round_medians=[round(x, 4) for x in med],
                         device_ms_spread=max(med) - min(med))
    out["group_minus_plain_ms"] = out["group"]["device_ms_median"] - out["plain"]["device_ms_median"]
    out["within_expectation"] = out["group_minus_plain_ms"] <= out["plain"]["device_ms_spread"]
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
