"""Cost of the step meter on the captured full-size training step (the bench configuration, synthetic batches): the
same trainer with and without an attached meter (engine.Trainer.attach_meter), two captured graphs of the same step,
alternating in one process.

  python tools/train_meter_micro.py [--rounds 6] [--steps 100] [--batch 8] [--log-interval 50] [--out FILE.json]
  python tools/train_meter_micro.py --profile-steps 5        # a few metered steps only, for a kernel trace

Per step, device events give the time on the GPU's timeline and perf_counter the host time of the loop body - for the
metered rounds that body is the runner's (demf_amd/train.py): the step, a ``snapshot()`` every ``--log-interval``
steps and a ``collect()`` after every step, so the host column shows whether logging costs an enqueue or a wait.  A
round is ``steps`` steps of one variant, the variants alternate after a warm-up, and the spread reported is the range of
the rounds' medians.  Prints one JSON line (and writes it to ``--out``).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--log-interval", type=int, default=50)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import bench
    from demf_amd import engine, meter
    from demf_amd.config import DeMFCfg
    from demf_amd.modules import DeMFHotPath
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = DeMFHotPath(DeMFCfg()).to(dev).train()
    tr = engine.Trainer(model)
    batches = [bench.make_batch(a.batch, seed=1000 + 7919 * i, device=dev)[0] for i in range(2)]
    m = meter.StepMeter(meter.loss_names(), ring_rows=max(128, 2 * a.log_interval, a.steps + 8))
    plain = tr.capture(batches[0], max_gt=8)
    tr.attach_meter(m)
    metered = tr.capture(batches[0], max_gt=8, dry=True, geo_pipe=plain.geo)
    assert plain.update_in_graph and metered.update_in_graph and metered.metered and not plain.metered
    variants = dict(plain=(plain, None), metered=(metered, m))
    seen = []

    def run(name, steps, timed):
        replay, mt = variants[name]
        tr.attach_meter(mt)                                 # (outside the timing: reads the step count once)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        host = []
        torch.cuda.synchronize()
        for k, (s, e) in enumerate(ev):
            s.record()
            t0 = time.perf_counter()
            replay.load(batches[k % 2])
            replay(next_points=batches[(k + 1) % 2]["points"])
            if mt is not None:
                if (k + 1) % a.log_interval == 0:
                    mt.snapshot()
                seen.extend(mt.collect())
            host.append((time.perf_counter() - t0) * 1e3)
            e.record()
        torch.cuda.synchronize()
        if mt is not None:
            mt.snapshot()
            seen.extend(mt.collect(wait=True))
        return ([s.elapsed_time(e) for s, e in ev], host) if timed else None

    if a.profile_steps:
        run("metered", a.profile_steps, False)
        print(json.dumps(dict(profiled_steps=a.profile_steps, rows=len(seen))))
        return
    for name in variants:                                   # warm-up
        run(name, 20, False)
    dev_ms = {k: [] for k in variants}
    host_ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name in variants:
            d, h = run(name, a.steps, True)
            dev_ms[name].append(d)
            host_ms[name].append(h)
    out = dict(batch=a.batch, rounds=a.rounds, steps_per_round=a.steps, log_interval=a.log_interval,
               metered_rows_collected=len(seen), all_rows_finite=all(not r["nonfinite"] for r in seen))
    for name in variants:
        med = [statistics.median(r) for r in dev_ms[name]]
        hmed = [statistics.median(r) for r in host_ms[name]]
        out[name] = dict(device_ms_median=statistics.median(sum(dev_ms[name], [])),
                         device_ms_round_medians=[round(x, 4) for x in med],
                         device_ms_spread=max(med) - min(med),
                         host_ms_median=statistics.median(sum(host_ms[name], [])),
                         host_ms_round_medians=[round(x, 4) for x in hmed],
                         host_ms_max=max(sum(host_ms[name], [])))
    out["metered_minus_plain_us"] = 1e3 * (out["metered"]["device_ms_median"] - out["plain"]["device_ms_median"])
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
