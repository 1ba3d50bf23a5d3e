"""Post-processing time per batch: DeMFVoteHead.get_bboxes_packed (decode -> extent/count -> NMS -> pack into a
DetectionStore, no host sync) against another revision's get_bboxes + bbox3d2result, alternating in one process.

  python tools/detect_micro.py [--other-head PATH/head.py] [--rounds 6] [--calls 100] [--B 8] [--K 256] [--N 20000]
  python tools/detect_micro.py --profile-calls 5        # a few calls only, for a kernel trace

--other-head: a copy of demf_amd/modules/head.py of the revision to compare with (for example
``git show REV:demf_amd/modules/head.py``); it is loaded as a sibling module of the package's own head.
Per call, device events give the time on the GPU's timeline (host stalls of a synchronising path included) and
perf_counter the host time; a round is ``calls`` calls of one path, the paths alternate, and the spread reported
is the range of the rounds' medians.  Prints one JSON line.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load_other(path):
    spec = importlib.util.spec_from_file_location("demf_amd.modules._other_head", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-head", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--K", type=int, default=256, help="proposals per ensemble layer (two layers)")
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--profile-calls", type=int, default=0)
    a = ap.parse_args()

    from demf_amd.config import head_kwargs
    from demf_amd.detections import DetectionStore
    from demf_amd.modules.detector import bbox3d2result
    from demf_amd.modules.head import DeMFVoteHead
    from oracle import fixtures
    cfg = fixtures.tiny_cfg()
    pts, dec = fixtures.make_decode_results(0, B=a.B, K=a.K, N=a.N)
    points = torch.from_numpy(pts).cuda()
    preds = dict(decode_res_all=[{k: torch.from_numpy(v).cuda() for k, v in d.items()} for d in dec])
    metas = [dict() for _ in range(a.B)]
    head = DeMFVoteHead(**head_kwargs(cfg)).cuda().eval()
    store = DetectionStore(a.B * max(a.calls, 20, a.profile_calls))      # reset between rounds, outside the timing

    def new():
        head.get_bboxes_packed(points, preds, metas, store)

    paths = {"packed": new}
    if a.other_head:
        other = _load_other(a.other_head).DeMFVoteHead(**head_kwargs(cfg)).cuda().eval()

        def old():
            return [bbox3d2result(b, s, l) for b, s, l in other.get_bboxes(points, preds, metas)]
        paths["other"] = old

    if a.profile_calls:
        for _ in range(a.profile_calls):
            new()
        torch.cuda.synchronize()
        print(json.dumps(dict(profiled_calls=a.profile_calls, rows=store.host_index()[1])))
        return

    for fn in paths.values():                                   # warm-up
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    rows = store.host_index()[1] // 20
    dev_ms = {k: [] for k in paths}
    host_ms = {k: [] for k in paths}
    for _ in range(a.rounds):
        for name, fn in paths.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
            host = []
            store.reset()
            torch.cuda.synchronize()
            for s, e in ev:
                s.record()
                t0 = time.perf_counter()
                fn()
                host.append((time.perf_counter() - t0) * 1e3)
                e.record()
            torch.cuda.synchronize()
            dev_ms[name].append([s.elapsed_time(e) for s, e in ev])
            host_ms[name].append(host)
    out = dict(B=a.B, K=2 * a.K, N=a.N, rounds=a.rounds, calls_per_round=a.calls, rows_per_call=rows)
    for name in paths:
        med = [statistics.median(r) for r in dev_ms[name]]
        hmed = [statistics.median(r) for r in host_ms[name]]
        out[name] = dict(device_ms_median=statistics.median(sum(dev_ms[name], [])),
                         device_ms_round_medians=[round(m, 4) for m in med],
                         device_ms_spread=max(med) - min(med),
                         host_ms_median=statistics.median(sum(host_ms[name], [])),
                         host_ms_round_medians=[round(m, 4) for m in hmed])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
