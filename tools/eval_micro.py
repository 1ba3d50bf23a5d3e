"""Device time of the indoor evaluation (demf_amd/evaluation.py) at SUN RGB-D val scale: 5 050 scenes x 512
survivors x 10 classes (per_class_proposal) ~ 26 M detections, ~10 GT per scene.  Inputs are uploaded first;
then the stages are timed with events: score / segment keys + the two stable sorts, the IoU + match kernel,
the gather into class order + the AP kernel.  Prints one JSON line (ms per stage, best of --reps)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=5050)
    ap.add_argument("--survivors", type=int, default=512)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--gt", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from demf_amd import ops
    from demf_amd.evaluation import _desc_score_key, _offsets
    rng = np.random.default_rng(0)
    B, K, C, G = a.scenes, a.survivors, a.classes, a.gt
    # ground truth: G boxes per scene; survivors: jittered GT and random boxes, each repeated once per class
    gt = np.empty((B, G, 7), np.float32)
    gt[..., :2] = rng.uniform(-4, 4, size=(B, G, 2))
    gt[..., 2] = rng.uniform(0, 1, size=(B, G))
    gt[..., 3:6] = rng.uniform(0.3, 2.0, size=(B, G, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, size=(B, G))
    gcls = rng.integers(0, C, size=(B, G))
    surv = np.empty((B, K, 7), np.float32)
    surv[..., :2] = rng.uniform(-4, 4, size=(B, K, 2))
    surv[..., 2:] = gt[:, rng.integers(0, G, size=K), 2:]
    src = rng.integers(0, G, size=(B, K // 4))
    surv[:, :K // 4] = np.take_along_axis(gt, src[..., None].repeat(7, -1), 1) + rng.normal(0, 0.1, (B, K // 4, 7))
    boxes = np.broadcast_to(surv[:, None], (B, C, K, 7)).reshape(-1, 7)
    scores = rng.random(B * C * K).astype(np.float32)
    pcls = np.broadcast_to(np.arange(C)[None, :, None], (B, C, K)).reshape(-1)
    scene = np.broadcast_to(np.arange(B)[:, None, None], (B, C, K)).reshape(-1)
    P = boxes.shape[0]
    pseg = pcls * B + scene
    gseg = (gcls * B + np.arange(B)[:, None]).reshape(-1)
    gorder = np.argsort(gseg, kind="stable")
    pred_counts, gt_counts = np.bincount(pseg, minlength=C * B), np.bincount(gseg, minlength=C * B)
    npos = np.bincount(gcls.reshape(-1), minlength=C)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()        # noqa: E731
    pb, sc = up(boxes), up(scores)
    pseg_d, pcls_d = up(pseg.astype(np.int32)), up(pcls.astype(np.int32))
    pred_off, gt_off = up(_offsets(pred_counts)), up(_offsets(gt_counts))
    gtb = up(gt.reshape(-1, 7)[gorder])
    cls_off, npos_d, ws_off = up(_offsets(np.bincount(pcls, minlength=C))), up(npos.astype(np.int32)), up(_offsets(npos))
    torch.cuda.synchronize()

    def run():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        skey = _desc_score_key(sc)
        order_seg = torch.sort((pseg_d.to(torch.int64) << 32) | skey, stable=True).indices.to(torch.int32)
        order_cls = torch.sort((pcls_d.to(torch.int64) << 32) | skey, stable=True).indices
        ev[1].record()
        tp = ops.eval_match(pb, order_seg, pred_off, gtb, gt_off, (0.25, 0.5), int(pred_counts.max()),
                            int(gt_counts.max()))
        ev[2].record()
        ap_, rec = ops.eval_ap(tp[order_cls], cls_off, npos_d, ws_off, int(npos.sum()))
        ev[3].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], tp, ap_

    best = None
    for _ in range(a.reps):
        t, tp, ap_ = run()
        best = t if best is None else [min(x, y) for x, y in zip(best, t)]
    print(json.dumps({"detections": P, "gt": B * G, "segments": C * B, "iou_pairs": int((pred_counts * gt_counts).sum()),
                      "tp_at_0.25": int(tp[:, 0].sum()), "mAP_0.25": float(ap_[:, 0].mean()),
                      "ms_keys_sort": round(best[0], 3), "ms_iou_match": round(best[1], 3),
                      "ms_gather_ap": round(best[2], 3), "ms_total": round(sum(best), 3)}))


if __name__ == "__main__":
    main()
