"""numpy / float64 restatement of mmdet3d 0.18.1 ``indoor_eval`` / ``eval_det_cls`` / ``average_precision``
([dep-recall], written from the semantics in demf_amd/evaluation.py), the check of the GPU evaluation.

Not a test module.  The IoU is an exact convex-polygon clip in the world frame (every footprint edge of one
box clips the other's footprint), a different construction from the kernel's box-frame slab clip; the
matching loop is upstream's, literally: per detection in score order a scan of its GT with ``iou > iou_max``.
"""
import math

import numpy as np


def _corners(b, ox, oy):
    """Footprint corners (counter-clockwise), relative to (ox, oy), of a bottom-centre box."""
    x, y, dx, dy, r = float(b[0]) - ox, float(b[1]) - oy, float(b[3]), float(b[4]), float(b[6])
    c, s = math.cos(r), math.sin(r)
    out = []
    for ux, uy in ((-dx / 2, -dy / 2), (dx / 2, -dy / 2), (dx / 2, dy / 2), (-dx / 2, dy / 2)):
        out.append((ux * c + uy * s + x, -ux * s + uy * c + y))    # geometry.rotation_3d_in_axis_z
    return out


def _clip(poly, a, b):
    """Keep the part of ``poly`` left of (or on) the directed line a -> b."""
    ex, ey = b[0] - a[0], b[1] - a[1]
    out = []
    n = len(poly)
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        dp = ex * (p[1] - a[1]) - ey * (p[0] - a[0])
        dq = ex * (q[1] - a[1]) - ey * (q[0] - a[0])
        if (dp >= 0) != (dq >= 0):
            t = dp / (dp - dq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if dq >= 0:
            out.append(q)
    return out


def bev_overlap(b1, b2):
    if float(b1[3]) * float(b1[4]) == 0.0 or float(b2[3]) * float(b2[4]) == 0.0:
        return 0.0
    r1 = 0.5 * math.hypot(float(b1[3]), float(b1[4]))
    r2 = 0.5 * math.hypot(float(b2[3]), float(b2[4]))
    if math.hypot(float(b2[0]) - float(b1[0]), float(b2[1]) - float(b1[1])) > r1 + r2:
        return 0.0
    ox, oy = float(b1[0]), float(b1[1])
    poly = _corners(b2, ox, oy)
    clip = _corners(b1, ox, oy)
    for k in range(4):
        poly = _clip(poly, clip[k], clip[(k + 1) % 4])
        if not poly:
            return 0.0
    a = 0.0
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        a += p[0] * q[1] - q[0] * p[1]
    return abs(a) * 0.5


def box3d_iou(b1, b2):
    """BaseInstance3DBoxes.overlaps(mode='iou') of two bottom-centre depth boxes, float64."""
    z1, h1, z2, h2 = float(b1[2]), float(b1[5]), float(b2[2]), float(b2[5])
    h = max(0.0, min(z1 + h1, z2 + h2) - max(z1, z2))
    inter = bev_overlap(b1, b2) * h if h > 0 else 0.0
    v1 = float(b1[3]) * float(b1[4]) * h1
    v2 = float(b2[3]) * float(b2[4]) * h2
    return inter / max(v1 + v2 - inter, 1e-8)


def iou_matrix(boxes1, boxes2):
    out = np.zeros((len(boxes1), len(boxes2)), np.float64)
    for i, a in enumerate(boxes1):
        for j, b in enumerate(boxes2):
            out[i, j] = box3d_iou(a, b)
    return out


def average_precision(recalls, precisions):
    """average_precision(mode='area') for one scale (float64; upstream stores the result in float32)."""
    mrec = np.concatenate([[0.0], recalls, [1.0]])
    mpre = np.concatenate([[0.0], precisions, [0.0]])
    for i in range(mpre.shape[0] - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1])


def eval_det_cls(pred, gt, iou_thr, iou_fn):
    """pred {img: [(row, box, score)]}, gt {img: [box]} -> ([(rec, prec, ap)] per threshold, {row: [tp]})."""
    class_recs, npos = {}, 0
    for img in gt:
        boxes = np.asarray(gt[img], np.float32).reshape(-1, 7)
        class_recs[img] = {"bbox": boxes, "det": [[False] * len(boxes) for _ in iou_thr]}
        npos += len(boxes)
    image_ids, confidence, ious, rows = [], [], [], []
    for img in pred:
        cur = pred[img]
        if not cur:
            continue
        pb = np.asarray([b for _, b, _ in cur], np.float32).reshape(-1, 7)
        gtb = class_recs[img]["bbox"]
        iou_cur = iou_fn(pb, gtb) if len(gtb) else None
        for i, (row, _, score) in enumerate(cur):
            image_ids.append(img)
            confidence.append(score)
            rows.append(row)
            ious.append(iou_cur[i] if iou_cur is not None else np.zeros(1))
    confidence = np.asarray(confidence, np.float32)
    # the product's order of ties: score descending, then scene, then position (the lists are built so)
    sorted_ind = np.argsort(-confidence, kind="stable")
    image_ids = [image_ids[x] for x in sorted_ind]
    ious = [ious[x] for x in sorted_ind]
    rows = [rows[x] for x in sorted_ind]
    nd = len(image_ids)
    tp_thr = [np.zeros(nd) for _ in iou_thr]
    fp_thr = [np.zeros(nd) for _ in iou_thr]
    for d in range(nd):
        R = class_recs[image_ids[d]]
        iou_max = -np.inf
        BBGT = R["bbox"]
        cur_iou = ious[d]
        jmax = -1
        if len(BBGT) > 0:
            for j in range(len(BBGT)):
                iou = cur_iou[j]
                if iou > iou_max:
                    iou_max = iou
                    jmax = j
        for k, thresh in enumerate(iou_thr):
            if iou_max > thresh:
                if not R["det"][k][jmax]:
                    tp_thr[k][d] = 1.0
                    R["det"][k][jmax] = 1
                else:
                    fp_thr[k][d] = 1.0
            else:
                fp_thr[k][d] = 1.0
    ret = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(len(iou_thr)):
            fp = np.cumsum(fp_thr[k])
            tp = np.cumsum(tp_thr[k])
            recall = tp / float(npos)
            precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            ret.append((recall, precision, average_precision(recall, precision)))
    flags = {rows[d]: [int(tp_thr[k][d]) for k in range(len(iou_thr))] for d in range(nd)}
    return ret, flags


def _np(x):
    t = getattr(x, "tensor", x)
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def indoor_eval_ref(gt_annos, dt_annos, metric, label2cat, iou_fn=iou_matrix):
    """-> (ret_dict with upstream's keys, tp (P, T) in the detections' concatenated row order, per-class
    {label: (ap list, rec list)}).  ``iou_fn(pred (n,7), gt (m,7))`` gives the IoU matrix of one class
    in one scene."""
    assert len(dt_annos) == len(gt_annos)
    pred, gt = {}, {}
    row = 0
    for img, (det, ann) in enumerate(zip(dt_annos, gt_annos)):
        boxes = _np(det["boxes_3d"]).astype(np.float32).reshape(-1, 7)
        labels, scores = _np(det["labels_3d"]).reshape(-1), _np(det["scores_3d"]).astype(np.float32).reshape(-1)
        for i in range(len(labels)):
            label = int(labels[i])
            pred.setdefault(label, {}).setdefault(img, []).append((row, boxes[i], scores[i]))
            gt.setdefault(label, {}).setdefault(img, [])
            row += 1
        if ann["gt_num"] != 0:
            gb = np.asarray(ann["gt_boxes_upright_depth"], np.float32).reshape(-1, 7).copy()
            gb[:, 2] = gb[:, 2] + gb[:, 5] * np.float32(-0.5)
            for i, label in enumerate(np.asarray(ann["class"]).reshape(-1)):
                gt.setdefault(int(label), {}).setdefault(img, []).append(gb[i])
    tp = np.zeros((row, len(metric)), np.uint8)
    per_class = {}
    for label in gt:
        if label in pred:
            res, flags = eval_det_cls(pred[label], gt[label], metric, iou_fn)
            for r, f in flags.items():
                tp[r] = f
            per_class[label] = ([float(a) for _, _, a in res], [float(r[-1]) for r, _, _ in res])
        else:
            per_class[label] = ([0.0] * len(metric), [0.0] * len(metric))
    ret = {}
    labels = sorted(per_class)
    for k, t in enumerate(metric):
        for label in labels:
            ret[f"{label2cat[label]}_AP_{t:.2f}"] = per_class[label][0][k]
        ret[f"mAP_{t:.2f}"] = float(np.mean([per_class[l][0][k] for l in labels])) if labels else float("nan")
        for label in labels:
            ret[f"{label2cat[label]}_rec_{t:.2f}"] = per_class[label][1][k]
        ret[f"mAR_{t:.2f}"] = float(np.mean([per_class[l][1][k] for l in labels])) if labels else float("nan")
    return ret, tp, per_class
