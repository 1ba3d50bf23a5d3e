"""numpy / float64 restatement of the test-time augmentation merge (demf_amd/tta.py, csrc/tta.hip): the mapping
back of a view's boxes, the three overlap modes, the greedy NMS and the merge, each with the package's tie rules.

Not a test module.  The footprint overlap is ``eval_reference.bev_overlap`` (a world-frame convex clip, a
different construction from the kernel's box-frame slab clip); its centre-distance test is applied to whole rows
at once here, so that only pairs that can overlap reach the Python clip.
"""
import math

import numpy as np

import eval_reference as er

MODES = ("bev", "aligned", "3d")


def map_back(boxes, params):
    """The inverse of ``pipeline.apply_aug_params(boxes, meta, params)`` on boxes (n,7), float64."""
    b = np.asarray(boxes, np.float64).reshape(-1, 7).copy()
    angle, scale = float(params["angle"]), float(params["scale"])
    b[:, :3] -= np.asarray(params["trans"], np.float64)
    b[:, :6] /= scale
    c, s = math.cos(angle), math.sin(angle)
    x, y = b[:, 0].copy(), b[:, 1].copy()
    b[:, 0], b[:, 1] = x * c + y * s, -x * s + y * c
    b[:, 6] += angle
    if params["flip"]:
        b[:, 0] = -b[:, 0]
        b[:, 6] = math.pi - b[:, 6]
    return b


def params_of_row(row):
    """A (8,) parameter row [flip, cos, sin, scale, tx, ty, tz, -] -> the parameter dict (float64)."""
    row = np.asarray(row, np.float64)
    return dict(flip=bool(row[0] != 0.0), angle=math.atan2(row[2], row[1]), scale=float(row[3]), trans=row[4:7])


def iou(a, b, mode="bev"):
    a, b = [float(v) for v in a], [float(v) for v in b]
    if mode == "aligned":
        l = max(0.0, min(a[0] + a[3] / 2, b[0] + b[3] / 2) - max(a[0] - a[3] / 2, b[0] - b[3] / 2))
        w = max(0.0, min(a[1] + a[4] / 2, b[1] + b[4] / 2) - max(a[1] - a[4] / 2, b[1] - b[4] / 2))
        ov = l * w
        return ov / max(a[3] * a[4] + b[3] * b[4] - ov, 1e-8)
    if mode == "3d":
        return er.box3d_iou(a, b)
    assert mode == "bev", mode
    ov = er.bev_overlap(a, b)
    return ov / max(a[3] * a[4] + b[3] * b[4] - ov, 1e-8)


def iou_row(boxes, i, mode, cols=None):
    """IoU of box i with the boxes ``cols`` (default: all) -> (len(cols),) float64."""
    boxes = np.asarray(boxes, np.float64)
    cols = np.arange(len(boxes)) if cols is None else np.asarray(cols)
    out = np.zeros(len(cols))
    if mode == "aligned":
        near = np.ones(len(cols), bool)
    else:       # eval_reference.bev_overlap's own test, for a whole row: further apart than the half-diagonals -> 0
        r = 0.5 * np.hypot(boxes[:, 3], boxes[:, 4])
        d = np.hypot(boxes[cols, 0] - boxes[i, 0], boxes[cols, 1] - boxes[i, 1])
        near = ~(d > r[i] + r[cols])
    for k in np.nonzero(near)[0]:
        out[k] = iou(boxes[i], boxes[cols[k]], mode)
    return out


def iou_matrix(boxes, mode):
    """(n,n) float64, symmetric; only the upper triangle is computed."""
    n = len(boxes)
    out = np.zeros((n, n))
    for i in range(n):
        cols = np.arange(i, n)
        out[i, i:] = iou_row(boxes, i, mode, cols)
    return np.maximum(out, out.T)


def nms(boxes, scores, thr, mode="bev", valid=None, ious=None):
    """Greedy NMS of one segment -> keep (n,) bool.  Visit order: score descending, ties the lower index first;
    candidates: valid rows whose score is neither NaN nor -inf; a visited box that is alive is kept and removes
    every alive box with ``iou > thr``.  ``ious``: a precomputed (n,n) matrix."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    scores = np.asarray(scores)
    n = len(scores)
    cand = np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool).copy()
    cand &= ~np.isnan(scores) & (scores != -np.inf)
    order = sorted(np.nonzero(cand)[0].tolist(), key=lambda i: (-float(scores[i]), i))
    alive, keep = cand.copy(), np.zeros(n, bool)
    for i in order:
        if not alive[i]:
            continue
        keep[i] = True
        alive[i] = False
        cols = np.nonzero(alive)[0]
        if len(cols):
            row = ious[i, cols] if ious is not None else iou_row(boxes, i, mode, cols)
            alive[cols[row > thr]] = False
    return keep


def nms_indices(boxes_xyxyr, scores, thr, mode="bev"):
    """``ops.nms_gpu`` / ``nms_normal_gpu``: (n,5) (x1, y1, x2, y2, ry) -> kept indices in score order."""
    b = np.asarray(boxes_xyxyr, np.float64)
    b7 = np.zeros((len(b), 7))
    b7[:, 0], b7[:, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    b7[:, 3], b7[:, 4], b7[:, 5], b7[:, 6] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], 1.0, b[:, 4]
    keep = nms(b7, scores, thr, mode)
    return np.asarray(sorted(np.nonzero(keep)[0].tolist(), key=lambda i: (-float(scores[i]), i)), np.int64)


def merge(views, params, C, thr, mode="bev", max_num=None):
    """The merge of ONE scene.  views: list over views of (boxes (n,7), scores (n,), labels (n,)) in the view
    store's row order; params: list of parameter dicts.  -> (boxes float64 (m,7), scores, labels int64, source
    (m,2) = (view, row)) ordered by score descending, then class, view, row ascending, cut at ``max_num``."""
    rows = []
    for c in range(C):
        bx, sc, src = [], [], []
        for v, (b, s, l) in enumerate(views):
            sel = np.nonzero(np.asarray(l) == c)[0]
            bx.append(map_back(np.asarray(b).reshape(-1, 7)[sel], params[v]))
            sc.append(np.asarray(s)[sel])
            src += [(v, int(r)) for r in sel]
        bx, sc = np.concatenate(bx), np.concatenate(sc)
        keep = nms(bx, sc, thr, mode)
        rows += [(-float(sc[i]), c, src[i][0], src[i][1], bx[i], sc[i]) for i in np.nonzero(keep)[0]]
    rows.sort(key=lambda r: r[:4])
    if max_num is not None:
        rows = rows[:max_num]
    if not rows:
        return np.zeros((0, 7)), np.zeros((0,), np.float32), np.zeros((0,), np.int64), np.zeros((0, 2), np.int64)
    return (np.stack([r[4] for r in rows]), np.asarray([r[5] for r in rows]),
            np.asarray([r[1] for r in rows], np.int64), np.asarray([r[2:4] for r in rows], np.int64))
