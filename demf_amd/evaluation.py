"""Indoor 3D detection evaluation on the GPU: mmdet3d 0.18.1 ``indoor_eval`` (restated; [dep-recall] -
mmdet3d's evaluation sources are not in the reference tree).  This is what the reference's
``eval.py --eval mAP`` reports for SUN RGB-D val through ``SUNRGBDDataset.evaluate``
(configs/_base_/datasets/sunrgbd-3d-10class.py:107; README.md:43: mAP@0.25 / mAP@0.5).

Semantics reproduced:
  * classes: every label with at least one ground-truth box OR at least one detection anywhere (upstream's
    parsing creates ``gt[label]`` for predicted labels).  A class with GT but no detection has AP = rec = 0.
    A class with detections but no GT has npos = 0, and upstream's ``tp / npos`` makes its AP and recall NaN,
    hence a NaN mAP / mAR: reproduced, not hidden.  mAP / mAR are plain means over the evaluated classes.
  * a scene with ``gt_num == 0`` contributes no GT; its detections are false positives.
  * GT boxes arrive gravity-centred and are moved to the bottom-centre form in fp32 as
    ``DepthInstance3DBoxes(.., origin=(0.5, 0.5, 0.5))`` does: ``z + dz * (0 - 0.5)``.
  * per class, detections are matched in descending score order; each takes its best GT (the FIRST maximum
    of the 3D IoU, ``BaseInstance3DBoxes.overlaps``) if that IoU is > threshold (strict, fp32 IoU against the
    fp32 threshold) and the GT is not taken yet; otherwise it is a false positive - no fall-back to a
    second-best GT.  AP is ``average_precision(mode='area')`` over ``[0, rec, 1]`` / ``[0, prec, 0]``.
  * order of equal scores: upstream sorts with the unstable ``np.argsort(-confidence)``, so its order of
    ties is undefined.  Here it is defined as score descending, then scene index, then position in that
    scene's result list.  This is a documented choice, not a parity claim.
  * AP and recall are computed in fp64 (upstream's ``average_precision`` stores AP in a float32 array, so
    upstream's number is this one rounded to float32).

Device work (csrc/eval3d.hip): one sort per ordering key (torch.sort, stable), then the segmented IoU +
greedy match kernel (one workgroup per (class, scene) segment) and the AP scan (one workgroup per class).
The number of launches does not depend on the number of scenes or classes.
"""
import numpy as np
import torch

from . import ops
from .config import SUNRGBD_CLASSES
from .detections import DetectionStore


def _rows(x):
    """DepthBoxes / tensor / array -> numpy."""
    t = getattr(x, "tensor", x)
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def _desc_score_key(scores):
    """fp32 scores -> int64 keys in [0, 2^32) that sort ascending in descending score order (-0.0 == 0.0)."""
    bits = (scores + 0.0).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    asc = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF, bits | 0x80000000)
    return 0xFFFFFFFF - asc


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def evaluate_detections(gt_annos, dt_annos, metric=(0.25, 0.5), label2cat=None, with_tp=False, device=None):
    """The device part of :func:`indoor_eval`.  ``dt_annos``: the list of result dicts, or a ``DetectionStore``
    holding one scene per annotation (its boxes and scores are read on the device, never copied to the host and
    back; a store whose rows did not fit raises RuntimeError).  -> dict(classes = the evaluated labels (ascending),
    ap / rec = (C, T) float64, and with ``with_tp`` tp = (P, T) uint8 flags of the detections concatenated
    over scenes in scene order)."""
    if len(gt_annos) != len(dt_annos):
        raise ValueError(f"{len(gt_annos)} ground-truth annotations but {len(dt_annos)} detection results")
    metric = [float(t) for t in metric]
    if not 1 <= len(metric) <= 4:
        raise ValueError(f"indoor_eval takes 1 to 4 IoU thresholds, got {len(metric)}")
    if label2cat is None:
        label2cat = dict(enumerate(SUNRGBD_CLASSES))
    nscene = len(dt_annos)

    store = dt_annos if isinstance(dt_annos, DetectionStore) else None
    if store is not None:
        # ---- a store: boxes and scores stay where they are; the per-row integers come to the host ---
        off, P = store.host_index()                                 # (raises if rows did not fit)
        counts = np.diff(off)
        pb, sc = store.boxes[:P], store.scores[:P]
        labels = store.labels[:P].cpu().numpy().astype(np.int64) if P else np.zeros(0, np.int64)
        if P and bool(torch.isnan(sc).any()):
            raise ValueError("detection scores must not be NaN")
        if device is None:
            device = store.device
    else:
        # ---- host: concatenate every scene ------------------------------------------------------
        pboxes = [_rows(d["boxes_3d"]).reshape(-1, 7) for d in dt_annos]
        counts = np.asarray([len(b) for b in pboxes], np.int64)
        P = int(counts.sum())
        boxes = np.concatenate(pboxes).astype(np.float32) if P else np.zeros((0, 7), np.float32)
        scores = np.concatenate([_rows(d["scores_3d"]).reshape(-1) for d in dt_annos]).astype(np.float32) \
            if nscene else np.zeros(0, np.float32)
        labels = np.concatenate([_rows(d["labels_3d"]).reshape(-1) for d in dt_annos]).astype(np.int64) \
            if nscene else np.zeros(0, np.int64)
        if scores.shape[0] != P or labels.shape[0] != P:
            raise ValueError("every result needs as many scores_3d and labels_3d as boxes_3d")
        if np.isnan(scores).any():
            raise ValueError("detection scores must not be NaN")
    scene = np.repeat(np.arange(nscene, dtype=np.int64), counts)
    gb, gl, gs = [], [], []
    for i, a in enumerate(gt_annos):
        if a["gt_num"] == 0:
            continue
        b = np.asarray(a["gt_boxes_upright_depth"], dtype=np.float32).reshape(-1, 7).copy()
        b[:, 2] = b[:, 2] + b[:, 5] * np.float32(0.0 - 0.5)          # gravity centre -> bottom centre
        gb.append(b)
        gl.append(np.asarray(a["class"], dtype=np.int64).reshape(-1))
        gs.append(np.full(len(b), i, np.int64))
    gboxes = np.concatenate(gb) if gb else np.zeros((0, 7), np.float32)
    glabels = np.concatenate(gl) if gl else np.zeros(0, np.int64)
    gscene = np.concatenate(gs) if gs else np.zeros(0, np.int64)
    if glabels.shape[0] != gboxes.shape[0]:
        raise ValueError("every annotation needs one class per ground-truth box")

    # ---- host: evaluated classes, segments (class, scene), offsets -------------------------------
    every = np.concatenate([labels, glabels])
    if every.size and every.min() >= 0 and every.max() < (1 << 20):
        classes = np.flatnonzero(np.bincount(every))
    else:
        classes = np.unique(every)
    missing = [int(l) for l in classes if int(l) not in label2cat]
    if missing:
        raise ValueError(f"labels {missing} are not in label2cat")
    C, T = len(classes), len(metric)
    pcls = np.searchsorted(classes, labels)
    gcls = np.searchsorted(classes, glabels)
    S = C * nscene
    if P >= (1 << 31) or S >= (1 << 31):
        raise ValueError("too many detections or (class, scene) pairs for 32-bit offsets")
    pseg = pcls * nscene + scene
    gseg = gcls * nscene + gscene
    pred_counts = np.bincount(pseg, minlength=S)
    gorder = np.argsort(gseg, kind="stable")
    gt_counts = np.bincount(gseg, minlength=S)
    npos = np.bincount(gcls, minlength=C)

    # ---- device: one upload per array, two sorts, match, AP -------------------------------------
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    npos_d, ws_off = up(npos.astype(np.int32)), up(_offsets(npos))
    cls_off = up(_offsets(np.bincount(pcls, minlength=C)))
    if P:
        if store is None:
            pb, sc = up(boxes), up(scores)
        pseg_d, pcls_d = up(pseg.astype(np.int32)), up(pcls.astype(np.int32))
        skey = _desc_score_key(sc)
        order_seg = torch.sort((pseg_d.to(torch.int64) << 32) | skey, stable=True).indices.to(torch.int32)
        order_cls = torch.sort((pcls_d.to(torch.int64) << 32) | skey, stable=True).indices
        tp = ops.eval_match(pb, order_seg, up(_offsets(pred_counts)), up(gboxes[gorder]), up(_offsets(gt_counts)),
                            metric, int(pred_counts.max()), int(gt_counts.max()) if S else 0)
        tp_sorted = tp[order_cls]
    else:
        tp = tp_sorted = torch.zeros((0, T), dtype=torch.uint8, device=dev)
    ap, rec = ops.eval_ap(tp_sorted, cls_off, npos_d, ws_off, int(npos.sum()))
    res = torch.stack([ap, rec]).cpu().numpy()
    out = dict(classes=[int(l) for l in classes], ap=res[0], rec=res[1])
    if with_tp:
        out["tp"] = tp.cpu().numpy()
    return out


def indoor_eval(gt_annos, dt_annos, metric=(0.25, 0.5), label2cat=None, logger=None, box_type_3d=None,
                box_mode_3d=None):
    """mmdet3d 0.18.1 ``indoor_eval`` on the GPU.

    gt_annos: upstream ``info['annos']`` dicts (``gt_num``, ``gt_boxes_upright_depth`` (n,7) gravity-centre,
    ``class`` (n,)); dt_annos: what ``DeMFVoteNet.simple_test`` returns (``boxes_3d`` depth boxes in the
    bottom-centre form, ``scores_3d``, ``labels_3d``) or the ``DetectionStore`` that ``predict_into`` filled; label2cat: label -> name, default the SUN RGB-D
    10 classes (config.SUNRGBD_CLASSES).  Boxes are depth boxes (``box_type_3d`` / ``box_mode_3d`` are taken
    for upstream's signature; the depth mode is the only one its indoor datasets use); ``logger`` is
    accepted and no table is printed.

    -> dict with ``{cat}_AP_{t:.2f}``, ``mAP_{t:.2f}``, ``{cat}_rec_{t:.2f}`` and ``mAR_{t:.2f}`` (Python floats)
    for every threshold t of ``metric``.  A label missing from ``label2cat`` raises ValueError."""
    if label2cat is None:
        label2cat = dict(enumerate(SUNRGBD_CLASSES))
    r = evaluate_detections(gt_annos, dt_annos, metric, label2cat)
    ret = {}
    for i, t in enumerate(metric):
        for c, label in enumerate(r["classes"]):
            ret[f"{label2cat[label]}_AP_{t:.2f}"] = float(r["ap"][c, i])
        ret[f"mAP_{t:.2f}"] = float(np.mean(r["ap"][:, i])) if r["classes"] else float("nan")
        for c, label in enumerate(r["classes"]):
            ret[f"{label2cat[label]}_rec_{t:.2f}"] = float(r["rec"][c, i])
        ret[f"mAR_{t:.2f}"] = float(np.mean(r["rec"][:, i])) if r["classes"] else float("nan")
    return ret
