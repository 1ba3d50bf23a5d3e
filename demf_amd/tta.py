"""Test-time augmentation: several views of a scene, merged on the device.

The reference's ``forward_test`` hands ``num_augs > 1`` to ``self.aug_test`` (demf/modeling/detectors/demfnet.py:
236-238), a method it inherits from a class whose members (``pts_bbox_head_joint``, ``fusion_layer``) it does not
have: multi-view testing is advertised and cannot run.  What mmdet3d 0.18.1 means by it [dep-recall]:

  MultiScaleFlipAug3D(pts_scale_ratio=[s0, s1, ...], flip=True, pcd_horizontal_flip=True): the views are scale-major,
      for each scale the unflipped view and then the flipped one; inside a view GlobalRotScaleTrans(rot 0, scale s,
      no translation), RandomFlip3D with the flag forced, PointSample drawn anew.  Flip and scale commute for these
      views, so ``data.augment_3d``'s flow order (HF, R, S, T) applies them.
  merge_aug_bboxes_3d: bbox3d_mapping_back per view, concatenation, a per-class NMS over the rows of all views
      (``nms_gpu`` on rotated footprints or ``nms_normal_gpu`` on axis-aligned ones), the kept rows sorted by score
      and cut at ``max_num``.

Here the views' detections lie view-major in one ``DetectionStore`` (scene ``v * B + b`` = view v of batch scene b)
and ``merge_views`` appends the merged scenes to another one through ``ops.tta_merge`` (csrc/tta.hip): three
launches, no host sync.  The image is never augmented (RandomFlip3D(sync_2d=False), image flip_ratio 0), so
``DeMFVoteNet.aug_predict_into`` runs the frozen image stream once per scene, not once per view.

Deviations from upstream, on purpose: the footprints are the package's own
(``geometry.rotation_3d_in_axis_z`` / ``ops.box3d_overlaps``); ties are ordered (score descending, then class, view,
row ascending; inside the NMS the lower (view, row) first); ``max_num`` defaults to the single-view worst case
(``K * C`` with ``per_class_proposal``, else ``K``) so that a store sized for single-view testing holds a merged
scene; ``nms_thr`` defaults to ``test_cfg["nms_thr"]``; the mapping back inverts the whole parameter row (flip, angle,
scale, translation); a third overlap mode, the rotated 3-D IoU, stands next to upstream's two.  No accuracy figure
has been measured with it: the mechanism is verified, not a mAP gain.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import ops
from .pipeline import identity_aug_params, param_row


@dataclass(frozen=True)
class TTACfg:
    """The views of a scene and how they are merged.  ``scales``: pts_scale_ratio; ``flip``: add the horizontally
    flipped view of every scale; ``nms_thr`` (None: ``test_cfg["nms_thr"]``); ``mode``: "bev" rotated BEV IoU
    (upstream's default), "aligned" axis-aligned BEV IoU, "3d" rotated 3-D IoU; ``max_num`` (None: the single-view
    worst case)."""
    scales: Tuple[float, ...] = (1.0,)
    flip: bool = True
    nms_thr: Optional[float] = None
    mode: str = "bev"
    max_num: Optional[int] = None

    def __post_init__(self):
        scales = tuple(float(s) for s in self.scales)
        object.__setattr__(self, "scales", scales)
        object.__setattr__(self, "flip", bool(self.flip))
        if not scales or any(not (s > 0.0) or not np.isfinite(s) for s in scales):
            raise ValueError(f"scales must be positive numbers, got {self.scales!r}")
        if self.num_views < 2:
            raise ValueError("test-time augmentation needs at least two views: more than one scale, or flip=True")
        if self.mode not in ops.NMS_MODES:
            raise ValueError(f"mode must be one of {sorted(ops.NMS_MODES)}, got {self.mode!r}")
        if self.nms_thr is not None and not (0.0 <= float(self.nms_thr) <= 1.0):
            raise ValueError(f"nms_thr must lie in [0, 1], got {self.nms_thr!r}")
        if self.max_num is not None and int(self.max_num) < 1:
            raise ValueError(f"max_num must be positive, got {self.max_num!r}")

    @property
    def num_views(self):
        return len(self.scales) * (2 if self.flip else 1)

    def check_limits(self, K, C):
        """Raise unless V views of at most ``K`` rows per class and ``C`` classes fit the merge kernels."""
        V = self.num_views
        if V * K > ops.NMS_MAX_SEGMENT or V * K * C > ops.TTA_MAX_CANDIDATES:
            raise ValueError(f"{V} views of K = {K} proposals and C = {C} classes: the merge takes V * K <= "
                             f"{ops.NMS_MAX_SEGMENT} and V * K * C <= {ops.TTA_MAX_CANDIDATES}")


def view_params(cfg):
    """-> the parameter dicts (``pipeline.draw_aug_params``'s form) of the views in view order: scale-major, the
    unflipped view before the flipped one.  A first scale of 1.0 makes view 0 ``identity_aug_params()``."""
    out = []
    for s in cfg.scales:
        for flip in ((False, True) if cfg.flip else (False,)):
            p = identity_aug_params()
            p["scale"], p["flip"] = float(s), flip
            out.append(p)
    return out


def param_rows(params, B):
    """View parameter dicts -> the (V * B, 8) fp32 rows of ``demf_points_prep`` / ``ops.tta_merge``, view-major."""
    return np.repeat(np.stack([param_row(p) for p in params]), int(B), axis=0)


def default_max_num(head):
    K, C, per_class = head.packed_shape()
    return K * C if per_class else K


def merge_views(view_store, params, out_store, first_view_scene, B, head, tta=None):
    """Merge the ``V * B`` view scenes of ``view_store`` from ``first_view_scene`` on (view-major) into ``B`` scenes
    appended to ``out_store``.  ``params``: the (V * B, 8) fp32 device array of parameter rows; ``head``: the vote
    head that wrote the views (its ``test_cfg`` gives ``nms_thr`` and ``per_class_proposal``); ``tta``: a ``TTACfg``
    for threshold, mode and ``max_num`` (None: the defaults).  No host sync.  -> out_store."""
    B = int(B)
    V = params.shape[0] // max(B, 1) if B else 0
    if B < 1 or V * B != params.shape[0] or V < 1:
        raise ValueError(f"params holds {params.shape[0]} rows, not a multiple of B = {B} scenes")
    if first_view_scene < 0 or first_view_scene + V * B > len(view_store):
        raise ValueError(f"the view store holds {len(view_store)} scenes: {V} views of {B} scenes from scene "
                         f"{first_view_scene} are not there")
    K, C, per_class = head.packed_shape()
    thr = head.test_cfg["nms_thr"] if tta is None or tta.nms_thr is None else tta.nms_thr
    mode = "bev" if tta is None else tta.mode
    max_num = (K * C if per_class else K) if tta is None or tta.max_num is None else int(tta.max_num)
    if V * K > ops.NMS_MAX_SEGMENT or V * K * C > ops.TTA_MAX_CANDIDATES:
        raise ValueError(f"{V} views of K = {K} proposals and C = {C} classes: the merge takes V * K <= "
                         f"{ops.NMS_MAX_SEGMENT} and V * K * C <= {ops.TTA_MAX_CANDIDATES}")
    first = out_store.reserve(B, max_num)
    ops.tta_merge(view_store.boxes, view_store.scores, view_store.labels, view_store.scene_off, view_store.state,
                  params, first_view_scene, B, V, C, K, thr, mode, max_num, first, out_store.boxes, out_store.scores,
                  out_store.labels, out_store.scene_off, out_store.state)
    return out_store
