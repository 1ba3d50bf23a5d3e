"""The trainable hot path of DeMFVoteNet: point backbone -> DeMF head -> loss.

Mirrors demf/modeling/detectors/demfnet.py:134-170 (forward_train) from line 150 on;
the frozen, no_grad image stream (demfnet.py:124-132) is outside the hot path and its
output pyramid ``img_features`` (list of 4 (B,256,H_l,W_l)) is an input here.
Attribute names (``pts_backbone``, ``pts_bbox_head``) match the reference detector so
checkpoints load with the same keys.
"""
import torch
import torch.nn as nn

from .. import ops
from ..config import DeMFCfg, VoteNetCfg, head_kwargs, votenet_head_kwargs
from .ca_head import CAVoteHead
from .head import DeMFVoteHead
from .pointnet2 import PointNet2SASSG


def _view_rows(img_metas, device):
    """View-major metas (a list over views of per-scene lists) -> the (V * B, 8) fp32 parameter rows of
    ``ops.tta_merge`` on ``device``, read back from what ``data.augment_3d`` wrote into the metas."""
    import numpy as np
    rows = []
    for metas in img_metas:
        for m in metas:
            if m.get("flip", False):
                raise ValueError("a view's image is flipped (flip=True): the views of a scene share one unflipped "
                                 "image, only the cloud is augmented")
            if m.get("pcd_vertical_flip", False):
                raise ValueError("vertically flipped views are not supported")
            rot = np.asarray(m.get("pcd_rotation", np.eye(3)), np.float64)          # rotation_z(angle).T
            t = np.asarray(m.get("pcd_trans", np.zeros(3)), np.float64)
            rows.append([1.0 if m.get("pcd_horizontal_flip", False) else 0.0, rot[0, 0], rot[0, 1],
                         float(m.get("pcd_scale_factor", 1.0)), t[0], t[1], t[2], 0.0])
    return torch.tensor(rows, dtype=torch.float32).to(device, non_blocking=True)


def _aug_views(points, img_metas):
    """Checks of the view lists -> (V, B, points as a list of (B,N,C) tensors)."""
    for var, name in ((points, "points"), (img_metas, "img_metas")):
        if not isinstance(var, (list, tuple)):
            raise TypeError("{} must be a list over views, but got {}".format(name, type(var)))
    if len(points) != len(img_metas):
        raise ValueError("num of augmentations ({}) != num of image meta ({})".format(len(points), len(img_metas)))
    if len(points) < 2:
        raise ValueError("test-time augmentation takes at least two views")
    pts = [torch.stack(p) if isinstance(p, (list, tuple)) else p for p in points]
    B = pts[0].shape[0]
    if any(p.shape[0] != B for p in pts) or any(len(m) != B for m in img_metas):
        raise ValueError("every view holds the same scenes: one (B,N,C) tensor and B metas per view")
    return len(pts), B, pts


def _aug_predict_into(head, forward_view, store, points, img_metas, tta, view_store, view_params):
    """What the two detectors' ``aug_predict_into`` share: every view's detections into ``view_store`` (view-major),
    then ``tta.merge_views`` into ``store``.  ``forward_view(v, points_v, metas_v)`` -> the head's ``bbox_preds``."""
    from ..detections import DetectionStore
    from ..tta import merge_views
    V, B, pts = _aug_views(points, img_metas)
    K, C, per_class = head.packed_shape()
    if tta is not None:
        tta.check_limits(K, C)
    if view_store is None:
        view_store = DetectionStore(V * B, device=pts[0].device)
    else:
        view_store.reset()
    rows = _view_rows(img_metas, "cpu")                                   # (also the metas' checks)
    rows = view_params if view_params is not None else rows.to(pts[0].device, non_blocking=True)
    for v in range(V):
        head.get_bboxes_packed(pts[v], forward_view(v, pts[v], img_metas[v]), img_metas[v], view_store)
    merge_views(view_store, rows, store, 0, B, head, tta)
    return view_store


class DeMFHotPath(nn.Module):
    def __init__(self, cfg: DeMFCfg = None):
        super().__init__()
        self.cfg = cfg or DeMFCfg()
        b = self.cfg.backbone
        self.pts_backbone = PointNet2SASSG(
            in_channels=b.in_channels, num_points=b.num_points, radius=b.radius,
            num_samples=b.num_samples, sa_channels=b.sa_channels, fp_channels=b.fp_channels,
            use_xyz=b.use_xyz, normalize_xyz=b.normalize_xyz)
        self.pts_bbox_head = DeMFVoteHead(**head_kwargs(self.cfg))
        for layer in self.pts_bbox_head.decoder:
            layer.init_weights()

    def extract_pts_feat(self, points, geometry=None):
        """ImVoteNet.extract_pts_feat as reached from demfnet.py:151-152."""
        x = self.pts_backbone(points, geometry)
        return x["fp_xyz"][-1], x["fp_features"][-1], x["fp_indices"][-1]

    @torch.no_grad()
    def index_geometry(self, points):
        """Coordinate-only pre-pass of the step: the backbone's FPS / ball-query / 3-NN indices and
        the head's seed FPS (class_agnostic_vote_head.py:429-430; seeds are input points)."""
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        geo = self.pts_backbone.index_geometry(points)
        bb = self.pts_backbone
        seed_xyz = ([points[..., :3]] + [t[1] for t in geo["sa"]])[bb.num_sa - bb.num_fp]
        if self.cfg.head.sample_mod == "seed":
            geo["sample_indices"] = ops.furthest_point_sample(seed_xyz.contiguous(),
                                                              self.pts_bbox_head.num_proposal)
        return geo

    def forward_head(self, points, img_features, img_metas, image_inputs=None, geometry=None):
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)                                    # demfnet.py:150
        seeds_3d, seed_3d_features, seed_indices = self.extract_pts_feat(points, geometry)
        feat_dict = dict(seed_points=seeds_3d, seed_features=seed_3d_features,
                         seed_indices=seed_indices,
                         sample_indices=None if geometry is None else geometry.get("sample_indices"))
        img_dict = dict(img_features=img_features, img_metas=img_metas, image_inputs=image_inputs)
        return self.pts_bbox_head(feat_dict, self.cfg.head.sample_mod, img_dict)  # :165

    def forward_train(self, points, img_features, img_metas, gt_bboxes_3d, gt_labels_3d,
                      geometry=None):
        """-> dict of losses (demfnet.py:134-170 with the image pyramid precomputed).
        ``geometry``: the coordinate-only pre-pass (``index_geometry``) when it was computed ahead
        of the step (engine.Trainer pipelines it under the previous step's backward)."""
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        bbox_preds = self.forward_head(points, img_features, img_metas, geometry=geometry)
        return self.pts_bbox_head.loss(bbox_preds, points, gt_bboxes_3d, gt_labels_3d, None, None,
                                       img_metas)                            # :167

    def param_groups(self, lr=0.008, weight_decay=0.01):
        """AdamW groups of demf_votenet.py:16-24: 'decoder' params at lr*0.05."""
        dec, rest = [], []
        for n, p in self.named_parameters():
            if p.requires_grad:
                (dec if "decoder" in n else rest).append(p)
        return [dict(params=rest, lr=lr, weight_decay=weight_decay),
                dict(params=dec, lr=lr * 0.05, weight_decay=weight_decay)]


class DeMFVoteNet(DeMFHotPath):
    """The whole detector with the reference's entry points
    (demf/modeling/detectors/demfnet.py:12-283): the trainable hot path above plus the frozen
    image stream under the reference's attribute names (``img_backbone``, ``img_neck``,
    ``img_encoder``), so a released checkpoint - or a stage-1 image checkpoint through the key
    remap of :85-101 - loads with ``load_state_dict``.

      forward_train(points, img, img_metas, gt_bboxes_3d, gt_labels_3d) -> dict of losses  (:134-170)
      simple_test(points, img_metas, img) -> list of dict(boxes_3d, scores_3d, labels_3d)  (:254-283)
      predict_into(store, points, img_metas, img): the same detections appended to a device-resident store
      forward_test(points, img_metas, img)  (:172-238; lists over augmentations: one -> simple_test, more -> aug_test)
      aug_test(points, img_metas, img) / aug_predict_into(store, ...): test-time augmentation, which :236-238
          dispatches to and the reference cannot run - the image stream once, the head per view, merged by tta.py
    """

    def __init__(self, cfg: DeMFCfg = None, image_stream=None, **image_stream_kwargs):
        super().__init__(cfg)
        from .image_stream import ImageStream
        stream = image_stream if image_stream is not None else ImageStream(**image_stream_kwargs)
        self.img_backbone, self.img_neck = stream.img_backbone, stream.img_neck
        self.img_encoder = stream.img_encoder
        self.freeze_img_branch_params()

    def freeze_img_branch_params(self):                                     # :103-112
        for m in (self.img_backbone, self.img_neck, self.img_encoder):
            for p in m.parameters():
                p.requires_grad_(False)

    def train(self, mode=True):                                              # :114-122
        super().train(mode)
        for m in (self.img_backbone, self.img_neck, self.img_encoder):
            m.eval()
        return self

    def load_state_dict(self, state_dict, strict=True, **kw):
        """+ the stage-1 key remap of ``_load_from_state_dict`` (:85-101)."""
        from ..data import remap_checkpoint
        return super().load_state_dict(remap_checkpoint(state_dict), strict=strict, **kw)

    @torch.no_grad()
    def extract_img_feat(self, img, img_metas):                             # :124-132
        """-> the channels-last token form of the 4-level pyramid (dict(tokens (B,S,C), spatial,
        ...)): what this package's head consumes without the flatten copy (:570-591).
        ``self.img_encoder(feats, img_metas)`` gives the reference's list of NCHW maps."""
        return self.img_encoder.forward_tokens(self.img_neck(self.img_backbone(img)), img_metas)

    def forward_train(self, points=None, img=None, img_metas=None, gt_bboxes_3d=None,
                      gt_labels_3d=None, **unused):
        img_features = self.extract_img_feat(img, img_metas)               # :148
        return super().forward_train(points, img_features, img_metas, gt_bboxes_3d, gt_labels_3d)

    @torch.no_grad()
    def simple_test(self, points=None, img_metas=None, img=None, bboxes_2d=None, rescale=False,
                    **unused):
        img_features = self.extract_img_feat(img, img_metas)               # :260
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)                                    # :262
        bbox_preds = self.forward_head(points, img_features, img_metas)    # :263-275
        # :278-282 (get_bboxes + bbox3d2result): the batch's store, brought to the host in one go
        return self.pts_bbox_head.get_bboxes_packed(points, bbox_preds, img_metas).results()

    @torch.no_grad()
    def predict_into(self, store, points=None, img_metas=None, img=None, **unused):
        """``simple_test`` whose detections stay on the device: the batch's scenes are appended to ``store``
        (detections.DetectionStore) and nothing is returned; the post-processing does not synchronise."""
        img_features = self.extract_img_feat(img, img_metas)
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        bbox_preds = self.forward_head(points, img_features, img_metas)
        self.pts_bbox_head.get_bboxes_packed(points, bbox_preds, img_metas, store)

    @torch.no_grad()
    def aug_predict_into(self, store, points=None, img_metas=None, img=None, tta=None, view_store=None,
                         view_params=None, **unused):
        """Test-time augmentation with the detections on the device (tta.py): ``points`` is a list over views of
        (B,N,C) clouds, ``img_metas`` a list over views of the scenes' metas (``data.augment_3d``'s, which name
        each view's flip / rotation / scale / translation), ``img`` ONE tensor - or a list whose entries are that
        tensor: the views share the unaugmented image, so the frozen image stream runs once.  The head runs per
        view into ``view_store`` (a ``DetectionStore`` of V * B scenes, view-major: made here when not given, else
        reset; pass one to inspect the views or to reuse its arrays) and ``tta.merge_views`` appends the B merged
        scenes to ``store``.  ``tta``: a ``tta.TTACfg`` (threshold, mode, ``max_num``; None: the defaults);
        ``view_params``: the (V * B, 8) device array of parameter rows when the loader made it already.  No host
        sync (without ``view_params`` one small upload).  -> the view store."""
        if isinstance(img, (list, tuple)):
            if not img:
                raise ValueError("img is an empty list")
            for other in img[1:]:
                if other is not img[0] and other.shape != img[0].shape:
                    raise ValueError("the views of a scene share one image: every entry of img must be the same "
                                     "tensor (or a copy of it, of the same shape); the first one is used")
            img = img[0]
        _aug_views(points, img_metas)
        _view_rows(img_metas, "cpu")                                        # (a flipped image is refused first)
        for metas in img_metas:                                             # :180-183
            for m in metas:
                m["batch_input_shape"] = tuple(img.shape[-2:])
        img_features = self.extract_img_feat(img, img_metas[0])
        return _aug_predict_into(self.pts_bbox_head,
                                 lambda v, p, metas: self.forward_head(p, img_features, metas),
                                 store, points, img_metas, tta, view_store, view_params)

    @torch.no_grad()
    def aug_test(self, points=None, img_metas=None, img=None, tta=None, **unused):
        """What the reference's ``forward_test`` dispatches ``num_augs > 1`` to (:236-238) and cannot run: the
        merged detections of the views -> list of dict(boxes_3d, scores_3d, labels_3d), one per scene."""
        from ..detections import DetectionStore
        store = DetectionStore(max(len(img_metas[0]), 1) if img_metas else 1, device=self._device())
        self.aug_predict_into(store, points, img_metas, img, tta=tta)
        return store.results()

    def _device(self):
        return next(self.parameters()).device

    def forward_test(self, points=None, img_metas=None, img=None, bboxes_2d=None, **kwargs):
        """:172-238: ``points`` / ``img_metas`` / ``img`` are lists over augmentations; one augmentation is
        ``simple_test``, more go to ``aug_test``."""
        for var, name in ((points, "points"), (img_metas, "img_metas")):
            if not isinstance(var, list):
                raise TypeError("{} must be a list, but got {}".format(name, type(var)))
        if len(points) != len(img_metas):
            raise ValueError("num of augmentations ({}) != num of image meta ({})".format(
                len(points), len(img_metas)))
        if len(points) != 1:                                                # :236-238
            kwargs.pop("rescale", None)
            return self.aug_test(points, img_metas, img, **kwargs)
        for _img, metas in zip(img, img_metas):                             # :180-183
            for m in metas:
                m["batch_input_shape"] = tuple(_img.shape[-2:])
        return self.simple_test(points[0], img_metas[0], img[0],
                                bboxes_2d=bboxes_2d[0] if bboxes_2d is not None else None, **kwargs)


class VoteNet(nn.Module):
    """The points-only class-agnostic VoteNet baseline of configs/baseline/votenet.py ("VoteNet*" in the
    reference's results): PointNet2SASSG -> CAVoteHead, no image.  Entry points and attribute names
    (``backbone``, ``bbox_head``) are those of mmdet3d's VoteNet detector ([dep-recall]: that class is not in
    the reference tree), so its checkpoints load with the same keys.

      forward_train(points, img_metas, gt_bboxes_3d, gt_labels_3d) -> dict of losses
      simple_test(points, img_metas) -> list of dict(boxes_3d, scores_3d, labels_3d)
      predict_into(store, points, img_metas): the same detections appended to a device-resident store
      forward_test(points, img_metas)  (lists over augmentations: one -> simple_test, more -> aug_test)
      aug_test(points, img_metas) / aug_predict_into(store, ...): test-time augmentation (tta.py)
    """

    def __init__(self, cfg: VoteNetCfg = None):
        super().__init__()
        self.cfg = cfg or VoteNetCfg()
        b = self.cfg.backbone
        self.backbone = PointNet2SASSG(
            in_channels=b.in_channels, num_points=b.num_points, radius=b.radius,
            num_samples=b.num_samples, sa_channels=b.sa_channels, fp_channels=b.fp_channels,
            use_xyz=b.use_xyz, normalize_xyz=b.normalize_xyz)
        self.bbox_head = CAVoteHead(**votenet_head_kwargs(self.cfg))

    def _sample_mod(self):
        h = self.cfg.head
        return h.train_sample_mod if self.training else h.test_sample_mod

    @torch.no_grad()
    def index_geometry(self, points):
        """Coordinate-only pre-pass of the step, as DeMFHotPath.index_geometry."""
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        geo = self.backbone.index_geometry(points)
        bb = self.backbone
        seed_xyz = ([points[..., :3]] + [t[1] for t in geo["sa"]])[bb.num_sa - bb.num_fp]
        if self._sample_mod() == "seed":
            geo["sample_indices"] = ops.furthest_point_sample(seed_xyz.contiguous(), self.bbox_head.num_proposal)
        return geo

    def forward_head(self, points, geometry=None):
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        x = self.backbone(points, geometry)
        feat_dict = dict(seed_points=x["fp_xyz"][-1], seed_features=x["fp_features"][-1],
                         seed_indices=x["fp_indices"][-1],
                         sample_indices=None if geometry is None else geometry.get("sample_indices"))
        return self.bbox_head(feat_dict, self._sample_mod())

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, geometry=None,
                      **unused):
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        bbox_preds = self.forward_head(points, geometry)
        return self.bbox_head.loss(bbox_preds, points, gt_bboxes_3d, gt_labels_3d, None, None, img_metas)

    def param_groups(self, lr=0.008, weight_decay=0.01):
        """One AdamW group (configs/_base_/schedules/schedule_3x.py:6): the baseline has no decoder group."""
        return [dict(params=[p for p in self.parameters() if p.requires_grad], lr=lr, weight_decay=weight_decay)]

    @torch.no_grad()
    def simple_test(self, points=None, img_metas=None, rescale=False, **unused):
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        bbox_preds = self.forward_head(points)
        return self.bbox_head.get_bboxes_packed(points, bbox_preds, img_metas).results()

    @torch.no_grad()
    def predict_into(self, store, points=None, img_metas=None, **unused):
        """``simple_test`` whose detections stay on the device (detections.DetectionStore); no host sync."""
        if isinstance(points, (list, tuple)):
            points = torch.stack(points)
        bbox_preds = self.forward_head(points)
        self.bbox_head.get_bboxes_packed(points, bbox_preds, img_metas, store)

    @torch.no_grad()
    def aug_predict_into(self, store, points=None, img_metas=None, tta=None, view_store=None, view_params=None,
                         **unused):
        """``DeMFVoteNet.aug_predict_into`` without the image: lists over views of clouds and metas -> the merged
        scenes appended to ``store``; no host sync.  -> the view store."""
        return _aug_predict_into(self.bbox_head, lambda v, p, metas: self.forward_head(p), store, points,
                                 img_metas, tta, view_store, view_params)

    @torch.no_grad()
    def aug_test(self, points=None, img_metas=None, tta=None, **unused):
        """The merged detections of the views -> list of dict(boxes_3d, scores_3d, labels_3d), one per scene."""
        from ..detections import DetectionStore
        store = DetectionStore(max(len(img_metas[0]), 1) if img_metas else 1,
                               device=next(self.parameters()).device)
        self.aug_predict_into(store, points, img_metas, tta=tta)
        return store.results()

    def forward_test(self, points=None, img_metas=None, **kwargs):
        for var, name in ((points, "points"), (img_metas, "img_metas")):
            if not isinstance(var, list):
                raise TypeError("{} must be a list, but got {}".format(name, type(var)))
        if len(points) != len(img_metas):
            raise ValueError("num of augmentations ({}) != num of image meta ({})".format(
                len(points), len(img_metas)))
        kwargs.pop("img", None)
        if len(points) != 1:
            kwargs.pop("rescale", None)
            return self.aug_test(points, img_metas, **kwargs)
        return self.simple_test(points[0], img_metas[0], **kwargs)


def bbox3d2result(bboxes, scores, labels):
    """mmdet3d.core.bbox3d2result: results to host memory."""
    return dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())
