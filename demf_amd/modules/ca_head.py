"""CAVoteHead - the head of the points-only class-agnostic VoteNet baseline - on the gfx950 operators.

Mirrors demf/modeling/heads/class_agnostic_vote_head.py:24-334 (CAVoteHead, a subclass of mmdet3d's VoteHead
[dep-recall]) as configs/_base_/models/votenet.py:18-65 + configs/baseline/votenet.py:6-39 build it: vote module,
one vote aggregation [256, 128, 128, 128], ONE prediction head ``conv_pred`` on 128 channels, no decoder and no
image.  The head regresses the log of the six distances from the proposal to the box faces
(ClassAgnosticBBoxCoder); everything else - targets, NMS, packing - is shared with DeMFVoteHead (VoteHeadBase).
State-dict names follow VoteHead: ``vote_module.*``, ``vote_aggregation.*``, ``conv_pred.*``.
"""
import torch
import torch.nn.functional as F

from .. import ops
from . import losses as L
from .coder import ClassAgnosticBBoxCoder
from .head import VoteHeadBase
from .pointnet2 import build_sa_module
from .vote import BaseConvBboxHead, VoteModule


class CAVoteHead(VoteHeadBase):
    # the loss terms this head has, in the order of the fused kernel's slots: no centre loss (:99-116)
    LOSS_NAMES = tuple(n for n in ops.HEAD_LOSS_NAMES if n != "center_loss")
    TARGET_NAMES = ("vote_targets", "vote_target_masks", "dir_class_targets", "dir_res_targets", "mask_targets",
                    "objectness_targets", "objectness_weights", "box_loss_weights", "distance_targets",
                    "centerness_targets", "dir_targets")                                       # :179-182

    def __init__(self, num_classes, bbox_coder, train_cfg=None, test_cfg=None, vote_module_cfg=None,
                 vote_aggregation_cfg=None, pred_layer_cfg=None, conv_cfg=None, norm_cfg=None,
                 objectness_loss=None, center_loss=None, dir_class_loss=None, dir_res_loss=None,
                 size_class_loss=None, size_res_loss=None, semantic_loss=None, iou_loss=None, init_cfg=None):
        super().__init__()
        self.num_classes = num_classes
        self.train_cfg, self.test_cfg = train_cfg or {}, test_cfg or {}
        self.gt_per_seed = vote_module_cfg["gt_per_seed"]
        self.num_proposal = vote_aggregation_cfg["num_point"]
        # (center_loss / size_class_loss are VoteHead kwargs the class-agnostic loss never evaluates)
        self.loss_cfg = dict(objectness=objectness_loss or {}, dir_class=dir_class_loss or {},
                             dir_res=dir_res_loss or {}, size_res=size_res_loss or {}, semantic=semantic_loss,
                             iou=iou_loss)
        bc = dict(bbox_coder)
        bc.pop("type", None)
        self.bbox_coder = ClassAgnosticBBoxCoder(**bc)
        self.num_dir_bins = self.bbox_coder.num_dir_bins
        vm = dict(vote_module_cfg)
        vl = vm.pop("vote_loss", {}) or {}
        self.vote_module = VoteModule(**vm, vote_loss_dst_weight=vl.get("loss_dst_weight", 1.0))
        self.vote_aggregation = build_sa_module(vote_aggregation_cfg)
        self.fp16_enabled = False
        ncls = num_classes + 2 if semantic_loss is not None else 2                             # :29-33
        nreg = 6 + self.num_dir_bins * 2                                                       # :35-37
        self.conv_pred = BaseConvBboxHead(**pred_layer_cfg, num_cls_out_channels=ncls,
                                          num_reg_out_channels=nreg)

    # ---- VoteHead.forward [dep-recall] ------------------------------------------------------------
    def forward(self, feat_dict, sample_mod):
        assert sample_mod in ["vote", "seed", "random", "spec"]
        if "seed_points" in feat_dict:
            seed_points, seed_features = feat_dict["seed_points"], feat_dict["seed_features"]
            seed_indices = feat_dict["seed_indices"]
        else:                                            # VoteHead._extract_input: the backbone's dict
            seed_points, seed_features = feat_dict["fp_xyz"][-1], feat_dict["fp_features"][-1]
            seed_indices = feat_dict["fp_indices"][-1]
        vote_points, vote_features, vote_offset = self.vote_module(seed_points, seed_features)
        if sample_mod == "vote":
            agg_in = dict(points_xyz=vote_points, features=vote_features)
        elif sample_mod == "seed":
            sample_indices = feat_dict.get("sample_indices")   # coordinate-only: may be prefetched
            if sample_indices is None:
                sample_indices = ops.furthest_point_sample(seed_points, self.num_proposal)
            agg_in = dict(points_xyz=vote_points, features=vote_features, indices=sample_indices)
        elif sample_mod == "random":
            B, num_seed = seed_points.shape[:2]
            sample_indices = torch.randint(0, num_seed, (B, self.num_proposal), dtype=torch.int32,
                                           device=seed_points.device)
            agg_in = dict(points_xyz=vote_points, features=vote_features, indices=sample_indices)
        else:  # 'spec'
            agg_in = dict(points_xyz=seed_points, features=seed_features, target_xyz=vote_points)
        aggregated_points, features, aggregated_indices = self.vote_aggregation(**agg_in)
        cls_p, reg_p = self.conv_pred(features)
        # split_pred's dict IS the result (VoteHead: results.update(decode_res)); built this way round the lazy
        # entries ("distance", "dir_res") stay unmaterialised
        results = self.bbox_coder.split_pred(cls_p, reg_p, aggregated_points)
        dict.update(results, seed_points=seed_points, seed_indices=seed_indices, vote_points=vote_points,
                    vote_features=vote_features, vote_offset=vote_offset, aggregated_points=aggregated_points,
                    aggregated_indices=aggregated_indices)
        # the raw conv rows ((B, Q, 12) / (B, Q, 30): the point-major storage behind cls_p / reg_p) for the
        # fused loss and decode kernels
        dict.__setitem__(results, "_rows", (cls_p.transpose(1, 2), reg_p.transpose(1, 2)))
        return results

    # ---- loss: :40-121 ------------------------------------------------------------------------------
    def _hyper(self):
        c = self.loss_cfg
        cw = c["objectness"].get("class_weight") or [1.0, 1.0]
        sem_w = c["semantic"].get("loss_weight", 1.0) if c["semantic"] is not None else 0.0
        iou_w = c["iou"].get("loss_weight", 1.0) if c["iou"] else 0.0
        # the twelve numbers of ops.head_loss; the centre weight and beta (slots 6 and 11) do not exist here
        return (cw[0], cw[1], c["objectness"].get("loss_weight", 1.0), c["dir_class"].get("loss_weight", 1.0),
                c["dir_res"].get("loss_weight", 1.0), c["size_res"].get("loss_weight", 1.0), 0.0, sem_w, iou_w,
                c["dir_res"].get("beta", 1.0), c["size_res"].get("beta", 1.0), 1.0)

    def _fusable(self, bbox_preds):
        rows = bbox_preds.get("_rows") if isinstance(bbox_preds, dict) else None
        c = self.loss_cfg
        return rows is not None and rows[0].is_cuda and rows[0].shape[-1] == 12 and rows[1].shape[-1] == 30 and \
            c["semantic"] is not None and bool(c["iou"])

    def loss(self, bbox_preds, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None,
             pts_instance_mask=None, img_metas=None, gt_bboxes_ignore=None, ret_target=False, vote_pack=None):
        """-> dict: ``vote_loss`` + LOSS_NAMES (+ ``_total``, their sum, on the fused path: what a training loop
        differentiates)."""
        targets = self._targets(points, gt_bboxes_3d, gt_labels_3d, bbox_preds, vote_pack)
        if self._fusable(bbox_preds):
            losses = self._loss_fused(bbox_preds, targets)
        else:
            losses = self._loss(bbox_preds, targets)
        if ret_target:
            losses["targets"] = self._reference_targets(targets)
        return losses

    def _loss(self, bbox_preds, targets):
        """The torch restatement of :57-116: the readable specification of csrc/loss.hip's distance form (and
        what runs without a GPU)."""
        (vote_targets, vote_target_masks, dir_class_targets, dir_res_targets, mask_targets, objectness_targets,
         objectness_weights, box_loss_weights, _, dir_targets, size_targets, center_targets) = targets
        # The reference builds the distance targets from the aggregated points WITHOUT detaching them (:271-294),
        # so the SmoothL1 and IoU terms send a gradient to the points through their targets: rebuilt here with it
        distance_targets = self._distance_targets(bbox_preds["ref_points"], center_targets, size_targets,
                                                  dir_targets).clamp(min=0)                     # :301
        c = self.loss_cfg
        vote_loss = self.vote_module.get_loss(bbox_preds["seed_points"], bbox_preds["vote_points"],
                                              bbox_preds["seed_indices"], vote_target_masks, vote_targets)
        ocw = c["objectness"].get("class_weight")
        if ocw is not None:
            ocw = torch.tensor(ocw, dtype=bbox_preds["obj_scores"].dtype, device=bbox_preds["obj_scores"].device)
        objectness_loss = L.cross_entropy_sum(bbox_preds["obj_scores"].transpose(2, 1), objectness_targets,
                                              objectness_weights, ocw, c["objectness"].get("loss_weight", 1.0))
        size_res_loss = L.smooth_l1_sum(bbox_preds["distance"], distance_targets,
                                        box_loss_weights.unsqueeze(-1).repeat(1, 1, 6),
                                        c["size_res"].get("beta", 1.0), c["size_res"].get("loss_weight", 1.0))
        dir_class_loss = L.cross_entropy_sum(bbox_preds["dir_class"].transpose(2, 1), dir_class_targets,
                                             box_loss_weights, None, c["dir_class"].get("loss_weight", 1.0))
        one_hot = F.one_hot(dir_class_targets, self.num_dir_bins).to(vote_targets.dtype)
        dir_res_norm = torch.sum(bbox_preds["dir_res_norm"] * one_hot, -1)
        dir_res_loss = L.smooth_l1_sum(dir_res_norm, dir_res_targets, box_loss_weights,
                                       c["dir_res"].get("beta", 1.0), c["dir_res"].get("loss_weight", 1.0))
        losses = dict(vote_loss=vote_loss, objectness_loss=objectness_loss, dir_class_loss=dir_class_loss,
                      dir_res_loss=dir_res_loss, size_res_loss=size_res_loss)
        if c["semantic"] is not None:
            losses["semantic_loss"] = L.cross_entropy_sum(
                bbox_preds["sem_scores"].transpose(2, 1), mask_targets, box_loss_weights, None,
                c["semantic"].get("loss_weight", 1.0))
        if c["iou"]:
            corners_pred = self.bbox_coder.decode_corners(bbox_preds["distance"], bbox_preds["ref_points"])
            corners_target = self.bbox_coder.decode_corners(distance_targets, bbox_preds["ref_points"])
            losses["iou_loss"] = L.axis_aligned_iou_loss_sum(corners_pred, corners_target, box_loss_weights,
                                                             c["iou"].get("loss_weight", 1.0))
        return losses

    def _distance_targets(self, points, center_targets, size_targets, dir_targets):
        """:271-294: the distances from ``points`` (B,Q,3) to the faces of the assigned boxes, in the boxes' frames
        (unclamped; what demf_proposal_targets writes), differentiable in ``points``."""
        from ..geometry import rotation_3d_in_axis_z
        canonical = points - center_targets
        if self.bbox_coder.with_rot:
            n = canonical.shape[0] * canonical.shape[1]
            canonical = rotation_3d_in_axis_z(canonical.reshape(n, 1, 3), -dir_targets.reshape(n)).reshape(points.shape)
        half = size_targets / 2.0
        return torch.cat([half - canonical, half + canonical], dim=-1)

    def _loss_fused(self, bbox_preds, targets):
        """The same through csrc/loss.hip: one kernel each way for the six per-proposal reductions
        (ops.ca_head_loss), one for the vote loss, one for the total."""
        (vote_targets, vote_target_masks, dir_class_targets, dir_res_targets, mask_targets, objectness_targets,
         objectness_weights, box_loss_weights, distance_targets, dir_targets, _, _) = targets
        cls_rows, reg_rows = bbox_preds["_rows"]
        R = cls_rows.shape[0] * cls_rows.shape[1]
        seven = ops.ca_head_loss(
            cls_rows.reshape(R, 12), reg_rows.reshape(R, 30), self._hyper(),
            distance_targets.reshape(R, 6).contiguous(), dir_class_targets.reshape(R),
            dir_res_targets.reshape(R).contiguous(), mask_targets.reshape(R), objectness_targets.reshape(R),
            objectness_weights.reshape(R).contiguous(), box_loss_weights.reshape(R).contiguous(),
            ref_points=bbox_preds["ref_points"].reshape(R, 3).contiguous(),
            dir_t=dir_targets.reshape(R).contiguous() if self.bbox_coder.with_rot else None)
        vote = ops.vote_loss(bbox_preds["vote_points"], bbox_preds["seed_points"], bbox_preds["seed_indices"],
                             vote_target_masks, vote_targets, self.gt_per_seed,
                             self.vote_module.vote_loss_dst_weight)
        out8 = ops.loss_total([seven], vote)                 # one vector: the mean is the vector itself
        losses = dict(vote_loss=vote)
        for i, name in enumerate(ops.HEAD_LOSS_NAMES):
            if name in self.LOSS_NAMES:                      # (slot 4, the centre loss, is an exact 0)
                losses[name] = out8[i]
        losses["_total"] = out8[7]
        return losses

    # ---- targets: :123-316 --------------------------------------------------------------------------
    @torch.no_grad()
    def _targets(self, points, gt_bboxes_3d, gt_labels_3d, bbox_preds, vote_pack=None):
        """The shared batched target generation (VoteHeadBase.get_targets).  Its distance targets are those of
        :279-294: the baseline coder encodes dims / 2 and uses it as it is (:21, :265), the DeMF coder encodes
        dims and the DeMF head halves it (:913-919) - the same six numbers, which demf_proposal_targets computes
        from dims / 2 for both."""
        return VoteHeadBase.get_targets(self, points, gt_bboxes_3d, gt_labels_3d, bbox_preds, vote_pack)

    @staticmethod
    def _reference_targets(targets):
        (vote_targets, vote_target_masks, dir_class_targets, dir_res_targets, mask_targets, objectness_targets,
         objectness_weights, box_loss_weights, distance_targets, dir_targets, _, _) = targets
        distance_targets = distance_targets.clamp(min=0)                                        # :301
        lo = torch.minimum(distance_targets[..., 0:3], distance_targets[..., 3:6])              # :302-309
        hi = torch.maximum(distance_targets[..., 0:3], distance_targets[..., 3:6])
        centerness = (lo.prod(dim=-1) / (hi.prod(dim=-1) + 1e-6) + 1e-6) ** (1 / 3)
        centerness = torch.clamp(centerness, min=0, max=1)
        return (vote_targets, vote_target_masks, dir_class_targets, dir_res_targets, mask_targets,
                objectness_targets, objectness_weights, box_loss_weights, distance_targets, centerness,
                dir_targets)

    @torch.no_grad()
    def get_targets(self, points, gt_bboxes_3d, gt_labels_3d, pts_semantic_mask=None, pts_instance_mask=None,
                    bbox_preds=None):
        """The reference's signature and its eleven targets (TARGET_NAMES, :179-182), distance targets clamped
        at 0 and centerness included (the loss uses neither the centerness nor the direction target)."""
        return self._reference_targets(self._targets(points, gt_bboxes_3d, gt_labels_3d, bbox_preds))

    # ---- test time: VoteHead.get_bboxes [dep-recall] as reached from :318-327 -----------------------
    def decode_scores(self, bbox_preds):
        """The torch restatement of the decode + scoring: coder.decode, softmax(obj_scores)[..., -1],
        softmax(sem_scores) -> the six outputs of ops.ca_detect_decode (its specification)."""
        box7 = self.bbox_coder.decode(bbox_preds)
        obj = F.softmax(bbox_preds["obj_scores"], dim=-1)[..., -1]
        sem = F.softmax(bbox_preds["sem_scores"], dim=-1)
        return box7, torch.cos(box7[..., 6]), torch.sin(box7[..., 6]), obj, sem, torch.argmax(sem, -1)

    def _decode(self, bbox_preds, fused=True):
        rows = bbox_preds.get("_rows")
        if fused and rows is not None and rows[0].is_cuda:
            return ops.ca_detect_decode(rows[1], rows[0], bbox_preds["ref_points"], self.num_dir_bins,
                                        self.bbox_coder.with_rot)
        return tuple(t.contiguous() for t in self.decode_scores(bbox_preds))

    @torch.no_grad()
    def get_bboxes_packed(self, points, bbox_preds, input_metas, store=None, fused=True):
        """``get_bboxes`` into a ``DetectionStore``: decode + score (one launch from the raw rows; ``fused=False``:
        the torch restatement) -> extent / point count -> class-aware aligned NMS -> pack.  -> the store."""
        return self._nms_pack(points, self._decode(bbox_preds, fused), store)

    @torch.no_grad()
    def get_bboxes(self, points, bbox_preds, input_metas, rescale=False, use_nms=True, fused=True):
        """-> list of (boxes, scores, labels) per scene, or the raw (B,K,7) boxes when ``use_nms`` is False."""
        if not use_nms:
            return self._decode(bbox_preds, fused)[0]
        return self._unpack(self.get_bboxes_packed(points, bbox_preds, input_metas, fused=fused), input_metas)
