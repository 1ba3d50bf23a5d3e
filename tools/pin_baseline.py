"""Golden-vector generator of the points-only baseline: runs the REAL reference CAVoteHead.loss / get_targets /
get_targets_single (demf/modeling/heads/class_agnostic_vote_head.py:24-316) and ClassAgnosticBBoxCoder.split_pred /
decode / decode_corners (demf/core/bbox/coders/class_agnostic_bbox_coder.py:8-137) on the CPU, under oracle/shim.py,
and writes

    tests/golden/ref_cavotehead.npz        inputs, the eleven targets, the losses, gradients (incl. the one that reaches
                                           the aggregated points through the distance targets), decoded boxes
    tests/golden/ref_baseline_config.json  configs/baseline/votenet.py and configs/_base_/models/votenet.py, evaluated

    python tools/pin_baseline.py           (needs the reference tree: DEMF_REFERENCE)

REAL: the two classes above.  RESTATED (oracle/deps.py): what they import from mmdet3d / mmdet - the loss classes,
VoteModule.get_loss, chamfer_distance, rotation_3d_in_axis, DepthInstance3DBoxes, PartialBinBasedBBoxCoder.  The
reference's CAVoteHead derives from mmdet3d's VoteHead, which the shim replaces by an empty module: the small
subclass below sets the attributes VoteHead.__init__ would set from the config.

The scene is hand-placed so that the head's branches are all taken (asserted below): positives in two boxes, proposals
near a centre but outside a thin box, proposals in the ignored 0.3-0.6 band, a positive ON a face (clamped distance
target exactly 0), a scene without ground truth.  Everything is run twice: in float32 (what the reference computes)
and in float64 on the same float32 inputs (``f64.*``: what the float32 numbers are roundings of).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import deps, shim  # noqa: E402
from oracle.pin_reference import _tag_tuples  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CONFIG_NAMES = {"baseline/votenet.py": ("model",), "_base_/models/votenet.py": ("model",)}
B, N, S, Q = 2, 256, 64, 32
TARGET_NAMES = ("vote_targets", "vote_target_masks", "dir_class_targets", "dir_res_targets", "mask_targets",
                "objectness_targets", "objectness_weights", "box_loss_weights", "distance_targets",
                "centerness_targets", "dir_targets")


def build_head():
    """The real CAVoteHead with the attributes mmdet3d VoteHead.__init__ sets, from the product's config."""
    from demf_amd.config import VoteNetCfg, votenet_head_kwargs
    ref = shim.reference()
    kw = votenet_head_kwargs(VoteNetCfg())

    class PinnedCAVoteHead(ref.head.CAVoteHead):
        def __init__(self):
            super().__init__()
            self.num_classes = kw["num_classes"]
            self.train_cfg, self.test_cfg = kw["train_cfg"], kw["test_cfg"]
            self.gt_per_seed = kw["vote_module_cfg"]["gt_per_seed"]
            self.num_proposal = kw["vote_aggregation_cfg"]["num_point"]
            self.bbox_coder = ref.coder.ClassAgnosticBBoxCoder(num_dir_bins=kw["bbox_coder"]["num_dir_bins"],
                                                               with_rot=kw["bbox_coder"]["with_rot"])
            self.num_dir_bins = self.bbox_coder.num_dir_bins
            self.vote_module = deps.VoteModule(**kw["vote_module_cfg"])
            for name in ("objectness_loss", "dir_class_loss", "dir_res_loss", "size_res_loss", "semantic_loss",
                         "iou_loss"):
                setattr(self, name, deps.build_loss(kw[name]))

    return PinnedCAVoteHead()


def make_scene(seed=5):
    """-> dict of float32 / int64 numpy inputs.  Scene 0: three boxes - A (rotated), B (axis-aligned, numbers on a
    binary grid), C (thin: 0.1 m along y); scene 1: no ground truth."""
    rng = np.random.default_rng(seed)
    gt0 = np.array([[-1.0, -1.0, 0.0, 1.2, 0.8, 1.0, 0.6],          # A: gravity centre (-1, -1, 0.5)
                    [1.0, 1.0, 0.25, 1.0, 0.5, 0.5, 0.0],            # B: gravity centre (1, 1, 0.5)
                    [2.0, -1.5, 0.0, 1.0, 0.1, 0.8, 0.0]],           # C: gravity centre (2, -1.5, 0.4)
                   np.float32)
    lab0 = np.array([3, 7, 1], np.int64)
    cA, cB, cC = np.array([-1.0, -1.0, 0.5]), np.array([1.0, 1.0, 0.5]), np.array([2.0, -1.5, 0.4])
    agg = rng.uniform([-3, -3, 0], [3, 3, 2], size=(B, Q, 3))
    a0 = agg[0]
    a0[0:6] = cA + rng.uniform(-0.12, 0.12, size=(6, 3))             # positives of A
    a0[6:11] = cB + rng.uniform(-0.1, 0.1, size=(5, 3))              # positives of B
    a0[11] = cB + [0.0, 0.25, 0.0]                                   # ON B's left face (dy / 2 = 0.25), 0.25 from the centre
    a0[12] = cC + [0.0, 0.15, 0.0]                                   # 0.15 from C's centre, outside its 0.05 half width
    a0[13] = cC + [0.1, -0.2, 0.05]
    a0[14] = cC + [-0.05, 0.12, -0.1]
    a0[15] = cA + [0.45, 0.0, 0.0]                                   # in the 0.3-0.6 band: objectness mask 0
    a0[16] = cB + [0.0, 0.0, 0.5]
    a0[17] = cA + [0.0, -0.35, 0.2]
    agg = np.round(agg * 1024) / 1024
    points = rng.uniform([-3, -3, 0, 0], [3, 3, 2, 2], size=(B, N, 4))
    for k, (c, half) in enumerate(((cA, 0.3), (cB, 0.2), (cC, 0.04))):
        points[0, 40 * k:40 * k + 40, :3] = c + rng.uniform(-half, half, size=(40, 3))
    points[0, 120:140, :3] = (cA + cB) / 2 + rng.uniform(-1.0, 1.0, size=(20, 3))
    points = points.astype(np.float32)
    seed_idx = np.stack([rng.permutation(N)[:S] for _ in range(B)]).astype(np.int64)
    seed_idx[0, :30] = np.arange(0, 120, 4)                          # seeds on points inside the boxes
    seed_pts = np.take_along_axis(points[..., :3], seed_idx[..., None].repeat(3, -1), 1)
    vote_pts = seed_pts + rng.normal(0, 0.3, size=seed_pts.shape)
    cls = rng.standard_normal((B, 12, Q))
    reg = rng.standard_normal((B, 30, Q)) * 0.5
    # log-distances near those of the assigned box for the positives: the IoU is then neither 0 nor 1
    reg[0, 0:6, 0:12] = np.log(np.array([0.6, 0.4, 0.5, 0.6, 0.4, 0.5]))[:, None] + rng.normal(0, 0.3, size=(6, 12))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)              # noqa: E731
    return dict(cls_preds=f32(cls), reg_preds=f32(reg), aggregated_points=f32(agg), points=points,
                seed_points=f32(seed_pts), seed_indices=seed_idx, vote_points=f32(vote_pts),
                gt_boxes_0=gt0, gt_labels_0=lab0, gt_boxes_1=np.zeros((0, 7), np.float32),
                gt_labels_1=np.zeros((0,), np.int64))


def run(head, scene, dtype):
    """The real split_pred -> loss (with ret_target) -> backward, and decode, in ``dtype``."""
    t = lambda k: torch.from_numpy(scene[k]).to(dtype)               # noqa: E731
    cls, reg, vote = t("cls_preds").requires_grad_(), t("reg_preds").requires_grad_(), t("vote_points").requires_grad_()
    # a leaf with a gradient, as the output of the vote aggregation is: the reference builds its distance targets from
    # the aggregated points without detaching them (:271-294), so the loss reaches them through the TARGETS
    agg = t("aggregated_points").requires_grad_()
    preds = head.bbox_coder.split_pred(cls, reg, agg)
    preds.update(seed_points=t("seed_points"), seed_indices=torch.from_numpy(scene["seed_indices"]),
                 vote_points=vote, aggregated_points=agg)
    gtb = [deps.DepthInstance3DBoxes(t("gt_boxes_%d" % b)) for b in range(B)]
    gtl = [torch.from_numpy(scene["gt_labels_%d" % b]) for b in range(B)]
    points = [p for p in t("points")]
    losses = head.loss(preds, points, gtb, gtl, None, None, None, ret_target=True)
    targets = losses.pop("targets")
    sum(losses.values()).backward()
    out = {"loss." + k: v.detach().numpy() for k, v in losses.items()}
    for n, v in zip(TARGET_NAMES, targets):
        out["target." + n] = v.detach().numpy()
    out.update({"grad.cls_preds": cls.grad.numpy(), "grad.reg_preds": reg.grad.numpy(),
                "grad.vote_points": vote.grad.numpy(), "grad.aggregated_points": agg.grad.numpy()})
    with torch.no_grad():
        out["decode"] = head.bbox_coder.decode(preds).numpy()
        out["corners"] = head.bbox_coder.decode_corners(preds["distance"], preds["ref_points"]).numpy()
        for k in ("distance", "dir_class", "dir_res_norm", "dir_res", "obj_scores", "sem_scores", "ref_points"):
            out["split." + k] = preds[k].detach().numpy()
    return out


def check_branches(scene, out):
    """The layout exercises the head's branches (scene 0; scene 1 has no ground truth)."""
    obj = out["target.objectness_targets"]
    bw, ow = out["target.box_loss_weights"], out["target.objectness_weights"]
    dist = out["target.distance_targets"]
    centres = np.array([[-1.0, -1.0, 0.5], [1.0, 1.0, 0.5], [2.0, -1.5, 0.4]])
    d = np.linalg.norm(scene["aggregated_points"][0][:, None, :] - centres[None], axis=-1)
    near, which = d.min(1), d.argmin(1)
    pos = obj[0] == 1
    assert pos.sum() >= 8 and len(set(which[pos])) >= 2, (pos.sum(), set(which[pos]))
    assert ((near < 0.3) & ~pos).sum() >= 2, "proposals near a centre but outside the box"
    assert ((near > 0.3) & (near < 0.6) & (ow[0] == 0)).sum() >= 2, "proposals in the ignored band"
    assert (pos & (dist[0] == 0).any(-1)).sum() >= 1, "a positive with a clamped distance target of exactly 0"
    assert ((~pos) & (dist[0] == 0).any(-1)).sum() >= 2, "negatives with clamped targets"
    assert scene["gt_boxes_1"].shape[0] == 0 and obj[1].sum() == 0 and (bw[1] == 0).all()
    for k, v in out.items():
        if k.startswith("loss."):
            assert np.isfinite(v) and v != 0, (k, v)
    assert sum(k.startswith("loss.") for k in out) == 7            # vote + six head terms: no centre loss
    assert all(np.abs(out["grad." + k]).max() > 0 for k in ("cls_preds", "reg_preds", "vote_points",
                                                             "aggregated_points"))


def config_goldens():
    out = {}
    for rel, names in CONFIG_NAMES.items():
        ns = {}
        with open(os.path.join(shim.REF, "configs", rel)) as f:
            exec(compile(f.read(), rel, "exec"), ns)
        out[rel] = {k: _tag_tuples(ns[k]) for k in names}
    return out


def main():
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "ref_baseline_config.json"), "w") as f:
        json.dump(config_goldens(), f, indent=1)
        f.write("\n")
    head, scene = build_head(), make_scene()
    out32 = run(head, scene, torch.float32)
    check_branches(scene, out32)
    out64 = run(head, scene, torch.float64)
    fixture = {"in." + k: v for k, v in scene.items()}
    fixture.update(out32)
    fixture.update({"f64." + k: v for k, v in out64.items()
                    if k.startswith(("loss.", "grad.")) or k in ("decode", "target.distance_targets")})
    path = os.path.join(GOLD, "ref_cavotehead.npz")
    np.savez_compressed(path, **fixture)
    size = os.path.getsize(path)
    assert size < 77 * 1024, size
    print("ref_cavotehead.npz: %d bytes, %d positives" % (size, int(out32["target.objectness_targets"].sum())))
    print({k: float(v) for k, v in out32.items() if k.startswith("loss.")})


if __name__ == "__main__":
    main()
