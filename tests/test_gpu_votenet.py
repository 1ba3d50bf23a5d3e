"""The points-only class-agnostic VoteNet baseline (demf_amd.modules.VoteNet: PointNet2SASSG -> CAVoteHead) on the GPU
as ONE chain - backbone, vote module, aggregation, prediction head, batched targets, the fused distance-form loss and
its backward, the fused decode + NMS + packing - against an fp64 oracle chain on the CPU built here from oracle/
pieces (oracle/deps.py modules, oracle/model.py's target generation) and the loss classes of oracle/deps.py.

Bars: those tests/test_gpu_model.py holds the DeMF path to at this size against its goldens - 1e-4 up to the vote
stage, 5e-4 of scale on the raw head outputs, 5e-4 on every loss term, per-parameter gradient norms within 1.5e-2
(the bulk within 5e-3), bit-exact indices and integer targets.  The input is chosen by the oracle alone: a fixed
seed (SEED), the first for which the SAME chain in fp32 on the CPU sits within half of those bars of its fp64 run and at least four
proposals are positive (an untrained 30-BatchNorm
network amplifies a single near-tie of a max-pool; such a seed says nothing about the kernels)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import deps, fixtures
from oracle import torch_ops as O
from oracle.model import OracleHead

pytestmark = pytest.mark.gpu

B, N, Q = 2, 2048, 64
LOSS_KEYS = ("vote_loss", "objectness_loss", "dir_class_loss", "dir_res_loss", "size_res_loss", "semantic_loss",
             "iou_loss")
INT_TARGETS = ("vote_target_masks", "dir_class_targets", "mask_targets", "objectness_targets")
TARGET_MAP = dict(vote_targets="vote_targets", vote_target_masks="vote_target_masks",
                  dir_class_targets="dir_class_targets", dir_res_targets="dir_res_targets", mask_targets="mask_targets",
                  objectness_targets="objectness_targets", objectness_weights="objectness_weights",
                  box_loss_weights="box_loss_weights", dir_targets="dir_targets")


def _cfg():
    """The scaled-down configuration of tests/test_gpu_detector.py (fixtures.tiny_cfg's backbone) under the baseline's
    head: 64 proposals, aggregation and prediction head at half the seed width, as in configs/_base_/models/votenet.py."""
    from demf_amd.config import CAHeadCfg, VoteNetCfg
    return VoteNetCfg(backbone=fixtures.tiny_cfg().backbone,
                      head=CAHeadCfg(in_channels=64, vote_conv_channels=(64, 64), num_proposal=Q, agg_radius=0.6,
                                     agg_num_sample=8, agg_mlp_channels=(64, 32, 32, 32), pred_in_channels=32,
                                     shared_conv_channels=(32, 32)))


class OracleCAHead(nn.Module):
    """CAVoteHead (class_agnostic_vote_head.py:24-316) from oracle pieces: VoteModule / PointSAModule /
    BaseConvBboxHead and the loss classes of oracle/deps.py, the target generation of oracle/model.py (the same
    quantities: :279-294 against :913-929), split_pred and decode_corners of class_agnostic_bbox_coder.py:88-137."""
    targets, targets_single = OracleHead.targets, OracleHead.targets_single

    def __init__(self, kw):
        super().__init__()
        from oracle.model import Coder
        self.gt_per_seed = kw["vote_module_cfg"]["gt_per_seed"]
        self.num_proposal = kw["vote_aggregation_cfg"]["num_point"]
        self.coder = Coder(kw["bbox_coder"]["num_dir_bins"])
        self.nb, self.train_cfg = self.coder.nb, kw["train_cfg"]
        self.losses = {k: deps.build_loss(kw[k]) for k in ("objectness_loss", "dir_res_loss", "dir_class_loss",
                                                           "size_res_loss", "semantic_loss", "iou_loss")}
        self.vote_module = deps.VoteModule(**kw["vote_module_cfg"])
        self.vote_aggregation = deps.build_sa_module(kw["vote_aggregation_cfg"])
        self.conv_pred = deps.BaseConvBboxHead(**kw["pred_layer_cfg"], num_cls_out_channels=kw["num_classes"] + 2,
                                               num_reg_out_channels=6 + 2 * self.nb)

    def forward(self, seed_points, seed_features, seed_indices):
        vote_points, vote_features, vote_offset = self.vote_module(seed_points, seed_features)
        sample = O.furthest_point_sample(seed_points, self.num_proposal)
        agg, feats, agg_idx = self.vote_aggregation(points_xyz=vote_points, features=vote_features, indices=sample)
        cls_p, reg_p = self.conv_pred(feats)
        c, r = cls_p.transpose(2, 1), reg_p.transpose(2, 1)
        nb = self.nb
        return dict(seed_points=seed_points, seed_indices=seed_indices, vote_points=vote_points,
                    vote_features=vote_features, aggregated_points=agg, aggregated_indices=agg_idx,
                    distance=r[..., 0:6].exp(), dir_class=r[..., 6:6 + nb], dir_res_norm=r[..., 6 + nb:6 + 2 * nb],
                    obj_scores=c[..., 0:2], sem_scores=c[..., 2:], ref_points=agg, _cls=c, _reg=r)

    def loss(self, p, points, gt_boxes, gt_labels):
        t = self.targets(points, [deps.DepthInstance3DBoxes(b) for b in gt_boxes], gt_labels, p["aggregated_points"])
        Lf, bw = self.losses, t["box_loss_weights"].to(points.dtype)
        dist_t = t["distance_targets"].clamp(min=0)
        onehot = F.one_hot(t["dir_class_targets"], self.nb).to(points.dtype)
        corners = lambda d: torch.cat([p["ref_points"] - d[..., 3:6], p["ref_points"] + d[..., 0:3]], -1)   # noqa: E731
        return dict(
            vote_loss=self.vote_module.get_loss(p["seed_points"], p["vote_points"], p["seed_indices"],
                                                t["vote_target_masks"], t["vote_targets"]),
            objectness_loss=Lf["objectness_loss"](p["obj_scores"].transpose(2, 1), t["objectness_targets"],
                                                  weight=t["objectness_weights"]),
            dir_class_loss=Lf["dir_class_loss"](p["dir_class"].transpose(2, 1), t["dir_class_targets"], weight=bw),
            dir_res_loss=Lf["dir_res_loss"](torch.sum(p["dir_res_norm"] * onehot, -1), t["dir_res_targets"], weight=bw),
            size_res_loss=Lf["size_res_loss"](p["distance"], dist_t, weight=bw.unsqueeze(-1).repeat(1, 1, 6)),
            semantic_loss=Lf["semantic_loss"](p["sem_scores"].transpose(2, 1), t["mask_targets"], weight=bw),
            iou_loss=Lf["iou_loss"](corners(p["distance"]), corners(dist_t), weight=bw)), t


class OracleVoteNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        from demf_amd.config import votenet_head_kwargs
        b = cfg.backbone
        self.backbone = deps.PointNet2SASSG(in_channels=b.in_channels, num_points=b.num_points, radius=b.radius,
                                            num_samples=b.num_samples, sa_channels=b.sa_channels,
                                            fp_channels=b.fp_channels, use_xyz=b.use_xyz, normalize_xyz=b.normalize_xyz)
        self.bbox_head = OracleCAHead(votenet_head_kwargs(cfg))

    def run(self, points, gt_boxes, gt_labels):
        x = self.backbone(points)
        preds = self.bbox_head(x["fp_xyz"][-1], x["fp_features"][-1], x["fp_indices"][-1])
        losses, targets = self.bbox_head.loss(preds, points, gt_boxes, gt_labels)
        self.zero_grad()
        sum(losses.values()).backward()
        grads = {n: p.grad.detach().clone() for n, p in self.named_parameters() if p.grad is not None}
        return dict(preds=preds, losses=losses, targets=targets, grads=grads)


def _batch(seed):
    """The seeded scene batch + three boxes per scene dropped onto proposals of the fp64 oracle chain (as
    oracle/pin_reference.py does for the DeMF goldens): the votes of an untrained network rarely end within 0.3 m of
    a box centre, and without positive proposals every box term of the loss is 0."""
    cfg = _cfg()
    batch = fixtures.make_scene_batch(B, N, fixtures.TINY_PYRAMID, fixtures.TINY_INPUT, 64, seed=seed, n_gt=4)
    m = OracleVoteNet(cfg)
    fixtures.seed_weights(m, seed)
    m = m.double().train()
    with torch.no_grad():
        x = m.backbone(torch.from_numpy(batch["points"]).double())
        agg = m.bbox_head(x["fp_xyz"][-1], x["fp_features"][-1], x["fp_indices"][-1])["aggregated_points"].numpy()
    rng = np.random.default_rng(seed + 100)
    for b in range(B):
        pick = rng.choice(agg.shape[1], size=3, replace=False)
        ctr = agg[b, pick] + rng.normal(0, 0.04, size=(3, 3))
        dims = rng.uniform(0.6, 1.4, size=(3, 3))
        yaw = rng.uniform(-np.pi, np.pi, size=(3, 1))
        extra = np.concatenate([ctr - [0, 0, 1] * dims * 0.5, dims, yaw], 1).astype(np.float32)
        batch["gt_boxes"][b] = np.concatenate([batch["gt_boxes"][b], extra], 0)
        batch["gt_labels"][b] = np.concatenate([batch["gt_labels"][b], rng.integers(0, 10, size=3)])
    return cfg, batch


def _oracle_run(cfg, batch, seed, dtype):
    m = OracleVoteNet(cfg)
    fixtures.seed_weights(m, seed)
    m = m.to(dtype).train()
    return m.run(torch.from_numpy(batch["points"]).to(dtype), [torch.from_numpy(b).to(dtype) for b in batch["gt_boxes"]],
                 [torch.from_numpy(l) for l in batch["gt_labels"]])


FWD_KEYS = (("seed_points", 1e-4), ("vote_points", 1e-4), ("aggregated_points", 1e-4), ("_cls", 5e-4), ("_reg", 5e-4))


def _deviation(run, truth, verbose=False):
    """The largest error of ``run`` against ``truth`` as a FRACTION of each bar -> (fraction, what); indices and integer
    targets must be equal (else inf)."""
    worst = (0.0, "")
    for k in ("seed_indices", "aggregated_indices"):
        if not torch.equal(run["preds"][k].cpu().long(), truth["preds"][k].long()):
            return float("inf"), k
    for k, bar in FWD_KEYS:
        t = truth["preds"][k].detach().double()
        e = float((run["preds"][k].detach().double().cpu() - t).abs().max()) / max(1.0, float(t.abs().max()))
        worst = max(worst, (e / bar, k))
    for k in INT_TARGETS:
        if not torch.equal(run["targets"][k].cpu(), truth["targets"][k]):
            return float("inf"), "target " + k
    for k in LOSS_KEYS:
        t = float(truth["losses"][k].detach())
        worst = max(worst, (abs(float(run["losses"][k].detach()) - t) / (5e-4 * max(abs(t), 1e-12)), "loss " + k))
    close, rows = [], []
    for n, g in truth["grads"].items():
        want, got = float(g.double().norm()), float(run["grads"][n].double().norm())
        worst = max(worst, (abs(got - want) / (1.5e-2 * want + 1e-4), "grad " + n))
        close.append(abs(got - want) <= 5e-3 * want + 1e-4)
        rows.append((abs(got - want) / (5e-3 * want + 1e-4), n, want, got))
    if verbose:
        print("[votenet] gradient norms within 5e-3: %.3f; furthest (x the 5e-3 bar, name, fp64 norm, norm): %s"
              % (np.mean(close), [(round(r[0], 2), r[1], "%.3e" % r[2], "%.3e" % r[3]) for r in sorted(rows)[::-1][:10]]))
    if np.mean(close) < 0.95:
        return float("inf"), "fewer than 95 % of the gradient norms within 5e-3"
    return worst


_CASE = {}
SEED = 1          # the input of every test below; found by trying seeds 1, 2, ... with the rule of the module docstring


def _qualified_case():
    """(cfg, batch, SEED, fp64 run), once per session.  The seed is fixed; that it (still) qualifies - the CPU fp32 chain
    within half of the bars of the fp64 one, at least four positive proposals - is asserted, by the CPU oracle alone."""
    if not _CASE:
        cfg, batch = _batch(SEED)
        truth = _oracle_run(cfg, batch, SEED, torch.float64)
        frac, what = _deviation(_oracle_run(cfg, batch, SEED, torch.float32), truth)
        pos = int(truth["targets"]["objectness_targets"].sum())
        print("[votenet] seed %d: cpu fp32 at %.2f of the bars (%s), %d positive proposals" % (SEED, frac, what, pos))
        assert frac <= 0.5 and pos >= 4, "seed %d no longer qualifies on this host: choose another by the same rule" % SEED
        _CASE.update(cfg=cfg, batch=batch, seed=SEED, truth=truth)
    return _CASE["cfg"], _CASE["batch"], _CASE["seed"], _CASE["truth"]


def _model(cfg, seed, train=True):
    from demf_amd.modules import VoteNet
    m = VoteNet(cfg)
    fixtures.seed_weights(m, seed)
    return m.cuda().train(train)


def _dev(batch):
    return (torch.from_numpy(batch["points"]).cuda(), [torch.from_numpy(b).cuda() for b in batch["gt_boxes"]],
            [torch.from_numpy(l).cuda() for l in batch["gt_labels"]])


def test_state_dicts_of_model_and_oracle_chain_agree():
    cfg = _cfg()
    from demf_amd.modules import VoteNet
    assert sorted(VoteNet(cfg).state_dict()) == sorted(OracleVoteNet(cfg).state_dict())


def test_forward_loss_backward_vs_fp64_oracle_chain():
    cfg, batch, seed, truth = _qualified_case()
    model = _model(cfg, seed)
    points, gb, gl = _dev(batch)
    preds = model.forward_head(points)
    assert not dict.__contains__(preds, "distance") and not dict.__contains__(preds, "dir_res")   # nothing materialised
    head = model.bbox_head
    tg = dict(zip(head.TARGET_NAMES, head.get_targets(points, gb, gl, None, None, preds)))
    losses = head.loss(preds, points, gb, gl)
    assert set(losses) == {"vote_loss", "_total", *head.LOSS_NAMES}
    total = losses.pop("_total")
    np.testing.assert_allclose(total.item(), sum(v.item() for v in losses.values()), rtol=1e-5)
    total.backward()
    run = dict(preds=dict(preds, _cls=preds["_rows"][0], _reg=preds["_rows"][1]), losses=losses,
               targets={k: tg[v] for k, v in TARGET_MAP.items()},
               grads={n: p.grad for n, p in model.named_parameters() if p.grad is not None})
    assert sorted(run["grads"]) == sorted(truth["grads"])
    frac, what = _deviation(run, truth, verbose=True)
    print("[votenet] seed %d: GPU at %.2f of the bars (%s)" % (seed, frac, what))
    assert frac <= 1.0, (frac, what)
    for k in ("vote_targets", "dir_res_targets", "objectness_weights", "box_loss_weights", "dir_targets"):
        np.testing.assert_allclose(tg[k].cpu().numpy(), truth["targets"][k].detach().numpy(), rtol=1e-4, atol=1e-4,
                                   err_msg=k)
    np.testing.assert_allclose(tg["distance_targets"].cpu().numpy(),
                               truth["targets"]["distance_targets"].detach().clamp(min=0).numpy(), rtol=1e-4, atol=1e-4)


def test_fused_loss_equals_torch_restatement_on_the_same_predictions():
    cfg, batch, seed, _ = _qualified_case()
    model = _model(cfg, seed)
    points, gb, gl = _dev(batch)
    preds = model.forward_head(points)
    head = model.bbox_head
    fused = head.loss(preds, points, gb, gl)
    plain = head._loss(preds, head._targets(points, gb, gl, preds))
    for k, v in plain.items():
        np.testing.assert_allclose(fused[k].item(), v.item(), rtol=2e-5, err_msg=k)
    params = [p for p in model.parameters() if p.requires_grad]
    g1 = torch.autograd.grad(fused["_total"], params, retain_graph=True, allow_unused=True)
    g2 = torch.autograd.grad(sum(plain.values()), params, allow_unused=True)
    for (n, _), a, b in zip(model.named_parameters(), g1, g2):
        assert (a is None) == (b is None), n
        if a is not None:
            assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-7, n


def test_get_bboxes_fused_equals_torch_restatement():
    """decode + score by the kernel (raw rows) and by the torch restatement (coder.decode + softmax), each followed by
    the shared point count / NMS / pack: the same boxes in the same order."""
    cfg, batch, seed, _ = _qualified_case()
    model = _model(cfg, seed, train=False)
    with torch.no_grad():
        for m in (model.bbox_head.conv_pred.conv_reg, model.bbox_head.conv_pred.conv_cls):
            m.weight.mul_(6.0)              # eval-mode BN on seeded weights: spread the scores and the sizes
    points, _, _ = _dev(batch)
    with torch.no_grad():
        preds = model.forward_head(points)
        a = model.bbox_head.get_bboxes(points, preds, None, fused=True)
        b = model.bbox_head.get_bboxes(points, preds, None, fused=False)
        raw_a = model.bbox_head.get_bboxes(points, preds, None, use_nms=False, fused=True)
        raw_b = model.bbox_head.get_bboxes(points, preds, None, use_nms=False, fused=False)
    np.testing.assert_allclose(raw_a.cpu().numpy(), raw_b.cpu().numpy(), rtol=0, atol=2e-5)
    assert sum(len(x[1]) for x in a) > 0, "no detection survives: the test would compare nothing"
    for (ba, sa, la), (bb, sb, lb) in zip(a, b):
        assert torch.equal(la, lb)
        np.testing.assert_allclose(ba.tensor.cpu().numpy(), bb.tensor.cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(sa.cpu().numpy(), sb.cpu().numpy(), rtol=0, atol=1e-6)
    res = model.simple_test(points, None)
    assert len(res) == B and all(set(r) == {"boxes_3d", "scores_3d", "labels_3d"} for r in res)
    assert [len(r["scores_3d"]) for r in res] == [len(x[1]) for x in a]


@pytest.mark.no_library_fallback
def test_reference_widths_run_on_the_packages_kernels():
    """configs/baseline/votenet.py sizes (20 000 points, 256 proposals, aggregation [256, 128, 128, 128], prediction head
    on 128 channels), B = 1, library fall-backs refused: one forward + loss + backward runs, everything is finite, and
    every GEMM-shaped launch reports a kernel form of this package (demf_mlp_last_form)."""
    from demf_amd import _ffi
    from demf_amd.config import VoteNetCfg
    from demf_amd.modules import VoteNet
    cfg = VoteNetCfg()
    batch = fixtures.make_scene_batch(1, 20000, fixtures.TINY_PYRAMID, fixtures.TINY_INPUT, 64, seed=1, n_gt=6)
    model = VoteNet(cfg)
    fixtures.seed_weights(model, 1)
    model.cuda().train()
    points, gb, gl = _dev(batch)
    record, orig, lib = [], _ffi.call, _ffi.load()

    def spy(name, *a):
        rc = orig(name, *a)
        record.append((name, lib.demf_mlp_last_form()))
        return rc
    try:
        _ffi.call = spy
        losses = model.forward_train(points, None, gb, gl)
        losses["_total"].backward()
    finally:
        _ffi.call = orig
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    names = [n for n, _ in record]
    assert "demf_ca_head_loss_fwd" in names and "demf_ca_head_loss_bwd" in names
    mlp = [(n, f) for n, f in record if n.startswith(("demf_mlp_gemm_fwd", "demf_mlp_bwd", "demf_mlp_gemm_bwd"))]
    assert mlp and all(f > 0 for _, f in mlp), mlp
    seen = {}
    for n, f in mlp:
        seen.setdefault(n, set()).add(f)
    print("[votenet] reference widths, kernel forms per entry point:", {k: sorted(v) for k, v in sorted(seen.items())})
