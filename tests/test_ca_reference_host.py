"""The points-only baseline on the CPU: the torch restatement of CAVoteHead (demf_amd/modules/ca_head.py) and the
float64 row-form reference of its two kernels (tests/ca_loss_reference.py) against the output of the REAL reference
classes (tests/golden/ref_cavotehead.npz, written by tools/pin_baseline.py), and the measurement that sets the
tolerance constants of the GPU kernel tests (tests/ca_loss_cases.py)."""
import math
import os

import numpy as np
import pytest
import torch

import ca_loss_cases as cc
import ca_loss_reference as cr
import loss_reference as lr
from helpers import load_golden

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_TARGETS = ("vote_target_masks", "dir_class_targets", "mask_targets", "objectness_targets")


@pytest.fixture(scope="module")
def gold():
    return load_golden(GOLD, "ref_cavotehead")


@pytest.fixture(scope="module")
def head():
    from demf_amd.config import VoteNetCfg, votenet_head_kwargs
    from demf_amd.modules import CAVoteHead
    return CAVoteHead(**votenet_head_kwargs(VoteNetCfg()))


def _inputs(gold, dtype=torch.float32):
    t = lambda k: torch.from_numpy(gold["in." + k])                          # noqa: E731
    f = lambda k: t(k).to(dtype)                                             # noqa: E731
    B = gold["in.points"].shape[0]
    return dict(cls=f("cls_preds"), reg=f("reg_preds"), agg=f("aggregated_points"), points=f("points"),
                seed_points=f("seed_points"), seed_indices=t("seed_indices"), vote_points=f("vote_points"),
                gt_boxes=[f("gt_boxes_%d" % b) for b in range(B)], gt_labels=[t("gt_labels_%d" % b) for b in range(B)])


def _preds(head, x, leaves=False):
    cls, reg, vote, agg = x["cls"], x["reg"], x["vote_points"], x["agg"]
    if leaves:
        cls, reg, vote, agg = (v.clone().requires_grad_() for v in (cls, reg, vote, agg))
    preds = head.bbox_coder.split_pred(cls, reg, agg)
    dict.update(preds, seed_points=x["seed_points"], seed_indices=x["seed_indices"], vote_points=vote,
                aggregated_points=agg)
    return preds, (cls, reg, vote, agg)


def _rows(gold):
    """The fixture in the kernels' row form: (cls (R,12), reg (R,30), ref (R,3), the row-form targets)."""
    cls = torch.from_numpy(gold["in.cls_preds"]).transpose(1, 2).reshape(-1, 12)
    reg = torch.from_numpy(gold["in.reg_preds"]).transpose(1, 2).reshape(-1, 30)
    ref = torch.from_numpy(gold["in.aggregated_points"]).reshape(-1, 3)
    t = lambda n: torch.from_numpy(gold["target." + n])                      # noqa: E731
    rest = (t("distance_targets").reshape(-1, 6), t("dir_class_targets").reshape(-1), t("dir_res_targets").reshape(-1),
            t("mask_targets").reshape(-1), t("objectness_targets").reshape(-1), t("objectness_weights").reshape(-1),
            t("box_loss_weights").reshape(-1))
    return cls, reg, ref, rest, t("dir_targets").reshape(-1)


# ---- the torch restatement against the real classes ------------------------------------------------------------
def test_split_pred_and_decode_match_the_reference_coder(gold, head):
    preds, _ = _preds(head, _inputs(gold))
    assert not dict.__contains__(preds, "distance") and not dict.__contains__(preds, "dir_res")    # lazy
    for k in ("distance", "dir_class", "dir_res_norm", "dir_res", "obj_scores", "sem_scores", "ref_points"):
        np.testing.assert_array_equal(preds[k].numpy(), gold["split." + k], err_msg=k)
    np.testing.assert_allclose(head.bbox_coder.decode(preds).numpy(), gold["decode"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(head.bbox_coder.decode_corners(preds["distance"], preds["ref_points"]).numpy(),
                                  gold["corners"])
    box7, cosy, siny, obj, sem, classes = head.decode_scores(preds)
    assert torch.equal(box7, head.get_bboxes(None, preds, None, use_nms=False))
    assert obj.shape == classes.shape == box7.shape[:2] and sem.shape[-1] == 10


def test_coder_encode_halves_the_dimensions(head):
    from demf_amd.modules import DeMFClassAgnosticBBoxCoder
    dims = torch.tensor([[1.0, 2.0, 0.5], [0.6, 0.7, 1.1]])
    centre, yaw, lab = torch.zeros(2, 3), torch.tensor([0.4, -2.9]), torch.tensor([1, 4])
    ours = head.bbox_coder.encode(centre, dims, yaw, lab, ret_dir_target=True)
    demf = DeMFClassAgnosticBBoxCoder(12).encode(centre, dims, yaw, lab, ret_dir_target=True)
    assert len(ours) == 5 and torch.equal(ours[1], dims / 2) and torch.equal(demf[1], dims)
    for a, b in zip(ours[2:], demf[2:]):
        assert torch.equal(a, b)


def test_targets_match_the_reference_head(gold, head):
    x = _inputs(gold)
    preds, _ = _preds(head, x)
    targets = head.get_targets(list(x["points"]), x["gt_boxes"], x["gt_labels"], None, None, preds)
    assert len(targets) == len(head.TARGET_NAMES) == 11
    for name, got in zip(head.TARGET_NAMES, targets):
        want = gold["target." + name]
        if name in INT_TARGETS:
            assert got.dtype == torch.int64
            np.testing.assert_array_equal(got.numpy(), want, err_msg=name)
        else:
            np.testing.assert_allclose(got.numpy(), want, rtol=2e-6, atol=2e-7, err_msg=name)
    obj = gold["target.objectness_targets"]
    assert obj[0].sum() >= 8 and obj[1].sum() == 0                           # the fixture has the branches
    assert (gold["target.distance_targets"][0][obj[0] == 1] == 0).any()


def test_loss_and_gradients_match_the_reference_head(gold, head):
    x = _inputs(gold)
    preds, leaves = _preds(head, x, leaves=True)
    losses = head.loss(preds, list(x["points"]), x["gt_boxes"], x["gt_labels"])
    assert set(losses) == {"vote_loss", *head.LOSS_NAMES} and "center_loss" not in losses
    for k, v in losses.items():
        np.testing.assert_allclose(v.detach().numpy(), gold["loss." + k], rtol=4e-6, err_msg=k)
    g = torch.autograd.grad(sum(losses.values()), leaves)
    # (aggregated_points: the gradient the reference sends to the proposal points through its distance targets)
    for name, got in zip(("cls_preds", "reg_preds", "vote_points", "aggregated_points"), g):
        want = gold["grad." + name]
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=1e-6 * np.abs(want).max(), err_msg=name)


def test_loss_in_float64_matches_the_reference_head_in_float64(gold, head):
    x = _inputs(gold, torch.float64)
    preds, _ = _preds(head, x)
    losses = head.loss(preds, list(x["points"]), x["gt_boxes"], x["gt_labels"])
    for k, v in losses.items():
        # (the reference's own box_loss_weights are float32 in its float64 run: objectness_targets.float(), :170)
        np.testing.assert_allclose(v.numpy(), gold["f64.loss." + k], rtol=2e-7, err_msg=k)


# ---- the float64 row-form reference of the kernels against the real classes ------------------------------------
def test_row_form_reference_matches_the_reference_head(gold, head):
    cls, reg, ref, rest, dir_t = _rows(gold)
    # (the fixture's distance targets are the clamped ones the reference returns; on the rows that carry a weight - the
    # positives, which lie inside their box - no raw target is negative, so the clamp's mask is the same)
    sums, A, g, T = cr.head_loss_ref(cls, reg, ref, head._hyper(), *rest, gout=torch.ones(7), dir_t=dir_t)
    from demf_amd import ops
    for i, name in enumerate(ops.HEAD_LOSS_NAMES):
        if name == "center_loss":
            assert float(sums[i]) == 0.0 and float(A[i]) == 0.0
            continue
        # against the reference's float64 run to its float32 weights' rounding, against its float32 run within the bound
        np.testing.assert_allclose(float(sums[i]), gold["f64.loss." + name], rtol=2e-7, err_msg=name)
        assert lr.error_units(gold["loss." + name], sums[i], A[i]) <= cc.C_F_CA, name
    B, Q = gold["in.aggregated_points"].shape[:2]
    for got, name, n in ((g[0], "cls_preds", 12), (g[1], "reg_preds", 30)):
        want = torch.from_numpy(gold["f64.grad." + name]).transpose(1, 2).reshape(B * Q, n)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=1e-7 * float(want.abs().max()), err_msg=name)
    want = torch.from_numpy(gold["f64.grad.aggregated_points"]).reshape(B * Q, 3)
    assert float(want.abs().max()) > 0
    np.testing.assert_allclose(g[2].numpy(), want.numpy(), rtol=1e-6, atol=1e-7 * float(want.abs().max()))
    assert lr.error_units(gold["grad.aggregated_points"].reshape(B * Q, 3), g[2], T[2]) <= cc.C_G_CA
    # with the targets held constant the loss does not depend on the reference points: rounding noise
    _, _, g0, T0 = cr.head_loss_ref(cls, reg, ref, head._hyper(), *rest, gout=torch.ones(7), ref_grad=False)
    assert float(g0[2].abs().max()) <= 1e-12 * float(g0[1].abs().max()) and float(T0[2].abs().max()) == 0.0


def test_row_form_decode_reference_matches_the_reference_coder(gold):
    cls, reg, ref, _, _ = _rows(gold)
    B, Q = gold["in.aggregated_points"].shape[:2]
    r = cr.decode_ref(reg.view(B, Q, 30), cls.view(B, Q, 12), ref.view(B, Q, 3))
    assert lr.error_units(gold["decode"], r["box7"], r["scale7"]) <= cc.C_BOX_CA
    assert lr.error_units(gold["f64.decode"], r["box7"], r["scale7"]) <= 0.5     # (class index * bin width in fp32, as upstream)


# ---- the constants of the GPU tests ----------------------------------------------------------------------------
def _pow2_of_4x(worst):
    return 2.0 ** math.ceil(math.log2(4 * worst))


def test_fp32_composition_sets_the_constants():
    """The fp32 torch composition against the fp64 reference over every case of ca_loss_cases: the constants are 4x
    its worst error, rounded up to a power of two.  The same composition in fp64 agrees with the reference to 1e-6
    units: the reference and the composition state the same formulas."""
    wf = wg = 0.0
    for name, (c, hyper) in cc.head_cases().items():
        sums, A, g, T = cr.head_loss_ref(c["cls"], c["reg"], c["ref"], hyper, *[c[k] for k in cc.CA_KEYS[2:]],
                                         gout=cc.GOUT, dir_t=c["dir_t"])
        for dtype in (torch.float32, torch.float64):
            s, gg = cc.head_composition(c, dtype, hyper)
            uf = max(lr.error_units(s[i], sums[i], A[i]) for i in range(7))
            uc, ur, up = (lr.error_units(a, b, t) for a, b, t in zip(gg, g, T))
            if dtype == torch.float64:
                assert max(uf, uc, ur, up) <= 1e-6, (name, uf, uc, ur, up)
            else:
                print("head %-10s composition fwd %.2f  grad cls %.2f reg %.2f ref %.2f" % (name, uf, uc, ur, up))
                wf, wg = max(wf, uf), max(wg, uc, ur, up)
    wb = ws = 0.0
    for name, c in cc.decode_cases().items():
        for rot in (True, False):
            r = cr.decode_ref(c["reg"], c["cls"], c["ref"], 12, rot)
            box, obj, sem, classes = cc.decode_composition(c, torch.float32, rot)
            assert torch.equal(classes, r["classes"]), name
            ub = lr.error_units(box, r["box7"], r["scale7"])
            us = max(lr.error_units(obj, r["obj"], torch.ones_like(r["obj"])),
                     lr.error_units(sem, r["sem"], torch.ones_like(r["sem"])))
            print("decode %-8s rot %d composition box %.2f score %.2f" % (name, rot, ub, us))
            wb, ws = max(wb, ub), max(ws, us)
    print("worst: fwd %.2f grad %.2f box %.2f score %.2f" % (wf, wg, wb, ws))
    assert cc.C_F_CA == _pow2_of_4x(wf)
    assert cc.C_G_CA == _pow2_of_4x(wg)
    assert cc.C_BOX_CA == _pow2_of_4x(wb)
    assert cc.C_SCORE_CA == _pow2_of_4x(ws)


def test_cases_hold_what_they_claim():
    cases = cc.head_cases()
    for R in cc.HEAD_ROWS:
        c = cases["R%d" % R][0]
        assert c["reg"].shape == (R, 30) and float(c["reg"][:, 0:6].abs().max()) <= 2.0
        assert torch.equal(c["reg"][:, 0:6], cc._q(c["reg"][:, 0:6])) and torch.equal(c["distance_t"], cc._q(c["distance_t"]))
    assert float(cases["nopos257"][0]["box_w"].abs().max()) == 0.0
    assert 0.4 < float((cases["objw0_513"][0]["obj_w"] == 0).float().mean()) < 0.8
    edge, hyper = cases["edges300"]
    beta = hyper[10]
    assert beta == cc.BETA_EDGE and math.log2(beta) == int(math.log2(beta))
    d = torch.exp(edge["reg"][:, 0:6]) - edge["distance_t"].clamp(min=0)
    pos = edge["box_w"] != 0
    assert int(((d.abs() == beta) & pos.unsqueeze(1)).sum()) >= 8            # rows exactly ON the branch point
    assert int(((d == 0) & pos.unsqueeze(1)).sum()) >= 12                    # ties
    assert int(((edge["distance_t"] < 0) & pos.unsqueeze(1)).sum()) >= 4     # clamped targets
    t = edge["distance_t"].clamp(min=0)
    vol = (t[:, 0:3] + t[:, 3:6]).prod(1)
    assert int(((vol == 0) & pos).sum()) >= 6                                # zero target volume = zero overlap
    dec = cc.decode_cases()
    assert sorted(v["reg"].shape[1] for k, v in dec.items() if k != "K1_rowE") == sorted(cc.DECODE_K)
    r = cr.decode_ref(dec["K256"]["reg"], dec["K256"]["cls"], dec["K256"]["ref"])
    yaw = r["box7"][..., 6]
    assert float(yaw.min()) == 0.0 and float(yaw.max()) > 2 * math.pi - 1e-3 and float(yaw.max()) < 2 * math.pi
    assert int((r["scale7"][..., 3:6] == 0).sum()) >= 8                      # sizes the 0.1 clamp replaces


# ---- configuration ---------------------------------------------------------------------------------------------
def test_votenet_cfg_equals_the_reference_config():
    import dataclasses
    import json

    from demf_amd.config import BackboneCfg, VoteNetCfg, votenet_head_kwargs
    from test_config_vs_reference import _assert_subset, _norm, _untag
    with open(os.path.join(GOLD, "ref_baseline_config.json")) as f:
        cfgs = json.load(f, object_hook=_untag)
    base, over = cfgs["_base_/models/votenet.py"]["model"], cfgs["baseline/votenet.py"]["model"]

    def merge(a, b):                                     # mmcv Config: a child dict updates its base key by key
        out = dict(a)
        for k, v in b.items():
            out[k] = merge(a[k], v) if isinstance(v, dict) and isinstance(a.get(k), dict) else v
        return out

    model = merge(base, over)
    assert model["type"] == "VoteNet"
    ref = dict(model["bbox_head"])
    assert ref.pop("type") == "CAVoteHead"
    ref["train_cfg"], ref["test_cfg"] = model["train_cfg"], model["test_cfg"]   # VoteNet hands them to its head
    _assert_subset(votenet_head_kwargs(VoteNetCfg()), ref, "bbox_head", ref_only_ok=(
        "conv_cfg", "norm_cfg",                          # layer-type selectors: Conv1d / BN1d are built in
        "num_sizes", "mean_sizes",                       # the class-agnostic coder ignores them (coder :10-14)
        "center_loss"))                                  # CAVoteHead.loss has no centre term (:99-116)
    bb = dict(model["backbone"])
    assert bb.pop("type") == "PointNet2SASSG"
    sa = bb.pop("sa_cfg")
    assert bb.pop("norm_cfg") == dict(type="BN2d")
    ours = dataclasses.asdict(BackboneCfg())
    assert ours.pop("use_xyz") == sa["use_xyz"] and ours.pop("normalize_xyz") == sa["normalize_xyz"]
    assert _norm(ours) == _norm(bb)


def test_votenet_state_dict_keys_and_param_groups():
    from demf_amd.modules import VoteNet
    m = VoteNet()
    keys = list(m.state_dict())
    assert all(k.startswith(("backbone.", "bbox_head.vote_module.", "bbox_head.vote_aggregation.",
                             "bbox_head.conv_pred.")) for k in keys)
    assert m.bbox_head.conv_pred.conv_cls.weight.shape == (12, 128, 1)
    assert m.bbox_head.conv_pred.conv_reg.weight.shape == (30, 128, 1)
    assert [tuple(l.conv.weight.shape[:2]) for l in m.bbox_head.vote_aggregation.mlps[0]] == \
        [(128, 259), (128, 128), (128, 128)]
    groups = m.param_groups(lr=0.008)
    assert len(groups) == 1 and len(groups[0]["params"]) == len(list(m.parameters()))
    assert not hasattr(m, "extract_img_feat")
