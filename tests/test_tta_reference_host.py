"""Hand cases of the fp64 reference of the test-time augmentation merge (tests/tta_reference.py), the view order of
``tta.view_params`` and the refusals of ``TTACfg`` / ``infer.parse_args``.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import tta_cases
import tta_reference as tref


def _box(x=0.0, y=0.0, z=0.0, dx=2.0, dy=1.0, dz=1.0, yaw=0.0):
    return [x, y, z, dx, dy, dz, yaw]


@pytest.mark.parametrize("mode", tref.MODES)
def test_two_identical_boxes_keep_the_first(mode):
    b = np.array([_box(yaw=0.3), _box(yaw=0.3)])
    assert tref.iou(b[0], b[1], mode) == pytest.approx(1.0, abs=1e-12)
    assert tref.nms(b, np.array([0.5, 0.9]), 0.25, mode).tolist() == [False, True]
    assert tref.nms(b, np.array([0.7, 0.7]), 0.25, mode).tolist() == [True, False]      # tie: the lower row first


def test_iou_exactly_at_the_threshold_is_kept():
    # a half-width box inside a unit square: overlap 0.5 of areas 1 and 0.5, iou = 0.5 / (1 + 0.5 - 0.5) = 0.5 exactly
    a, b = _box(dx=1.0, dy=1.0), _box(x=0.25, dx=0.5, dy=1.0)
    assert tref.iou(a, b, "bev") == 0.5 and tref.iou(a, b, "aligned") == 0.5
    boxes, scores = np.array([a, b]), np.array([0.9, 0.8])
    for mode in ("bev", "aligned"):
        assert tref.nms(boxes, scores, 0.5, mode).tolist() == [True, True]               # `>` suppresses
        assert tref.nms(boxes, scores, np.nextafter(0.5, 0.0), mode).tolist() == [True, False]


def test_chain_where_the_middle_falls_and_the_end_survives():
    a, b, c = _box(x=0.0, dx=1.0), _box(x=0.5, dx=1.0), _box(x=1.0, dx=1.0)            # iou(a,b) = iou(b,c) = 1/3
    assert tref.iou(a, c, "bev") == 0.0
    keep = tref.nms(np.array([a, b, c]), np.array([0.9, 0.8, 0.7]), 0.3, "bev")
    assert keep.tolist() == [True, False, True]
    # with B first, both neighbours fall
    assert tref.nms(np.array([a, b, c]), np.array([0.8, 0.9, 0.7]), 0.3, "bev").tolist() == [False, True, False]


def test_yaw_plus_pi_and_quarter_turn_with_swapped_sizes_are_the_same_footprint():
    a = _box(x=0.3, y=-0.2, dx=1.7, dy=0.6, yaw=0.4)
    assert tref.iou(a, _box(x=0.3, y=-0.2, dx=1.7, dy=0.6, yaw=0.4 + math.pi), "bev") == pytest.approx(1.0, abs=1e-12)
    assert tref.iou(a, _box(x=0.3, y=-0.2, dx=0.6, dy=1.7, yaw=0.4 + math.pi / 2), "bev") == \
        pytest.approx(1.0, abs=1e-12)


def test_bev_merges_two_stacked_boxes_and_3d_does_not():
    boxes = np.array([_box(z=0.0, dz=1.0), _box(z=1.5, dz=1.0)])
    scores = np.array([0.9, 0.8])
    assert tref.nms(boxes, scores, 0.25, "bev").tolist() == [True, False]
    assert tref.nms(boxes, scores, 0.25, "3d").tolist() == [True, True]
    assert tref.iou(boxes[0], boxes[1], "3d") == 0.0


def test_aligned_mode_ignores_yaw():
    a, b = _box(dx=2.0, dy=0.5, yaw=0.0), _box(dx=2.0, dy=0.5, yaw=math.pi / 2)
    assert tref.iou(a, b, "aligned") == 1.0
    assert tref.iou(a, b, "bev") == pytest.approx(0.25 / 1.75, abs=1e-12)
    assert tref.nms(np.array([a, b]), np.array([0.9, 0.8]), 0.25, "aligned").tolist() == [True, False]
    assert tref.nms(np.array([a, b]), np.array([0.9, 0.8]), 0.25, "bev").tolist() == [True, True]


def test_degenerate_box_overlaps_nothing_and_invalid_rows_are_no_candidates():
    boxes = np.array([_box(), _box(dx=0.0), _box(x=0.1)])
    assert tref.iou(boxes[0], boxes[1], "bev") == 0.0
    keep = tref.nms(boxes, np.array([0.9, 0.8, np.nan]), 0.25, "bev")
    assert keep.tolist() == [True, True, False]
    assert tref.nms(boxes, np.array([0.9, 0.8, 0.7]), 0.25, "bev", valid=[0, 1, 1]).tolist() == [False, True, True]


def test_merge_tie_order_and_cut():
    # two classes, two views, all scores tied: order = class, then view, then row; the cut takes a prefix of it
    far = [_box(x=10.0 * k) for k in range(4)]
    ident = dict(flip=False, angle=0.0, scale=1.0, trans=np.zeros(3))
    views = [(np.array([far[0], far[1]]), np.full(2, 0.5, np.float32), np.array([1, 0])),
             (np.array([far[2], far[3]]), np.full(2, 0.5, np.float32), np.array([0, 1]))]
    boxes, scores, labels, src = tref.merge(views, [ident, ident], 2, 0.25)
    assert labels.tolist() == [0, 0, 1, 1] and src.tolist() == [[0, 1], [1, 0], [0, 0], [1, 1]]
    assert tref.merge(views, [ident, ident], 2, 0.25, max_num=3)[3].tolist() == [[0, 1], [1, 0], [0, 0]]
    # a higher score goes first whatever its class; inside the NMS the lower (view, row) wins a tie
    views[1][1][1] = 0.75
    assert tref.merge(views, [ident, ident], 2, 0.25)[3].tolist()[0] == [1, 1]
    dup = [(np.array([far[0]]), np.array([0.5], np.float32), np.array([0])) for _ in range(2)]
    assert tref.merge(dup, [ident, ident], 1, 0.25)[3].tolist() == [[0, 0]]


def test_nms_indices_are_in_score_order():
    b = np.array([[0, 0, 1, 1, 0.0], [5, 5, 6, 6, 0.3], [0.05, 0, 1.05, 1, 0.0]])
    assert tref.nms_indices(b, np.array([0.5, 0.9, 0.7]), 0.25).tolist() == [1, 2]
    assert tref.nms_indices(b, np.array([0.5, 0.9, 0.7]), 0.25, "aligned").tolist() == [1, 2]


@pytest.mark.parametrize("flip,scale,angle,trans", list(itertools.product(
    (False, True), (0.5, 0.9, 2.0), (0.0, 0.3, -1.1), ((0.0, 0.0, 0.0), (0.7, -1.3, 0.2)))))
def test_mapping_back_inverts_apply_aug_params(flip, scale, angle, trans):
    """``augment_3d`` itself in float64 (the package's ``apply_aug_params`` rounds to fp32 at the end), then the
    reference's mapping back: the input boxes to 1e-12."""
    from demf_amd.data import augment_3d
    from demf_amd.pipeline import _Replay, apply_aug_params
    params = dict(flip=flip, angle=angle, scale=scale, trans=np.asarray(trans))
    boxes, _ = tta_cases.raw(5, 40)
    boxes = boxes.astype(np.float64)
    b = boxes.copy()                                # augment_3d's box arithmetic, kept in float64
    if flip:
        b[:, 0] = -b[:, 0]
        b[:, 6] = -b[:, 6] + np.pi
    from demf_amd.data import rotation_z
    b[:, :3] = b[:, :3] @ rotation_z(angle).T
    b[:, 6] -= angle
    b[:, :6] *= scale
    b[:, :3] += np.asarray(trans)
    got32, meta = apply_aug_params(boxes, dict(), params)
    assert np.allclose(got32, b, rtol=1e-6, atol=1e-6)        # the float64 restatement IS apply_aug_params
    assert meta["pcd_horizontal_flip"] == flip and meta["pcd_scale_factor"] == scale
    assert np.abs(tref.map_back(b, params) - boxes).max() <= 1e-12
    # and from the fp32 boxes the package makes: fp32 rounding of the forward only
    assert np.abs(tref.map_back(got32, params) - boxes).max() <= 4e-6 * max(1.0, 1.0 / scale) * 8
    # the parameter row names the same transform
    from demf_amd.pipeline import param_row
    back = tref.params_of_row(param_row(params))
    assert back["flip"] == flip and back["angle"] == pytest.approx(angle, abs=1e-7)
    assert back["scale"] == pytest.approx(scale, rel=1e-7) and np.allclose(back["trans"], trans, atol=1e-7)
    assert augment_3d is not None and _Replay is not None


def test_view_params_order_and_identity_first_view():
    from demf_amd.pipeline import identity_aug_params
    from demf_amd.tta import TTACfg, param_rows, view_params
    vp = view_params(TTACfg(scales=(1.0, 0.9, 1.1), flip=True))
    assert [(p["scale"], p["flip"]) for p in vp] == [(1.0, False), (1.0, True), (0.9, False), (0.9, True),
                                                     (1.1, False), (1.1, True)]
    ident = identity_aug_params()
    assert set(vp[0]) == set(ident) and all(np.array_equal(vp[0][k], ident[k]) for k in ident)
    assert all(p["angle"] == 0.0 and not np.any(p["trans"]) for p in vp)
    assert [(p["scale"], p["flip"]) for p in view_params(TTACfg(scales=(0.9, 1.1), flip=False))] == \
        [(0.9, False), (1.1, False)]
    rows = param_rows(vp, 3)
    assert rows.shape == (18, 8) and rows.dtype == np.float32
    assert rows[:, 0].tolist() == [0.0] * 3 + [1.0] * 3 + [0.0] * 3 + [1.0] * 3 + [0.0] * 3 + [1.0] * 3
    assert np.array_equal(rows[:, 3], np.repeat(np.float32([1.0, 1.0, 0.9, 0.9, 1.1, 1.1]), 3))


def test_tta_cfg_refusals():
    from demf_amd.tta import TTACfg
    assert TTACfg(scales=(1.0,), flip=True).num_views == 2
    assert TTACfg(scales=[1.0, 0.9], flip=False).num_views == 2
    with pytest.raises(ValueError, match="at least two views"):
        TTACfg(scales=(1.0,), flip=False)
    for bad in ((1.0, 0.0), (-0.9, 1.0), (), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="scales must be positive"):
            TTACfg(scales=bad)
    with pytest.raises(ValueError, match="mode must be one of"):
        TTACfg(mode="rotated")
    with pytest.raises(ValueError, match="nms_thr"):
        TTACfg(nms_thr=1.5)
    with pytest.raises(ValueError, match="max_num"):
        TTACfg(max_num=0)
    TTACfg(scales=(1.0, 0.9), flip=True).check_limits(256, 10)           # V * K = 1024: the limit
    with pytest.raises(ValueError, match=r"V \* K <= 1024"):
        TTACfg(scales=(1.0, 0.9), flip=True).check_limits(257, 10)
    with pytest.raises(ValueError, match=r"V \* K \* C <= 16384"):
        TTACfg(scales=(1.0, 0.9), flip=True).check_limits(256, 17)


def test_pipeline_takes_tta_in_test_mode_only():
    from demf_amd.pipeline import ScenePipeline, SceneLoader
    from demf_amd.tta import TTACfg
    with pytest.raises(ValueError, match="mode='test'"):
        ScenePipeline(None, "train", tta=TTACfg())
    assert ScenePipeline(None, "test", tta=TTACfg()).tta.num_views == 2
    with pytest.raises(ValueError, match="the given pipeline brings its own"):
        SceneLoader([], 1, pipeline=ScenePipeline(None, "test"), tta=TTACfg(), device="cpu")


def test_parse_args_refusals(capsys):
    from demf_amd import infer
    base = ["--data-root", "r", "--ann-file", "a.pkl", "--checkpoint", "c.pth"]
    assert infer.parse_args(base).tta is None
    a = infer.parse_args(base + ["--tta-scales", "0.9,1.0,1.1", "--tta-flip", "--tta-mode", "3d", "--tta-nms-thr",
                                 "0.4", "--model", "votenet"])
    assert a.tta.scales == (0.9, 1.0, 1.1) and a.tta.flip and a.tta.mode == "3d" and a.tta.nms_thr == 0.4
    assert a.tta.num_views == 6
    assert infer.parse_args(base + ["--tta-flip"]).tta.num_views == 2
    assert infer.parse_args(base + ["--tta-scales", "1.0,0.9"]).tta.num_views == 2
    for bad in (["--tta-scales", "1.0"], ["--tta-scales", "1.0,0"], ["--tta-scales", "1.0,-0.9", "--tta-flip"],
                ["--tta-scales", "1.0,x"], ["--tta-mode", "3d"], ["--tta-nms-thr", "0.3"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + bad)
    capsys.readouterr()


def test_the_margin_filter_drops_few_boxes_and_leaves_no_knife_edge_pair():
    for n, thr in ((65, 0.25), (256, 0.25), (256, 0.5)):
        boxes, scores, ious = tta_cases.filtered(1, n, thr, "bev")
        assert boxes.shape == (n, 7) and boxes.dtype == np.float32 and len(np.unique(scores)) == n
        off = ious[~np.eye(n, dtype=bool)]
        assert not (np.abs(off - thr) < tta_cases.MARGIN).any()
        assert (off > thr).sum() > n                       # a clustered scene: the NMS has work to do
        keep = tref.nms(boxes, scores, thr, "bev", ious=ious)
        assert np.array_equal(keep, tref.nms(boxes, scores, thr, "bev"))      # the matrix is the row form's
        assert 0 < keep.sum() < n
