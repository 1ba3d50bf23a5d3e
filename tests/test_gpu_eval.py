"""Indoor detection evaluation on the GPU (csrc/eval3d.hip, demf_amd/evaluation.py) against the float64
restatement of mmdet3d 0.18.1 indoor_eval (tests/eval_reference.py)."""
import math

import numpy as np
import pytest
import torch

import eval_reference as ref

pytestmark = pytest.mark.gpu

CATS = {i: f"c{i}" for i in range(10)}


def _iou(b1, b2):
    from demf_amd import ops
    return ops.box3d_overlaps(torch.from_numpy(np.ascontiguousarray(b1, np.float32)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(b2, np.float32)).cuda()).cpu().numpy()


def _random_boxes(rng, n, lo=-3.0, hi=3.0):
    b = np.empty((n, 7))
    b[:, 0:2] = rng.uniform(lo, hi, size=(n, 2))
    b[:, 2] = rng.uniform(-0.5, 0.5, size=n)
    b[:, 3:6] = rng.uniform(0.2, 2.5, size=(n, 3))
    b[:, 6] = rng.uniform(-math.pi, math.pi, size=n)
    return b


def _families(b, rng):
    """Adversarial partners of box b (bottom-centre form)."""
    x, y, z, dx, dy, dz, r = b
    c, s = math.cos(r), math.sin(r)
    ax = lambda u, v: (x + u * c + v * s, y - u * s + v * c)                          # noqa: E731 local -> world
    out = [b.copy()]                                                                 # identical
    out.append(np.array([x, y, z + 0.1 * dz, 0.5 * dx, 0.7 * dy, 0.5 * dz, r]))       # nested
    out.append(np.array([*ax(dx, 0), z, dx, dy, dz, r]))                             # shared edge
    out.append(np.array([*ax(0.4 * dx, 0), z, dx, dy, dz, r]))                       # collinear overlapping edges
    out.append(np.array([*ax(0.3 * dx, 0.5 * dy), z, 0.6 * dx, dy, dz, r]))          # collinear edge, half inside
    out.append(np.array([x, y, z, dx, dy, dz, r + math.pi]))                         # yaw + pi
    out.append(np.array([x, y, z, dy, dx, dz, r + math.pi / 2]))                     # yaw + pi/2, dx <-> dy
    out.append(np.array([x, y, z, 0.0, dy, dz, r]))                                  # zero size
    out.append(np.array([x, y, z + dz, dx, dy, dz, r]))                              # touching in z
    out.append(np.array([x + rng.normal(0, 0.2), y + rng.normal(0, 0.2), z, dx, dy, dz, r + rng.normal(0, 0.3)]))
    return out


def _pairs_case(seed=0, N=4096, M=64, far=True):
    rng = np.random.default_rng(seed)
    b2 = _random_boxes(rng, M)
    b1 = _random_boxes(rng, N)
    if far:                                                                 # half the boxes: centres around 1e2 m
        b2[M // 2:, 0:2] += rng.uniform(95.0, 105.0, size=(M - M // 2, 2))
        b1[N // 2:, 0:2] += b2[M // 2:, 0:2].mean(0)
    fam = []
    for j in range(M):
        for f in _families(b2[j], rng):
            fam.append(f)
    b1[:len(fam)] = np.asarray(fam)
    return b1.astype(np.float32), b2.astype(np.float32), len(_families(b2[0], rng))


def test_box3d_overlaps_vs_float64_restatement():
    b1, b2, nf = _pairs_case()
    got = _iou(b1, b2)
    want = ref.iou_matrix(b1.astype(np.float64), b2.astype(np.float64))
    assert got.shape == (4096, 64)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    fam = got[np.arange(64 * nf), np.repeat(np.arange(64), nf)].reshape(64, nf)
    np.testing.assert_allclose(fam[:, 0], 1.0, atol=1e-6)           # identical
    np.testing.assert_allclose(fam[:, 5], 1.0, atol=1e-5)           # yaw + pi
    np.testing.assert_allclose(fam[:, 6], 1.0, atol=1e-5)           # yaw + pi/2, sizes swapped
    assert np.all(fam[:, 7] == 0)                                   # zero size
    assert np.all(fam[:, 8] < 1e-6)                                 # touching in z (up to fp32 rounding of z + dz)
    assert (want > 0.25).sum() > 500                                # the case has real overlaps


def test_box3d_overlaps_invariances():
    rng = np.random.default_rng(3)
    b1, b2, _ = _pairs_case(seed=3, N=1024, M=64, far=False)   # (fp32 rounding of rotated far centres)
    base = _iou(b1, b2)
    for phi in (0.7, -2.1, math.pi):
        c, s = math.cos(phi), math.sin(phi)
        rot = []
        for b in (b1, b2):
            r = b.astype(np.float64).copy()
            x, y = r[:, 0].copy(), r[:, 1].copy()
            r[:, 0], r[:, 1] = x * c + y * s, -x * s + y * c               # geometry.rotation_3d_in_axis_z
            r[:, 6] += phi
            rot.append(r.astype(np.float32))
        np.testing.assert_allclose(_iou(*rot), base, rtol=0, atol=1e-5)
    np.testing.assert_allclose(_iou(b2, b1), base.T, rtol=0, atol=1e-5)
    same = _iou(b2, b2)
    ok = (b2[:, 3] * b2[:, 4] * b2[:, 5]) > 0
    np.testing.assert_allclose(np.diag(same)[ok], 1.0, atol=1e-6)
    shift = rng.uniform(-1, 1, size=3).astype(np.float32)
    moved = [b.copy() for b in (b1, b2)]
    for m in moved:
        m[:, :3] += shift
    np.testing.assert_allclose(_iou(*moved), base, rtol=0, atol=1e-5)


def test_box3d_overlaps_empty_and_shape_checks():
    from demf_amd import ops
    z = torch.zeros((0, 7), device="cuda")
    assert ops.box3d_overlaps(z, torch.zeros((3, 7), device="cuda")).shape == (0, 3)
    with pytest.raises(ValueError):
        ops.box3d_overlaps(torch.zeros((2, 6), device="cuda"), torch.zeros((3, 7), device="cuda"))


# ---- synthetic datasets -------------------------------------------------------------------------------
def _dataset(seed, scenes=300, classes=10, max_gt=30):
    rng = np.random.default_rng(seed)
    gt_annos, dt_annos = [], []
    for _ in range(scenes):
        n = int(rng.integers(0, max_gt + 1))
        g = _random_boxes(rng, n, -4, 4)
        g[:, 2] += g[:, 5] * 0.5                                          # gravity centre
        gl = rng.integers(0, classes, size=n)
        gt_annos.append({"gt_num": n, "gt_boxes_upright_depth": g.astype(np.float32), "class": gl})
        boxes, labels = [], []
        for i in range(n):
            bottom = g[i].copy()
            bottom[2] -= bottom[5] * 0.5
            for _k in range(int(rng.choice([0, 1, 1, 1, 2, 3]))):            # misses, hits, duplicates
                j = bottom.copy()
                j[:3] += rng.normal(0, 0.15, size=3) * bottom[3:6]
                j[3:6] *= rng.uniform(0.8, 1.2, size=3)
                j[6] += rng.normal(0, 0.2)
                boxes.append(j)
                labels.append(gl[i] if rng.random() > 0.1 else rng.integers(0, classes))
        fp = _random_boxes(rng, int(rng.integers(0, 6)), -4, 4)
        boxes.extend(fp)
        labels.extend(rng.integers(0, classes, size=len(fp)))
        dt_annos.append({"boxes_3d": np.asarray(boxes, np.float32).reshape(-1, 7),
                         "labels_3d": np.asarray(labels, np.int64)})
    P = sum(len(d["labels_3d"]) for d in dt_annos)
    scores = (rng.permutation(P) + 1).astype(np.float32) / np.float32(P + 1)       # distinct
    o = 0
    for d in dt_annos:
        d["scores_3d"] = scores[o:o + len(d["labels_3d"])]
        o += len(d["labels_3d"])
    return gt_annos, dt_annos


def _to_torch(dt_annos):
    from demf_amd.geometry import DepthBoxes
    return [dict(boxes_3d=DepthBoxes(torch.from_numpy(d["boxes_3d"])), scores_3d=torch.from_numpy(d["scores_3d"]),
                 labels_3d=torch.from_numpy(d["labels_3d"])) for d in dt_annos]


def _compare(got, want, tol=1e-9):
    assert set(got) == set(want)
    for k, v in want.items():
        if math.isnan(v):
            assert math.isnan(got[k]), k
        else:
            assert abs(got[k] - v) <= tol, (k, got[k], v)


def test_indoor_eval_vs_restatement_on_gpu_iou():
    """(a) the restatement reads the GPU's own IoU: TP flags equal, AP / rec to 1e-9."""
    from demf_amd import evaluation
    gt, dt = _dataset(11)
    want, want_tp, _ = ref.indoor_eval_ref(gt, dt, (0.25, 0.5), CATS, iou_fn=_iou)
    r = evaluation.evaluate_detections(gt, _to_torch(dt), (0.25, 0.5), CATS, with_tp=True)
    np.testing.assert_array_equal(r["tp"], want_tp)
    assert want_tp[:, 0].sum() > 1000 and want_tp[:, 1].sum() > 300
    _compare(evaluation.indoor_eval(gt, _to_torch(dt), (0.25, 0.5), CATS), want)


@pytest.mark.parametrize("metric", [(0.25,), (0.5,), (0.5, 0.25), (0.125, 0.75, 0.25, 0.5)])
def test_indoor_eval_threshold_count_and_order(metric):
    """One threshold, descending thresholds and four unordered ones (exact in fp32) against the restatement on
    the GPU's IoU: every threshold's TP positions must be complete before the AP pass reads them."""
    from demf_amd import evaluation
    gt, dt = _dataset(13, scenes=200)
    want, want_tp, _ = ref.indoor_eval_ref(gt, dt, metric, CATS, iou_fn=_iou)
    r = evaluation.evaluate_detections(gt, _to_torch(dt), metric, CATS, with_tp=True)
    np.testing.assert_array_equal(r["tp"], want_tp)
    assert want_tp.sum(0).min() > 10                  # (24 TPs at 0.75 in this set)
    for _ in range(3):                             # repeated: an ordering fault would show as a varying AP
        _compare(evaluation.indoor_eval(gt, _to_torch(dt), metric, CATS), want)


def test_indoor_eval_vs_float64_restatement():
    """(b) fp64 IoU on both sides of a threshold by more than 1e-4 (and unambiguous best GT)."""
    from demf_amd import evaluation
    metric = (0.25, 0.5)
    gt, dt = _dataset(12, scenes=200)
    for g, d in zip(gt, dt):                       # drop detections whose fp64 IoU sits near a decision
        if g["gt_num"] == 0 or len(d["labels_3d"]) == 0:
            continue
        gb = g["gt_boxes_upright_depth"].astype(np.float64).copy()
        gb[:, 2] -= gb[:, 5] * 0.5
        iou = ref.iou_matrix(d["boxes_3d"].astype(np.float64), gb)
        same = d["labels_3d"][:, None] == np.asarray(g["class"])[None, :]
        iou = np.where(same, iou, -1.0)
        near = np.zeros(len(iou), bool)
        for t in metric:
            near |= (np.abs(iou - t) < 1e-4).any(1)
        srt = np.sort(iou, 1)
        if iou.shape[1] > 1:
            near |= (srt[:, -1] - srt[:, -2] < 1e-4) & (srt[:, -1] > 0)
        keep = ~near
        for k in ("boxes_3d", "labels_3d", "scores_3d"):
            d[k] = d[k][keep]
    want, want_tp, _ = ref.indoor_eval_ref(gt, dt, metric, CATS)
    r = evaluation.evaluate_detections(gt, _to_torch(dt), metric, CATS, with_tp=True)
    np.testing.assert_array_equal(r["tp"], want_tp)
    _compare(evaluation.indoor_eval(gt, _to_torch(dt), metric, CATS), want)


# ---- edge cases, hand-computed -------------------------------------------------------------------------
def _box(x, y=0.0, z=0.0, dx=1.0, dy=1.0, dz=1.0, r=0.0):
    return [x, y, z, dx, dy, dz, r]


def _gt(boxes, classes):
    """bottom-centre boxes -> an annos dict (gravity centre)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 7).copy()
    b[:, 2] += b[:, 5] * 0.5
    return {"gt_num": len(classes), "gt_boxes_upright_depth": b, "class": np.asarray(classes, np.int64)}


def _dt(boxes, scores, labels):
    return {"boxes_3d": np.asarray(boxes, np.float32).reshape(-1, 7), "scores_3d": np.asarray(scores, np.float32),
            "labels_3d": np.asarray(labels, np.int64)}


def _run(gt, dt, metric=(0.25, 0.5)):
    from demf_amd import evaluation
    r = evaluation.evaluate_detections(gt, _to_torch(dt), metric, CATS, with_tp=True)
    out = evaluation.indoor_eval(gt, _to_torch(dt), metric, CATS)
    want, want_tp, _ = ref.indoor_eval_ref(gt, dt, metric, CATS, iou_fn=_iou)
    np.testing.assert_array_equal(r["tp"], want_tp)
    _compare(out, want)
    return out, r["tp"]


def test_scene_without_gt_and_class_without_detections():
    gt = [{"gt_num": 0, "gt_boxes_upright_depth": np.zeros((0, 7), np.float32), "class": np.zeros(0, np.int64)},
          _gt([_box(0), _box(5)], [0, 1])]
    dt = [_dt([_box(0)], [0.9], [0]), _dt([_box(0)], [0.8], [0])]
    out, tp = _run(gt, dt)
    assert tp[:, 0].tolist() == [0, 1]                      # scene 0 has no GT: its detection is FP
    assert out["c0_AP_0.25"] == pytest.approx(0.5, abs=1e-12) and out["c0_rec_0.25"] == 1.0
    assert out["c1_AP_0.25"] == 0.0 and out["c1_rec_0.50"] == 0.0        # GT, no detection
    assert out["mAP_0.25"] == pytest.approx(0.25, abs=1e-12) and out["mAR_0.50"] == pytest.approx(0.5)


def test_class_with_detections_but_no_gt_is_nan():
    gt = [_gt([_box(0)], [0])]
    dt = [_dt([_box(0), _box(3)], [0.9, 0.8], [0, 2])]
    out, _ = _run(gt, dt)
    assert out["c0_AP_0.50"] == 1.0
    assert math.isnan(out["c2_AP_0.25"]) and math.isnan(out["c2_rec_0.25"])
    assert math.isnan(out["mAP_0.25"]) and math.isnan(out["mAR_0.50"])


def test_no_detections_at_all():
    gt = [_gt([_box(0)], [0]), _gt([_box(1), _box(4)], [3, 3])]
    out, tp = _run(gt, [_dt([], [], []), _dt([], [], [])])
    assert tp.shape == (0, 2)
    assert out["c0_AP_0.25"] == 0.0 and out["c3_AP_0.50"] == 0.0 and out["mAP_0.25"] == 0.0
    assert out["mAR_0.25"] == 0.0 and set(out) == {f"{k}_{t}" for t in ("0.25", "0.50")
                                                   for k in ("c0_AP", "c3_AP", "mAP", "c0_rec", "c3_rec", "mAR")}


def test_two_detections_on_one_gt():
    gt = [_gt([_box(0)], [0])]
    out, tp = _run(gt, [_dt([_box(0), _box(0.05)], [0.9, 0.8], [0, 0])])
    assert tp.tolist() == [[1, 1], [0, 0]]
    assert out["c0_AP_0.25"] == 1.0 and out["c0_rec_0.50"] == 1.0


def test_best_gt_taken_is_fp_even_with_second_gt_above_threshold():
    # det 2: IoU 0.818 with GT A (taken by det 1), 0.667 with GT B: FP, no fall-back
    gt = [_gt([_box(0), _box(0.3)], [0, 0])]
    out, tp = _run(gt, [_dt([_box(0), _box(0.1)], [0.9, 0.8], [0, 0])])
    assert tp.tolist() == [[1, 1], [0, 0]]
    assert out["c0_AP_0.50"] == pytest.approx(0.5, abs=1e-12) and out["c0_rec_0.50"] == 0.5


def test_iou_exactly_half_is_not_above_threshold():
    gt = [_gt([_box(0, dx=2.0)], [0])]
    dt = [_dt([_box(0.25)], [0.9], [0])]
    assert _iou(dt[0]["boxes_3d"], [_box(0, dx=2.0)])[0, 0] == 0.5
    out, tp = _run(gt, dt)
    assert tp.tolist() == [[1, 0]]
    assert out["c0_AP_0.25"] == 1.0 and out["c0_AP_0.50"] == 0.0


def test_tied_scores_follow_scene_then_position():
    # equal scores: scene 0 (FP) before scene 1 (TP) -> prec 1/2 at the TP; in a scene, position 0 takes the GT
    gt = [_gt([_box(9)], [0]), _gt([_box(0)], [0])]
    out, tp = _run(gt, [_dt([_box(0)], [0.5], [0]), _dt([_box(0), _box(0)], [0.5, 0.5], [0, 0])])
    assert tp[:, 0].tolist() == [0, 1, 0]
    assert out["c0_AP_0.25"] == pytest.approx(0.25, abs=1e-12)           # (1/2) / npos 2


def test_segment_above_supported_size_raises():
    from demf_amd import evaluation
    many = [_box(0.01 * i) for i in range(257)]
    with pytest.raises(RuntimeError, match="at most 4096 and 256"):
        evaluation.indoor_eval([_gt(many, [0] * 257)], _to_torch([_dt([_box(0)], [0.9], [0])]), (0.25,), CATS)
    with pytest.raises(RuntimeError, match="at most 4096"):
        evaluation.indoor_eval([_gt([_box(0)], [0])],
                               _to_torch([_dt([_box(0)] * 4097, np.linspace(0, 1, 4097), [0] * 4097)]), (0.25,), CATS)
    with pytest.raises(ValueError, match="label2cat"):
        evaluation.indoor_eval([_gt([_box(0)], [0])], _to_torch([_dt([_box(0)], [0.9], [12])]), (0.25,), CATS)


def test_end_to_end_from_get_bboxes():
    from demf_amd import evaluation
    from demf_amd.modules import DeMFHotPath
    from demf_amd.modules.detector import bbox3d2result
    from oracle import fixtures
    pts, dec = fixtures.make_decode_results(7, B=4, K=256, N=20000)
    head = DeMFHotPath(fixtures.tiny_cfg()).pts_bbox_head.cuda().eval()
    preds = dict(decode_res_all=[{k: torch.from_numpy(v).cuda() for k, v in d.items()} for d in dec])
    res = head.get_bboxes(torch.from_numpy(pts).cuda(), preds, [dict() for _ in range(len(pts))])
    dt = [bbox3d2result(b, s, l) for b, s, l in res]
    rng = np.random.default_rng(7)
    gt = []
    for d in dt:                                       # ground truth: some surviving boxes, jittered
        b = d["boxes_3d"].tensor.numpy()
        pick = rng.choice(len(b), size=min(len(b), 6), replace=False) if len(b) else np.zeros(0, int)
        g = b[pick].astype(np.float64)
        g[:, :3] += rng.normal(0, 0.05, size=(len(g), 3))
        g[:, 2] += g[:, 5] * 0.5
        gt.append({"gt_num": len(g), "gt_boxes_upright_depth": g.astype(np.float32),
                   "class": d["labels_3d"].numpy()[pick]})
    assert sum(len(d["labels_3d"]) for d in dt) > 100
    got = evaluation.evaluate_detections(gt, dt, (0.25, 0.5), CATS, with_tp=True)
    want, want_tp, _ = ref.indoor_eval_ref(gt, dt, (0.25, 0.5), CATS, iou_fn=_iou)
    np.testing.assert_array_equal(got["tp"], want_tp)
    assert want_tp.sum() > 0
    _compare(evaluation.indoor_eval(gt, dt, (0.25, 0.5), CATS), want)


@pytest.mark.parametrize("pair", [((8, 10), (512, 10)), ((64, 2), (64, 10))])
def test_launch_count_does_not_depend_on_scenes_or_classes(monkeypatch, pair):
    from demf_amd import _ffi, evaluation
    real = _ffi.call
    counts = []
    for scenes, classes in pair:
        gt, dt = _dataset(20 + scenes + classes, scenes=scenes, classes=classes, max_gt=8)
        n = [0]

        def counting(*a, _n=n):
            _n[0] += 1
            return real(*a)
        monkeypatch.setattr(_ffi, "call", counting)
        evaluation.indoor_eval(gt, _to_torch(dt), (0.25, 0.5), CATS)
        monkeypatch.setattr(_ffi, "call", real)
        counts.append(n[0])
    assert counts[0] == counts[1] == 2
