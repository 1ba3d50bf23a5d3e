"""Indoor detection evaluation without a GPU: the new C entries are exported, bound and validate their
arguments before any launch; ops.box3d_overlaps has no CPU path; the fp64 restatement the GPU tests check
against (tests/eval_reference.py) agrees with hand-computed values."""
import math

import numpy as np
import pytest

from demf_amd import _ffi

import eval_reference as ref

NEW = ("demf_box3d_iou", "demf_eval_match", "demf_eval_ap")


def test_new_entries_are_exported_and_bound():
    lib = _ffi.load()
    for name in NEW:
        assert name in _ffi.SIGNATURES
        assert hasattr(lib, name)


def test_bad_arguments_are_reported_not_launched():
    import ctypes
    thr = (ctypes.c_float * 2)(0.25, 0.5)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_box3d_iou", -1, 4, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_box3d_iou", 2, 3, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_eval_match", 4, 5, thr, 8, 8, *([None] * 7))
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_eval_match", 4, 2, thr, 8, 8, *([None] * 7))
    with pytest.raises(RuntimeError, match=r"code -3\).*at most 4096 and 256"):
        _ffi.call("demf_eval_match", 4, 2, thr, 8, 257, *([None] * 7))
    with pytest.raises(RuntimeError, match="at most 4096"):
        _ffi.call("demf_eval_match", 4, 2, thr, 4097, 3, *([None] * 7))
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_eval_ap", 3, 0, *([None] * 8))
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_eval_ap", 3, 2, *([None] * 8))
    assert b"null pointer" in _ffi.load().demf_last_error()


def test_box3d_overlaps_refuses_cpu_tensors():
    import torch
    from demf_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.box3d_overlaps(torch.zeros(2, 7), torch.zeros(3, 7))


def test_sunrgbd_classes():
    from demf_amd.config import SUNRGBD_CLASSES
    assert SUNRGBD_CLASSES == ('bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand',
                               'bookshelf', 'bathtub')


def test_reference_iou_square_vs_square_at_45_degrees():
    a = [0, 0, 0, 1, 1, 1, 0.0]
    b = [0, 0, 0, 1, 1, 1, math.pi / 4]
    assert ref.box3d_iou(a, b) == pytest.approx(math.sqrt(2) / 2, abs=1e-12)
    assert ref.box3d_iou(b, a) == pytest.approx(math.sqrt(2) / 2, abs=1e-12)


def test_reference_iou_half_height_shift():
    a = [1, 2, 0, 2, 3, 1, 0.3]
    b = [1, 2, 0.5, 2, 3, 1, 0.3]
    assert ref.box3d_iou(a, b) == pytest.approx(1 / 3, abs=1e-12)


def test_reference_iou_degenerate_cases():
    a = [0, 0, 0, 2, 1, 1, 0.0]
    assert ref.box3d_iou(a, a) == pytest.approx(1.0, abs=1e-12)
    assert ref.box3d_iou(a, [0, 0, 0, 2, 1, 1, math.pi]) == pytest.approx(1.0, abs=1e-12)
    assert ref.box3d_iou(a, [0, 0, 0, 1, 2, 1, math.pi / 2]) == pytest.approx(1.0, abs=1e-12)
    assert ref.box3d_iou(a, [2, 0, 0, 2, 1, 1, 0.0]) == 0.0                  # shared edge
    assert ref.box3d_iou(a, [0, 0, 0, 0, 1, 1, 0.0]) == 0.0                  # zero size
    assert ref.box3d_iou([0, 0, 0, 2, 1, 1, 0.0], [0, 0, 0, 1, 1, 1, 0.0]) == pytest.approx(0.5, abs=1e-12)
    assert ref.box3d_iou(a, [1, 0, 0, 2, 1, 1, 0.0]) == pytest.approx(1 / 3, abs=1e-12)   # collinear edges


def test_reference_ap_tp_fp_tp():
    rec = np.array([0.5, 0.5, 1.0])
    prec = np.array([1.0, 0.5, 2 / 3])
    assert ref.average_precision(rec, prec) == pytest.approx((1 + 2 / 3) / 2, abs=1e-15)


def test_reference_eval_tp_fp_tp():
    """Two GT of one class; detections in score order hit GT 0, GT 0 again (FP), GT 1."""
    g = np.array([[0, 0, 0.5, 1, 1, 1, 0], [5, 0, 0.5, 1, 1, 1, 0]], np.float32)
    d = np.array([[0, 0, 0, 1, 1, 1, 0], [0.05, 0, 0, 1, 1, 1, 0], [5, 0, 0, 1, 1, 1, 0]], np.float32)
    gt = [dict(gt_num=2, gt_boxes_upright_depth=g, **{"class": np.array([0, 0])})]
    dt = [dict(boxes_3d=d, scores_3d=np.array([0.9, 0.8, 0.7], np.float32), labels_3d=np.array([0, 0, 0]))]
    ret, tp, _ = ref.indoor_eval_ref(gt, dt, (0.25, 0.5), {0: "bed"})
    assert tp[:, 0].tolist() == [1, 0, 1]
    assert ret["bed_AP_0.25"] == pytest.approx((1 + 2 / 3) / 2, abs=1e-12)
    assert ret["bed_rec_0.50"] == 1.0
    assert ret["mAP_0.50"] == pytest.approx((1 + 2 / 3) / 2, abs=1e-12)
