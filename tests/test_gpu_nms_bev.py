"""``ops.nms_bev`` (csrc/tta.hip: demf_nms_bev) against the fp64 reference (tests/tta_reference.py) on cases filtered
by decision margin before either side runs (tests/tta_cases.py): ``keep`` exactly equal."""
import numpy as np
import pytest
import torch

import tta_cases
import tta_reference as tref

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 256, 1024)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _run(boxes, scores, starts, counts, thr, mode, **kw):
    from demf_amd import ops
    keep = ops.nms_bev(_dev(boxes, np.float32).view(-1, 7), _dev(scores, np.float32), _dev(starts, np.int32),
                       _dev(counts, np.int32), thr, mode, **kw)
    assert keep.dtype == torch.uint8 and keep.shape == (len(scores),)
    return keep.cpu().numpy().astype(bool)


@pytest.mark.parametrize("thr", [0.25, 0.5])
@pytest.mark.parametrize("mode", tref.MODES)
def test_one_segment_of_every_size(mode, thr):
    """n = 63 / 64 / 65: the wave edge; 256 and 1024: several waves, 1024 the segment limit.  n_max = n picks the
    workgroup size, so every power of two from 64 to 1024 runs."""
    kept = {}
    for n in SIZES:
        boxes, scores, ious = tta_cases.filtered(11, n, thr, mode)
        want = tref.nms(boxes, scores, thr, mode, ious=ious)
        got = _run(boxes, scores, [0], [n], thr, mode, n_max=n)
        kept[n] = int(want.sum())
        assert np.array_equal(got, want), (n, np.nonzero(got != want)[0][:8])
        if n:                       # the default n_max = 1024: the same decisions from the largest workgroup
            assert np.array_equal(_run(boxes, scores, [0], [n], thr, mode), want), n
    print("kept per size:", kept)
    assert kept[1] == 1 and 1 <= kept[2] <= 2 and 20 < kept[1024] < 1000


@pytest.mark.parametrize("mode", tref.MODES)
def test_segments_of_different_sizes_in_one_call(mode):
    """Five segments behind a non-zero seg_start, an empty one between two full ones; rows before, between and
    behind the segments are in no segment and keep their zero."""
    thr, sizes = 0.25, (200, 0, 65, 1, 130)
    parts = [tta_cases.filtered(20 + k, n, thr, mode) for k, n in enumerate(sizes)]
    gap = 7
    starts, at = [], gap
    for n in sizes:
        starts.append(at)
        at += n + (gap if n == 65 else 0)
    R = at + gap
    boxes, scores = np.zeros((R, 7), np.float32), np.full(R, 2.0, np.float32)
    boxes[:, 3:6] = 1.0                                     # rows outside the segments: real boxes, top scores
    want = np.zeros(R, bool)
    for s, n, (b, sc, ious) in zip(starts, sizes, parts):
        boxes[s:s + n], scores[s:s + n] = b, sc
        want[s:s + n] = tref.nms(b, sc, thr, mode, ious=ious)
    got = _run(boxes, scores, starts, sizes, thr, mode, n_max=200)
    assert np.array_equal(got, want)
    assert want.sum() > 40 and not got[:gap].any() and not got[R - gap:].any()


def test_valid_mask_tied_scores_and_a_degenerate_box():
    thr = 0.25
    boxes, scores, ious = tta_cases.filtered(31, 256, thr, "bev")
    rng = np.random.default_rng(31)
    valid = rng.random(256) < 0.7
    want = tref.nms(boxes, scores, thr, "bev", valid=valid, ious=ious)
    assert np.array_equal(_run(boxes, scores, [0], [256], thr, "bev", valid=_dev(valid.astype(np.uint8))), want)
    assert np.array_equal(_run(boxes, scores, [0], [256], thr, "bev", valid=_dev(valid)), want)      # bool mask
    assert not want[~valid].any() and 0 < want.sum() < valid.sum()
    # ties: eight score levels over 256 boxes - the lower row goes first
    tied = (np.floor(scores * 8) / 8).astype(np.float32)
    want = tref.nms(boxes, tied, thr, "bev", ious=ious)
    assert np.array_equal(_run(boxes, tied, [0], [256], thr, "bev"), want)
    assert not np.array_equal(want, tref.nms(boxes, scores, thr, "bev", ious=ious))
    # NaN and -inf scores are no candidates
    odd = scores.copy()
    odd[5], odd[9] = np.nan, -np.inf
    assert np.array_equal(_run(boxes, odd, [0], [256], thr, "bev"), tref.nms(boxes, odd, thr, "bev", ious=ious))
    # a box with dx = 0 overlaps nothing: it is kept and removes nobody, though it lies inside box 1
    deg = np.array([[0, 0, 0, 0.0, 1, 1, 0.2], [0, 0, 0, 2, 2, 1, 0.0], [0.1, 0, 0, 2, 2, 1, 0.1]], np.float32)
    sc = np.array([0.9, 0.8, 0.7], np.float32)
    for mode in ("bev", "3d"):
        want = tref.nms(deg, sc, thr, mode)
        assert want.tolist() == [True, True, False]
        assert np.array_equal(_run(deg, sc, [0], [3], thr, mode), want)


def test_n_max_beyond_1024_raises_without_launching(monkeypatch):
    from demf_amd import _ffi, ops
    boxes, scores, _ = tta_cases.filtered(11, 65, 0.25, "bev")
    args = (_dev(boxes), _dev(scores), _dev([0], np.int32), _dev([65], np.int32), 0.25)
    real, names = _ffi.call, []

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_ffi, "call", recording)
    with pytest.raises(RuntimeError, match="n_max=1025 boxes per segment exceeds 1024"):
        ops.nms_bev(*args, n_max=1025)
    assert names == ["demf_nms_bev"]
    with pytest.raises(ValueError, match="mode must be one of"):
        ops.nms_bev(*args, mode="rotated")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.nms_bev(args[0].cpu(), *args[1:])
    assert names == ["demf_nms_bev"]


def test_a_segment_larger_than_n_max_sets_the_overflow_word_and_keeps_nothing():
    from demf_amd import ops
    thr = 0.25
    a, b = tta_cases.filtered(40, 65, thr, "bev"), tta_cases.filtered(41, 64, thr, "bev")
    boxes, scores = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (_dev(boxes), _dev(scores), _dev([0, 65], np.int32), _dev([65, 64], np.int32), thr, "bev")
    keep = ops.nms_bev(*args, n_max=64, overflow=flag).cpu().numpy().astype(bool)
    assert flag.item() == 1
    assert not keep[:65].any()
    assert np.array_equal(keep[65:], tref.nms(b[0], b[1], thr, "bev", ious=b[2]))
    # a segment that leaves the arrays is refused the same way; the other one is untouched by it
    flag.zero_()
    args = (_dev(boxes), _dev(scores), _dev([70, 0], np.int32), _dev([64, 65], np.int32), thr, "bev")
    keep = ops.nms_bev(*args, n_max=65, overflow=flag).cpu().numpy().astype(bool)
    assert flag.item() == 1 and not keep[65:].any()
    assert np.array_equal(keep[:65], tref.nms(a[0], a[1], thr, "bev", ious=a[2]))
    flag.zero_()
    ops.nms_bev(*args[:2], _dev([0, 65], np.int32), _dev([65, 64], np.int32), thr, "bev", n_max=65, overflow=flag)
    assert flag.item() == 0


def test_upstream_shaped_entries_on_200_boxes():
    from demf_amd import ops
    thr = 0.25
    for mode, fn in (("bev", ops.nms_gpu), ("aligned", ops.nms_normal_gpu)):
        b7, scores, _ = tta_cases.filtered(50, 200, thr, mode)
        xyxyr = np.stack([b7[:, 0] - b7[:, 3] / 2, b7[:, 1] - b7[:, 4] / 2, b7[:, 0] + b7[:, 3] / 2,
                          b7[:, 1] + b7[:, 4] / 2, b7[:, 6]], 1).astype(np.float32)
        # the corner form rounds once more: filter its own pairs by the margin, here, before the GPU runs
        back = np.zeros((200, 7))
        x = xyxyr.astype(np.float64)
        back[:, 0], back[:, 1] = (x[:, 0] + x[:, 2]) / 2, (x[:, 1] + x[:, 3]) / 2
        back[:, 3], back[:, 4], back[:, 5], back[:, 6] = x[:, 2] - x[:, 0], x[:, 3] - x[:, 1], 1.0, x[:, 4]
        ious = tref.iou_matrix(back, mode)
        assert not (np.abs(ious - thr) < tta_cases.MARGIN).any()
        want = tref.nms_indices(xyxyr, scores, thr, mode)
        got = fn(_dev(xyxyr), _dev(scores), thr)
        assert got.dtype == torch.int64 and got.is_cuda
        assert got.cpu().tolist() == want.tolist() and 10 < len(want) < 200
        if mode == "bev":
            top = np.argsort(-scores, kind="stable")[:50]             # pre_maxsize: the 50 best; indices stay global
            sub = top[tref.nms_indices(xyxyr[top], scores[top], thr, mode)]
            got = fn(_dev(xyxyr), _dev(scores), thr, pre_maxsize=50, post_max_size=5)
            assert got.cpu().tolist() == sub[:5].tolist() and len(sub) > 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.nms_gpu(torch.zeros(3, 5), torch.zeros(3), 0.25)
