"""``tta.merge_views`` / ``ops.tta_merge`` (csrc/tta.hip: demf_tta_merge) against the fp64 merge of
tests/tta_reference.py: the mapping back, the per-class NMS across views, the tie-ordered cut and the store protocol.

Box bound: 8 fp32 ulp of max(1, largest |coordinate| of the box) - at most four chained fp32 operations per
coordinate (subtract, divide, two products and a sum of the turn) plus cosf / sinf / atan2f, doubled."""
import itertools

import numpy as np
import pytest
import torch

import tta_cases
import tta_reference as tref

pytestmark = pytest.mark.gpu


class _Head:
    """What ``merge_views`` reads of a vote head."""

    def __init__(self, K, C, per_class=True, nms_thr=0.25):
        self.K, self.C = K, C
        self.test_cfg = dict(nms_thr=nms_thr, per_class_proposal=per_class)

    def packed_shape(self):
        return self.K, self.C, self.test_cfg["per_class_proposal"]


def _params(flip=False, scale=1.0, angle=0.0, trans=(0.0, 0.0, 0.0)):
    return dict(flip=flip, angle=angle, scale=scale, trans=np.asarray(trans, np.float64))


def _store_from(scenes, max_scenes=None):
    """Scenes [(boxes (n,7), scores (n,), labels (n,))] -> a DetectionStore holding them as ``detect_pack`` would."""
    from demf_amd.detections import DetectionStore
    n = sum(len(s[1]) for s in scenes)
    st = DetectionStore(max_scenes or len(scenes), max_rows=max(n, 1))
    off = np.cumsum([0] + [len(s[1]) for s in scenes]).astype(np.int32)
    if n:
        st.boxes[:n] = torch.from_numpy(np.concatenate([np.asarray(s[0], np.float32).reshape(-1, 7) for s in scenes]))
        st.scores[:n] = torch.from_numpy(np.concatenate([np.asarray(s[1], np.float32) for s in scenes]))
        st.labels[:n] = torch.from_numpy(np.concatenate([np.asarray(s[2], np.int32) for s in scenes]))
    st.scene_off[:len(off)] = torch.from_numpy(off)
    st.state[0] = n
    st._scenes = len(scenes)
    return st


def _rows_dev(params, B):
    from demf_amd.tta import param_rows
    return torch.from_numpy(param_rows(params, B)).cuda()


def _case(seed, B, V, K, C, thr, mode="bev", half=4.0, per_class=True, empty=(), params=None, fill=1.0):
    """A batch of views from margin-filtered segments.  Per (scene, class) a filtered case of about ``fill * V * K``
    boxes (exactly V * K at fill 1) is dealt round-robin to the views and pushed through ``apply_aug_params`` with
    the view's parameters.  -> (view scenes view-major [(boxes fp32, scores, labels)], params)."""
    from demf_amd.pipeline import apply_aug_params
    params = params or [_params(flip=bool(v & 1), scale=(1.0, 0.9, 2.0, 0.5)[(v >> 1) % 4]) for v in range(V)]
    scenes = [[None] * B for _ in range(V)]
    for b in range(B):
        per_view = [([], [], []) for _ in range(V)]
        for c in range(C):
            n = 0 if b in empty else (V * K if fill == 1.0 else int(fill * V * K) - (b + c) % 3)
            boxes, scores, _ = tta_cases.filtered(seed * 1000 + b * 50 + c, n, thr, mode, half)
            for v in range(V):
                per_view[v][0].append(apply_aug_params(boxes[v::V], dict(), params[v])[0])
                per_view[v][1].append(scores[v::V])
                per_view[v][2].append(np.full(len(scores[v::V]), c, np.int32))
        for v in range(V):
            bx, sc, lb = (np.concatenate(x) for x in per_view[v])
            if not per_class and len(sc):                  # any order of the classes inside a view scene
                perm = np.random.default_rng([seed, b, v]).permutation(len(sc))
                bx, sc, lb = bx[perm], sc[perm], lb[perm]
            scenes[v][b] = (bx.reshape(-1, 7), sc, lb)
    return [s for view in scenes for s in view], params


def _want(view_scenes, params, B, C, thr, mode, max_num):
    V = len(params)
    return [tref.merge([view_scenes[v * B + b] for v in range(V)], params, C, thr, mode, max_num) for b in range(B)]


def _assert_scene(got, want, what=""):
    gb, gs, gl = got["boxes_3d"].tensor.numpy(), got["scores_3d"].numpy(), got["labels_3d"].numpy()
    wb, ws, wl, _ = want
    assert gl.tolist() == wl.tolist(), what
    assert gs.dtype == np.float32 and np.array_equal(gs.view(np.int32), np.asarray(ws, np.float32).view(np.int32)), what
    if len(wl):
        tol = 8 * np.spacing(np.maximum(1.0, np.abs(wb).max(1)).astype(np.float32)).astype(np.float64)
        err = np.abs(gb.astype(np.float64) - wb).max(1)
        print(f"{what}: {len(wl)} rows, largest box error {np.max(err / (tol / 8)):.2f} ulp (bound 8)")
        assert (err <= tol).all(), (what, float(np.max(err / (tol / 8))))


def _merge(view_scenes, params, B, head, tta=None, out=None, first_view=0, view_store=None):
    from demf_amd.detections import DetectionStore
    from demf_amd.tta import merge_views
    vs = view_store if view_store is not None else _store_from(view_scenes)
    out = out if out is not None else DetectionStore(B)
    merge_views(vs, _rows_dev(params, B), out, first_view, B, head, tta)
    return out


# ---- 1. mapping back ----------------------------------------------------------------------------------------
def test_mapping_back_of_every_parameter_combination():
    """24 views = flip x scale {0.5, 0.9, 2.0} x angle {0, 0.3} x translation; thr = 1.0: nothing is suppressed, so
    every row comes back and must be the fp64 mapping back of its view's fp32 box."""
    from demf_amd.tta import TTACfg
    combos = list(itertools.product((False, True), (0.5, 0.9, 2.0), (0.0, 0.3), ((0.0, 0.0, 0.0), (0.7, -1.3, 0.2))))
    params = [_params(f, s, a, t) for f, s, a, t in combos]
    B, V, K, C = 2, len(params), 20, 3
    views, _ = _case(2, B, V, K, C, 1.0, half=40.0, params=params)       # (sparse: a quick reference)
    head = _Head(K, C, nms_thr=1.0)
    got = _merge(views, params, B, head).results()
    want = _want(views, params, B, C, 1.0, "bev", K * C)
    for b in range(B):
        assert len(want[b][2]) == K * C               # the default max_num = K * C cuts the V * K * C rows
        _assert_scene(got[b], want[b], f"scene {b}")
    # without the cut every row is there
    every = _merge(views, params, B, head, TTACfg(max_num=V * K * C)).results()
    for b, w in enumerate(_want(views, params, B, C, 1.0, "bev", None)):
        assert len(w[2]) == V * K * C
        _assert_scene(every[b], w, f"scene {b}, all rows")


# ---- 2. duplicates ------------------------------------------------------------------------------------------
def test_a_flipped_and_doubled_copy_of_view_0_changes_nothing():
    from demf_amd.pipeline import apply_aug_params
    B, K, C, thr = 2, 64, 4, 0.25
    p1 = _params(flip=True, scale=2.0)
    v0, v1, want = [], [], []
    for b in range(B):
        bx, sc, lb, rows = [], [], [], []
        for c in range(C):
            boxes, scores, ious = tta_cases.filtered(300 + b * 10 + c, K, thr, "bev")
            keep = tref.nms(boxes, scores, thr, "bev", ious=ious)
            rows += [(-float(scores[i]), c, i, boxes[i], scores[i]) for i in np.nonzero(keep)[0]]
            bx.append(boxes), sc.append(scores), lb.append(np.full(K, c, np.int32))
        bx, sc, lb = np.concatenate(bx), np.concatenate(sc), np.concatenate(lb)
        v0.append((bx, sc, lb))
        v1.append((apply_aug_params(bx, dict(), p1)[0], sc * np.float32(0.5), lb))
        rows.sort(key=lambda r: r[:3])
        want.append(rows)
    got = _merge(v0 + v1, [_params(), p1], B, _Head(K, C, nms_thr=thr)).results()
    for b in range(B):
        assert got[b]["labels_3d"].tolist() == [r[1] for r in want[b]]
        assert np.array_equal(got[b]["scores_3d"].numpy(), np.asarray([r[4] for r in want[b]], np.float32))
        assert np.array_equal(got[b]["boxes_3d"].tensor.numpy(), np.stack([r[3] for r in want[b]]))   # bit for bit
        assert 10 < len(want[b]) < K * C


# ---- 3. against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,K,C,half", [(1, 2, 20, 1, 4.0), (3, 2, 64, 10, 4.0), (2, 4, 64, 10, 4.0),
                                          (2, 4, 256, 10, 32.0)])
def test_merge_against_the_reference(B, V, K, C, half):
    """(2,4,256,10): every segment holds the limit of 1024 rows, a scene 10 240 candidates (in a 32 m half-width scene,
    so that the Python reference clips thousands of pairs, not hundreds of thousands)."""
    thr = 0.25
    empty = (1,) if B == 3 else ()                 # a scene without survivors between two with some
    views, params = _case(7, B, V, K, C, thr, half=half, empty=empty)
    head = _Head(K, C, nms_thr=thr)
    out = _merge(views, params, B, head)
    want = _want(views, params, B, C, thr, "bev", K * C)
    off, rows = out.host_index()
    assert np.diff(off).tolist() == [len(w[2]) for w in want] and rows == off[-1]
    assert out.state.tolist() == [rows, 0]
    got = out.results()
    for b in range(B):
        _assert_scene(got[b], want[b], f"({B},{V},{K},{C}) scene {b}")
        assert (len(want[b][2]) == 0) == (b in empty)
    assert sum(len(w[2]) for w in want) >= 10 * C


@pytest.mark.parametrize("mode", ["aligned", "3d"])
def test_the_other_overlap_modes(mode):
    from demf_amd.tta import TTACfg
    B, V, K, C, thr = 2, 2, 64, 3, 0.5
    views, params = _case(9, B, V, K, C, thr, mode)
    got = _merge(views, params, B, _Head(K, C), TTACfg(nms_thr=thr, mode=mode)).results()
    for b, w in enumerate(_want(views, params, B, C, thr, mode, K * C)):
        _assert_scene(got[b], w, f"{mode} scene {b}")
        assert 10 < len(w[2]) < V * K * C


def test_max_num_cuts_inside_a_run_of_tied_scores():
    """Every segment's scores are the same V * K values (one linspace, permuted), so each score appears in all C
    classes: the order inside a run is (class, view, row) and a cut inside it must take that prefix."""
    from demf_amd.tta import TTACfg
    B, V, K, C, thr = 2, 2, 32, 6, 0.25
    views, params = _case(13, B, V, K, C, thr)
    full = _want(views, params, B, C, thr, "bev", None)
    for b in range(B):
        assert len(np.unique(full[b][1])) < len(full[b][1]) / 2          # runs of tied scores
    cuts = [k for k in range(1, len(full[0][1])) if full[0][1][k] == full[0][1][k - 1]]
    for max_num in (cuts[0], cuts[len(cuts) // 2], 1):
        got = _merge(views, params, B, _Head(K, C, nms_thr=thr), TTACfg(max_num=max_num)).results()
        for b, w in enumerate(_want(views, params, B, C, thr, "bev", max_num)):
            assert len(w[2]) == max_num
            _assert_scene(got[b], w, f"max_num {max_num} scene {b}")


def test_without_per_class_proposal():
    """Rows of a view scene in any class order, at most K of them: the ranges are found from the labels; the
    default max_num is K."""
    B, V, K, C, thr = 2, 2, 60, 5, 0.25
    views, params = _case(17, B, V, K // C, C, thr, per_class=False)       # K / C rows per class: K per view scene
    head = _Head(K, C, per_class=False, nms_thr=thr)
    got = _merge(views, params, B, head).results()
    for b, w in enumerate(_want(views, params, B, C, thr, "bev", K)):
        _assert_scene(got[b], w, f"scene {b}")
        assert 10 < len(w[2]) <= K


# ---- 4. store protocol --------------------------------------------------------------------------------------
def test_two_batches_of_different_size_append_to_one_store():
    from demf_amd.detections import DetectionStore
    V, K, C, thr = 2, 32, 4, 0.25
    head = _Head(K, C, nms_thr=thr)
    out = DetectionStore(5)
    want = []
    for seed, B in ((21, 3), (22, 2)):
        views, params = _case(seed, B, V, K, C, thr, fill=0.8)
        assert _merge(views, params, B, head, out=out) is out
        want += _want(views, params, B, C, thr, "bev", K * C)
    assert len(out) == 5 and out.max_rows == 5 * K * C
    off, rows = out.host_index()
    assert np.diff(off).tolist() == [len(w[2]) for w in want] and out.state.tolist() == [rows, 0]
    for b, (g, w) in enumerate(zip(out.results(), want)):
        _assert_scene(g, w, f"scene {b}")
    # views that start behind other scenes of the view store
    views, params = _case(22, 2, V, K, C, thr, fill=0.8)
    pad = [(np.zeros((3, 7), np.float32), np.ones(3, np.float32), np.zeros(3, np.int32))]
    shifted = _merge(None, params, 2, head, first_view=1, view_store=_store_from(pad + views)).results()
    for b in range(2):
        _assert_scene(shifted[b], want[3 + b], f"shifted scene {b}")
    with pytest.raises(RuntimeError, match="5 of at most 5 scenes"):
        _merge(views, params, 2, head, out=out)
    with pytest.raises(ValueError, match="are not there"):
        _merge(None, params, 2, head, first_view=2, view_store=_store_from(pad + views))


def test_overflow_is_detected_and_nothing_is_written_behind_the_capacity():
    from demf_amd.detections import DetectionStore
    B, V, K, C, thr = 3, 2, 32, 4, 0.25
    views, params = _case(23, B, V, K, C, thr)
    head = _Head(K, C, nms_thr=thr)
    free = _merge(views, params, B, head)
    off, total = free.host_index()
    cap, guard = int(off[1] + (off[2] - off[1]) // 2), 64          # the capacity ends inside the second scene
    assert off[1] < cap < off[2] < total
    store = DetectionStore(B, max_rows=cap + guard)
    big = (store.boxes, store.scores, store.labels)
    for t in big:
        t.fill_(-7)
    store.boxes, store.scores, store.labels = big[0][:cap], big[1][:cap], big[2][:cap]
    store.max_rows = cap
    _merge(views, params, B, head, out=store)
    torch.cuda.synchronize()
    for t in big:
        assert bool((t[cap:] == -7).all()), "canary behind the capacity overwritten"
    assert torch.equal(big[0][:cap], free.boxes[:cap]) and torch.equal(big[1][:cap], free.scores[:cap])
    assert torch.equal(big[2][:cap], free.labels[:cap])
    assert store.state.tolist() == [total, 1] and store.scene_off[:B + 1].tolist() == off.tolist()
    with pytest.raises(RuntimeError, match=rf"{total} rows are needed, the capacity is {cap} rows"):
        store.results()
    # a view scene with more than K rows of a class cannot be merged: the overflow word says so
    small = _merge(views, params, B, _Head(K // 2, C, nms_thr=thr))
    assert small.state.tolist()[1] == 1


def test_more_than_1024_rows_per_class_raise_without_launching(monkeypatch):
    from demf_amd import _ffi, ops
    from demf_amd.detections import DetectionStore
    views, params = _case(24, 1, 4, 4, 2, 0.25)
    vs, out = _store_from(views), DetectionStore(1, max_rows=16)
    real, names = _ffi.call, []

    def recording(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_ffi, "call", recording)
    with pytest.raises(ValueError, match=r"V \* K <= 1024"):
        _merge(None, params, 1, _Head(257, 2), view_store=vs, out=out)            # V * K = 1028
    assert names == [] and len(out) == 0
    arrays = (vs.boxes, vs.scores, vs.labels, vs.scene_off, vs.state, _rows_dev(params, 1))
    dst = (out.boxes, out.scores, out.labels, out.scene_off, out.state)
    with pytest.raises(RuntimeError, match=r"V \* K = 1028 rows per class \(at most 1024\)"):
        ops.tta_merge(*arrays, 0, 1, 4, 2, 257, 0.25, "bev", 16, 0, *dst)
    with pytest.raises(RuntimeError, match=r"V \* K \* C = 17408 candidates per scene \(at most 16384\)"):
        ops.tta_merge(*arrays, 0, 1, 4, 17, 256, 0.25, "bev", 16, 0, *dst)
    assert names == ["demf_tta_merge"] * 2                   # refused by the entry point: nothing was launched
    torch.cuda.synchronize()
    assert out.state.tolist() == [0, 0] and out.scene_off.tolist() == [0, 0]


# ---- 5. capture, launch count -------------------------------------------------------------------------------
def test_capture_replays_on_fresh_view_store_contents():
    from demf_amd.detections import DetectionStore
    from demf_amd.tta import merge_views
    B, V, K, C, thr = 2, 4, 64, 10, 0.25
    head = _Head(K, C, nms_thr=thr)
    first, params = _case(31, B, V, K, C, thr, fill=0.9)
    fresh, _ = _case(32, B, V, K, C, thr, fill=0.7)
    static = _store_from(first)
    static_rows = _rows_dev(params, B)
    out = DetectionStore(B, max_rows=B * K * C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        merge_views(static, static_rows, out, 0, B, head)                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    before = [r["scores_3d"].clone() for r in out.results()]
    out.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        merge_views(static, static_rows, out, 0, B, head)
    assert len(out) == B
    src = _store_from(fresh)
    n = src.max_rows
    assert n <= static.max_rows
    static.boxes[:n].copy_(src.boxes), static.scores[:n].copy_(src.scores), static.labels[:n].copy_(src.labels)
    static.scene_off.copy_(src.scene_off), static.state.copy_(src.state)
    g.replay()
    torch.cuda.synchronize()
    got, eager = out.results(), _merge(fresh, params, B, head).results()
    for a, b in zip(got, eager):
        assert torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)
        assert torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["labels_3d"], b["labels_3d"])
    assert sum(len(r["labels_3d"]) for r in got) > 100
    assert any(a["scores_3d"].shape != f.shape or not torch.equal(a["scores_3d"], f) for a, f in zip(got, before))


def test_ffi_call_count_does_not_depend_on_batch_or_views(monkeypatch):
    from demf_amd import _ffi
    real = _ffi.call
    counts = []
    for B, V in ((2, 2), (8, 4)):
        views, params = _case(40 + B, B, V, 16, 3, 0.25)
        vs, rows = _store_from(views), _rows_dev(params, B)
        names = []

        def recording(name, *a, _n=names):
            _n.append(name)
            return real(name, *a)
        monkeypatch.setattr(_ffi, "call", recording)
        from demf_amd.detections import DetectionStore
        from demf_amd.tta import merge_views
        out = merge_views(vs, rows, DetectionStore(B), 0, B, _Head(16, 3))
        monkeypatch.setattr(_ffi, "call", real)
        counts.append(names)
        assert out.host_index()[1] > 0
    assert counts[0] == counts[1] == ["demf_tta_merge"]


# ---- 6. evaluation ------------------------------------------------------------------------------------------
def test_evaluation_from_the_merged_store_equals_evaluation_from_its_results():
    from demf_amd import evaluation
    from test_gpu_detections import CATS, _gt_from
    B, V, K, C, thr = 3, 2, 64, 10, 0.25
    views, params = _case(51, B, V, K, C, thr)
    store = _merge(views, params, B, _Head(K, C, nms_thr=thr))
    dt = store.results()
    gt = _gt_from(dt, 51)
    a, b = evaluation.indoor_eval(gt, store, (0.25, 0.5), CATS), evaluation.indoor_eval(gt, dt, (0.25, 0.5), CATS)
    assert set(a) == set(b) and "mAP_0.25" in a
    for k, v in a.items():
        assert v == b[k] or (np.isnan(v) and np.isnan(b[k])), (k, v, b[k])
    assert max(v for k, v in a.items() if "_AP_" in k and not np.isnan(v)) > 0
