"""Measure test-time augmentation (demf_amd/tta.py, csrc/tta.hip) on one GPU.

    python tools/bench_tta.py [--views 2 4 6] [--reps 20] [--out profiles/tta_bench.json]

At the reference size - K = 256 candidates per scene (two ensemble layers of 128 proposals), C = 10 classes, B = 8
scenes of 20 000 points and an 800 x 1120 image canvas - and V views (scale-major, unflipped then flipped) the tool
records, with device events around the work, after a warm-up, best and median of --reps repetitions:

merge   per launch of ``tta.merge_views`` (three kernels): the views' detections of a seeded-weights forward of the
        full-size ``DeMFVoteNet`` on a synthetic batch, merged into a fresh store, with the rows the views hold and
        the rows kept next to it.  ``merge_full_segments`` is the same launch at full occupancy: every (scene, class)
        segment holds V * K rows of clustered boxes (tests/tta_cases.py), the most work the limits admit.
batch   per batch: ``aug_predict_into`` (the image stream once, the head per view, the merge) next to V calls of
        ``predict_into`` on the same inputs (the image stream per view, no merge).  The difference is the image stream
        saved minus the merge.

V * K must not exceed 1024: a view count the merge refuses at K = 256 (V = 6) is recorded as refused and measured at
the largest K that fits instead.  The yardsticks printed next to the result are the single-view post-processing's
0.23 ms per batch and the image stream's 21 ms of a 25.5 ms test batch (README).  No accuracy
figure is measured here or anywhere: no SUN RGB-D data is on the test machines.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))          # tta_cases: the seeded clustered boxes

B, N_POINTS, C = 8, 20000, 10
IMG_HW, IMG_SCALE = (530, 730), (1333, 800)
YARDSTICKS = dict(single_view_postprocess_ms_per_batch=0.23, image_stream_ms_per_batch=21.0,
                  test_batch_ms=25.5, head_forward_ms_about=4.0)


def _say(text):
    print("[bench_tta] " + text, file=sys.stderr, flush=True)


def _events(fn, reps, before=None):
    import torch
    ms = []
    for i in range(reps + 3):                       # three warm-up rounds
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
    return dict(ms_best=round(min(ms), 4), ms_median=round(statistics.median(ms), 4), reps=reps)


def _model(num_proposal, seed=1):
    from bench_baseline import _seed_weights
    from demf_amd.config import DeMFCfg
    from demf_amd.modules import DeMFVoteNet
    cfg = DeMFCfg()
    if num_proposal != cfg.head.num_proposal:
        import dataclasses
        cfg = dataclasses.replace(cfg, head=dataclasses.replace(cfg.head, num_proposal=num_proposal))
    model = DeMFVoteNet(cfg)
    _seed_weights(model, seed)
    import torch
    with torch.no_grad():          # as the tests' tiny detector: boxes that hold points, distinct scores above score_thr
        for i, pred in enumerate(model.pts_bbox_head.conv_preds):
            pred.conv_reg.bias[3:6] = 0.8 + 0.1 * i
            pred.conv_reg.weight.mul_(4.0)
            pred.conv_cls.weight.mul_(8.0)
    return model.cuda().eval()


def _full_views(V, K, seed=0):
    """The merge's worst case by occupancy: a view store in which every (scene, class) holds K rows in every view -
    clustered boxes of tests/tta_cases.py (each object about four times, as the views of a scene see it), dealt
    round-robin to the views and pushed through ``apply_aug_params``.  -> (view store, parameter rows, TTACfg)."""
    import numpy as np
    import torch

    import tta_cases
    from demf_amd.detections import DetectionStore
    from demf_amd.pipeline import apply_aug_params
    from demf_amd.tta import TTACfg, param_rows, view_params
    tta = TTACfg(scales={2: (1.0,), 4: (1.0, 0.9), 6: (1.0, 0.9, 1.1)}[V], flip=True)
    vp = view_params(tta)
    scenes = []
    for v in range(V):
        for b in range(B):
            bx, sc, lb = [], [], []
            for c in range(C):
                boxes, scores = tta_cases.raw(seed + b * C + c, V * K)
                bx.append(apply_aug_params(boxes[v::V], dict(), vp[v])[0])
                sc.append(scores[v::V])
                lb.append(np.full(K, c, np.int32))
            scenes.append((np.concatenate(bx), np.concatenate(sc), np.concatenate(lb)))
    n = sum(len(s[1]) for s in scenes)
    st = DetectionStore(V * B, max_rows=n)
    st.boxes.copy_(torch.from_numpy(np.concatenate([s[0] for s in scenes])))
    st.scores.copy_(torch.from_numpy(np.concatenate([s[1] for s in scenes])))
    st.labels.copy_(torch.from_numpy(np.concatenate([s[2] for s in scenes])))
    st.scene_off.copy_(torch.from_numpy(np.cumsum([0] + [len(s[1]) for s in scenes]).astype(np.int32)))
    st.state[0] = n
    st._scenes = V * B
    return st, torch.from_numpy(param_rows(vp, B)).cuda(), tta


def _inputs(tta, seed=0):
    """A synthetic batch in V views: clouds in front of the camera, one random image, ``augment_3d``'s metas."""
    import numpy as np
    import torch

    from demf_amd import synthetic
    from demf_amd.data import resize_meta
    from demf_amd.pipeline import apply_aug_params
    from demf_amd.tta import param_rows, view_params
    rng = np.random.default_rng(seed)
    base = []
    for b in range(B):
        m = resize_meta(dict(sample_idx=b, depth2img=synthetic.depth2img(), flip=False), IMG_HW, IMG_SCALE, 32)
        m["pad_shape"] = tuple(m["batch_input_shape"]) + (3,)
        base.append(m)
    xyz = rng.uniform([-2.5, 1.0, -1.0], [2.5, 6.0, 1.5], size=(B, N_POINTS, 3)).astype(np.float32)
    pts = torch.from_numpy(np.concatenate([xyz, xyz[..., 2:3] + 1.0], -1)).cuda()
    vp = view_params(tta)
    points, metas = [], []
    for p in vp:
        v = pts.clone()
        if p["flip"]:
            v[..., 0] = -v[..., 0]
        v[..., :3] *= p["scale"]
        v[..., 3] *= p["scale"]
        points.append(v.contiguous())
        metas.append([apply_aug_params(np.zeros((0, 7), np.float32), m, p)[1] for m in base])
    img = torch.from_numpy(rng.standard_normal((B, 3) + tuple(base[0]["batch_input_shape"])).astype(np.float32)).cuda()
    return points, metas, img, torch.from_numpy(param_rows(vp, B)).cuda()


def measure(V, K, reps):
    import torch

    from demf_amd.detections import DetectionStore
    from demf_amd.tta import TTACfg, merge_views
    scales = {2: (1.0,), 4: (1.0, 0.9), 6: (1.0, 0.9, 1.1)}[V]
    tta = TTACfg(scales=scales, flip=True)
    model = _model(K // 2)
    head = model.pts_bbox_head
    assert head.packed_shape() == (K, C, True), head.packed_shape()
    points, metas, img, rows = _inputs(tta)
    view_store = DetectionStore(V * B, device=img.device)
    out = DetectionStore(B, device=img.device)
    model.aug_predict_into(out, points, metas, img, tta=tta, view_store=view_store, view_params=rows)
    off, n_view = view_store.host_index()
    kept = out.host_index()[1]
    res = dict(V=V, K=K, C=C, B=B, view_rows=int(n_view), merged_rows=int(kept),
               merged_rows_per_scene=[int(x) for x in (out.host_index()[0][1:] - out.host_index()[0][:-1])])
    res["merge"] = _events(lambda: merge_views(view_store, rows, out, 0, B, head, tta), reps, before=out.reset)
    _say(f"V = {V}, K = {K}: merge {res['merge']['ms_median']} ms for {n_view} view rows -> {kept} rows")
    full_store, full_rows, _ = _full_views(V, K)
    full_out = DetectionStore(B, device=img.device)
    merge_views(full_store, full_rows, full_out, 0, B, head, tta)
    res["merge_full_segments"] = dict(
        view_rows=int(full_store.host_index()[1]), merged_rows=int(full_out.host_index()[1]),
        **_events(lambda: merge_views(full_store, full_rows, full_out, 0, B, head, tta), reps, before=full_out.reset))
    _say(f"V = {V}, K = {K}: merge of full segments {res['merge_full_segments']['ms_median']} ms for "
         f"{res['merge_full_segments']['view_rows']} view rows -> {res['merge_full_segments']['merged_rows']} rows")
    res["aug_predict_into"] = _events(
        lambda: model.aug_predict_into(out, points, metas, img, tta=tta, view_store=view_store, view_params=rows),
        reps, before=out.reset)
    plain = DetectionStore(V * B, device=img.device)

    def per_view():
        for v in range(V):
            model.predict_into(plain, points[v], metas[v], img)
    res["predict_into_per_view"] = _events(per_view, reps, before=plain.reset)
    res["saved_ms_median"] = round(res["predict_into_per_view"]["ms_median"] - res["aug_predict_into"]["ms_median"], 4)
    _say(f"V = {V}, K = {K}: aug_predict_into {res['aug_predict_into']['ms_median']} ms, {V} x predict_into "
         f"{res['predict_into_per_view']['ms_median']} ms")
    del model
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--views", type=int, nargs="+", default=[2, 4, 6], choices=(2, 4, 6))
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    args = p.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "bench_tta needs a HIP device: a timing without one says nothing"
    from demf_amd import ops
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, yardsticks=YARDSTICKS,
                  limits=dict(V_times_K=ops.NMS_MAX_SEGMENT, V_times_K_times_C=ops.TTA_MAX_CANDIDATES),
                  accuracy="not measured: no SUN RGB-D data on the test machines", runs=[])
    for V in args.views:
        K = 256
        if V * K > ops.NMS_MAX_SEGMENT:
            fit = (ops.NMS_MAX_SEGMENT // V) // 2 * 2
            result["runs"].append(dict(V=V, K=K, refused=f"V * K = {V * K} exceeds {ops.NMS_MAX_SEGMENT}",
                                       measured_instead_at_K=fit))
            K = fit
        result["runs"].append(measure(V, K, args.reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
