"""Test-time augmentation through the loader, the detectors and the test runner: the tiny detector of
tests/test_gpu_detections.py on the dataset of pipeline_reference.write_dataset, four views (scales 1.0 and 0.9, each
unflipped and flipped)."""
import json
import os

import numpy as np
import pytest
import torch

import pipeline_reference as pref
import tta_reference as tref

pytestmark = pytest.mark.gpu

NUM_POINTS, SEED = 2048, 1


def _cfg():
    from demf_amd.tta import TTACfg
    return TTACfg(scales=(1.0, 0.9), flip=True)


def _dataset(tmp_path):
    from demf_amd.dataset import SUNRGBDDataset
    from test_gpu_pipeline import SPECS
    ann, _ = pref.write_dataset(str(tmp_path), SPECS, jpeg=True)
    return SUNRGBDDataset(str(tmp_path), ann, test_mode=True), ann


def _kw():
    from test_gpu_pipeline import IMG_SCALE
    return dict(num_points=NUM_POINTS, img_scale=IMG_SCALE, seed=SEED)


def _same_meta(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        if isinstance(v, dict):
            _same_meta(v, b[k])
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k
        else:
            assert v == b[k], k


def test_loader_views(tmp_path):
    from demf_amd import ops
    from demf_amd import pipeline as pl
    from demf_amd.tta import param_rows, view_params
    ds, _ = _dataset(tmp_path)
    cfg = _cfg()
    V, B = cfg.num_views, 4
    plain_loader = pl.SceneLoader(ds, B, "test", workers=4, **_kw())
    plain = next(iter(plain_loader))
    loader = pl.SceneLoader(ds, B, "test", workers=4, tta=cfg, **_kw())
    batch = next(iter(loader))
    assert isinstance(batch["points"], list) and len(batch["points"]) == V == len(batch["img_metas"]) == 4
    assert isinstance(batch["img"], torch.Tensor) and torch.equal(batch["img"], plain["img"])
    # view 0 is the single-view batch, bit for bit
    assert torch.equal(batch["points"][0], plain["points"])
    for m, n in zip(batch["img_metas"][0], plain["img_metas"]):
        _same_meta(m, n)
    # records and image bytes travel once: only the other views' parameter rows and sample keys are added
    assert loader.last_upload_bytes == plain_loader.last_upload_bytes + (V - 1) * B * (8 * 4 + 8)
    # the metas are augment_3d's own for the view's parameters; view_params is the device array of the rows
    vp = view_params(cfg)
    assert torch.equal(batch["view_params"].cpu(), torch.from_numpy(param_rows(vp, B)))
    for v in range(V):
        for m in batch["img_metas"][v]:
            assert m["pcd_horizontal_flip"] == vp[v]["flip"] and m["pcd_scale_factor"] == vp[v]["scale"]
            assert m["transformation_3d_flow"] == ["HF", "R", "S", "T"] and m["flip"] is False
            assert m["batch_input_shape"] == tuple(batch["img"].shape[-2:])
    # every view's points are points_prep alone with that view's rows and keys (drawn after the existing draw)
    pipe = loader.pipeline
    scenes = [pipe.load(i) for i in range(B)]
    raw = torch.from_numpy(np.concatenate([s["raw"] for s in scenes])).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s["raw"]) for s in scenes])]).astype(np.int64)).cuda()
    floor = ops.points_floor(raw, off)
    for v in range(V):
        keys = []
        for i in range(B):
            rng = pipe.scene_rng(i)
            draws = [int(rng.integers(0, 2 ** 63 - 1)) for _ in range(V)]
            keys.append(draws[v])
        alone = ops.points_prep(raw, off, floor, torch.from_numpy(param_rows([vp[v]], B)).cuda(),
                                torch.tensor(keys, dtype=torch.int64).cuda(), NUM_POINTS)
        assert torch.equal(batch["points"][v], alone), v
    assert not torch.equal(batch["points"][1][..., 1:3], batch["points"][0][..., 1:3])      # another sample
    # wait() reaches the tensors inside the lists
    assert batch.wait() is batch


def _numpy_merge(view_store, rows, B, head, tta=None):
    K, C, per_class = head.packed_shape()
    off, n = view_store.host_index()
    bx, sc, lb = (t[:n].cpu().numpy() for t in (view_store.boxes, view_store.scores, view_store.labels))
    rows = rows.cpu().numpy()
    V = len(rows) // B
    out = []
    for b in range(B):
        views = [(bx[off[s]:off[s + 1]], sc[off[s]:off[s + 1]], lb[off[s]:off[s + 1]])
                 for s in (v * B + b for v in range(V))]
        out.append(tref.merge(views, [tref.params_of_row(rows[v * B + b]) for v in range(V)], C,
                              head.test_cfg["nms_thr"], "bev", K * C if per_class else K))
    return out


def _knife_edge_pairs(view_store, rows, B, head, margin=1e-4):
    """The model's boxes are what they are and cannot be filtered before the GPU runs: count the same-class pairs
    of a scene whose fp64 IoU lies within ``margin`` of the threshold, for the message of a failed comparison (a
    pair much closer than that, about 1e-6, is where fp32 and fp64 may decide differently)."""
    K, C, _ = head.packed_shape()
    off, n = view_store.host_index()
    bx, lb = view_store.boxes[:n].cpu().numpy(), view_store.labels[:n].cpu().numpy()
    rows = rows.cpu().numpy()
    V = len(rows) // B
    thr = head.test_cfg["nms_thr"]
    count = 0
    for b in range(B):
        back, lab = [], []
        for v in range(V):
            s = v * B + b
            back.append(tref.map_back(bx[off[s]:off[s + 1]], tref.params_of_row(rows[s])))
            lab.append(lb[off[s]:off[s + 1]])
        back, lab = np.concatenate(back), np.concatenate(lab)
        for c in range(C):
            ious = tref.iou_matrix(back[lab == c], "bev")
            count += int((np.abs(ious - thr) < margin).sum()) // 2
    return count


def test_aug_predict_into_and_forward_test(tmp_path, monkeypatch):
    from demf_amd import pipeline as pl
    from demf_amd.detections import DetectionStore
    from test_gpu_detections import _assert_same_run, _detector
    ds, _ = _dataset(tmp_path)
    cfg = _cfg()
    V, B = cfg.num_views, 4
    det = _detector().cuda().eval()
    head = det.pts_bbox_head
    batch = next(iter(pl.SceneLoader(ds, B, "test", workers=4, tta=cfg, **_kw())))
    plain = next(iter(pl.SceneLoader(ds, B, "test", workers=4, **_kw())))
    calls = [0]
    real = det.extract_img_feat

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(det, "extract_img_feat", counting)
    store, view_store = DetectionStore(B), DetectionStore(V * B)
    assert det.aug_predict_into(store, **batch, tta=cfg, view_store=view_store) is view_store
    assert calls[0] == 1 and len(store) == B and len(view_store) == V * B
    # the merged store is the numpy merge of that same view store
    got = store.results()
    want = _numpy_merge(view_store, batch["view_params"], B, head)
    edge = f"{_knife_edge_pairs(view_store, batch['view_params'], B, head)} same-class pairs within 1e-4 of nms_thr"
    print("rows per view scene:", np.diff(view_store.host_index()[0]).tolist(), "merged:",
          [len(g["labels_3d"]) for g in got], edge)
    assert sum(len(g["labels_3d"]) for g in got) > 0
    for b in range(B):
        gb, gs, gl = got[b]["boxes_3d"].tensor.numpy(), got[b]["scores_3d"].numpy(), got[b]["labels_3d"].numpy()
        wb, ws, wl, _ = want[b]
        assert gl.tolist() == wl.tolist() and np.array_equal(gs, np.asarray(ws, np.float32)), edge
        if len(wl):
            tol = 8 * np.spacing(np.maximum(1.0, np.abs(wb).max(1)).astype(np.float32)).astype(np.float64)
            assert (np.abs(gb - wb).max(1) <= tol).all()
    # view 0's scenes are the plain batch's detections (another forward: the bar of two runs)
    single = DetectionStore(B)
    det.predict_into(single, **plain)
    assert calls[0] == 2
    off, n = view_store.host_index()
    view0 = [dict(labels_3d=view_store.labels[off[b]:off[b + 1]].cpu().to(torch.int64),
                  scores_3d=view_store.scores[off[b]:off[b + 1]].cpu()) for b in range(B)]
    _assert_same_run(view0, single.results())
    # the metas' rows are the loader's: without view_params the result is the same merge
    calls[0] = 0
    again = det.aug_test(batch["points"], batch["img_metas"], batch["img"], tta=cfg)
    assert calls[0] == 1
    _assert_same_run(again, got)
    # forward_test dispatches lists of four to aug_test
    ft = det.forward_test(batch["points"], batch["img_metas"], [batch["img"]] * V)
    _assert_same_run(ft, got)
    assert calls[0] == 2
    # refusals: a flipped image, views of different size
    flipped = [[dict(m) for m in metas] for metas in batch["img_metas"]]
    flipped[1][0]["flip"] = True
    with pytest.raises(ValueError, match="image is flipped"):
        det.aug_predict_into(DetectionStore(B), batch["points"], flipped, batch["img"])
    with pytest.raises(ValueError, match="num of augmentations"):
        det.forward_test(batch["points"], batch["img_metas"][:2], [batch["img"]] * V)
    assert calls[0] == 2


def test_votenet_aug_test_on_points_alone(tmp_path):
    from demf_amd import pipeline as pl
    from demf_amd.detections import DetectionStore
    from test_gpu_detections import _assert_same_run
    from test_gpu_votenet_run import _model
    ds, _ = _dataset(tmp_path)
    cfg = _cfg()
    V, B = cfg.num_views, 4
    model = _model().cuda().eval()
    batch = next(iter(pl.SceneLoader(ds, B, "test", workers=4, with_img=False, tta=cfg, **_kw())))
    assert "img" not in batch and len(batch["points"]) == V
    store, view_store = DetectionStore(B), DetectionStore(V * B)
    model.aug_predict_into(store, **batch, tta=cfg, view_store=view_store)
    got = store.results()
    want = _numpy_merge(view_store, batch["view_params"], B, model.bbox_head)
    print("votenet rows per view scene:", np.diff(view_store.host_index()[0]).tolist(),
          "merged:", [len(g["labels_3d"]) for g in got])
    edge = f"{_knife_edge_pairs(view_store, batch['view_params'], B, model.bbox_head)} pairs within 1e-4 of nms_thr"
    for b in range(B):
        assert got[b]["labels_3d"].tolist() == want[b][2].tolist(), edge
        assert np.array_equal(got[b]["scores_3d"].numpy(), np.asarray(want[b][1], np.float32)), edge
    _assert_same_run(model.aug_test(batch["points"], batch["img_metas"]), got)
    _assert_same_run(model.forward_test(batch["points"], batch["img_metas"]), got)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_run_test_with_tta(tmp_path, batch_size, capsys):
    from demf_amd import infer
    from demf_amd import pipeline as pl
    from demf_amd.modules import DeMFVoteNet
    from test_gpu_detections import _assert_same_run, _detector
    from test_gpu_detector import STREAM, _cfg256
    ds, ann = _dataset(tmp_path)
    cfg = _cfg()
    det = _detector().cuda()
    store = infer.run_test(det, ds, batch_size=batch_size, workers=4, tta=cfg, **_kw())
    assert not det.training and len(store) == len(ds) == 4
    res = store.results()
    loop = []
    for batch in pl.SceneLoader(ds, batch_size, "test", workers=4, tta=cfg, **_kw()):
        loop += det.aug_test(batch["points"], batch["img_metas"], batch["img"], tta=cfg)
    _assert_same_run(res, loop)
    assert sum(len(r["labels_3d"]) for r in res) > 0
    # the command line
    root = str(tmp_path)
    path = os.path.join(root, "mmcv.pth")
    torch.save(dict(state_dict={k: v.cpu() for k, v in det.state_dict().items()}), path)
    capsys.readouterr()
    ret = infer.main(["--data-root", root, "--ann-file", os.path.basename(ann), "--checkpoint", path, "--batch-size",
                      str(batch_size), "--workers", "4", "--tta-scales", "1.0,0.9", "--tta-flip"],
                     model=DeMFVoteNet(_cfg256(), **STREAM), **_kw())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    printed = json.loads(lines[-1])
    assert "mAP_0.25" in printed and "mAP_0.50" in printed and set(printed) == set(ret) == set(ds.evaluate(store))
