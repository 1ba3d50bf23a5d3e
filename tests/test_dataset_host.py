"""SUN RGB-D infos reading and the host half of the scene pipeline, without a GPU: demf_amd/dataset.py against the
mmdet3d 0.18.1 infos layout, the per-scene random draws and box / metadata helper of demf_amd/pipeline.py against
data.augment_3d, the batch padding metadata, and argument checking of the new C entries and ops wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from demf_amd import _ffi, data, ops, synthetic
from demf_amd.dataset import SUNRGBDDataset, load_infos
from demf_amd.modules.head import compose_projection
from demf_amd import pipeline as pl

import pipeline_reference as ref

SPECS = [(3000, (53, 73), 3), (2500, (43, 56), 0), (4000, (44, 59), 5), (1200, (40, 40), 1)]


@pytest.fixture()
def dataset_dir(tmp_path):
    ann, scenes = ref.write_dataset(str(tmp_path), SPECS, jpeg=False)
    return tmp_path, ann, scenes


def test_infos_paths_calib_and_boxes(dataset_dir):
    root, ann, scenes = dataset_dir
    ds = SUNRGBDDataset(str(root), "sunrgbd_infos_train.pkl")
    assert len(ds) == 4 and len(load_infos(ann)) == 4
    for i, s in enumerate(scenes):
        info = ds.get_data_info(i)
        assert info["sample_idx"] == i + 1
        assert info["pts_filename"] == str(root / "points" / f"{i + 1:06d}.bin")
        assert info["img_filename"] == str(root / "sunrgbd_trainval" / "image" / f"{i + 1:06d}.png")
        assert info["depth2img"].dtype == np.float32
        np.testing.assert_allclose(info["depth2img"], ref.depth2img(s["K"].astype(np.float32),
                                                                    s["Rt"].astype(np.float32)), rtol=1e-6)
        a = ds.get_ann_info(i)
        assert a["gt_bboxes_3d"].dtype == np.float32 and a["gt_labels_3d"].dtype == np.int64
        if SPECS[i][2] == 0:
            assert a["gt_bboxes_3d"].shape == (0, 7) and a["gt_labels_3d"].shape == (0,)
            continue
        want = s["boxes"].copy()
        want[:, 2] = want[:, 2] + want[:, 5] * np.float32(-0.5)             # fp32, as DepthInstance3DBoxes does
        np.testing.assert_array_equal(a["gt_bboxes_3d"], want)
        np.testing.assert_allclose(a["gt_bboxes_3d"], ref.bottom_center(s["boxes"]), atol=1e-6)
        np.testing.assert_array_equal(a["gt_labels_3d"], s["labels"])
        assert info["ann_info"]["gt_bboxes_3d"].shape == (SPECS[i][2], 7)


def test_test_mode_and_filter_empty_gt(dataset_dir):
    root, ann, _ = dataset_dir
    assert len(SUNRGBDDataset(str(root), ann, filter_empty_gt=True)) == 3
    test = SUNRGBDDataset(str(root), ann, test_mode=True, filter_empty_gt=True)
    assert len(test) == 4 and "ann_info" not in test.get_data_info(0)


def test_infos_must_be_a_list(tmp_path):
    import pickle
    p = tmp_path / "bad.pkl"
    p.write_bytes(pickle.dumps({"a": 1}))
    with pytest.raises(ValueError, match="list"):
        load_infos(str(p))


def test_draws_and_box_meta_helper_equal_augment_3d():
    """draw_aug_params(default_rng(s)) + apply_aug_params == augment_3d(..., default_rng(s)), exactly, for 50 seeds;
    and the GPU parameter row carries the same transform."""
    pts = np.random.default_rng(0).uniform(-3, 3, size=(100, 4)).astype(np.float32)
    boxes = np.array([[0.2, 3.0, -0.5, 1.0, 0.8, 0.9, 0.3], [-1.0, 2.0, 0.1, 0.4, 1.9, 1.2, -1.1]], np.float32)
    base = data.resize_meta(dict(depth2img=np.eye(3, dtype=np.float32)), (530, 730), (1333, 800))
    flips = 0
    for s in range(50):
        apts, abox, ameta = data.augment_3d(pts, boxes, base, np.random.default_rng(s))
        p = pl.draw_aug_params(np.random.default_rng(s))
        bx, meta = pl.apply_aug_params(boxes, base, p)
        np.testing.assert_array_equal(bx, abox)
        assert set(meta) == set(ameta)
        for k in ameta:
            np.testing.assert_array_equal(np.asarray(meta[k]), np.asarray(ameta[k]), err_msg=k)
        flips += p["flip"]
        row = pl.param_row(p)
        x = np.where(row[0] != 0, -pts[:, 0].astype(np.float64), pts[:, 0])
        c, sn = np.float64(row[1]), np.float64(row[2])
        got = np.stack([(x * c - pts[:, 1] * sn) * row[3] + row[4], (x * sn + pts[:, 1] * c) * row[3] + row[5],
                        pts[:, 2] * np.float64(row[3]) + row[6]], 1)
        np.testing.assert_allclose(got, apts[:, :3], atol=2e-6)
    assert 10 < flips < 40


def test_test_mode_flow_is_the_identity():
    base = data.resize_meta(dict(depth2img=synthetic.depth2img()), (427, 561), (1333, 800))
    bx, meta = pl.apply_aug_params(np.zeros((0, 7), np.float32), base, pl.identity_aug_params())
    assert meta["transformation_3d_flow"] == ["HF", "R", "S", "T"] and meta["pcd_horizontal_flip"] is False
    np.testing.assert_array_equal(np.abs(meta["pcd_rotation"]), np.eye(3))
    assert meta["pcd_scale_factor"] == 1.0 and not np.any(meta["pcd_trans"])
    np.testing.assert_array_equal(pl.param_row(pl.identity_aug_params()), [0, 1, 0, 1, 0, 0, 0, 0])
    M, *ab = compose_projection(meta)
    M0, *ab0 = compose_projection(dict(base, transformation_3d_flow=[]))
    np.testing.assert_allclose(M, M0, rtol=0, atol=1e-9)
    assert ab == ab0


def test_scene_load_and_batch_input_shape(dataset_dir):
    """Host half of the loader: per-scene metadata from resize_meta, the batch's padded shape as every scene's
    batch_input_shape; train draws depend on (seed, epoch, index), test mode draws nothing."""
    root, ann, scenes = dataset_dir
    ds = SUNRGBDDataset(str(root), ann)
    p = pl.ScenePipeline(ds, "train", img_scale=(1333, 800), seed=3)
    loaded = [p.load(i) for i in range(len(ds))]
    for s, spec in zip(loaded, SPECS):
        assert s["raw"].shape == (spec[0], 6) and s["img"].shape == spec[1] + (3,)
        h, w = ref.rescale_shape(*spec[1], (1333, 800))
        assert s["meta"]["img_shape"] == (h, w, 3) and s["meta"]["ori_shape"] == spec[1] + (3,)
        assert s["meta"]["pad_shape"] == (-(-h // 32) * 32, -(-w // 32) * 32, 3)
    (Hp, Wp), metas = pl.collate_metas([s["meta"] for s in loaded])
    want = (max(-(-m["img_shape"][0] // 32) * 32 for m in metas), max(-(-m["img_shape"][1] // 32) * 32 for m in metas))
    assert (Hp, Wp) == want == (800, 1120)
    assert all(m["batch_input_shape"] == (Hp, Wp) for m in metas)
    assert [s["meta"]["pad_shape"][:2] for s in loaded] != [(Hp, Wp)] * len(loaded)
    # the draws are augment_3d's for the scene's generator
    again = p.load(2)
    assert again["seed"] == loaded[2]["seed"] and again["params"]["angle"] == loaded[2]["params"]["angle"]
    assert p.load(2, epoch=1)["seed"] != loaded[2]["seed"]
    w = pl.draw_aug_params(p.scene_rng(2))
    assert w["angle"] == loaded[2]["params"]["angle"] and w["flip"] == loaded[2]["params"]["flip"]
    t = pl.ScenePipeline(SUNRGBDDataset(str(root), ann, test_mode=True), "test", seed=3).load(0)
    assert t["params"]["angle"] == 0.0 and t["gt_labels_3d"] is None
    with pytest.raises(ValueError, match="mode"):
        pl.ScenePipeline(ds, "val")


def test_new_entries_report_bad_arguments():
    for name in ("demf_points_floor", "demf_points_prep", "demf_image_prep"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_points_floor", 2, 6, 0, None, None, None, None)             # no points at all
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_points_floor", 0, 6, 10, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_points_floor", 2, 6, 10, None, None, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_points_prep", 2, -5, 6, 10, *([None] * 8))
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_points_prep", 2, 20, 6, 10, *([None] * 8))
    ms = (ctypes.c_float * 6)(*ops.IMG_NORM[0], *ops.IMG_NORM[1])
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_image_prep", 2, 32, 30, 100, None, None, None, ms, None, None)     # Wp % 4 != 0
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_image_prep", 2, 32, 32, 100, None, None, None, ms, None, None)


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    raw, off = torch.zeros(10, 6), torch.tensor([0, 10])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.points_floor(raw, off)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.points_prep(raw, off, torch.zeros(1), torch.zeros(1, 8), torch.zeros(1, dtype=torch.int64), 20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.image_prep(torch.zeros(12, dtype=torch.uint8), off, torch.zeros(1, 4, dtype=torch.int32), (32, 32))
