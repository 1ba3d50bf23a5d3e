"""Raw RGB-D frames end to end: ``SceneLoader(RGBDFrames, pipeline=FramePipeline)`` against the prepared-dataset path
fed the very records ``ops.depth_to_points`` makes of the same frames (written as ``.bin`` + infos in the layout of
tests/pipeline_reference.write_dataset), through the loaders, ``infer.run_test`` and the ``--frames`` command line."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import frame_reference as fref

pytestmark = pytest.mark.gpu

SIZES = [(53, 73), (43, 56), (44, 59), (48, 64)]              # the image sizes of test_gpu_pipeline.SPECS
NUM_POINTS, SEED = 2048, 1


def _rotl16(d, s):
    d = np.asarray(d, np.uint32)
    return (((d << s) | (d >> (16 - s))) & 0xFFFF).astype(np.uint16)


def _synthetic_frame(rng, h, w):
    """A tilted camera 1.2 m above a floor, a back wall at 5 m and two fronto-parallel box faces; a few holes."""
    K = np.array([[529.5 * w / 730, 0, w / 2], [0, 529.5 * h / 530, h / 2], [0, 0, 1.0]]).astype(np.float32)
    tilt = rng.uniform(0.15, 0.3)
    Rt = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]]).astype(np.float32)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    a, b = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    down = Rt[2, 0] * a + Rt[2, 1] * 1.0 + Rt[2, 2] * (-b)            # height gained per metre of depth
    z = np.where(down < -1e-6, -1.2 / np.minimum(down, -1e-6), 5.0)
    z = np.minimum(z, 5.0)
    for _ in range(2):
        y0, x0 = rng.integers(h // 4, h // 2), rng.integers(0, w // 2)
        face = rng.uniform(1.5, 3.0)
        z[y0:y0 + h // 3, x0:x0 + w // 3] = np.minimum(z[y0:y0 + h // 3, x0:x0 + w // 3], face)
    mm = np.rint(z * 1000.0).astype(np.uint16)
    mm[rng.random((h, w)) < 0.03] = 0
    return _rotl16(mm, 3), rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), K, Rt


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """The four frames on disk twice: raw (PNG colour + 16-bit PNG depth + manifest) and prepared (``.bin`` records
    from ``ops.depth_to_points`` + infos pickle).  -> (root, ann file, manifest path, frame dicts)."""
    from PIL import Image
    from demf_amd import ops
    from demf_amd.dataset import RGBDFrames
    root = str(tmp_path_factory.mktemp("frames"))
    for d in ("points", "depth", os.path.join("sunrgbd_trainval", "image")):
        os.makedirs(os.path.join(root, d))
    rng = np.random.default_rng(3)
    manifest, infos, made = [], [], []
    for i, (h, w) in enumerate(SIZES):
        idx = i + 1
        depth, rgb, K, Rt = _synthetic_frame(rng, h, w)
        Image.fromarray(rgb).save(os.path.join(root, "sunrgbd_trainval", "image", f"{idx:06d}.png"))
        Image.fromarray(depth).save(os.path.join(root, "depth", f"{idx:06d}.png"))
        manifest.append(dict(id=idx, image=f"sunrgbd_trainval/image/{idx:06d}.png", depth=f"depth/{idx:06d}.png",
                             K=[float(x) for x in K.reshape(-1)], Rt=[float(x) for x in Rt.reshape(-1)]))
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=idx), pts_path=f"points/{idx:06d}.bin",
                          image=dict(image_idx=idx, image_shape=np.array((h, w), np.int32),
                                     image_path=f"image/{idx:06d}.png"),
                          calib=dict(K=K, Rt=Rt), annos=dict(gt_num=0)))
        made.append(dict(depth=depth, rgb=rgb, K=K, Rt=Rt))
    frames = RGBDFrames(root, manifest)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
    for i, m in enumerate(made):
        h, w = m["depth"].shape
        calib = frames.calib_row(frames.get_data_info(i)["calib"])
        raw, off = ops.depth_to_points(up(m["depth"].reshape(-1)), up(np.array([0, h * w], np.int64)),
                                       up(m["rgb"].reshape(-1)), up(np.array([0, 3 * h * w], np.int64)),
                                       up(np.array([[h, w, h, w]], np.int32)), up(calib[None]), shift=3)
        rec = raw[:int(off[1])].cpu().numpy()
        want = fref.frame_records(m["depth"], m["rgb"], calib, 3)
        assert np.array_equal(rec.view(np.uint32), want.view(np.uint32)) and len(rec) > NUM_POINTS
        rec.tofile(os.path.join(root, "points", f"{i + 1:06d}.bin"))
    ann = os.path.join(root, "sunrgbd_infos_val.pkl")
    with open(ann, "wb") as f:
        pickle.dump(infos, f)
    path = os.path.join(root, "frames.json")
    with open(path, "w") as f:
        json.dump(manifest, f)
    return root, ann, path, made


def _loaders(both, batch_size):
    from demf_amd import pipeline as pl
    from demf_amd.dataset import RGBDFrames, SUNRGBDDataset
    from test_gpu_pipeline import IMG_SCALE
    root, ann, manifest, _ = both
    kw = dict(num_points=NUM_POINTS, img_scale=IMG_SCALE, seed=SEED)
    frames = RGBDFrames(root, manifest)
    return (pl.SceneLoader(SUNRGBDDataset(root, ann, test_mode=True), batch_size, "test", workers=4, **kw),
            pl.SceneLoader(frames, batch_size, "test", workers=4, pipeline=pl.FramePipeline(frames, **kw)))


@pytest.mark.parametrize("batch_size", [2, 3])
def test_frame_loader_equals_scene_loader(both, batch_size):
    scenes, frames = _loaders(both, batch_size)
    assert len(scenes) == len(frames) == -(-4 // batch_size)
    n = 0
    for a, b in zip(scenes, frames):
        assert a.indices == b.indices
        assert torch.equal(a["points"].view(torch.int32), b["points"].view(torch.int32))
        assert torch.equal(a["img"].view(torch.int32), b["img"].view(torch.int32))
        assert bool(torch.isfinite(b["points"]).all()) and b["points"].shape[1:] == (NUM_POINTS, 4)
        assert "gt_labels_3d" not in b
        for ma, mb in zip(a["img_metas"], b["img_metas"]):
            np.testing.assert_array_equal(ma["depth2img"], mb["depth2img"])
            np.testing.assert_array_equal(ma["scale_factor"], mb["scale_factor"])
            for k in ("img_shape", "pad_shape", "ori_shape", "batch_input_shape", "sample_idx"):
                assert ma[k] == mb[k], k
            assert mb["depth_filename"].endswith(".png") and "pts_filename" not in mb
            n += 1
    assert n == 4
    assert 0 < frames.last_upload_bytes < scenes.last_upload_bytes     # 2 B per pixel instead of 24 B per record


def test_loader_takes_its_mode_from_a_given_pipeline(both):
    from demf_amd import pipeline as pl
    from demf_amd.dataset import RGBDFrames
    root, _, manifest, _ = both
    frames = RGBDFrames(root, manifest)
    pipe = pl.FramePipeline(frames, num_points=64)
    ld = pl.SceneLoader(frames, 2, pipeline=pipe)
    assert ld.mode == "test" and ld.pipeline is pipe
    with pytest.raises(ValueError, match="mode"):
        pl.SceneLoader(frames, 2, "train", pipeline=pipe)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_run_test_over_frames_equals_run_test_over_the_prepared_scenes(both, batch_size):
    from demf_amd import infer
    from demf_amd import pipeline as pl
    from demf_amd.dataset import RGBDFrames, SUNRGBDDataset
    from test_gpu_detections import _assert_same_run, _detector
    from test_gpu_pipeline import IMG_SCALE
    root, ann, manifest, _ = both
    kw = dict(num_points=NUM_POINTS, img_scale=IMG_SCALE, seed=SEED)
    det = _detector().cuda()
    want = infer.run_test(det, SUNRGBDDataset(root, ann, test_mode=True), batch_size=batch_size, workers=4,
                          **kw).results()
    frames = RGBDFrames(root, manifest)
    got = infer.run_test(det, frames, batch_size=batch_size, workers=4, pipeline=pl.FramePipeline(frames, **kw)).results()
    print("rows per frame:", [len(r["labels_3d"]) for r in got])
    assert len(got) == 4 and sum(len(r["labels_3d"]) for r in got) >= 1
    _assert_same_run(got, want)


def test_command_line_over_a_manifest(both, capsys):
    from demf_amd import infer
    from demf_amd.modules import DeMFVoteNet
    from test_gpu_detections import _detector
    from test_gpu_detector import STREAM, _cfg256
    from test_gpu_pipeline import IMG_SCALE
    root, _, manifest, _ = both
    ckpt, out = os.path.join(root, "det.pth"), os.path.join(root, "results.pkl")
    torch.save(dict(state_dict={k: v.cpu() for k, v in _detector().state_dict().items()}), ckpt)
    capsys.readouterr()
    ret = infer.main(["--data-root", root, "--frames", manifest, "--checkpoint", ckpt, "--out", out],
                     model=DeMFVoteNet(_cfg256(), **STREAM), num_points=NUM_POINTS, img_scale=IMG_SCALE, seed=SEED)
    assert ret is None and capsys.readouterr().out.strip() == ""
    with open(out, "rb") as f:
        dumped = pickle.load(f)
    assert len(dumped) == 4 and all(set(r) == {"boxes_3d", "scores_3d", "labels_3d"} for r in dumped)
    assert sum(len(r["labels_3d"]) for r in dumped) >= 1
