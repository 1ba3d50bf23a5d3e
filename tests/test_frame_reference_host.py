"""The parts of the RGB-D frame front end that need no device: the numpy reference of tests/frame_reference.py against
values worked out by hand and against ``data.depth2img_from_calib`` (round trip), the frame manifest and calibration
readers of demf_amd/dataset.py, and the ``--frames`` rules of the demf_amd.infer command line."""
import json
import os

import numpy as np
import pytest

import frame_reference as fref


def _rotl16(d, s):
    d = np.asarray(d, np.uint32)
    return (((d << s) | (d >> (16 - s))) & 0xFFFF).astype(np.uint16)


# ---- the reference by hand ---------------------------------------------------------------------------------------
# stored words, shift 3: 8000 -> 1000 mm, 0 -> no reading, 16000 -> 2000 mm, 6465 -> 9000 mm (beyond z_max = 8 m),
# 7 -> 57 344 (the low bits wrap to the top: 57.344 m, clamped), 8000 -> 1000 mm
HAND_DEPTH = np.array([[8000, 0, 16000], [6465, 7, 8000]], np.uint16)
HAND_RGB = np.array([[[255, 0, 51], [9, 9, 9], [0, 255, 255]], [[51, 51, 0], [255, 255, 255], [0, 0, 0]]], np.uint8)
HAND_K = [[2.0, 0, 1.0], [0, 2.0, 0.5], [0, 0, 1.0]]           # fx = fy = 2, cx = 1, cy = 0.5
HAND_RT = [[0, 1.0, 0], [0, 0, 2.0], [-1.0, 0, 0]]             # p = (c1, 2 c2, -c0) = (z, -2 y3, -x3)


def test_rotation_of_the_depth_words():
    assert fref.rotate_right16(np.array([7, 8000, 6465, 0, 0xFFFF], np.uint16), 3).tolist() == \
        [57344, 1000, 9000, 0, 0xFFFF]
    assert fref.rotate_right16(np.array([7, 8000], np.uint16), 0).tolist() == [7, 8000]
    d = np.arange(0, 65536, 251, dtype=np.uint16)
    for s in (1, 3, 15):
        assert np.array_equal(fref.rotate_right16(_rotl16(d, s), s), d)


def test_reference_on_a_2x3_frame_by_hand():
    f51 = np.float32(51) / np.float32(255)
    rec = fref.frame_records(HAND_DEPTH, HAND_RGB, fref.calib_row(HAND_K, HAND_RT), shift=3)
    # pixel (u, v), z: x3 = (u - 1) z / 2, y3 = (v - 0.5) z / 2
    want = np.array([
        [1.0, 0.5, 0.5, 1.0, 0.0, f51],        # (0,0) z 1: x3 -0.5, y3 -0.25
        [2.0, 1.0, -1.0, 0.0, 1.0, 1.0],       # (2,0) z 2: x3  1,   y3 -0.5
        [8.0, -4.0, 4.0, f51, f51, 0.0],       # (0,1) z 8 (9 m clamped): x3 -4, y3 2
        [8.0, -4.0, 0.0, 1.0, 1.0, 1.0],       # (1,1) z 8 (57.344 m clamped): x3 0, y3 2
        [1.0, -0.5, -0.5, 0.0, 0.0, 0.0],      # (2,1) z 1: x3 0.5, y3 0.25
    ], np.float32)
    assert rec.dtype == np.float32 and rec.shape == (5, 6)
    np.testing.assert_array_equal(rec, want)
    # the toolbox's 1-based grid: u + 1, v + 1
    rec1 = fref.frame_records(HAND_DEPTH, HAND_RGB, fref.calib_row(HAND_K, HAND_RT, pixel_origin=1.0), shift=3)
    np.testing.assert_array_equal(rec1[0, :3], np.array([1.0, -0.5, 0.0], np.float32))    # x3 0, y3 0.25
    np.testing.assert_array_equal(rec1[4, :3], np.array([1.0, -1.5, -1.0], np.float32))   # x3 1, y3 0.75
    # plain millimetres: every non-zero word is a reading; 7 mm stays 7 mm
    rec0 = fref.frame_records(HAND_DEPTH, HAND_RGB, fref.calib_row(HAND_K, HAND_RT), shift=0)
    assert rec0.shape == (5, 6) and rec0[3, 0] == np.float32(0.007) and rec0[0, 0] == np.float32(8.0)
    # a batch: offsets, an empty frame in the middle
    recs, off = fref.depth_to_points([HAND_DEPTH, np.zeros((1, 4), np.uint16), HAND_DEPTH[:1]],
                                     [HAND_RGB, np.zeros((1, 4, 3), np.uint8), HAND_RGB[:1]],
                                     [fref.calib_row(HAND_K, HAND_RT)] * 3)
    assert off.tolist() == [0, 5, 5, 7] and off.dtype == np.int64
    np.testing.assert_array_equal(recs, np.concatenate([want, want[:2]]))


@pytest.mark.parametrize("seed", [0, 1])
def test_round_trip_through_depth2img(seed):
    """A record of pixel (u, v), projected in fp64 through the fp32 ``depth2img_from_calib(K, Rt)``, lands on (u, v)
    within 1e-3 px: measured 6.5e-5 px at worst over five random calibrations, the bar is 15 x that for fp32 storage
    of points and matrix at other calibrations."""
    from demf_amd.data import depth2img_from_calib
    rng = np.random.default_rng(seed)
    h, w = 530, 730
    mm = rng.integers(400, 9500, size=(h, w)).astype(np.uint16)
    mm[rng.random((h, w)) < 0.1] = 0
    K = np.array([[529.5 + rng.uniform(-20, 20), 0, w / 2 + rng.uniform(-10, 10)],
                  [0, 529.5 + rng.uniform(-20, 20), h / 2 + rng.uniform(-10, 10)], [0, 0, 1.0]])
    tilt, roll = rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05)
    rx = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
    ry = np.array([[np.cos(roll), 0, np.sin(roll)], [0, 1, 0], [-np.sin(roll), 0, np.cos(roll)]])
    Rt = rx @ ry
    rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    rec = fref.frame_records(_rotl16(mm, 3), rgb, fref.calib_row(K, Rt), shift=3)
    valid = mm != 0
    assert len(rec) == valid.sum() > 300000
    v, u = np.nonzero(valid)                                         # row-major, the records' order
    uvw = rec[:, :3].astype(np.float64) @ depth2img_from_calib(K, Rt).astype(np.float64).T
    err = np.maximum(np.abs(uvw[:, 0] / uvw[:, 2] - u), np.abs(uvw[:, 1] / uvw[:, 2] - v)).max()
    print(f"round trip: worst {err:.3g} px over {len(rec)} pixels")
    assert err <= 1e-3
    np.testing.assert_array_equal(rec[:, 3:], rgb[valid].astype(np.float32) / np.float32(255))
    # depth along the camera axis is what was stored, clamped at 8 m
    np.testing.assert_allclose(uvw[:, 2], np.minimum(mm[valid] / 1000.0, 8.0), rtol=1e-6)


# ---- dataset ---------------------------------------------------------------------------------------------------------
def _manifest(n=3):
    rng = np.random.default_rng(5)
    return [dict(id=f"f{i}", image=f"image/{i}.png", depth=f"depth/{i}.png",
                 K=[500.0 + i, 0, 320.5, 0, 501.0, 240.25, 0, 0, 1.0], Rt=rng.uniform(-1, 1, 9).tolist())
            for i in range(n)]


def test_frames_from_list_and_from_manifest_file(tmp_path):
    from demf_amd.data import depth2img_from_calib
    from demf_amd.dataset import RGBDFrames
    frames = _manifest()
    with open(tmp_path / "frames.json", "w") as f:
        json.dump(frames, f)
    for ds in (RGBDFrames(str(tmp_path), frames), RGBDFrames(str(tmp_path), "frames.json"),
               RGBDFrames(str(tmp_path), str(tmp_path / "frames.json"))):
        assert len(ds) == 3
        assert (ds.shift, ds.depth_scale, ds.z_max, ds.pixel_origin) == (3, 1000.0, 8.0, 0.0)
        for i, fr in enumerate(frames):
            info = ds.get_data_info(i)
            assert set(info) == {"sample_idx", "img_filename", "depth_filename", "calib", "depth2img"}
            assert info["sample_idx"] == f"f{i}"
            assert info["img_filename"] == os.path.join(str(tmp_path), f"image/{i}.png")
            assert info["depth_filename"] == os.path.join(str(tmp_path), f"depth/{i}.png")
            K, Rt = np.array(fr["K"]).reshape(3, 3), np.array(fr["Rt"]).reshape(3, 3)
            np.testing.assert_array_equal(info["calib"]["K"], K)
            np.testing.assert_array_equal(info["calib"]["Rt"], Rt)
            assert info["depth2img"].dtype == np.float32
            np.testing.assert_array_equal(info["depth2img"], depth2img_from_calib(K, Rt))
            np.testing.assert_array_equal(ds.calib_row(info["calib"]), fref.calib_row(K, Rt))
    ds = RGBDFrames(str(tmp_path), frames, shift=0, depth_scale=5000.0, z_max=10.0, pixel_origin=1.0)
    np.testing.assert_array_equal(ds.calib_row(ds.get_data_info(1)["calib"]),
                                  fref.calib_row(frames[1]["K"], frames[1]["Rt"], 1.0, 5000.0, 10.0))
    for bad in ([dict(image="a", depth="b", K=[1.0] * 9)], [dict(image="a", depth="b", K=[1.0] * 8, Rt=[1.0] * 9)],
                dict(frames=[])):
        with pytest.raises(ValueError):
            RGBDFrames(str(tmp_path), bad)
    with pytest.raises(ValueError):
        RGBDFrames(str(tmp_path), frames, shift=16)


def test_read_sunrgbd_calib(tmp_path):
    from demf_amd.dataset import read_sunrgbd_calib
    rt_cols = [0.979589, 0.012593, -0.200614, 0.012593, 0.992231, 0.123772, 0.200614, -0.123772, 0.971820]
    k_cols = [529.5, 0, 0, 0, 529.5, 0, 365, 265, 1]
    path = tmp_path / "000001.txt"
    path.write_text(" ".join(map(str, rt_cols)) + "\n" + " ".join(map(str, k_cols)) + "\n")
    c = read_sunrgbd_calib(str(path))
    assert c["K"].dtype == np.float64 and c["Rt"].dtype == np.float64
    np.testing.assert_array_equal(c["K"], [[529.5, 0, 365], [0, 529.5, 265], [0, 0, 1]])          # column-major file
    np.testing.assert_array_equal(c["Rt"], np.array(rt_cols).reshape(3, 3).T)
    assert c["Rt"][0, 2] == 0.200614 and c["Rt"][2, 0] == -0.200614
    (tmp_path / "short.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError):
        read_sunrgbd_calib(str(tmp_path / "short.txt"))
    (tmp_path / "eight.txt").write_text(" ".join(["1"] * 9) + "\n" + " ".join(["1"] * 8) + "\n")
    with pytest.raises(ValueError):
        read_sunrgbd_calib(str(tmp_path / "eight.txt"))


def test_frame_pipeline_refuses_what_is_not_a_registered_16_bit_depth(tmp_path):
    from PIL import Image
    from demf_amd.dataset import RGBDFrames
    from demf_amd.pipeline import FramePipeline
    rng = np.random.default_rng(2)
    os.makedirs(tmp_path / "d")
    Image.fromarray(rng.integers(0, 256, size=(6, 8, 3), dtype=np.uint8)).save(tmp_path / "d" / "c.png")
    words = rng.integers(0, 65536, size=(6, 8)).astype(np.uint16)
    Image.fromarray(words).save(tmp_path / "d" / "ok.png")
    Image.fromarray(words[:5]).save(tmp_path / "d" / "small.png")
    Image.fromarray((words >> 8).astype(np.uint8)).save(tmp_path / "d" / "eight.png")
    np.testing.assert_array_equal(FramePipeline.read_depth(str(tmp_path / "d" / "ok.png")), words)
    fr = [dict(image="d/c.png", depth=f"d/{n}.png", K=np.eye(3).reshape(-1).tolist(), Rt=np.eye(3).reshape(-1).tolist())
          for n in ("ok", "small", "eight")]
    pipe = FramePipeline(RGBDFrames(str(tmp_path), fr), img_scale=(64, 48), num_points=16, seed=3)
    s = pipe.load(0)
    assert s["depth"].dtype == np.uint16 and np.array_equal(s["depth"], words) and s["calib"].shape == (16,)
    assert s["meta"]["depth_filename"].endswith("ok.png") and s["gt_labels_3d"] is None
    assert (s["params"]["flip"], s["params"]["angle"], s["params"]["scale"]) == (False, 0.0, 1.0)
    assert s["seed"] == int(np.random.default_rng([3, 0]).integers(0, 2 ** 63 - 1))
    with pytest.raises(ValueError, match="registered"):
        pipe.load(1)
    with pytest.raises(ValueError, match="16-bit"):
        pipe.load(2)


# ---- command line ------------------------------------------------------------------------------------------------------
def test_frames_argument_rules():
    from demf_amd.infer import parse_args
    a = parse_args(["--data-root", "R", "--frames", "m.json", "--checkpoint", "c.pth", "--out", "o.pkl"])
    assert (a.data_root, a.frames, a.ann_file, a.checkpoint, a.out) == ("R", "m.json", None, "c.pth", "o.pkl")
    assert a.no_eval is True                                                   # implied: no ground truth
    a = parse_args(["--data-root", "R", "--ann-file", "v.pkl", "--checkpoint", "c.pth"])
    assert a.frames is None and a.no_eval is False
    for bad in (["--data-root", "R", "--frames", "m.json", "--checkpoint", "c"],                        # no --out
                ["--data-root", "R", "--frames", "m.json", "--ann-file", "v.pkl", "--checkpoint", "c", "--out", "o"],
                ["--data-root", "R", "--checkpoint", "c", "--out", "o"]):                               # neither
        with pytest.raises(SystemExit):
            parse_args(bad)
