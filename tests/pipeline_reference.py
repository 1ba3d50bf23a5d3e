"""Float64 numpy restatement of the scene input pipeline (mmdet3d 0.18.1 / mmcv 0.18-era transforms,
[dep-recall]) that tests/test_gpu_pipeline.py holds csrc/pipeline.hip and demf_amd/pipeline.py against, plus a writer
of small SUN RGB-D-layout datasets.  Independent of the product code except for data.augment_3d / add_height,
which tests/test_data_path.py already pins."""
import os
import pickle

import numpy as np

MEAN = np.array([123.675, 116.28, 103.53])
STD = np.array([58.395, 57.12, 57.375])
AXIS = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])


def percentile_floor(z):
    """np.percentile(z, 0.99) restated: linear interpolation between the order statistics of rank
    floor(0.0099 (n-1)) and the next, in float64."""
    s = np.sort(np.asarray(z, np.float64))
    n = s.shape[0]
    v = (n - 1) * 0.0099
    lo = int(np.floor(v))
    hi = min(lo + 1, n - 1)
    t = v - lo
    return s[lo] + (s[hi] - s[lo]) * t


def rescale_shape(h, w, img_scale):
    """mmcv rescale_size with keep_ratio: (h, w) scaled to fit (long, short) edges."""
    long_e, short_e = max(img_scale), min(img_scale)
    s = min(long_e / max(h, w), short_e / min(h, w))
    return int(h * s + 0.5), int(w * s + 0.5)


def _taps(n_out, n_in):
    d = np.arange(n_out, dtype=np.float64)
    s = (d + 0.5) * n_in / n_out - 0.5
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    low = s < 0
    i0[low], f[low] = 0, 0.0
    high = i0 >= n_in - 1
    i0[high], f[high] = n_in - 1, 0.0
    return i0, np.minimum(i0 + 1, n_in - 1), f


def resize_bilinear(img, h_out, w_out):
    """cv2.resize(INTER_LINEAR) in float64 before rounding: (h, w, 3) uint8 -> (h_out, w_out, 3) float64."""
    x = np.asarray(img, np.float64)
    y0, y1, fy = _taps(h_out, x.shape[0])
    x0, x1, fx = _taps(w_out, x.shape[1])
    fx = fx[None, :, None]
    top = x[y0][:, x0] * (1 - fx) + x[y0][:, x1] * fx
    bot = x[y1][:, x0] * (1 - fx) + x[y1][:, x1] * fx
    return top * (1 - fy[:, None, None]) + bot * fy[:, None, None]


def image_levels(img, h_out, w_out):
    """-> (pre-rounding float64 values, uint8 levels) of the resized image, both (3, h_out, w_out)."""
    pre = resize_bilinear(img, h_out, w_out).transpose(2, 0, 1)
    return pre, np.clip(np.rint(pre), 0, 255)


def levels_of(out):
    """Normalised (3, H, W) float output -> the uint8 levels it was made from."""
    return np.rint(np.asarray(out, np.float64) * STD[:, None, None] + MEAN[:, None, None])


def bottom_center(boxes):
    b = np.asarray(boxes, np.float64).reshape(-1, 7).copy()
    b[:, 2] -= b[:, 5] / 2
    return b


def depth2img(K, Rt):
    return np.asarray(K, np.float64).reshape(3, 3) @ (AXIS @ np.asarray(Rt, np.float64).reshape(3, 3).T)


# ---- a small SUN RGB-D-layout dataset on disk ----------------------------------------------------------------------

def make_scene(rng, n_points, img_hw, n_gt):
    """A room-like cloud (with r, g, b columns) around n_gt boxes in front of the camera, an image, calibration."""
    lo, hi = np.array([-2.0, 1.0, -1.2]), np.array([2.0, 5.0, 1.2])
    xyz = rng.uniform(lo, hi, size=(n_points, 3))
    xyz[:, 2] = np.where(rng.random(n_points) < 0.2, -1.2 + rng.normal(0, 0.01, n_points), xyz[:, 2])
    ctr = rng.uniform([-1.5, 2.0, -0.8], [1.5, 4.5, 0.2], size=(n_gt, 3))
    dims = rng.uniform([0.5, 0.5, 0.4], [1.5, 1.5, 1.0], size=(n_gt, 3))
    yaw = rng.uniform(-np.pi, np.pi, size=(n_gt, 1))
    boxes = np.concatenate([ctr, dims, yaw], 1).astype(np.float32)
    # a quarter of the points on the objects, so that the boxes are not empty
    if n_gt:
        k = n_points // 4
        which = rng.integers(0, n_gt, size=k)
        xyz[:k] = ctr[which] + rng.uniform(-0.5, 0.5, size=(k, 3)) * dims[which] * 0.8
    rgb = rng.uniform(0, 1, size=(n_points, 3))
    raw = np.concatenate([xyz, rgb], 1).astype(np.float32)
    h, w = img_hw
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    K = np.array([[529.5 * w / 730, 0, w / 2], [0, 529.5 * h / 530, h / 2], [0, 0, 1.0]])
    tilt = rng.uniform(-0.1, 0.1)
    Rt = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
    labels = rng.integers(0, 10, size=n_gt)
    return raw, img, K, Rt, boxes, labels


def write_dataset(root, specs, split="train", seed=0, jpeg=True):
    """specs: list of (n_points, (h, w), n_gt).  Writes points/*.bin, sunrgbd_trainval/image/*.{jpg,png} and
    sunrgbd_infos_{split}.pkl under ``root`` in mmdet3d 0.18.1's layout; -> (ann file path, per-scene arrays)."""
    from PIL import Image
    from demf_amd.config import SUNRGBD_CLASSES
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "points"), exist_ok=True)
    os.makedirs(os.path.join(root, "sunrgbd_trainval", "image"), exist_ok=True)
    infos, scenes = [], []
    for i, (n, hw, n_gt) in enumerate(specs):
        idx = i + 1
        raw, img, K, Rt, boxes, labels = make_scene(rng, n, hw, n_gt)
        raw.tofile(os.path.join(root, "points", f"{idx:06d}.bin"))
        ext = "jpg" if jpeg else "png"
        Image.fromarray(img).save(os.path.join(root, "sunrgbd_trainval", "image", f"{idx:06d}.{ext}"))
        annos = dict(gt_num=0) if n_gt == 0 else dict(
            gt_num=n_gt, name=np.array([SUNRGBD_CLASSES[l] for l in labels]),
            bbox=np.zeros((n_gt, 4), np.float32), location=boxes[:, :3], dimensions=boxes[:, 3:6] * 0.5,
            rotation_y=boxes[:, 6], index=np.arange(n_gt, dtype=np.int32), **{"class": labels.astype(np.int64)},
            gt_boxes_upright_depth=boxes)
        infos.append(dict(point_cloud=dict(num_features=6, lidar_idx=idx), pts_path=f"points/{idx:06d}.bin",
                          image=dict(image_idx=idx, image_shape=np.array(hw, np.int32),
                                     image_path=f"image/{idx:06d}.{ext}"),
                          calib=dict(K=K.astype(np.float32), Rt=Rt.astype(np.float32)), annos=annos))
        scenes.append(dict(raw=raw, img=img, K=K, Rt=Rt, boxes=boxes, labels=labels))
    ann = os.path.join(root, f"sunrgbd_infos_{split}.pkl")
    with open(ann, "wb") as f:
        pickle.dump(infos, f)
    return ann, scenes
