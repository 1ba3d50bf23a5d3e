"""SUN RGB-D scenes as mmdet3d 0.18.1's ``SUNRGBDDataset`` reads them (configs/_base_/datasets/sunrgbd-3d-10class.py;
the infos are what ``tools/create_data.py sunrgbd`` writes) [dep-recall: restated from upstream's published
behaviour, its sources are not in the reference tree].

Layout under ``data_root``::

    sunrgbd_infos_{train,val}.pkl        list of dicts, one per scene:
        point_cloud:  {num_features: 6, lidar_idx: <sample idx>}
        pts_path:     'points/000001.bin'                 (N, 6) float32 records: x y z r g b
        image:        {image_idx, image_shape, image_path: 'image/000001.jpg'}
        calib:        {K (3,3) or (9,), Rt (3,3)}
        annos:        {gt_num, name, class (n,), gt_boxes_upright_depth (n,7) gravity centre, ...}
    sunrgbd_trainval/image/000001.jpg

The per-point and per-pixel pipeline that turns a scene into the detector's tensors is ``pipeline.SceneLoader``.
"""
import os
import pickle

import numpy as np

from .config import SUNRGBD_CLASSES
from .data import depth2img_from_calib


def load_infos(ann_file):
    """The infos pickle -> list of dicts.  A pickle can execute code while it is read: only load infos files from
    a trusted source (the ones ``create_data.py`` wrote)."""
    with open(ann_file, "rb") as f:
        infos = pickle.load(f)
    if not isinstance(infos, list):
        raise ValueError(f"{ann_file}: expected a list of scene dicts, got {type(infos).__name__}")
    return infos


def upright_to_bottom_center(boxes):
    """gt_boxes_upright_depth (n,7) gravity-centred -> the bottom-centre depth boxes of
    ``DepthInstance3DBoxes(boxes, origin=(0.5, 0.5, 0.5))``, fp32: z + dz * (0 - 0.5)."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 7).copy()
    b[:, 2] = b[:, 2] + b[:, 5] * np.float32(0.0 - 0.5)
    return b


def read_sunrgbd_calib(path):
    """Upstream's ``calib/*.txt`` of a SUN RGB-D scene: line 1 the tilt matrix Rt, line 2 the intrinsics K, each 9
    values in column-major order [dep-recall].  -> dict(K (3,3), Rt (3,3)) float64, row-major as everywhere here."""
    with open(path) as f:
        lines = [l for l in f.read().splitlines() if l.strip()]
    if len(lines) < 2:
        raise ValueError(f"{path}: expected two lines (Rt, K), got {len(lines)}")
    mats = []
    for name, line in zip(("Rt", "K"), lines[:2]):
        vals = [float(v) for v in line.split()]
        if len(vals) != 9:
            raise ValueError(f"{path}: {name} has {len(vals)} values, expected 9")
        mats.append(np.array(vals, np.float64).reshape(3, 3).T)     # column-major on disk
    return dict(K=mats[1], Rt=mats[0])


class RGBDFrames:
    """Raw RGB-D frames - a colour image, a registered 16-bit depth PNG and a calibration each - for
    ``pipeline.FramePipeline``.  No annotations.

    ``frames``: a list of dicts ``{"id", "image", "depth", "K" (9 floats), "Rt" (9 floats)}`` or the path of a JSON
    file holding such a list (absolute or relative to ``data_root``); image and depth paths are relative to
    ``data_root``, K and Rt row-major.  ``shift`` / ``depth_scale`` / ``z_max`` / ``pixel_origin``: how a depth word
    becomes metres and which pixel grid the intrinsics refer to (see ``ops.depth_to_points``); the defaults are SUN
    RGB-D's storage (words rotated left by 3, millimetres, far readings clamped to 8 m) [dep-recall] with a 0-based
    pixel grid, which is the one ``depth2img`` projects onto."""

    CLASSES = SUNRGBD_CLASSES

    def __init__(self, data_root, frames, shift=3, depth_scale=1000.0, z_max=8.0, pixel_origin=0.0):
        import json
        self.data_root = str(data_root)
        if isinstance(frames, (str, os.PathLike)):
            path = str(frames) if os.path.isabs(str(frames)) else os.path.join(self.data_root, str(frames))
            with open(path) as f:
                frames = json.load(f)
        if not isinstance(frames, (list, tuple)):
            raise ValueError(f"expected a list of frame dicts, got {type(frames).__name__}")
        if not 0 <= int(shift) <= 15:
            raise ValueError(f"shift must be in 0..15, got {shift}")
        if not (float(depth_scale) > 0 and float(z_max) > 0):
            raise ValueError("depth_scale and z_max must be positive")
        self.shift, self.depth_scale, self.z_max = int(shift), float(depth_scale), float(z_max)
        self.pixel_origin = float(pixel_origin)
        self.frames = []
        for i, fr in enumerate(frames):
            missing = [k for k in ("image", "depth", "K", "Rt") if k not in fr]
            if missing:
                raise ValueError(f"frame {i}: missing {missing}")
            K, Rt = np.asarray(fr["K"], np.float64), np.asarray(fr["Rt"], np.float64)
            if K.size != 9 or Rt.size != 9:
                raise ValueError(f"frame {i}: K and Rt must hold 9 values each, got {K.size} and {Rt.size}")
            self.frames.append(dict(id=fr.get("id", i), image=str(fr["image"]), depth=str(fr["depth"]),
                                    K=K.reshape(3, 3), Rt=Rt.reshape(3, 3)))

    def __len__(self):
        return len(self.frames)

    def calib_row(self, calib):
        """-> the (16,) fp64 row of ``ops.depth_to_points``."""
        K, Rt = calib["K"], calib["Rt"]
        return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], Rt.reshape(9),
                               [self.pixel_origin, self.depth_scale, self.z_max]]).astype(np.float64)

    def get_data_info(self, index):
        """-> dict(sample_idx, img_filename, depth_filename, calib (K, Rt), depth2img (3,3) fp32)."""
        fr = self.frames[index]
        return dict(sample_idx=fr["id"], img_filename=os.path.join(self.data_root, fr["image"]),
                    depth_filename=os.path.join(self.data_root, fr["depth"]),
                    calib=dict(K=fr["K"], Rt=fr["Rt"]), depth2img=depth2img_from_calib(fr["K"], fr["Rt"]))


class SUNRGBDDataset:
    """mmdet3d SUNRGBDDataset (modality: points + image) over an infos file.

    ``filter_empty_gt`` drops scenes without ground truth in training, as upstream's ``_filter_imgs`` /
    ``pre_pipeline`` do; in ``test_mode`` every scene is kept and no annotation is required."""

    CLASSES = SUNRGBD_CLASSES

    def __init__(self, data_root, ann_file, classes=SUNRGBD_CLASSES, test_mode=False, filter_empty_gt=False):
        self.data_root = str(data_root)
        self.ann_file = ann_file if os.path.isabs(str(ann_file)) else os.path.join(self.data_root, str(ann_file))
        self.CLASSES = tuple(classes)
        self.cat2id = {name: i for i, name in enumerate(self.CLASSES)}
        self.test_mode = test_mode
        infos = load_infos(self.ann_file)
        if filter_empty_gt and not test_mode:
            infos = [i for i in infos if i.get("annos", {}).get("gt_num", 0) > 0]
        self.data_infos = infos

    def __len__(self):
        return len(self.data_infos)

    def get_data_info(self, index):
        """-> dict(sample_idx, pts_filename, img_filename, depth2img (3,3) fp32 = K @ (AXIS @ Rt^T), calib,
        [ann_info unless test_mode])."""
        info = self.data_infos[index]
        calib = info["calib"]
        out = dict(
            sample_idx=info["point_cloud"]["lidar_idx"],
            pts_filename=os.path.join(self.data_root, info["pts_path"]),
            img_filename=os.path.join(self.data_root, "sunrgbd_trainval", info["image"]["image_path"]),
            depth2img=depth2img_from_calib(calib["K"], calib["Rt"]),
            calib=calib,
            img_info=dict(filename=info["image"]["image_path"]),
        )
        if not self.test_mode:
            out["ann_info"] = self.get_ann_info(index)
        return out

    def get_ann_info(self, index):
        """-> dict(gt_bboxes_3d (n,7) fp32 bottom-centre depth boxes, gt_labels_3d (n,) int64); a scene with
        ``gt_num == 0`` gets (0,7) / (0,)."""
        annos = self.data_infos[index]["annos"]
        if annos["gt_num"] == 0:
            return dict(gt_bboxes_3d=np.zeros((0, 7), np.float32), gt_labels_3d=np.zeros((0,), np.int64))
        boxes = upright_to_bottom_center(annos["gt_boxes_upright_depth"])
        labels = np.asarray(annos["class"], dtype=np.int64).reshape(-1)
        if labels.shape[0] != boxes.shape[0]:
            raise ValueError(f"scene {index}: {boxes.shape[0]} boxes but {labels.shape[0]} classes")
        return dict(gt_bboxes_3d=boxes, gt_labels_3d=labels)

    def evaluate(self, results, metric=(0.25, 0.5), logger=None):
        """indoor_eval of ``results`` (one ``simple_test`` dict per scene, in dataset order, or a
        ``DetectionStore`` holding the scenes in that order) against the infos'
        annotations -> ``{cat}_AP_{t}``, ``mAP_{t}``, ``{cat}_rec_{t}``, ``mAR_{t}`` (evaluation.indoor_eval)."""
        from .evaluation import indoor_eval
        if len(results) != len(self):
            raise ValueError(f"{len(results)} results for {len(self)} scenes")
        gt_annos = [info["annos"] for info in self.data_infos]
        label2cat = dict(enumerate(self.CLASSES))
        return indoor_eval(gt_annos, results, metric, label2cat, logger=logger)
