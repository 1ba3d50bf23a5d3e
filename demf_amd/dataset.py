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
