"""Device-resident detections of many scenes in a fixed-shape form.

``DeMFVoteHead.get_bboxes_packed`` appends a batch's survivors to a ``DetectionStore`` without a host sync
(csrc/detect.hip: demf_detect_pack); ``evaluation.indoor_eval`` / ``SUNRGBDDataset.evaluate`` read the store's
boxes and scores where they lie.  Layout:

  boxes (R,7) fp32 bottom-centre depth boxes, scores (R,) fp32, labels (R,) int32  - R = ``max_rows``
  scene_off (S+1,) int32: scene i's rows are scene_off[i] .. scene_off[i+1]; scene_off[len(store)] is the row
      cursor of the next append (it keeps counting when rows no longer fit)
  state (2,) int32: [rows needed so far, overflow word]

Row order inside a scene is the reference's (``multiclass_nms_single`` with ``per_class_proposal``): class-major,
proposal index ascending inside a class.  The host knows how many SCENES were appended (it passes the batch size
each time); how many ROWS they hold is known to the device only, until ``results()`` asks.
"""
import numpy as np
import torch

from .geometry import DepthBoxes


class DetectionStore:
    def __init__(self, max_scenes, max_rows=None, device=None):
        if int(max_scenes) < 1:
            raise ValueError(f"max_scenes must be positive, got {max_scenes}")
        if max_rows is not None and int(max_rows) < 0:
            raise ValueError(f"max_rows must not be negative, got {max_rows}")
        self.max_scenes = int(max_scenes)
        self.max_rows = None if max_rows is None else int(max_rows)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.scene_off = torch.zeros((self.max_scenes + 1,), dtype=torch.int32, device=self.device)
        self.state = torch.zeros((2,), dtype=torch.int32, device=self.device)
        self.boxes = self.scores = self.labels = None
        self._scenes = 0
        if self.max_rows is not None:
            self._allocate(self.max_rows)

    def _allocate(self, rows):
        self.max_rows = int(rows)
        self.boxes = torch.empty((self.max_rows, 7), dtype=torch.float32, device=self.device)
        self.scores = torch.empty((self.max_rows,), dtype=torch.float32, device=self.device)
        self.labels = torch.empty((self.max_rows,), dtype=torch.int32, device=self.device)

    def __len__(self):
        return self._scenes

    def reset(self):
        """Forget every scene (the arrays stay allocated)."""
        self.scene_off.zero_()
        self.state.zero_()
        self._scenes = 0

    def reserve(self, batch, rows_per_scene):
        """Called by the appending side before its launch: checks that ``batch`` more scenes fit, allocates the
        worst case (``max_scenes * rows_per_scene`` rows) of a store made without ``max_rows`` at its first append,
        and counts the scenes.  -> the store index of the batch's first scene."""
        first = self._scenes
        if first + batch > self.max_scenes:
            raise RuntimeError(f"DetectionStore holds {first} of at most {self.max_scenes} scenes: "
                               f"{batch} more do not fit")
        if (first + batch) * int(rows_per_scene) >= (1 << 31):
            raise RuntimeError("too many detection rows for 32-bit offsets")
        if self.boxes is None:
            self._allocate(self.max_scenes * int(rows_per_scene))
        self._scenes = first + batch
        return first

    def host_index(self):
        """THE synchronisation point: -> (scene_off (len+1,) int64 numpy, rows).  Raises if rows did not fit."""
        n = self._scenes
        head = torch.cat([self.state, self.scene_off[:n + 1]]).cpu().numpy().astype(np.int64)
        off = head[2:]
        if head[1] != 0:
            raise RuntimeError(f"DetectionStore overflow: {int(off[-1])} rows are needed, the capacity is "
                               f"{self.max_rows} rows (max_rows)")
        return off, int(off[-1])

    def results(self):
        """-> what ``DeMFVoteNet.simple_test`` returns for the appended scenes: a list of dict(boxes_3d=DepthBoxes,
        scores_3d, labels_3d (int64)) in host memory.  One sync and four device -> host copies, however many
        scenes the store holds."""
        off, rows = self.host_index()
        if rows:
            boxes, scores = self.boxes[:rows].cpu(), self.scores[:rows].cpu()
            labels = self.labels[:rows].cpu().to(torch.int64)
        else:
            boxes, scores = torch.zeros((0, 7)), torch.zeros((0,))
            labels = torch.zeros((0,), dtype=torch.int64)
        return [dict(boxes_3d=DepthBoxes(boxes[a:b].clone()), scores_3d=scores[a:b].clone(),
                     labels_3d=labels[a:b].clone()) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


class Detection2DStore:
    """Device-resident 2D detections of many images, fixed shape (``modules.Detr2D.predict_into``; csrc/detr2d.hip:
    demf_detr2d_select writes one image's block per workgroup, without a host sync):

      rows (S,k,6) fp32 = [x1, y1, x2, y2, score, class] in the order (logit descending, flat index ascending),
          zeros behind an image's ``counts`` rows;  counts (S,) int32;  flag (1,) int32, bit 0 = a NaN logit was met

    ``score_thr``: the filter of ``extract_bboxes_2d`` (0.09 upstream); negative keeps all k places."""

    def __init__(self, max_images, k=100, score_thr=0.09, device=None):
        if int(max_images) < 1 or int(k) < 1:
            raise ValueError(f"max_images and k must be positive, got {max_images} and {k}")
        self.max_images, self.k, self.score_thr = int(max_images), int(k), float(score_thr)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rows = torch.zeros((self.max_images, self.k, 6), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros((self.max_images,), dtype=torch.int32, device=self.device)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._images = 0

    def __len__(self):
        return self._images

    def reset(self):
        """Forget every image (the arrays stay allocated)."""
        self.counts.zero_()
        self.flag.zero_()
        self._images = 0

    def reserve(self, batch, k):
        """Called by the appending side before its launch: checks that ``batch`` more images of ``k`` rows fit and
        counts them.  -> the store index of the batch's first image."""
        first = self._images
        if int(k) != self.k:
            raise RuntimeError(f"Detection2DStore was made for k = {self.k} rows per image, the detector writes {k}")
        if first + batch > self.max_images:
            raise RuntimeError(f"Detection2DStore holds {first} of at most {self.max_images} images: "
                               f"{batch} more do not fit")
        self._images = first + batch
        return first

    def results(self, per_class=False, num_classes=None):
        """THE synchronisation point -> per image the (n,6) tensor ``extract_bboxes_2d`` returns, in host memory;
        ``per_class``: mmdet's ``bbox2result`` instead - a list of ``num_classes`` (n_c,5) float32 arrays per image,
        rows in score order inside a class.  Raises if a NaN logit was met."""
        n = self._images
        counts = torch.cat([self.flag, self.counts[:n]]).cpu().numpy()
        if counts[0] != 0:
            raise RuntimeError("Detection2DStore: a NaN class logit was met while selecting detections")
        rows = self.rows[:n].cpu()
        out = [rows[i, :int(c)].clone() for i, c in enumerate(counts[1:])]
        if not per_class:
            return out
        if num_classes is None:
            raise ValueError("results(per_class=True) needs num_classes")
        res = []
        for r in out:
            r = r.numpy()
            res.append([r[r[:, 5] == c, :5].astype(np.float32) for c in range(int(num_classes))])
        return res
