"""Scene input pipeline: SUN RGB-D infos -> the batch ``DeMFVoteNet.forward_train`` / ``simple_test`` take.

The reference runs mmdet3d 0.18.1 / mmcv pipelines per scene on host workers (configs/demf/demf_votenet.py:184-216)
[dep-recall: their sources are not in the reference tree]:

    train  LoadPointsFromFile(shift_height, load_dim=6, use_dim=[0,1,2]) -> LoadImageFromFile -> LoadAnnotations3D
           -> Resize(img_scale, keep_ratio) -> Normalize(to_rgb) -> Pad(32) -> RandomFlip3D(sync_2d=False)
           -> GlobalRotScaleTrans(rot +-pi/6, scale 0.85-1.15, shift_height) -> PointSample(20000) -> collate
    test   the same without the 3-D augmentation (MultiScaleFlipAug3D(flip=False)); points are still sampled.

Here the host only reads the ``.bin`` records (``np.fromfile``) and decodes the JPEG (PIL, ``convert('RGB')``, so no
BGR swap is needed for ``to_rgb``) in a thread pool, draws the per-scene random parameters and packs the batch into
pinned buffers.  The raw records and uint8 pixels are uploaded as they are and csrc/pipeline.hip does the rest on the
loader's own stream: the floor percentile, the sample + augmentation, and the resize + normalise + pad.

``FramePipeline`` is the same pipeline in test mode with another point source: instead of the ``.bin`` of the offline
export it uploads a raw frame's 16-bit depth image and csrc/frame.hip unprojects it into the records on the device.

Random draws: one ``numpy.random.Generator`` per scene draws flip, angle, scale, translation in ``data.augment_3d``'s
order (``draw_aug_params``), then the 64-bit key of the point sample.  So ``augment_3d(pts, boxes, meta,
default_rng(s))`` and ``draw_aug_params(default_rng(s))`` apply the same transform; the boxes and metadata are
produced by replaying those parameters through ``augment_3d`` itself (``apply_aug_params``).  The point sample is a
keyed permutation, not ``np.random.choice``'s stream: same distribution, different indices.
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from .data import augment_3d, resize_meta

ROT_RANGE = (-np.pi / 6, np.pi / 6)            # demf_votenet.py GlobalRotScaleTrans
SCALE_RANGE = (0.85, 1.15)
TRANSLATION_STD = (0.0, 0.0, 0.0)
FLIP_RATIO = 0.5                               # RandomFlip3D flip_ratio_bev_horizontal
LOAD_DIM = 6


def draw_aug_params(rng, flip_ratio=FLIP_RATIO, rot_range=ROT_RANGE, scale_range=SCALE_RANGE,
                    translation_std=TRANSLATION_STD):
    """The draws of ``data.augment_3d`` in its order: flip, angle, scale, translation."""
    flip = bool(rng.random() < flip_ratio)
    angle = float(rng.uniform(*rot_range))
    scale = float(rng.uniform(*scale_range))
    trans = rng.normal(scale=np.asarray(translation_std, np.float64), size=3)
    return dict(flip=flip, angle=angle, scale=scale, trans=trans)


def identity_aug_params():
    """Test mode: no flip, angle 0, scale 1, no translation."""
    return dict(flip=False, angle=0.0, scale=1.0, trans=np.zeros(3))


class _Replay:
    """Stands in for the generator ``augment_3d`` draws from and hands back given parameters."""

    def __init__(self, params):
        self._uniform = iter((params["angle"], params["scale"]))
        self._trans = np.asarray(params["trans"], np.float64)

    def random(self):
        return 0.5                              # compared with flip_ratio 1.0 (flip) or 0.0 (no flip)

    def uniform(self, lo, hi):
        return next(self._uniform)

    def normal(self, scale=None, size=None):
        return self._trans.copy()


def apply_aug_params(boxes, meta, params, sync_2d=False):
    """Boxes (n,7) and metadata of ``augment_3d`` for given parameters (the points are left to the GPU): the
    parameters are replayed through ``augment_3d`` itself, so the arithmetic is exactly that function's.
    -> (boxes fp32, meta with flip / pcd_* / transformation_3d_flow)."""
    _, bx, m = augment_3d(np.zeros((0, 4), np.float32), np.asarray(boxes, np.float32).reshape(-1, 7), meta,
                          _Replay(params), flip_ratio=1.0 if params["flip"] else 0.0, sync_2d=sync_2d)
    return bx, m


def param_row(params):
    """-> the (8,) fp32 row of demf_points_prep: [flip, cos, sin, scale, tx, ty, tz, 0]."""
    t = np.asarray(params["trans"], np.float64)
    return np.array([1.0 if params["flip"] else 0.0, np.cos(params["angle"]), np.sin(params["angle"]),
                     params["scale"], t[0], t[1], t[2], 0.0], np.float32)


def pad_to(n, divisor=32):
    return int(-(-n // divisor) * divisor)


def collate_metas(metas, pad_divisor=32):
    """The collate step's padding: every image is padded to the batch's largest padded shape, which every scene's
    ``batch_input_shape`` then names (the per-scene padded shape stays in ``pad_shape``).  -> ((Hp, Wp), metas)."""
    Hp = max(pad_to(m["img_shape"][0], pad_divisor) for m in metas)
    Wp = max(pad_to(m["img_shape"][1], pad_divisor) for m in metas)
    out = []
    for m in metas:
        m = dict(m)
        m["batch_input_shape"] = (Hp, Wp)
        out.append(m)
    return (Hp, Wp), out


class ScenePipeline:
    """Per-scene host work (``load``) and the batched device work (``to_device``) of one pipeline mode."""

    def __init__(self, dataset, mode="train", img_scale=(1333, 800), num_points=20000, seed=0,
                 img_norm=ops.IMG_NORM, pad_divisor=32, with_img=True, image_shapes=None, tta=None):
        """``with_img=False`` (a points-only model): no image file is opened, nothing of it is uploaded and
        ``image_prep`` is not launched; the batch has no ``img`` and its metas carry no image entries.  Points, random
        draws and ground truth are those of the ``with_img=True`` pipeline for the same seed.

        ``with_img=False, image_shapes=mapping`` (training from ``featcache.FeatureCache``): dataset index -> the
        image's (h, w) as stored on disk.  Still no image file is opened and the batch has no ``img``, but every
        scene's meta is the complete one of the ``with_img=True`` pipeline, built from the stored shape, and
        ``to_device`` collates the metas (``batch_input_shape`` = the batch maximum).

        ``tta`` (a ``tta.TTACfg``, test mode only): every scene is prepared in V views.  Records and image bytes are
        uploaded once and ``points_floor`` runs once; ``points_prep`` runs once per view with that view's parameter
        rows and sample keys.  The batch then carries ``points`` as a list of V tensors, ``img_metas`` as a list of V
        lists (each made by ``apply_aug_params`` from the view's parameters), ONE ``img``, and ``view_params``: the
        (V * B, 8) device array of parameter rows, view-major.  View 0 has the sample key of the single-view batch
        (and, with a first scale of 1.0, its parameters); view v > 0 draws its key from the scene's generator after
        that draw, in view order."""
        if tta is not None and mode != "test":
            raise ValueError("tta is test-time augmentation: it goes with mode='test'")
        self.tta = tta
        if image_shapes is not None and with_img:
            raise ValueError("image_shapes stands in for the decoded image: it goes with with_img=False")
        if mode not in ("train", "test"):
            raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
        self.dataset, self.mode, self.with_img = dataset, mode, bool(with_img)
        self.img_scale, self.num_points, self.seed = tuple(img_scale), int(num_points), int(seed)
        self.img_norm, self.pad_divisor = img_norm, pad_divisor
        self.image_shapes = image_shapes

    def scene_rng(self, index, epoch=0):
        key = [self.seed, epoch, int(index)] if self.mode == "train" else [self.seed, int(index)]
        return np.random.default_rng(key)

    @staticmethod
    def read_image(path):
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def _scene(self, index, epoch, info, img, source_meta, **source):
        """What ``load`` returns, from a decoded image and the point source's own entries: random draws, boxes and
        metadata."""
        rng = self.scene_rng(index, epoch)
        params = draw_aug_params(rng) if self.mode == "train" else identity_aug_params()
        seed = int(rng.integers(0, 2 ** 63 - 1))
        if img is not None:
            hw = img.shape[:2]
        else:                                       # with_img=False: no image entries, or those of the stored shape
            hw = None if self.image_shapes is None else self.image_shapes[int(index)]
        if hw is None:
            meta = dict(sample_idx=info["sample_idx"], **source_meta, flip=False)
        else:
            h, w = int(hw[0]), int(hw[1])
            meta = dict(sample_idx=info["sample_idx"], **source_meta,
                        img_filename=info["img_filename"], depth2img=info["depth2img"], flip=False,
                        img_norm_cfg=dict(mean=np.asarray(self.img_norm[0], np.float32),
                                          std=np.asarray(self.img_norm[1], np.float32), to_rgb=True))
            meta = resize_meta(meta, (h, w), self.img_scale, self.pad_divisor)
            meta["pad_shape"] = tuple(meta["batch_input_shape"]) + (3,)
        ann = info.get("ann_info")
        boxes = ann["gt_bboxes_3d"] if ann is not None else np.zeros((0, 7), np.float32)
        views = None
        if self.tta is not None:                    # view 0: the draw above; the others draw their keys after it
            from .tta import view_params
            views = []
            for v, p in enumerate(view_params(self.tta)):
                key = seed if v == 0 else int(rng.integers(0, 2 ** 63 - 1))
                views.append(dict(params=p, seed=key, meta=apply_aug_params(boxes, meta, p)[1]))
            params = views[0]["params"]
        boxes, meta = apply_aug_params(boxes, meta, params)
        return dict(index=int(index), img=img, params=params, seed=seed, meta=meta, gt_bboxes_3d=boxes,
                    gt_labels_3d=None if ann is None else ann["gt_labels_3d"], views=views, **source)

    def _view_words(self, scenes):
        """-> (parameter rows (V * B, 8) fp32, sample keys (V * B,) int64), view-major; one view without ``tta``."""
        if self.tta is None:
            return (np.stack([param_row(s["params"]) for s in scenes]),
                    np.array([s["seed"] for s in scenes], np.int64))
        V = self.tta.num_views
        return (np.stack([param_row(s["views"][v]["params"]) for v in range(V) for s in scenes]),
                np.array([s["views"][v]["seed"] for v in range(V) for s in scenes], np.int64))

    def _view_points(self, raw_d, poff_d, floor, params, seeds, B):
        """``points_prep`` once per view: -> the (B, num_points, 4) tensor, or the list of V of them with ``tta``."""
        params = params.view(-1, 8)
        if self.tta is None:
            return ops.points_prep(raw_d, poff_d, floor, params, seeds, self.num_points)
        return [ops.points_prep(raw_d, poff_d, floor, params[v * B:(v + 1) * B], seeds[v * B:(v + 1) * B],
                                self.num_points) for v in range(self.tta.num_views)]

    def _view_metas(self, scenes, collate):
        """The batch's metas (``collate``: through ``collate_metas``): a list per scene, or V of them with ``tta``."""
        def one(metas):
            return collate_metas(metas, self.pad_divisor)[1] if collate else [dict(m) for m in metas]
        if self.tta is None:
            return one([s["meta"] for s in scenes])
        return [one([s["views"][v]["meta"] for s in scenes]) for v in range(self.tta.num_views)]

    def load(self, index, epoch=0):
        """Host part of one scene: file reads, JPEG decode, random draws, boxes and metadata."""
        info = self.dataset.get_data_info(index)
        raw = np.fromfile(info["pts_filename"], dtype=np.float32)
        if raw.size == 0 or raw.size % LOAD_DIM:
            raise ValueError(f"{info['pts_filename']}: {raw.size} floats is not a positive multiple of {LOAD_DIM}")
        return self._scene(index, epoch, info, self.read_image(info["img_filename"]) if self.with_img else None,
                           dict(pts_filename=info["pts_filename"]), raw=raw.reshape(-1, LOAD_DIM))

    # ---- the point source: what is uploaded for the clouds and how it becomes (raw, offsets) on the device ----------
    def pack_source(self, scenes):
        """-> (pinned buffers uploaded as they are, small host arrays that travel in the batch's one small upload)."""
        npts = np.array([s["raw"].shape[0] for s in scenes], np.int64)
        raw_h = torch.empty((int(npts.sum()), LOAD_DIM), dtype=torch.float32, pin_memory=True)
        raw_np = raw_h.numpy()
        poff = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
        for b, s in enumerate(scenes):
            raw_np[poff[b]:poff[b + 1]] = s["raw"]
        return dict(raw=raw_h), dict(poff=poff)

    def source_records(self, big, small, img_d):
        """On the pipeline's stream: the uploaded buffers -> (raw (total, 6) records, offsets (B+1,) int64)."""
        return big["raw"], small["poff"]

    def to_device(self, scenes, device, stream=None):
        """Pack ``load`` results into pinned buffers, upload them and run the kernels on ``stream`` (default:
        the current stream).  -> (batch dict, uploaded bytes).  The batch is valid on ``stream`` once the call
        returns; another stream must wait on it first."""
        B = len(scenes)
        if not self.with_img:
            return self._to_device_points(scenes, device, stream)
        nbytes = np.array([s["img"].size for s in scenes], np.int64)
        img_h = torch.empty((int(nbytes.sum()),), dtype=torch.uint8, pin_memory=True)
        img_np = img_h.numpy()
        ioff = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)
        for b, s in enumerate(scenes):
            img_np[ioff[b]:ioff[b + 1]] = s["img"].reshape(-1)
        shp = []
        for s in scenes:
            h, w = s["img"].shape[:2]
            nh, nw = s["meta"]["img_shape"][:2]
            shp += [h, w, nh, nw]
        big, words = self.pack_source(scenes)
        # every small array as whole 8-byte words of one upload: params (B,8) fp32, the source's, offsets, seeds, shapes
        rows, keys = self._view_words(scenes)
        words = dict(params=rows.reshape(-1), **words, ioff=ioff, seeds=keys, shapes=np.array(shp, np.int32))
        words = {k: np.ascontiguousarray(v).reshape(-1) for k, v in words.items()}
        at, n = {}, 0
        for k, v in words.items():
            if v.nbytes % 8:
                raise ValueError(f"{k}: {v.nbytes} bytes is not a whole number of 8-byte words")
            at[k] = (n, n + v.nbytes // 8)
            n += v.nbytes // 8
        small = torch.empty((n,), dtype=torch.int64, pin_memory=True)
        sm = small.numpy()
        for k, v in words.items():
            sm[at[k][0]:at[k][1]].view(v.dtype)[:] = v
        (Hp, Wp), _ = collate_metas([s["meta"] for s in scenes], self.pad_divisor)
        metas = self._view_metas(scenes, True)
        stream = torch.cuda.current_stream(device) if stream is None else stream
        with torch.cuda.stream(stream):
            big_d = {k: t.to(device, non_blocking=True) for k, t in big.items()}
            img_d = img_h.to(device, non_blocking=True)
            small_d = small.to(device, non_blocking=True)
            sd = {k: small_d[a:b].view(getattr(torch, str(words[k].dtype))) for k, (a, b) in at.items()}
            sd["shapes"] = sd["shapes"].view(B, 4)
            raw_d, poff_d = self.source_records(big_d, sd, img_d)
            floor = ops.points_floor(raw_d, poff_d)
            points = self._view_points(raw_d, poff_d, floor, sd["params"], sd["seeds"], B)
            img = ops.image_prep(img_d, sd["ioff"], sd["shapes"], (Hp, Wp), *self.img_norm)
            batch = dict(points=points, img=img, img_metas=metas)
            if self.tta is not None:
                batch["view_params"] = sd["params"].view(-1, 8)
            if all(s["gt_labels_3d"] is not None for s in scenes):
                batch["gt_bboxes_3d"] = [torch.from_numpy(np.ascontiguousarray(s["gt_bboxes_3d"])).to(device)
                                         for s in scenes]
                batch["gt_labels_3d"] = [torch.from_numpy(np.ascontiguousarray(s["gt_labels_3d"])).to(device)
                                         for s in scenes]
        uploaded = sum(t.numel() * t.element_size() for t in big.values()) + img_h.numel() + small.numel() * 8
        return batch, uploaded

    def _to_device_points(self, scenes, device, stream=None):
        """``to_device`` without the image: the same point source, parameters, seeds and kernels (``points_floor``,
        ``points_prep``) in the same order; no image bytes, offsets or shapes travel and ``image_prep`` is not launched."""
        B = len(scenes)
        big, words = self.pack_source(scenes)
        rows, keys = self._view_words(scenes)
        words = dict(params=rows.reshape(-1), **words, seeds=keys)
        words = {k: np.ascontiguousarray(v).reshape(-1) for k, v in words.items()}
        at, n = {}, 0
        for k, v in words.items():
            if v.nbytes % 8:
                raise ValueError(f"{k}: {v.nbytes} bytes is not a whole number of 8-byte words")
            at[k] = (n, n + v.nbytes // 8)
            n += v.nbytes // 8
        small = torch.empty((n,), dtype=torch.int64, pin_memory=True)
        sm = small.numpy()
        for k, v in words.items():
            sm[at[k][0]:at[k][1]].view(v.dtype)[:] = v
        stream = torch.cuda.current_stream(device) if stream is None else stream
        with torch.cuda.stream(stream):
            big_d = {k: t.to(device, non_blocking=True) for k, t in big.items()}
            small_d = small.to(device, non_blocking=True)
            sd = {k: small_d[a:b].view(getattr(torch, str(words[k].dtype))) for k, (a, b) in at.items()}
            raw_d, poff_d = self.source_records(big_d, sd, None)
            floor = ops.points_floor(raw_d, poff_d)
            points = self._view_points(raw_d, poff_d, floor, sd["params"], sd["seeds"], B)
            # (with image_shapes the image metas are complete: collated as the image batch's are)
            metas = self._view_metas(scenes, self.image_shapes is not None)
            batch = dict(points=points, img_metas=metas)
            if self.tta is not None:
                batch["view_params"] = sd["params"].view(-1, 8)
            if all(s["gt_labels_3d"] is not None for s in scenes):
                batch["gt_bboxes_3d"] = [torch.from_numpy(np.ascontiguousarray(s["gt_bboxes_3d"])).to(device)
                                         for s in scenes]
                batch["gt_labels_3d"] = [torch.from_numpy(np.ascontiguousarray(s["gt_labels_3d"])).to(device)
                                         for s in scenes]
        return batch, sum(t.numel() * t.element_size() for t in big.values()) + small.numel() * 8


class FramePipeline(ScenePipeline):
    """``ScenePipeline`` in test mode over raw RGB-D frames (``dataset.RGBDFrames``): the host decodes the colour
    image and the 16-bit depth PNG; the depth words are uploaded as they are and ``ops.depth_to_points`` makes the
    records on the device from them and from the colour bytes that ``image_prep`` reads anyway.  The valid-pixel
    counts stay on the device.  Everything else - metadata, point sample, image - is ``ScenePipeline``'s."""

    def __init__(self, dataset, img_scale=(1333, 800), num_points=20000, seed=0, img_norm=ops.IMG_NORM,
                 pad_divisor=32, tta=None):
        super().__init__(dataset, "test", img_scale, num_points, seed, img_norm, pad_divisor, tta=tta)

    @staticmethod
    def read_depth(path):
        """A 16-bit depth PNG -> (h, w) uint16, the stored words untouched."""
        from PIL import Image
        with Image.open(path) as im:
            if im.mode not in ("I;16", "I;16L", "I;16B", "I;16N"):
                raise ValueError(f"{path}: depth must be a 16-bit greyscale image (PIL mode 'I;16'), got mode "
                                 f"{im.mode!r}")
            d = np.asarray(im)
        if d.dtype != np.uint16 or d.ndim != 2:
            raise ValueError(f"{path}: depth decoded as {d.dtype} {d.shape}, expected a 2-D uint16 image")
        return np.ascontiguousarray(d)

    def load(self, index, epoch=0):
        """Host part of one frame: colour and depth decode, metadata, the point sample's seed."""
        info = self.dataset.get_data_info(index)
        img = self.read_image(info["img_filename"])
        depth = self.read_depth(info["depth_filename"])
        if depth.shape != img.shape[:2]:
            raise ValueError(f"{info['depth_filename']}: depth is {depth.shape}, the image {img.shape[:2]}; colour "
                             "and depth must be registered")
        return self._scene(index, epoch, info, img, dict(depth_filename=info["depth_filename"]), depth=depth,
                           calib=self.dataset.calib_row(info["calib"]))

    def pack_source(self, scenes):
        npix = np.array([s["depth"].size for s in scenes], np.int64)
        depth_h = torch.empty((int(npix.sum()),), dtype=torch.uint16, pin_memory=True)
        depth_np = depth_h.numpy()
        doff = np.concatenate([[0], np.cumsum(npix)]).astype(np.int64)
        for b, s in enumerate(scenes):
            depth_np[doff[b]:doff[b + 1]] = s["depth"].reshape(-1)
        return dict(depth=depth_h), dict(doff=doff, calib=np.stack([s["calib"] for s in scenes]).astype(np.float64))

    def source_records(self, big, small, img_d):
        B = small["doff"].numel() - 1
        return ops.depth_to_points(big["depth"], small["doff"], img_d, small["ioff"], small["shapes"],
                                   small["calib"].view(B, 16), self.dataset.shift)


class SceneBatch(dict):
    """A batch dict (``points``, ``img``, ``img_metas`` [, ``gt_bboxes_3d``, ``gt_labels_3d``]) plus ``indices`` (the
    dataset indices of its scenes) and ``event`` (recorded on the loader's stream behind the batch's kernels)."""
    indices = ()
    event = None

    def wait(self, stream=None):
        """Make ``stream`` (default: the current one) wait for the batch and keep its memory alive there."""
        stream = torch.cuda.current_stream() if stream is None else stream
        stream.wait_event(self.event)
        def walk(v):
            if isinstance(v, (list, tuple)):        # (with tta: ``points`` is a list over views)
                for t in v:
                    walk(t)
            elif isinstance(v, torch.Tensor) and v.is_cuda:
                v.record_stream(stream)
        for v in self.values():
            walk(v)
        return self


def shard_chunks(order, batch_size, rank=0, world=1, mode="train", drop_last=False):
    """The index arrays rank ``rank`` of ``world`` iterates over ``order`` (an epoch's scene order), as a list.

    ``world == 1``: ``order`` cut into chunks of ``batch_size``; the short last one is kept unless ``drop_last``.
    Train mode, ``world > 1``: ``order`` (the permutation a single process draws) is extended by wrap-around to a
    multiple of ``world * batch_size`` (``drop_last``: cut down to one), cut into chunks of ``batch_size``, and rank r
    takes chunks r, r + W, r + 2W, ...: every rank runs the same number of full batches, and optimizer step k of the
    W ranks consumes the chunks a single process with ``accumulate = W`` consumes in its group k.
    Test mode, ``world > 1``: contiguous shards, rank r takes ``order[r * q : (r + 1) * q]`` with q = ceil(n / W),
    chunked by ``batch_size``; a shard may be empty."""
    order = np.asarray(order)
    bs, rank, world = int(batch_size), int(rank), int(world)
    if bs < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard_chunks: batch_size {bs}, rank {rank} of {world}")
    if mode not in ("train", "test"):
        raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
    n = len(order)
    if world > 1 and mode == "train":
        group = world * bs
        total = n // group * group if drop_last else -(-n // group) * group
        if n == 0 or total == 0:
            return []
        ext = order[np.arange(total) % n]
        return [ext[i:i + bs] for i in range(rank * bs, total, group)]
    if world > 1:
        q = -(-n // world)
        order = order[rank * q:min(n, (rank + 1) * q)]
    chunks = [order[i:i + bs] for i in range(0, len(order), bs)]
    if drop_last and chunks and len(chunks[-1]) < bs:
        chunks.pop()
    return chunks


class SceneLoader:
    """Batches of a dataset through ``ScenePipeline`` with host reads in ``workers`` threads and the device work on
    the loader's own stream, one batch ahead: while the consumer runs step k, batch k+1's kernels are queued on the
    loader stream and batch k+2's files are being read.  Every yielded batch has already been made to wait for on
    the current stream (``SceneBatch.wait``).

    Train mode reshuffles per epoch (a permutation keyed on (seed, epoch)) and draws every scene's augmentation from
    (seed, epoch, index); iterating the loader again runs the next epoch (RepeatDataset(times=5) is five epochs).
    Test mode keeps the dataset order, with no augmentation; the point sample is keyed on (seed, index).

    ``pipeline``: an instance (e.g. ``FramePipeline`` over ``RGBDFrames``) to use in place of the ``ScenePipeline``
    the loader would build; it then brings its own ``img_scale`` / ``num_points`` / ``seed``, and ``mode`` defaults
    to its mode (``"train"`` otherwise).

    ``rank`` / ``world``: the loader yields this rank's share of every epoch (``shard_chunks``); the permutation and
    the augmentations stay keyed on (seed, epoch[, index]), so a scene looks the same whichever rank draws it."""

    def __init__(self, dataset, batch_size, mode=None, seed=0, img_scale=(1333, 800), num_points=20000,
                 workers=8, drop_last=False, device=None, pipeline=None, with_img=None, image_shapes=None, tta=None,
                 rank=0, world=1):
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError(f"rank {rank} of world {world}")
        self.rank, self.world = int(rank), int(world)
        if tta is not None and pipeline is not None:
            raise ValueError("tta belongs to the pipeline the loader builds; the given pipeline brings its own")
        if mode is None:
            mode = "train" if pipeline is None else pipeline.mode
        if pipeline is not None and pipeline.mode != mode:
            raise ValueError(f"the given pipeline is in {pipeline.mode!r} mode, the loader in {mode!r}")
        if pipeline is not None and with_img is not None and bool(with_img) != pipeline.with_img:
            raise ValueError(f"the given pipeline was built with_img={pipeline.with_img}, the loader asks for {with_img}")
        if pipeline is not None and image_shapes is not None:
            raise ValueError("image_shapes belongs to the pipeline the loader builds; the given pipeline brings its own")
        self.pipeline = ScenePipeline(dataset, mode, img_scale, num_points, seed,
                                      with_img=True if with_img is None else with_img,
                                      image_shapes=image_shapes, tta=tta) if pipeline is None else pipeline
        self.dataset, self.batch_size, self.mode, self.seed = dataset, int(batch_size), mode, int(seed)
        self.drop_last = drop_last
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.workers = int(workers)
        self.epoch = 0
        self.last_upload_bytes = 0
        self._stream = None
        self._lock = threading.Lock()

    def __len__(self):
        n = len(self.dataset)
        if self.world > 1:
            return len(shard_chunks(np.arange(n), self.batch_size, self.rank, self.world, self.mode, self.drop_last))
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _order(self, epoch):
        n = len(self.dataset)
        if self.mode == "train":
            return np.random.default_rng([self.seed, epoch]).permutation(n)
        return np.arange(n)

    def _submit(self, pool, indices, epoch):
        return [pool.submit(self.pipeline.load, int(i), epoch) for i in indices]

    def _to_device(self, futures, indices):
        scenes = [f.result() for f in futures]
        batch, nbytes = self.pipeline.to_device(scenes, self.device, self._stream)
        self.last_upload_bytes = nbytes
        out = SceneBatch(batch)
        out.indices = tuple(int(i) for i in indices)
        out.event = torch.cuda.Event()
        out.event.record(self._stream)
        return out

    def __iter__(self):
        with self._lock:
            epoch = self.epoch
            self.epoch += 1
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
        order = self._order(epoch)
        chunks = shard_chunks(order, self.batch_size, self.rank, self.world, self.mode, self.drop_last)
        if not chunks:
            return
        pool = ThreadPoolExecutor(max_workers=max(1, self.workers))
        try:
            nxt = self._submit(pool, chunks[0], epoch)
            pending = None
            for k, idx in enumerate(chunks):
                cur = nxt
                if k + 1 < len(chunks):
                    nxt = self._submit(pool, chunks[k + 1], epoch)
                ready = self._to_device(cur, idx)
                if pending is not None:
                    yield pending.wait()
                pending = ready
            yield pending.wait()
        finally:
            pool.shutdown(wait=True, cancel_futures=True)
