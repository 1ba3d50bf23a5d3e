"""A frozen image-feature cache: train without the image stream.

The reference's training pipeline never augments the image (configs/demf/demf_votenet.py:194-197: a fixed
``Resize((1333, 800), keep_ratio)``, ``RandomFlip(flip_ratio=0.0)``, ``Normalize``, ``Pad(32)``; all randomness is in
the 3-D flow) and the image branch is frozen, so a scene's encoder tokens are the same in every one of the 36 x 5
passes of a run.  ``FeatureCache`` evaluates them once and keeps them on the device; ``train.fit(feature_cache=...)``
then runs neither the JPEG decode nor the image stream in its loop.

An ENTRY is the scene's encoder output evaluated ALONE: ``model.extract_img_feat(img[1,3,Hp,Wp], [meta])["tokens"][0]``
with (Hp, Wp) the scene's own padded shape ``pad_to(img_shape, 32)`` - every row of the scene's own levels, its own
padding rows included, as fp32 (exact) or bf16 (round to nearest even, half the bytes).  That is deliberately NOT the
value the scene has inside a mixed-shape batch, where the collate pads to the batch maximum and GroupNorm statistics
and border pixels see the extra zero columns (the reference has the same batch dependence); at equal image shapes the
cached and the uncached features are the same computation.  DESIGN.md section 3.15 has the measured difference.

Layout: one device ``arena`` (rows, C); scene i owns rows ``[row0_i, row0_i + sum_l h_il w_il)``, level after level,
each level row-major; the device ``table`` (N, 1 + 2L) int64 holds ``[row0, h_0, w_0, ..]`` per scene.
``assemble`` places a batch's scenes on the batch's canvas with one launch (``ops.assemble_tokens``,
csrc/featcache.hip).

On disk (``save`` / ``load``): ``index.json`` + raw little-endian data files (bf16 as uint16 words), each written under
a temporary name and renamed into place.  The index carries a fingerprint of everything the tokens depend on; ``load``
refuses a cache whose fingerprint, scene list or file sizes do not match.
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import ops
from .data import resize_meta
from .pipeline import ScenePipeline, pad_to

LAYOUT_VERSION = 1
INDEX_FILE = "index.json"
MAX_FILE_BYTES = 1 << 34          # a data file holds whole scenes up to this many bytes, then the next file starts
CHUNK_BYTES = 32 << 20            # the pinned staging buffer of save / load
RESERVE_BYTES = 4 << 30           # build(max_bytes=None): device memory left free for the training step itself
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STATE_PREFIXES = ("img_backbone.", "img_neck.", "img_encoder.")


# ---- fingerprint and index (host only) ------------------------------------------------------------------------------
def image_state(model):
    """The image branch's parameters and buffers, name -> CPU tensor."""
    return {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith(STATE_PREFIXES)}


def fingerprint(state, dtype, channels, img_scale, pad_divisor, img_norm, compute_dtype, version=LAYOUT_VERSION):
    """sha256 over everything a cached token depends on: layout version, storage dtype, C, img_scale, pad divisor,
    normalisation constants, the compute dtype and the names, shapes and bytes of the image branch's state in sorted
    key order.  ``state``: name -> tensor or ndarray."""
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
    h = hashlib.sha256()
    head = dict(version=int(version), dtype=str(dtype), C=int(channels), img_scale=[int(v) for v in img_scale],
                pad_divisor=int(pad_divisor), mean=[float(np.float32(v)) for v in img_norm[0]],
                std=[float(np.float32(v)) for v in img_norm[1]], compute_dtype=str(compute_dtype))
    h.update(json.dumps(head, sort_keys=True).encode())
    for name in sorted(state):
        v = state[name]
        a = v.detach().cpu().contiguous() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
        h.update(json.dumps([name, str(a.dtype), list(a.shape)]).encode())
        h.update(a.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def index_to_json(index):
    """The index dict -> JSON text (plain lists and numbers only)."""
    def plain(v):
        if isinstance(v, dict):
            return {str(k): plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, (np.integer,)):
            return int(v)
        if isinstance(v, (np.floating,)):
            return float(v)
        return v
    return json.dumps(plain(index), indent=1, sort_keys=True)


def index_from_json(text):
    """JSON text -> the index dict, checked: version, dtype, consecutive rows, file sizes that add up."""
    index = json.loads(text)
    for k in ("version", "dtype", "C", "levels", "img_scale", "pad_divisor", "fingerprint", "rows", "files", "scenes"):
        if k not in index:
            raise ValueError(f"feature cache index: no {k!r} entry")
    if index["version"] != LAYOUT_VERSION:
        raise ValueError(f"feature cache index: layout version {index['version']}, this package reads {LAYOUT_VERSION}")
    if index["dtype"] not in DTYPES:
        raise ValueError(f"feature cache index: dtype {index['dtype']!r}")
    row = 0
    for s in index["scenes"]:
        if s["row0"] != row or len(s["levels"]) != index["levels"]:
            raise ValueError(f"feature cache index: scene {s['sample_idx']} does not follow its predecessor")
        row += sum(int(h) * int(w) for h, w in s["levels"])
    if row != index["rows"] or sum(f["rows"] for f in index["files"]) != row:
        raise ValueError("feature cache index: the scenes' rows, the files' rows and the total disagree")
    return index


def scene_geometry(ori_shape, img_scale, pad_divisor, level_shapes):
    """(h, w) of the stored image -> (img_shape (h, w), padded (Hp, Wp), own level shapes)."""
    m = resize_meta({}, (int(ori_shape[0]), int(ori_shape[1])), img_scale, pad_divisor)
    nh, nw = m["img_shape"][:2]
    padded = (pad_to(nh, pad_divisor), pad_to(nw, pad_divisor))
    return (int(nh), int(nw)), padded, [tuple(s) for s in level_shapes(padded)]


def arena_rows(ori_shapes, img_scale=(1333, 800), pad_divisor=32, level_shapes=None):
    """Rows of arena the scenes of ``ori_shapes`` [(h, w)] need (x C x element size = bytes), from shapes alone."""
    if level_shapes is None:
        from .modules.image_stream import pyramid_level_shapes as level_shapes
    return sum(h * w for o in ori_shapes for h, w in scene_geometry(o, img_scale, pad_divisor, level_shapes)[2])


def _image_size(path):
    """(h, w) of an image file from its header (nothing is decoded)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return int(h), int(w)


# ---- the cache --------------------------------------------------------------------------------------------------------
class FeatureCache:
    """Device-resident encoder tokens of every scene of one dataset, for one model's frozen image branch."""

    def __init__(self, model, index, arena):
        self.model, self.index, self.arena = model, index, arena
        self.dtype, self.channels, self.levels = index["dtype"], int(index["C"]), int(index["levels"])
        self.img_scale, self.pad_divisor = tuple(index["img_scale"]), int(index["pad_divisor"])
        rows = [[s["row0"]] + [int(v) for hw in s["levels"] for v in hw] for s in index["scenes"]]
        self.table_host = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 1 + 2 * self.levels)
        self.table = self.table_host.to(arena.device)
        self.ori_shapes = {i: tuple(s["ori_shape"]) for i, s in enumerate(index["scenes"])}
        self._shapes = {}

    def __len__(self):
        return len(self.index["scenes"])

    @property
    def nbytes(self):
        return self.arena.numel() * self.arena.element_size()

    # ---- building ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _level_fn(model):
        from .modules.image_stream import pyramid_level_shapes
        return lambda padded: pyramid_level_shapes(padded, model.img_backbone, model.img_neck)

    @staticmethod
    def _fingerprint(model, dtype, channels, img_scale, pad_divisor, img_norm=ops.IMG_NORM):
        return fingerprint(image_state(model), dtype, channels, img_scale, pad_divisor, img_norm,
                           ops.get_compute_dtype())

    @classmethod
    def build(cls, model, dataset, img_scale=(1333, 800), dtype="fp32", max_bytes=None, pad_divisor=32,
              device=None):
        """Walk ``dataset`` in order, prepare every image as ``ScenePipeline`` does (decode, ``ops.image_prep`` with
        ``ops.IMG_NORM``, pad 32), run the image stream at B = 1 in eval mode and keep the rows.  The bytes needed are
        known from the image files' headers before anything is allocated: more than ``max_bytes`` (default: the free
        device memory minus ``RESERVE_BYTES``) raises ``MemoryError`` with the figure - the cache never spills."""
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        C = int(model.img_encoder.embed_dims)
        levels_of = cls._level_fn(model)
        scenes, row = [], 0
        for i in range(len(dataset)):
            info = dataset.get_data_info(i)
            ori = _image_size(info["img_filename"])
            img_shape, _, levels = scene_geometry(ori, img_scale, pad_divisor, levels_of)
            scenes.append(dict(sample_idx=int(info["sample_idx"]), ori_shape=list(ori), img_shape=list(img_shape),
                               levels=[list(s) for s in levels], row0=row))
            row += sum(h * w for h, w in levels)
        tdt = DTYPES[dtype]
        need = row * C * torch.empty((), dtype=tdt).element_size()
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(device)[0] - RESERVE_BYTES
        if need > max_bytes:
            raise MemoryError(f"the feature cache of {len(scenes)} scenes needs {need} bytes ({row} rows x {C} "
                              f"channels, {dtype}); {max(int(max_bytes), 0)} are allowed")
        arena = torch.empty((row, C), dtype=tdt, device=device)
        was_training = model.training
        model.eval()
        try:
            pipe = ScenePipeline(dataset, "test", img_scale, pad_divisor=pad_divisor)
            for i, s in enumerate(scenes):
                info = dataset.get_data_info(i)
                tokens, spatial = cls._scene_tokens(model, pipe, info, s, device)
                if [list(sp) for sp in spatial] != s["levels"] or tokens.shape[1] != C:
                    raise RuntimeError(f"scene {s['sample_idx']}: the stream's levels {spatial} x {tokens.shape[1]} are "
                                       f"not the {s['levels']} x {C} its shape predicts")
                n = tokens.shape[0]
                arena[s["row0"]:s["row0"] + n].copy_(tokens)          # (fp32 -> bf16: round to nearest even)
        finally:
            model.train(was_training)
        index = dict(version=LAYOUT_VERSION, dtype=dtype, C=C, levels=len(scenes[0]["levels"]) if scenes else 0,
                     img_scale=[int(v) for v in img_scale], pad_divisor=int(pad_divisor), rows=row,
                     fingerprint=cls._fingerprint(model, dtype, C, img_scale, pad_divisor), files=[], scenes=scenes)
        return cls(model, index, arena)

    @staticmethod
    def _scene_tokens(model, pipe, info, scene, device):
        """One scene alone through the stream -> ((rows, C) fp32 tokens, level shapes)."""
        img = pipe.read_image(info["img_filename"])
        if list(img.shape[:2]) != list(scene["ori_shape"]):
            raise RuntimeError(f"{info['img_filename']}: decoded as {img.shape[:2]}, its header said {scene['ori_shape']}")
        h, w = img.shape[:2]
        nh, nw = scene["img_shape"]
        padded = (pad_to(nh, pipe.pad_divisor), pad_to(nw, pipe.pad_divisor))
        src = torch.from_numpy(np.array(img, copy=True).reshape(-1)).to(device)      # (PIL's array is read-only)
        off = torch.tensor([0, img.size], dtype=torch.int64, device=device)
        shp = torch.tensor([[h, w, nh, nw]], dtype=torch.int32, device=device)
        x = ops.image_prep(src, off, shp, padded, *pipe.img_norm)
        meta = dict(img_shape=(nh, nw, 3), ori_shape=(h, w, 3), pad_shape=padded + (3,), batch_input_shape=padded)
        out = model.extract_img_feat(x, [meta])
        return out["tokens"][0], [tuple(sp) for sp in out["spatial"]]

    def verify(self):
        """Raise ``ValueError`` unless the model's image branch (and the compute dtype) still are what the entries
        were computed with - e.g. after weights were loaded into the model."""
        now = self._fingerprint(self.model, self.dtype, self.channels, self.img_scale, self.pad_divisor)
        if now != self.index["fingerprint"]:
            raise ValueError("the feature cache no longer matches the model's image branch or the compute dtype "
                             "(were weights loaded after it was built?)")

    # ---- host metadata ----------------------------------------------------------------------------------------------
    def meta_entries(self, index):
        """The recorded 2-D meta of dataset index ``index``: sample_idx, ori_shape, img_shape, scale_factor, pad_shape,
        batch_input_shape (of the scene alone) and its own level shapes."""
        s = self.index["scenes"][int(index)]
        m = resize_meta(dict(sample_idx=s["sample_idx"]), tuple(s["ori_shape"]), self.img_scale, self.pad_divisor)
        m["pad_shape"] = tuple(m["batch_input_shape"]) + (3,)
        m["levels"] = [tuple(hw) for hw in s["levels"]]
        return m

    def entry(self, index):
        """Scene ``index``'s stored rows, (sum h_l w_l, C), a view of the arena."""
        s = self.index["scenes"][int(index)]
        return self.arena[s["row0"]:s["row0"] + sum(h * w for h, w in s["levels"])]

    # ---- a batch ----------------------------------------------------------------------------------------------------
    def level_shapes(self, padded):
        padded = (int(padded[0]), int(padded[1]))
        if padded not in self._shapes:
            self._shapes[padded] = self._level_fn(self.model)(padded)
        return self._shapes[padded]

    def assemble(self, indices, img_metas, out=None):
        """The ``img_features`` of the batch of dataset ``indices`` (a host sequence) whose collated metas are
        ``img_metas``: the batch's level shapes are those of ``img_metas[0]["batch_input_shape"]``.  With the head's
        sample-then-project attention: ``dict(tokens, spatial, padding_zeroed=True)``, the head's padding mask of these
        metas applied in the same launch, bf16 rows exactly when ``head.BF16_TOKENS``, the bf16 compute mode and bf16
        storage all hold.  Otherwise ``dict(tokens, spatial)`` with fp32 rows and no mask
        (``prepare_image_inputs`` masks as it does for the stream's tokens).  ``out``: the dict of an earlier call of
        the same shapes, overwritten in place."""
        from .modules import head as head_mod
        idx = [int(i) for i in indices]
        if len(idx) != len(img_metas):
            raise ValueError(f"{len(idx)} indices for {len(img_metas)} metas")
        for i, m in zip(idx, img_metas):
            if not 0 <= i < len(self):
                raise IndexError(f"scene index {i} is outside the cache of {len(self)} scenes")
            if "sample_idx" in m and int(m["sample_idx"]) != int(self.index["scenes"][i]["sample_idx"]):
                raise ValueError(f"index {i} is scene {self.index['scenes'][i]['sample_idx']} in the cache, "
                                 f"{m['sample_idx']} in the batch")
        spatial = self.level_shapes(img_metas[0]["batch_input_shape"])
        S = sum(h * w for h, w in spatial)
        head = self.model.pts_bbox_head
        dev = self.arena.device
        # (B words from pinned memory: a pageable upload would make the host wait for the step in flight)
        ih = torch.tensor(idx, dtype=torch.int64).pin_memory()
        idx_d = ih.to(dev, non_blocking=True)
        if out is not None and [tuple(s) for s in out["spatial"]] != [tuple(s) for s in spatial]:
            raise ValueError("assemble: `out` holds levels %s, the batch has %s" % (out["spatial"], spatial))
        buf = None if out is None else out["tokens"]
        if head._sample_first(True, self.channels, S):
            mask = head._meta_tensors(img_metas, spatial, dev, torch.float32)["mask_u8"]
            bf16 = bool(head_mod.BF16_TOKENS and ops.get_compute_dtype() == "bf16" and self.dtype == "bf16")
            tokens = ops.assemble_tokens(self.arena, self.table, idx_d, spatial, mask, bf16=bf16, out=buf,
                                         table_host=self.table_host, indices_host=ih)
            return out if out is not None else dict(tokens=tokens, spatial=list(spatial), padding_zeroed=True)
        tokens = ops.assemble_tokens(self.arena, self.table, idx_d, spatial, None, bf16=False, out=buf,
                                     table_host=self.table_host, indices_host=ih)
        return out if out is not None else dict(tokens=tokens, spatial=list(spatial))

    # ---- disk -------------------------------------------------------------------------------------------------------
    def _file_plan(self):
        """Whole scenes per data file, at most MAX_FILE_BYTES each -> [dict(name, rows, bytes)]."""
        row_bytes = self.channels * self.arena.element_size()
        files, rows = [], 0
        for s in self.index["scenes"]:
            n = sum(h * w for h, w in s["levels"])
            if rows and (rows + n) * row_bytes > MAX_FILE_BYTES:
                files.append(rows)
                rows = 0
            rows += n
        if rows or not files:
            files.append(rows)
        return [dict(name=f"tokens_{k:03d}.bin", rows=r, bytes=r * row_bytes) for k, r in enumerate(files)]

    def _words(self):
        """The arena as raw storage words: fp32 as it is, bf16 as int16-sized words (uint16 on disk)."""
        return self.arena.view(torch.int16) if self.arena.dtype == torch.bfloat16 else self.arena

    def save(self, directory):
        """``index.json`` + the data files under ``directory``; every file is written under a temporary name and
        renamed into place, the index last (a reader sees the old cache or the whole new one)."""
        os.makedirs(directory, exist_ok=True)
        files = self._file_plan()
        words = self._words().reshape(-1)
        per_row = self.channels
        stage = torch.empty((max(CHUNK_BYTES // words.element_size(), 1),), dtype=words.dtype, pin_memory=True)
        at = 0
        for f in files:
            tmp = os.path.join(directory, f["name"] + ".tmp")
            with open(tmp, "wb") as fh:
                end = at + f["rows"] * per_row
                while at < end:
                    n = min(stage.numel(), end - at)
                    stage[:n].copy_(words[at:at + n])
                    fh.write(stage[:n].numpy().tobytes())
                    at += n
            os.replace(tmp, os.path.join(directory, f["name"]))
        index = dict(self.index, files=files)
        tmp = os.path.join(directory, INDEX_FILE + ".tmp")
        with open(tmp, "w") as fh:
            fh.write(index_to_json(index))
        os.replace(tmp, os.path.join(directory, INDEX_FILE))
        return directory

    @classmethod
    def load(cls, directory, model, dataset, device=None):
        """Read a saved cache for ``model`` and ``dataset`` through a pinned staging buffer in chunks of
        ``CHUNK_BYTES``.  Raises ``ValueError`` when the fingerprint is not this model's, when the dataset's
        ``sample_idx`` list differs from the recorded one, or when a data file does not have its recorded size."""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with open(os.path.join(directory, INDEX_FILE)) as fh:
            index = index_from_json(fh.read())
        want = cls._fingerprint(model, index["dtype"], index["C"], index["img_scale"], index["pad_divisor"])
        if want != index["fingerprint"]:
            raise ValueError(f"{directory}: the cache was built for another image branch, storage or compute setting "
                             f"(fingerprint {index['fingerprint'][:12]}.., this model {want[:12]}..)")
        have = [int(dataset.get_data_info(i)["sample_idx"]) for i in range(len(dataset))]
        if have != [int(s["sample_idx"]) for s in index["scenes"]]:
            raise ValueError(f"{directory}: the dataset's scenes are not the {len(index['scenes'])} recorded ones, in "
                             "their order")
        tdt = DTYPES[index["dtype"]]
        for f in index["files"]:
            size = os.path.getsize(os.path.join(directory, f["name"]))
            if size != f["bytes"]:
                raise ValueError(f"{directory}/{f['name']}: {size} bytes, the index records {f['bytes']}")
        arena = torch.empty((index["rows"], index["C"]), dtype=tdt, device=device)
        words = (arena.view(torch.int16) if tdt == torch.bfloat16 else arena).reshape(-1)
        esize = words.element_size()
        stage = torch.empty((max(CHUNK_BYTES // esize, 1),), dtype=words.dtype, pin_memory=True)
        stage_np = stage.numpy()
        at = 0
        for f in index["files"]:
            with open(os.path.join(directory, f["name"]), "rb") as fh:
                left = f["bytes"] // esize
                while left:
                    n = min(stage.numel(), left)
                    got = fh.readinto(memoryview(stage_np[:n]).cast("B"))
                    if got != n * esize:
                        raise ValueError(f"{directory}/{f['name']}: the file ends early")
                    words[at:at + n].copy_(stage[:n])          # (synchronous: the buffer is free again afterwards)
                    at += n
                    left -= n
        return cls(model, index, arena)
