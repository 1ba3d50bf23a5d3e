"""Device time of the scene input pipeline kernels (csrc/pipeline.hip) at SUN RGB-D sizes, and the loader's scenes/s.

Kernels, with device events, best of --reps, after upload, at B = 8 and 16: ~50 000 raw 6-float records per scene,
20 000 sampled points, images of 530x730 / 427x561 / 441x591 mixed in a batch -> Resize(1333, 800) -> 800x1120.
Each kernel's shape-derived byte count and its time at --bw TB/s (the measured copy rate) are printed, with the
kernel's fraction of that bound.  The loader: a synthetic on-disk dataset (.bin + JPEG + infos) read through
pipeline.SceneLoader with W host threads; scenes/s over one epoch after a warm-up batch, and the bytes uploaded per
batch.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

IMG_SIZES = ((530, 730), (427, 561), (441, 591))


def _pad32(n):
    return -(-n // 32) * 32


def kernels(B, n_raw, k, reps, bw):
    from demf_amd import ops
    from demf_amd import pipeline as pl
    from demf_amd.data import resize_meta
    rng = np.random.default_rng(B)
    raw = rng.uniform(-3, 3, size=(B * n_raw, 6)).astype(np.float32)
    off = np.arange(B + 1, dtype=np.int64) * n_raw
    params = np.stack([pl.param_row(pl.draw_aug_params(rng)) for _ in range(B)])
    seeds = rng.integers(0, 2 ** 62, size=B)
    hw = [IMG_SIZES[b % 3] for b in range(B)]
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in hw]
    outs = [resize_meta({}, s, (1333, 800))["img_shape"][:2] for s in hw]
    Hp, Wp = max(_pad32(o[0]) for o in outs), max(_pad32(o[1]) for o in outs)
    ioff = np.concatenate([[0], np.cumsum([i.size for i in imgs])]).astype(np.int64)
    shp = np.array([[*s, *o] for s, o in zip(hw, outs)], np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    raw_d, off_d, prm_d, seeds_d = up(raw), up(off), up(params), up(seeds.astype(np.int64))
    img_d, ioff_d, shp_d = up(np.concatenate([i.reshape(-1) for i in imgs])), up(ioff), up(shp)
    floor = ops.points_floor(raw_d, off_d)
    pts = ops.points_prep(raw_d, off_d, floor, prm_d, seeds_d, k)
    img = ops.image_prep(img_d, ioff_d, shp_d, (Hp, Wp))
    torch.cuda.synchronize()
    best = [float("inf")] * 3
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        ops.points_floor(raw_d, off_d)
        ev[1].record()
        ops.points_prep(raw_d, off_d, floor, prm_d, seeds_d, k, out=pts)
        ev[2].record()
        ops.image_prep(img_d, ioff_d, shp_d, (Hp, Wp), out=img)
        ev[3].record()
        torch.cuda.synchronize()
        best = [min(b, ev[i].elapsed_time(ev[i + 1])) for i, b in enumerate(best)]
    # shape-derived bytes: the records once (the 4 radix passes re-read them from L2); k sampled records (a 24-byte
    # record touches one or two 64-byte segments: counted as 64) + the (B,k,4) output; the uint8 source + the fp32 output
    nb = {"floor": B * n_raw * 24, "prep": B * k * (64 + 16), "image": int(img_d.numel()) + B * 3 * Hp * Wp * 4}
    res = {}
    for (name, b), ms in zip(nb.items(), best):
        bound_us = b / (bw * 1e12) * 1e6
        res[name] = dict(us=round(ms * 1e3, 2), bytes=b, bound_us=round(bound_us, 2),
                         fraction_of_bound=round(bound_us / (ms * 1e3), 3))
    res["pad_shape"] = [Hp, Wp]
    return res


def loader(workers, B, tmp):
    from demf_amd.dataset import SUNRGBDDataset
    from demf_amd.pipeline import SceneLoader
    ds = SUNRGBDDataset(tmp, "sunrgbd_infos_train.pkl")
    ld = SceneLoader(ds, B, "train", seed=0, workers=workers, drop_last=True)
    it = iter(ld)
    next(it)                                                # warm-up: pinned pool, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch in it:
        n += len(batch.indices)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(workers=workers, scenes=n, scenes_per_s=round(n / dt, 1), upload_mb_per_batch=round(ld.last_upload_bytes / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw-points", type=int, default=50000)
    ap.add_argument("--num-points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bw", type=float, default=6.29, help="copy rate in TB/s the bound is taken at")
    ap.add_argument("--scenes", type=int, default=136)
    ap.add_argument("--workers", default="4,8,16")
    a = ap.parse_args()
    out = {"kernels": {f"B{B}": kernels(B, a.raw_points, a.num_points, a.reps, a.bw) for B in (8, 16)}}
    import pipeline_reference as ref
    with tempfile.TemporaryDirectory() as tmp:
        ref.write_dataset(tmp, [(a.raw_points, IMG_SIZES[i % 3], 1 + i % 5) for i in range(a.scenes)], jpeg=True)
        out["loader_B8"] = [loader(int(w), 8, tmp) for w in a.workers.split(",")]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
