"""Measure the frozen image-feature cache (demf_amd/featcache.py, csrc/featcache.hip) on one GPU.

    python tools/bench_featcache.py [--parts kernel loop caveat bytes] [--out profiles/featcache_bench.json]

kernel  ``demf_tokens_assemble`` at the reference size: B = 8 and 16 distinct scenes, canvas 800 x 1120, own shapes of
        530x730 / 427x561 / 441x591 images, the four arena x output dtype pairs, with the padding mask.
        Device events, best and median of --reps launches; shape-derived bytes (own rows read + B S C written + the
        mask) and the fraction bytes / --bw TB/s.  ``pyramid_to_tokens_k`` (fp32 maps -> fp32 tokens, same B) is timed
        in the same run the same way: the neighbour to compare with.
loop    loader + captured step with a new batch every step, B = 8, on a synthetic on-disk set of --scenes scenes: (a)
        uncached (JPEG decode, image_prep, image stream), (b) cached with the image-free loader, (c) the captured step
        alone on resident tokens.  Alternating windows of --window-epochs passes each, host clock around a window that
        ends in a synchronise; median and range of ms per step.  (b) - (c) is what assemble + copy + loader cost,
        (a) / (b) the gain.
caveat  a mixed-shape batch: the largest difference on image positions between the cached (alone) tokens and the
        batched stream's, relative to the output scale.
bytes   arena bytes for 5 285 scenes at the reference size, both dtypes (from shapes).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

IMG_SIZES = ((530, 730), (427, 561), (441, 591))
CANVAS = (800, 1120)
TRAIN_SCENES = 5285
DT = ("fp32", "bf16")


def _say(text):
    print("[bench_featcache] " + text, file=sys.stderr, flush=True)


def _events(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return min(us), statistics.median(us)


def _row(us, nbytes, bw):
    bound = nbytes / (bw * 1e12) * 1e6
    return dict(us_best=round(us[0], 2), us_median=round(us[1], 2), bytes=int(nbytes), bound_us=round(bound, 2),
                fraction_of_bound=round(bound / us[0], 3))


def part_kernel(reps, bw):
    import numpy as np
    import torch

    from demf_amd import featcache, ops
    from demf_amd.geometry import level_masks
    from demf_amd.modules.image_stream import pyramid_level_shapes
    dev, C = torch.device("cuda"), 256
    canvas = pyramid_level_shapes(CANVAS)
    S = sum(h * w for h, w in canvas)
    out = {}
    for B in (8, 16):
        geo = [featcache.scene_geometry(IMG_SIZES[b % 3], (1333, 800), 32, pyramid_level_shapes) for b in range(B)]
        rows, at = [], 0
        for _, _, levels in geo:
            rows.append([at] + [v for hw in levels for v in hw])
            at += sum(h * w for h, w in levels)
        table_h = torch.tensor(rows, dtype=torch.int64)
        table, idx_h = table_h.to(dev), torch.arange(B, dtype=torch.int64)
        idx = idx_h.to(dev)
        metas = [dict(img_shape=g[0] + (3,), batch_input_shape=CANVAS) for g in geo]
        mask_h = np.concatenate([m.reshape(B, -1) for m in level_masks(metas, canvas)], 1)
        mask = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
        res = dict(own_rows=at, canvas_rows=B * S, masked_rows=int(mask_h.sum()))
        for adt in DT:
            arena = torch.randn((at, C), device=dev).to(featcache.DTYPES[adt])
            for odt in DT:
                buf = torch.empty((B, S, C), dtype=featcache.DTYPES[odt], device=dev)
                fn = lambda: ops.assemble_tokens(arena, table, idx, canvas, mask, bf16=odt == "bf16", out=buf,     # noqa: E731
                                                 table_host=table_h, indices_host=idx_h)
                nbytes = at * C * arena.element_size() + B * S * C * buf.element_size() + B * S
                res[f"{adt}_to_{odt}"] = _row(_events(fn, reps), nbytes, bw)
            del arena
        feats = [torch.randn((B, C, h, w), device=dev) for h, w in canvas]
        buf = torch.empty((B, S, C), dtype=torch.float32, device=dev)
        res["pyramid_to_tokens_fp32"] = _row(_events(lambda: ops.pyramid_to_tokens(feats, mask, out=buf), reps),
                                             2 * B * S * C * 4 + B * S, bw)
        # what engine.load adds behind assemble: the device copy into the step's static token buffer
        src = torch.empty_like(buf)
        res["static_copy_fp32"] = _row(_events(lambda: buf.copy_(src), reps), 2 * B * S * C * 4, bw)
        out[f"B{B}"] = res
        _say(f"kernel B = {B} done")
        del feats, buf, src
        torch.cuda.empty_cache()
    return out


def _model(seed=1):
    from bench_baseline import _seed_weights
    from demf_amd.modules import DeMFVoteNet
    model = DeMFVoteNet()
    _seed_weights(model, seed)
    return model.cuda().train()


def _lookahead(it):
    from demf_amd.train import _lookahead as la
    return la(it)


def part_loop(model, ds, cache, B, windows, window_epochs, workers):
    import functools

    import torch

    from demf_amd import engine
    from demf_amd.modules import DeMFHotPath
    from demf_amd.pipeline import SceneLoader
    trainer = engine.Trainer(model, lr=1e-4, forward=functools.partial(DeMFHotPath.forward_train, model))
    steppers = dict(uncached=trainer.bucketed(), cached=trainer.bucketed())
    loaders = dict(uncached=SceneLoader(ds, B, "train", seed=0, workers=workers, drop_last=True),
                   cached=SceneLoader(ds, B, "train", seed=0, workers=workers, drop_last=True, with_img=False,
                                      image_shapes=cache.ori_shapes))
    last = {}

    def epoch(name):
        n = 0
        for batch, nxt in _lookahead(loaders[name]):
            sb = dict(points=batch["points"], gt_bboxes_3d=batch["gt_bboxes_3d"], gt_labels_3d=batch["gt_labels_3d"],
                      img_metas=batch["img_metas"])
            if name == "cached":
                sb["img_features"] = cache.assemble(batch.indices, batch["img_metas"])
            else:
                sb["img_features"] = model.extract_img_feat(batch["img"], batch["img_metas"])
            last[name] = steppers[name].step(sb, next_points=None if nxt is None else nxt["points"])
            n += 1
        return n

    def resident(n):
        r = next(iter(steppers["cached"].graphs.values()))
        for _ in range(n):
            last["resident"] = r(next_points=r.static["points"])
        return n
    per_epoch = len(loaders["cached"])
    loops = dict(uncached=lambda: sum(epoch("uncached") for _ in range(window_epochs)),
                 cached=lambda: sum(epoch("cached") for _ in range(window_epochs)),
                 resident=lambda: resident(per_epoch * window_epochs))
    for name in ("uncached", "cached"):            # every shape captured and warm before the first timed window
        epoch(name)
        _say(f"loop {name} warm")
    resident(4)
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(windows):
        for name, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / n * 1e3)
            _say(f"window {name}: {ms[name][-1]:.3f} ms per step")
    res = {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                   last_loss=float(last[k])) for k, v in ms.items()}
    res["steps_per_window"] = per_epoch * window_epochs
    res["graphs"] = {k: dict(s.stats) for k, s in steppers.items()}
    res["cached_minus_resident_ms"] = round(res["cached"]["median_ms"] - res["resident"]["median_ms"], 3)
    res["uncached_over_cached"] = round(res["uncached"]["median_ms"] / res["cached"]["median_ms"], 3)
    return res


def part_caveat(model, ds, cache):
    """Scenes 0, 1, 2 have the three image sizes: one batch of them, cached (alone) against the batched stream."""
    import torch

    from demf_amd.pipeline import ScenePipeline
    idx = [0, 1, 2, 3]
    pipe = ScenePipeline(ds, "test")
    batch, _ = pipe.to_device([pipe.load(i) for i in idx], torch.device("cuda"))
    ref = model.extract_img_feat(batch["img"], batch["img_metas"])
    got = cache.assemble(idx, batch["img_metas"])
    spatial = [tuple(s) for s in ref["spatial"]]
    head = model.pts_bbox_head
    keep = ~head._meta_tensors(batch["img_metas"], spatial, torch.device("cuda"), torch.float32)["mask_u8"].bool()
    scale = ref["tokens"][keep].abs().max().item()
    diff = (got["tokens"].float() - ref["tokens"]).abs()
    per = [diff[b][keep[b]].max().item() for b in range(len(idx))]
    # image positions of the canvas that the scene ALONE does not have (its own level is narrower than the nearest-
    # neighbour mask of the canvas says): zero rows in the cache, values in the batched stream
    inside = torch.zeros_like(keep)
    start, per_level = 0, []
    for l, (H, W) in enumerate(spatial):
        for b, i in enumerate(idx):
            h, w = cache.meta_entries(i)["levels"][l]
            inside[b, start:start + H * W].view(H, W)[:h, :w] = True
        sl = slice(start, start + H * W)
        k = keep[:, sl] & inside[:, sl]
        per_level.append(dict(level=[H, W], max_relative_to_scale=(diff[:, sl][k].max().item() / scale),
                              rms_relative_to_scale=(diff[:, sl][k].pow(2).mean().sqrt().item() / scale)))
        start += H * W
    both = keep & inside
    return dict(pad_shapes=[list(m["pad_shape"][:2]) for m in batch["img_metas"]],
                batch_input_shape=list(batch["img_metas"][0]["batch_input_shape"]), output_scale=scale,
                max_abs_difference_per_scene=per, max_relative_to_scale=max(per) / scale,
                image_positions=int(keep.sum()), image_positions_outside_own_levels=int((keep & ~inside).sum()),
                max_relative_to_scale_inside_own_levels=diff[both].max().item() / scale,
                rms_relative_to_scale_inside_own_levels=diff[both].pow(2).mean().sqrt().item() / scale,
                share_of_values_above_one_percent_of_scale=(diff[both] > 1e-2 * scale).float().mean().item(),
                per_level=per_level, storage=cache.dtype)


def part_bytes():
    from demf_amd import featcache
    rows = featcache.arena_rows([IMG_SIZES[0]]) * TRAIN_SCENES
    return dict(scenes=TRAIN_SCENES, rows=rows, fp32_bytes=rows * 256 * 4, bf16_bytes=rows * 256 * 2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parts", nargs="+", default=["kernel", "loop", "caveat", "bytes"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--bw", type=float, default=6.29, help="copy rate in TB/s the bound is taken at")
    ap.add_argument("--scenes", type=int, default=136)
    ap.add_argument("--raw-points", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-epochs", type=int, default=2)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--cache-dtype", choices=DT, default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    result = {}
    if "bytes" in a.parts:
        result["bytes"] = part_bytes()
    if set(a.parts) & {"kernel", "loop", "caveat"}:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_featcache needs a HIP device: a time taken elsewhere says nothing")
        result["device"] = torch.cuda.get_device_name(0)
    if "kernel" in a.parts:
        result["kernel"] = part_kernel(a.reps, a.bw)
    if set(a.parts) & {"loop", "caveat"}:
        import pipeline_reference as ref

        from demf_amd import featcache
        from demf_amd.dataset import SUNRGBDDataset
        with tempfile.TemporaryDirectory() as tmp:
            ref.write_dataset(tmp, [(a.raw_points, IMG_SIZES[i % 3], 1 + i % 5) for i in range(a.scenes)], jpeg=True)
            ds = SUNRGBDDataset(tmp, "sunrgbd_infos_train.pkl")
            model = _model()
            t0 = time.perf_counter()
            cache = featcache.FeatureCache.build(model, ds, dtype=a.cache_dtype)
            torch.cuda.synchronize()
            _say("cache built")
            result["build"] = dict(scenes=len(cache), bytes=cache.nbytes, dtype=cache.dtype,
                                   seconds=round(time.perf_counter() - t0, 2))
            if "caveat" in a.parts:
                result["caveat"] = part_caveat(model, ds, cache)
            if "loop" in a.parts:
                result["loop"] = part_loop(model, ds, cache, a.batch, a.windows, a.window_epochs, a.workers)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
