"""Times of the 2D detector's test side at the reference size -> profiles/detr2d_bench.json.

  python tools/bench_detr2d.py [--batch 8] [--height 800] [--width 1120] [--iters 20] [--repeats 3] [--out F]

B = 8 images of the reference's scale (1333, 800) - SUN RGB-D's 530 x 730 frames become 800 x 1102, padded to
800 x 1120: S = 18 609 tokens - through the full-size ``Detr2D`` (ResNet-50, 6 encoder and 6 decoder layers, 300
queries) with seeded random weights.  Timed with device events around ``iters`` calls after a warm-up, ``repeats``
windows per variant, the variants ALTERNATED inside one process so that they see the same machine:

  kernels        decoder + head + select on the kernel path, the six layers' value projections as one launch
  kernels_value6 the same with one value projection per layer (DEMF_DETR2D_VALUE_ONE=0)
  modules        the module path of this commit (ops.linear, torch elementwise; library fall-backs allowed)
  image_stream   backbone + neck + encoder in front of them (once; it is the same for every variant)

and the largest difference between the two paths' outputs at this size.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--height", type=int, default=800)
    p.add_argument("--width", type=int, default=1120)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "detr2d_bench.json"))
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_detr2d.py needs a HIP device: a CPU run measures nothing")
    from demf_amd import _ffi, ops
    from demf_amd.detections import Detection2DStore
    from demf_amd.modules import Detr2D, detr2d
    torch.manual_seed(0)
    B, H, W = args.batch, args.height, args.width
    det = Detr2D().cuda()
    head = det.img_bbox_head
    with torch.no_grad():           # offsets and attention logits that depend on the query, as trained weights do
        for layer in head.transformer.decoder.layers:
            layer.attentions[1].sampling_offsets.weight.normal_(0, 0.02)
            layer.attentions[1].attention_weights.weight.normal_(0, 0.05)
        # class scores on both sides of the filter and boxes that depend on the image (the initialisation's zero last
        # box layer and -4.6 class bias would keep nothing)
        head.cls_branches[0].bias.fill_(-2.0)
        head.cls_branches[0].weight.normal_(0, 0.1)
        head.reg_branches[0][4].weight.normal_(0, 0.05)
    img = torch.randn(B, 3, H, W, device="cuda")
    metas = [dict(img_shape=(H, W - 18 if W > 18 else W, 3), batch_input_shape=(H, W),
                  scale_factor=(1.509, 1.509, 1.509, 1.509)) for _ in range(B)]
    store = Detection2DStore(B, k=head.max_per_img)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    ops.LIBRARY_FALLBACK = False
    enc = det.extract_img_feat(img, metas)              # (also the warm-up of the image stream)
    stream_ms = [timed(lambda: det.extract_img_feat(img, metas), 3) for _ in range(args.repeats)]
    st = det.img_encoder._static(metas, enc["spatial"], enc["tokens"].device)
    S = enc["tokens"].shape[1]

    def tail(fused, value_one, fallback):
        def run():
            detr2d.FUSED, detr2d.VALUE_ONE_LAUNCH, ops.LIBRARY_FALLBACK = fused, value_one, fallback
            store.reset()
            _, logits, boxes = head(enc, st)
            det._select(logits, boxes, metas, store.score_thr, False, store)
            return logits, boxes
        return run
    variants = dict(kernels=tail(True, True, False), kernels_value6=tail(True, False, False),
                    modules=tail(False, False, True))
    outs, launches = {}, {}
    real = _ffi.call
    for name, fn in variants.items():                   # warm-up, outputs, library calls per batch
        fn()
        n = [0]

        def counting(*a, _n=n):
            _n[0] += 1
            return real(*a)
        _ffi.call = counting
        try:
            outs[name] = [t.clone() for t in fn()]
        finally:
            _ffi.call = real
        launches[name] = n[0]
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            times[name].append(timed(fn, args.iters))
    detr2d.FUSED, detr2d.VALUE_ONE_LAUNCH, ops.LIBRARY_FALLBACK = True, True, False
    res = store.results()
    diff = {name: dict(logits=float((outs[name][0] - outs["modules"][0]).abs().max()),
                       boxes=float((outs[name][1] - outs["modules"][1]).abs().max()))
            for name in ("kernels", "kernels_value6")}
    out = dict(device=torch.cuda.get_device_name(0), batch=B, image=[H, W], tokens=S, queries=head.num_query,
               decoder_layers=len(head.transformer.decoder.layers), iters=args.iters, repeats=args.repeats,
               compute_dtype=ops.get_compute_dtype(),
               decoder_head_select_ms={k: dict(min=min(v), median=sorted(v)[len(v) // 2], all=v) for k, v in times.items()},
               image_stream_ms=dict(min=min(stream_ms), median=sorted(stream_ms)[len(stream_ms) // 2], all=stream_ms),
               library_entry_calls_per_batch=launches, max_abs_diff_vs_modules=diff,
               detections_kept=[int(len(r)) for r in res])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
