"""The test loop and its command line: what the reference's ``eval.py --eval mAP`` does (README.md:43-46).

  python -m demf_amd.infer --data-root R --ann-file sunrgbd_infos_val.pkl --checkpoint C
                           [--batch-size 8] [--workers 8] [--out results.pkl] [--no-eval] [--model {demf,votenet}]
                           [--tta-scales 0.9,1.0,1.1] [--tta-flip] [--tta-mode bev|3d|aligned] [--tta-nms-thr T]
                           [--gpus N]
  python -m demf_amd.infer --data-root R --frames manifest.json --checkpoint C --out results.pkl
  python -m demf_amd.infer --model detr2d --data-root R (--ann-file F | --frames M) --checkpoint C --out results.pkl
                           [--score-thr 0.09] [--max-per-img 100]

``--model detr2d`` runs the image branch's 2D detector (``modules.Detr2D``, a stage-1 checkpoint) over the images and
pickles mmdet's per-class ``bbox2result`` lists; no 2D metric is built, so nothing is evaluated and ``--out`` is
required; ``--gpus``, ``--tta-*`` and ``--feature-cache`` do not apply to it.

``--frames`` runs raw RGB-D frames (``dataset.RGBDFrames``: colour image, 16-bit depth PNG, calibration) through
``pipeline.FramePipeline``; they carry no ground truth, so nothing is evaluated and ``--out`` is required.

``run_test`` feeds a dataset through ``SceneLoader(mode="test")`` and ``DeMFVoteNet.predict_into``; the
detections of every scene stay on the device in one ``DetectionStore`` and nothing in the loop waits for the
GPU, so the loader's one-batch-ahead overlap holds.

``--gpus N`` starts N ranks of this module (``ranks.launch``; the reference's ``multi_gpu_test``); under a launcher
(``RANK`` in the environment) ``main`` joins the process group instead.  Every rank then runs a contiguous shard of
the dataset into a store of its own, ``ranks.merge_stores`` leaves all detections in dataset order in one store on
every rank, and rank 0 alone evaluates, prints and writes ``--out``.  Without either: single process, one GPU.

``--tta-scales`` / ``--tta-flip`` turn on test-time augmentation (tta.py): every scene is prepared in V views (scale-
major, the unflipped view before the flipped one), the image stream runs once per scene, the head once per view, and
the views' detections are merged on the device by a per-class rotated NMS.  It works with ``--model votenet`` and with
``--frames``.  No accuracy figure has been measured with it.
"""
import argparse
import json
import os
import pickle
import sys

import torch

from . import ranks
from .detections import DetectionStore
from .pipeline import SceneLoader


def run_test(model, dataset, batch_size=8, workers=8, num_points=20000, img_scale=(1333, 800), seed=0,
             store=None, pipeline=None, tta=None):
    """Detections of every scene of ``dataset`` in dataset order -> the ``DetectionStore`` holding them (``store``,
    or a new worst-case one).  The last batch may be smaller; there is no host sync inside the loop.  ``pipeline``:
    a test-mode pipeline instance for the loader to use (``FramePipeline`` for raw frames), which then brings its
    own ``num_points`` / ``img_scale`` / ``seed`` (and its own ``tta``).  ``tta``: a ``tta.TTACfg``; the loader then
    prepares every scene's views, one view store of V * batch_size scenes is allocated once and reused, and every
    batch goes through ``aug_predict_into``.

    In a process group of W > 1 ranks every rank runs its test shard (``pipeline.shard_chunks``) and gets the MERGED
    store back, all scenes in dataset order (``store`` must then be None); ``tta`` and ``pipeline`` shard the same
    scene list."""
    # (a model without an image stream - modules.VoteNet - is fed points alone: no image is read, decoded or uploaded)
    world, rank = ranks.world(), ranks.rank()
    loader = SceneLoader(dataset, batch_size, "test", seed=seed, img_scale=img_scale, num_points=num_points,
                         workers=workers, pipeline=pipeline,
                         with_img=hasattr(model, "extract_img_feat") if pipeline is None else None,
                         tta=tta if pipeline is None else None, rank=rank, world=world)
    if pipeline is not None and tta is not None and pipeline.tta != tta:
        raise ValueError("the given pipeline was built with another tta than run_test is asked for")
    tta = loader.pipeline.tta
    model.eval()
    if _is_detr2d(model):
        # the 2D detector: images alone matter (the loader still reads and prepares the points - skipping them would
        # change its batches for the other models - and predict_into ignores them); rows into a Detection2DStore
        if world > 1 or tta is not None:
            raise ValueError("the 2D detector runs in one process and without test-time augmentation")
        from .detections import Detection2DStore
        if store is None:
            store = Detection2DStore(max(len(dataset), 1), k=model.img_bbox_head.max_per_img, device=loader.device)
        for batch in loader:
            model.predict_into(store, **batch)
        return store
    if world > 1:
        # this rank's contiguous shard into a store of the common capacity (q scenes, worst-case rows: known from
        # the model's configuration, so an empty shard allocates it too), then the ranks' stores merged in rank
        # order = dataset order, on every rank
        if store is not None:
            raise ValueError("run_test under ranks returns the merged store: it does not take one to append to")
        n = len(dataset)
        q = -(-n // world)
        counts = [max(0, min(n, (r + 1) * q) - r * q) for r in range(world)]
        cap = max(q, 1)
        store = DetectionStore(cap, max_rows=cap * ranks.rows_per_scene(model, tta), device=loader.device)
    elif store is None:
        store = DetectionStore(max(len(dataset), 1), device=loader.device)
    if tta is None:
        for batch in loader:
            model.predict_into(store, **batch)
    else:
        view_store = DetectionStore(tta.num_views * int(batch_size), device=loader.device)
        for batch in loader:
            model.aug_predict_into(store, **batch, tta=tta, view_store=view_store)
    return ranks.merge_stores(store, counts) if world > 1 else store


def _is_detr2d(model):
    from .modules.detr2d import Detr2D
    return isinstance(model, Detr2D)


def _model_state(ckpt):
    """The model's state dict inside an mmcv checkpoint ({"state_dict": ...}, what the reference publishes), a
    ``Trainer.state_dict()`` ({"model": ...}) or a bare state dict."""
    if not isinstance(ckpt, dict):
        raise ValueError(f"a checkpoint is a dict, got {type(ckpt).__name__}")
    for key in ("state_dict", "model"):
        if isinstance(ckpt.get(key), dict):
            return ckpt[key]
    if ckpt and all(isinstance(v, torch.Tensor) for v in ckpt.values()):
        return ckpt
    raise ValueError("checkpoint layout not recognised: expected {'state_dict': ...}, {'model': ...} or a state dict")


def load_checkpoint(model, path):
    """Load the weights at ``path`` into ``model`` through its ``load_state_dict`` (for ``DeMFVoteNet`` that
    applies the stage-1 key remap).  Missing or unexpected keys are an error."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(_model_state(ckpt), strict=True)
    return model


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m demf_amd.infer", description=__doc__.split("\n")[0])
    p.add_argument("--data-root", required=True)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--ann-file", help="infos file, absolute or relative to --data-root")
    src.add_argument("--frames", help="JSON manifest of raw RGB-D frames, absolute or relative to --data-root; "
                                      "no ground truth: implies --no-eval and needs --out")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--workers", type=int, default=8)
    p.add_argument("--out", default=None, help="pickle the per-scene results (the reference's --out)")
    p.add_argument("--no-eval", action="store_true", help="do not evaluate (then --out is required)")
    p.add_argument("--model", choices=("demf", "votenet", "detr2d"), default="demf",
                   help="demf: DeMFVoteNet; votenet: the points-only class-agnostic baseline (modules.VoteNet); "
                        "detr2d: the image branch's 2D detector (modules.Detr2D) from a stage-1 checkpoint - no 2D "
                        "metric exists, so --out is required and nothing is evaluated")
    p.add_argument("--score-thr", type=float, default=None,
                   help="--model detr2d: keep detections with a score above this (default 0.09, the reference's filter)")
    p.add_argument("--max-per-img", type=int, default=None,
                   help="--model detr2d: detections selected per image before the score filter (default 100)")
    p.add_argument("--tta-scales", default=None,
                   help="test-time augmentation: comma-separated point-cloud scale ratios, e.g. 0.9,1.0,1.1")
    p.add_argument("--tta-flip", action="store_true",
                   help="test-time augmentation: add the horizontally flipped view of every scale")
    p.add_argument("--tta-mode", choices=("bev", "3d", "aligned"), default="bev",
                   help="overlap of the merging NMS: rotated BEV (default), rotated 3-D, axis-aligned BEV")
    p.add_argument("--tta-nms-thr", type=float, default=None,
                   help="IoU threshold of the merging NMS (default: the head's test_cfg nms_thr)")
    p.add_argument("--gpus", type=int, default=None,
                   help="run as N ranks, one GPU each (started here unless a launcher already set RANK); "
                        "--workers is per rank")
    args = p.parse_args(argv)
    if args.batch_size < 1 or args.workers < 1:
        p.error("--batch-size and --workers must be positive")
    if args.gpus is not None and args.gpus < 1:
        p.error("--gpus must be positive")
    args.tta = None
    if args.tta_scales is not None or args.tta_flip:
        from .tta import TTACfg
        try:
            scales = tuple(float(x) for x in (args.tta_scales or "1.0").split(","))
            args.tta = TTACfg(scales=scales, flip=args.tta_flip, nms_thr=args.tta_nms_thr, mode=args.tta_mode)
        except ValueError as e:
            p.error(f"--tta-scales / --tta-flip: {e}")
    elif args.tta_nms_thr is not None or args.tta_mode != "bev":
        p.error("--tta-mode and --tta-nms-thr go with --tta-scales / --tta-flip")
    if args.model == "detr2d":
        if args.gpus is not None:
            p.error("--model detr2d runs in one process: --gpus is not supported")
        if args.tta is not None:
            p.error("--model detr2d has no test-time augmentation: --tta-scales / --tta-flip are not supported")
        if not args.out:
            p.error("--model detr2d: no 2D metric is built, nothing is evaluated: --out is required")
        args.no_eval = True
        args.score_thr = 0.09 if args.score_thr is None else args.score_thr
        args.max_per_img = 100 if args.max_per_img is None else args.max_per_img
        if args.max_per_img < 1:
            p.error("--max-per-img must be positive")
    elif args.score_thr is not None or args.max_per_img is not None:
        p.error("--score-thr and --max-per-img go with --model detr2d")
    if args.frames:
        args.no_eval = True
        if not args.out:
            p.error("--frames has no ground truth to evaluate against: --out is required")
    if args.no_eval and not args.out:
        p.error("--no-eval without --out would discard the detections")
    return args


def main(argv=None, model=None, **loader_kwargs):
    """-> the ``indoor_eval`` dict (None with ``--no-eval``), also printed as one JSON line.  ``model``: the
    detector to use instead of the full-size ``DeMFVoteNet()``; ``loader_kwargs`` go to ``run_test``
    (``num_points``, ``img_scale``, ``seed``)."""
    args = parse_args(argv)
    if "RANK" in os.environ:
        from . import engine
        ranks.check_gpus(args.gpus)
        engine.init_distributed()
    elif args.gpus is not None and args.gpus > 1:
        if model is not None or loader_kwargs:
            raise ValueError("--gpus starts new processes: a model or loader arguments given in this one cannot follow")
        return ranks.launch("demf_amd.infer", sys.argv[1:] if argv is None else list(argv), args.gpus)
    from .dataset import RGBDFrames, SUNRGBDDataset
    if args.frames:
        from .pipeline import FramePipeline
        dataset = RGBDFrames(args.data_root, args.frames)
        loader_kwargs["pipeline"] = FramePipeline(dataset, tta=args.tta,
                                                  **{k: loader_kwargs.pop(k) for k in
                                                     ("num_points", "img_scale", "seed") if k in loader_kwargs})
    else:
        dataset = SUNRGBDDataset(args.data_root, args.ann_file, test_mode=True)
    if model is None:
        from .modules import DeMFVoteNet, Detr2D, VoteNet
        model = VoteNet() if args.model == "votenet" else \
            Detr2D(max_per_img=args.max_per_img) if args.model == "detr2d" else DeMFVoteNet()
    if (args.model == "detr2d") != _is_detr2d(model):
        raise ValueError("--model detr2d goes with a modules.Detr2D, and only with one")
    load_checkpoint(model, args.checkpoint)
    model.cuda()
    if args.model == "detr2d":
        from .detections import Detection2DStore
        model.img_bbox_head.max_per_img = args.max_per_img
        store = run_test(model, dataset, batch_size=args.batch_size, workers=args.workers,
                         store=Detection2DStore(max(len(dataset), 1), k=args.max_per_img, score_thr=args.score_thr),
                         **loader_kwargs)
        with open(args.out, "wb") as f:
            pickle.dump(store.results(per_class=True, num_classes=model.img_bbox_head.num_classes), f)
        print("--model detr2d: %d images written to %s; not evaluated (no 2D metric is built)"
              % (len(store), args.out))
        return None
    store = run_test(model, dataset, batch_size=args.batch_size, workers=args.workers, tta=args.tta,
                     **loader_kwargs)
    if ranks.rank() != 0:                       # (the merged store is on every rank; rank 0 alone reports)
        return None
    if args.out:
        with open(args.out, "wb") as f:
            pickle.dump(store.results(), f)
    if args.no_eval:
        return None
    ret = dataset.evaluate(store)
    print(json.dumps(ret))
    return ret


if __name__ == "__main__":
    _ret = main(sys.argv[1:])
    sys.exit(_ret if isinstance(_ret, int) else 0)
