"""Training from the frozen image-feature cache: ``train.fit(feature_cache=...)`` with every image file deleted and the
image stream made to raise, eager and captured; the image-free loader against the image loader; the command line."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 5


def _dataset(tmp_path, specs):
    import pipeline_reference as pref
    from demf_amd.dataset import SUNRGBDDataset
    ann, _ = pref.write_dataset(str(tmp_path), specs, jpeg=True)
    return ann, SUNRGBDDataset(str(tmp_path), ann)


def _remove_images(root):
    files = glob.glob(os.path.join(str(root), "sunrgbd_trainval", "image", "*"))
    assert len(files) == 4
    for f in files:
        os.remove(f)


def _never(*a, **k):
    raise AssertionError("the image stream ran in a cached training loop")


@pytest.mark.parametrize("graphs", [False, True])
def test_fit_without_images_or_the_stream(tmp_path, graphs):
    from demf_amd import featcache, infer, train
    from test_gpu_featcache import SPECS, _detector
    from test_gpu_pipeline import IMG_SCALE
    from test_gpu_train import SAME_SIZE, _fit_kwargs
    # ONE image size for the captured run, so that a shape key repeats; two padded shapes for the eager one
    specs = SAME_SIZE if graphs else SPECS
    assert sum(1 for s in specs if s[2] == 0) == 1
    _, ds = _dataset(tmp_path, specs)
    det = _detector()
    cache = featcache.FeatureCache.build(det, ds, img_scale=IMG_SCALE, dtype="fp32")
    _remove_images(tmp_path)
    det.extract_img_feat = _never
    init = {k: v.clone() for k, v in det.state_dict().items()}
    work = str(tmp_path / "work")
    steps = []
    out = train.fit(det, ds, work, val_set=None, graphs=graphs, feature_cache=cache,
                    on_step=lambda info: steps.append((info["indices"], info["loss"].clone())), **_fit_kwargs())
    torch.cuda.synchronize()
    with open(os.path.join(work, "train.log.json")) as f:
        lines = [json.loads(l) for l in f if l.strip()]
    print(json.dumps(lines))
    assert [(l["mode"], l["epoch"], l["iter"]) for l in lines] == [("train", 1, 1), ("train", 1, 2), ("train", 2, 3),
                                                                   ("train", 2, 4)]
    for l in lines:
        assert all(np.isfinite(v) for k, v in l.items() if k != "mode"), l
        assert l["loss"] > 0 and l["grad_norm"] > 0
    assert len(steps) == 4 and all(bool(torch.isfinite(loss)) for _, loss in steps)
    assert sorted(i for idx, _ in steps[:2] for i in idx) == [0, 1, 2, 3]
    if graphs:
        assert out["stepper"].stats["replayed"] > 0 and out["stepper"].stats["captured"] >= 1, out["stepper"].stats
    sd = det.state_dict()
    assert sum(1 for k, v in sd.items() if k.startswith("pts_") and not torch.equal(v, init[k])) > 50
    assert all(torch.equal(v, init[k]) for k, v in sd.items() if k.startswith("img_"))
    fresh = _detector(seed=2)
    infer.load_checkpoint(fresh, os.path.join(work, "epoch_2.pth"))
    for k, v in sd.items():
        assert torch.equal(fresh.state_dict()[k].cpu(), v.cpu()), k
    # a cache of another model, or one whose weights moved underneath it, is refused
    with pytest.raises(ValueError, match="another model"):
        train.fit(fresh, ds, work, val_set=None, feature_cache=cache, **_fit_kwargs())


def test_image_free_loader_equals_the_image_loader(tmp_path):
    from demf_amd import pipeline as pl
    from test_gpu_featcache import SPECS
    from test_gpu_pipeline import IMG_SCALE
    _, ds = _dataset(tmp_path, SPECS)
    shapes = {i: s[1] for i, s in enumerate(SPECS)}
    kw = dict(seed=SEED, img_scale=IMG_SCALE, num_points=2048, workers=2)
    a = pl.SceneLoader(ds, 3, "train", **kw)
    b = pl.SceneLoader(ds, 3, "train", with_img=False, image_shapes=shapes, **kw)
    a.epoch = b.epoch = 3
    want = list(a)
    _remove_images(tmp_path)
    got = list(b)
    from test_featcache_host import _same_meta
    assert len(want) == len(got) == 2
    mixed = 0
    for x, y in zip(want, got):
        assert x.indices == y.indices and "img" in x and "img" not in y
        assert torch.equal(x["points"], y["points"])
        assert ("gt_bboxes_3d" in x) == ("gt_bboxes_3d" in y)
        for k in ("gt_bboxes_3d", "gt_labels_3d"):
            for p, q in zip(x.get(k, []), y.get(k, [])):
                assert torch.equal(p, q)
        for m, n in zip(x["img_metas"], y["img_metas"]):
            _same_meta(m, n)
            assert "img_filename" in n and "depth2img" in n
        Hp = max(pl.pad_to(m["img_shape"][0]) for m in y["img_metas"])
        Wp = max(pl.pad_to(m["img_shape"][1]) for m in y["img_metas"])
        assert all(tuple(m["batch_input_shape"]) == (Hp, Wp) for m in y["img_metas"])
        assert tuple(x["img"].shape[-2:]) == (Hp, Wp)
        mixed += any(tuple(m["pad_shape"][:2]) != (Hp, Wp) for m in y["img_metas"])
    assert mixed, "no batch mixed the two padded shapes: batch_input_shape was never a maximum"


def test_command_line_builds_then_loads_the_cache(tmp_path, capsys):
    from demf_amd import train
    from test_gpu_featcache import SPECS, _detector
    from test_gpu_pipeline import IMG_SCALE
    ann, ds = _dataset(tmp_path, SPECS)
    work, cdir = str(tmp_path / "work"), str(tmp_path / "cache")
    argv = ["--data-root", str(tmp_path), "--ann-file", os.path.basename(ann), "--work-dir", work, "--no-graphs",
            "--batch-size", "2", "--epochs", "1", "--seed", str(SEED), "--workers", "2", "--log-interval", "1",
            "--feature-cache", cdir, "--feature-cache-dtype", "bf16"]
    kw = dict(num_points=2048, img_scale=IMG_SCALE, repeat=1, echo=False)
    det = _detector()
    capsys.readouterr()
    train.main(argv, model=det, **kw)
    assert "building" in capsys.readouterr().out
    assert os.path.exists(os.path.join(cdir, "index.json"))
    with open(os.path.join(cdir, "index.json")) as f:
        assert json.load(f)["dtype"] == "bf16"
    # the second run finds the cache: no image is needed any more
    _remove_images(tmp_path)
    det.extract_img_feat = _never
    ret = train.main(argv[:-2], model=det, resume_from=os.path.join(work, "epoch_1.pth"), max_epochs=2, **kw)
    assert "loaded 4 scenes" in capsys.readouterr().out
    assert ret["iter"] == 4 and os.path.exists(os.path.join(work, "epoch_2.pth"))
