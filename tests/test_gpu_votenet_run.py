"""The points-only VoteNet baseline through the engine, the loader and the runners: a batch without ``img_features`` is
a legal batch (engine.Trainer / capture / StepCache), ``SceneLoader(with_img=False)`` yields the ``with_img=True``
loader's points and ground truth without touching an image, ``train.fit`` trains a model without ``extract_img_feat``
from points alone and ``infer.run_test`` evaluates it.  Scaled-down configuration of tests/test_gpu_votenet.py; bars of
tests/test_gpu_engine.py (captured against eager: loss 1e-4, gradient rel-L2 1e-3, parameters 6e-4)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures

pytestmark = pytest.mark.gpu

SEED = 5
SPECS = [(6000, (53, 73), 3), (5000, (53, 73), 0), (7000, (53, 73), 4), (4500, (53, 73), 2)]


def _model(seed=1):
    from demf_amd.modules import VoteNet
    from test_gpu_votenet import _cfg
    m = VoteNet(_cfg())
    fixtures.seed_weights(m, seed)
    return m


def _setup(seed=3, lr=1e-3, **kw):
    from demf_amd import engine, synthetic
    model = _model(seed).cuda().train()
    raw = synthetic.make_scene_batch(3, 2048, fixtures.TINY_PYRAMID, fixtures.TINY_INPUT, 64, seed=seed, n_gt=4)
    batch = dict(points=torch.from_numpy(raw["points"]).cuda(),
                 gt_bboxes_3d=[torch.from_numpy(b).cuda() for b in raw["gt_boxes"]],
                 gt_labels_3d=[torch.from_numpy(l).cuda() for l in raw["gt_labels"]])
    return engine.Trainer(model, lr=lr, **kw), model, batch


def test_captured_step_equals_eager_step():
    """The same weights and batch: one eager optimizer step against one replay of the captured step (ONE hipGraph with the
    update inside) - the same loss and the same updated parameters; a second batch loaded into the static buffers."""
    from demf_amd import engine
    ta, ma, batch = _setup()
    tb, mb, _ = _setup()
    assert engine.StepCache.key(batch)[1] is None                  # no pyramid in the shape key
    la = ta.step(batch)
    replay = tb.capture(batch, warmup=1, dry=True)
    assert "img_features" not in replay.static and replay.geo is not None     # the pre-pass pipeline is in use
    lb = replay()
    torch.cuda.synchronize()
    pa, pb = ta.opt.flat.double(), tb.opt.flat.double()
    print("captured vs eager: loss %.6f / %.6f, parameters rel-L2 %.2e"
          % (la.item(), lb.item(), ((pa - pb).norm() / pa.norm()).item()))
    assert abs(la.item() - lb.item()) <= 1e-4 * abs(la.item())
    assert ((pa - pb).norm() / pa.norm()).item() < 6e-4
    assert tb.opt.t == ta.opt.t == 1
    _, _, other = _setup(seed=4)
    replay.load(other)
    l2 = replay()
    want = ta.step(other)
    torch.cuda.synchronize()
    assert abs(l2.item() - want.item()) <= 1e-3 * abs(want.item())
    with pytest.raises(ValueError, match="image pyramid"):
        replay.load(dict(other, img_features=[torch.zeros(3, 64, 2, 2, device="cuda")], img_metas=[{}] * 3))


def test_step_cache_replays_points_only_batches():
    tr, model, batch = _setup()
    stepper = tr.bucketed(max_graphs=2, capture_on=2, warmup=1)
    losses = [float(stepper.step(batch, next_points=batch["points"])) for _ in range(5)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert stepper.stats["captured"] == 1 and stepper.stats["replayed"] >= 3, stepper.stats


# ---- loader ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import pipeline_reference as pref
    from demf_amd.dataset import SUNRGBDDataset
    root = str(tmp_path_factory.mktemp("votenet"))
    ann, _ = pref.write_dataset(root, SPECS, jpeg=True)
    return dict(root=root, ann=ann, train=SUNRGBDDataset(root, ann), val=SUNRGBDDataset(root, ann, test_mode=True))


@pytest.mark.parametrize("mode", ["train", "test"])
def test_loader_without_images_yields_the_same_points_and_ground_truth(data, mode, monkeypatch):
    from demf_amd import ops
    from demf_amd import pipeline as pl
    from test_gpu_pipeline import IMG_SCALE
    ds = data["train"] if mode == "train" else data["val"]
    kw = dict(seed=SEED, img_scale=IMG_SCALE, num_points=2048, workers=2)
    ref_loader = pl.SceneLoader(ds, 2, mode, **kw)
    with_img = list(ref_loader)
    calls = []
    monkeypatch.setattr(pl.ScenePipeline, "read_image", staticmethod(lambda path: calls.append(path)))
    monkeypatch.setattr(ops, "image_prep", lambda *a, **k: calls.append("image_prep"))
    loader = pl.SceneLoader(ds, 2, mode, with_img=False, **kw)
    without = list(loader)
    assert not calls, calls                                         # no image read, no image_prep launch
    assert len(with_img) == len(without) == 2
    for a, b in zip(with_img, without):
        assert a.indices == b.indices and "img" not in b and "img" in a
        assert torch.equal(a["points"], b["points"])                # bit for bit
        assert ("gt_bboxes_3d" in a) == ("gt_bboxes_3d" in b) == (mode == "train")
        for k in ("gt_bboxes_3d", "gt_labels_3d") if mode == "train" else ():
            assert len(a[k]) == len(b[k]) and all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        for ma, mb in zip(a["img_metas"], b["img_metas"]):
            assert "img_shape" not in mb and mb["sample_idx"] == ma["sample_idx"]
            for k in ("pcd_horizontal_flip", "pcd_scale_factor", "transformation_3d_flow"):
                assert ma.get(k) == mb.get(k), k
            assert np.array_equal(ma.get("pcd_rotation"), mb.get("pcd_rotation"))
    assert 0 < loader.last_upload_bytes < ref_loader.last_upload_bytes     # the image bytes stay on the host's disk
    with pytest.raises(ValueError, match="with_img"):
        pl.SceneLoader(ds, 2, mode, pipeline=pl.ScenePipeline(ds, mode, with_img=True), with_img=False)


# ---- fit / run_test --------------------------------------------------------------------------------------------
def _fit_kwargs(**kw):
    from test_gpu_pipeline import IMG_SCALE
    out = dict(batch_size=2, num_points=2048, img_scale=IMG_SCALE, max_epochs=1, repeat=3, log_interval=1,
               eval_interval=1, seed=SEED, workers=2, echo=False)
    out.update(kw)
    return out


def _log(work):
    with open(os.path.join(work, "train.log.json")) as f:
        return [json.loads(l) for l in f if l.strip()]


@pytest.mark.parametrize("accumulate", [1, 2])
def test_fit_three_optimizer_steps_and_checkpoint_round_trip(data, accumulate):
    """``fit`` on the synthetic dataset, captured steps: three optimizer steps (accumulate 1: repeat 3 x 2 batches -> 6
    steps, of which the first three are compared; accumulate 2: 6 batches -> 3 steps), log lines without ``center_loss``,
    validation through ``run_test`` + ``indoor_eval``, then the checkpoint back into a fresh model and trainer."""
    from demf_amd import engine, infer, meter, train
    work = os.path.join(data["root"], "work_acc%d" % accumulate)
    model = _model()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    out = train.fit(model, data["train"], work, val_set=data["val"], accumulate=accumulate, **_fit_kwargs())
    torch.cuda.synchronize()
    steps = 6 // accumulate
    assert out["iter"] == out["trainer"].opt.t == out["meter"].next_t == steps >= 3
    lines = _log(work)
    train_lines = [l for l in lines if l["mode"] == "train"]
    assert len(train_lines) == steps
    terms = set(model.bbox_head.LOSS_NAMES) | {"vote_loss"}
    assert "center_loss" not in terms and "center_loss" in meter.loss_names()
    for l in train_lines:
        assert set(l) - {"discarded"} == {"mode", "epoch", "iter", "lr", "loss", "grad_norm", "time"} | terms, sorted(l)
        assert all(np.isfinite(v) for k, v in l.items() if k != "mode") and l["loss"] > 0 and l["grad_norm"] > 0
        assert l["loss"] == pytest.approx(sum(l[k] for k in terms), rel=1e-4)
    val_lines = [l for l in lines if l["mode"] == "val"]
    assert len(val_lines) == 1 and "mAP_0.25" in val_lines[0] and set(out["val"]) == set(val_lines[0]) - {"mode", "epoch", "iter"}
    assert out["stepper"].stats["captured"] >= 1 and out["stepper"].stats["replayed"] > 0, out["stepper"].stats
    assert model.training
    sd = model.state_dict()
    assert sum(not torch.equal(v.cpu(), init[k]) for k, v in sd.items()) > 50
    ckpt = train.load_checkpoint_file(os.path.join(work, "latest.pth"))
    assert ckpt["meta"]["iter"] == steps and ckpt["meta"]["accumulate"] == accumulate
    fresh = _model(seed=2)
    infer.load_checkpoint(fresh, os.path.join(work, "latest.pth"))
    for k, v in sd.items():
        assert torch.equal(fresh.state_dict()[k], v.cpu()), k
    tr = engine.Trainer(fresh.cuda(), accumulate=accumulate)
    m = meter.StepMeter(train.model_loss_names(fresh))
    tr.attach_meter(m)
    assert train.restore_checkpoint(ckpt, fresh, tr, m) == ckpt["meta"]
    assert tr.opt.t == steps and m.next_t == steps
    assert torch.equal(tr.opt.exp_avg.cpu(), ckpt["trainer"]["optimizer"]["exp_avg"])


def test_command_lines_train_then_infer(data, capsys):
    from demf_amd import infer, train
    from test_gpu_pipeline import IMG_SCALE
    work = os.path.join(data["root"], "work_cli")
    capsys.readouterr()
    train.main(["--data-root", data["root"], "--ann-file", os.path.basename(data["ann"]), "--work-dir", work,
                "--model", "votenet", "--batch-size", "2", "--epochs", "1", "--seed", str(SEED), "--workers", "2",
                "--log-interval", "1"], model=_model(), num_points=2048, img_scale=IMG_SCALE, repeat=1)
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["mode"] for l in printed] == ["train", "train"] and "center_loss" not in printed[0]
    ret = infer.main(["--data-root", data["root"], "--ann-file", data["ann"], "--model", "votenet",
                      "--checkpoint", os.path.join(work, "latest.pth")], model=_model(seed=7), num_points=2048,
                     img_scale=IMG_SCALE)
    assert "mAP_0.25" in ret and "mAP_0.50" in ret


def test_run_test_equals_get_bboxes_of_the_torch_restatement(data):
    """``run_test`` (no image read; fused decode, packed store) -> ``indoor_eval``, against ``get_bboxes`` of the torch
    restatement (coder.decode + softmax, then the shared NMS + pack) on the same weights and the same loader batches:
    the same boxes in the same order."""
    from demf_amd import infer
    from demf_amd import pipeline as pl
    from test_gpu_pipeline import IMG_SCALE
    model = _model().cuda().eval()
    with torch.no_grad():
        for m in (model.bbox_head.conv_pred.conv_reg, model.bbox_head.conv_pred.conv_cls):
            m.weight.mul_(6.0)              # eval-mode BN on seeded weights: spread the scores and the sizes
    store = infer.run_test(model, data["val"], batch_size=2, workers=2, num_points=2048, img_scale=IMG_SCALE, seed=SEED)
    got = store.results()
    assert len(got) == len(SPECS) and sum(len(r["scores_3d"]) for r in got) > 0
    want = []
    with torch.no_grad():
        for batch in pl.SceneLoader(data["val"], 2, "test", seed=SEED, img_scale=IMG_SCALE, num_points=2048, workers=2,
                                    with_img=False):
            preds = model.forward_head(batch["points"])
            want += model.bbox_head.get_bboxes(batch["points"], preds, None, fused=False)
    for r, (bx, sc, lb) in zip(got, want):
        assert torch.equal(r["labels_3d"], lb.cpu())
        box = r["boxes_3d"].tensor if hasattr(r["boxes_3d"], "tensor") else r["boxes_3d"]
        np.testing.assert_allclose(box.numpy(), bx.tensor.cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(r["scores_3d"].numpy(), sc.cpu().numpy(), rtol=0, atol=1e-6)
    ret = data["val"].evaluate(store)
    assert "mAP_0.25" in ret and "mAP_0.50" in ret
