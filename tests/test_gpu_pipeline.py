"""The scene input pipeline on the GPU (csrc/pipeline.hip, demf_amd/pipeline.py, demf_amd/dataset.py): the floor
percentile against numpy, the keyed point sample, the augmented points against data.augment_3d, the resized images
against the float64 restatement (tests/pipeline_reference.py), the metadata against the head's projection, graph
capture, and the whole chain infos -> loader -> DeMFVoteNet -> indoor evaluation."""
import numpy as np
import pytest
import torch

from demf_amd import data, ops
from demf_amd import pipeline as pl
from demf_amd.dataset import SUNRGBDDataset
from demf_amd.modules.head import compose_projection

import pipeline_reference as ref

pytestmark = pytest.mark.gpu


def _ragged(clouds):
    raw = np.concatenate(clouds).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return torch.from_numpy(raw).cuda(), torch.from_numpy(off).cuda()


def _records(z, rng):
    r = rng.uniform(-3, 3, size=(len(z), 6)).astype(np.float32)
    r[:, 2] = z
    return r


def _ulp_close(got, want):
    w = np.float32(want)
    return abs(np.float64(got) - np.float64(w)) <= np.spacing(np.abs(w))


def test_floor_is_numpys_percentile():
    rng = np.random.default_rng(0)
    cases = [rng.normal(0, 1, 1), rng.normal(0, 1, 2), rng.uniform(-1, 2, 101), rng.uniform(-1.3, 1.5, 50000),
             rng.normal(0.2, 0.8, 200000),
             rng.integers(0, 5, 30000) / 4.0 - 1.0,                           # heavy ties
             np.full(777, -0.8125),                                          # all equal
             np.concatenate([np.full(500, -0.0), np.full(500, 0.0), -rng.uniform(0, 1e-3, 20)]),   # +-0.0, negatives
             -rng.uniform(1, 2, 4096), np.concatenate([np.full(40, -1e-30), rng.uniform(0, 1, 960)])]
    clouds = [_records(np.asarray(z, np.float32), rng) for z in cases]
    floor = ops.points_floor(*_ragged(clouds)).cpu().numpy()
    for z, got in zip(cases, floor):
        want = np.percentile(np.asarray(z, np.float32), 0.99)
        assert _ulp_close(got, want), (len(z), got, want)
        assert _ulp_close(got, ref.percentile_floor(np.asarray(z, np.float32)))


def _prep(clouds, k, seeds, params=None):
    raw, off = _ragged(clouds)
    B = len(clouds)
    if params is None:
        params = np.tile(pl.param_row(pl.identity_aug_params()), (B, 1))
    floor = ops.points_floor(raw, off)
    out, idx = ops.points_prep(raw, off, floor, torch.from_numpy(np.asarray(params, np.float32)).cuda(),
                               torch.tensor(seeds, dtype=torch.int64).cuda(), k, return_index=True)
    return out.cpu().numpy(), idx.cpu().numpy(), floor.cpu().numpy()


def test_sampling_without_and_with_replacement():
    rng = np.random.default_rng(1)
    sizes = [20000, 50000, 33333, 4000, 1, 20001]
    clouds = [_records(rng.uniform(-1, 1, n).astype(np.float32), rng) for n in sizes]
    seeds = [11, 11, 12, 13, 14, 15]
    out, idx, _ = _prep(clouds, 20000, seeds)
    for b, n in enumerate(sizes):
        assert idx[b].min() >= 0 and idx[b].max() < n
        if n >= 20000:
            assert len(np.unique(idx[b])) == 20000
        np.testing.assert_array_equal(out[b][:, :3], clouds[b][idx[b], :3])
    assert not np.array_equal(idx[0], idx[2][:20000])                   # different seeds
    assert not np.array_equal(idx[1][:100], idx[0][:100])               # same seed, different scene size
    assert len(np.unique(idx[3])) < 4000 + 1 and idx[3].max() < 4000
    assert (idx[4] == 0).all()
    again = _prep(clouds, 20000, seeds)[1]
    np.testing.assert_array_equal(again, idx)                            # deterministic per seed
    # same cloud, different seeds in one batch -> different subsets
    _, idx2, _ = _prep([clouds[1], clouds[1]], 20000, [1, 2])
    assert not np.array_equal(np.sort(idx2[0]), np.sort(idx2[1]))


def test_sample_is_uniform():
    """N = 1000, k = 400 over 400 keys: per-point inclusion counts and the first index against uniform."""
    rng = np.random.default_rng(2)
    cloud = _records(rng.uniform(0, 1, 1000).astype(np.float32), rng)
    S = 400
    _, idx, _ = _prep([cloud] * S, 400, list(range(1000, 1000 + S)))
    for row in idx:
        assert len(np.unique(row)) == 400
    counts = np.bincount(idx.reshape(-1), minlength=1000)
    p = 0.4
    stat = (((counts - S * p) ** 2) / (S * p * (1 - p))).sum()          # ~ chi2(999): mean 999, sd 45
    assert 999 - 8 * 45 < stat < 999 + 8 * 45, stat
    first = np.bincount(idx[:, 0] // 100, minlength=10)                  # 10 bins of 40 expected
    chi = ((first - S / 10) ** 2 / (S / 10)).sum()                       # chi2(9): p(> 40) ~ 5e-6
    assert chi < 40, (first, chi)


def test_points_equal_augment_3d():
    rng = np.random.default_rng(3)
    B, k = 8, 20000
    clouds = [_records(rng.uniform(-1.2, 1.4, 50000).astype(np.float32), rng) for _ in range(B)]
    for c in clouds:
        c[:, 0] = rng.uniform(-3.5, 3.5, len(c))
        c[:, 1] = rng.uniform(0.5, 4.0, len(c))
    tstd = (0.1, 0.1, 0.05)
    params = [pl.draw_aug_params(np.random.default_rng(s), translation_std=tstd) for s in range(B)]
    assert 0 < sum(p["flip"] for p in params) < B
    out, idx, floor = _prep(clouds, k, list(range(B)), np.stack([pl.param_row(p) for p in params]))
    boxes = np.zeros((1, 7), np.float32)
    for b in range(B):
        pts = data.add_height(clouds[b][:, :3])[idx[b]]
        want, _, meta = data.augment_3d(pts, boxes, {}, np.random.default_rng(b), translation_std=tstd)
        assert meta["pcd_horizontal_flip"] == params[b]["flip"]
        np.testing.assert_allclose(out[b][:, :3], want[:, :3], rtol=0, atol=2e-6)
        np.testing.assert_allclose(out[b][:, 3], want[:, 3], rtol=0, atol=2e-6)
    # the flip alone is exact: identity rotation / scale / translation with and without it
    ident = pl.param_row(pl.identity_aug_params())
    flip = ident.copy()
    flip[0] = 1.0
    o2, i2, _ = _prep(clouds[:2], 1000, [5, 5], np.stack([ident, flip]))
    np.testing.assert_array_equal(o2[0][:, 1:3], clouds[0][i2[0], 1:3])
    np.testing.assert_array_equal(o2[1][:, 0], -clouds[1][i2[1], 0])


SIZES = [((530, 730), (800, 1102)), ((427, 561), (800, 1051)), ((441, 591), (800, 1072)), ((1, 1), (3, 5)),
         ((2, 3), (7, 9)), ((5, 7), (40, 57)), ((100, 150), (37, 55)), ((64, 48), (64, 48))]


def _images(seed):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw, _ in SIZES]
    flat = np.concatenate([i.reshape(-1) for i in imgs])
    off = np.concatenate([[0], np.cumsum([i.size for i in imgs])]).astype(np.int64)
    shp = np.array([[*hw, *o] for hw, o in SIZES], np.int32)
    return imgs, flat, off, shp


def test_image_resize_normalise_pad():
    imgs, flat, off, shp = _images(4)
    Hp, Wp = 800, 1120
    out = ops.image_prep(torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(shp).cuda(),
                         (Hp, Wp)).cpu().numpy()
    assert out.shape == (len(SIZES), 3, Hp, Wp)
    near_half = 0
    for b, (img, (_, (h, w))) in enumerate(zip(imgs, SIZES)):
        pad = out[b].copy()
        pad[:, :h, :w] = 0
        assert not pad.any(), f"scene {b}: padding is not zero"
        pre, want = ref.image_levels(img, h, w)
        got = ref.levels_of(out[b][:, :h, :w])
        bad = got != want
        tie = np.abs(pre - np.floor(pre) - 0.5) < 1e-3
        assert not (bad & ~tie).any(), (b, np.argwhere(bad & ~tie)[:5])
        assert (np.abs(got - want)[bad] <= 1).all()
        near_half += int(bad.sum())
        # the normalised values are (level - mean) / std in fp32
        np.testing.assert_allclose(out[b][:, :h, :w], (got - ref.MEAN[:, None, None]) / ref.STD[:, None, None],
                                   rtol=0, atol=1e-5)
    print(f"pixels one level off at a .5 boundary: {near_half}")


def test_metadata_round_trip_through_the_head_projection():
    """Projecting the GPU-augmented points with the metadata the pipeline writes lands every point where the raw
    point lands with identity metadata (test_data_path's check, here with the device transform), flip on and off."""
    rng = np.random.default_rng(5)
    base = data.resize_meta(dict(depth2img=ref.depth2img(np.array([[529.5, 0, 365], [0, 529.5, 265], [0, 0, 1]]),
                                                         np.eye(3)).astype(np.float32), flip=False),
                            (530, 730), (1333, 800))
    cloud = _records(rng.uniform(-1, 1, 3000).astype(np.float32), rng)
    cloud[:, 1] = rng.uniform(1.0, 5.0, len(cloud))
    plain = dict(base, transformation_3d_flow=[])
    seen = set()
    for s in range(12):
        p = pl.draw_aug_params(np.random.default_rng(s), translation_std=(0.1, 0.1, 0.05))
        _, meta = pl.apply_aug_params(np.zeros((0, 7), np.float32), base, p)
        out, idx, _ = _prep([cloud], 500, [s], pl.param_row(p)[None])
        M, au, bu, av, bv = compose_projection(meta)
        M0, au0, bu0, av0, bv0 = compose_projection(plain)

        def uv(P, a, b_, c, d, pts):
            q = np.concatenate([pts[:, :3].astype(np.float64), np.ones((len(pts), 1))], 1) @ P.T
            return np.stack([q[:, 0] / q[:, 2] * a + b_, q[:, 1] / q[:, 2] * c + d], 1)

        np.testing.assert_allclose(uv(M, au, bu, av, bv, out[0]), uv(M0, au0, bu0, av0, bv0, cloud[idx[0]]),
                                   rtol=0, atol=2e-5)
        seen.add(p["flip"])
    assert seen == {True, False}


def test_capture_replays_on_fresh_inputs():
    B, k = 3, 2048

    def inputs(seed):
        r = np.random.default_rng(seed)
        clouds = [_records(r.uniform(-1, 1, n).astype(np.float32), r) for n in (5000, 3000, 1500)]
        params = np.stack([pl.param_row(pl.draw_aug_params(r)) for _ in range(B)])
        imgs = [r.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((53, 73), (43, 56), (44, 59))]
        return (np.concatenate(clouds), np.array([0, 5000, 8000, 9500], np.int64), params,
                r.integers(0, 2 ** 62, size=B), np.concatenate([i.reshape(-1) for i in imgs]),
                np.array([0, 53 * 73 * 3, 53 * 73 * 3 + 43 * 56 * 3, 53 * 73 * 3 + 43 * 56 * 3 + 44 * 59 * 3]),
                np.array([[53, 73, 200, 276], [43, 56, 200, 260], [44, 59, 200, 268]], np.int32))

    def upload(arrs, into=None):
        ts = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrs]
        ts[0] = ts[0].float()
        ts[2] = ts[2].float()
        ts[3], ts[5] = ts[3].long(), ts[5].long()
        if into is None:
            return [t.cuda() for t in ts]
        for d, t in zip(into, ts):
            d.copy_(t)
        return into

    def run(st):
        raw, off, prm, seeds, img, ioff, shp = st
        floor = ops.points_floor(raw, off)
        pts, idx = ops.points_prep(raw, off, floor, prm, seeds, k, return_index=True)
        im = ops.image_prep(img, ioff, shp, (224, 288))
        return floor, pts, idx, im

    static = upload(inputs(1))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(static)
    fresh = inputs(2)
    upload(fresh, into=static)
    g.replay()
    torch.cuda.synchronize()
    eager = run(upload(fresh))
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    assert not torch.equal(outs[1], run(upload(inputs(1)))[1])


# ---- the whole chain ---------------------------------------------------------------------------------------------

SPECS = [(6000, (53, 73), 3), (5000, (43, 56), 0), (7000, (44, 59), 4), (4500, (48, 64), 2)]
IMG_SCALE = (320, 240)


@pytest.fixture()
def scenes_dir(tmp_path):
    ann, scenes = ref.write_dataset(str(tmp_path), SPECS, jpeg=True)
    return str(tmp_path), ann, scenes


def test_two_loaders_with_one_seed_agree(scenes_dir):
    root, ann, _ = scenes_dir
    ds = SUNRGBDDataset(root, ann)
    a = list(pl.SceneLoader(ds, 2, "train", seed=7, img_scale=IMG_SCALE, num_points=2048, workers=4))
    b = list(pl.SceneLoader(ds, 2, "train", seed=7, img_scale=IMG_SCALE, num_points=2048, workers=2))
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x.indices == y.indices
        assert torch.equal(x["points"], y["points"]) and torch.equal(x["img"], y["img"])
        for m, n in zip(x["img_metas"], y["img_metas"]):
            assert m["batch_input_shape"] == n["batch_input_shape"] == tuple(x["img"].shape[-2:])
            np.testing.assert_array_equal(m["pcd_rotation"], n["pcd_rotation"])
    loader = pl.SceneLoader(ds, 4, "train", seed=7, img_scale=IMG_SCALE, num_points=2048)
    e0, e1 = next(iter(loader)), next(iter(loader))
    assert e0.indices != e1.indices or not torch.equal(e0["points"], e1["points"])   # reshuffled / redrawn per epoch
    assert loader.last_upload_bytes < 4 * (7000 * 24 + 53 * 73 * 3) + 4096


def test_end_to_end_train_test_and_evaluate(scenes_dir):
    from demf_amd import fused
    from demf_amd.modules import DeMFVoteNet
    from oracle import fixtures
    from test_gpu_detector import STREAM, _cfg256
    root, ann, _ = scenes_dir
    cfg = _cfg256()
    det = DeMFVoteNet(cfg, **STREAM)
    fixtures.seed_weights(det, 1)
    det.cuda().train()
    train = pl.SceneLoader(SUNRGBDDataset(root, ann), 2, "train", seed=1, img_scale=IMG_SCALE, num_points=2048)
    fused.rng_state(torch.device("cuda"), seed=3)
    n = 0
    for batch in train:
        assert batch["points"].shape == (2, 2048, 4) and batch["img"].shape[:2] == (2, 3)
        losses = det.forward_train(**batch)
        total = losses.pop("_total")
        assert all(torch.isfinite(v).all() for v in losses.values()), losses
        total.backward()
        n += 1
    assert n == 2
    assert any(p.grad is not None and p.grad.abs().sum() > 0 for p in det.parameters())

    det.eval()
    test_ds = SUNRGBDDataset(root, ann, test_mode=True)
    results = []
    for batch in pl.SceneLoader(test_ds, 2, "test", seed=1, img_scale=IMG_SCALE, num_points=2048):
        assert "gt_bboxes_3d" not in batch
        assert all(m["transformation_3d_flow"] == ["HF", "R", "S", "T"] and not m["pcd_horizontal_flip"]
                   for m in batch["img_metas"])
        results += det.simple_test(**batch)
    assert len(results) == len(test_ds)
    ret = test_ds.evaluate(results)
    assert "mAP_0.25" in ret and "mAP_0.50" in ret

    # the dataset's own ground truth as detections scores 1.0: infos conversion and evaluation share the convention
    ds = SUNRGBDDataset(root, ann)
    gt = []
    for i in range(len(ds)):
        a = ds.get_ann_info(i)
        gt.append(dict(boxes_3d=torch.from_numpy(a["gt_bboxes_3d"]), scores_3d=torch.ones(len(a["gt_labels_3d"])),
                       labels_3d=torch.from_numpy(a["gt_labels_3d"])))
    ret = ds.evaluate(gt)
    assert ret["mAP_0.25"] == 1.0 and ret["mAP_0.50"] == 1.0, ret
