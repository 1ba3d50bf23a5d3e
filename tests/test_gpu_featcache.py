"""``featcache.FeatureCache`` on a tiny stream over a four-scene dataset in two image shapes (one scene without ground
truth): what an entry is, what ``assemble`` returns for mixed- and same-shape batches, bf16 storage, the disk round
trip and its refusals, the memory limit, and ``pyramid_level_shapes`` against the stream's real output shapes."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures

pytestmark = pytest.mark.gpu

# landscape and portrait: padded 256 x 320 and 320 x 256 at IMG_SCALE, so a mixed batch's canvas is 320 x 320
SPECS = [(6000, (53, 73), 3), (5000, (73, 53), 0), (7000, (53, 73), 4), (4500, (73, 53), 2)]
_STATE = {}


def _detector(seed=1):
    from demf_amd.modules import DeMFVoteNet
    from test_gpu_detector import STREAM, _cfg256
    det = DeMFVoteNet(_cfg256(), **STREAM)
    fixtures.seed_weights(det, seed)
    return det.cuda().train()


def _setup(tmp_path_factory):
    """One dataset, model and fp32 cache shared by the tests below (never modified afterwards)."""
    if _STATE:
        return _STATE
    import pipeline_reference as pref
    from demf_amd import featcache
    from demf_amd.dataset import SUNRGBDDataset
    from test_gpu_pipeline import IMG_SCALE
    root = str(tmp_path_factory.mktemp("featcache"))
    ann, _ = pref.write_dataset(root, SPECS, jpeg=True)
    ds = SUNRGBDDataset(root, ann)
    det = _detector()
    cache = featcache.FeatureCache.build(det, ds, img_scale=IMG_SCALE, dtype="fp32")
    _STATE.update(root=root, ann=ann, ds=ds, det=det, cache=cache, scale=IMG_SCALE)
    return _STATE


def _alone(st, i):
    """Scene i through ScenePipeline's own host and device halves, alone -> (tokens (rows, C), spatial, meta)."""
    from demf_amd import pipeline as pl
    pipe = pl.ScenePipeline(st["ds"], "test", img_scale=st["scale"], num_points=1024)
    batch, _ = pipe.to_device([pipe.load(i)], torch.device("cuda"))
    out = st["det"].extract_img_feat(batch["img"], batch["img_metas"])
    return out["tokens"][0], [tuple(s) for s in out["spatial"]], batch["img_metas"][0]


def _batch_metas(st, idx):
    from demf_amd import pipeline as pl
    pipe = pl.ScenePipeline(st["ds"], "train", img_scale=st["scale"], num_points=1024, seed=2, with_img=False,
                            image_shapes=st["cache"].ori_shapes)
    batch, _ = pipe.to_device([pipe.load(i) for i in idx], torch.device("cuda"))
    assert "img" not in batch
    return batch["img_metas"]


def _placement(cache, idx, spatial):
    """The cache's own entries on the canvas ``spatial`` by plain indexing (fp32 or bf16 as stored)."""
    C = cache.channels
    out = torch.zeros((len(idx), sum(h * w for h, w in spatial), C), dtype=cache.arena.dtype, device=cache.arena.device)
    for b, i in enumerate(idx):
        rows, r, start = cache.entry(i), 0, 0
        for (H, W), (h, w) in zip(spatial, cache.meta_entries(i)["levels"]):
            out[b, start:start + H * W].view(H, W, C)[:h, :w] = rows[r:r + h * w].view(h, w, C)
            r += h * w
            start += H * W
    return out


def test_entries_are_the_stream_alone(tmp_path_factory):
    st = _setup(tmp_path_factory)
    cache = st["cache"]
    assert len(cache) == 4 and cache.dtype == "fp32" and cache.arena.dtype == torch.float32
    assert cache.ori_shapes == {i: s[1] for i, s in enumerate(SPECS)}
    row = 0
    for i in range(4):
        tokens, spatial, meta = _alone(st, i)
        rec = cache.meta_entries(i)
        assert rec["levels"] == spatial and rec["sample_idx"] == meta["sample_idx"]
        assert tuple(rec["img_shape"]) == tuple(meta["img_shape"]) and tuple(rec["ori_shape"]) == tuple(meta["ori_shape"])
        assert tuple(rec["pad_shape"]) == tuple(meta["pad_shape"])
        assert int(cache.table_host[i, 0]) == row and cache.entry(i).shape == tokens.shape
        row += tokens.shape[0]
        diff = (cache.entry(i) - tokens).abs().max().item()
        print(f"scene {i}: levels {spatial}, max |entry - fresh run| = {diff:.3g}")
        assert torch.allclose(cache.entry(i), tokens, rtol=1e-4, atol=1e-4)
    assert row == cache.arena.shape[0]
    assert cache.meta_entries(0)["levels"] != cache.meta_entries(1)["levels"]


def test_mixed_shape_batch_is_the_placement_of_the_entries(tmp_path_factory, monkeypatch):
    st = _setup(tmp_path_factory)
    cache, head = st["cache"], st["det"].pts_bbox_head
    idx = [0, 1, 3, 0]
    metas = _batch_metas(st, idx)
    assert all(tuple(m["batch_input_shape"]) == (320, 320) for m in metas)
    out = cache.assemble(idx, metas)
    spatial = [tuple(s) for s in out["spatial"]]
    assert spatial == [(40, 40), (20, 20), (10, 10), (5, 5)] and out["padding_zeroed"] is True
    assert out["tokens"].dtype == torch.float32
    mask = head._meta_tensors(metas, spatial, torch.device("cuda"), torch.float32)["mask_u8"].bool()
    placed = _placement(cache, idx, spatial)
    assert mask.any() and not mask.all()
    assert torch.equal(out["tokens"].view(torch.int32), placed.masked_fill(mask[..., None], 0.0).view(torch.int32))
    assert bool((out["tokens"][mask] == 0).all())
    # the head takes it as it takes pyramid_tokens' dict
    ii = head.prepare_image_inputs(out, metas)
    assert ii["value_tokens"] is not None and ii["value_tokens"][0] is out["tokens"]
    # into the dict of an earlier call
    again = cache.assemble([1, 1, 0, 3], _batch_metas(st, [1, 1, 0, 3]), out=out)
    assert again is out
    # without the sample-then-project attention: fp32 rows, no mask, no padding_zeroed
    monkeypatch.setattr(head, "_sample_first", lambda *a, **k: False)
    plain = cache.assemble(idx, metas)
    assert set(plain) == {"tokens", "spatial"} and plain["tokens"].dtype == torch.float32
    assert torch.equal(plain["tokens"].view(torch.int32), placed.view(torch.int32))


def test_same_shape_batch_against_the_batched_stream(tmp_path_factory):
    """Scenes of one image shape: cached (alone) and batched features are the same computation; each side is within
    the stream's own 1e-4 bar (tests/test_gpu_image_stream.py) of exact arithmetic, so 2e-4 of the output scale."""
    from demf_amd import pipeline as pl
    st = _setup(tmp_path_factory)
    cache, head = st["cache"], st["det"].pts_bbox_head
    idx = [0, 2]
    pipe = pl.ScenePipeline(st["ds"], "test", img_scale=st["scale"], num_points=1024)
    batch, _ = pipe.to_device([pipe.load(i) for i in idx], torch.device("cuda"))
    ref = st["det"].extract_img_feat(batch["img"], batch["img_metas"])
    out = cache.assemble(idx, batch["img_metas"])
    assert [tuple(s) for s in out["spatial"]] == [tuple(s) for s in ref["spatial"]]
    spatial = [tuple(s) for s in ref["spatial"]]
    keep = ~head._meta_tensors(batch["img_metas"], spatial, torch.device("cuda"), torch.float32)["mask_u8"].bool()
    scale = ref["tokens"][keep].abs().max().item()
    diff = (out["tokens"] - ref["tokens"])[keep].abs().max().item()
    print(f"same-shape batch: max difference on image positions {diff:.3g}, output scale {scale:.3g}")
    assert diff <= 2e-4 * scale


def test_bf16_storage_is_the_rounded_fp32_entries(tmp_path_factory, monkeypatch):
    from demf_amd import featcache
    st = _setup(tmp_path_factory)
    det, cache = st["det"], st["cache"]
    # the stream's outputs of the fp32 build, replayed: what is under test is the storage, not two runs of the stream
    real, seen = det.extract_img_feat, {}

    def replay(img, metas):
        key = (tuple(img.shape), float(img.double().sum()))
        if key not in seen:
            seen[key] = real(img, metas)
        return seen[key]
    monkeypatch.setattr(det, "extract_img_feat", replay)
    a = featcache.FeatureCache.build(det, st["ds"], img_scale=st["scale"], dtype="fp32")
    b = featcache.FeatureCache.build(det, st["ds"], img_scale=st["scale"], dtype="bf16")
    assert b.dtype == "bf16" and b.arena.dtype == torch.bfloat16 and b.nbytes * 2 == a.nbytes
    assert torch.equal(b.arena.view(torch.int16), a.arena.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(a.table_host, b.table_host) and a.index["fingerprint"] != b.index["fingerprint"]
    # a bf16 cache in the fp32 compute mode hands out fp32 rows: the exact widening of the stored words
    idx = [1, 0]
    metas = _batch_metas(st, idx)
    out = b.assemble(idx, metas)
    mask = det.pts_bbox_head._meta_tensors(metas, out["spatial"], torch.device("cuda"), torch.float32)["mask_u8"].bool()
    assert out["tokens"].dtype == torch.float32
    assert torch.equal(out["tokens"], _placement(b, idx, out["spatial"]).float().masked_fill(mask[..., None], 0.0))
    assert torch.allclose(cache.arena, a.arena, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_save_load_round_trip_and_refusals(tmp_path_factory, tmp_path, dtype, monkeypatch):
    from demf_amd import featcache
    from demf_amd.dataset import SUNRGBDDataset
    st = _setup(tmp_path_factory)
    det, ds = st["det"], st["ds"]
    if dtype == "fp32":
        cache = st["cache"]
    else:
        cache = featcache.FeatureCache(det, dict(st["cache"].index, dtype="bf16", fingerprint=featcache.FeatureCache.
                                                 _fingerprint(det, "bf16", 256, st["scale"], 32)),
                                       st["cache"].arena.to(torch.bfloat16))
    monkeypatch.setattr(featcache, "CHUNK_BYTES", 100_000)             # several chunks, the last one partial
    monkeypatch.setattr(featcache, "MAX_FILE_BYTES", cache.nbytes // 2)      # and more than one data file
    d = str(tmp_path / "cache")
    cache.save(d)
    names = sorted(os.listdir(d))
    assert names[0] == "index.json" and len(names) >= 3 and not any(n.endswith(".tmp") for n in names)
    assert sum(os.path.getsize(os.path.join(d, n)) for n in names[1:]) == cache.nbytes
    back = featcache.FeatureCache.load(d, det, ds)
    bits = torch.int16 if dtype == "bf16" else torch.int32
    assert back.dtype == dtype and torch.equal(back.arena.view(bits), cache.arena.view(bits))
    assert torch.equal(back.table_host, cache.table_host) and torch.equal(back.table.cpu(), cache.table_host)
    assert back.index["scenes"] == cache.index["scenes"] and back.ori_shapes == cache.ori_shapes
    words = np.fromfile(os.path.join(d, names[1]), dtype=np.uint16 if dtype == "bf16" else np.float32)
    head_rows = cache.arena[:words.size // 256]
    assert np.array_equal(words.view(np.int16 if dtype == "bf16" else np.int32),
                          head_rows.view(bits).cpu().numpy().reshape(-1))
    # a dataset in another order
    other = SUNRGBDDataset(st["root"], st["ann"])
    other.data_infos = list(reversed(other.data_infos))
    with pytest.raises(ValueError, match="recorded"):
        featcache.FeatureCache.load(d, det, other)
    # one image-branch weight changed
    w = det.img_neck.convs[0].gn.bias
    old = w.detach().clone()
    try:
        with torch.no_grad():
            w[0] += 1e-3
        with pytest.raises(ValueError, match="fingerprint"):
            featcache.FeatureCache.load(d, det, ds)
        with pytest.raises(ValueError, match="no longer matches"):
            cache.verify()
    finally:
        with torch.no_grad():
            w.copy_(old)
    cache.verify()
    # a truncated data file
    path = os.path.join(d, names[-1])
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 4)
    with pytest.raises(ValueError, match="bytes, the index records"):
        featcache.FeatureCache.load(d, det, ds)


def test_max_bytes_raises_before_anything_is_allocated(tmp_path_factory, monkeypatch):
    from demf_amd import featcache
    st = _setup(tmp_path_factory)

    def never(*a, **k):
        raise AssertionError("the stream ran")
    monkeypatch.setattr(st["det"], "extract_img_feat", never)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    need = st["cache"].nbytes
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        featcache.FeatureCache.build(st["det"], st["ds"], img_scale=st["scale"], dtype="fp32", max_bytes=1)
    with pytest.raises(MemoryError, match=f"needs {need // 2} bytes"):
        featcache.FeatureCache.build(st["det"], st["ds"], img_scale=st["scale"], dtype="bf16", max_bytes=need // 2 - 1)
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize("shape", [(256, 320), (320, 256), (288, 352), (256, 288), (320, 224)])
def test_level_shapes_equal_the_streams(tmp_path_factory, shape):
    """The two padded shapes of the dataset, and canvases whose last level is not a divisor: height and width with
    % 64 in {0, 32}."""
    from demf_amd.modules.image_stream import pyramid_level_shapes
    st = _setup(tmp_path_factory)
    det = st["det"]
    assert {shape[0] % 64, shape[1] % 64} <= {0, 32}
    meta = dict(img_shape=shape + (3,), pad_shape=shape + (3,), batch_input_shape=shape)
    out = det.extract_img_feat(torch.zeros((1, 3) + shape, device="cuda"), [meta])
    got = pyramid_level_shapes(shape, det.img_backbone, det.img_neck)
    assert got == [tuple(s) for s in out["spatial"]]
    assert got == pyramid_level_shapes(shape)                            # the tiny stream has the reference's geometry
