"""The host side of the frozen image-feature cache (demf_amd/featcache.py): index JSON, fingerprint, command line,
the image-free loader's host half, level shapes from conv parameters, argument checks of the assembler."""
import os

import numpy as np
import pytest
import torch


def _index():
    from demf_amd import featcache
    scenes = [dict(sample_idx=7, ori_shape=[53, 73], img_shape=[232, 320], levels=[[29, 40], [15, 20], [8, 10], [4, 5]],
                   row0=0),
              dict(sample_idx=9, ori_shape=[43, 56], img_shape=[240, 313], levels=[[30, 40], [15, 20], [8, 10], [4, 5]],
                   row0=29 * 40 + 15 * 20 + 80 + 20)]
    rows = scenes[1]["row0"] + 30 * 40 + 15 * 20 + 80 + 20
    return dict(version=featcache.LAYOUT_VERSION, dtype="bf16", C=256, levels=4, img_scale=[320, 240], pad_divisor=32,
                rows=rows, fingerprint="ab" * 32, files=[dict(name="tokens_000.bin", rows=rows, bytes=rows * 512)],
                scenes=scenes)


def test_index_json_round_trip():
    from demf_amd import featcache
    index = _index()
    text = featcache.index_to_json(dict(index, rows=np.int64(index["rows"])))      # numpy scalars are written as numbers
    assert featcache.index_from_json(text) == index
    assert featcache.index_to_json(featcache.index_from_json(text)) == text
    bad = dict(index, scenes=[index["scenes"][0], dict(index["scenes"][1], row0=5)])
    with pytest.raises(ValueError, match="does not follow"):
        featcache.index_from_json(featcache.index_to_json(bad))
    with pytest.raises(ValueError, match="disagree"):
        featcache.index_from_json(featcache.index_to_json(dict(index, rows=index["rows"] + 1)))
    with pytest.raises(ValueError, match="layout version"):
        featcache.index_from_json(featcache.index_to_json(dict(index, version=0)))
    with pytest.raises(ValueError, match="no 'fingerprint'"):
        featcache.index_from_json(featcache.index_to_json({k: v for k, v in index.items() if k != "fingerprint"}))


def test_fingerprint_changes_with_each_ingredient():
    from demf_amd import featcache, ops
    state = {"img_backbone.conv1.weight": torch.arange(12.0).view(2, 6), "img_neck.convs.0.gn.bias": torch.zeros(3),
             "img_encoder.level_embeds": torch.ones(4, 2)}
    base = dict(state=state, dtype="fp32", channels=256, img_scale=(1333, 800), pad_divisor=32, img_norm=ops.IMG_NORM,
                compute_dtype="fp32", version=featcache.LAYOUT_VERSION)
    fp = lambda **kw: featcache.fingerprint(**dict(base, **kw))       # noqa: E731
    ref = fp()
    assert ref == fp() and len(ref) == 64
    assert ref == fp(state=dict(reversed(list(state.items())))), "the key order of the state must not matter"
    other = [fp(version=featcache.LAYOUT_VERSION + 1), fp(dtype="bf16"), fp(channels=128), fp(img_scale=(1333, 801)),
             fp(pad_divisor=64), fp(img_norm=((123.675, 116.28, 103.53), (58.395, 57.12, 57.0))),
             fp(img_norm=((123.0, 116.28, 103.53), ops.IMG_NORM[1])), fp(compute_dtype="bf16")]
    changed = dict(state)
    changed["img_neck.convs.0.gn.bias"] = torch.tensor([0.0, 0.0, 1e-30])
    other.append(fp(state=changed))                                                     # bytes
    other.append(fp(state={("x" + k if "neck" in k else k): v for k, v in state.items()}))       # a name
    reshaped = dict(state)
    reshaped["img_backbone.conv1.weight"] = state["img_backbone.conv1.weight"].view(3, 4)
    other.append(fp(state=reshaped))                                                    # a shape, same bytes
    other.append(fp(state={k: v for k, v in state.items() if "encoder" not in k}))
    assert len(set(other + [ref])) == len(other) + 1
    with pytest.raises(ValueError):
        fp(dtype="fp16")


def test_command_line_flags():
    from demf_amd import train
    base = ["--data-root", "r", "--ann-file", "a", "--work-dir", "w"]
    args = train.parse_args(base)
    assert args.feature_cache is None and args.feature_cache_dtype is None
    args = train.parse_args(base + ["--feature-cache", "dir"])
    assert args.feature_cache == "dir" and args.feature_cache_dtype is None
    args = train.parse_args(base + ["--feature-cache", "dir", "--feature-cache-dtype", "bf16"])
    assert args.feature_cache == "dir" and args.feature_cache_dtype == "bf16"
    for bad in (["--feature-cache-dtype", "bf16"], ["--feature-cache", "d", "--feature-cache-dtype", "fp16"],
                ["--feature-cache", "d", "--model", "votenet"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)


@pytest.mark.parametrize("mode", ["train", "test"])
def test_image_free_pipeline_opens_no_image(tmp_path, mode):
    """``ScenePipeline(with_img=False, image_shapes=...)``: the image files are removed first; records, draws, seeds,
    boxes and EVERY meta entry are those of the ``with_img=True`` pipeline."""
    import pipeline_reference as pref
    from demf_amd import pipeline as pl
    from demf_amd.dataset import SUNRGBDDataset
    specs = [(600, (53, 73), 3), (500, (43, 56), 0)]
    ann, _ = pref.write_dataset(str(tmp_path), specs, jpeg=True)
    ds = SUNRGBDDataset(str(tmp_path), ann, test_mode=mode == "test")
    a = pl.ScenePipeline(ds, mode, img_scale=(200, 120), num_points=128, seed=3)
    shapes = {i: s[1] for i, s in enumerate(specs)}
    b = pl.ScenePipeline(ds, mode, img_scale=(200, 120), num_points=128, seed=3, with_img=False, image_shapes=shapes)
    want = [a.load(i, epoch=2) for i in range(2)]
    for i in range(2):
        os.remove(ds.get_data_info(i)["img_filename"])
    got = [b.load(i, epoch=2) for i in range(2)]
    for x, y in zip(want, got):
        assert y["img"] is None and x["img"] is not None
        assert x["seed"] == y["seed"] and x["index"] == y["index"]
        assert np.array_equal(pl.param_row(x["params"]), pl.param_row(y["params"]))
        assert np.array_equal(x["raw"], y["raw"]) and np.array_equal(x["gt_bboxes_3d"], y["gt_bboxes_3d"])
        assert set(x["meta"]) == set(y["meta"]) and {"img_shape", "pad_shape", "depth2img", "img_filename",
                                                     "img_norm_cfg", "scale_factor", "ori_shape"} <= set(y["meta"])
        _same_meta(x["meta"], y["meta"])
    with pytest.raises(ValueError):
        pl.ScenePipeline(ds, mode, with_img=True, image_shapes=shapes)


def _same_meta(x, y):
    assert set(x) == set(y)
    for k, v in x.items():
        if isinstance(v, dict):
            _same_meta(v, y[k])
        elif isinstance(v, np.ndarray) or torch.is_tensor(v):
            assert np.array_equal(np.asarray(v), np.asarray(y[k])), k
        elif isinstance(v, (list, tuple)) and v and isinstance(v[0], np.ndarray):
            assert len(v) == len(y[k]) and all(np.array_equal(p, q) for p, q in zip(v, y[k])), k
        else:
            assert v == y[k], k


def test_level_shapes_reference_geometry():
    """Strides 8 / 16 / 32 and the extra 3x3 stride-2 pad-1 level, from the modules' conv parameters."""
    from demf_amd.modules.image_stream import ChannelMapper, ResNet50, pyramid_level_shapes
    assert pyramid_level_shapes((800, 1120)) == [(100, 140), (50, 70), (25, 35), (13, 18)]
    assert pyramid_level_shapes((608, 800)) == [(76, 100), (38, 50), (19, 25), (10, 13)]
    assert pyramid_level_shapes((64, 96)) == [(8, 12), (4, 6), (2, 3), (1, 2)]
    with torch.device("meta"):
        bb = ResNet50(base=16, blocks=(1, 1, 1, 1))
        nk = ChannelMapper(bb.out_channels, 256, 4, 32)
    assert pyramid_level_shapes((256, 320), bb, nk) == [(32, 40), (16, 20), (8, 10), (4, 5)]


def test_arena_rows_from_shapes():
    from demf_amd import featcache
    # 530 x 730 -> 800 x 1102 -> padded 800 x 1120: 14 000 + 3 500 + 875 + 234 rows
    assert featcache.arena_rows([(530, 730)]) == 18609
    assert featcache.arena_rows([(530, 730), (530, 730)]) == 2 * 18609


def test_assembler_reports_bad_arguments_before_any_launch():
    """As tests/test_abi.py holds of every entry: validation comes before device work, so this runs without a GPU."""
    import ctypes
    from demf_amd import _ffi
    hw = (ctypes.c_int * 2)(5, 7)
    table = (ctypes.c_longlong * 3)(0, 6, 7)
    idx = (ctypes.c_longlong * 1)(0)
    A = ctypes.addressof
    call = lambda B, C, S, L, N, rows, t=table, i=idx: _ffi.call(       # noqa: E731
        "demf_tokens_assemble", B, C, S, L, N, rows, None, 0, None, A(t), None, A(i), A(hw), None, None, 0, None)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        call(1, 6, 35, 1, 1, 100)
    with pytest.raises(RuntimeError, match="at most 8"):
        call(1, 8, 35, 9, 1, 100)
    with pytest.raises(RuntimeError, match="S = 36"):
        call(1, 8, 36, 1, 1, 100)
    with pytest.raises(RuntimeError, match="larger than the batch's"):
        call(1, 8, 35, 1, 1, 100)                                       # the scene is 6 x 7 on a 5 x 7 canvas
    with pytest.raises(RuntimeError, match="outside the table"):
        call(1, 8, 35, 1, 1, 100, i=(ctypes.c_longlong * 1)(1))
    fits = (ctypes.c_longlong * 3)(90, 5, 7)
    with pytest.raises(RuntimeError, match="of an arena of 100"):
        call(1, 8, 35, 1, 1, 100, t=fits)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(1, 8, 35, 1, 1, 200, t=fits)                               # everything valid but the device pointers


def test_assemble_tokens_refuses_cpu_tensors():
    from demf_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.assemble_tokens(torch.zeros(35, 8), torch.tensor([[0, 5, 7]]), torch.tensor([0]), [(5, 7)])
