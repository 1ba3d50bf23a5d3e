"""The 2D detector (modules/detr2d.py) without a GPU: state-dict naming and round trips, the CPU module path against
the fp64 restatement (tests/detr2d_reference.py), the library's refusals, the store and the command line."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detr2d_reference as ref
from demf_amd import _ffi
from oracle import fixtures

TINY = dict(base=8, blocks=(1, 1, 1, 1), embed_dims=32, num_layers=1, num_heads=4, feedforward_channels=64,
            gn_groups=8, num_feats=16)
PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3)]


def _tiny(**kw):
    from demf_amd.modules import Detr2D
    m = Detr2D(num_query=kw.pop("num_query", 20), num_decoder_layers=kw.pop("num_decoder_layers", 2), **TINY, **kw)
    fixtures.seed_weights(m, 7)
    return m


def test_state_dict_keys_are_the_stage_one_checkpoints():
    m = _tiny()
    keys = set(m.stage1_state_dict())
    h = "img_bbox_head."
    want = {h + "query_embedding.weight", h + "transformer.reference_points.weight",
            h + "transformer.reference_points.bias", h + "transformer.level_embeds"}
    for n in range(2):
        want |= {h + "cls_branches.%d.%s" % (n, p) for p in ("weight", "bias")}
        want |= {h + "reg_branches.%d.%d.%s" % (n, i, p) for i in (0, 2, 4) for p in ("weight", "bias")}
        d = h + "transformer.decoder.layers.%d." % n
        want |= {d + "attentions.0.attn." + p for p in ("in_proj_weight", "in_proj_bias", "out_proj.weight",
                                                         "out_proj.bias")}
        want |= {d + "attentions.1.%s.%s" % (s, p) for s in ("sampling_offsets", "attention_weights", "value_proj",
                                                               "output_proj") for p in ("weight", "bias")}
        want |= {d + "ffns.0.layers.%s.%s" % (s, p) for s in ("0.0", "1") for p in ("weight", "bias")}
        want |= {d + "norms.%d.%s" % (i, p) for i in range(3) for p in ("weight", "bias")}
    e = h + "transformer.encoder.layers.0."
    want |= {e + "attentions.0.%s.%s" % (s, p) for s in ("sampling_offsets", "attention_weights", "value_proj",
                                                           "output_proj") for p in ("weight", "bias")}
    want |= {e + "ffns.0.layers.%s.%s" % (s, p) for s in ("0.0", "1") for p in ("weight", "bias")}
    want |= {e + "norms.%d.%s" % (i, p) for i in range(2) for p in ("weight", "bias")}
    head_keys = {k for k in keys if k.startswith(h)}
    assert head_keys == want, sorted(head_keys ^ want)
    rest = keys - head_keys
    assert rest and all(k.startswith(("img_backbone.", "img_neck.")) for k in rest)
    # the reference configuration: six prediction levels
    from demf_amd.modules import DeformableDETRHead
    full = set(DeformableDETRHead().state_dict())
    assert {"cls_branches.%d.weight" % n for n in range(6)} <= full
    assert {"reg_branches.%d.%d.bias" % (n, i) for n in range(6) for i in (0, 2, 4)} <= full
    assert "query_embedding.weight" in full and tuple(DeformableDETRHead().query_embedding.weight.shape) == (300, 512)


def test_stage_one_round_trip_is_bit_equal_and_strict():
    a, b = _tiny(), _tiny()
    fixtures.seed_weights(b, 8)
    sd = a.stage1_state_dict()
    res = b.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = b.stage1_state_dict()
    assert set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    # upstream shares ONE class / box branch between the prediction levels: all keys accepted, equal after the load
    h = b.img_bbox_head
    assert torch.equal(back["img_bbox_head.cls_branches.0.weight"], back["img_bbox_head.cls_branches.1.weight"])
    assert h.cls_branches[0] is h.cls_branches[1] and h.reg_branches[0] is h.reg_branches[1]
    with pytest.raises(RuntimeError, match="Missing key"):
        b.load_state_dict({k: v for k, v in sd.items() if "query_embedding" not in k}, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        b.load_state_dict(dict(sd, **{"img_bbox_head.fc_other.weight": torch.zeros(1)}), strict=True)


def test_the_export_feeds_the_fusion_detectors_image_branch():
    from demf_amd.modules import DeMFVoteNet
    m = _tiny()
    det = DeMFVoteNet(fixtures.tiny_cfg(), **TINY)
    res = det.load_state_dict(m.stage1_state_dict(), strict=False)
    assert not res.unexpected_keys
    assert res.missing_keys and all(k.startswith(("pts_backbone.", "pts_bbox_head.")) for k in res.missing_keys)
    own = det.state_dict()
    for k, v in m.state_dict().items():
        if k.startswith(("img_backbone.", "img_neck.", "img_encoder.")):
            assert torch.equal(own[k], v), k


def _cpu_ops(monkeypatch):
    """The module path's two device operators as CPU stand-ins: F.linear and the restatement's sampling core."""
    from demf_amd import ops
    from demf_amd.modules import transformer

    def linear(x, w, b=None, row_mask=None):
        y = F.linear(x, w, b)
        return y if row_mask is None else y.masked_fill(row_mask.unsqueeze(-1), 0.0)

    class Msda:
        apply = staticmethod(ref.msda_function)
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(transformer, "MultiScaleDeformableAttnFunction", Msda)


def test_cpu_module_path_matches_the_fp64_restatement(monkeypatch):
    """B = 2 padded images of different img_shape, 2 decoder layers, Q = 20: logits and boxes to 1e-10, the selected
    indices equal."""
    from demf_amd.modules import DeformableDETRHead
    from demf_amd.modules.detr2d import meta_rows, select_host
    from demf_amd.modules.image_stream import DeformableDetrEncoder
    _cpu_ops(monkeypatch)
    E, H, Q, C = 64, 4, 20, 10
    head = DeformableDETRHead(Q, C, E, num_layers=2, num_heads=H, feedforward_channels=96, max_per_img=100)
    fixtures.seed_weights(head, 3)
    head.double().eval()
    _, metas = fixtures.make_images(5, B=2, H=96, W=160)
    assert metas[0]["img_shape"] != metas[1]["img_shape"]
    st = DeformableDetrEncoder(num_layers=1, embed_dims=E, num_heads=H, num_feats=E // 2)._static(metas, PYRAMID, "cpu")
    S = sum(h * w for h, w in PYRAMID)
    g = torch.Generator().manual_seed(1)
    memory = torch.randn(2, S, E, generator=g, dtype=torch.float64)
    enc = dict(tokens=memory, spatial=PYRAMID, mask_flatten=st["mask_flatten"], valid_ratios=st["valid_ratios"].double())
    assert st["mask_flatten"].any() and not st["mask_flatten"].all()
    with torch.no_grad():
        hs, logits, boxes = head(enc, st)
    assert head.last_path == "modules"
    sd = {"img_bbox_head." + k: v for k, v in head.state_dict().items()}
    whs, wref = ref.decoder(sd, memory, st["mask_flatten"], st["valid_ratios"], PYRAMID, 2, H=H)
    wl, wb = ref.branches(sd, whs[-1], wref, 1)
    assert (hs - whs[-1]).abs().max().item() <= 1e-10
    assert (logits - wl).abs().max().item() <= 1e-10
    assert (boxes - wb).abs().max().item() <= 1e-10
    for m, sf in zip(metas, ((1.5, 1.25, 1.5, 1.25), (0.5, 0.75, 0.5, 0.75))):
        m["scale_factor"] = np.asarray(sf, np.float32)
    meta = meta_rows(metas)
    for thr, rescale in ((-1.0, True), (0.09, False)):
        rows, counts, idx = select_host(logits, boxes, meta, 100, thr, rescale)
        want = ref.select(wl, wb, meta, 100, thr, rescale)
        for b in range(2):
            assert np.array_equal(idx[b].numpy(), want[b]["idx"])
            assert int(counts[b]) == want[b]["n"]
            assert np.abs(rows[b, :want[b]["n"]].numpy() - want[b]["rows"]).max(initial=0.0) <= 1e-9
            assert not rows[b, want[b]["n"]:].any()


def test_refusals_are_reported_not_launched():
    with pytest.raises(RuntimeError, match=r"code -3\).*at most 512 queries x 32 channels"):
        _ffi.call("demf_attn_fwd_eval", 2, 8, 513, 32, None, 0.1, None, None)
    with pytest.raises(RuntimeError, match=r"code -3\).*at most 512 queries x 32 channels"):
        _ffi.call("demf_attn_fwd_eval", 2, 8, 300, 16, None, 0.1, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_attn_fwd_eval", 2, 8, 0, 32, None, 0.1, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_attn_fwd_eval", 2, 8, 300, 32, None, 0.1, None, None)
    with pytest.raises(RuntimeError, match=r"code -3\).*8193 candidates.*at most 8192 and 1024"):
        _ffi.call("demf_detr2d_select", 2, 8193, 1, 100, None, None, None, 0, 0.09, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"code -3\).*k = 1025"):
        _ffi.call("demf_detr2d_select", 2, 300, 10, 1025, None, None, None, 0, 0.09, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_detr2d_select", 2, 300, 10, 100, None, None, None, 0, 0.09, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"code -3\).*at most 32 classes"):
        _ffi.call("demf_detr2d_head", 4, 33, 256, *([None] * 7), 1, None, None, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _ffi.call("demf_detr2d_head", 4, 10, 255, *([None] * 7), 1, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_detr2d_head", 4, 10, 256, *([None] * 7), 1, None, None, None)
    assert b"null pointer" in _ffi.load().demf_last_error()
    assert _ffi.CONSTANTS["DEMF_ATTN_EVAL_MAX_Q"] == 512 and _ffi.CONSTANTS["DEMF_DETR2D_MAX_CANDIDATES"] == 8192
    assert _ffi.CONSTANTS["DEMF_DETR2D_MAX_K"] == 1024


def test_operators_refuse_cpu_tensors():
    from demf_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_eval(torch.zeros(6, 768), 2, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.detr2d_head(torch.zeros(3, 256), torch.zeros(3, 256), torch.zeros(10, 256), torch.zeros(10),
                        torch.zeros(4, 256), torch.zeros(4), torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.detr2d_select(torch.zeros(1, 3, 10), torch.zeros(1, 3, 4), torch.zeros(1, 6), 5, 0.09, False,
                          torch.zeros(1, 5, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_store_reserve_reset_and_results():
    from demf_amd.detections import Detection2DStore
    st = Detection2DStore(3, k=4, device="cpu")
    assert len(st) == 0 and tuple(st.rows.shape) == (3, 4, 6) and st.counts.dtype == torch.int32
    assert st.reserve(2, 4) == 0 and len(st) == 2
    with pytest.raises(RuntimeError, match="2 more do not fit"):
        st.reserve(2, 4)
    with pytest.raises(RuntimeError, match="k = 4"):
        st.reserve(1, 5)
    st.rows[0, :2] = torch.tensor([[1., 2, 3, 4, 0.9, 7], [0, 0, 5, 5, 0.5, 2]])
    st.counts[:2] = torch.tensor([2, 0], dtype=torch.int32)
    res = st.results()
    assert [tuple(r.shape) for r in res] == [(2, 6), (0, 6)] and res[0][0, 5] == 7
    per = st.results(per_class=True, num_classes=10)
    assert len(per) == 2 and len(per[0]) == 10 and per[0][7].shape == (1, 5) and per[0][2].shape == (1, 5)
    assert per[0][0].shape == (0, 5) and per[0][7].dtype == np.float32
    st.flag[0] = 1
    with pytest.raises(RuntimeError, match="NaN"):
        st.results()
    st.reset()
    assert len(st) == 0 and int(st.flag) == 0 and st.reserve(3, 4) == 0
    with pytest.raises(ValueError):
        Detection2DStore(0, device="cpu")


def test_test_side_only():
    m = _tiny()
    with pytest.raises(NotImplementedError):
        m.extract_bboxes_2d(None, None, train=True)
    with pytest.raises(NotImplementedError):
        m.train()
    assert not m.training and not any(p.requires_grad for p in m.parameters())


def test_command_line_of_the_2d_detector(capsys):
    from demf_amd.infer import parse_args
    base = ["--data-root", "R", "--ann-file", "F", "--checkpoint", "C", "--model", "detr2d"]
    a = parse_args(base + ["--out", "o.pkl"])
    assert a.no_eval and a.score_thr == 0.09 and a.max_per_img == 100
    a = parse_args(base + ["--out", "o.pkl", "--score-thr", "0.3", "--max-per-img", "50"])
    assert a.score_thr == 0.3 and a.max_per_img == 50
    for extra, word in ((["--out", "o.pkl", "--gpus", "2"], "--gpus"), (["--out", "o.pkl", "--tta-scales", "0.9,1.1"], "tta"),
                        ([], "--out is required"), (["--out", "o.pkl", "--feature-cache", "D"], "feature-cache")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--data-root", "R", "--ann-file", "F", "--checkpoint", "C", "--score-thr", "0.2"])
    assert "go with --model detr2d" in capsys.readouterr().err
