"""The 2D detector on the device: kernel path against module path against the fp64 restatement, the cached weight-only
pieces, predict_into / the store, and the runner's command line."""
import os
import pickle

import numpy as np
import pytest
import torch

import detr2d_reference as ref
import pipeline_reference as pref
from oracle import fixtures

pytestmark = pytest.mark.gpu

PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3)]
# widths the convolution kernels take, so the whole detector runs without a library kernel
WIDTHS = dict(base=64, blocks=(1, 1, 1, 1), embed_dims=256, num_layers=1, num_heads=8, feedforward_channels=256,
              gn_groups=32, num_feats=128)
SPECS = [(6000, (53, 73), 3), (5000, (43, 56), 0), (7000, (44, 59), 4), (4500, (48, 64), 2)]
IMG_SCALE = (320, 240)


def _head(Q, seed=3, layers=2):
    from demf_amd.modules import DeformableDETRHead
    head = DeformableDETRHead(Q, 10, 256, num_layers=layers, num_heads=8, feedforward_channels=384)
    fixtures.seed_weights(head, seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                       # offsets / logits that actually depend on the query
        for layer in head.transformer.decoder.layers:
            a = layer.attentions[1]
            a.sampling_offsets.weight.copy_(torch.randn(a.sampling_offsets.weight.shape, generator=g) * 0.02)
            a.attention_weights.weight.copy_(torch.randn(a.attention_weights.weight.shape, generator=g) * 0.05)
    return head.cuda().eval()


def _memory(seed=1, B=3):
    from demf_amd.modules.image_stream import DeformableDetrEncoder
    _, metas = fixtures.make_images(5, B=B, H=96, W=160)
    st = DeformableDetrEncoder(num_layers=1)._static(metas, PYRAMID, torch.device("cuda"))
    S = sum(h * w for h, w in PYRAMID)
    tokens = torch.randn(B, S, 256, generator=torch.Generator().manual_seed(seed)).cuda()
    return dict(tokens=tokens, spatial=PYRAMID, mask_flatten=st["mask_flatten"], valid_ratios=st["valid_ratios"]), st


def _err(got, want, name):
    got, want = got.double().cpu(), want.double().cpu()
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(f"{name}: max err {err:.3e}, scale {scale:.3f}")
    return err, scale


def _both_paths(head, enc, st, mode, value_one):
    from demf_amd import ops
    from demf_amd.modules import detr2d
    ops.set_compute_dtype(mode)
    prev, prev_value = ops.LIBRARY_FALLBACK, detr2d.VALUE_ONE_LAUNCH
    try:
        detr2d.VALUE_ONE_LAUNCH = value_one
        detr2d.FUSED = False
        want = head(enc, st)
        assert head.last_path == "modules"
        detr2d.FUSED = True
        ops.LIBRARY_FALLBACK = False             # the kernel path calls no library fall-back
        assert head.fused_ok(enc["tokens"])
        got = head(enc, st)
        assert head.last_path == "kernels"
    finally:
        detr2d.FUSED, detr2d.VALUE_ONE_LAUNCH = True, prev_value
        ops.LIBRARY_FALLBACK = prev
        ops.set_compute_dtype("f32")
    return got, want


@pytest.mark.parametrize("value_one", [True, False], ids=["values_one_launch", "values_per_layer"])
@pytest.mark.parametrize("Q", [300, 37])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_kernel_path_matches_the_module_path(mode, Q, value_one):
    """embed 256, 8 heads, 4 levels, P = 4, 2 decoder layers, B = 3 padded images: decoder output and logits within
    1e-4 of scale (f32 mode) / 3e-2 (bf16 mode) - the bars of test_fused_encoder_layers_match_the_module_path -, boxes
    within 1e-4 normalised.  In the bf16 mode a box is the sigmoid (slope <= 1/4) of a sum that carries the logits' own
    bf16 bar, so its bound there is 3e-2 / 4 = 7.5e-3: the two paths round to bf16 at different points and 1e-4 is
    below what the format allows (measured on MI355X: 2.3e-3 at Q = 300, 1.9e-3 at Q = 37; f32 mode 3.3e-7).  Both
    forms of the value projection: one launch for all layers (the default) and one per layer."""
    head = _head(Q)
    enc, st = _memory()
    assert st["mask_flatten"].any()
    (hs, lg, bx), (whs, wlg, wbx) = _both_paths(head, enc, st, mode, value_one)
    tol = 1e-4 if mode == "f32" else 3e-2
    for got, want, name in ((hs, whs, "decoder output"), (lg, wlg, "logits")):
        err, scale = _err(got, want, f"{name} Q={Q} {mode}")
        assert err <= tol * scale, (name, err, scale)
    err, _ = _err(bx, wbx, f"boxes Q={Q} {mode}")
    assert err <= (1e-4 if mode == "f32" else 3e-2 / 4)
    assert all(torch.isfinite(t).all() for t in (hs, lg, bx)) and tuple(bx.shape) == (3, Q, 4)


def test_module_path_matches_the_fp64_restatement():
    from demf_amd.modules import detr2d
    head = _head(300)
    enc, st = _memory()
    try:
        detr2d.FUSED = False
        hs, lg, bx = head(enc, st)
    finally:
        detr2d.FUSED = True
    sd = {"img_bbox_head." + k: v for k, v in head.state_dict().items()}
    whs, wref = ref.decoder(sd, enc["tokens"], enc["mask_flatten"], enc["valid_ratios"], PYRAMID, 2)
    wlg, wbx = ref.branches(sd, whs[-1], wref, 1)
    for got, want, name in ((hs, whs[-1], "decoder output"), (lg, wlg, "logits")):
        err, scale = _err(got, want, name + " vs fp64")
        assert err <= 1e-4 * scale, (name, err, scale)
    assert _err(bx, wbx, "boxes vs fp64")[0] <= 1e-4


def test_weight_only_pieces_follow_a_load_state_dict():
    """The reference points and layer 0's self-attention block are cached per weight version: after loading other
    weights the kernel path computes what a freshly built model computes."""
    head, other = _head(300, seed=3), _head(300, seed=4)
    enc, st = _memory()
    first = head(enc, st)
    assert head.last_path == "kernels"
    pk = head._pack(3)
    assert head._pack(3) is pk
    head.load_state_dict(other.state_dict())
    got, want = head(enc, st), other(enc, st)
    assert head._pack(3) is not pk
    for a, b, c in zip(got, want, first):
        assert torch.equal(a, b)
        assert not torch.allclose(a, c, atol=1e-3)


def _detector(seed=1, num_query=37):
    from demf_amd.modules import Detr2D
    det = Detr2D(num_query=num_query, num_decoder_layers=2, **WIDTHS)
    fixtures.seed_weights(det, seed)
    with torch.no_grad():     # two classes far above the score threshold, eight far below: 74 of the k = 100 places pass
        det.img_bbox_head.cls_branches[0].bias.copy_(torch.tensor([8., -12, -12, 8, -12, -12, -12, -12, -12, -12]))
        det.img_bbox_head.reg_branches[0][4].weight.mul_(4.0)
    return det


@pytest.mark.no_library_fallback
def test_predict_into_fills_the_store_in_image_order():
    """Two batches through predict_into: results() equals extract_bboxes_2d per image and the restatement's selection
    on the same logits; simple_test_img_only returns all k places.  (Two forwards of the image stream differ in the
    last bits - its split-K convolutions add their partial tiles atomically -, so runs are compared at the bar of
    tests/test_gpu_detections.py::_assert_same_run, not bit for bit.)"""
    from demf_amd.detections import Detection2DStore
    from demf_amd.modules.detr2d import meta_rows
    det = _detector().cuda()
    k = det.img_bbox_head.max_per_img
    batches = []
    for seed in (5, 6):
        img, metas = fixtures.make_images(seed, B=2, H=96, W=160)
        for m in metas:
            m["scale_factor"] = np.asarray([0.5, 0.5, 0.5, 0.5], np.float32)
        batches.append((torch.from_numpy(img).cuda(), metas))
    store = Detection2DStore(4, k=k)
    for img, metas in batches:
        det.predict_into(store, img=img, img_metas=metas, points=None)
    assert det.img_bbox_head.last_path == "kernels" and len(store) == 4
    res = store.results()
    per = store.results(per_class=True, num_classes=10)
    i = 0
    for img, metas in batches:
        _, logits, boxes = det.forward_head(det.extract_img_feat(img, metas), metas)
        # condition on the inputs: the k-th / (k+1)-th logits and the threshold are separated by more than 1e-3
        assert ref.well_separated(logits.cpu(), k, 0.09)
        want = ref.select(logits.cpu(), boxes.cpu(), meta_rows(metas), k, 0.09, False)
        direct = det.extract_bboxes_2d(img, metas)
        full = det.simple_test_img_only(img, metas, rescale=True)
        wfull = ref.select(logits.cpu(), boxes.cpu(), meta_rows(metas), k, -1.0, True)
        for b in range(2):
            got = res[i]
            assert 0 < len(got) < k and got.shape == direct[b].shape, (len(got), len(direct[b]))
            assert torch.equal(got[:, 5], direct[b][:, 5].cpu())
            assert torch.allclose(got[:, 4], direct[b][:, 4].cpu(), rtol=1e-4, atol=1e-6)
            assert torch.allclose(got[:, :4], direct[b][:, :4].cpu(), rtol=1e-4, atol=1e-3)
            assert len(got) == want[b]["n"] and np.array_equal(got[:, 5].numpy(), want[b]["rows"][:, 5])
            assert np.abs(got[:, 4].double().numpy() - want[b]["rows"][:, 4]).max() <= 1e-6
            assert np.abs(got[:, :4].double().numpy() - want[b]["rows"][:, :4]).max() <= 1e-5 * 160
            assert bool((got[:-1, 4] >= got[1:, 4]).all()) and bool((got[:, 4] > 0.09).all())
            assert sum(len(a) for a in per[i]) == len(got) and len(per[i]) == 10
            assert np.array_equal(per[i][3], got[got[:, 5] == 3, :5].numpy())
            bb, lab = full[b]
            assert tuple(bb.shape) == (k, 5) and lab.dtype == torch.int64
            assert np.array_equal(lab.cpu().numpy(), wfull[b]["rows"][:, 5].astype(np.int64))
            assert np.abs(bb[:, :4].double().cpu().numpy() - wfull[b]["rows"][:, :4]).max() <= 1e-5 * 320
            i += 1
    store.reset()
    assert len(store) == 0


_RUNNER_CHILD = r"""
import sys
import torch
from demf_amd import infer
from demf_amd.modules import Detr2D
root, ann, ckpt, out = sys.argv[1:5]
WIDTHS = dict(base=64, blocks=(1, 1, 1, 1), embed_dims=256, num_layers=1, num_heads=8, feedforward_channels=256,
              gn_groups=32, num_feats=128)
ret = infer.main(["--model", "detr2d", "--data-root", root, "--ann-file", ann, "--checkpoint", ckpt, "--out", out,
                  "--batch-size", "3", "--workers", "2", "--score-thr", "0.05", "--max-per-img", "50"],
                 model=Detr2D(num_query=37, num_decoder_layers=2, **WIDTHS), num_points=2048, img_scale=(320, 240), seed=1)
assert ret is None
print("RUNNER_OK")
"""


def test_runner_command_line_writes_per_class_results(tmp_path):
    """``demf_amd.infer --model detr2d ... --out`` in a fresh child process on the synthetic dataset of the other
    runner tests: a stage-1 checkpoint in, a pickle of len(dataset) entries with C arrays each out.  (The child
    hands ``infer.main`` a narrow detector: the full-size one would spend the test's time on its 160 MB checkpoint.)"""
    import subprocess
    import sys
    from conftest import ROOT
    from demf_amd.dataset import SUNRGBDDataset
    root = str(tmp_path)
    ann, _ = pref.write_dataset(root, SPECS, jpeg=True)
    n = len(SUNRGBDDataset(root, ann, test_mode=True))
    ckpt, out = os.path.join(root, "stage1.pth"), os.path.join(root, "results.pkl")
    torch.save(dict(meta=dict(epoch=1), state_dict=_detector(seed=2).stage1_state_dict()), ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", _RUNNER_CHILD, root, os.path.basename(ann), ckpt, out], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUNNER_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert "not evaluated" in r.stdout
    with open(out, "rb") as f:
        dumped = pickle.load(f)
    assert len(dumped) == n == 4
    for per in dumped:
        assert len(per) == 10 and all(a.ndim == 2 and a.shape[1] == 5 and a.dtype == np.float32 for a in per)
        assert sum(len(a) for a in per) <= 50 and all((a[:, 4] > 0.05).all() for a in per)
    assert sum(len(a) for per in dumped for a in per) > 0
