"""The three kernels of csrc/detr2d.hip against the fp64 restatement (tests/detr2d_reference.py)."""
import os

import numpy as np
import pytest
import torch

import detr2d_reference as ref

pytestmark = pytest.mark.gpu


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _close(a, b, tol, name=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item()
    print(f"{name}: max err {err:.3e}, scale {b.abs().max().item():.3f}, bound {tol:.1e} of scale")
    assert err <= tol * max(1.0, b.abs().max().item()), f"{name}: max err {err:.3e} (scale {b.abs().max().item():.2f})"


# ---- demf_attn_fwd_eval -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 300, 512])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attn_eval_vs_fp64(mode, Q):
    """softmax(q k^T / sqrt d) v for B = 2, H = 8, Dh = 32: every output element written (NaN pre-fill), 1e-5 of scale
    in f32 mode, 2e-2 in bf16 mode against the statement with q, k, v rounded where the kernel rounds them - the bars
    demf_attn_core_fwd is held to; at Q = 256 the two kernels are compared in the attention-core test below."""
    from demf_amd import ops
    B, H, Dh = 2, 8, 32
    qkv = _r(B * Q, 3 * H * Dh, seed=Q, scale=1.5)
    out = torch.full((B * Q, H * Dh), float("nan"), device="cuda")
    ops.set_compute_dtype(mode)
    try:
        got = ops.attn_eval(qkv, B, H, out=out)
    finally:
        ops.set_compute_dtype("f32")
    assert got is out and torch.isfinite(out).all()
    x = qkv.float().bfloat16().double() if mode == "bf16" else qkv.double()
    _close(out, ref.attention(x.cpu(), B, H), 2e-2 if mode == "bf16" else 1e-5, f"attn_eval Q={Q} {mode}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attn_eval_agrees_with_the_attention_core_at_256(mode):
    from demf_amd import _ffi, ops
    B, H, Q, Dh = 2, 8, 256, 32
    qkv = _r(B * Q, 3 * H * Dh, seed=3, scale=1.5)
    core, stats = torch.empty(B * Q, H * Dh, device="cuda"), torch.empty(B * H * Q, 2, device="cuda")
    ops.set_compute_dtype(mode)
    try:
        _ffi.call("demf_attn_core_fwd", B, H, Q, Dh, qkv.data_ptr(), 1.0 / np.sqrt(Dh), 0.0, None, 0, core.data_ptr(),
                  stats.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
        got = ops.attn_eval(qkv, B, H)
    finally:
        ops.set_compute_dtype("f32")
    _close(got, core, 2e-2 if mode == "bf16" else 1e-5, f"attn_eval vs attn_core {mode}")


# ---- demf_detr2d_head -----------------------------------------------------------------------------------------------
SPECIAL_REF = [(0.0, 1.0), (1e-6, 1.0 - 1e-6), (1.0, 0.0), (3e-6, 0.5), (1.0 - 3e-6, 1e-5), (-0.25, 1.25)]


@pytest.mark.parametrize("C", [1, 10])
@pytest.mark.parametrize("R", [1, 7, 600])
def test_detr2d_head_vs_fp64(R, C):
    """Logits 1e-5 of scale, normalised boxes 1e-5 absolute (fp32 log / sigmoid err a few 1e-7, slope <= 1/4);
    reference points exactly 0, exactly 1, inside the eps clamp and outside [0, 1]; at R = 600 the 300 reference
    rows are shared by two images (row r reads reference[r % 300])."""
    from demf_amd import ops
    K = 256
    hs, hid = _r(R, K, seed=R + C), _r(R, K, seed=R + C + 1).relu()
    wc, bc = _r(C, K, seed=5, scale=1 / 16), _r(C, seed=6)
    wr, br = _r(4, K, seed=7, scale=1 / 16), _r(4, seed=8)
    nref = 300 if R == 600 else R
    rp = torch.rand(nref, 2, generator=torch.Generator().manual_seed(9))
    n = min(nref, len(SPECIAL_REF))
    rp[:n] = torch.tensor(SPECIAL_REF[:n])
    rp = rp.cuda()
    logits = torch.full((R, C), float("nan"), device="cuda")
    boxes = torch.full((R, 4), float("nan"), device="cuda")
    ops.detr2d_head(hs, hid, wc, bc, wr, br, rp, logits, boxes)
    wl, wb = ref.head_tail(hs.cpu(), hid.cpu(), wc.cpu(), bc.cpu(), wr.cpu(), br.cpu(), rp.cpu().repeat(R // nref, 1))
    _close(logits, wl, 1e-5, f"logits R={R} C={C}")
    err = (boxes.double().cpu() - wb).abs().max().item()
    print(f"boxes R={R} C={C}: max abs err {err:.3e}")
    assert err <= 1e-5 and torch.isfinite(boxes).all()


# ---- demf_detr2d_select ---------------------------------------------------------------------------------------------
META = torch.tensor([[480., 640., 1.25, 1.5, 1.25, 1.5], [375., 500., 0.8, 0.75, 0.8, 0.75],
                     [600., 333., 2.0, 2.0, 2.0, 2.0]])
SHAPES = [(300, 10, 100), (7, 10, 100), (300, 10, 1), (819, 10, 100), (300, 1, 100)]


def _candidates(Q, C, seed, k=100, ties=False):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(3, Q, C, generator=g) * 2.5 - 1.0
    if ties:
        lg = torch.round(lg)                 # runs of bit-equal logits across queries and classes
    else:
        # images 1 and 2: the score threshold falls about halfway into the k selected places (image 0: behind them)
        m = max(1, min(k, Q * C) // 2)
        for b in (1, 2):
            lg[b] += ref.THR_LOGIT - torch.sort(lg[b].reshape(-1), descending=True)[0][m - 1 + b] + 0.05
        lg[(lg - ref.THR_LOGIT).abs() < 2e-3] += 0.01       # nothing inside the threshold's rounding band
    bx = torch.rand(3, Q, 4, generator=g)
    bx[..., 2:] *= 0.8
    bx[:, ::5, 0] *= 0.1                     # boxes over the left / top border: the clamp
    bx[:, 1::7, 1] = 1.0 - 0.1 * bx[:, 1::7, 1]
    return lg, bx


def _run_select(lg, bx, k, thr, rescale):
    from demf_amd import ops
    B = lg.shape[0]
    rows = torch.full((B, k, 6), float("nan"), device="cuda")
    counts = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.detr2d_select(lg.cuda(), bx.cuda(), META.cuda(), k, thr, rescale, rows, counts, flag)
    torch.cuda.synchronize()
    return rows.cpu(), counts.cpu(), int(flag.item())


def _check_select(lg, bx, k, thr, rescale):
    """Rows, order and counts against the restatement; a second run whose boxes encode the query index (zero size,
    cx = (q + 0.5) / Q) recovers the selected (query, label) pairs exactly."""
    B, Q, C = lg.shape
    # condition on the inputs: no logit within 1e-3 of the threshold's logit, so the prefix cannot differ by rounding
    assert thr < 0 or not bool(((lg.double() - np.log(thr / (1 - thr))).abs() < 1e-3).any())
    want = ref.select(lg, bx, META, k, thr, rescale)
    rows, counts, flag = _run_select(lg, bx, k, thr, rescale)
    assert flag == 0
    enc = torch.zeros(B, Q, 4)
    enc[..., 0] = (torch.arange(Q, dtype=torch.float64)[None] + 0.5).float() / Q
    enc[..., 1] = 0.5
    qrows, qcounts, _ = _run_select(lg, enc, k, thr, False)
    for b in range(B):
        n = want[b]["n"]
        assert int(counts[b]) == n == int(qcounts[b]), (b, int(counts[b]), n)
        got = rows[b].double().numpy()
        assert not got[n:].any(), "rows beyond the count are zero"
        w = want[b]["rows"]
        assert np.array_equal(got[:n, 5], w[:, 5]), "labels, in order"
        q = np.round(qrows[b, :n, 0].double().numpy() / float(META[b, 1]) * Q - 0.5).astype(np.int64)
        assert np.array_equal(q, want[b]["idx"][:n] // C), "queries, in order"
        assert np.array_equal(qrows[b, :n, 5].numpy().astype(np.int64), want[b]["idx"][:n] % C)
        if n:
            assert np.abs(got[:n, 4] - w[:, 4]).max() <= 1e-6, "scores"
            ih, iw = float(META[b, 0]), float(META[b, 1])
            ext = np.array([iw, ih, iw, ih]) / (META[b, 2:6].double().numpy() if rescale else 1.0)
            assert (np.abs(got[:n, :4] - w[:, :4]) <= 1e-5 * ext).all(), "pixel coordinates"
    return want


@pytest.mark.parametrize("Q,C,k", SHAPES)
def test_detr2d_select_is_exact(Q, C, k):
    lg, bx = _candidates(Q, C, seed=Q + C + k, k=k)
    for thr in (-1.0, 0.09):
        for rescale in (False, True):
            want = _check_select(lg, bx, k, thr, rescale)
            if thr < 0:
                assert all(w["n"] == min(k, Q * C) for w in want)
    assert any(0 < w["n"] < min(k, Q * C) for w in want) or k == 1 or Q * C < k, "the threshold cuts inside the k places"


def test_detr2d_select_breaks_ties_by_flat_index():
    """Bit-equal logits across queries and classes, also across the k-th place: the lower flat index q * C + c first."""
    Q, C, k = 300, 10, 100
    lg, bx = _candidates(Q, C, seed=11, ties=True)
    s = torch.sort(lg.reshape(3, -1), 1, descending=True)[0]
    assert bool((s[:, k - 1] == s[:, k]).all()) and bool((s[:, :k - 1] == s[:, 1:k]).any())
    for thr in (-1.0, 0.09):
        _check_select(lg, bx, k, thr, True)


def test_detr2d_select_flags_nan_and_orders_it_last():
    from demf_amd.detections import Detection2DStore
    from demf_amd import ops
    Q, C, k = 7, 10, 100
    lg, bx = _candidates(Q, C, seed=2)
    lg[1, 3, 4] = float("nan")
    want = ref.select(lg, bx, META, k, -1.0, False)
    rows, counts, flag = _run_select(lg, bx, k, -1.0, False)        # (the launch ends normally)
    assert flag == 1 and counts.tolist() == [70, 70, 70]
    assert int(want[1]["idx"][-1]) == 3 * C + 4 and torch.isnan(rows[1, 69, 4]) and int(rows[1, 69, 5]) == 4
    assert np.array_equal(rows[1, :69, 5].numpy(), want[1]["rows"][:69, 5])
    assert torch.isfinite(rows[0]).all() and torch.isfinite(rows[2]).all()
    store = Detection2DStore(3, k=k)
    first = store.reserve(3, k)
    ops.detr2d_select(lg.cuda(), bx.cuda(), META.cuda(), k, 0.09, False, store.rows[first:first + 3],
                      store.counts[first:first + 3], store.flag)
    with pytest.raises(RuntimeError, match="NaN"):
        store.results()


_SYNC_DEBUG_CHILD = r"""
import torch
from demf_amd import ops
from demf_amd.detections import Detection2DStore
g = torch.Generator().manual_seed(0)
B, Q, C, K, k = 2, 300, 10, 256, 100
r = lambda *s: torch.randn(*s, generator=g).cuda()
hs, hid, wc, bc, wr, br = r(B * Q, K), r(B * Q, K).relu(), r(C, K) / 16, r(C), r(4, K) / 16, r(4)
rp = torch.rand(Q, 2, generator=g).cuda()
meta = torch.tensor([[480., 640., 1, 1, 1, 1], [375., 500., 1, 1, 1, 1]]).cuda()
store = Detection2DStore(2 * B, k=k)
logits, boxes = torch.empty(B * Q, C, device="cuda"), torch.empty(B * Q, 4, device="cuda")
torch.cuda.synchronize()
torch.cuda.set_sync_debug_mode("error")
try:
    for _ in range(2):
        ops.detr2d_head(hs, hid, wc, bc, wr, br, rp, logits, boxes)
        first = store.reserve(B, k)
        ops.detr2d_select(logits.view(B, Q, C), boxes.view(B, Q, 4), meta, k, store.score_thr, False,
                          store.rows[first:first + B], store.counts[first:first + B], store.flag)
finally:
    torch.cuda.set_sync_debug_mode("default")
res = store.results()
assert len(res) == 4 and all(torch.equal(a, b) for a, b in zip(res[:2], res[2:]))
assert all(0 < len(a) <= k for a in res) and all((a[:, 4] > 0.09).all() for a in res)
print("SYNC_DEBUG_OK")
"""


def test_head_select_and_append_do_not_synchronise():
    """Under torch.cuda.set_sync_debug_mode("error"), in a process of its own (as tests/test_gpu_detections.py)."""
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", _SYNC_DEBUG_CHILD], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SYNC_DEBUG_OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
