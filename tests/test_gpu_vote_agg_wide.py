"""The vote aggregation's 256 -> 256 layers on the one-launch backward (demf_mlp_bwd_fused_wide, csrc/mlp_bwd.hip:
all 128-column chunks of the layer below in ONE launch of the (256, 128) one-pass kernel, chunk and slab sequence
derived from the block id - csrc/wide_map.h).

Everything is driven through ops.shared_mlp_pool(x, ns, layers, True) with 128 input channels and the channels
(256, 256, 256): layers 2 and 3 are the wide layers (layer 3 with the sparse pooled gradient, layer 2 with a dense
one); layer 1 reads the raw input rows and keeps its weight-gradient and input-gradient launches.

Method and bars of tests/test_gpu_mlp.py::test_shared_mlp_pool_fwd_bwd, restated: an fp64 reference of
(linear -> train-mode batch norm -> relu) x 3 -> max over ns whose BACKWARD runs on the kernels' own ReLU masks and
pooled rows (read from the tensors the autograd node saved), after checking that those decisions differ from the fp64
reference's in at most 4 + numel / 10^6 places, all at |z| < 2e-5; output within 1e-4 of scale, every gradient within
1e-3 of scale, running statistics within 1e-4.  The fp64 reference is evaluated on the device (65 536 x 256 rows).
bf16 mode: the bar of tests/test_gpu_mlp_bwd_fused.py for these entry points - the same stack on the two-launch path,
identical outputs, gradients within 3e-3 of scale.

Which kernel form ran is read back per call from demf_mlp_last_form() by a spy on _ffi.call: a dispatch condition
that silently stops matching would otherwise pass every numeric check on the slower kernel.  The FORWARD of layers 2
and 3 is not changed (the producer / consumer forward takes 128-channel inputs only): asserted as mlp_gemm_kernel -
for layer 2 at up to 16 384 rows the few-row tile kernel."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GENERIC, TILE, RES, PC, FUSED, FUSED_COLS, FUSED_WIDE, POOL = 1, 2, 3, 4, 5, 6, 7, 8     # include/demf_hip.h DEMF_FORM_*
LD, CHANS = 128, (256, 256, 256)

CASES = [  # (groups, ns)
    (1024, 16),     # R = 16 384: exactly the dispatch threshold; 512 slabs over 2 x 120 workgroups
    (1028, 16),     # R = 16 448: 514 slabs - uneven slab counts between the workgroups of a chunk
    (1026, 16),     # R = 16 416: R % 64 = 32, an odd slab count (513)
    (512, 32),      # ns = 32 groups in the sparse gradient
    (4096, 16),     # R = 65 536: 2 048 slabs, more than eight per workgroup
]


@functools.lru_cache(maxsize=None)
def _inputs(Rp, ns):
    """fp64 inputs as tests/test_gpu_mlp.py builds them: a negative BN scale on a layer below, a negative and a zero
    scale on the pooled layer, weights randn / sqrt(K)."""
    g = torch.Generator().manual_seed(1000 * ns + Rp)
    R = Rp * ns
    x = torch.randn(R, LD, generator=g, dtype=torch.float64) * 0.7 + 0.1
    layers, k = [], LD
    for n in CHANS:
        layers.append((torch.randn(n, k, generator=g, dtype=torch.float64) / np.sqrt(k),
                       1.0 + 0.2 * torch.randn(n, generator=g, dtype=torch.float64),
                       0.1 * torch.randn(n, generator=g, dtype=torch.float64)))
        k = n
    layers[0][1][0] = -0.7
    layers[1][1][3] = -0.6
    layers[-1][1][1] = -0.5
    layers[-1][1][2] = 0.0
    go = torch.randn(Rp, CHANS[-1], generator=g, dtype=torch.float64)
    return x.cuda(), [tuple(t.cuda() for t in l) for l in layers], go.cuda()


def _bn(y, g, b, eps=1e-5):
    mean, var = y.mean(0), y.var(0, unbiased=False)
    return (y - mean) / torch.sqrt(var + eps) * g + b


@functools.lru_cache(maxsize=None)
def _forward64(Rp, ns):
    """The fp64 forward of a case, computed once: pre-activations z_l, raw outputs' running statistics, pooled output."""
    x, layers, _ = _inputs(Rp, ns)
    zs, stats, h = [], [], x
    with torch.no_grad():
        for W, g, b in layers:
            y = h @ W.t()
            stats.append((0.1 * y.mean(0), 0.9 + 0.1 * y.var(0, unbiased=True)))
            z = _bn(y, g, b)
            zs.append(z)
            h = torch.relu(z)
        out = h.view(Rp, ns, -1).max(1).values
    return zs, stats, out


def _run(Rp, ns, record=None):
    """One forward + backward on the kernels; ``record`` collects (entry point, form it took) per call."""
    from demf_amd import _ffi, ops
    x, layers, go = _inputs(Rp, ns)
    xg = x.float().requires_grad_(True)
    lg = []
    for W, g, b in layers:
        n = W.shape[0]
        lg.append((W.float().requires_grad_(), g.float().requires_grad_(), b.float().requires_grad_(),
                   torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")))
    orig = _ffi.call
    lib = _ffi.load()

    def spy(name, *a):
        rc = orig(name, *a)
        if record is not None:
            record.append((name, lib.demf_mlp_last_form()))
        return rc
    try:
        _ffi.call = spy
        out = ops.shared_mlp_pool(xg, ns, lg, True)
        saved = out.grad_fn.saved_tensors
        out.backward(go.float())
    finally:
        _ffi.call = orig
    grads = [t.grad for l in lg for t in l[:3]] + [xg.grad]
    return out.detach(), grads, saved, lg


def _forms(record, prefix):
    return [(n, f) for n, f in record if n.startswith(prefix)]


def _check_forms(record, R, wide):
    """Forward: three GEMM launches; the pooled layer 3 on mlp_gemm_kernel, layer 2 too (up to 16 384 rows: on the
    few-row tile kernel).  Backward: layers 3 and 2 on the wide form (or, with it switched off, on the two-launch path:
    an input-gradient launch each, no one-pass call for them).  Layer 1 (raw 128-channel input rows, no layer below)
    has no one-pass form."""
    fwd = _forms(record, "demf_mlp_gemm_fwd")
    assert len(fwd) == 3, fwd
    assert [f for _, f in fwd[1:]] == [TILE if R <= 16384 else GENERIC, GENERIC], fwd
    names = [n for n, _ in record]
    if wide:
        w = _forms(record, "demf_mlp_bwd_fused_wide")
        assert len(w) == 2 and all(f == FUSED_WIDE for _, f in w), w
        assert not _forms(record, "demf_mlp_gemm_bwd_dx_red") and "demf_mlp_bwd_fused_cols" not in names
    else:
        assert "demf_mlp_bwd_fused_wide" not in names and "demf_mlp_bwd_fused_cols" not in names
        dx = _forms(record, "demf_mlp_gemm_bwd_dx_red")
        assert len(dx) == 2 and all(f in (GENERIC, TILE) for _, f in dx), dx


def _close(a, b, tol, name):
    a, b = a.detach().double(), b.detach().double()
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    print("%-14s err %.3e  bar %.3e" % (name, err, tol * scale))
    assert err <= tol * scale, f"{name}: err {err:.3e} > {tol:g} x {scale:.3e}"


def _check_against_fp64(Rp, ns, out, grads, saved, lg):
    x, layers, go = _inputs(Rp, ns)
    zs, stats, out_r = _forward64(Rp, ns)
    L = len(CHANS)
    arg = saved[1].long()
    masks = []
    for l in range(L):
        Y, ss = saved[2 + l].double(), saved[2 + L + l].double()
        n = Y.shape[1]
        assert Y.numel() == Rp * ns * n
        m = Y * ss[:n] + ss[n:] > 0                     # exact sign of the kernels' one fma
        diff = m != (zs[l] > 0)
        nd = int(diff.sum())
        assert nd <= 4 + zs[l].numel() // 10 ** 6, f"layer {l}: {nd} ReLU masks differ"
        assert nd == 0 or zs[l][diff].abs().max().item() < 2e-5, f"layer {l}: mask differs at |z| = {zs[l][diff].abs().max().item():.2e}"
        masks.append(m)
    top = torch.relu(zs[-1]).view(Rp, ns, -1)
    picked = top.gather(1, arg.view(Rp, 1, -1)).squeeze(1)
    assert (top.max(1).values - picked).abs().max().item() < 2e-5, "pooled row is not (within round-off) the maximum"

    xr = x.clone().requires_grad_(True)
    lr = [tuple(t.clone().requires_grad_() for t in l) for l in layers]
    h = xr
    for (W, g, b), m in zip(lr, masks):
        h = _bn(h @ W.t(), g, b) * m
    h.view(Rp, ns, -1).gather(1, arg.view(Rp, 1, -1)).squeeze(1).backward(go)

    _close(out, out_r, 1e-4, "out")
    for i, rl in enumerate(lr):
        _close(grads[3 * i], rl[0].grad, 1e-3, f"dW{i}")
        _close(grads[3 * i + 1], rl[1].grad, 1e-3, f"dgamma{i}")
        _close(grads[3 * i + 2], rl[2].grad, 1e-3, f"dbeta{i}")
    _close(grads[-1], xr.grad, 1e-3, "dx")
    for i, (rm, rv) in enumerate(stats):
        _close(lg[i][3], rm, 1e-4, f"running_mean{i}")
        _close(lg[i][4], rv, 1e-4, f"running_var{i}")


def _wide_expected():
    from demf_amd import ops
    return ops._FUSED_WIDE_MIN_R > 0 and ops._FUSED_COLS_MIN_R <= 0 and not ops._NO_BWD_FUSE


@pytest.mark.parametrize("Rp,ns,mode", [c + ("f32",) for c in CASES] + [c + ("f32x3",) for c in CASES[:2]])
def test_wide_backward_against_fp64_on_the_kernels_branch(Rp, ns, mode):
    from demf_amd import ops
    if "DEMF_TEST_EXPECT_WIDE" in os.environ:       # (set by the switch test's child process: the switch must have arrived)
        assert _wide_expected() == bool(int(os.environ["DEMF_TEST_EXPECT_WIDE"]))
    ops.set_compute_dtype(mode)
    try:
        record = []
        out, grads, saved, lg = _run(Rp, ns, record)
    finally:
        ops.set_compute_dtype("f32")
    _check_forms(record, Rp * ns, wide=_wide_expected())
    _check_against_fp64(Rp, ns, out, grads, saved, lg)


@pytest.mark.parametrize("Rp,ns", CASES[:2])
def test_wide_backward_bf16_equals_the_two_launch_path(Rp, ns):
    from demf_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        record = []
        out_w, g_w, _, _ = _run(Rp, ns, record)
        _check_forms(record, Rp * ns, wide=True)
        ops._NO_BWD_FUSE = True
        calls = []
        out_u, g_u, _, _ = _run(Rp, ns, calls)
        assert not [n for n, _ in calls if n.startswith("demf_mlp_bwd_fused")]
    finally:
        ops._NO_BWD_FUSE = False
        ops.set_compute_dtype("f32")
    assert torch.equal(out_w, out_u)
    for i, (a, b) in enumerate(zip(g_w, g_u)):
        scale = max(1e-6, float(b.abs().max()))
        err = float((a - b).abs().max())
        print("bf16 gradient %d: err %.3e scale %.3e" % (i, err, scale))
        assert err <= 3e-3 * scale, (i, err, scale)


def test_wide_backward_equals_the_per_chunk_form():
    """Same kernel, same operands, another accumulation order (half as many dW partials, other row ranges per
    workgroup): identical forward, gradients within 2e-5 of scale in f32."""
    from demf_amd import ops
    Rp, ns = 1028, 16
    cols_min = ops._FUSED_COLS_MIN_R
    try:
        record = []
        out_w, g_w, _, _ = _run(Rp, ns, record)
        _check_forms(record, Rp * ns, wide=True)
        ops._FUSED_COLS_MIN_R = 16384
        record = []
        out_c, g_c, _, _ = _run(Rp, ns, record)
        cols = _forms(record, "demf_mlp_bwd_fused_cols")
        assert len(cols) == 4 and all(f == FUSED_COLS for _, f in cols), cols
        assert not _forms(record, "demf_mlp_bwd_fused_wide")
    finally:
        ops._FUSED_COLS_MIN_R = cols_min
    assert torch.equal(out_w, out_c)
    for i, (a, b) in enumerate(zip(g_w, g_c)):
        scale = max(1e-6, float(b.abs().max()))
        err = float((a - b).abs().max())
        print("gradient %d: err %.3e scale %.3e" % (i, err, scale))
        assert err <= 2e-5 * scale, (i, err, scale)


def test_switch_off_takes_the_two_launch_path():
    """DEMF_FUSED_WIDE_MIN_R=0 in a fresh process: the 1024 x 16 f32 case again - the backward of layers 2 and 3 on the
    two-launch path (asserted by the case itself from the switch's value), the same bars."""
    env = dict(os.environ, DEMF_FUSED_WIDE_MIN_R="0", DEMF_TEST_EXPECT_WIDE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_vote_agg_wide.py") +
                        "::test_wide_backward_against_fp64_on_the_kernels_branch[1024-16-f32]"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "1 passed" in r.stdout
