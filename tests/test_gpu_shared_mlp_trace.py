"""What ops.shared_mlp_pool LAUNCHES, pinned call by call: the safety net under any restructuring of the shared-MLP
autograd node (demf_amd/ops.py).  The numeric tests (test_gpu_mlp*.py, test_gpu_vote_agg_wide.py, ...) pin which
buffer feeds which launch; this file pins the rest - which entry points run, in which order, with which scalars,
which pointer arguments are null, which kernel form each took, and what the node saves for its backward.

Every case of CASES runs a seeded forward and backward (inputs as tests/test_gpu_mlp_bwd_fused.py::_make builds
them) under the defaults and under every setting of SETTINGS, with a spy on _ffi.call and on ops.dw_job.  The form is
kept per thread, so a case starts from a fixed tiny launch and runs its backward on the calling thread: what a case
records does not depend on the tests before it.  Per call:

  ["demf_...", [scalars], "1011...", form]   an _ffi.call: the c_int / c_longlong / c_float arguments in order, one
                                             character per c_void_p argument (0 = null; the stream is the last), and
                                             demf_mlp_last_form() right after the call
  ["dw_job", [R, N, K, ldx, ns, lddw, dw_off], "10...", defer, leaf is None]
                                             an ops.dw_job: tensor arguments G dP arg Y vec6 xprev pss dW
  ["saved", [[shape, dtype], ...]]           out.grad_fn.saved_tensors, before the backward
  ["grads", [shape | null, ...]]             .grad of every input leaf, after the backward

tests/shared_mlp_trace.json holds the expected lists under "<case> <setting>"; a setting whose trace equals the
case's default trace is stored as the string "= default" (the test compares in that form, so "this switch does not
reach this stack" is pinned too).  The file was produced by this test itself, run on an MI355X with
DEMF_RECORD_TRACE=<path> against the ops.py of the commit BEFORE the node was restructured, and committed unchanged;
regenerate it the same way only when a launch is meant to change.

(An ld % 4 != 0 stack - the transposed-weight demf_mlp_gemm_bwd_dx branch - has no case: the library's forward
refuses K % 4 != 0, csrc/mlp.hip mlp_check, so the branch cannot be reached through the node.)"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

JSON_PATH = os.path.join(ROOT, "tests", "shared_mlp_trace.json")

# (groups, ns, ld, channels, x_grad)
PLAIN = [
    (256, 64, 4, (64, 64, 128), False),          # R = 16 384: the threshold of the no-Y0, no-Y and bf16-row forms
    (255, 64, 4, (64, 64, 128), False),          # R = 16 320: just under it
    (900, 64, 4, (32, 96, 64), False),           # fused first layer with N0 = 32
    (520, 32, 64, (128, 128, 128), True),
    (300, 16, 36, (128, 128, 256), True),
    (1024, 16, 128, (256, 256, 256), True),      # R = 16 384: the threshold of the wide backward
    (1023, 16, 128, (256, 256, 256), True),      # just under it
    (45, 16, 64, (128, 128, 128), True),         # few rows
    (1000, 4, 32, (64, 64, 64), True),
    (1000, 1, 64, (64, 32), True),               # ns = 1
    (50, 8, 36, (32, 32, 64), True),             # ns = 8: pooling as its own launch
    (77, 16, 20, (48, 80, 112), True),           # odd widths
]
# conv biases + num_batches_tracked: the zero bias gradients and the bookkeeping pointer
BIAS = [(300, 16, 36, (128, 128, 256), True), (256, 64, 4, (64, 64, 128), False)]
# the group-first first layer: (B, N, M, ns, C, channels, radius, normalize_xyz) of
# tests/test_gpu_mlp.py::test_factored_first_layer_matches_grouped_reference, with / without coordinate gradients
GEO = [(1, 257, 33, 16, 64, (64, 128), 1.2, False), (2, 300, 64, 64, 8, (256, 64, 64), 0.9, True)]

CASES = ([("plain", c) for c in PLAIN] + [("bias", c) for c in BIAS] + [("eval", PLAIN[0])] +
         [(kind, c) for c in GEO for kind in ("geo", "geo_xyzgrad")])

# (label, module attributes of ops, compute dtype)
SETTINGS = [
    ("default", {}, "f32"),
    ("_NO_BWD_FUSE=True", {"_NO_BWD_FUSE": True}, "f32"),
    ("_POOL_NOY=False", {"_POOL_NOY": False}, "f32"),
    ("_SA1_X4=False", {"_SA1_X4": False}, "f32"),
    ("_NO_FIRST_FUSE=True", {"_NO_FIRST_FUSE": True}, "f32"),
    ("_NO_RED_FUSE=True", {"_NO_RED_FUSE": True}, "f32"),
    ("_NO_FUSED_POOL=True", {"_NO_FUSED_POOL": True}, "f32"),
    ("_VEC_FIN=0", {"_VEC_FIN": 0}, "f32"),
    ("_VEC_FIN=3", {"_VEC_FIN": 3}, "f32"),
    ("_FUSED_COLS_MIN_R=16384", {"_FUSED_COLS_MIN_R": 16384}, "f32"),
    ("_FUSED_WIDE_MIN_R=0", {"_FUSED_WIDE_MIN_R": 0}, "f32"),
    ("bf16", {}, "bf16"),
    ("bf16 _NO_BF16_STORE=False", {"_NO_BF16_STORE": False}, "bf16"),
    ("f32x3", {}, "f32x3"),
]


def _case_id(kind, c):
    return kind + "-" + "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _make(Rp, ns, ld, chans, seed):
    """tests/test_gpu_mlp_bwd_fused.py::_make"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rp * ns, ld, generator=g, dtype=torch.float64) * 0.7 + 0.1
    layers, k = [], ld
    for n in chans:
        layers.append((torch.randn(n, k, generator=g, dtype=torch.float64) / np.sqrt(k),
                       1.0 + 0.2 * torch.randn(n, generator=g, dtype=torch.float64),
                       0.1 * torch.randn(n, generator=g, dtype=torch.float64)))
        k = n
    layers[1][1][3] = -0.6
    go = torch.randn(Rp, chans[-1], generator=g, dtype=torch.float64)
    return x.float().cuda(), [tuple(t.float().cuda() for t in l) for l in layers], go.float().cuda()


@functools.lru_cache(maxsize=None)
def _make_geo(B, N, M, ns, C, chans, radius):
    from demf_amd import ops
    g = torch.Generator().manual_seed(N + ns)
    xyz = (torch.rand(B, N, 3, generator=g, dtype=torch.float64) * 2.0).float().cuda()
    feat = (torch.randn(B, N, C, generator=g, dtype=torch.float64) * 0.6).float().cuda().view(B * N, C)
    centre = ops.gather_rows_cl(xyz, ops.furthest_point_sample(xyz, M))
    idx = ops.ball_query(0.0, radius, ns, xyz, centre)
    inv = ops.invert_index(idx, N)
    layers, k = [], C + 3
    for n in chans:
        layers.append(((torch.randn(n, k, generator=g, dtype=torch.float64) / np.sqrt(k)).float().cuda(),
                       (1.0 + 0.2 * torch.randn(n, generator=g, dtype=torch.float64)).float().cuda(),
                       (0.1 * torch.randn(n, generator=g, dtype=torch.float64)).float().cuda()))
        k = n
    go = torch.randn(B * M, chans[-1], generator=g, dtype=torch.float64).float().cuda()
    return xyz, feat, centre, idx, inv, layers, go


def _settle_form():
    """A fixed tiny launch, so that the form reported after a call that sets none does not depend on what ran before
    this case."""
    from demf_amd import _ffi, ops
    x, W, Y = (torch.zeros(4, 4, device="cuda") for _ in range(3))
    _ffi.call("demf_mlp_gemm_fwd", 4, 4, 4, 4, x.data_ptr(), None, W.data_ptr(), Y.data_ptr(), None, ops._stream())


def _trace(kind, c):
    """One forward (+ backward) of a case under the current switches, spied on."""
    from demf_amd import _ffi, ops
    ops.reset_accumulators()
    training, geo = kind != "eval", None
    if kind.startswith("geo"):
        B, N, M, ns, C, chans, radius, norm = c
        xyz, feat, centre, idx, inv, layers, go = _make_geo(B, N, M, ns, C, chans, radius)
        xyz, centre = xyz.clone(), centre.clone()
        if kind == "geo_xyzgrad":
            xyz.requires_grad_()
            centre.requires_grad_()
        x = feat.clone().requires_grad_()
        geo = (xyz, centre, idx, inv[0], inv[1], radius, norm)
        leaves = [x, xyz, centre]
    else:
        Rp, ns, ld, chans, xgrad = c
        x, layers, go = _make(Rp, ns, ld, chans, Rp + ns)
        x = x.clone().requires_grad_(xgrad)
        leaves = [x]
    ls = []
    for W, gm, bt in layers:
        n = W.shape[0]
        layer = [W.clone().requires_grad_(), gm.clone().requires_grad_(), bt.clone().requires_grad_(),
                 torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")]
        if kind == "bias":
            layer += [torch.full((n,), 0.05, device="cuda").requires_grad_(),
                      torch.zeros((), dtype=torch.int64, device="cuda")]
        ls.append(tuple(layer))
        leaves += [t for t in layer if t.requires_grad]
    lib = _ffi.load()
    scalar = (ctypes.c_int, ctypes.c_longlong, ctypes.c_float)
    rec, orig_call, orig_job = [], _ffi.call, ops.dw_job

    def spy(name, *a):
        rc = orig_call(name, *a)
        sig = _ffi.SIGNATURES[name]
        assert len(sig) == len(a), name
        rec.append([name, [v for t, v in zip(sig, a) if t in scalar],
                    "".join("01"[bool(v)] for t, v in zip(sig, a) if t is ctypes.c_void_p), lib.demf_mlp_last_form()])
        return rc

    def job(R, N, K, ldx, G, dP, arg, ns_, Y, vec6, xprev, pss, dW, lddw, dw_off=0, defer=True, leaf=None):
        rec.append(["dw_job", [R, N, K, ldx, ns_, lddw, dw_off],
                    "".join("01"[t is not None] for t in (G, dP, arg, Y, vec6, xprev, pss, dW)), bool(defer), leaf is None])
        return orig_job(R, N, K, ldx, G, dP, arg, ns_, Y, vec6, xprev, pss, dW, lddw, dw_off=dw_off, defer=defer, leaf=leaf)
    _settle_form()
    try:
        _ffi.call, ops.dw_job = spy, job
        out = ops.shared_mlp_pool(x, ns, ls, training, geo=geo)
        if out.grad_fn is not None:
            rec.append(["saved", [[list(t.shape), str(t.dtype).replace("torch.", "")] for t in out.grad_fn.saved_tensors]])
        if training:
            # (on this thread: the form is kept per thread, and what an earlier test left on the autograd engine's
            # device thread must not show after a call that sets none)
            with torch.autograd.set_multithreading_enabled(False):
                out.backward(go)
            rec.append(["grads", [None if t.grad is None else list(t.grad.shape) for t in leaves]])
    finally:
        _ffi.call, ops.dw_job = orig_call, orig_job
    return rec


def _record(kind, c):
    """{"<case> <setting>": trace | "= default"} for every setting."""
    from demf_amd import ops
    cid, got = _case_id(kind, c), {}
    for label, attrs, dtype in (SETTINGS[:1] if kind == "eval" else SETTINGS):
        prev = {k: getattr(ops, k) for k in attrs}       # (AttributeError: the switch moved - the A/B would be void)
        try:
            for k, v in attrs.items():
                setattr(ops, k, v)
            ops.set_compute_dtype(dtype)
            t = json.loads(json.dumps(_trace(kind, c)))
        finally:
            for k, v in prev.items():
                setattr(ops, k, v)
            ops.set_compute_dtype("f32")
            ops.reset_accumulators()
        got[cid + " " + label] = "= default" if label != "default" and t == got[cid + " default"] else t
    return got


def _dump(table):
    """Compact: one line per call, nothing indented."""
    parts = []
    for key, t in table.items():
        if isinstance(t, str):
            parts.append(json.dumps(key) + ":" + json.dumps(t))
        else:
            parts.append(json.dumps(key) + ":[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in t) + "\n]")
    return "{\n" + ",\n".join(parts) + "\n}\n"


@pytest.mark.parametrize("kind,c", CASES, ids=[_case_id(k, c) for k, c in CASES])
def test_launches_match_the_recorded_trace(kind, c):
    got = _record(kind, c)
    path = os.environ.get("DEMF_RECORD_TRACE")
    if path:
        table = json.load(open(path)) if os.path.exists(path) else {}
        table.update(got)
        with open(path, "w") as f:
            f.write(_dump(table))
        return
    want = json.load(open(JSON_PATH))
    for key, t in got.items():
        assert key in want, key
        if t != want[key]:
            default = key.split(" ")[0] + " default"          # (a case id holds no blank)
            now = t if isinstance(t, list) else got[default]
            exp = want[key] if isinstance(want[key], list) else want[default]
            diff = [(i, a, b) for i, (a, b) in enumerate(zip(now, exp)) if a != b][:4]
            pytest.fail("%s: %d lines now (equal to the default's: %s), %d recorded (equal to the default's: %s); first "
                        "differences (line, now, recorded): %s"
                        % (key, len(now), isinstance(t, str), len(exp), isinstance(want[key], str), diff))


def test_the_recorded_file_has_no_stale_entries():
    keys = {_case_id(k, c) + " " + s[0] for k, c in CASES for s in (SETTINGS[:1] if k == "eval" else SETTINGS)}
    assert set(json.load(open(JSON_PATH))) == keys
