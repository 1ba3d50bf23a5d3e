"""Three three-layer ops.shared_mlp_pool forwards ("f32" mode) at the smallest shapes whose MIDDLE layer reaches the three
special forward forms of csrc/mlp.hip launch_gemm_t - weight-resident (K = N = 64, R >= 16 384), producer / consumer
(K = 128, R >= 16 384) and the few-row tile kernel (R <= 16 384) - printed as one JSON line: the form that layer's
launch took (demf_mlp_last_form), each output's shape and whether it is finite.  tests/test_gpu_switch_arrives.py runs
this in one process with the defaults and in one with DEMF_FWD_RES / DEMF_FWD_PC / DEMF_FWD_TILE = 0."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from demf_amd import _ffi, ops

CASES = [(64, 16384, 16), (128, 16384, 16), (64, 2048, 16)]      # (channels of every layer, rows, ns)

ops.set_compute_dtype("f32")
lib, orig = _ffi.load(), _ffi.call
forms, shapes, finite = [], [], True
for C, R, ns in CASES:
    g = torch.Generator().manual_seed(C + R)
    x = (torch.randn(R, C, generator=g) * 0.7 + 0.1).cuda()
    layers = [((torch.randn(C, C, generator=g) / C ** 0.5).cuda(), torch.ones(C, device="cuda"),
               torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")) for _ in range(3)]
    fwd = []

    def spy(name, *a):
        rc = orig(name, *a)
        if name.startswith("demf_mlp_gemm_fwd"):
            fwd.append(lib.demf_mlp_last_form())
        return rc
    _ffi.call = spy
    try:
        with torch.no_grad():
            out = ops.shared_mlp_pool(x, ns, layers, True)
    finally:
        _ffi.call = orig
    torch.cuda.synchronize()
    assert len(fwd) == 3, fwd           # one forward launch per layer
    forms.append(fwd[1])
    shapes.append(list(out.shape))
    finite = finite and bool(torch.isfinite(out).all())
print(json.dumps(dict(forms=forms, shapes=shapes, finite=finite)))
