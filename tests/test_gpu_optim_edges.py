"""The kernels of csrc/optim.hip, launched directly through _ffi.call, against the float64 restatement of
tests/optim_reference.py at launch edges: the float4 body and the scalar tail, more than one workgroup, the
per-segment workgroup caps (1024 for demf_adamw_state_f32, 2048 for demf_adamw_f32 / demf_zero_f32, 1024 x 2048
elements for demf_sumsq_f32) with the grid-stride second pass behind them, segment starts and base pointers off
16 bytes, and every value of the 64-byte device state.

AdamW: one step at a time, the reference started from the fp32 state the launch itself started from, pass rule
|got - ref64| <= C * 2^-24 * S + 2^-126 per element of p', m', v' (constants and their measurement:
tests/optim_cases.py).  Sums of squares: relative bound (k + 2) * 2^-24 with k the fp32 additions of one thread,
from the launch geometry.  Copies and fills: bit-exact, between sentinel guard bands.  Every AdamW check prints its
worst ratios before asserting."""
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_reference as ref

pytestmark = pytest.mark.gpu

MAX_NORM = 10.0
LRS = (0.008, 0.0004, 0.002, 0.016)
WDS = (0.01, 0.02, 0.0, 0.05)
PAD = 0xA5
KEYS = ("p", "g", "m", "v")


def _call(name, *args):
    from demf_amd import _ffi
    _ffi.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(host, off):
    """``host`` on the device at ``off`` floats behind an allocation's (256-byte aligned) base."""
    base = torch.empty(off + host.size, dtype=torch.float32, device="cuda")
    view = base[off:]
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 4 * (off % 4)
    return view


# ---- the 64-byte device state -----------------------------------------------------------------------------------
def _state(sumsq=0.0, t=0, lr_factor=1.0, ticket=0):
    b = np.full(64, PAD, np.uint8)
    b[0:8] = np.array([sumsq], np.float64).view(np.uint8)
    b[8:16] = np.array([t], np.int64).view(np.uint8)
    b[16:20] = np.array([ticket], np.uint32).view(np.uint8)
    b[20:24] = np.array([lr_factor], np.float32).view(np.uint8)
    return _dev(b), b


def _read_state(dev):
    b = dev.cpu().numpy()
    return dict(sumsq_bits=int(b[0:8].view(np.uint64)[0]), sumsq=float(b[0:8].view(np.float64)[0]),
                t=int(b[8:16].view(np.int64)[0]), ticket=int(b[16:20].view(np.uint32)[0]), rest=bytes(b[20:]))


def _assert_state_advanced(dev, before_bytes, t0, label):
    s = _read_state(dev)
    assert s["t"] == t0 + 1, (label, s["t"], t0)
    assert s["sumsq_bits"] == 0, (label, s["sumsq"])                     # the bits of +0.0
    assert s["ticket"] == 0, (label, s["ticket"])
    assert s["rest"] == bytes(before_bytes[20:]), label                  # lr_factor and the pad


# ---- demf_adamw_state_f32 ---------------------------------------------------------------------------------------
def _segments(sizes, layout):
    """[(start, n, lr, weight_decay)], total length.  contiguous: back to back from 0; aligned4: every start
    rounded up to a multiple of 4; gapped: odd gaps in front of and between the segments, a pad behind the last."""
    gaps = {"contiguous": (0, 0, 0, 0, 0), "aligned4": None, "gapped": (2, 3, 7, 1, 9)}[layout]
    segs, pos = [], 0
    for i, n in enumerate(sizes):
        pos = -(-pos // 4) * 4 if gaps is None else pos + gaps[i]
        segs.append((pos, n, LRS[i], WDS[i]))
        pos += n
    return segs, pos + (5 if gaps is None else gaps[4])


def _fill(segs, total, seed, fresh=False, zero_grad=False):
    """Host p, g, m, v of ``total`` floats: generator inputs inside the segments, sentinels everywhere else."""
    host = {k: np.full(total, oc.SENTINEL, np.float32) for k in KEYS}
    for i, (start, n, _, _) in enumerate(segs):
        for k, x in zip(KEYS, oc.adamw_inputs(n, seed + 101 * i, fresh=fresh)):
            host[k][start:start + n] = x
        if zero_grad:
            host["g"][start:start + n] = 0.0
    return host


def _true_sumsq(segs, host):
    return float(sum((host["g"][s:s + n].astype(np.float64) ** 2).sum() for s, n, _, _ in segs))


def _launch_state(segs, bufs, state, max_norm, grad_scale, nseg=None):
    n = len(segs)
    arr = ((ctypes.c_longlong * n)(*[s[0] for s in segs]), (ctypes.c_longlong * n)(*[s[1] for s in segs]),
           (ctypes.c_float * n)(*[s[2] for s in segs]), (ctypes.c_float * n)(*[s[3] for s in segs]))
    a = [ctypes.cast(x, ctypes.c_void_p) for x in arr]
    _call("demf_adamw_state_f32", n if nseg is None else nseg, a[0], a[1], a[2], a[3], bufs["p"].data_ptr(),
          bufs["g"].data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), state.data_ptr(), float(max_norm),
          float(grad_scale), float(oc.BETA1), float(oc.BETA2), float(oc.EPS))


def _check_step(label, segs, before, after, sumsq, t_step, lr_factor, max_norm, grad_scale):
    """``after`` against one reference step from ``before`` per segment; everything outside the segments, and
    the whole gradient buffer, bit-identical."""
    total = before["p"].size
    inside = np.zeros(total, bool)
    worst = [0.0, 0.0, 0.0]
    for start, n, lr, wd in segs:
        sl = slice(start, start + n)
        inside[sl] = True
        r = oc.step_ratios(tuple(after[k][sl] for k in "pmv"), tuple(before[k][sl] for k in KEYS), sumsq=sumsq,
                           t=t_step, lr=lr, lr_factor=lr_factor, weight_decay=wd, max_norm=max_norm,
                           grad_scale=grad_scale)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("optim-edges %-34s ratio p %.2f m %.2f v %.2f" % (label, *worst))
    assert np.array_equal(_bits(after["g"]), _bits(before["g"])), label + ": grad was written"
    for k in "pmv":
        assert np.array_equal(_bits(after[k])[~inside], _bits(before[k])[~inside]), label + ": %s outside" % k
    msg = "%s: worst ratio p %.2f (C %g) m %.2f (C %g) v %.2f (C %g)" % (label, worst[0], oc.C_P, worst[1], oc.C_M,
                                                                     worst[2], oc.C_V)
    assert worst[0] <= oc.C_P and worst[1] <= oc.C_M and worst[2] <= oc.C_V, msg
    return worst


def _run_state(label, segs, total, seed, t0=9, lr_factor=1.0, grad_scale=1.0, max_norm=MAX_NORM, sumsq="true",
               offs=(0, 0, 0, 0), zero_grad=False):
    host = _fill(segs, total, seed, fresh=(t0 == 0), zero_grad=zero_grad)
    if sumsq == "true":
        sumsq = _true_sumsq(segs, host)
    bufs = {k: _place(host[k], o) for k, o in zip(KEYS, offs)}
    state, sbytes = _state(sumsq, t0, lr_factor)
    _launch_state(segs, bufs, state, max_norm, grad_scale)
    torch.cuda.synchronize()
    after = {k: bufs[k].cpu().numpy() for k in KEYS}
    _assert_state_advanced(state, sbytes, t0, label)
    return _check_step(label, segs, host, after, sumsq, t0 + 1, lr_factor, max_norm, grad_scale)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 1_048_576, 1_048_577, 1_049_603])
def test_state_adamw_one_segment(n):
    """The tail alone, one float4, a float4 plus a tail, around one workgroup's 1024 elements, the 1024-workgroup
    cap (1 048 576), the cap plus one element (a second grid-stride pass that is a scalar tail), and a second pass
    of 256 float4s with a 3-element tail."""
    _run_state("one_segment_%d" % n, [(0, n, LRS[0], WDS[0])], n, seed=n)


@pytest.mark.parametrize("nseg", [1, 2, 3, 4])
@pytest.mark.parametrize("layout", ["contiguous", "aligned4", "gapped"])
def test_state_adamw_segment_layouts(layout, nseg):
    """Segments of 5, 1024, 1025 and 3 elements (1, 1, 2, 1 workgroups: every block0 is a lookup boundary) with
    their own lr and weight decay; gap and pad elements of p, m, v keep their sentinel bits."""
    segs, total = _segments((5, 1024, 1025, 3)[:nseg], layout)
    if layout == "contiguous" and nseg > 2:
        assert any(s[0] % 4 for s in segs)
    if layout == "aligned4":
        assert all(s[0] % 4 == 0 for s in segs)
    if layout == "gapped":
        assert segs[0][0] > 0 and total > segs[-1][0] + segs[-1][1]
    _run_state("%s_%d" % (layout, nseg), segs, total, seed=10 * nseg)


def test_state_adamw_production_pair():
    """The two parameter groups of the full model, contiguous: group 0 is past the 1024-workgroup cap (second pass,
    scalar tail), group 1 starts off 16 bytes (the whole group on the scalar branch)."""
    from demf_amd.config import DeMFCfg
    from demf_amd.modules import DeMFHotPath
    groups = DeMFHotPath(DeMFCfg()).param_groups(lr=0.008, weight_decay=0.01)
    sizes = [sum(p.numel() for p in g["params"] if p.requires_grad) for g in groups]
    assert len(sizes) == 2
    n0, start1 = sizes[0], sizes[0]
    assert n0 > 1_048_576, "group 0 no longer needs the grid-stride second pass: this case lost its point"
    assert start1 % 4 != 0, "group 1 no longer starts off 16 bytes: this case lost its point"
    segs = [(0, sizes[0], groups[0]["lr"], groups[0]["weight_decay"]),
            (start1, sizes[1], groups[1]["lr"], groups[1]["weight_decay"])]
    _run_state("production_%d_%d" % tuple(sizes), segs, sum(sizes), seed=77)


@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (0, 1, 0, 0), (1, 1, 1, 1)], ids=["aligned", "grad_offset", "all_offset"])
def test_state_adamw_base_alignment(offs):
    """Base pointers of p, g, m, v at +0 / +1 float: all aligned (float4 body), the gradient alone offset and all
    four offset (scalar branch for everything)."""
    segs, total = _segments((1029, 515), "contiguous")
    _run_state("base_%d%d%d%d" % offs, segs, total, seed=5, offs=offs)


@pytest.mark.parametrize("grad_scale", oc.GRAD_SCALES)
@pytest.mark.parametrize("lr_factor", oc.LR_FACTORS)
@pytest.mark.parametrize("t0", oc.T_VALUES)
def test_state_adamw_device_values(t0, lr_factor, grad_scale):
    """Step count, lr factor and grad scale as the device block holds them, two workgroups with a tail, clipped by
    the gradients' own norm."""
    _run_state("t%d_f%g_s%g" % (t0, lr_factor, grad_scale), [(0, 1029, LRS[0], WDS[0])], 1029, seed=t0 % 1000 + 3,
               t0=t0, lr_factor=lr_factor, grad_scale=grad_scale)


@pytest.mark.parametrize("case", ["below", "above", "zero", "inf", "nan", "max_norm_0_stale"])
def test_state_adamw_norm_cases(case):
    """The clip coefficient from the state's sumsq: below the threshold (1), above it, exactly 0 with all-zero
    gradients, inf (coefficient 0) and NaN (not clipped: `c < 1` is false) as optim_reference states the rule;
    max_norm = 0 ignores a stale sumsq and still clears it."""
    segs, total = _segments((1029, 7), "contiguous")
    kw = dict(below=dict(sumsq=4.0), above=dict(sumsq="true"), zero=dict(sumsq=0.0, zero_grad=True),
              inf=dict(sumsq=float("inf")), nan=dict(sumsq=float("nan")),
              max_norm_0_stale=dict(sumsq=1e12, max_norm=0.0))[case]
    want = dict(below=0.5, zero=0.5, inf=0.0, nan=0.5, max_norm_0_stale=0.5)
    if case == "above":
        host = _fill(segs, total, 21)
        assert ref.clip_coef(_true_sumsq(segs, host), 0.5, MAX_NORM) < 0.5 * 0.1
    else:
        assert ref.clip_coef(kw["sumsq"], 0.5, kw.get("max_norm", MAX_NORM)) == want[case]
    _run_state("norm_" + case, segs, total, seed=21, grad_scale=0.5, **kw)


@pytest.mark.parametrize("sizes", [(5,), (1_048_577, 5)], ids=["one_workgroup", "1025_workgroups"])
def test_state_adamw_back_to_back(sizes):
    """Two launches with no host write to the state in between: the last workgroup's ticket reset, the step count
    and the cleared sumsq are what the second launch starts from."""
    segs, total = _segments(sizes, "contiguous")
    host = _fill(segs, total, 31)
    sumsq = _true_sumsq(segs, host)
    bufs = {k: _place(host[k], 0) for k in KEYS}
    state, sbytes = _state(sumsq, 9, 0.1)
    _launch_state(segs, bufs, state, MAX_NORM, 1.0)
    mid_dev = {k: bufs[k].clone() for k in KEYS}
    mid_state = state.clone()
    _launch_state(segs, bufs, state, MAX_NORM, 1.0)
    torch.cuda.synchronize()
    mid = {k: mid_dev[k].cpu().numpy() for k in KEYS}
    after = {k: bufs[k].cpu().numpy() for k in KEYS}
    _assert_state_advanced(mid_state, sbytes, 9, "first")
    _assert_state_advanced(state, sbytes, 10, "second")
    _check_step("back_to_back_1_%s" % (sizes,), segs, host, mid, sumsq, 10, 0.1, MAX_NORM, 1.0)
    _check_step("back_to_back_2_%s" % (sizes,), segs, mid, after, 0.0, 11, 0.1, MAX_NORM, 1.0)   # sumsq was cleared


@pytest.mark.parametrize("case", ["nseg0", "nseg5", "empty_segment"])
def test_state_adamw_rejects(case):
    sizes = {"nseg0": (5, 4, 3, 2, 1), "nseg5": (5, 4, 3, 2, 1), "empty_segment": (5, 0, 3)}[case]
    segs, pos = [], 0
    for n in sizes:
        segs.append((pos, n, 0.008, 0.01))
        pos += n
    host = {k: oc.adamw_inputs(pos, 1)[i] for i, k in enumerate(KEYS)}
    bufs = {k: _place(host[k], 0) for k in KEYS}
    state, sbytes = _state(123.0, 4, 0.1)
    with pytest.raises(RuntimeError, match="adamw_state"):
        _launch_state(segs, bufs, state, MAX_NORM, 1.0, nseg={"nseg0": 0, "nseg5": 5}.get(case))
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy(), sbytes)
    for k in KEYS:
        assert np.array_equal(_bits(bufs[k].cpu().numpy()), _bits(host[k])), k


# ---- demf_adamw_f32 ---------------------------------------------------------------------------------------------
def _run_flat(n, norm_mode, step, off, seed):
    x = oc.adamw_inputs(n, seed, fresh=(step == 1))
    host = dict(zip(KEYS, x))
    guard = 4
    bufs, full = {}, {}
    for k in KEYS:                                   # sentinel bands in front of and behind every buffer
        full[k] = np.full(guard + n + guard, oc.SENTINEL, np.float32)
        full[k][guard:guard + n] = host[k]
        bufs[k] = _place(full[k], off)
    grad_scale, max_norm = 0.5, MAX_NORM
    if norm_mode == "null":
        norm_dev, coef = None, ref.w32(grad_scale)
    else:
        # the norm is over ALL groups, not this buffer's own: any device scalar; 345.5 * 0.5 clips, 3 * 0.5 does not
        norm32 = np.float32(345.5 if norm_mode == "clipped" else 3.0)
        norm_dev = _dev(np.array([norm32], np.float32))
        coef = ref.clip_coef(np.float64(norm32) ** 2, grad_scale, max_norm)
        assert (coef < grad_scale) == (norm_mode == "clipped")
    ptr = lambda k: bufs[k].data_ptr() + 4 * guard
    _call("demf_adamw_f32", n, ptr("p"), ptr("g"), ptr("m"), ptr("v"), None if norm_dev is None else norm_dev.data_ptr(),
          float(max_norm), grad_scale, LRS[0], float(oc.BETA1), float(oc.BETA2), float(oc.EPS), WDS[0], step)
    torch.cuda.synchronize()
    after = {k: bufs[k].cpu().numpy() for k in KEYS}
    label = "flat_%d_%s_step%d_off%d" % (n, norm_mode, step, off)
    return _check_flat(label, guard, n, full, after, coef, step)


def _check_flat(label, guard, n, before, after, coef, step):
    sl = slice(guard, guard + n)
    r = oc.step_ratios(tuple(after[k][sl] for k in "pmv"), tuple(before[k][sl] for k in KEYS), sumsq=None, t=step,
                       lr=LRS[0], lr_factor=1.0, weight_decay=WDS[0], max_norm=None, grad_scale=None, coef=coef)
    print("optim-edges %-34s ratio p %.2f m %.2f v %.2f" % (label, *r))
    assert np.array_equal(_bits(after["g"]), _bits(before["g"])), label
    for k in "pmv":
        for band in (slice(0, guard), slice(guard + n, None)):
            assert np.array_equal(_bits(after[k][band]), _bits(before[k][band])), label + ": %s guard" % k
    assert r[0] <= oc.C_P and r[1] <= oc.C_M and r[2] <= oc.C_V, \
        "%s: worst ratio p %.2f (C %g) m %.2f (C %g) v %.2f (C %g)" % (label, r[0], oc.C_P, r[1], oc.C_M, r[2], oc.C_V)
    return r


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_flat_adamw_small(n):
    """The per-group entry point with the step passed by the host: no norm (grad_scale alone), a device norm that
    clips and one that does not, steps 1 and 10, base pointers aligned and at +1 float."""
    for norm_mode in ("null", "clipped", "unclipped"):
        for step in (1, 10):
            for off in (0, 1):
                _run_flat(n, norm_mode, step, off, seed=n + step)


@pytest.mark.parametrize("norm_mode,step,off", [("null", 1, 0), ("clipped", 10, 0), ("unclipped", 10, 1)])
def test_flat_adamw_past_the_workgroup_cap(norm_mode, step, off):
    """2 098 179 elements: 2048 workgroups x 1024 elements, then a second grid-stride pass of 256 float4s and a
    3-element tail."""
    _run_flat(2_098_179, norm_mode, step, off, seed=9)


# ---- sums of squares --------------------------------------------------------------------------------------------
SUMSQ_N = (1, 255, 2048, 2049, 2_097_929)
S0 = 3.25


def _sumsq_bound(ref_sum, k, fp64_adds, total):
    """(k + 2) * 2^-24 relative for one thread's k fp32 additions (the squares' own roundings included), plus the
    fp64 part: the wave and workgroup sums and one atomic per workgroup, each within 2^-53 of the running total."""
    return (k + 2) * 2.0 ** -24 * ref_sum + (fp64_adds + 16) * 2.0 ** -53 * total


def _k_sumsq_f32(n):
    blocks = min(1024, -(-n // 2048))
    return -(-n // (blocks * 256)), blocks


def _k_multi_copy(words, vec, bps):
    threads = bps * 256
    if vec:
        return 4 * -(-(words // 4) // threads) + (1 if words % 4 else 0)
    return -(-words // threads)


def _sumsq_input(n, seed):
    return oc.adamw_inputs(n, seed)[1] if n > 1 else np.array([-3.7], np.float32)


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_f32_added_onto_the_state(n):
    x = _sumsq_input(n, n)
    want = float((x.astype(np.float64) ** 2).sum())
    k, blocks = _k_sumsq_f32(n)
    if n == SUMSQ_N[-1]:
        assert blocks == 1024 and k == 9                # past 1024 x 2048: a second pass for some threads
    state, sbytes = _state(S0, 7, 0.1)
    src = _dev(x)
    _call("demf_sumsq_f32", n, src.data_ptr(), state.data_ptr())
    torch.cuda.synchronize()
    s = _read_state(state)
    err, bound = abs(s["sumsq"] - (S0 + want)), _sumsq_bound(want, k, blocks, S0 + want)
    print("sumsq_f32 n %d k %d: err %.3e bound %.3e" % (n, k, err, bound))
    assert err <= bound, (n, s["sumsq"], S0 + want, err, bound)
    assert state.cpu().numpy()[8:].tobytes() == sbytes[8:].tobytes()          # t, ticket, lr_factor, pad


@pytest.mark.parametrize("off", [0, 1], ids=["vector", "scalar"])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_multi_copy_sumsq_added_onto_the_state(n, off):
    x = _sumsq_input(n, n + 1)
    want = float((x.astype(np.float64) ** 2).sum())
    bps = 64 if n > 4096 else 4
    k = _k_multi_copy(n, off == 0, bps)
    src = _place(x, off)
    dst = _place(np.full(n, oc.SENTINEL, np.float32), 0)
    table = _dev(np.array([[src.data_ptr()], [dst.data_ptr()], [n]], np.int64))
    state, sbytes = _state(S0, 7, 0.1)
    _call("demf_multi_copy_sumsq", 1, table.data_ptr(), bps, state.data_ptr())
    torch.cuda.synchronize()
    s = _read_state(state)
    err, bound = abs(s["sumsq"] - (S0 + want)), _sumsq_bound(want, k, bps, S0 + want)
    print("multi_copy_sumsq n %d off %d k %d: err %.3e bound %.3e" % (n, off, k, err, bound))
    assert err <= bound, (n, s["sumsq"], S0 + want, err, bound)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(x))
    assert state.cpu().numpy()[8:].tobytes() == sbytes[8:].tobytes()


@pytest.mark.parametrize("entry", ["sumsq_f32", "multi_copy_sumsq"])
def test_sumsq_zero_and_non_finite_input(entry):
    """All-zero input leaves the state's sumsq bits as they are; one inf or NaN element makes it non-finite."""
    n = 2049
    for special in (0.0, float("inf"), float("nan")):
        x = np.zeros(n, np.float32) if special == 0.0 else oc.adamw_inputs(n, 3)[1]
        if special != 0.0:
            x[1500] = special
        src = _dev(x)
        state, sbytes = _state(S0, 7, 0.1)
        if entry == "sumsq_f32":
            _call("demf_sumsq_f32", n, src.data_ptr(), state.data_ptr())
        else:
            dst = _place(np.full(n, oc.SENTINEL, np.float32), 0)
            table = _dev(np.array([[src.data_ptr()], [dst.data_ptr()], [n]], np.int64))
            _call("demf_multi_copy_sumsq", 1, table.data_ptr(), 4, state.data_ptr())
        torch.cuda.synchronize()
        got = state.cpu().numpy()
        if special == 0.0:
            assert got.tobytes() == sbytes.tobytes()
        else:
            s = _read_state(state)
            assert (np.isinf(s["sumsq"]) and s["sumsq"] > 0) if np.isinf(special) else np.isnan(s["sumsq"]), s["sumsq"]
            assert got[8:].tobytes() == sbytes[8:].tobytes()


# ---- demf_multi_copy / demf_multi_copy_sumsq, bit-exact ---------------------------------------------------------
GUARD = 8
COPY_WORDS = (0, 1, 3, 4, 5, 1023, 1025, 262_147)


def _spans(words, offs):
    """Start of each piece in one buffer: GUARD sentinel floats, then ``off`` floats behind a 16-byte boundary."""
    starts, pos = [], 0
    for w, o in zip(words, offs):
        s = pos + GUARD + o
        starts.append(s)
        pos = -(-(s + w) // 4) * 4
    return starts, pos + GUARD


def _copy_data(n, seed, as_float):
    rng = np.random.default_rng(seed)
    if not as_float:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)   # NaN patterns too
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    x[::13] = -0.0
    x[5::17] = np.float32(1e-40)                       # denormal: copied bit for bit, its square is 0
    return x


def _run_copy(entry, specs, bps, seed):
    """specs: (words, src_off or None for a null source, dst_off).  One launch over the whole table; the
    destination buffer, guard bands included, against the expected bits; returns the state's sumsq gain check."""
    with_sum = entry == "demf_multi_copy_sumsq"
    words = [s[0] for s in specs]
    sstart, slen = _spans(words, [s[1] or 0 for s in specs])
    dstart, dlen = _spans(words, [s[2] for s in specs])
    src = _copy_data(slen, seed, with_sum)
    dst = np.full(dlen, oc.SENTINEL, np.float32)
    want = dst.copy()
    ref_sum = bound = 0.0
    for (w, so, do), ss, ds in zip(specs, sstart, dstart):
        piece = src[ss:ss + w]
        want[ds:ds + w] = 0.0 if so is None else piece
        if with_sum and so is not None:
            s = float((piece.astype(np.float64) ** 2).sum())
            ref_sum += s
            bound += (_k_multi_copy(w, so % 4 == 0 and do % 4 == 0, bps) + 2) * 2.0 ** -24 * s
    dsrc, ddst = _place(src, 0), _place(dst, 0)
    table = np.array([[0 if so is None else dsrc.data_ptr() + 4 * ss for (_, so, _), ss in zip(specs, sstart)],
                      [ddst.data_ptr() + 4 * ds for ds in dstart], words], np.int64)
    dtable = _dev(table)
    for (w, so, do), a_s, a_d in zip(specs, table[0], table[1]):
        assert a_d % 16 == 4 * do and (so is None or a_s % 16 == 4 * so)
    if with_sum:
        state, sbytes = _state(S0, 7, 0.1)
        _call(entry, len(specs), dtable.data_ptr(), bps, state.data_ptr())
    else:
        _call(entry, len(specs), dtable.data_ptr(), bps)
    torch.cuda.synchronize()
    got = ddst.cpu().numpy()
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (entry, bps, "first wrong word %d of %d, %d wrong" % (bad[0], dlen, bad.size))
    assert np.array_equal(_bits(dsrc.cpu().numpy()), _bits(src))
    if with_sum:
        s = _read_state(state)
        if ref_sum == 0.0:
            assert state.cpu().numpy().tobytes() == sbytes.tobytes()          # null sources add nothing
        else:
            err = abs(s["sumsq"] - (S0 + ref_sum))
            bound += (len(specs) * bps + 16) * 2.0 ** -53 * (S0 + ref_sum)
            print("%s %d pieces bps %d: sumsq err %.3e bound %.3e" % (entry, len(specs), bps, err, bound))
            assert err <= bound, (s["sumsq"], S0 + ref_sum, err, bound)
        assert state.cpu().numpy()[8:].tobytes() == sbytes[8:].tobytes()


@pytest.mark.parametrize("bps", [1, 4, 64])
@pytest.mark.parametrize("entry", ["demf_multi_copy", "demf_multi_copy_sumsq"])
def test_multi_copy_offsets_and_sizes(entry, bps):
    """Every size x source offset x destination offset (0-3 floats each) as the 128 pieces of one table: the
    float4 body with its 4q tail where both sit on 16 bytes, the scalar loop everywhere else."""
    specs = [(w, so, do) for w in COPY_WORDS for so in range(4) for do in range(4)]
    if bps != 64:                                       # the 1 MB pieces once per entry point, at their production width
        specs = [s for s in specs if s[0] != COPY_WORDS[-1]]
    _run_copy(entry, specs, bps, seed=bps)


@pytest.mark.parametrize("nseg", [1, 2, 119])
@pytest.mark.parametrize("entry", ["demf_multi_copy", "demf_multi_copy_sumsq"])
def test_multi_copy_segment_counts_and_null_sources(entry, nseg):
    """1, 2 and 119 pieces (the full model's parameter count) in one table; every third piece of the long table
    and the second of the pair has a null source: zero-filled, nothing added to sumsq."""
    rng = np.random.default_rng(nseg)
    specs = []
    for i in range(nseg):
        w = int(rng.choice(COPY_WORDS[1:-1]))
        null = (nseg == 2 and i == 1) or (nseg == 119 and i % 3 == 2)
        specs.append((w, None if null else int(rng.integers(0, 4)) * (i % 2), int(rng.integers(0, 4)) * (i % 2)))
    _run_copy(entry, specs, 4, seed=100 + nseg)


def test_multi_copy_only_null_sources():
    for entry in ("demf_multi_copy", "demf_multi_copy_sumsq"):
        _run_copy(entry, [(1025, None, 0), (5, None, 3), (4, None, 1)], 4, seed=1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
def test_multi_copy_class_counts_words_of_64_bit_types(dtype):
    """ops.MultiCopy on 8-byte elements: 2 words each; a piece at +8 bytes takes the scalar loop, one on 16 bytes
    the float4 body with a 2-word tail (1025 elements = 2050 words)."""
    from demf_amd import ops
    g = torch.Generator().manual_seed(2)
    sent = -7777
    dsts, srcs, wants, bases = [], [], [], []
    for n, off, null in ((1025, 0, False), (1025, 1, False), (3, 1, False), (7, 0, True)):
        base = torch.full((GUARD + off + n + GUARD,), sent, dtype=dtype, device="cuda")
        s = None if null else torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g).to(dtype).cuda()
        want = base.clone()
        want[GUARD + off:GUARD + off + n] = 0 if null else s
        bases.append(base), dsts.append(base[GUARD + off:GUARD + off + n]), srcs.append(s), wants.append(want)
        assert dsts[-1].data_ptr() % 16 == 8 * off
    mc = ops.MultiCopy(dsts, srcs)
    assert mc.table.cpu()[2].tolist() == [2050, 2050, 6, 14]
    mc()
    torch.cuda.synchronize()
    for base, want in zip(bases, wants):
        assert torch.equal(base, want)


# ---- demf_zero_f32 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 2_097_157, 4_194_304])
def test_zero_f32(n, off):
    """2 097 157: past 2048 workgroups x 256 float4s, a second pass and a 1-element tail; 4 194 304: the step
    arena's size.  Base on 16 bytes (float4 body) and at +1 float (scalar loop); the bands on both sides stay."""
    host = np.full(GUARD + off + n + GUARD, oc.SENTINEL, np.float32)
    host[GUARD + off:GUARD + off + n] = oc.adamw_inputs(min(n, 4096), 1)[0][np.arange(n) % min(n, 4096)] + 1.5
    buf = _place(host, 0)
    _call("demf_zero_f32", n, buf.data_ptr() + 4 * (GUARD + off))
    torch.cuda.synchronize()
    want = host.copy()
    want[GUARD + off:GUARD + off + n] = 0.0
    got = buf.cpu().numpy()
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, "first wrong word %d (piece %d..%d), %d wrong" % (bad[0], GUARD + off, GUARD + off + n, bad.size)
