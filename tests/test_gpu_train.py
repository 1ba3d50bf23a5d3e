"""The step meter (csrc/meter.hip, demf_amd/meter.py), metered training steps (engine.Trainer.attach_meter) and the
training runner (demf_amd/train.py) on the GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------
def _state(sumsq, t, lr_factor):
    """The optimizer's 64-byte device state, built by hand: { double sumsq; int64 t; uint32 ticket; float lr_factor }."""
    st = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st.view(torch.float64)[0] = sumsq
    st.view(torch.int64)[1] = t
    st.view(torch.float32)[5] = lr_factor
    return st


def _ring(rows, guard=2):
    """A ring whose every word but the stamps is a canary, inside a larger canary buffer."""
    from demf_amd import meter
    big = torch.full((rows + 2 * guard, 16), CANARY, dtype=torch.int32, device="cuda")
    ring = big[guard:guard + rows]
    host = meter.empty_ring(rows)
    host[:, 2:] = CANARY
    ring.copy_(torch.from_numpy(host))
    return big, ring


def _scalars(n, values):
    """n single-float device tensors: up to eight views at offsets 0..7 of ONE 8-vector (as the loss terms are views of
    loss_total's output), the rest tensors of their own."""
    vec = torch.tensor(values[:8] + [0.0] * max(0, 8 - n), dtype=torch.float32, device="cuda")
    out = [vec[i] for i in range(min(n, 8))]
    out += [torch.tensor(v, dtype=torch.float32, device="cuda") for v in values[8:n]]
    if n == 1:                                              # a view at a NONZERO offset on its own
        out = [vec[5]]
        vec[5] = values[0]
    assert all(s.numel() == 1 for s in out)
    return vec, out


def _host_norm_clip(sumsq, grad_scale, max_norm):
    """The expressions of adamw_state_k on the host, in fp32 where the kernel is."""
    norm = np.float32(np.sqrt(np.float64(sumsq)))
    gs = np.float32(grad_scale)
    clip = np.float32(1.0)
    if max_norm > 0:
        c = np.float32(max_norm) / (norm * gs + np.float32(1e-6))
        clip = c if c < 1 else np.float32(1.0)
    return norm * gs, clip


def _within_one_ulp(got, want):
    got, want = np.float32(got), np.float32(want)
    return abs(np.float64(got) - np.float64(want)) <= np.spacing(abs(want))


@pytest.mark.parametrize("n", [1, 8, 10])
@pytest.mark.parametrize("sumsq,grad_scale,max_norm", [(1234.5678, 1.0, 10.0), (4.0, 0.5, 10.0), (3.7e-5, 1.0, 0.0),
                                                      (9.87654321e9, 0.125, 35.0)])
def test_kernel_row_contents(n, sumsq, grad_scale, max_norm):
    from demf_amd import meter, ops
    names = [f"s{i}" for i in range(n)]
    values = [float(np.float32(0.1 * (i + 1) ** 2 - 0.7)) for i in range(n)]
    vec, scalars = _scalars(n, values)
    if n > 1:
        assert scalars[3].data_ptr() == vec.data_ptr() + 12           # views at nonzero offsets, no copies
    lr = float(np.float32(0.1) * np.float32(0.1))
    st = _state(sumsq, 41, lr)
    before = st.clone()
    big, ring = _ring(8)
    ops.step_meter(scalars, st, grad_scale, max_norm, ring)
    torch.cuda.synchronize()
    assert torch.equal(st, before)                                    # the meter only reads the state
    host = ring.cpu().numpy()
    rows, nxt = meter.decode_ring(host, names, 41)
    assert nxt == 42 and len(rows) == 1
    r = rows[0]
    want_norm, want_clip = _host_norm_clip(sumsq, grad_scale, max_norm)
    print(f"n={n} grad_norm {r['grad_norm']!r} (host {float(want_norm)!r}) clip {r['clip']!r} (host {float(want_clip)!r})")
    assert r["t"] == 41 and r["nonfinite"] == ()
    assert np.float32(r["lr_factor"]).tobytes() == np.float32(lr).tobytes()
    for name, v in zip(names, values):
        assert np.float32(r[name]).tobytes() == np.float32(v).tobytes(), name
    assert _within_one_ulp(r["grad_norm"], want_norm)
    assert _within_one_ulp(r["clip"], want_clip)
    assert (want_clip < 1) == (max_norm > 0 and float(want_norm) > max_norm)
    # row 41 % 8 = 1: unused scalar slots are zero, every other row and the guard rows keep their canaries
    assert (host[1, 6 + n:] == 0).all()
    want = np.full((12, 16), CANARY, np.int32)
    want[2:10, :2] = -1
    got = big.cpu().numpy()
    got[2 + 1] = want[2 + 1]
    assert (got == want).all()


def test_ring_wraps_and_touches_one_row_per_step():
    from demf_amd import meter, ops
    names = ("a", "b", "c")
    big, ring = _ring(4)
    vec, scalars = _scalars(3, [0.0, 0.0, 0.0])
    st = _state(9.0, 0, 1.0)
    prev = big.cpu().numpy()
    for t in range(6):
        st.view(torch.int64)[1] = t
        vec[:3] = torch.tensor([t + 0.5, -t, 100.0 + t], device="cuda")
        ops.step_meter(scalars, st, 1.0, 10.0, ring)
        now = big.cpu().numpy()
        changed = np.nonzero((now != prev).any(1))[0].tolist()
        assert changed == [2 + t % 4], (t, changed)               # (two guard rows in front)
        prev = now
    host = ring.cpu().numpy()
    assert host[:, :2].copy().view(np.int64)[:, 0].tolist() == [4, 5, 2, 3]       # 0 and 1 overwritten by 4 and 5
    rows, nxt = meter.decode_ring(host, names, 2)
    assert [(r["t"], r["a"], r["b"], r["c"]) for r in rows] == [(t, t + 0.5, -t, 100.0 + t) for t in range(2, 6)]
    assert all(r["grad_norm"] == 3.0 and r["clip"] == 1.0 for r in rows) and nxt == 6
    with pytest.raises(RuntimeError, match="overrun"):
        meter.decode_ring(host, names, 0)
    assert (big[:2] == CANARY).all() and (big[6:] == CANARY).all()


@pytest.mark.parametrize("n", [1, 8, 10])
def test_nonfinite_values_set_exactly_their_own_bit(n):
    from demf_amd import meter, ops
    names = [f"s{i}" for i in range(n)]
    cases = [(0, float("nan")), (n // 2, float("inf")), (n - 1, float("-inf"))]
    _, ring = _ring(8)
    t = 0
    for i, bad in cases:
        values = [1.0 + k for k in range(n)]
        values[i] = bad
        _, scalars = _scalars(n, values)
        ops.step_meter(scalars, _state(4.0, t, 1.0), 1.0, 10.0, ring)
        torch.cuda.synchronize()
        host = ring.cpu().numpy()
        assert int(host[t % 8, 2:3].view(np.uint32)[0]) == 1 << i, (i, bad)
        r = meter.decode_ring(host, names, t)[0][0]
        assert r["nonfinite"] == (names[i],) and r["grad_norm"] == 2.0
        stored = [r[k] for k in names]
        assert (np.isnan(stored[i]) if np.isnan(bad) else stored[i] == bad), "the value itself is still stored"
        assert [v for k, v in enumerate(stored) if k != i] == [v for k, v in enumerate(values) if k != i]
        t += 1
    for sumsq in (float("inf"), float("nan")):
        _, scalars = _scalars(n, [1.0 + k for k in range(n)])
        ops.step_meter(scalars, _state(sumsq, t, 1.0), 1.0, 10.0, ring)
        host = ring.cpu().numpy()
        assert int(host[t % 8, 2:3].view(np.uint32)[0]) == meter.FLAG_GRAD_NORM
        r = meter.decode_ring(host, names, t)[0][0]
        assert r["nonfinite"] == ("grad_norm",) and not np.isfinite(r["grad_norm"])
        t += 1


def test_bad_arguments_return_an_error_and_leave_the_ring_alone():
    from demf_amd import _ffi, ops
    big, ring = _ring(4)
    before = big.clone()
    vec, scalars = _scalars(10, [float(i) for i in range(10)])
    st = _state(1.0, 0, 1.0)
    stream = torch.cuda.current_stream().cuda_stream

    def table(ptrs):
        return (ctypes.c_void_p * len(ptrs))(*ptrs)
    good = table([s.data_ptr() for s in scalars])
    eleven = table([s.data_ptr() for s in scalars] + [scalars[0].data_ptr()])
    holed = table([s.data_ptr() for s in scalars[:4]] + [None] + [s.data_ptr() for s in scalars[5:]])
    A = ctypes.addressof
    for what, args in (("n=0", (0, A(good), st.data_ptr(), 1.0, 10.0, ring.data_ptr(), 4)),
                       ("n=11", (11, A(eleven), st.data_ptr(), 1.0, 10.0, ring.data_ptr(), 4)),
                       ("ring of 0 rows", (10, A(good), st.data_ptr(), 1.0, 10.0, ring.data_ptr(), 0)),
                       ("null pointer", (10, A(good), st.data_ptr(), 1.0, 10.0, None, 4)),
                       ("null pointer", (10, A(good), None, 1.0, 10.0, ring.data_ptr(), 4)),
                       ("null pointer", (10, None, st.data_ptr(), 1.0, 10.0, ring.data_ptr(), 4)),
                       (r"null pointer \(scalar 4\)", (10, A(holed), st.data_ptr(), 1.0, 10.0, ring.data_ptr(), 4))):
        with pytest.raises(RuntimeError, match="demf_step_meter failed .*" + what):
            _ffi.call("demf_step_meter", *args, stream)
    # the Python wrapper refuses before it reaches the library
    with pytest.raises(ValueError):
        ops.step_meter([], st, 1.0, 10.0, ring)
    with pytest.raises(ValueError):
        ops.step_meter(scalars + scalars[:1], st, 1.0, 10.0, ring)
    with pytest.raises(TypeError):
        ops.step_meter([vec], st, 1.0, 10.0, ring)                    # ten floats are not a scalar
    with pytest.raises(TypeError):
        ops.step_meter([torch.zeros(1)], st, 1.0, 10.0, ring)         # a CPU tensor
    with pytest.raises(ValueError):
        ops.step_meter(scalars, st, 1.0, 10.0, big[:, :8])
    torch.cuda.synchronize()
    assert torch.equal(big, before)


def test_captured_launch_reads_fresh_values_at_every_replay():
    from demf_amd import meter, ops
    names = ("a", "b")
    vec, scalars = _scalars(2, [1.0, 2.0])
    st = _state(16.0, 5, 1.0)
    big, ring = _ring(4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.step_meter(scalars, st, 1.0, 10.0, ring)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.step_meter(scalars, st, 1.0, 10.0, ring)
    for t, a, b, sumsq in ((6, 10.5, -3.0, 25.0), (7, 11.5, -4.0, 900.0)):
        st.view(torch.int64)[1] = t
        st.view(torch.float64)[0] = sumsq
        vec[:2] = torch.tensor([a, b], device="cuda")
        g.replay()
    torch.cuda.synchronize()
    rows, nxt = meter.decode_ring(ring.cpu().numpy(), names, 5)
    assert nxt == 8
    assert [(r["t"], r["a"], r["b"], r["grad_norm"]) for r in rows] == [(5, 1.0, 2.0, 4.0), (6, 10.5, -3.0, 5.0),
                                                                       (7, 11.5, -4.0, 30.0)]
    assert rows[2]["clip"] == pytest.approx(1.0 / 3.0, rel=1e-6) and rows[1]["clip"] == 1.0


# ---- 2. eager metered steps ---------------------------------------------------------------------------------------
def _tiny_batch(seed, n_gt):
    """A batch as tests/test_gpu_engine.py builds it: three scenes of 1024 points on the tiny configuration."""
    from demf_amd import synthetic
    cfg = fixtures.tiny_cfg()
    raw = synthetic.make_scene_batch(3, 1024, fixtures.TINY_PYRAMID, fixtures.TINY_INPUT, cfg.head.embed_dims,
                                     seed=seed, n_gt=n_gt)
    return dict(points=torch.from_numpy(raw["points"]).cuda(),
                img_features=[torch.from_numpy(f).cuda() for f in raw["img_features"]],
                img_metas=raw["img_metas"],
                gt_bboxes_3d=[torch.from_numpy(b).cuda() for b in raw["gt_boxes"]],
                gt_labels_3d=[torch.from_numpy(l).cuda() for l in raw["gt_labels"]])


def _setup(seed=3, lr=1e-3, metered=True, **kw):
    """The trainer and batch of tests/test_gpu_engine.py, with a meter attached."""
    from demf_amd import engine, meter
    from demf_amd.modules import DeMFHotPath
    model = DeMFHotPath(fixtures.tiny_cfg())
    fixtures.seed_weights(model, seed)
    model.cuda().train()
    tr = engine.Trainer(model, lr=lr, **kw)
    m = None
    if metered:
        m = meter.StepMeter(meter.loss_names(), ring_rows=8)
        tr.attach_meter(m)
    return tr, m, _tiny_batch(seed, 4)


def _sumsq_squares_per_thread(n):
    """The launch geometry of demf_sumsq_f32 (csrc/optim.hip): min(1024, ceil(n / 2048)) workgroups of 256 threads, a
    grid-stride loop - so one thread adds at most ceil(n / threads) squares in fp32 before the fp64 block sums."""
    blocks = min(1024, -(-n // 2048))
    return -(-n // (blocks * 256))


def test_eager_metered_steps():
    from demf_amd import meter
    tr, m, batch = _setup()
    names = meter.loss_names()
    n = tr.flat.flat.numel()
    k = _sumsq_squares_per_thread(n)
    bar = (k + 2) * 2.0 ** -24
    totals, norms = [], []
    for _ in range(3):
        totals.append(tr.step(batch).clone())
        # FlatGrads: the update reads the flat gradient buffer and leaves it in place (demf_adamw_state_f32 takes
        # `grad` as const), so after the step it still holds the gradients whose norm was metered
        norms.append(float(tr.flat.flat.double().norm()))
    m.snapshot()
    rows = m.collect(wait=True)
    assert [r["t"] for r in rows] == [0, 1, 2] and tr.opt.t == 3 and m.next_t == 3
    assert m.collect(wait=True) == []
    for r, total, norm in zip(rows, totals, norms):
        assert r["nonfinite"] == () and r["lr_factor"] == 1.0
        assert np.float32(r["_total"]).tobytes() == np.float32(total.item()).tobytes()
        terms = [r[k_] for k_ in names[:-1]]
        assert abs(r["_total"] - sum(terms)) <= 8 * 2.0 ** -24 * sum(abs(v) for v in terms)
        rel = abs(r["grad_norm"] - norm) / norm
        print(f"t={r['t']} grad_norm {r['grad_norm']:.6f} fp64 {norm:.6f} rel {rel:.2e} (bar {bar:.2e}, k={k}, n={n})")
        assert rel <= bar
        want_clip = min(1.0, 10.0 / (r["grad_norm"] + 1e-6))
        assert r["clip"] == pytest.approx(want_clip, rel=1e-6)
    assert len({r["_total"] for r in rows}) == 3                       # three different steps


def test_meter_adds_exactly_one_launch_per_step(monkeypatch):
    from demf_amd import _ffi
    real = _ffi.call
    seqs = {}
    for metered in (False, True):
        tr, m, batch = _setup(metered=metered)
        tr.step(batch)                                                 # first step: one-off workspace queries
        per_step = []
        for _ in range(2):
            names = []

            def recording(name, *a, _names=names):
                _names.append(name)
                return real(name, *a)
            monkeypatch.setattr(_ffi, "call", recording)
            tr.step(batch)
            monkeypatch.setattr(_ffi, "call", real)
            per_step.append(names)
        seqs[metered] = per_step
    for plain, metered in zip(seqs[False], seqs[True]):
        assert plain.count("demf_step_meter") == 0 and metered.count("demf_step_meter") == 1
        i = metered.index("demf_step_meter")
        assert metered[i - 1] == "demf_sumsq_f32" and metered[i + 1] == "demf_adamw_state_f32"
        assert metered[:i] + metered[i + 1:] == plain and len(plain) > 50


def test_attach_meter_needs_the_device_path():
    from demf_amd import engine
    from demf_amd.modules import DeMFHotPath
    tr = engine.Trainer(DeMFHotPath(fixtures.tiny_cfg()))              # CPU: torch.optim.AdamW
    with pytest.raises(RuntimeError, match="CPU / gloo"):
        tr.attach_meter(object())


# ---- 3. captured metered steps ------------------------------------------------------------------------------------
def _pair():
    return [_tiny_batch(11, 4), _tiny_batch(12, 2)]                    # one shape, one GT bucket


def test_captured_metered_steps_in_a_step_cache():
    from demf_amd import meter
    batches = _pair()
    tr, m, _ = _setup(lr=2e-4)
    sc = tr.bucketed(max_graphs=1, capture_on=1, warmup=1)
    got = []
    for i in range(4):
        nxt = batches[(i + 1) % 2]["points"]
        got.append(float(sc.step(batches[i % 2], next_points=nxt)))
    assert next(iter(sc.graphs.values())).update_in_graph and next(iter(sc.graphs.values())).metered
    m.snapshot()
    rows = m.collect(wait=True)
    # the ring started at -1 and the dry capture's warm-up pass ran no update: no row for a step that did not happen
    assert [r["t"] for r in rows] == [0, 1, 2, 3] and tr.opt.t == 4
    stamps = m.ring.cpu().numpy()[:, :2].copy().view(np.int64)[:, 0].tolist()
    assert stamps == [0, 1, 2, 3, -1, -1, -1, -1]
    for r, loss in zip(rows, got):
        assert r["nonfinite"] == ()
        assert np.float32(r["_total"]).tobytes() == np.float32(loss).tobytes()
    assert abs(got[0] - got[1]) > 1e-3 * got[0]                        # the two batches really differ
    # the same batches without a meter: same bookkeeping
    tr2, _, _ = _setup(lr=2e-4, metered=False)
    sc2 = tr2.bucketed(max_graphs=1, capture_on=1, warmup=1)
    plain = [float(sc2.step(batches[i % 2], next_points=batches[(i + 1) % 2]["points"])) for i in range(4)]
    assert sc2.stats == sc.stats == dict(eager=0, replayed=4, captured=1, evicted=0)
    assert tr2.opt.t == 4 and plain == pytest.approx(got, rel=5e-3)
    assert not next(iter(sc2.graphs.values())).metered
    # a captured step is metered or not for good
    tr2.attach_meter(meter.StepMeter(meter.loss_names(), ring_rows=8))
    with pytest.raises(RuntimeError, match="captured without a step meter"):
        sc2.step(batches[0])


@pytest.mark.parametrize("overlap", [False, True])
def test_captured_step_with_an_eager_or_deferred_update(overlap):
    """The update outside the graph: the replay closure hands ITS loss tensors to the metered update - also when that
    update is deferred behind an overlapped collective (here a spin kernel in its place) and enqueued by the next
    replay or by flush()."""
    batches = _pair()
    tr, m, _ = _setup(lr=2e-4)
    if overlap:
        tr.allreduce_stub_us, tr.allreduce_overlap = 20, True
    replay = tr.capture(batches[0], warmup=1, dry=True, max_gt=8, update_in_graph=False)
    assert replay.metered and not replay.update_in_graph
    # a second graph alive at the same time, as in a StepCache: its loss tensors are not the first one's
    other = tr.capture(batches[1], warmup=1, dry=True, max_gt=8, update_in_graph=False, geo_pipe=replay.geo)
    got = []
    for i in range(4):
        r = replay if i % 2 == 0 else other
        r.load(batches[i % 2])                                         # (the two share the pre-pass pipeline)
        got.append(float(r()))
    assert bool(getattr(tr, "_pending_update", False)) == overlap
    tr.flush()
    m.snapshot()
    rows = m.collect(wait=True)
    assert [r["t"] for r in rows] == [0, 1, 2, 3] and tr.opt.t == 4
    for r, loss in zip(rows, got):
        assert np.float32(r["_total"]).tobytes() == np.float32(loss).tobytes()
    assert abs(got[0] - got[1]) > 1e-3 * got[0]


# ---- 4. no host sync ----------------------------------------------------------------------------------------------
_SYNC_DEBUG_CHILD = """
import time
import torch
from demf_amd import meter
names = ("a", "b", "_total")
m = meter.StepMeter(names, ring_rows=8)
vec = torch.tensor([1.5, 2.5, 4.0], device="cuda")
scalars = [vec[0], vec[1], vec[2]]
st = torch.zeros(64, dtype=torch.uint8, device="cuda")
st.view(torch.float64)[0] = 4.0
st.view(torch.float32)[5] = 1.0
steps = [st.clone() for _ in range(3)]
for t, s in enumerate(steps):
    s.view(torch.int64)[1] = t
m.record(scalars, steps[0], 1.0, 10.0)
m.snapshot()                                    # (allocates the pinned buffer)
torch.cuda.synchronize()
assert [r["t"] for r in m.collect()] == [0]
torch.cuda.set_sync_debug_mode("error")
try:
    for s in steps[1:]:
        m.record(scalars, s, 1.0, 10.0)
    m.snapshot()
    rows = m.collect(wait=False)
    deadline = time.time() + 60
    while len(rows) < 2 and time.time() < deadline:
        rows += m.collect(wait=False)
finally:
    torch.cuda.set_sync_debug_mode("default")
assert [(r["t"], r["a"], r["_total"], r["grad_norm"]) for r in rows] == [(1, 1.5, 4.0, 2.0), (2, 1.5, 4.0, 2.0)], rows
print("SYNC_DEBUG_OK")
"""


def test_record_snapshot_collect_do_not_synchronise():
    """record + snapshot + collect(wait=False) under torch.cuda.set_sync_debug_mode("error"), in a process of its own
    (as tests/test_gpu_detections.py::test_no_host_sync_under_sync_debug_mode, and for its reason)."""
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", _SYNC_DEBUG_CHILD], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SYNC_DEBUG_OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


# ---- 5. the runner end to end -------------------------------------------------------------------------------------
SEED = 5
MIXED = [(6000, (53, 73), 3), (5000, (43, 56), 0), (7000, (44, 59), 4), (4500, (48, 64), 2)]
SAME_SIZE = [(6000, (53, 73), 3), (5000, (53, 73), 0), (7000, (53, 73), 4), (4500, (53, 73), 2)]


def _detector(seed=1):
    from demf_amd.modules import DeMFVoteNet
    from test_gpu_detector import STREAM, _cfg256
    det = DeMFVoteNet(_cfg256(), **STREAM)
    fixtures.seed_weights(det, seed)
    return det


def _fit_kwargs(**kw):
    from test_gpu_pipeline import IMG_SCALE
    out = dict(batch_size=2, num_points=2048, img_scale=IMG_SCALE, max_epochs=2, repeat=1, lr_steps=(1,),
               log_interval=1, eval_interval=2, seed=SEED, workers=4, echo=False)
    out.update(kw)
    return out


def _log(work_dir):
    with open(os.path.join(work_dir, "train.log.json")) as f:
        return [json.loads(l) for l in f if l.strip()]


_RUNS = {}


def _run(tmp_path_factory, graphs):
    """One two-epoch run per mode, shared by the tests below (never modified afterwards)."""
    if graphs in _RUNS:
        return _RUNS[graphs]
    import pipeline_reference as pref
    from demf_amd import train
    from demf_amd.dataset import SUNRGBDDataset
    root = str(tmp_path_factory.mktemp("graphs" if graphs else "eager"))
    # one scene without ground truth either way; ONE image size for the captured run, so that a shape key repeats
    specs = SAME_SIZE if graphs else MIXED
    assert sum(1 for s in specs if s[2] == 0) == 1
    ann, _ = pref.write_dataset(root, specs, jpeg=True)
    ds = SUNRGBDDataset(root, ann)
    val = SUNRGBDDataset(root, ann, test_mode=True)
    det = _detector()
    init = {k: v.clone() for k, v in det.state_dict().items()}
    steps = []
    work = os.path.join(root, "work")
    out = train.fit(det, ds, work, val_set=val, graphs=graphs, on_step=lambda info: steps.append(
        (info["epoch"], info["iter"], info["indices"], info["loss"].clone())), **_fit_kwargs())
    torch.cuda.synchronize()
    _RUNS[graphs] = dict(root=root, ann=ann, ds=ds, det=det, init=init, steps=steps, work=work, out=out)
    return _RUNS[graphs]


@pytest.mark.parametrize("graphs", [False, True])
def test_runner_end_to_end(tmp_path_factory, graphs):
    from demf_amd import infer, meter
    from demf_amd import pipeline as pl
    from test_gpu_pipeline import IMG_SCALE
    run = _run(tmp_path_factory, graphs)
    det, out = run["det"], run["out"]
    lines = _log(run["work"])
    train_lines = [l for l in lines if l["mode"] == "train"]
    print(json.dumps(train_lines))
    assert [(l["epoch"], l["iter"]) for l in train_lines] == [(1, 1), (1, 2), (2, 3), (2, 4)]
    want_keys = {"mode", "epoch", "iter", "lr", "loss", "grad_norm", "time"} | set(meter.loss_names()[:-1])
    for l in train_lines:
        assert set(l) == want_keys
        assert all(np.isfinite(v) for k, v in l.items() if k != "mode"), l
        assert l["loss"] > 0 and l["grad_norm"] > 0 and l["time"] > 0
    assert train_lines[0]["lr"] == train_lines[1]["lr"] == pytest.approx(0.008, rel=1e-6)
    assert train_lines[2]["lr"] == train_lines[3]["lr"] == pytest.approx(0.1 * train_lines[0]["lr"], rel=1e-6)
    # log_interval = 1: a line is one step, and its loss is the one that step returned
    for l, (_, _, _, loss) in zip(train_lines, run["steps"]):
        assert l["loss"] == float(loss)
    val_lines = [l for l in lines if l["mode"] == "val"]
    assert len(val_lines) == 1 and lines[-1] is val_lines[0] and len(lines) == 5
    assert "mAP_0.25" in val_lines[0] and "mAP_0.50" in val_lines[0] and val_lines[0]["epoch"] == 2
    assert set(out["val"]) == set(val_lines[0]) - {"mode", "epoch", "iter"}
    # the mode afterwards: training, the frozen image branch in eval
    assert det.training and det.pts_bbox_head.training
    assert not (det.img_backbone.training or det.img_neck.training or det.img_encoder.training)
    sd = det.state_dict()
    moved = [k for k, v in sd.items() if k.startswith("pts_") and not torch.equal(v.cpu(), run["init"][k].cpu())]
    assert len(moved) > 50
    assert all(torch.equal(v.cpu(), run["init"][k].cpu()) for k, v in sd.items() if k.startswith("img_"))
    assert sorted(f for f in os.listdir(run["work"]) if not f.endswith(".json")) == ["epoch_2.pth", "latest.pth"]
    fresh = _detector(seed=2)
    infer.load_checkpoint(fresh, os.path.join(run["work"], "latest.pth"))
    got = fresh.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v.cpu()), k
    # every iteration saw the scenes a bare loader with the same seed yields
    bare = pl.SceneLoader(run["ds"], 2, "train", seed=SEED, img_scale=IMG_SCALE, num_points=2048, workers=4)
    want = [(e + 1, b.indices) for e in range(2) for b in bare]
    assert [(e, idx) for e, _, idx, _ in run["steps"]] == want
    assert sorted(i for _, idx in want[:2] for i in idx) == [0, 1, 2, 3]
    assert [i for _, i, _, _ in run["steps"]] == [1, 2, 3, 4]
    assert out["trainer"].opt.t == 4 and out["iter"] == 4 and out["meter"].next_t == 4
    if graphs:
        assert out["stepper"].stats["replayed"] > 0 and out["stepper"].stats["captured"] >= 1, out["stepper"].stats
    else:
        assert out["stepper"] is None


def test_command_line(tmp_path_factory, capsys):
    from demf_amd import train
    from test_gpu_pipeline import IMG_SCALE
    run = _run(tmp_path_factory, False)
    work = os.path.join(run["root"], "work_cli")
    capsys.readouterr()
    ret = train.main(["--data-root", run["root"], "--ann-file", os.path.basename(run["ann"]), "--val-ann-file", run["ann"],
                      "--work-dir", work, "--no-graphs", "--batch-size", "2", "--epochs", "1", "--seed", str(SEED),
                      "--workers", "4", "--log-interval", "1"],
                     model=_detector(), num_points=2048, img_scale=IMG_SCALE, repeat=1)
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    ref = _log(run["work"])
    filed = _log(work)
    assert [l["mode"] for l in printed] == [l["mode"] for l in filed] == ["train", "train", "val"]
    assert printed[:2] == filed[:2] and set(printed[2]) == set(filed[2])
    assert set(printed[0]) == set(ref[0]) and set(printed[-1]) == set(ref[-1]) and set(ret["val"]) == set(run["out"]["val"])
    assert sorted(f for f in os.listdir(work) if f.endswith(".pth")) == ["epoch_1.pth", "latest.pth"]
    # the same seed, data and weights: the first epoch sees the same scenes and starts from the same loss
    assert printed[0]["loss"] == pytest.approx(ref[0]["loss"], rel=1e-3)


# ---- 6. resume ----------------------------------------------------------------------------------------------------
def test_resume_continues_the_run(tmp_path_factory):
    from demf_amd import engine, fused, meter, train
    from demf_amd.modules import DeMFHotPath
    import functools
    a = _run(tmp_path_factory, False)                                  # run A: two epochs, uninterrupted
    work = os.path.join(a["root"], "work_b")
    steps = []
    on_step = lambda info: steps.append((info["epoch"], info["iter"], info["indices"], info["loss"].clone()))  # noqa: E731
    first = train.fit(_detector(), a["ds"], work, graphs=False, on_step=on_step, **_fit_kwargs(max_epochs=1))
    latest = os.path.join(work, "latest.pth")
    ckpt = train.load_checkpoint_file(latest)
    assert ckpt["meta"]["epoch"] == 1 and ckpt["meta"]["iter"] == 2 and ckpt["meter"] == dict(next_t=2)
    assert first["trainer"].opt.t == 2
    # straight after loading, a fresh model / trainer / meter hold the checkpoint bit for bit
    det = _detector(seed=9).cuda()
    tr = engine.Trainer(det, forward=functools.partial(DeMFHotPath.forward_train, det))
    m = meter.StepMeter(meter.loss_names())
    tr.attach_meter(m)
    meta = train.restore_checkpoint(ckpt, det, tr, m)
    assert meta == ckpt["meta"]
    sd = det.state_dict()
    assert set(sd) == set(ckpt["state_dict"])
    n_bn = 0
    for k, v in ckpt["state_dict"].items():                            # parameters and BatchNorm buffers
        assert torch.equal(sd[k].cpu(), v), k
        n_bn += k.endswith("running_mean") and k.startswith("pts_")
    assert n_bn > 5
    opt = ckpt["trainer"]["optimizer"]
    assert torch.equal(tr.opt.exp_avg.cpu(), opt["exp_avg"]) and torch.equal(tr.opt.exp_avg_sq.cpu(), opt["exp_avg_sq"])
    assert float(opt["exp_avg"].abs().sum()) > 0
    assert tr.opt.t == opt["t"] == 2
    assert tr.opt.lr_factor == opt["lr_factor"] == 1.0
    assert float(tr.opt.state.view(torch.float32)[5]) == 1.0
    assert fused.get_rng_state("cuda") == list(ckpt["trainer"]["dropout_rng"])
    assert m.next_t == 2
    del tr, m, det
    # run B goes on from the file with a fresh model
    second = train.fit(_detector(seed=9), a["ds"], work, graphs=False, resume_from=latest, on_step=on_step,
                       **_fit_kwargs(max_epochs=2))
    torch.cuda.synchronize()
    assert [(e, i, idx) for e, i, idx, _ in steps] == [(e, i, idx) for e, i, idx, _ in a["steps"]]
    assert steps[2][0] == 2 and steps[2][1] == 3
    assert second["trainer"].opt.t == 4 and second["iter"] == 4 and second["meter"].next_t == 4
    lines = _log(work)
    assert [(l["epoch"], l["iter"]) for l in lines] == [(1, 1), (1, 2), (2, 3), (2, 4)]
    assert lines[2]["lr"] == pytest.approx(0.0008, rel=1e-6)
    # (two runs differ in their last bits through the backbone's fp32 atomics: finiteness only)
    assert all(np.isfinite(v) for l in lines for k, v in l.items() if k != "mode")
    assert all(bool(torch.isfinite(loss)) for _, _, _, loss in steps)
    assert sorted(f for f in os.listdir(work) if f.endswith(".pth")) == ["epoch_2.pth", "latest.pth"]
    assert train.load_checkpoint_file(latest)["meta"]["iter"] == 4
