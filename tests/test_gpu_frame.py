"""csrc/frame.hip (ops.depth_to_points) against the fp64 numpy restatement of tests/frame_reference.py: records and
offsets BIT for bit - every step is one IEEE operation in a fixed order, so there is nothing to tolerate - at the
edges of the tile, for every validity pattern, ragged batches, and chained into the input pipeline's kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frame_reference as fref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _tile():
    from demf_amd import ops
    return ops.FRAME_TILE


def _rotl16(d, s):
    d = np.asarray(d, np.uint32)
    return (((d << s) | (d >> (16 - s))) & 0xFFFF).astype(np.uint16)


def _calib(rng, h, w, **kw):
    K = np.array([[529.5 * w / 730 + rng.uniform(-3, 3), 0, w / 2 + rng.uniform(-2, 2)],
                  [0, 529.5 * h / 530 + rng.uniform(-3, 3), h / 2 + rng.uniform(-2, 2)], [0, 0, 1.0]])
    tilt, roll = rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05)
    rx = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
    ry = np.array([[np.cos(roll), 0, np.sin(roll)], [0, 1, 0], [-np.sin(roll), 0, np.cos(roll)]])
    return fref.calib_row(K, rx @ ry, **kw)


PATTERNS = ("all", "none", "first", "last", "checker", "random")


def _mask(pattern, h, w, rng):
    m = np.zeros((h, w), bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m.flat[0] = True
    elif pattern == "last":
        m.flat[-1] = True
    elif pattern == "checker":
        m = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    elif pattern == "random":
        m = rng.random((h, w)) < 0.5
    return m


def _frame(rng, h, w, pattern, shift, **calib_kw):
    """-> (stored depth words, rgb, calib row): readings of 0.3 .. 12 m in millimetres (a third beyond z_max = 8 m)."""
    mm = rng.integers(300, 12000, size=(h, w)).astype(np.uint16)
    mm[~_mask(pattern, h, w, rng)] = 0
    return _rotl16(mm, shift), rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), _calib(rng, h, w, **calib_kw)


def _upload(frames):
    depths, rgbs, calibs = zip(*frames)
    doff = np.concatenate([[0], np.cumsum([d.size for d in depths])]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([c.size for c in rgbs])]).astype(np.int64)
    shp = np.array([[*d.shape, *d.shape] for d in depths], np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
    return (up(np.concatenate([d.reshape(-1) for d in depths])), up(doff),
            up(np.concatenate([c.reshape(-1) for c in rgbs])), up(roff), up(shp), up(np.stack(calibs)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(frames, shift, what=""):
    """Run the operator into a sentinel-filled buffer and compare with the reference, bit for bit."""
    from demf_amd import ops
    args = _upload(frames)
    total = args[0].numel()
    out = torch.full((total, 6), SENTINEL, dtype=torch.float32, device="cuda")
    raw, off = ops.depth_to_points(*args, shift=shift, out=out)
    assert raw is out and off.dtype == torch.int64 and off.shape == (len(frames) + 1,) and off.is_cuda
    want, want_off = fref.depth_to_points(*zip(*frames), shift=shift)
    got, got_off = raw.cpu().numpy(), off.cpu().numpy()
    print(f"{what}: {total} pixels, offsets {got_off.tolist()}, expected {want_off.tolist()}")
    np.testing.assert_array_equal(got_off, want_off)
    n = int(want_off[-1])
    assert np.array_equal(_bits(got[:n]), _bits(want)), \
        f"{what}: {(_bits(got[:n]) != _bits(want)).any(1).sum()} of {n} records differ"
    assert (got[n:] == SENTINEL).all(), f"{what}: rows at or beyond offsets[B] were written"
    return raw, off, args


def _sizes():
    T = _tile()
    return [(1, T - 1), (1, T), (1, T + 1), (1, 2 * T + 1), (1, 1), (3, 5), (37, 53), (127, 129)]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", range(8))
def test_one_frame_bit_equal_at_tile_edges(size, pattern):
    h, w = _sizes()[size]
    rng = np.random.default_rng(100 * size + PATTERNS.index(pattern))
    _check([_frame(rng, h, w, pattern, 3)], 3, f"{h}x{w} {pattern}")


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("origin", [0.0, 1.0])
def test_ragged_batch_with_an_empty_frame_in_the_middle(shift, origin):
    """B = 3, a calibration per frame, the middle frame without a valid pixel: its two offsets are equal."""
    T = _tile()
    rng = np.random.default_rng(7 + shift)
    frames = [_frame(rng, 37, 53, "random", shift, pixel_origin=origin),
              _frame(rng, 1, T - 1, "none", shift, pixel_origin=origin),
              _frame(rng, 127, 129, "checker", shift, pixel_origin=origin, z_max=6.0, depth_scale=1250.0)]
    _, off, _ = _check(frames, shift, f"ragged shift {shift} origin {origin}")
    off = off.tolist()
    assert off[0] == 0 and off[1] == off[2] and off[3] > off[2] > 0


def test_frames_that_end_inside_a_tile_and_first_frame_empty():
    T = _tile()
    rng = np.random.default_rng(11)
    frames = [_frame(rng, 3, 5, "none", 3), _frame(rng, 1, T + 1, "all", 3), _frame(rng, 1, 1, "all", 3),
              _frame(rng, 1, T - 1, "last", 3), _frame(rng, 37, 53, "random", 3)]
    _check(frames, 3, "five frames")


def test_readings_beyond_z_max_are_clamped_not_dropped():
    rng = np.random.default_rng(12)
    depth, rgb, calib = _frame(rng, 3, 5, "all", 3)
    depth[1, 2] = _rotl16(np.uint16(9000), 3)                     # 9 m
    depth[2, 4] = 7                                               # rotates to 57 344: 57.344 m
    raw, off, _ = _check([(depth, rgb, calib)], 3, "z_max")
    assert off.tolist() == [0, 15]
    want = fref.frame_records(depth, rgb, calib, 3)
    assert np.array_equal(_bits(raw.cpu().numpy()[:15]), _bits(want))


def test_full_frame_and_two_runs_bit_identical():
    from demf_amd import ops
    rng = np.random.default_rng(13)
    raw, off, args = _check([_frame(rng, 530, 730, "random", 3)], 3, "530x730")
    again, off2 = ops.depth_to_points(*args, shift=3, out=torch.full_like(raw, SENTINEL))
    assert torch.equal(raw.view(torch.int32), again.view(torch.int32)) and torch.equal(off, off2)
    assert 150000 < int(off[-1]) < 250000


# ---- operator behaviour ----------------------------------------------------------------------------------------------
def test_ffi_call_count_does_not_depend_on_batch(monkeypatch):
    from demf_amd import _ffi, ops
    real = _ffi.call
    rng = np.random.default_rng(14)
    counts = []
    for B in (1, 3):
        args = _upload([_frame(rng, 37, 53, "random", 3) for _ in range(B)])
        names = []

        def recording(name, *a, _n=names):
            _n.append(name)
            return real(name, *a)
        monkeypatch.setattr(_ffi, "call", recording)
        ops.depth_to_points(*args)
        monkeypatch.setattr(_ffi, "call", real)
        counts.append(names)
    assert counts[0] == counts[1] == ["demf_depth_to_points"]


def test_bad_arguments_raise_without_a_launch(monkeypatch):
    from demf_amd import _ffi, ops
    rng = np.random.default_rng(15)
    good = _upload([_frame(rng, 3, 5, "all", 3) for _ in range(2)])
    calls = []
    monkeypatch.setattr(_ffi, "call", lambda *a: calls.append(a))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.depth_to_points(*[t.cpu() for t in good])
    for i in range(6):
        bad = list(good)
        bad[i] = good[i].cpu()
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.depth_to_points(*bad)
    wrong = {0: torch.int16, 1: torch.int32, 2: torch.int8, 3: torch.int32, 4: torch.int64, 5: torch.float32}
    for i, dt in wrong.items():
        bad = list(good)
        bad[i] = good[i].to(dt)
        with pytest.raises(TypeError):
            ops.depth_to_points(*bad)
    with pytest.raises(ValueError, match="calib"):
        ops.depth_to_points(*good[:5], good[5][:, :15].contiguous())
    with pytest.raises(ValueError):
        ops.depth_to_points(*good[:4], good[4][:1], good[5])                   # shapes of another B
    with pytest.raises(ValueError):
        ops.depth_to_points(good[0][:0], *good[1:])                            # no pixels
    with pytest.raises(ValueError):
        ops.depth_to_points(*good, shift=16)
    with pytest.raises(ValueError, match="out must be"):
        ops.depth_to_points(*good, out=torch.empty((29, 6), device="cuda"))
    assert calls == []


_SYNC_DEBUG_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import numpy as np
import torch
import test_gpu_frame as t
from demf_amd import ops
rng = np.random.default_rng(16)
frames = [t._frame(rng, 37, 53, "random", 3), t._frame(rng, 3, 5, "none", 3), t._frame(rng, 127, 129, "random", 3)]
args = t._upload(frames)
first = ops.depth_to_points(*args)
torch.cuda.synchronize()
torch.cuda.set_sync_debug_mode("error")
try:
    raw, off = ops.depth_to_points(*args)
finally:
    torch.cuda.set_sync_debug_mode("default")
assert torch.equal(off, first[1]) and int(off[-1]) > 1000
n = int(off[-1])
assert torch.equal(raw[:n].view(torch.int32), first[0][:n].view(torch.int32))
print("SYNC_DEBUG_OK")
"""


def test_no_host_sync_under_sync_debug_mode():
    """ops.depth_to_points under torch.cuda.set_sync_debug_mode("error"): a synchronising torch call would raise.  In
    a process of its own, as in test_gpu_detections.py (the mode, once set, changes what torch's profiler records)."""
    from conftest import ROOT
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    flags = ["-s"] if sys.flags.no_user_site else []
    child = _SYNC_DEBUG_CHILD.format(tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + flags + ["-c", child], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "SYNC_DEBUG_OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


# ---- into the input pipeline's kernels ---------------------------------------------------------------------------------
def test_chain_into_points_floor_and_points_prep():
    """depth_to_points -> points_floor -> points_prep equals the same two operators fed the reference's records
    uploaded from the host, bit for bit; the frame without a valid pixel gives NaN, as those kernels define."""
    from demf_amd import ops
    from demf_amd import pipeline as pl
    rng = np.random.default_rng(17)
    k = 2048
    frames = [_frame(rng, 37, 53, "checker", 3),                  # 981 valid < k: sampled with replacement
              _frame(rng, 3, 5, "none", 3),
              _frame(rng, 127, 129, "random", 3)]                 # ~8 000 valid > k: keyed permutation
    raw, off, _ = _check(frames, 3, "chain")
    want, want_off = fref.depth_to_points(*zip(*frames), shift=3)
    assert want_off[1] < k < want_off[3] - want_off[2]
    raw_ref, off_ref = torch.from_numpy(want).cuda(), torch.from_numpy(want_off).cuda()
    params = torch.from_numpy(np.stack([pl.param_row(pl.identity_aug_params())] * 3)).cuda()
    seeds = torch.tensor([5, 6, 7], dtype=torch.int64, device="cuda")
    floor, floor_ref = ops.points_floor(raw, off), ops.points_floor(raw_ref, off_ref)
    pts = ops.points_prep(raw, off, floor, params, seeds, k)
    pts_ref = ops.points_prep(raw_ref, off_ref, floor_ref, params, seeds, k)
    assert torch.equal(floor.view(torch.int32), floor_ref.view(torch.int32))
    assert torch.equal(pts.view(torch.int32), pts_ref.view(torch.int32))
    assert bool(torch.isnan(floor[1])) and bool(torch.isnan(pts[1]).all())
    assert bool(torch.isfinite(floor[[0, 2]]).all()) and bool(torch.isfinite(pts[[0, 2]]).all())
