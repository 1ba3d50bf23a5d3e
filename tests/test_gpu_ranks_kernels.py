"""csrc/ranks.hip on the GPU, single process: ops.store_concat and ops.meter_merge bit for bit against the numpy
restatement (ranks_reference.py), with guard rows and guard scenes behind every destination array."""
import ctypes

import numpy as np
import pytest
import torch

import ranks_reference as rref

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
GUARD = 5


# ---- store_concat ---------------------------------------------------------------------------------------------------
def _rank_stores(rng, counts, S, R, fills):
    """Stacked source arrays of W ranks.  ``fills[r]``: the rows of rank r's scenes (a list of n_r ints; their sum may
    exceed R: the rank overflowed, its cursor keeps counting and its state[1] is set).  Everything the rank did not
    write is noise, as in a store that is reused."""
    W = len(counts)
    off = rng.integers(-50, 50, size=(W, S + 1)).astype(np.int32)          # noise behind the cursor
    state = np.zeros((W, 2), np.int32)
    boxes = rng.standard_normal((W, R, 7)).astype(np.float32)
    scores = rng.random((W, R)).astype(np.float32)
    labels = rng.integers(0, 10, size=(W, R)).astype(np.int32)
    for r in range(W):
        assert len(fills[r]) == counts[r]
        off[r, :counts[r] + 1] = np.concatenate([[0], np.cumsum(fills[r])])
        state[r] = (off[r, counts[r]], int(off[r, counts[r]] > R))
    return off, state, boxes, scores, labels


def _guarded(scenes, rows):
    """Destination arrays as views into canary buffers with GUARD scenes / rows behind them (and, inside, canaries
    where nothing must be written)."""
    def mk(shape, dtype):
        big = torch.full((shape[0] + GUARD,) + tuple(shape[1:]), CANARY, dtype=torch.int32, device="cuda")
        return big, big[:shape[0]].view(dtype)
    out = {}
    out["scene_off"] = mk((scenes + 1,), torch.int32)
    out["state"] = mk((2,), torch.int32)
    out["boxes"] = mk((rows, 7), torch.float32)
    out["scores"] = mk((rows,), torch.float32)
    out["labels"] = mk((rows,), torch.int32)
    return out


def _run_concat(counts, src, scenes, rows):
    from demf_amd import ops
    dst = _guarded(scenes, rows)
    before = {k: v[1].cpu().numpy().copy() for k, v in dst.items()}
    dev = [torch.from_numpy(a).cuda() for a in src]
    ops.store_concat(counts, *dev, dst["boxes"][1], dst["scores"][1], dst["labels"][1], dst["scene_off"][1],
                     dst["state"][1])
    torch.cuda.synchronize()
    want = rref.store_concat(counts, *src, before)
    for k, (big, view) in dst.items():
        got = view.cpu().numpy()
        assert got.view(np.uint32).tobytes() == want[k].view(np.uint32).tobytes(), k
        assert (big[view.shape[0]:] == CANARY).all(), f"{k}: guard written"
    return want


def test_one_rank_is_the_identity():
    rng = np.random.default_rng(1)
    counts, S, R = [3], 4, 40
    src = _rank_stores(rng, counts, S, R, [[7, 0, 12]])
    want = _run_concat(counts, src, S, R)
    assert (want["scene_off"][:4] == src[0][0, :4]).all() and want["state"].tolist() == [19, 0]
    assert (want["boxes"][:19] == src[2][0, :19]).all()


def test_three_ranks_with_an_empty_one_and_empty_scenes():
    rng = np.random.default_rng(2)
    counts, S, R = [2, 0, 1], 2, 6
    want = _run_concat(counts, _rank_stores(rng, counts, S, R, [[1, 2], [], [1]]), 5, 9)
    assert want["scene_off"][:4].tolist() == [0, 1, 3, 4] and want["state"].tolist() == [4, 0]
    # scenes with zero rows in the middle of a rank and at a rank's end, and a rank exactly full (rows_r == R)
    counts, S, R = [4, 3, 2], 4, 10
    fills = [[3, 0, 2, 0], [4, 6, 0], [0, 5]]
    want = _run_concat(counts, _rank_stores(rng, counts, S, R, fills), 9, 30)
    assert want["scene_off"][:10].tolist() == [0, 3, 3, 5, 5, 9, 15, 15, 15, 20] and want["state"].tolist() == [20, 0]


def test_a_rank_that_overflowed():
    rng = np.random.default_rng(3)
    counts, S, R = [2, 2], 3, 8
    src = _rank_stores(rng, counts, S, R, [[5, 6], [2, 1]])             # rank 0 needs 11 rows, holds 8
    assert src[1][0].tolist() == [11, 1]
    want = _run_concat(counts, src, 4, 20)
    assert want["scene_off"][:5].tolist() == [0, 5, 11, 13, 14] and want["state"].tolist() == [14, 1]
    # rows 8 .. 10 of the destination have no source (nothing is read beyond R): they keep their canaries
    assert (want["scores"][8:11].view(np.uint32) == CANARY).all()
    assert (want["scores"][11:14] == src[3][1, :3]).all()


def test_a_destination_one_row_too_small():
    rng = np.random.default_rng(4)
    counts, S, R = [2, 1, 2], 2, 7
    fills = [[3, 4], [2], [1, 3]]
    src = _rank_stores(rng, counts, S, R, fills)
    want = _run_concat(counts, src, 5, 12)                               # 13 rows are needed
    assert want["state"].tolist() == [13, 1] and want["scene_off"][5] == 13
    assert (want["scores"][9:12] == src[3][2, :3]).all()                 # every row below max_rows is there
    fits = _run_concat(counts, src, 5, 13)
    assert fits["state"].tolist() == [13, 0]


def test_sixteen_ranks_straddle_workgroups():
    rng = np.random.default_rng(5)
    W, S, R = 16, 6, 3000
    counts = [int(c) for c in rng.integers(0, S + 1, size=W)]
    counts[3], counts[7] = 0, S
    fills = []
    for r in range(W):
        total = [0, 1, 255, 256, 257, 1023, 1025, 2999, 3000][r % 9] if counts[r] else 0
        cut = np.sort(rng.integers(0, total + 1, size=max(counts[r] - 1, 0)))
        fills.append(np.diff(np.concatenate([[0], cut, [total]])).astype(int).tolist() if counts[r] else [])
    src = _rank_stores(rng, counts, S, R, fills)
    rows = int(sum(sum(f) for f in fills))
    want = _run_concat(counts, src, sum(counts) + 2, rows + 3)
    assert want["state"].tolist() == [rows, 0]


def test_bad_arguments_write_nothing():
    from demf_amd import _ffi, ops
    rng = np.random.default_rng(6)
    W, S, R = 65, 1, 2
    counts = [1] * W
    src = _rank_stores(rng, counts, S, R, [[1]] * W)
    dst = _guarded(W, W * R)
    dev = [torch.from_numpy(a).cuda() for a in src]
    args = (dst["boxes"][1], dst["scores"][1], dst["labels"][1], dst["scene_off"][1], dst["state"][1])
    with pytest.raises(RuntimeError, match=r"code -3.*at most 64"):
        ops.store_concat(counts, *dev, *args)
    tab = (ctypes.c_int * 2)(1, 1)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ffi.call("demf_store_concat", 2, ctypes.addressof(tab), S, R, None, dev[1].data_ptr(),
                  dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), W, W * R, args[0].data_ptr(),
                  args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), args[4].data_ptr(), None)
    with pytest.raises(RuntimeError, match="holds 2 scenes, its capacity is 1"):
        ops.store_concat([2, 0], *[d[:2].contiguous() for d in dev], *args)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.store_concat([1] * 4, *[d[:4].contiguous() for d in dev], args[0], args[1], args[2],
                         dst["scene_off"][1][:4], args[4])
    torch.cuda.synchronize()
    for k, (big, _) in dst.items():
        assert (big == CANARY).all(), k


# ---- meter_merge ----------------------------------------------------------------------------------------------------
def _rings(rng, W, rows):
    """W rings holding the same steps (a wrapped run: row i holds step 3 * rows + i), equal head words, each rank its
    own scalars - of mixed sign and magnitude, so that the fp64 sum and its one rounding matter."""
    from demf_amd import meter
    rings = np.stack([meter.empty_ring(rows) for _ in range(W)])
    f = rings.view(np.float32)
    head = rng.random((rows, 3)).astype(np.float32)
    for r in range(W):
        rings[r, :, :2] = (3 * rows + np.arange(rows, dtype=np.int64)).view(np.int32).reshape(rows, 2)
        f[r, :, 3:6] = head
        f[r, :, 6:] = (rng.standard_normal((rows, 10)) * 10.0 ** rng.integers(-3, 4, size=(rows, 10))).astype(np.float32)
    if rows > 1:
        rings[:, rows - 1] = meter.empty_ring(1)[0]                    # a row never written, on every rank
    return rings


def _run_merge(rings):
    from demf_amd import ops
    W, rows, _ = rings.shape
    big = torch.full((rows + 2 * GUARD, 16), CANARY, dtype=torch.int32, device="cuda")
    out = big[GUARD:GUARD + rows]
    got = ops.meter_merge(torch.from_numpy(rings).cuda(), out)
    torch.cuda.synchronize()
    assert got is out
    want = rref.meter_merge(rings)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert (big[:GUARD] == CANARY).all() and (big[GUARD + rows:] == CANARY).all()
    return want


@pytest.mark.parametrize("W", [1, 2, 8, 16])
@pytest.mark.parametrize("rows", [1, 128, 257])
def test_meter_merge_matches_the_reference(W, rows):
    rings = _rings(np.random.default_rng([7, W, rows]), W, rows)
    want = _run_merge(rings)
    if W == 1:
        assert want.tobytes() == rings[0].tobytes()                     # a bit copy
    else:
        assert (want[:, :6] == rings[0][:, :6]).all()


def test_meter_merge_flags_nonfinite_values_and_disagreeing_stamps():
    from demf_amd import meter
    rng = np.random.default_rng(8)
    W, rows = 3, 8
    rings = _rings(rng, W, rows)
    f = rings.view(np.float32)
    f[1, 2, 6 + 4] = np.nan
    rings[1, 2, 2] = 1 << 4                                             # rank 1 flagged its NaN ...
    f[2, 2, 6 + 9] = -np.inf
    rings[2, 2, 2] = 1 << 9                                             # ... rank 2 its Inf
    rings[2, 3, 2] = meter.FLAG_GRAD_NORM                               # grad_norm's flag from a rank other than 0
    rings[0, 4, 2] = 0b11
    rings[1, 5, :2].view(np.int64)[0] += 1                              # one row with disagreeing stamps
    want = _run_merge(rings)
    names = [f"s{i}" for i in range(10)]
    assert want.view(np.uint32)[2, 2] == (1 << 4) | (1 << 9)
    assert np.isnan(want.view(np.float32)[2, 10]) and want.view(np.float32)[2, 15] == -np.inf
    assert want.view(np.uint32)[3, 2] == meter.FLAG_GRAD_NORM and want[4, 2] == 0b11
    assert (want[5] == meter.empty_ring(1)[0]).all()
    with pytest.raises(RuntimeError, match="overrun"):
        meter.decode_ring(want, names, 3 * rows)                        # decode_ring reports the dropped row


def test_meter_merge_refuses_more_than_64_ranks():
    from demf_amd import ops
    rings = torch.zeros((65, 2, 16), dtype=torch.int32, device="cuda")
    out = torch.full((2, 16), CANARY, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"code -3.*at most 64"):
        ops.meter_merge(rings, out)
    torch.cuda.synchronize()
    assert (out == CANARY).all()
