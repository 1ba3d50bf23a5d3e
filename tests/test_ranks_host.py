"""The host side of the multi-rank layer: pipeline.shard_chunks (against its rules and the restatement in
ranks_reference.py), the reference functions themselves on hand-made cases, ranks.launch_command, the ``world`` rule
of a checkpoint's meta, and autoscale_lr with ranks.  No GPU."""
import sys

import numpy as np
import pytest

import ranks_reference as rref


def _today(order, bs, drop_last):
    """SceneLoader.__iter__'s chunking before ranks existed, verbatim."""
    chunks = [order[i:i + bs] for i in range(0, len(order), bs)]
    if drop_last and chunks and len(chunks[-1]) < bs:
        chunks.pop()
    return chunks


def _lists(chunks):
    return [[int(i) for i in c] for c in chunks]


# ---- shard_chunks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 8])
@pytest.mark.parametrize("bs", [1, 2, 3])
@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("drop_last", [False, True])
def test_one_rank_is_todays_chunking(n, bs, mode, drop_last):
    from demf_amd.pipeline import shard_chunks
    order = np.random.default_rng([3, n]).permutation(n) if mode == "train" else np.arange(n)
    got = shard_chunks(order, bs, 0, 1, mode, drop_last)
    assert _lists(got) == _lists(_today(order, bs, drop_last))
    assert _lists(got) == rref.shard_chunks(order, bs, 0, 1, mode, drop_last)
    assert all(isinstance(c, np.ndarray) for c in got)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 7, 8, 24, 50])
@pytest.mark.parametrize("bs", [1, 2, 3])
def test_train_shards(world, n, bs):
    from demf_amd.pipeline import shard_chunks
    order = np.random.default_rng([5, n]).permutation(n)
    single = _lists(_today(order, bs, False))
    per_rank = [_lists(shard_chunks(order, bs, r, world, "train", False)) for r in range(world)]
    want_len = -(-n // (world * bs))
    assert all(len(c) == want_len for c in per_rank)                     # the same number of chunks ...
    assert all(len(b) == bs for c in per_rank for b in c)                # ... every one full
    assert {i for c in per_rank for b in c for i in b} == set(range(n))  # every scene is seen
    for r, chunks in enumerate(per_rank):
        assert chunks == rref.shard_chunks(order, bs, r, world, "train", False)
        for j, c in enumerate(chunks):
            k = j * world + r
            if k < len(single) and len(single[k]) == bs:                 # chunk j of rank r = single-process chunk jW+r
                assert c == single[k]
    # optimizer step j of the W ranks = group j of a single process with accumulate = W, where that group is whole
    for j in range(n // (world * bs)):
        assert [per_rank[r][j] for r in range(world)] == single[j * world:(j + 1) * world]
    # the padding is the order's own head, wrapped around as often as it takes (n < W * B)
    flat = [i for j in range(want_len) for r in range(world) for i in per_rank[r][j]]
    assert flat == [int(order[k % n]) for k in range(want_len * world * bs)]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("n", [0, 5, 24, 50])
def test_train_shards_drop_last(world, n):
    from demf_amd.pipeline import shard_chunks
    bs = 2
    order = np.random.default_rng([6, n]).permutation(n)
    single = _lists(_today(order, bs, True))
    per_rank = [_lists(shard_chunks(order, bs, r, world, "train", True)) for r in range(world)]
    steps = n // (world * bs)
    assert all(len(c) == steps for c in per_rank)
    for r in range(world):
        assert per_rank[r] == [single[j * world + r] for j in range(steps)]
        assert per_rank[r] == rref.shard_chunks(order, bs, r, world, "train", True)


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 50])
@pytest.mark.parametrize("bs", [1, 3])
def test_test_shards_are_contiguous(world, n, bs):
    from demf_amd.pipeline import shard_chunks
    per_rank = [_lists(shard_chunks(np.arange(n), bs, r, world, "test", False)) for r in range(world)]
    q = -(-n // world)
    flat = []
    for r, chunks in enumerate(per_rank):
        mine = [i for c in chunks for i in c]
        assert mine == list(range(min(n, r * q), min(n, (r + 1) * q)))   # contiguous, in order, ranks in order
        assert all(len(c) == bs for c in chunks[:-1]) and all(1 <= len(c) <= bs for c in chunks)
        assert chunks == rref.shard_chunks(np.arange(n), bs, r, world, "test", False)
        flat += mine
    assert flat == list(range(n))                                        # disjoint and covering
    if n < world:
        assert sum(1 for c in per_rank if not c) == world - n            # empty shards


def test_shard_chunks_refuses_bad_arguments():
    from demf_amd.pipeline import shard_chunks
    for kw in (dict(rank=2, world=2), dict(rank=-1, world=2), dict(rank=0, world=0)):
        with pytest.raises(ValueError):
            shard_chunks(np.arange(4), 2, mode="train", **kw)
    with pytest.raises(ValueError):
        shard_chunks(np.arange(4), 0)
    with pytest.raises(ValueError):
        shard_chunks(np.arange(4), 2, 0, 2, "val")


class _Len:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_loader_len_counts_the_ranks_batches(monkeypatch):
    """len(loader) under ranks: ceil(n / (W * B)) full batches in train mode, the shard's batches in test mode."""
    from demf_amd import pipeline as pl
    monkeypatch.setattr(pl.torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(pl, "ScenePipeline", lambda *a, **k: None)
    mk = lambda n, bs, mode, **kw: pl.SceneLoader(_Len(n), bs, mode, **kw)    # noqa: E731
    assert len(mk(50, 4, "train")) == 13 and len(mk(50, 4, "train", drop_last=True)) == 12
    assert [len(mk(50, 4, "train", rank=r, world=3)) for r in range(3)] == [5, 5, 5]
    assert [len(mk(50, 4, "train", rank=r, world=3, drop_last=True)) for r in range(3)] == [4, 4, 4]
    assert [len(mk(9, 2, "test", rank=r, world=4)) for r in range(4)] == [2, 2, 2, 0]
    with pytest.raises(ValueError):
        mk(9, 2, "test", rank=4, world=4)


# ---- the reference functions on hand-made cases ---------------------------------------------------------------------
def _dst(scenes, rows, fill=-7):
    return dict(scene_off=np.full(scenes + 1, fill, np.int32), state=np.full(2, fill, np.int32),
                boxes=np.full((rows, 7), fill, np.float32), scores=np.full(rows, fill, np.float32),
                labels=np.full(rows, fill, np.int32))


def test_reference_store_concat_by_hand():
    # rank 0: 2 scenes of 1 and 2 rows; rank 1: none; rank 2: 1 scene of 1 row.  S = 2, R = 3.
    off = np.array([[0, 1, 3], [0, 0, 0], [0, 1, 99]], np.int32)
    state = np.array([[3, 0], [0, 0], [1, 0]], np.int32)
    boxes = np.arange(3 * 3 * 7, dtype=np.float32).reshape(3, 3, 7)
    scores = np.arange(9, dtype=np.float32).reshape(3, 3) + 0.5
    labels = np.arange(9, dtype=np.int32).reshape(3, 3) + 100
    out = rref.store_concat([2, 0, 1], off, state, boxes, scores, labels, _dst(4, 6))
    assert out["scene_off"].tolist() == [0, 1, 3, 4, -7] and out["state"].tolist() == [4, 0]
    assert out["scores"].tolist() == [0.5, 1.5, 2.5, 6.5, -7, -7] and out["labels"].tolist() == [100, 101, 102, 106, -7, -7]
    assert (out["boxes"][3] == boxes[2, 0]).all() and (out["boxes"][:3] == boxes[0]).all() and (out["boxes"][4:] == -7).all()
    # a destination one row too small: counted, not written, overflow word set
    small = rref.store_concat([2, 0, 1], off, state, boxes, scores, labels, _dst(4, 3))
    assert small["state"].tolist() == [4, 1] and small["scene_off"].tolist() == [0, 1, 3, 4, -7]
    assert small["scores"].tolist() == [0.5, 1.5, 2.5]
    # a rank that overflowed: its cursor is past R, only R rows exist; the rows behind keep their place
    off2 = off.copy()
    off2[0] = [0, 1, 5]
    state2 = state.copy()
    state2[0] = [5, 1]
    over = rref.store_concat([2, 0, 1], off2, state2, boxes, scores, labels, _dst(4, 8))
    assert over["scene_off"].tolist() == [0, 1, 5, 6, -7] and over["state"].tolist() == [6, 1]
    assert over["scores"].tolist() == [0.5, 1.5, 2.5, -7, -7, 6.5, -7, -7]


def test_reference_meter_merge_by_hand():
    from demf_amd import meter
    rings = np.stack([meter.empty_ring(3) for _ in range(2)])
    f = rings.view(np.float32)
    for r in range(2):
        rings[r, 1, :2].view(np.int64)[0] = 7                       # row 1: step 7 on both ranks
        rings[r, 2, :2].view(np.int64)[0] = 8 + r                   # row 2: the ranks disagree
        f[r, 1, 3:6] = (0.1, 2.5, 1.0)
        f[r, 1, 6:9] = (1.0 + r, np.float32(0.1) if r == 0 else np.float32(0.2), 3.0)
    rings[1, 1, 2] = 0b100 | meter.FLAG_GRAD_NORM
    rings[0, 1, 2] = 0b001
    f[1, 1, 8] = np.inf
    out = rref.meter_merge(rings)
    assert (out[0] == meter.empty_ring(1)[0]).all() and (out[2] == meter.empty_ring(1)[0]).all()
    rows, nxt = meter.decode_ring(out[1:2], ("a", "b", "c"), 7)
    assert nxt == 8 and rows[0]["t"] == 7 and rows[0]["a"] == 1.5 and rows[0]["c"] == np.inf
    assert rows[0]["b"] == float(np.float32((np.float64(np.float32(0.1)) + np.float64(np.float32(0.2))) / 2))
    assert rows[0]["nonfinite"] == ("a", "c", "grad_norm") and rows[0]["grad_norm"] == 2.5
    assert (rref.meter_merge(rings[:1]) == rings[0]).all()          # W = 1: a copy
    # once a later step (9, row 0) has arrived, the row the ranks disagreed on (step 8) is reported as missing
    for r in range(2):
        rings[r, 0, :2].view(np.int64)[0] = 9
    with pytest.raises(RuntimeError, match="overrun: step 8 was expected in row 2, which holds step -1"):
        meter.decode_ring(rref.meter_merge(rings), ("a", "b", "c"), 7)


# ---- launcher, meta, lr ---------------------------------------------------------------------------------------------
def test_launch_command():
    from demf_amd import ranks
    cmd = ranks.launch_command("demf_amd.train", ["--data-root", "R", "--gpus", 8], 8, port=29511)
    assert cmd == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                   "--master-addr", "127.0.0.1", "--master-port", "29511", "-m", "demf_amd.train",
                   "--data-root", "R", "--gpus", "8"]
    assert "--master-port" not in ranks.launch_command("demf_amd.infer", [], 2)
    with pytest.raises(ValueError):
        ranks.launch_command("demf_amd.infer", [], 0)


def test_no_process_group_is_one_rank():
    from demf_amd import ranks
    assert (ranks.world(), ranks.rank()) == (1, 0)
    assert ranks.broadcast_object(dict(a=1)) == dict(a=1)
    ranks.barrier()


def test_world_meta_rule():
    from demf_amd import train
    assert train.check_resume_world({}, 1) == 1                     # absent reads as 1
    assert train.check_resume_world(dict(world=2), 2) == 2
    with pytest.raises(ValueError, match="world = 2 ranks, this run has world = 1"):
        train.check_resume_world(dict(world=2), 1, "x.pth")
    with pytest.raises(ValueError, match="world = 1 ranks, this run has world = 8"):
        train.check_resume_world(dict(accumulate=1), 8)


def test_autoscale_lr_with_ranks():
    from demf_amd import train
    assert train.autoscale_lr(0.008, 1, 8) == 0.008
    assert train.autoscale_lr(0.008, 2, 4) == 0.008
    assert train.autoscale_lr(0.008, 1, 2) == 0.002


def test_gpus_option_is_parsed():
    from demf_amd import infer, train
    a = train.parse_args(["--data-root", "R", "--ann-file", "a.pkl", "--work-dir", "W", "--gpus", "8"])
    assert a.gpus == 8 and train.parse_args(["--data-root", "R", "--ann-file", "a.pkl", "--work-dir", "W"]).gpus is None
    b = infer.parse_args(["--data-root", "R", "--ann-file", "a.pkl", "--checkpoint", "C", "--gpus", "2"])
    assert b.gpus == 2
    with pytest.raises(SystemExit):
        infer.parse_args(["--data-root", "R", "--ann-file", "a.pkl", "--checkpoint", "C", "--gpus", "0"])
