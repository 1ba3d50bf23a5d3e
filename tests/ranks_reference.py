"""numpy restatement of csrc/ranks.hip (demf_store_concat, demf_meter_merge; the mean in fp64) and of
pipeline.shard_chunks, written from their specifications (include/demf_hip.h) with plain loops."""
import numpy as np

ROW_WORDS, HEAD_WORDS = 16, 6


def shard_chunks(order, batch_size, rank, world, mode, drop_last):
    """-> list of index lists."""
    order = [int(i) for i in order]
    n, B, W = len(order), int(batch_size), int(world)
    if W == 1:
        chunks = [order[i:i + B] for i in range(0, n, B)]
        if drop_last and chunks and len(chunks[-1]) < B:
            chunks.pop()
        return chunks
    if mode == "train":
        if n == 0:
            return []
        ext = list(order)
        if drop_last:
            ext = ext[:n - n % (W * B)]
        else:
            k = 0
            while len(ext) % (W * B):
                ext.append(order[k % n])               # wrap-around
                k += 1
        chunks = [ext[i:i + B] for i in range(0, len(ext), B)]
        return [c for j, c in enumerate(chunks) if j % W == int(rank)]
    q = (n + W - 1) // W
    mine = order[int(rank) * q:min(n, (int(rank) + 1) * q)]
    chunks = [mine[i:i + B] for i in range(0, len(mine), B)]
    if drop_last and chunks and len(chunks[-1]) < B:
        chunks.pop()
    return chunks


def store_concat(counts, scene_off, state, boxes, scores, labels, dst):
    """``dst``: dict(scene_off (S'+1,), state (2,), boxes (R',7), scores (R',), labels (R',)) of numpy arrays holding
    the destination's PREVIOUS contents -> a dict of new arrays: what the kernel leaves there.  Rows are moved as
    raw 32-bit words."""
    W = len(counts)
    out = {k: v.copy() for k, v in dst.items()}
    max_rows = out["scores"].shape[0]
    R = scores.shape[1]
    b32 = lambda a: a.view(np.uint32)                   # noqa: E731
    base, first, over = 0, 0, 0
    for r in range(W):
        n = int(counts[r])
        rows = max(int(scene_off[r, n]), 0)
        over |= int(state[r, 1] != 0)
        for i in range(n):
            out["scene_off"][first + i] = np.int64(base + int(scene_off[r, i])).astype(np.int32)
        for j in range(min(rows, R)):
            if base + j < max_rows:
                b32(out["boxes"])[base + j] = b32(boxes)[r, j]
                b32(out["scores"])[base + j] = b32(scores)[r, j]
                b32(out["labels"])[base + j] = b32(labels)[r, j]
        base += rows
        first += n
    out["scene_off"][first] = np.int64(base).astype(np.int32)
    out["state"][0] = np.int64(base).astype(np.int32)
    out["state"][1] = 1 if (over or base > max_rows) else 0
    return out


def meter_merge(rings):
    """(W, rows, 16) int32 -> (rows, 16) int32."""
    rings = np.ascontiguousarray(rings, dtype=np.int32)
    W, rows, _ = rings.shape
    if W == 1:
        return rings[0].copy()
    out = np.zeros((rows, ROW_WORDS), np.int32)
    u = rings.view(np.uint32)
    f = rings.view(np.float32)
    stamps = rings[:, :, :2].copy().view(np.int64)[:, :, 0]
    for i in range(rows):
        if not (stamps[:, i] == stamps[0, i]).all():
            out[i, :2] = -1
            continue
        out[i, :2] = rings[0, i, :2]
        out.view(np.uint32)[i, 2] = np.bitwise_or.reduce(u[:, i, 2])
        out[i, 3:HEAD_WORDS] = rings[0, i, 3:HEAD_WORDS]
        for w in range(HEAD_WORDS, ROW_WORDS):
            s = np.float64(0.0)
            with np.errstate(all="ignore"):
                for r in range(W):
                    s = s + np.float64(f[r, i, w])
                out.view(np.float32)[i, w] = np.float32(s / np.float64(W))
    return out
