"""Float64 restatements of the gather / scatter / interpolation operations of csrc/group_gather.hip and the
interpolation half of csrc/three_nn_interp.hip, each written from the operation's definition in plain numpy.  No GPU,
not a test module.

Copies return the gathered values in the input's own dtype (a copy has nothing to round).  Every SUM returns a
``Sum``: per destination element the float64 value, the number of terms ``n`` that went into it and ``S = sum |term|``,
a ``prefill`` counting as one more term; ``hits`` counts the terms without the prefill, so that ``hits == 0`` marks the
elements an accumulating kernel must leave alone (and a gathering one must write as +0.0).

Pass rule of the edge tests for a sum computed in fp32 in any order, with at most two roundings per term before it is
added:  |got - value| <= (n + 2) * 2^-24 * S + 2^-126  (``Sum.bound``)."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126


class Sum(collections.namedtuple("Sum", "value n S hits")):
    def bound(self):
        return (self.n + 2) * U * self.S + TINY


def _scatter(shape, dest, terms, prefill=None):
    """value[dest] += terms over every entry (np.add.at: repeated destinations all count)."""
    terms = np.asarray(terms, F64)
    if prefill is None:
        value, n, S = np.zeros(shape, F64), np.zeros(shape, np.int64), np.zeros(shape, F64)
    else:
        value = np.array(prefill, F64).reshape(shape)
        n, S = np.ones(shape, np.int64), np.abs(value)
    hits = np.zeros(shape, np.int64)
    np.add.at(value, dest, terms)
    np.add.at(S, dest, np.abs(terms))
    np.add.at(hits, dest, 1)
    return Sum(value, n + hits, S, hits)


def _batch_of(idx):
    """-> (b, i): for every entry of idx (B, ...) its scene and its point, both flattened."""
    idx = np.asarray(idx, np.int64)
    b = np.broadcast_to(np.arange(idx.shape[0]).reshape((-1,) + (1,) * (idx.ndim - 1)), idx.shape)
    return b.reshape(-1), idx.reshape(-1)


# ---- gathers -------------------------------------------------------------------------------------------------------
def gather_rows(feat, idx):
    """Point-major: feat (B, N, C), idx (B, ...) -> (B, ..., C), out[b, e] = feat[b, idx[b, e]]."""
    b, i = _batch_of(idx)
    return feat[b, i].reshape(idx.shape + feat.shape[2:])


def gather_rows_bwd(gout, idx, N, prefill=None):
    """The transpose: gfeat (B, N, C)[b, idx[b, e]] += gout[b, e]."""
    B, C = gout.shape[0], gout.shape[-1]
    b, i = _batch_of(idx)
    return _scatter((B, N, C), (b, i), np.asarray(gout, F64).reshape(b.size, C), prefill)


def group_points(feat, idx):
    """Channel-major: feat (B, C, N), idx (B, J) -> (B, C, J), out[b, c, j] = feat[b, c, idx[b, j]]."""
    return np.ascontiguousarray(np.swapaxes(gather_rows(np.swapaxes(feat, 1, 2), idx), 1, 2))


def group_points_bwd(gout, idx, N, prefill=None):
    """gfeat (B, C, N)[b, c, idx[b, j]] += gout[b, c, j]."""
    pre = None if prefill is None else np.swapaxes(np.asarray(prefill), 1, 2)
    s = gather_rows_bwd(np.swapaxes(gout, 1, 2), idx, N, pre)
    return Sum(*[np.ascontiguousarray(np.swapaxes(a, 1, 2)) for a in s])


# ---- fused [feat | (xyz_j - center) / r | 0] rows -------------------------------------------------------------------
def group_concat(xyz, center, feat, idx, ldo, xyz_col, feat_col, radius, normalize):
    """xyz (B, N, 3), center (B, M, 3), feat (B, N, C) or None, idx (B, M, ns) -> (B, M, ns, ldo) float32.
    The coordinates are (fl32(p) - fl32(q)) / fl32(r): two IEEE single roundings, evaluated in numpy float32;
    without ``normalize`` the divisor is 1.  Every other column is +0.0."""
    B, M, ns = idx.shape
    out = np.zeros((B, M, ns, ldo), F32)
    if feat is not None and feat.shape[2] > 0:
        out[..., feat_col:feat_col + feat.shape[2]] = gather_rows(feat, idx)
    r = F32(radius) if normalize else F32(1.0)
    rel = (gather_rows(xyz.astype(F32), idx) - center.astype(F32)[:, :, None, :]) / r
    assert rel.dtype == F32
    out[..., xyz_col:xyz_col + 3] = rel
    return out


def group_concat_bwd(gout, idx, N, C, xyz_col, feat_col, radius, normalize, pre_feat=None, pre_xyz=None, pre_center=None):
    """-> (gfeat (B, N, C), gxyz (B, N, 3), gcenter (B, M, 3)) as Sums:
    gfeat[b, idx] += g[feat columns];  gxyz[b, idx] += g[xyz columns] / r;  gcenter[b, m] -= g[xyz columns] / r."""
    B, M, ns = idx.shape
    g = np.asarray(gout, F64)
    b, i = _batch_of(idx)
    gfeat = _scatter((B, N, C), (b, i), g[..., feat_col:feat_col + C].reshape(b.size, C), pre_feat)
    gx = g[..., xyz_col:xyz_col + 3] / (F64(F32(radius)) if normalize else 1.0)
    gxyz = _scatter((B, N, 3), (b, i), gx.reshape(b.size, 3), pre_xyz)
    m = np.broadcast_to(np.arange(M)[None, :, None], idx.shape).reshape(-1)
    gcenter = _scatter((B, M, 3), (b, m), -gx.reshape(b.size, 3), pre_center)
    return gfeat, gxyz, gcenter


# ---- 3-tap interpolation -------------------------------------------------------------------------------------------
def _two_sum_exact(a, b):
    """True where the float64 sum a + b carries no rounding error (Knuth's TwoSum residual is zero)."""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0


def interp3(w, f):
    """out = fma(w2, f2, fma(w0, f0, fl32(w1 * f1))) with w (..., 3) and f (..., 3, C) float32 -> (float32 (..., C),
    exact): every product of two singles is exact in float64, so each step is one float64 sum rounded ONCE to single -
    unless that float64 sum is itself inexact (double rounding possible): ``exact`` is False there and the caller
    takes the element from an fma evaluation instead."""
    w, f = np.asarray(w, F32).astype(F64)[..., None], np.asarray(f, F32).astype(F64)
    p1 = (w[..., 1, :] * f[..., 1, :]).astype(F32).astype(F64)
    a0 = w[..., 0, :] * f[..., 0, :]
    t = (a0 + p1).astype(F32).astype(F64)
    a2 = w[..., 2, :] * f[..., 2, :]
    out = (a2 + t).astype(F32)
    return out, _two_sum_exact(a0, p1) & _two_sum_exact(a2, t)


def three_interpolate_cl(feat, idx, w, skip=None):
    """Point-major: feat (B, m, C), idx (B, n, 3), w (B, n, 3) -> (out (B, n, C [+ Cs]) float32, exact (B, n, C));
    ``skip`` (B, n, Cs) is copied behind the interpolated columns."""
    out, exact = interp3(w, gather_rows(feat, idx))
    if skip is not None:
        out = np.concatenate([out, np.asarray(skip, F32)], -1)
    return out, exact


def three_interpolate_cl_bwd(gout, idx, w, m, prefill=None):
    """gfeat (B, m, C)[b, idx[b, t, k]] += gout[b, t] * w[b, t, k] for the three taps k."""
    B, n, C = gout.shape
    b, i = _batch_of(idx)                                                   # (B * n * 3,)
    terms = np.asarray(gout, F64)[:, :, None, :] * np.asarray(w, F64)[..., None]      # exact products
    return _scatter((B, m, C), (b, i), terms.reshape(b.size, C), prefill)


def three_interpolate(feat, idx, w):
    """Channel-major: feat (B, C, m) -> (out (B, C, n), exact)."""
    out, exact = three_interpolate_cl(np.swapaxes(feat, 1, 2), idx, w)
    return np.ascontiguousarray(np.swapaxes(out, 1, 2)), np.ascontiguousarray(np.swapaxes(exact, 1, 2))


def three_interpolate_bwd(gout, idx, w, m, prefill=None):
    """Channel-major: gout (B, C, n) -> Sum of (B, C, m)."""
    pre = None if prefill is None else np.swapaxes(np.asarray(prefill), 1, 2)
    s = three_interpolate_cl_bwd(np.swapaxes(gout, 1, 2), idx, w, m, pre)
    return Sum(*[np.ascontiguousarray(np.swapaxes(a, 1, 2)) for a in s])


# ---- max over the ns neighbours ------------------------------------------------------------------------------------
def maxpool_ns(x):
    """x (R, ns, C) -> (max (R, C) in x's dtype, arg (R, C) int32: the FIRST position holding the maximum)."""
    R, ns, C = x.shape
    best, arg = x[:, 0, :].copy(), np.zeros((R, C), np.int32)
    for s in range(1, ns):
        better = x[:, s, :] > best
        best = np.where(better, x[:, s, :], best)
        arg = np.where(better, np.int32(s), arg)
    return best, arg


def maxpool_ns_bwd(gout, arg, ns):
    """gx (R, ns, C): gout at the arg position, +0.0 everywhere else."""
    R, C = gout.shape
    gx = np.zeros((R, ns, C), gout.dtype)
    r, c = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
    gx[r, arg, c] = gout
    return gx


# ---- column sum ----------------------------------------------------------------------------------------------------
def colsum(x, prefill=None):
    """x (R, N) -> Sum over the rows, on top of ``prefill`` (N,)."""
    x = np.asarray(x, F64)
    R, N = x.shape
    value, S = x.sum(0), np.abs(x).sum(0)
    n = np.full(N, R, np.int64)
    if prefill is not None:
        p = np.asarray(prefill, F64)
        value, S, n = value + p, S + np.abs(p), n + 1
    return Sum(value, n, S, np.full(N, R, np.int64))


# ---- CSR inversion -------------------------------------------------------------------------------------------------
def invert_index(idx, N):
    """idx (B, E) with values in [0, N) -> (off (B, N + 1), rows (B, E)) int32: rows[b, off[b, j]:off[b, j + 1]] are
    the entry positions e with idx[b, e] == j, ascending."""
    idx = np.asarray(idx, np.int64)
    B, E = idx.shape
    off, rows = np.zeros((B, N + 1), np.int32), np.zeros((B, E), np.int32)
    for b in range(B):
        off[b, 1:] = np.cumsum(np.bincount(idx[b], minlength=N))
        rows[b] = np.argsort(idx[b], kind="stable")          # by point; equal points keep their entry order
    return off, rows


def gather_sum(gout, off, rows, C, feat_col):
    """The gather form of group_concat's feature gradient: gfeat (B, N, C)[b, j] = sum over rows[b, off[j]:off[j+1]]
    of gout (B, E, ldo)[b, e, feat_col:feat_col + C], an empty list giving +0.0.  -> Sum."""
    B, N = off.shape[0], off.shape[1] - 1
    E = rows.shape[1]
    j = np.repeat(np.arange(N)[None], B, 0)
    dest = np.stack([np.repeat(j[b], np.diff(off[b])) for b in range(B)]) if E else np.zeros((B, 0), np.int64)
    b = np.repeat(np.arange(B), E)
    src = np.asarray(gout, F64)[b, rows.reshape(-1).astype(np.int64), feat_col:feat_col + C]
    return _scatter((B, N, C), (b, dest.reshape(-1)), src)
