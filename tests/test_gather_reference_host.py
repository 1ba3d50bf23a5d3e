"""tests/gather_reference.py against independent CPU statements of the same operations: torch float64 autograd through
index_select / gather / max, explicit Python loops, and the C oracle (oracle.kernels) where it has the operation.
Shows that the reference the GPU edge tests judge by is not itself the thing that is wrong.  No GPU."""
import numpy as np
import pytest
import torch

import gather_cases as gc
import gather_reference as ref
from oracle import kernels as ok

F32, F64 = np.float32, np.float64
SHAPES = [(1, 1, 1, 1), (2, 5, 9, 3), (3, 17, 40, 8)]          # (B, N, E, C)


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, F64)).requires_grad_(grad)


def _check_sum(s, value, label):
    """The value against autograd's; n, S and hits against their definitions."""
    assert np.allclose(s.value, value, rtol=1e-13, atol=1e-13), label
    assert (s.n >= s.hits).all() and (s.S >= np.abs(s.value) - 1e-12).all(), label
    assert s.bound().shape == s.value.shape and (s.bound() > 0).all()


@pytest.mark.parametrize("B,N,E,C", SHAPES)
def test_gathers_and_their_transposes(B, N, E, C):
    rng = gc.gen("host_gather%d" % N)
    idx = gc.indices(rng, B, E, N)
    feat, gout, pre = gc.normal(rng, B, N, C), gc.normal(rng, B, E, C), gc.normal(rng, B, N, C)
    f = _t(feat, True)
    out = torch.stack([f[b].index_select(0, torch.from_numpy(idx[b]).long()) for b in range(B)])
    assert np.array_equal(ref.gather_rows(feat, idx), out.detach().numpy().astype(F32))
    out.backward(_t(gout))
    _check_sum(ref.gather_rows_bwd(gout, idx, N), f.grad.numpy(), "rows bwd")
    s = ref.gather_rows_bwd(gout, idx, N, pre)
    _check_sum(s, f.grad.numpy() + pre, "rows bwd on a prefill")
    count = np.stack([np.bincount(idx[b], minlength=N) for b in range(B)])
    assert np.array_equal(s.hits, np.broadcast_to(count[..., None], s.hits.shape))
    assert np.array_equal(s.n, s.hits + 1)
    if N >= 4:
        assert (s.hits[:, gc.unused(N)] == 0).all() and np.array_equal(s.value[:, gc.unused(N)], pre[:, gc.unused(N)].astype(F64))
    # S by an explicit loop over the entries
    S = np.abs(pre.astype(F64))
    for b in range(B):
        for e in range(E):
            S[b, idx[b, e]] += np.abs(gout[b, e].astype(F64))
    assert np.allclose(s.S, S, rtol=1e-14)
    # channel-major, against the C oracle (fp32: a copy is exact, the scatter is compared at fp32 accuracy)
    fcm, gcm = np.ascontiguousarray(feat.transpose(0, 2, 1)), np.ascontiguousarray(gout.transpose(0, 2, 1))
    assert np.array_equal(ref.group_points(fcm, idx), ok.group_points_fwd(fcm, idx[:, :, None])[..., 0])
    sc = ref.group_points_bwd(gcm, idx, N)
    assert (np.abs(ok.group_points_bwd(gcm[..., None], idx[:, :, None], N) - sc.value) <= sc.bound()).all()
    assert np.array_equal(sc.value, ref.gather_rows_bwd(gout, idx, N).value.transpose(0, 2, 1))


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("B,N,M,ns,C,ldo,xyz_col,feat_col", [(2, 9, 4, 3, 5, 11, 5, 0), (1, 6, 2, 2, 0, 4, 0, 0),
                                                              (2, 12, 3, 4, 4, 12, 0, 4)])
def test_group_concat_and_its_three_gradients(B, N, M, ns, C, ldo, xyz_col, feat_col, normalize):
    rng = gc.gen("host_concat%d" % ldo)
    idx = gc.indices(rng, B, M * ns, N).reshape(B, M, ns)
    xyz, center, feat = gc.normal(rng, B, N, 3), gc.normal(rng, B, M, 3), gc.normal(rng, B, N, C)
    gout = gc.normal(rng, B, M, ns, ldo)
    got = ref.group_concat(xyz, center, feat if C else None, idx, ldo, xyz_col, feat_col, gc.RADIUS, normalize)
    tx, tc, tf = _t(xyz, True), _t(center, True), _t(feat, True)
    r = float(F32(gc.RADIUS)) if normalize else 1.0
    li = torch.from_numpy(idx).long()
    rows = []
    for b in range(B):
        rel = (tx[b][li[b]] - tc[b][:, None, :]) / r
        cols = [torch.zeros(M, ns, 1, dtype=torch.float64) for _ in range(ldo)]
        for k in range(3):
            cols[xyz_col + k] = rel[..., k:k + 1]
        for k in range(C):
            cols[feat_col + k] = tf[b][li[b]][..., k:k + 1]
        rows.append(torch.cat(cols, -1))
    out = torch.stack(rows)
    want = out.detach().numpy()
    assert np.abs(got - want).max() <= 2 * 2.0 ** -24 * np.abs(want).max() / min(r, 1.0)
    pad = np.ones(ldo, bool)
    pad[xyz_col:xyz_col + 3] = False
    pad[feat_col:feat_col + C] = False
    assert not got[..., pad].view(np.uint32).any(), "pad columns are +0.0"
    assert np.array_equal(got[..., feat_col:feat_col + C], want[..., feat_col:feat_col + C].astype(F32))
    out.backward(_t(gout))
    gf, gx, gcn = ref.group_concat_bwd(gout, idx, N, C, xyz_col, feat_col, gc.RADIUS, normalize)
    _check_sum(gf, tf.grad.numpy() if C else np.zeros((B, N, 0)), "gfeat")
    _check_sum(gx, tx.grad.numpy(), "gxyz")
    _check_sum(gcn, tc.grad.numpy(), "gcenter")
    assert (gcn.hits == ns).all()


@pytest.mark.parametrize("B,m,n,C", [(1, 1, 1, 1), (2, 3, 7, 5), (2, 40, 33, 9)])
def test_interpolation_and_its_transpose(B, m, n, C):
    rng = gc.gen("host_interp%d" % m)
    idx, w = gc.triplets(rng, B, n, m)
    feat, gout = gc.normal(rng, B, m, C), gc.normal(rng, B, n, C)
    out, exact = ref.three_interpolate_cl(feat, idx, w)
    fcm = np.ascontiguousarray(feat.transpose(0, 2, 1))
    oracle = ok.three_interpolate_fwd(fcm, idx, w).transpose(0, 2, 1)           # the C oracle evaluates the same fma chain
    assert exact.mean() > 0.5 and np.array_equal(out[exact].view(np.uint32), oracle[exact].view(np.uint32))
    out_cm, exact_cm = ref.three_interpolate(fcm, idx, w)
    assert np.array_equal(out_cm, out.transpose(0, 2, 1)) and np.array_equal(exact_cm, exact.transpose(0, 2, 1))
    f = _t(feat, True)
    li = torch.from_numpy(idx).long()
    o = torch.stack([(f[b][li[b]] * _t(w[b])[..., None]).sum(1) for b in range(B)])
    assert np.abs(out - o.detach().numpy()).max() <= 4 * 2.0 ** -24 * np.abs(feat).max()
    o.backward(_t(gout))
    s = ref.three_interpolate_cl_bwd(gout, idx, w, m)
    _check_sum(s, f.grad.numpy(), "interp bwd")
    assert s.hits.sum() == 3 * B * n * C
    gcm = np.ascontiguousarray(gout.transpose(0, 2, 1))
    scm = ref.three_interpolate_bwd(gcm, idx, w, m)
    assert np.array_equal(scm.value, s.value.transpose(0, 2, 1))
    assert (np.abs(ok.three_interpolate_bwd(gcm, idx, w, m) - scm.value) <= scm.bound()).all()
    skip = gc.normal(rng, B, n, 4)
    cat, _ = ref.three_interpolate_cl(feat, idx, w, skip)
    assert np.array_equal(cat[..., :C], out) and np.array_equal(cat[..., C:], skip)


def test_interp3_flags_an_inexact_float64_sum():
    w = np.array([[1.0, 1.0, 0.0]], F32)
    f = np.array([[[2.0 ** 60], [1.0 + 2.0 ** -23], [0.0]]], F32)            # 2^60 + (1 + 2^-23): 84 bits apart
    out, exact = ref.interp3(w, f)
    assert not exact.any() and out[0, 0] == F32(2.0 ** 60)
    out, exact = ref.interp3(w, np.array([[[1.5], [0.25], [3.0]]], F32))
    assert exact.all() and out[0, 0] == F32(1.75)


@pytest.mark.parametrize("R,ns,C", [(1, 1, 1), (4, 2, 3), (5, 16, 7)])
def test_maxpool_first_maximum_and_its_scatter(R, ns, C):
    x = gc.maxpool_input("host", R, ns, C)
    best, arg = ref.maxpool_ns(x)
    tv, ti = torch.from_numpy(x).double().max(1)
    assert np.array_equal(best, tv.numpy().astype(F32))
    for r in range(R):                       # first maximum, by a loop (torch.max does not promise which one)
        for c in range(C):
            col = list(x[r, :, c])
            assert arg[r, c] == col.index(max(col)) and best[r, c] == max(col)
    gout = gc.normal(gc.gen("host_pool"), R, C)
    gx = ref.maxpool_ns_bwd(gout, arg, ns)
    assert np.array_equal(gx.sum(1), gout) and np.count_nonzero(gx) <= R * C
    xt = torch.from_numpy(np.where(np.isfinite(x), x, 0)).double().requires_grad_()
    # autograd of gather at the reference's arg positions
    xt.gather(1, torch.from_numpy(arg).long()[:, None, :]).backward(_t(gout)[:, None, :])
    assert np.array_equal(gx, xt.grad.numpy().astype(F32))


@pytest.mark.parametrize("R,N", [(1, 1), (7, 5), (130, 33)])
def test_colsum(R, N):
    rng = gc.gen("host_colsum%d" % R)
    x, pre = gc.normal(rng, R, N), gc.normal(rng, N)
    s = ref.colsum(x, pre)
    _check_sum(s, torch.from_numpy(x).double().sum(0).numpy() + pre, "colsum")
    assert (s.n == R + 1).all() and np.allclose(s.S, np.abs(x.astype(F64)).sum(0) + np.abs(pre))
    assert (ref.colsum(x).n == R).all()


@pytest.mark.parametrize("B,N,E", [(1, 1, 1), (2, 5, 0), (2, 9, 40), (3, 64, 500)])
def test_invert_index_and_the_gather_sum(B, N, E):
    rng = gc.gen("host_invert%d" % N)
    idx = gc.indices(rng, B, E, N)
    off, rows = ref.invert_index(idx, N)
    for b in range(B):
        lists = [[e for e in range(E) if idx[b, e] == j] for j in range(N)]     # ascending by construction
        assert off[b, 0] == 0 and off[b, N] == E
        for j in range(N):
            assert list(rows[b, off[b, j]:off[b, j + 1]]) == lists[j]
    C, ldo, col = 4, 12, 4
    gout = gc.normal(rng, B, E, ldo)
    s = ref.gather_sum(gout, off, rows, C, col)
    t = ref.gather_rows_bwd(gout[..., col:col + C], idx, N)
    assert np.allclose(s.value, t.value, rtol=1e-14, atol=1e-14) and np.array_equal(s.n, t.n) and np.allclose(s.S, t.S)
    assert not s.value[s.hits == 0].view(np.uint64).any()


def test_case_index_sets_hold_what_they_promise():
    for B, E, N in [(2, 15, 29), (2, 70, 40), (2, 257, 37)]:
        idx = gc.indices(gc.gen("host_sets"), B, E, N)
        for b in range(B):
            assert {0, N - 1} <= set(idx[b]) and gc.unused(N) not in set(idx[b])
            assert np.count_nonzero(idx[b] == gc.hot(N)) >= E // 3
        assert (gc.indices(gc.gen("x"), B, E, N, same=True) == gc.hot(N)).all()
    idx = gc.list_indices(gc.gen("host_lists"), 2, 40, 70, "lengths")
    for b in range(2):
        assert tuple(np.bincount(idx[b], minlength=40)[1:8]) == gc.LIST_LENGTHS
    for form, shapes in gc.INVERT.items():
        for N, E in shapes:
            assert gc.fits_lds(N, E) == (form == "lds"), (form, N, E)


def test_grid_stride_cases_pass_the_grid_caps():
    """Every "2nd_trip" case has more rows (points, elements) than one pass of its capped grid covers."""
    rows = lambda c: c["B"] * c["M"] * c["ns"]
    assert rows(gc.GROUP_CONCAT_FWD["thin_2nd_trip"][0]) > gc.GRID_ELEMS
    for table in (gc.GROUP_CONCAT_FWD, gc.GROUP_CONCAT_BWD):
        for name in ("vec4_2nd_trip", "scalar_2nd_trip"):
            assert gc.GRID_ELEMS > rows(table[name][0]) > gc.GRID_ROWS
    c = gc.GATHER_ROWS["2nd_trip"][0]
    assert c["B"] * c["M"] > gc.GRID_ROWS
    c = gc.INTERP_CL["2nd_trip"][0]
    assert c["B"] * c["n"] > gc.GRID_ROWS
    c = gc.MAXPOOL["2nd_trip"][0]
    assert c["R"] * c["C"] > gc.GRID_ELEMS and c["ns"] == 2
    for name, lpr in (("C4_2nd_trip", 16), ("C128_2nd_trip", 32), ("C256_2nd_trip", 64)):
        c = gc.BWD_GATHER[name][0]
        assert lpr == (64 if c["C"] >= 256 else 32 if c["C"] >= 128 else 16)
        assert c["B"] * c["N"] > gc.GRID_ROWS * 64 // lpr and c["N"] <= 16384
