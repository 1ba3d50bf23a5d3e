"""Shapes and inputs of the gather / scatter edge tests (tests/test_gpu_gather_edges.py), each the smallest that reaches
its dispatch branch, with the reason it is there.  Not a test module.  Everything is built on the CPU from seeded
generators, so the GPU test and the float64 reference see identical numbers.

Launch geometry the shapes are chosen against (csrc/group_gather.hip, csrc/three_nn_interp.hip):
  channel-major kernels   8 channels per thread, 256 entries per block
  wave-per-row kernels    4 rows per block, at most 4096 blocks: the grid-stride loop's second trip starts above
                          16 384 rows
  thread-per-element      256 per block, at most 4096 blocks: second trip above 1 048 576 elements
  bwd_gather              LPR = 16 / 32 / 64 lanes per point for C < 128 / < 256 / >= 256: second trip above
                          65 536 / 32 768 / 16 384 points
"""
import numpy as np

F32 = np.float32
SENTINEL = F32(-7777.25)
RADIUS = 0.3            # not a power of two: the division rounds
GRID_ROWS = 16384       # wave-per-row kernels
GRID_ELEMS = 1048576    # thread-per-element kernels
LDS_LIMIT = 150 * 1024  # invert_index keeps its lists in LDS while 4 * (2N + 1 + E) fits


def gen(name):
    """A generator seeded by a case name (its bytes: independent of the interpreter's string hashing)."""
    return np.random.default_rng(list(name.encode()))


def normal(rng, *shape):
    return rng.standard_normal(shape).astype(F32)


def indices(rng, B, E, N, same=False):
    """(B, E) int32 in [0, N).  Where the sizes allow: entries 0 and N - 1 are present, point ``unused(N)`` is never
    referenced, point ``hot(N)`` holds every third entry.  ``same``: every entry is ``hot(N)``."""
    if same or N == 1:
        return np.full((B, E), hot(N), np.int32)
    idx = rng.integers(0, N, (B, E))
    if N >= 4:
        idx[idx == unused(N)] = hot(N)
    idx[:, 2::3] = hot(N)
    if E >= 2:
        idx[:, 0], idx[:, 1] = 0, N - 1
        if B > 1:
            idx[1, 0], idx[1, 1] = N - 1, 0
    return idx.astype(np.int32)


def hot(N):
    return N // 3


def unused(N):
    return (2 * N) // 3


def triplets(rng, B, n, m):
    """idx (B, n, 3) and weights (B, n, 3) of an interpolation: the three_nn shape (three distinct sources, positive
    weights summing to one) for most targets; every 5th target has i0 = i1 = i2 (three atomics on one address), every
    7th a zero weight.  Source ``unused(m)`` is never referenced where m allows."""
    idx = indices(rng, B, n * 3, m).reshape(B, n, 3)
    idx[:, ::5, 1] = idx[:, ::5, 0]
    idx[:, ::5, 2] = idx[:, ::5, 0]
    w = rng.uniform(0.05, 1.0, (B, n, 3))
    w = (w / w.sum(-1, keepdims=True)).astype(F32)
    w[:, ::7, 1] = 0.0
    return idx, w


# ---- channel-major group / gather / interpolate: (C, J or n) ---------------------------------------------------------
CM_C = (1, 7, 8, 9, 131)            # one thread's 8 channels: a partial group, exactly one, one and a bit, 17 groups
CM_J = (1, 255, 256, 257)           # one block of 256 entries: a single one, one short, exactly, one over
CM_N = 37                           # source points

# ---- group_concat_cl_fwd -------------------------------------------------------------------------------------------
# name -> dict(B, N, M, ns, C, ldo, xyz_col, feat_col, out_shift, feat_shift, normalize), and why
_GC = dict(B=2, N=29, M=5, ns=3, xyz_col=None, feat_col=0, out_shift=0, feat_shift=0, normalize=1, same=False)


def _gc(**kw):
    d = dict(_GC, **kw)
    if d["xyz_col"] is None:
        d["xyz_col"] = d["feat_col"] + d["C"]
    return d


GROUP_CONCAT_FWD = {
    # thin form: one thread per row, ldo <= 8
    "thin_ld3_C0": (_gc(C=0, ldo=3), "coordinates alone, scalar stores"),
    "thin_ld4_C1": (_gc(C=1, ldo=4), "the SA1 row: one float4 store"),
    "thin_ld4_C1_xyz_first": (_gc(C=1, ldo=4, xyz_col=0, feat_col=3), "columns in the other order: feat_col = 3"),
    "thin_ld5_C2": (_gc(C=2, ldo=5), "odd pitch, scalar stores"),
    "thin_ld7_C3_pad": (_gc(C=3, ldo=7), "one pad column inside the row"),
    "thin_ld8_C4_pad": (_gc(C=4, ldo=8), "two float4 stores, one pad column"),
    "thin_ld8_C5_xyz_first": (_gc(C=5, ldo=8, xyz_col=0, feat_col=3), "full row, columns in the other order"),
    "thin_ld4_raw": (_gc(C=1, ldo=4, normalize=0), "normalize_xyz = 0: the divisor is 1"),
    "thin_ld4_same": (_gc(C=1, ldo=4, same=True), "every entry the same index"),
    "thin_ld4_out_off4": (_gc(C=1, ldo=4, out_shift=1), "out 4 bytes off: float4 stores impossible, the wave kernel"),
    "thin_ld8_out_off4": (_gc(C=4, ldo=8, out_shift=1), "out 4 bytes off at ldo = 8"),
    "thin_2nd_trip": (_gc(N=100, M=8200, ns=64, C=1, ldo=4), "1 049 600 rows: the thread-per-row loop's second trip"),
    # wave form, float4
    "vec4_C4": (_gc(C=4, ldo=12), "one lane copies, ldo > 8"),
    "vec4_C64": (_gc(C=64, ldo=68), "16 lanes"),
    "vec4_C256": (_gc(C=256, ldo=260), "every lane once"),
    "vec4_C260": (_gc(C=260, ldo=264), "second trip of the c += 256 loop"),
    "vec4_C64_col4": (_gc(C=64, ldo=72, xyz_col=0, feat_col=4), "feat_col = 4, a pad column at 3 and at 68.."),
    "vec4_C260_col4": (_gc(C=260, ldo=264, xyz_col=0, feat_col=4), "feat_col = 4 with the second trip, pad column 3"),
    "vec4_raw": (_gc(C=64, ldo=68, normalize=0), "normalize_xyz = 0"),
    "vec4_same": (_gc(C=64, ldo=68, same=True), "every entry the same index"),
    "vec4_2nd_trip": (_gc(N=50, M=130, ns=64, C=8, ldo=12), "16 640 rows: beyond the grid cap"),
    # wave form, scalar: each reason in turn
    "scalar_C5": (_gc(C=5, ldo=12), "C % 4 != 0"),
    "scalar_C131": (_gc(C=131, ldo=136), "C % 4 != 0, three trips of the c += 64 loop"),
    "scalar_ld11": (_gc(C=8, ldo=11), "ldo % 4 != 0"),
    "scalar_col3": (_gc(C=8, ldo=12, xyz_col=0, feat_col=3), "feat_col % 4 != 0"),
    "scalar_feat_off4": (_gc(C=8, ldo=12, feat_shift=1), "feat 4 bytes off"),
    "scalar_2nd_trip": (_gc(N=50, M=130, ns=64, C=5, ldo=9), "16 640 rows in the scalar form"),
}

# ---- group_concat_cl_bwd: shape as above + which gradients are asked for ---------------------------------------------
GROUP_CONCAT_BWD = {
    "vec4_C4": (_gc(C=4, ldo=12), "float4 loads, one lane"),
    "vec4_C64": (_gc(C=64, ldo=68), "16 lanes"),
    "vec4_C256": (_gc(C=256, ldo=260), "every lane once"),
    "vec4_C260_col4": (_gc(C=260, ldo=264, xyz_col=0, feat_col=4), "second trip of c += 256, feat_col = 4"),
    "scalar_C5": (_gc(C=5, ldo=12), "C % 4 != 0"),
    "scalar_C131": (_gc(C=131, ldo=136), "three trips of c += 64"),
    "scalar_ld11": (_gc(C=8, ldo=11), "ldo % 4 != 0"),
    "scalar_col3": (_gc(C=8, ldo=12, xyz_col=0, feat_col=3), "feat_col % 4 != 0"),
    "scalar_gout_off4": (_gc(C=8, ldo=12, out_shift=1), "grad_out 4 bytes off"),
    "C0_xyz": (_gc(C=0, ldo=4), "coordinate gradients alone"),
    "raw": (_gc(C=8, ldo=12, normalize=0), "normalize_xyz = 0: no 1/r"),
    "same": (_gc(C=8, ldo=12, same=True), "every entry the same index: all atomics of a scene on one row"),
    "vec4_2nd_trip": (_gc(N=50, M=130, ns=64, C=8, ldo=12), "16 640 rows: beyond the grid cap"),
    "scalar_2nd_trip": (_gc(N=50, M=130, ns=64, C=5, ldo=9), "16 640 rows in the scalar form"),
}
GROUP_CONCAT_BWD_FORMS = ("feat_and_xyz", "feat_only", "xyz_only", "neither")

# ---- group_concat_cl_bwd_gather: (B, N, E, C, ldo, feat_col, lists) --------------------------------------------------
# lists: "lengths" = points with 0, 1, 3, 4, 5, 7, 8 entries (each side of the 4-way unroll) plus the usual index set;
#        "same" = one list of length E; "sparse" = a small E over many points (grid-stride cases);
#        "lds" / "global" / "split" = off and rows come from demf_invert_index[_ws] in that form, on the GPU
BWD_GATHER = {
    "C4": (dict(B=2, N=40, E=70, C=4, ldo=4, feat_col=0, lists="lengths"), "LPR 16, one lane per point"),
    "C64": (dict(B=2, N=40, E=70, C=64, ldo=68, feat_col=0, lists="lengths"), "LPR 16, every lane, ldo > C"),
    "C124_col4": (dict(B=2, N=40, E=70, C=124, ldo=128, feat_col=4, lists="lengths"), "LPR 16, two trips, feat_col 4"),
    "C128": (dict(B=2, N=40, E=70, C=128, ldo=132, feat_col=0, lists="lengths"), "LPR 32, every lane once"),
    "C252_col4": (dict(B=2, N=40, E=70, C=252, ldo=256, feat_col=4, lists="lengths"), "LPR 32, two trips"),
    "C256": (dict(B=2, N=40, E=70, C=256, ldo=260, feat_col=0, lists="lengths"), "LPR 64, every lane once"),
    "C260_col4": (dict(B=2, N=40, E=70, C=260, ldo=264, feat_col=4, lists="lengths"), "LPR 64, second trip of one lane"),
    "C512": (dict(B=2, N=40, E=70, C=512, ldo=512, feat_col=0, lists="lengths"), "LPR 64, two full trips"),
    "C64_same": (dict(B=2, N=40, E=70, C=64, ldo=68, feat_col=0, lists="same"), "one list of length E, all others empty"),
    "C256_same": (dict(B=2, N=40, E=70, C=256, ldo=260, feat_col=0, lists="same"), "the same at LPR 64"),
    "C4_2nd_trip": (dict(B=5, N=16384, E=64, C=4, ldo=4, feat_col=0, lists="sparse"), "81 920 points at LPR 16"),
    "C128_2nd_trip": (dict(B=3, N=16384, E=64, C=128, ldo=128, feat_col=0, lists="sparse"), "49 152 points at LPR 32"),
    "C256_2nd_trip": (dict(B=2, N=16384, E=64, C=256, ldo=256, feat_col=0, lists="sparse"), "32 768 points at LPR 64"),
    "from_lds_lists": (dict(B=2, N=1025, E=3000, C=8, ldo=12, feat_col=4, lists="lds"), "lists inverted on the GPU, LDS form"),
    "from_global_lists": (dict(B=2, N=12000, E=30000, C=4, ldo=8, feat_col=4, lists="global"), "global-list form"),
    "from_split_lists": (dict(B=2, N=12000, E=30000, C=4, ldo=8, feat_col=4, lists="split"), "five-launch form"),
}
LIST_LENGTHS = (0, 1, 3, 4, 5, 7, 8)


def list_indices(rng, B, N, E, lists):
    if lists == "same":
        return indices(rng, B, E, N, same=True)
    if lists in INVERT:
        return invert_indices(lists, N, E, B)
    if lists != "lengths":
        return indices(rng, B, E, N)
    # points 1..7 hold exactly LIST_LENGTHS entries (point 1 none); the rest is the usual set over the other points
    fixed = np.concatenate([np.full(L, 1 + k) for k, L in enumerate(LIST_LENGTHS)])
    rest = indices(rng, B, E - fixed.size, N - 8) + 8
    rest[:, 3] = 0
    idx = np.concatenate([np.broadcast_to(fixed, (B, fixed.size)), rest], 1)
    for b in range(B):
        idx[b] = idx[b, rng.permutation(E)]
    return idx.astype(np.int32)


# ---- gather_rows_cl ------------------------------------------------------------------------------------------------
GATHER_ROWS_C = (1, 63, 64, 65, 131, 256)       # the c += 64 loop: a partial wave, one short, exactly one trip, one over, 3, 4
GATHER_ROWS = {("C%d" % c): (dict(B=2, N=23, M=11, C=c, same=False), "width %d" % c) for c in GATHER_ROWS_C}
GATHER_ROWS["same"] = (dict(B=2, N=23, M=11, C=65, same=True), "every entry the same index")
GATHER_ROWS["2nd_trip"] = (dict(B=2, N=23, M=8200, C=5, same=False), "16 400 rows: beyond the grid cap")

# ---- three_interpolate_cl ------------------------------------------------------------------------------------------
INTERP_CL_C = (1, 63, 64, 65, 256, 260)
INTERP_CL = {}
for _c in INTERP_CL_C:
    INTERP_CL["C%d_m300" % _c] = (dict(B=2, m=300, n=9, C=_c, pad=0, col0=0), "width %d, ldo = C" % _c)
    INTERP_CL["C%d_pitched" % _c] = (dict(B=2, m=300, n=9, C=_c, pad=7, col0=3), "width %d inside rows of C + 7 at column 3" % _c)
INTERP_CL["m1"] = (dict(B=2, m=1, n=9, C=65, pad=0, col0=0), "one source: every tap on it")
INTERP_CL["m2_pitched"] = (dict(B=2, m=2, n=9, C=65, pad=4, col0=4), "two sources")
INTERP_CL["2nd_trip"] = (dict(B=2, m=300, n=8200, C=3, pad=2, col0=1), "16 400 rows: beyond the grid cap")
INTERP_CAT_CS = (1, 24, 65)

# ---- maxpool_ns ----------------------------------------------------------------------------------------------------
MAXPOOL = {("ns%d_C%d" % (ns, c)): (dict(R=7, ns=ns, C=c), "ns %d, C %d" % (ns, c)) for ns in (1, 2, 16, 64) for c in (1, 70, 256)}
MAXPOOL["2nd_trip"] = (dict(R=4100, ns=2, C=256), "1 049 600 outputs: the loop's second trip")


def maxpool_input(name, R, ns, C):
    """Values from a 5-value set, so that ties are everywhere; column 0 of every row all equal; +-inf sprinkled in;
    row 1 holds -inf everywhere (the first of them must win)."""
    rng = gen("maxpool" + name)
    x = rng.choice(np.array([-1.5, -0.25, 0.0, 0.75, 2.0], F32), (R, ns, C))
    x[rng.random((R, ns, C)) < 0.03] = -np.inf
    x[rng.random((R, ns, C)) < 0.03] = np.inf
    x[:, :, 0] = F32(0.75)
    if R > 1:
        x[1] = -np.inf
    if R > 2 and ns > 1:
        x[2, ns - 1] = 2.0            # the maximum only at the last position
        x[2, :ns - 1] = np.minimum(x[2, :ns - 1], F32(0.75))
    return x


# ---- colsum --------------------------------------------------------------------------------------------------------
COLSUM_N = (1, 3, 4, 5, 100, 255, 256, 257, 1024, 1028, 1030)
# N: 1..5 around one float4; 100 -> cgp 25 / 100, neither divides 256 (idle threads in the fold); 255..257 around one
# pass of the scalar kernel; 1024 one pass of the float4 kernel, 1028 / 1030 its second pass / the scalar kernel's fifth
COLSUM_LD_EXTRA = (0, 1, 4)          # ld = N, N + 1 (leaves float4), N + 4


def colsum_rows(rpb):
    return (1, rpb - 1, rpb, rpb + 1, 3 * rpb + 1)


# ---- invert_index --------------------------------------------------------------------------------------------------
def fits_lds(N, E):
    return 4 * (2 * N + 1 + E) <= LDS_LIMIT


# form -> [(N, E)]: "lds" and "global" through demf_invert_index, "split" through demf_invert_index_ws with a workspace
INVERT = {
    "lds": [(1, 300), (1023, 4000), (1024, 4000), (1025, 4000), (16384, 5000), (1025, 0), (1, 0)],
    "global": [(1023, 37000), (1024, 37000), (1025, 37000), (12000, 30000), (16384, 30000)],
    "split": [(1, 38400), (1023, 37000), (1024, 37000), (1025, 37000), (16384, 30000)],
}
LONG_LIST = 400         # entries of the hot point in the global-list form (its insertion sort is quadratic: <= 512)


def invert_indices(form, N, E, B=2):
    """The usual set; in the global-list and split forms the hot point's list is cut to LONG_LIST entries so that the
    one-thread insertion sort stays short, the rest spread over the other points."""
    rng = gen("invert_%s_%d_%d" % (form, N, E))
    if N == 1 or E == 0:
        return np.zeros((B, E), np.int32)
    idx = indices(rng, B, E, N)
    if form != "lds":
        for b in range(B):
            at = np.flatnonzero(idx[b] == hot(N))[LONG_LIST:]
            repl = rng.integers(0, N, at.size)
            repl[(repl == unused(N)) | (repl == hot(N))] = 0 if N < 3 else 1
            idx[b, at] = repl
        assert max(np.bincount(idx[b], minlength=N).max() for b in range(B)) <= 512
    return idx
