"""Shapes and inputs of the deformable-attention edge tests (tests/test_gpu_msda_edges.py), each row with the reason it
is there, and ``form_of``: the dispatch conditions of csrc/msda.hip restated, naming the kernel a case lands on.  Not a
test module.  Everything is built on the CPU from seeded generators, so the GPU test, the child process and the float64
reference see identical numbers.

Launch geometry the shapes are chosen against (csrc/msda.hip):
  direct kernels      G = Dh / 4 lanes per (scene, query, head) item, 256 threads per block; (L, P) = (4, 2) and (4, 4)
                      are compile-time, every other pair a runtime loop; any other Dh, a value pointer off 16 bytes
                      (8 for bf16) or an out / grad_out pointer off 16 bytes takes the generic one-thread-per-item kernels
  raw, wave form      one wave per row b * Q + q, 4 rows per block, H = 8 and even, 8-byte aligned operands only; with
                      DEMF_MSDA_XCD the grid is rounded up to a multiple of 8 blocks and remapped
  raw, lane form      8 lanes per (row, head): everything else the raw entry accepts
  head form           one workgroup per (scene, head, chunk of queries), 8 waves x 8 queries per pass; chunks =
                      ceil(DEMF_MSDA_HEAD_WGS / (8 B)) before rounding the chunk to a multiple of 64 queries
"""
import itertools

import numpy as np

import msda_reference as ref
from gather_cases import SENTINEL, gen, normal  # noqa: F401  (SENTINEL: re-exported to the GPU test)

F32, F64 = np.float32, np.float64
GARBAGE = F32(3.0e30)         # fills every column a kernel has no business reading
FAR = 1.0e6                   # the far-outside location
DEFAULT_SWITCHES = {"DEMF_MSDA_RAW_LANES": 0, "DEMF_MSDA_XCD": 0, "DEMF_MSDA_NT": 1, "DEMF_MSDA_HEAD_WGS": 256}
CHILD_SWITCHES = dict(DEFAULT_SWITCHES, DEMF_MSDA_XCD=1, DEMF_MSDA_NT=0)

# pyramids: the first L levels of a list.  Power-of-two sides take the exact "edge" locations, the others random ones.
PYRAMIDS = {
    "pow2": ((8, 16), (4, 8), (2, 4), (1, 2), (1, 1), (2, 2), (4, 1), (16, 2)),
    "odd": ((7, 5), (13, 18), (3, 4), (2, 3), (1, 1), (1, 6), (5, 1), (3, 2)),       # levels 4-6: 1x1, 1xW, Hx1
    "thin_pow2": ((1, 1), (1, 8), (4, 1), (2, 2)),                                    # both clamps collapse, exactly
    "thin_odd": ((1, 1), (1, 6), (5, 1), (3, 2)),
    # the head form: a one-pixel-wide level among the memory levels and among the staged ones
    "head_pow2": ((8, 16), (4, 1), (1, 8), (1, 2)),
    "head_odd": ((7, 5), (1, 9), (3, 4), (6, 1)),
    "head_odd2": ((5, 1), (13, 18), (1, 1), (3, 1)),
}


def pyramid(kind, L):
    shapes = PYRAMIDS[kind][:L]
    assert len(shapes) == L
    return shapes


def is_exact(kind):
    return "pow2" in kind


# ---- sampling locations ----------------------------------------------------------------------------------------------
def edge_coordinates(n):
    """Pixel coordinates of one axis of size n: outside by the strict comparison, the half-pixel border, 0, an interior
    integer (the kink), n - 1, n - 0.5, n (outside)."""
    return (-1.0, -0.5, 0.0, float(n // 2), n - 1.0, n - 0.5, float(n))


def edge_pairs(Hl, Wl):
    """(x, y) pixel pairs: every edge coordinate on one axis with an interior fraction on the other, then on both."""
    ex, ey = edge_coordinates(Wl), edge_coordinates(Hl)
    fx, fy = (0.25 if Wl > 1 else -0.25), (0.75 if Hl > 1 else -0.75)
    return [(x, fy) for x in ex] + [(fx, y) for y in ey] + list(itertools.product(ex, ey))


def _all_outside(loc, shapes, exact):
    """Query 0 of every scene: each of its samples outside, cycling far outside on x, on y, on both, and just outside
    by the strict comparison (pixel -1 on x, pixel H_l on y)."""
    B, Q, H, L, P, _ = loc.shape
    if Q < 2:
        return
    for l, (Hl, Wl) in enumerate(shapes):
        kinds = [(FAR, 0.5), (0.5, -FAR), (-FAR, FAR), (-0.5 / Wl, 0.5), (0.5, (Hl + 0.5) / Hl)]
        if not exact:
            kinds = kinds[:3]                 # (just outside needs exact arithmetic: the power-of-two pyramids)
        for k in range(B * H * P):
            b, h, p = k // (H * P), (k // P) % H, k % P
            loc[b, 0, h, l, p] = kinds[(k + l) % len(kinds)]


def edge_locations(shapes, B, Q, H, P):
    """Exact (dyadic) locations on power-of-two levels, cycling through edge_pairs of each level."""
    L = len(shapes)
    loc = np.zeros((B, Q, H, L, P, 2), F64)
    k = np.arange(B * Q * H * P).reshape(B, Q, H, P)
    if Q >= 2:                                 # (query 0 is overwritten below: count the others only)
        k[:, 1:] = np.arange(B * (Q - 1) * H * P).reshape(B, Q - 1, H, P)
    for l, (Hl, Wl) in enumerate(shapes):
        pairs = np.array(edge_pairs(Hl, Wl), F64)
        xy = pairs[(k + 3 * l) % len(pairs)]
        loc[:, :, :, l, :, 0] = (xy[..., 0] + 0.5) / Wl
        loc[:, :, :, l, :, 1] = (xy[..., 1] + 0.5) / Hl
    _all_outside(loc, shapes, True)
    return loc


def random_targets(rng, shapes, B, Q, H, P):
    loc = rng.uniform(-0.25, 1.25, (B, Q, H, len(shapes), P, 2))
    _all_outside(loc, shapes, False)
    return loc


def direct_locations(name, kind, shapes, B, Q, H, P):
    """-> (loc float32 (B, Q, H, L, P, 2), (eps_x, eps_y)).  Random locations are drawn in float64 and redrawn, from
    the case's own generator, while any sample is within 8 eps_loc of an integer."""
    if is_exact(kind):
        loc64 = edge_locations(shapes, B, Q, H, P)
        loc = loc64.astype(F32)
        assert np.array_equal(loc.astype(F64), loc64)
        eps = ref.eps_of_direct(shapes, loc64)
        inside = np.abs(loc64) < 2
        assert not eps[0][inside[..., 0] & inside[..., 1]].any() and not eps[1][inside[..., 0] & inside[..., 1]].any()
        return loc, eps
    rng = gen("msda_loc_" + name)
    loc = random_targets(rng, shapes, B, Q, H, P).astype(F32)
    for _ in range(100):
        eps = ref.eps_of_direct(shapes, loc)
        bad = ~ref.robust(shapes, loc.astype(F64), *eps)
        if not bad.any():
            return loc, eps
        loc[bad] = rng.uniform(-0.25, 1.25, (int(bad.sum()), 2)).astype(F32)
    raise AssertionError("no robust draw")


def attention_weights(rng, B, Q, H, L, P):
    """Normal weights (so: negative ones), every 5th exactly zero, and in every third item one that dominates."""
    w = normal(rng, B, Q, H, L * P)
    w.reshape(-1)[::5] = 0.0
    q, h = np.meshgrid(np.arange(Q), np.arange(H), indexing="ij")
    w[:, (q + h) % 3 == 0, (L * P) // 2] *= 100.0
    return w.reshape(B, Q, H, L, P)


# ---- direct entries --------------------------------------------------------------------------------------------------
GV_MODES = ("random", "zero", "null")          # grad_value: accumulate onto a prefill, onto zeros, or not wanted
RUNTIME_LP = ((4, 1), (1, 3), (3, 2), (8, 1))
_D = dict(entry="direct", B=2, Q=5, H=3, L=4, P=2, pyr="odd", value_shift=0, out_shift=0, gout_shift=0, gv="random")


def _d(**kw):
    return dict(_D, **kw)


DIRECT = {}
for _i, _G in enumerate((1, 2, 4, 8, 16, 32, 64)):
    _H = 3 if _G < 32 else 2
    _L, _P = RUNTIME_LP[_i % 4]
    DIRECT["G%d_L4P2" % _G] = (_d(Dh=4 * _G, H=_H, gv=GV_MODES[_i % 3]),
                               "G = %d, the (4, 2) template, odd pyramid; H = %d: the head offset matters" % (_G, _H))
    DIRECT["G%d_L4P4_edges" % _G] = (_d(Dh=4 * _G, H=2, Q=8, P=4, pyr="pow2", gv=GV_MODES[(_i + 1) % 3]),
                                     "G = %d, the (4, 4) template, every exact edge pair of every level" % _G)
    DIRECT["G%d_L%dP%d" % (_G, _L, _P)] = (_d(Dh=4 * _G, H=_H, L=_L, P=_P, pyr="odd" if _L != 3 else "pow2",
                                              gv=GV_MODES[(_i + 2) % 3]),
                                           "G = %d, the runtime loop at (L, P) = (%d, %d)" % (_G, _L, _P))
DIRECT.update({
    "gen_Dh5": (_d(Dh=5), "generic: Dh no multiple of 4"),
    "gen_Dh12_edges": (_d(Dh=12, H=2, Q=8, P=4, pyr="pow2", gv="zero"), "generic: G = 3 is no power of two; exact edges"),
    "gen_Dh20": (_d(Dh=20, L=8, P=1, gv="null"), "generic: G = 5; 8 levels with the 1x1, 1xW and Hx1 ones"),
    "gen_Dh512": (_d(Dh=512, H=1, Q=3), "generic: G = 128 is past a wave"),
    "gen_value_off": (_d(Dh=32, value_shift=1), "generic both ways: value 4 bytes off 16-byte alignment"),
    "gen_out_off": (_d(Dh=32, out_shift=1, gout_shift=1, gv="zero"), "generic: out (forward) / grad_out (backward) 4 bytes off"),
    "prod_H1_Dh256": (_d(H=1, Dh=256, B=3, Q=7), "the fusion attention's value path: G = 64, whole-wave reduction"),
    "prod_H1_Dh256_edges": (_d(H=1, Dh=256, Q=32, pyr="pow2", gv="zero"), "the same on every exact edge pair"),
    "prod_H1_Dh4": (_d(H=1, Dh=4, B=3, Q=7, gv="zero"), "the fusion attention's 4-channel path: G = 1"),
    "prod_H1_Dh4_thin_edges": (_d(H=1, Dh=4, Q=32, pyr="thin_pow2"), "G = 1 on 1x1, 1xW, Hx1 levels, exact edges"),
    "prod_H8_Dh32": (_d(H=8, Dh=32, gv="null"), "the reference configuration H = 8, Dh = 32, L = 4, P = 2"),
    "prod_H8_Dh32_thin_edges": (_d(H=8, Dh=32, Q=4, P=4, pyr="thin_pow2"), "the same on collapsed levels, exact edges"),
    "threads_256": (_d(B=1, Q=4, H=8, Dh=32), "items * G = 256: exactly one block"),
    "threads_255": (_d(B=3, Q=85, H=1, Dh=4, gv="zero"), "items * G = 255: one short of a block; B = 3"),
    "threads_256_G1": (_d(B=2, Q=128, H=1, Dh=4, gv="null"), "items * G = 256 at G = 1"),
    "threads_257": (_d(B=1, Q=1, H=257, Dh=4, pyr="thin_odd"), "items * G = 257: one thread in the second block"),
    "threads_264_G8": (_d(B=3, Q=11, H=1, Dh=32), "items * G = 264: a second block holding one item's 8 lanes; B = 3"),
    "single_item": (_d(B=1, Q=1, H=1, Dh=32, gv="zero"), "a single item: 8 live lanes, 56 kept for the reductions"),
    "single_item_G64": (_d(B=1, Q=1, H=1, Dh=256), "a single item at G = 64"),
})

BF16 = {
    "bf16_G1": (_d(entry="bf16", H=1, Dh=4, B=3, Q=7), "bf16 rows, G = 1"),
    "bf16_G8_edges": (_d(entry="bf16", H=8, Dh=32, Q=4, P=4, pyr="pow2", gv="zero"), "bf16 rows, G = 8, exact edges"),
    "bf16_G64": (_d(entry="bf16", H=1, Dh=256, B=3, Q=7, gv="null"), "bf16 rows, G = 64 (the fusion attention in bf16 mode)"),
    "bf16_gen_Dh12": (_d(entry="bf16", Dh=12, L=3, P=2), "bf16 rows, the generic kernels' one-element loader"),
}


def direct_inputs(name, c):
    """-> dict(shapes, lsi, S, value, loc, attw, gout, prefill, eps); value is rounded to bf16 for the bf16 entries
    (``value_bits`` holds the 2-byte rows)."""
    shapes = pyramid(c["pyr"], c["L"])
    lsi = ref.level_starts(shapes)
    S = int(sum(h * w for h, w in shapes))
    B, Q, H, Dh, L, P = (c[k] for k in ("B", "Q", "H", "Dh", "L", "P"))
    rng = gen("msda_direct_" + name)
    d = dict(shapes=np.array(shapes, np.int64), lsi=lsi, S=S)
    d["value"] = normal(rng, B, S, H, Dh)
    if c["entry"] == "bf16":
        d["value_bits"], d["value"] = ref.bf16_round(d["value"])
    d["attw"] = attention_weights(rng, B, Q, H, L, P)
    d["gout"] = normal(rng, B, Q, H * Dh)
    d["prefill"] = {"random": normal(rng, B, S, H, Dh), "zero": np.zeros((B, S, H, Dh), F32), "null": None}[c["gv"]]
    d["loc"], d["eps"] = direct_locations(name, c["pyr"], shapes, B, Q, H, P)
    return d


# ---- raw entries -----------------------------------------------------------------------------------------------------
_R = dict(entry="raw", B=1, Q=1, H=8, P=4, L=4, Dh=32, pyr="odd", vpitch=None, v_off=0, ldraw=None, off_col0=0,
          lgt_col0=None, raw_shift=0, ref_shift=0)


def _r(**kw):
    d = dict(_R, **kw)
    n = d["H"] * 4 * d["P"]
    if d["lgt_col0"] is None:
        d["lgt_col0"] = d["off_col0"] + 2 * n
    if d["ldraw"] is None:
        d["ldraw"] = d["lgt_col0"] + n
    if d["vpitch"] is None:
        d["vpitch"] = d["H"] * 32
    assert d["off_col0"] + 2 * n <= d["lgt_col0"] and d["lgt_col0"] + n <= d["ldraw"] and d["v_off"] + d["H"] * 32 <= d["vpitch"]
    return d


_ROWS = {1: (1, 1, "odd"), 3: (1, 3, "thin_odd"), 4: (2, 2, "odd"), 5: (1, 5, "thin_pow2"), 37: (1, 37, "pow2"),
         130: (2, 65, "odd")}
RAW = {}
for _P in (2, 4):
    for _rows in (1, 3, 4, 5, 37):
        _B, _Q, _pyr = _ROWS[_rows]
        RAW["wave_P%d_rows%d" % (_P, _rows)] = (_r(B=_B, Q=_Q, P=_P, pyr=_pyr),
                                                "wave form: %d rows against 4 per block, %s pyramid" % (_rows, _pyr))
RAW.update({
    "lane_H4": (_r(B=2, Q=3, H=4, pyr="pow2"), "lane form by H != 8; exact edges"),
    "lane_ldraw_odd": (_r(B=2, Q=3, P=2, ldraw=8 * 4 * 2 * 3 + 1), "lane form by an odd row pitch"),
    "lane_off_col_odd": (_r(B=1, Q=5, off_col0=1, ldraw=386, pyr="thin_pow2"), "lane form by an odd offset column"),
    "lane_raw_off": (_r(B=1, Q=37, P=2, raw_shift=1, pyr="pow2"), "lane form by raw 4 bytes off 8-byte alignment; 2 blocks"),
    "lane_ref_off": (_r(B=2, Q=2, ref_shift=1, pyr="thin_odd"), "lane form by ref 4 bytes off 8-byte alignment"),
    "detr_li0": (_r(B=2, Q=13, vpitch=1536, v_off=0, off_col0=2, lgt_col0=264, ldraw=400),
                 "the 2D detector's call, layer 0: Q != S, value pitch 1536, a gap behind the offsets, a wide raw row"),
    "detr_li5": (_r(B=2, Q=13, vpitch=1536, v_off=1280, off_col0=2, lgt_col0=264, ldraw=400, pyr="pow2"),
                 "the same at layer 5: the value pointer 256 * 5 floats into the row; exact edges"),
})

XCD = {}
for _P in (2, 4):
    for _rows in (1, 5, 37, 130):
        _B, _Q, _pyr = _ROWS[_rows]
        XCD["xcd_P%d_rows%d" % (_P, _rows)] = (_r(B=_B, Q=_Q, P=_P, pyr=_pyr),
                                               "XCD order, plain loads: %d rows, grid rounded up to 8 blocks" % _rows)

HEAD = {}
for (_qi, _Q), (_bi, _B) in itertools.product(enumerate((1, 8, 63, 64, 65, 130)), enumerate((1, 32))):
    _P, _first = (2, 4)[(_qi + _bi) % 2], (2, 3)[(_qi // 2 + _bi) % 2]
    _pyr = ("head_odd", "head_pow2", "head_odd2")[_qi % 3]
    _vp = 1536 if (_bi == 0 and _qi % 2 == 0) else 256
    HEAD["head_P%d_LS%d_Q%d_B%d" % (_P, _first, _Q, _B)] = (
        _r(entry="head", B=_B, Q=_Q, P=_P, pyr=_pyr, vpitch=_vp, v_off=256 if _vp > 256 else 0, first=_first),
        "head form <%d, %d>: %s, value pitch %d, %s" % (_P, _first, "chunks of 64 queries" if _B == 1 else
                                                        "one chunk, %d pass(es)" % ((_Q + 63) // 64), _vp, _pyr))

LOGIT_KINDS = ("random", "equal", "equal_at_-1e4", "one_+80_rest_-80")


def logits(rng, R, H, NP):
    """Every (row, head) takes one of LOGIT_KINDS, in turn."""
    lg = 2.0 * normal(rng, R, H, NP)
    r, h = np.meshgrid(np.arange(R), np.arange(H), indexing="ij")
    kind = (r + h) % 4
    lg[kind == 1] = 0.7
    lg[kind == 2] = -1.0e4
    hot = np.full((R, H, NP), -80.0, F32)
    hot[r, h, (r + 3 * h) % NP] = 80.0
    lg[kind == 3] = hot[kind == 3]
    return lg


def raw_inputs(name, c):
    """-> dict(shapes, lsi, S, raw (R, ldraw), ref (R, L, 2), vbuf (B, S, vpitch), value (B, S, H, Dh), off, lgt,
    loc, attw (float64, from the front end), eps, attw_err).  Offsets are redrawn while a sample's pixel coordinate is
    within 8 eps_loc of an integer."""
    B, Q, H, P, L, Dh = (c[k] for k in ("B", "Q", "H", "P", "L", "Dh"))
    shapes = pyramid(c["pyr"], L)
    S, R, n = int(sum(h * w for h, w in shapes)), B * Q, H * L * P
    rng = gen("msda_raw_" + name)
    d = dict(shapes=np.array(shapes, np.int64), lsi=ref.level_starts(shapes), S=S)
    norm = d["shapes"][:, ::-1].astype(F64)[None, None, :, None, :]
    if is_exact(c["pyr"]):
        target = edge_locations(shapes, B, Q, H, P).reshape(R, H, L, P, 2)
        rp = np.full((R, L, 2), 0.5, F32)
        rp[1::2] = 0.25
    else:
        target = random_targets(rng, shapes, B, Q, H, P).reshape(R, H, L, P, 2)
        rp = rng.uniform(0.0, 1.0, (R, L, 2)).astype(F32)
    to_off = lambda t, where=Ellipsis: ((t - rp.astype(F64)[:, None, :, None, :])[where] * np.broadcast_to(norm, t.shape)[where]).astype(F32)
    off = to_off(target)
    lgt = logits(rng, R, H, L * P)
    for _ in range(100):
        loc, attw = ref.raw_front_end(off, lgt, rp, shapes)
        eps = ref.eps_of_raw(off, rp, shapes)
        bad = ~ref.robust(shapes, loc, *eps)
        if not bad.any():
            break
        assert not is_exact(c["pyr"]), "an exact case needs no redraw"
        target[bad] = rng.uniform(-0.25, 1.25, (int(bad.sum()), 2))
        off[bad] = to_off(target, bad)
    else:
        raise AssertionError("no robust draw")
    if is_exact(c["pyr"]):
        assert np.array_equal(loc, target)
    raw = np.full((R, c["ldraw"]), GARBAGE, F32)
    raw[:, c["off_col0"]:c["off_col0"] + 2 * n] = off.reshape(R, 2 * n)
    raw[:, c["lgt_col0"]:c["lgt_col0"] + n] = lgt.reshape(R, n)
    vbuf = np.full((B, S, c["vpitch"]), GARBAGE, F32)
    value = normal(rng, B, S, H, Dh)
    vbuf[:, :, c["v_off"]:c["v_off"] + H * Dh] = value.reshape(B, S, H * Dh)
    shp = (B, Q, H, L, P)
    d.update(raw=raw, ref=rp, vbuf=vbuf, value=value, off=off, lgt=lgt, loc=loc.reshape(shp + (2,)), attw=attw.reshape(shp),
             eps=tuple(e.reshape(shp) for e in eps), attw_err=ref.softmax_weight_error(lgt, L, P).reshape(shp))
    if c["entry"] == "head":
        d["staged"] = S - int(d["lsi"][c["first"]])
    return d


# ---- what a case lands on --------------------------------------------------------------------------------------------
_GS = (1, 2, 4, 8, 16, 32, 64)
FORMS = (["msda_%s_kernel<%d,%d,%d>" % (d, g, tl, tp) for d in ("fwd", "bwd") for g in _GS for tl, tp in ((4, 2), (4, 4), (0, 0))]
         + ["msda_fwd_generic", "msda_bwd_generic"]
         # the bf16 instantiations differ from their fp32 twins in the loader alone (ld4 / ld1 of 2-byte rows): one
         # entry per loader and direction, not per G
         + ["msda_%s_kernel<bf16>" % d for d in ("fwd", "bwd")] + ["msda_%s_generic<bf16>" % d for d in ("fwd", "bwd")]
         + ["msda_fwd_raw_kernel<8,4,%d>" % p for p in (2, 4)]
         + ["msda_fwd_raw_wave_kernel<4,%d,%s>" % (p, nt) for p in (2, 4) for nt in ("true", "false")]
         + ["xcd block order"]
         + ["msda_fwd_raw_head_kernel<%d,%d>" % (p, ls) for p in (2, 4) for ls in (2, 3)])


def form_of(c, switches=DEFAULT_SWITCHES):
    """The kernel instantiation(s) a case runs, by the conditions of msda_fwd_impl / msda_bwd_impl,
    demf_msda_fwd_raw_f32 and demf_msda_fwd_raw_head_f32 (shifts are in 4-byte words off 16-byte alignment)."""
    e = c["entry"]
    if e in ("direct", "bf16"):
        Dh, G = c["Dh"], c["Dh"] // 4
        names = []
        for d, other in (("fwd", "out_shift"), ("bwd", "gout_shift")):
            value_ok = c["value_shift"] % (4 if e == "direct" else 2) == 0       # 16 bytes, or 8 for 2-byte rows
            fast = Dh % 4 == 0 and G in _GS and value_ok and c[other] % 4 == 0
            if e == "bf16":
                names.append("msda_%s_kernel<bf16>" % d if fast else "msda_%s_generic<bf16>" % d)
            elif fast:
                tl, tp = (c["L"], c["P"]) if (c["L"], c["P"]) in ((4, 2), (4, 4)) else (0, 0)
                names.append("msda_%s_kernel<%d,%d,%d>" % (d, G, tl, tp))
            else:
                names.append("msda_%s_generic" % d)
        return names
    assert c["Dh"] == 32 and c["L"] == 4 and c["P"] in (2, 4)
    if e == "head":
        assert c["first"] in (2, 3)
        return ["msda_fwd_raw_head_kernel<%d,%d>" % (c["P"], c["first"])]
    wave = (c["H"] == 8 and not switches["DEMF_MSDA_RAW_LANES"] and c["ldraw"] % 2 == 0 and c["off_col0"] % 2 == 0
            and c["raw_shift"] % 2 == 0 and c["ref_shift"] % 2 == 0)
    if not wave:
        return ["msda_fwd_raw_kernel<8,4,%d>" % c["P"]]
    names = ["msda_fwd_raw_wave_kernel<4,%d,%s>" % (c["P"], "true" if switches["DEMF_MSDA_NT"] else "false")]
    return names + (["xcd block order"] if switches["DEMF_MSDA_XCD"] else [])


def head_chunks(c, switches=DEFAULT_SWITCHES):
    """(chunks, queries per chunk, passes of a workgroup) of the head form's launch."""
    chunks = max(1, (switches["DEMF_MSDA_HEAD_WGS"] + c["B"] * 8 - 1) // (c["B"] * 8))
    qpc = ((c["Q"] + chunks - 1) // chunks + 63) // 64 * 64
    return (c["Q"] + qpc - 1) // qpc, qpc, (min(qpc, c["Q"]) + 63) // 64


# ---- refusals --------------------------------------------------------------------------------------------------------
# entry -> the scalar arguments of a call that would be accepted, in the entry's order (pointers are filled in between)
ACCEPTED = {
    "demf_msda_fwd_f32": dict(B=1, S=18, H=8, Dh=32, L=4, Q=2, P=4),
    "demf_msda_bwd_f32": dict(B=1, S=18, H=8, Dh=32, L=4, Q=2, P=4),
    "demf_msda_fwd_bf16": dict(B=1, S=18, H=8, Dh=32, L=4, Q=2, P=4),
    "demf_msda_bwd_bf16": dict(B=1, S=18, H=8, Dh=32, L=4, Q=2, P=4),
    "demf_msda_fwd_raw_f32": dict(B=1, S=18, H=8, Dh=32, L=4, Q=2, P=4, vpitch=256, ldraw=384, off_col0=0, lgt_col0=256),
    "demf_msda_fwd_raw_head_f32": dict(B=1, S=18, Q=2, P=4, vpitch=256, ldraw=384, off_col0=0, lgt_col0=256,
                                       first_staged_level=2, staged_tokens=6),
}
# (entry, what changes, why it must be refused); "null": the index of the pointer argument passed as NULL
REFUSED = [
    ("demf_msda_fwd_f32", dict(L=9), "more than 8 levels"),
    ("demf_msda_bwd_f32", dict(L=9), "more than 8 levels"),
    ("demf_msda_fwd_f32", dict(P=0), "no points"),
    ("demf_msda_bwd_f32", dict(P=0), "no points"),
    ("demf_msda_fwd_f32", dict(Dh=0), "no channels"),
    ("demf_msda_bwd_bf16", dict(Dh=0), "no channels"),
    ("demf_msda_fwd_f32", dict(S=1 << 20, H=8, Dh=256), "S * H * Dh = 2^31"),
    ("demf_msda_bwd_f32", dict(S=1 << 20, H=8, Dh=256), "S * H * Dh = 2^31"),
    ("demf_msda_fwd_bf16", dict(S=1 << 20, H=8, Dh=256), "S * H * Dh = 2^31"),
    ("demf_msda_fwd_f32", dict(null=0), "value is NULL"),
    ("demf_msda_fwd_f32", dict(null=5), "out is NULL"),
    ("demf_msda_bwd_f32", dict(null=7), "grad_sampling_loc is NULL"),
    ("demf_msda_fwd_raw_f32", dict(null=4), "ref is NULL"),
    ("demf_msda_fwd_raw_head_f32", dict(null=3), "raw is NULL"),
    ("demf_msda_fwd_raw_f32", dict(L=9), "more than 8 levels"),
    ("demf_msda_fwd_raw_f32", dict(Dh=16), "the raw forms are built for Dh = 32"),
    ("demf_msda_fwd_raw_f32", dict(P=3), "the raw forms are built for P in {2, 4}"),
    ("demf_msda_fwd_raw_f32", dict(vpitch=264), "value pitch no multiple of Dh"),
    ("demf_msda_fwd_raw_head_f32", dict(first_staged_level=1), "levels 1 .. 3 are never staged"),
    ("demf_msda_fwd_raw_head_f32", dict(staged_tokens=18), "staged_tokens >= S"),
    ("demf_msda_fwd_raw_head_f32", dict(P=3), "P in {2, 4}"),
    ("demf_msda_fwd_raw_head_f32", dict(vpitch=128), "a pitch below 8 heads x 32 channels"),
    ("demf_msda_fwd_raw_head_f32", dict(S=2000, staged_tokens=1300), "1300 tokens x 128 bytes + exchange slots > 160 KB"),
]
RETURNS_EARLY = [(entry, dict(**{k: 0})) for entry in ACCEPTED for k in ("B", "Q")]
