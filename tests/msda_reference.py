"""Float64 reference, error bounds and mutations for the multi-scale deformable attention kernels of csrc/msda.hip.
No GPU, not a test module.

REFERENCE.  Every float64 result a test judges by comes from the project's C oracle, ``oracle.kernels.msda_fwd`` /
``msda_bwd`` with ``dtype=np.float64`` (pinned to torch.grid_sample and autograd by tests/test_oracle_kernels.py), fed
the kernels' own float32 operands widened exactly.  For the raw forms ``raw_front_end`` evaluates in float64 what the
header comment of demf_msda_fwd_raw_f32 states: weights = softmax over the L*P logits of a head,
loc = ref + offset / (W_l, H_l).  ``Geometry`` restates the bilinear cell in numpy for what the oracle does not
return - magnitudes of uncancelled terms, differences between corners, the scatter counts of grad_value - and for the
mutations of ``MUTATIONS``; tests/test_msda_reference_host.py pins it to the oracle.

COORDINATE ROUNDING, eps_loc (u = 2^-24, one float32 rounding).  With p = loc * size (size = H_l or W_l, an integer,
so the float64 product of the float32 loc is exact) the pixel coordinate is p - 0.5.
  direct forms   fl(fl(p) - 0.5) or, contracted, fl(p - 0.5):  |error| <= u |p| + u |p - 0.5|           (eps_direct)
  raw forms      q = fl(off / size): u |off / size|;  loc = fl(ref + q): u |loc|;  both scaled by size on the way to
                 the pixel, then the direct form's two:  |error| <= u (|off| + |loc| size + |p| + |p - 0.5|) (eps_raw)
Where every one of these operations is exact in float32 (dyadic locations on power-of-two levels) eps_loc is 0.  The
cases are built (msda_cases) so that no sample's pixel coordinate lies within 8 eps_loc of an integer unless the sample
is outside the level by more than that on some axis: kernel and reference then sit in the same bilinear cell with the
same set of valid corners, for every sample, and no test drops an element.

BOUNDS, per element, all of the form c(n) u sum|term| + coordinate term.  V0..V3 are the corner values of a sample
((low,low), (low,high col), (high row, low), (high,high); an invalid corner counts as 0), lh / lw the fractions, hh =
1 - lh, hw = 1 - lw, top = grad_out.
  forward        n = 4 L P products.  A product carries <= 3 roundings in its bilinear weight (hh, hw, their product),
                 one for weight * attention in the wave / head forms, and is then added through <= n fma steps:
                 c = n + 8.  sum|term| = sum |attw| sum_k w_k |V_k| (the oracle on |value|, |attw|).
                 coordinate: sum_samples |attw| (eps_y max(|V2 - V0|, |V3 - V1|) + eps_x max(|V1 - V0|, |V3 - V2|)),
                 the sample being bilinear in (lh, lw).
  grad_attw      n = 4 Dh products, c = n + 8, sum|term| = sum_ch |top| sum_k w_k |V_k| (the oracle's grad_attw on
                 |value|, |grad_out|); coordinate as the forward's with |top| for |attw|, summed over the channels.
  grad_loc       x: attw W_l sum_ch top (hh (V1 - V0) + lh (V3 - V2)).  Magnitude over the UNCANCELLED terms,
                 |attw| W_l sum_ch |top| (hh (|V1| + |V0|) + lh (|V3| + |V2|)); c = 4 Dh + 12 (the difference, hh,
                 two products, the channel reduction, attw, W_l).  It does not depend on lw; its coordinate term is
                 eps_y |attw| W_l sum_ch |top| |V3 - V2 - V1 + V0|.  y likewise with H_l, hw / lw and eps_x.
  grad_value     (n + 2) u sum|term| + 2^-126 with n the number of contributions to the element, the prefill
                 included (gather_reference.Sum), plus the coordinate term the weights carry:
                 sum over contributions |attw top| (eps_y |dw_k/dlh| + eps_x |dw_k/dlw|), dw_k/dlh in {hw, lw},
                 dw_k/dlw in {hh, lh}.  (Zero on the power-of-two cases; on the odd pyramids a weight is only as good
                 as its coordinate, and without this term a correct kernel leaves the bound.)
  raw forms      add the error of the softmax weights, for logit x_i of a head with maximum m:
                 |d attw_i| <= attw_i u (|x_i - m| + sum_j attw_j |x_j - m| + 4 E + L P + 1) + 2^-126
                 (argument rounding of numerator and denominator, E ulp <= 2 E u per expf in both, the L P - 1
                 additions, the division; 2^-126 for a weight that underflows), times the sample's sum_k w_k |V_k|.
                 E = 4 x the worst error in ulp of numpy's float32 exp against float64 on the cases' own arguments:
                 measured 2.374 ulp (numpy's vectorised exp; tests/test_msda_reference_host.py prints it), so
                 E = 9.5 - the margin is there because the device function is a polynomial and is not correctly
                 rounded.
EXACT RULES, bit for bit: an output element with no valid term is +0.0; grad_loc and grad_attw of a sample with no
valid corner are 0; a grad_value element with no contribution keeps its prefill."""
import numpy as np

from gather_reference import Sum, U, TINY

F32, F64 = np.float32, np.float64
SLACK = 1.0 + 2.0 ** -10            # the second-order terms of the first-order bounds above
MUTATIONS = ("drop_corner", "swap_hw", "start_plus_one", "nonstrict_border", "trunc_for_floor", "head_plus_one",
             "softmax_over_P", "divide_by_hw_swapped")
FRONT_END_MUTATIONS = ("softmax_over_P", "divide_by_hw_swapped")


def _is_f32(x):
    with np.errstate(over="ignore"):
        return x.astype(F32).astype(F64) == x


def eps_direct(p):
    """p = loc * size in float64 -> the bound on the float32 error of p - 0.5."""
    p = np.asarray(p, F64)
    exact = _is_f32(p) & _is_f32(p - 0.5)
    return np.where(exact, 0.0, U * (np.abs(p) + np.abs(p - 0.5)) * SLACK)


def eps_raw(ref, off, size):
    """ref, off float64 views of float32 numbers, size the level's W or H -> the bound for ref + off / size."""
    ref, off, size = np.asarray(ref, F64), np.asarray(off, F64), np.asarray(size, F64)
    q = off / size
    loc = ref + q
    p = loc * size
    exact = _is_f32(q) & _is_f32(loc) & _is_f32(p) & _is_f32(p - 0.5)
    return np.where(exact, 0.0, U * (np.abs(off) + np.abs(loc) * size + np.abs(p) + np.abs(p - 0.5)) * SLACK)


def level_starts(shapes):
    sizes = [h * w for h, w in shapes]
    return np.array([0] + list(np.cumsum(sizes)[:-1]), np.int64)


def _lv(shapes, col):
    """(L, 1) float64 column of the level shapes, broadcasting over (..., L, P)."""
    return np.asarray(shapes, np.int64)[:, col].astype(F64)[:, None]


def pixel(shapes, loc):
    """loc (..., L, P, 2) float64 -> (x, y) pixel coordinates."""
    loc = np.asarray(loc, F64)
    return loc[..., 0] * _lv(shapes, 1) - 0.5, loc[..., 1] * _lv(shapes, 0) - 0.5


def eps_of_direct(shapes, loc):
    """-> (eps_x, eps_y), each (..., L, P)."""
    loc = np.asarray(loc, F64)
    return eps_direct(loc[..., 0] * _lv(shapes, 1)), eps_direct(loc[..., 1] * _lv(shapes, 0))


def robust(shapes, loc, eps_x, eps_y):
    """The construction condition, per sample: outside the level by more than 8 eps on some axis, or on both axes at
    least 8 eps from every integer (eps = 0: always)."""
    x, y = pixel(shapes, loc)
    W, H = _lv(shapes, 1), _lv(shapes, 0)
    out = (x < -1 - 8 * eps_x) | (x > W + 8 * eps_x) | (y < -1 - 8 * eps_y) | (y > H + 8 * eps_y)
    near = lambda p, e: (e > 0) & (np.abs(p - np.round(p)) <= 8 * e)
    return out | ~(near(x, eps_x) | near(y, eps_y))


# ---- the raw forms' front end ----------------------------------------------------------------------------------------
def raw_columns(raw, H, L, P, off_col0, lgt_col0):
    """raw (R, ldraw) -> offsets (R, H, L, P, 2) and logits (R, H, L * P), as stored."""
    R, n = raw.shape[0], H * L * P
    return raw[:, off_col0:off_col0 + 2 * n].reshape(R, H, L, P, 2), raw[:, lgt_col0:lgt_col0 + n].reshape(R, H, L * P)


def raw_front_end(off, lgt, ref, shapes, dtype=F64, mut=None):
    """off (R, H, L, P, 2), lgt (R, H, L*P), ref (R, L, 2) -> loc (R, H, L, P, 2), attw (R, H, L, P) in ``dtype``:
    attw = softmax over a head's L * P logits, loc = ref + off / (W_l, H_l)."""
    R, H, L, P, _ = off.shape
    x = np.asarray(lgt, dtype)
    if mut == "softmax_over_P":
        x = x.reshape(R, H, L, P)
    e = np.exp(x - x.max(-1, keepdims=True))
    attw = (e / e.sum(-1, keepdims=True, dtype=dtype)).reshape(R, H, L, P)
    cols = (0, 1) if mut == "divide_by_hw_swapped" else (1, 0)
    norm = np.asarray(shapes, np.int64)[:, cols].astype(dtype)[None, None, :, None, :]
    loc = np.asarray(ref, dtype)[:, None, :, None, :] + np.asarray(off, dtype) / norm
    assert loc.dtype == dtype and attw.dtype == dtype
    return loc, attw


def eps_of_raw(off, ref, shapes):
    """-> (eps_x, eps_y), each (R, H, L, P)."""
    off, ref = np.asarray(off, F64), np.asarray(ref, F64)[:, None, :, None, :]
    return eps_raw(ref[..., 0], off[..., 0], _lv(shapes, 1)), eps_raw(ref[..., 1], off[..., 1], _lv(shapes, 0))


def exp_arguments(lgt):
    """The float32 arguments x - max the kernels hand to expf."""
    x = np.asarray(lgt, F32)
    return x - x.max(-1, keepdims=True)


def exp_ulp_error(args):
    """Worst error, in ulp of the float64 result, of numpy's float32 exp on ``args`` (normal results only)."""
    a = np.asarray(args, F32).reshape(-1)
    want = np.exp(a.astype(F64))
    keep = want >= 2.0 ** -126
    got, want = np.exp(a)[keep].astype(F64), want[keep]
    return float((np.abs(got - want) / np.spacing(want.astype(F32)).astype(F64)).max()) if keep.any() else 0.0


EXP_ULP = 9.5           # E: 4 x the measured 2.374 (see the module docstring)


def softmax_weight_error(lgt, L, P):
    """lgt (R, H, L*P) float32 -> the bound on |attw_fp32 - attw_fp64|, (R, H, L, P)."""
    x = np.asarray(lgt, F64)
    d = np.abs(x - x.max(-1, keepdims=True))
    with np.errstate(under="ignore"):
        e = np.exp(-d)
    w = e / e.sum(-1, keepdims=True)
    rel = U * (d + (w * d).sum(-1, keepdims=True) + 4 * EXP_ULP + L * P + 1) * SLACK
    return (w * rel + TINY).reshape(x.shape[:2] + (L, P))


# ---- the bilinear cell in numpy --------------------------------------------------------------------------------------
class Geometry:
    """The cells of loc (N, H, L, P, 2) float64 on one scene's pyramid: per sample the four corners' tokens, weights
    and validity.  ``mut`` applies one of MUTATIONS."""

    def __init__(self, shapes, lsi, loc, S, mut=None):
        shapes = np.asarray(shapes, np.int64)
        if mut == "swap_hw":
            shapes = shapes[:, ::-1]
        Hl, Wl = shapes[:, 0][:, None], shapes[:, 1][:, None]
        start = np.asarray(lsi, np.int64)[:, None] + (1 if mut == "start_plus_one" else 0)
        loc = np.asarray(loc, F64)
        h_im, w_im = loc[..., 1] * Hl - 0.5, loc[..., 0] * Wl - 0.5
        if mut == "nonstrict_border":
            inside = (h_im >= -1) & (w_im >= -1) & (h_im <= Hl) & (w_im <= Wl)
        else:
            inside = (h_im > -1) & (w_im > -1) & (h_im < Hl) & (w_im < Wl)
        fl = np.trunc if mut == "trunc_for_floor" else np.floor
        hf, wf = fl(h_im), fl(w_im)
        self.lh, self.lw = h_im - hf, w_im - wf
        self.hh, self.hw = 1 - self.lh, 1 - self.lw
        rows = np.stack([hf, hf, hf + 1, hf + 1], -1)
        cols = np.stack([wf, wf + 1, wf, wf + 1], -1)
        Hk, Wk = Hl[..., None], Wl[..., None]
        self.ok = inside[..., None] & (rows >= 0) & (rows <= Hk - 1) & (cols >= 0) & (cols <= Wk - 1)
        if mut == "drop_corner":
            self.ok[..., 1] = False
        r, c = np.clip(rows, 0, Hk - 1).astype(np.int64), np.clip(cols, 0, Wk - 1).astype(np.int64)
        self.tok = np.minimum(start[..., None] + r * Wk + c, S - 1)
        self.wt = np.stack([self.hh * self.hw, self.hh * self.lw, self.lh * self.hw, self.lh * self.lw], -1) * self.ok
        # |d w_k / d lh| and |d w_k / d lw|
        self.dwt_h = np.stack([self.hw, self.lw, self.hw, self.lw], -1) * self.ok
        self.dwt_w = np.stack([self.hh, self.hh, self.lh, self.lh], -1) * self.ok
        self.Hl, self.Wl = Hl.astype(F64), Wl.astype(F64)
        self.head_shift = 1 if mut == "head_plus_one" else 0

    def corners(self, value):
        """value (S, H, Dh) -> V (N, H, L, P, 4, Dh), invalid corners as 0."""
        H = value.shape[1]
        h = ((np.arange(H) + self.head_shift) % H)[None, :, None, None, None]
        return np.asarray(value, F64)[self.tok, h] * self.ok[..., None]


class Result:
    """Everything the edge tests judge one case by.  Arrays are float64; ``None`` where not asked for."""


def evaluate(value, shapes, lsi, loc, attw, gout=None, prefill=None, eps=None, attw_err=None, mut=None,
             want_gvalue=True):
    """value (B, S, H, Dh), loc (B, Q, H, L, P, 2), attw (B, Q, H, L, P), gout (B, Q, H*Dh) or None, all exactly
    representable inputs (float32 values or float64 locations / weights of the raw front end).  -> Result with
      out, gattw, gloc, gvalue          the numpy restatement (``mut``: mutated)
      *_mag, *_coord                    sum|term| and the coordinate term of each bound
      out_terms (B, Q, H)               number of valid corners behind an output row of one head
      valid (B, Q, H, L, P)             the sample has a valid corner
      gvalue: a Sum (prefill included), gvalue_coord its coordinate term."""
    value = np.asarray(value)
    B, S, H, Dh = value.shape
    _, Q, _, L, P, _ = loc.shape
    ex, ey = eps if eps is not None else (np.zeros(loc.shape[:-1]), np.zeros(loc.shape[:-1]))
    r = Result()
    r.out, r.out_coord, r.out_softmax = (np.zeros((B, Q, H, Dh)) for _ in range(3))
    r.out_terms = np.zeros((B, Q, H), np.int64)
    r.valid = np.zeros((B, Q, H, L, P), bool)
    with_bwd = gout is not None
    if with_bwd:
        top_all = np.asarray(gout, F64).reshape(B, Q, H, Dh)
        r.gattw, r.gattw_coord = np.zeros((B, Q, H, L, P)), np.zeros((B, Q, H, L, P))
        r.gloc, r.gloc_mag, r.gloc_coord = (np.zeros((B, Q, H, L, P, 2)) for _ in range(3))
        if want_gvalue:
            shape = (B, S, H, Dh)
            if prefill is None:
                gv, gn, gS = np.zeros(shape), np.zeros(shape, np.int64), np.zeros(shape)
            else:
                gv = np.array(prefill, F64).reshape(shape)
                gn, gS = np.ones(shape, np.int64), np.abs(gv)
            ghits, gcoord = np.zeros(shape, np.int64), np.zeros(shape)
    for b in range(B):
        g = Geometry(shapes, lsi, loc[b], S, mut)
        aw = np.asarray(attw[b], F64)
        V = g.corners(value[b])
        r.valid[b] = g.ok.any(-1)
        r.out_terms[b] = g.ok.sum((-1, -2, -3))
        samp = (g.wt[..., None] * V).sum(-2)                                   # (Q, H, L, P, Dh)
        r.out[b] = (aw[..., None] * samp).sum((2, 3))
        adj_h = np.maximum(np.abs(V[..., 2, :] - V[..., 0, :]), np.abs(V[..., 3, :] - V[..., 1, :]))
        adj_w = np.maximum(np.abs(V[..., 1, :] - V[..., 0, :]), np.abs(V[..., 3, :] - V[..., 2, :]))
        coord = ey[b][..., None] * adj_h + ex[b][..., None] * adj_w
        r.out_coord[b] = (np.abs(aw)[..., None] * coord).sum((2, 3))
        if attw_err is not None:
            r.out_softmax[b] = (attw_err[b][..., None] * (g.wt[..., None] * np.abs(V)).sum(-2)).sum((2, 3))
        if not with_bwd:
            continue
        top = top_all[b][:, :, None, None, :]                                  # (Q, H, 1, 1, Dh)
        r.gattw[b] = (top * samp).sum(-1)
        r.gattw_coord[b] = (np.abs(top) * coord).sum(-1)
        a = np.abs
        hh, lh, hw, lw = (t[..., None] for t in (g.hh, g.lh, g.hw, g.lw))
        gw = hh * (V[..., 1, :] - V[..., 0, :]) + lh * (V[..., 3, :] - V[..., 2, :])
        gh = hw * (V[..., 2, :] - V[..., 0, :]) + lw * (V[..., 3, :] - V[..., 1, :])
        gw_mag = hh * (a(V[..., 1, :]) + a(V[..., 0, :])) + lh * (a(V[..., 3, :]) + a(V[..., 2, :]))
        gh_mag = hw * (a(V[..., 2, :]) + a(V[..., 0, :])) + lw * (a(V[..., 3, :]) + a(V[..., 1, :]))
        cross = a(V[..., 3, :] - V[..., 2, :] - V[..., 1, :] + V[..., 0, :])
        r.gloc[b, ..., 0] = aw * g.Wl * (top * gw).sum(-1)
        r.gloc[b, ..., 1] = aw * g.Hl * (top * gh).sum(-1)
        r.gloc_mag[b, ..., 0] = a(aw) * g.Wl * (a(top) * gw_mag).sum(-1)
        r.gloc_mag[b, ..., 1] = a(aw) * g.Hl * (a(top) * gh_mag).sum(-1)
        r.gloc_coord[b, ..., 0] = a(aw) * g.Wl * ey[b] * (a(top) * cross).sum(-1)
        r.gloc_coord[b, ..., 1] = a(aw) * g.Hl * ex[b] * (a(top) * cross).sum(-1)
        if want_gvalue:
            okk = g.ok                                                        # (Q, H, L, P, 4)
            hsel = np.broadcast_to(((np.arange(H) + g.head_shift) % H)[None, :, None, None, None], okk.shape)
            tok, hd = g.tok[okk], hsel[okk]
            awt = np.broadcast_to(aw[..., None, None] * top_all[b][:, :, None, None, None, :], okk.shape + (Dh,))[okk]
            terms = g.wt[okk][:, None] * awt                                   # (n, Dh)
            cterm = np.abs(awt) * (np.broadcast_to(ey[b][..., None], okk.shape)[okk] * g.dwt_h[okk]
                                   + np.broadcast_to(ex[b][..., None], okk.shape)[okk] * g.dwt_w[okk])[:, None]
            np.add.at(gv[b], (tok, hd), terms)
            np.add.at(gS[b], (tok, hd), np.abs(terms))
            np.add.at(gcoord[b], (tok, hd), cterm)
            np.add.at(ghits[b], (tok, hd), 1)
    r.out = r.out.reshape(B, Q, H * Dh)
    r.out_coord, r.out_softmax = r.out_coord.reshape(B, Q, H * Dh), r.out_softmax.reshape(B, Q, H * Dh)
    r.gvalue = Sum(gv, gn + ghits, gS, ghits) if with_bwd and want_gvalue else None
    r.gvalue_coord = gcoord if with_bwd and want_gvalue else None
    return r


def gamma(c):
    return c * U * SLACK


class Judged:
    """Float64 reference values (the oracle's) and per-element bounds of one case."""


def judge(value, shapes, lsi, loc, attw, gout=None, prefill=None, eps=None, attw_err=None, want_gvalue=True):
    """The oracle's float64 results with the bounds of the module docstring.  -> Judged with
    out, out_bound, out_zero (elements with no valid term), and with ``gout``: gattw, gattw_bound, gloc, gloc_bound,
    dead (samples without a valid corner), gvalue (Sum with the oracle's value), gvalue_bound."""
    from oracle import kernels as ok
    value64 = np.asarray(value, F64)
    B, S, H, Dh = value64.shape
    _, Q, _, L, P, _ = loc.shape
    loc64, attw64 = np.asarray(loc, F64), np.asarray(attw, F64)
    e = evaluate(value, shapes, lsi, loc64, attw64, gout, prefill, eps, attw_err, want_gvalue=want_gvalue)
    j = Judged()
    j.numpy = e
    j.out = ok.msda_fwd(value64, shapes, lsi, loc64, attw64, dtype=F64)
    mag = ok.msda_fwd(np.abs(value64), shapes, lsi, loc64, np.abs(attw64), dtype=F64)
    j.out_bound = gamma(4 * L * P + 8) * mag + e.out_coord + e.out_softmax + TINY
    j.out_zero = np.repeat(e.out_terms == 0, Dh, -1).reshape(B, Q, H * Dh)
    if gout is None:
        return j
    gout64 = np.asarray(gout, F64)
    gv, j.gloc, j.gattw = ok.msda_bwd(value64, shapes, lsi, loc64, attw64, gout64, dtype=F64)
    _, _, gattw_mag = ok.msda_bwd(np.abs(value64), shapes, lsi, loc64, attw64, np.abs(gout64), dtype=F64)
    j.gattw_bound = gamma(4 * Dh + 8) * gattw_mag + e.gattw_coord + TINY
    j.gloc_bound = gamma(4 * Dh + 12) * e.gloc_mag + e.gloc_coord + TINY
    j.dead = ~e.valid
    if want_gvalue:
        s = e.gvalue
        j.gvalue = Sum(gv + (0.0 if prefill is None else np.asarray(prefill, F64)), s.n, s.S, s.hits)
        j.gvalue_bound = j.gvalue.bound() + e.gvalue_coord * SLACK
    return j


def bf16_round(x):
    """float32 -> (the uint16 upper halves after round-to-nearest-even, the same values widened to float32)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return u.astype(np.uint16), (u << 16).astype(np.uint32).view(F32).reshape(np.shape(x))
