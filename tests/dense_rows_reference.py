"""Float64 restatements of the row kernels of csrc/dense.hip and of rows_ln_pos_kernel (csrc/rows_gemm.hip):
numpy on the CPU, no autograd, closed-form backward formulas, plus a host restatement of csrc/rng.h.  Every function
starts from the kernels' own fp32 inputs (promoted exactly) and returns ``{name: (value, scale)}``; an output passes
when, for EVERY element,

    |got - value| <= C * 2^-24 * scale + 2^-126

with C the constant of its group (tests/dense_rows_cases.py).  2^-126 is the smallest normal fp32 number: the GPU
flushes denormal results (exp(-100) of a softmax row) to zero.  Two outputs are a flushed probability times a factor
and carry that factor on the floor, as a third tuple element: the softmax's `out` (2^-126 * max(mask, 1)) and its
`dscores` (2^-126 * (1 + |d| + |sum(d * prob)|)).  Where ``value`` is not finite (the all-zero row of
the L2 kernels: 0 / 0) ``got`` must be non-finite too; a scale of 0 demands the exact value.

The backward functions take the PRIMAL inputs and redo the forward in fp64; a kernel's backward is fed the fp32
roundings of the reference's intermediates (stats, prob, y, norm, w, uvw), and each scale below covers that rounding.

Scales (u = 2^-24 is factored out; `mean_c`, `max_c`, `sum_c` run over a row's channels, `sum_r` over rows).  They
are built from the reference's own intermediates and the inputs, never from kernel output.

LayerNorm over s = identity + mask * x (mask = keep / (1 - p) as fp32), xh = (s - mean) * rstd, kappa = max_c|s| * rstd
(how many units of xh one rounding of the mean is worth), g = d * gamma with d = dy + dy2:
  s       |identity| + |mask * x|
  mean    max_c|s|
  rstd    rstd * (1 + kappa)        (one rounding of each s_c moves the variance by 2 u max|s| mean|s - mean|)
  y       max_c|s| * rstd * |gamma_c| + |beta_c|
  ds      rstd * (|g| + A + |xh| * B + kappa * (B + |xh| * A) + kappa^2 * u * A) (+ |ds_prev| when accumulated),
          A = mean_c|g|, B = mean_c|g * xh|; the last term is the mean's rounding squared, which alone is left on a
          constant row (xh = 0, kappa = max|s| / sqrt(eps))
  dx      ds's scale * mask
  dgamma  |prefill| + sum_r |d| * (|xh| + kappa)
  dbeta   |prefill| + sum_r |d|
Softmax rows, t = logit - row max:
  prob    prob * (1 + |t|)                      out: the same * mask
  dscores prob * (|d| + sum_c |d| * prob * (1 + |t|)) * (1 + |t|), d = dout * mask
Sampling preparation (px, py, pw = rows 0-2 of M applied to (x, y, z, 1); S(.) = the same sum over absolute terms):
  xw = px / pw            (S(px) + |xw| * S(pw)) / |pw|              (likewise yw)
  u0 = xw * au + bu       scale(xw) * |au| + |xw * au| + |bu|         (likewise v0)
  loc                     scale(u0) * vr + |u * vr| + 2 |off| / W_l   (u = clamp(u0, 0, 1); y with v0, H_l)
  w                       w * (1 + |t|)
  draw offsets            (|dloc| + |dloc2|) / W_l   (or H_l)
  draw logits             w * (|dw| + |dw2| + sum_i (|dw| + |dw2|) * w * (1 + |t|)) * (1 + |t|)
  dpts                    first-order propagation of  S(du) = sum (|dloc| + |dloc2|) * vr  through
                          gx = du * au / pw, gw = -(gx * xw + gy * yw), dpts = gx * M0 + gy * M1 + gw * M2,
                          every product adding its own magnitude and pw its S(pw) / |pw|
Row L2 normalisation, s = x (or rows + votes[:, 3:] in the vote tail), n = |s|_2, y = s / n:
  norm    n                 y    |y|              vote_xyz   |seed| + |votes[:, :3]|
  dx      (|g| + |y| * sum_c |y * g|) / n         (dvotes[:, 3:] and drows: the same; dvotes[:, :3] exact)
rows_ln_pos, s = x + resid:
  y       LayerNorm's y scale  (gamma given)  |  |x| + |resid|  (gamma null)
  ypos    y's scale + |y| + |pos|
"""
import numpy as np

F64 = np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -126


def _d(a):
    return None if a is None else np.asarray(a, dtype=F64)


def units(got, value, scale, floor=FLOOR):
    """max over elements of max(|got - value| - floor, 0) / (2^-24 * scale); scale 0: exact or inf; a non-finite
    ``value`` wants a non-finite ``got`` (and a finite one a finite ``got``)."""
    got, value, scale, floor = (np.asarray(a, dtype=F64).reshape(-1) for a in (
        got, value, np.broadcast_to(scale, np.shape(value)), np.broadcast_to(floor, np.shape(value))))
    assert got.shape == value.shape, (got.shape, value.shape)
    if got.size == 0:
        return 0.0
    fin = np.isfinite(value)
    bad = fin != np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.where(fin & ~bad, np.abs(got - value), 0.0)
        over = np.maximum(err - floor, 0.0)
        un = np.where(scale > 0, over / (U * np.where(scale > 0, scale, 1.0)), np.where(err == 0, 0.0, np.inf))
    un = np.where(bad, np.inf, un)
    return float(un.max())


# ---- csrc/rng.h ---------------------------------------------------------------------------------------------------
def mix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def dropout_keep(seed, step, op, start, n, p):
    """Keep bits of elements start .. start + n - 1 for the device state (seed, step) and operator id ``op``."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    w = lambda v: np.array([v & 0xFFFFFFFF], dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = mix32(w(seed) ^ np.uint32(0x9E3779B9))
        h = mix32(h ^ w(seed >> 32))
        h = mix32(h ^ w(step))
        h = mix32(h ^ w(step >> 32) ^ w((int(op) & 0xFFFFFFFF) * 0x632BE5AB))
        idx = np.arange(start, start + n, dtype=np.uint64)
        h = mix32(h ^ (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        h = mix32(h ^ (idx >> np.uint64(32)).astype(np.uint32))
    # (float)(h >> 8) * 2^-24 is exact in fp32; the comparison is against p as fp32
    return (h >> np.uint32(8)).astype(F64) * 2.0 ** -24 >= float(np.float32(p))


def dropout_scale(seed, step, op, start, n, p):
    """fp32 multipliers keep / (1 - p), the quotient taken in fp32 as the kernels take it; all ones for p = 0."""
    if p == 0:
        return np.ones(n, np.float32)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(dropout_keep(seed, step, op, start, n, p), inv, np.float32(0.0)).astype(np.float32)


# ---- dropout + residual + LayerNorm ---------------------------------------------------------------------------------
def _ln_core(s, eps):
    mean = s.mean(-1, keepdims=True)
    var = ((s - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    return mean, rstd, np.abs(s).max(-1, keepdims=True)


def ln_fwd(x, identity, gamma, beta, eps, mask=None):
    x, identity, gamma, beta, mask = _d(x), _d(identity), _d(gamma), _d(beta), _d(mask)
    mx = x if mask is None else x * mask.reshape(x.shape)
    s = mx if identity is None else identity + mx
    mean, rstd, smax = _ln_core(s, eps)
    y = (s - mean) * rstd * gamma + beta
    return dict(s=(s, np.abs(mx) + (0.0 if identity is None else np.abs(identity))),
                mean=(mean[:, 0], smax[:, 0]), rstd=(rstd[:, 0], (rstd * (1.0 + smax * rstd))[:, 0]),
                y=(y, smax * rstd * np.abs(gamma) + np.abs(beta)))


def ln_bwd(dy, dy2, x, identity, gamma, eps, mask=None, ds_prev=None, dgamma0=None, dbeta0=None):
    """Gradients of sum(dy * y) at the exact s: ds (added onto ds_prev when given), dx = ds * mask (ds_prev not
    included), dgamma / dbeta added onto their prefill."""
    d = _d(dy) + (0.0 if dy2 is None else _d(dy2))
    gamma, mask = _d(gamma), _d(mask)
    s = ln_fwd(x, identity, gamma, np.zeros_like(gamma), eps, mask)["s"][0]
    mean, rstd, smax = _ln_core(s, eps)
    xh = (s - mean) * rstd
    g = d * gamma
    m1, m2 = g.mean(-1, keepdims=True), (g * xh).mean(-1, keepdims=True)
    ds = rstd * (g - m1 - xh * m2)
    kappa = smax * rstd
    A, B = np.abs(g).mean(-1, keepdims=True), np.abs(g * xh).mean(-1, keepdims=True)
    sc = rstd * (np.abs(g) + A + np.abs(xh) * B + kappa * (B + np.abs(xh) * A) + kappa ** 2 * U * A)
    m = 1.0 if mask is None else mask.reshape(s.shape)
    p0 = lambda a: 0.0 if a is None else _d(a)
    return dict(ds=(ds + p0(ds_prev), sc + np.abs(p0(ds_prev))), dx=(ds * m, sc * m),
                dgamma=((d * xh).sum(0) + p0(dgamma0), (np.abs(d) * (np.abs(xh) + kappa)).sum(0) + np.abs(p0(dgamma0))),
                dbeta=(d.sum(0) + p0(dbeta0), np.abs(d).sum(0) + np.abs(p0(dbeta0))))


def rows_ln_pos(x, resid, gamma, beta, eps, pos):
    x, resid, gamma, beta, pos = _d(x), _d(resid), _d(gamma), _d(beta), _d(pos)
    s = x if resid is None else x + resid
    if gamma is None:
        y, sy = s, np.abs(x) + (0.0 if resid is None else np.abs(resid))
    else:
        mean, rstd, smax = _ln_core(s, eps)
        y, sy = (s - mean) * rstd * gamma + beta, smax * rstd * np.abs(gamma) + np.abs(beta)
    out = dict(y=(y, sy))
    if pos is not None:
        out["ypos"] = (y + pos, sy + np.abs(y) + np.abs(pos))
    return out


# ---- softmax + dropout ----------------------------------------------------------------------------------------------
def softmax_fwd(scores, mask=None):
    sc = _d(scores)
    t = sc - sc.max(-1, keepdims=True)
    e = np.exp(t)
    prob = e / e.sum(-1, keepdims=True)
    sp = prob * (1.0 + np.abs(t))
    m = 1.0 if mask is None else _d(mask).reshape(sc.shape)
    return dict(prob=(prob, sp), out=(prob * m, sp * m, FLOOR * np.maximum(m, 1.0)))


def softmax_bwd(scores, dout, mask=None):
    """In place over dout: dscores = prob * (d - sum(d * prob)), d = dout * mask."""
    sc = _d(scores)
    t = sc - sc.max(-1, keepdims=True)
    prob = softmax_fwd(scores)["prob"][0]
    d = _d(dout) * (1.0 if mask is None else _d(mask).reshape(sc.shape))
    dot = (d * prob).sum(-1, keepdims=True)
    sdot = (np.abs(d) * prob * (1.0 + np.abs(t))).sum(-1, keepdims=True)
    return dict(dscores=(prob * (d - dot), prob * (np.abs(d) + sdot) * (1.0 + np.abs(t)), FLOOR * (1.0 + np.abs(d) + np.abs(dot))))


# ---- sampling-location preparation ----------------------------------------------------------------------------------
def _project(pts, M, ab, Q):
    """Per row: xw, yw, u0, v0 and their scales, pw and S(pw) / |pw|, the row's M (R, 4, 4) and ab (R, 4)."""
    pts, M, ab = _d(pts), _d(M).reshape(-1, 4, 4), _d(ab).reshape(-1, 4)
    R = pts.shape[0]
    b = np.arange(R) // Q
    Mr, abr = M[b], ab[b]
    hom = np.concatenate([pts, np.ones((R, 1))], 1)
    pr = np.einsum("rij,rj->ri", Mr[:, :3], hom)
    Sp = np.einsum("rij,rj->ri", np.abs(Mr[:, :3]), np.abs(hom))
    pw = pr[:, 2]
    xw, yw = pr[:, 0] / pw, pr[:, 1] / pw
    sxw = (Sp[:, 0] + np.abs(xw) * Sp[:, 2]) / np.abs(pw)
    syw = (Sp[:, 1] + np.abs(yw) * Sp[:, 2]) / np.abs(pw)
    u0, v0 = xw * abr[:, 0] + abr[:, 1], yw * abr[:, 2] + abr[:, 3]
    su0 = sxw * np.abs(abr[:, 0]) + np.abs(xw * abr[:, 0]) + np.abs(abr[:, 1])
    sv0 = syw * np.abs(abr[:, 2]) + np.abs(yw * abr[:, 2]) + np.abs(abr[:, 3])
    return dict(b=b, M=Mr, ab=abr, pw=pw, rpw=Sp[:, 2] / np.abs(pw), xw=xw, yw=yw, sxw=sxw, syw=syw, u0=u0, v0=v0,
                su0=su0, sv0=sv0)


def _split_raw(raw, R, H, L, P):
    raw = _d(raw).reshape(R, H * L * P * 3)
    return raw[:, :H * L * P * 2].reshape(R, H, L, P, 2), raw[:, H * L * P * 2:].reshape(R, H, L * P)


def prep_fwd(pts, M, ab, vr, shapes, raw, Q, H, L, P):
    R = np.shape(pts)[0]
    pj = _project(pts, M, ab, Q)
    vr, shapes = _d(vr).reshape(-1, L, 2)[pj["b"]], _d(shapes).reshape(L, 2)
    off, lg = _split_raw(raw, R, H, L, P)
    wh = np.stack([shapes[:, 1], shapes[:, 0]], -1)                              # (L, 2): (W_l, H_l)
    uv = np.clip(np.stack([pj["u0"], pj["v0"]], -1), 0.0, 1.0)                   # (R, 2)
    suv = np.stack([pj["su0"], pj["sv0"]], -1)
    ref = (uv[:, None] * vr)[:, None, :, None, :]                                # (R, 1, L, 1, 2)
    loc = ref + off / wh[None, None, :, None, :]
    sloc = (suv[:, None] * vr)[:, None, :, None, :] + np.abs(ref) + 2.0 * np.abs(off) / wh[None, None, :, None, :]
    t = lg - lg.max(-1, keepdims=True)
    e = np.exp(t)
    w = e / e.sum(-1, keepdims=True)
    uvw = np.stack([pj["u0"], pj["v0"], pj["xw"], pj["yw"]], -1)
    suvw = np.stack([pj["su0"], pj["sv0"], pj["sxw"], pj["syw"]], -1)
    return dict(loc=(loc, np.broadcast_to(sloc, loc.shape)), w=(w.reshape(R, H, L, P), (w * (1 + np.abs(t))).reshape(R, H, L, P)),
                uvw=(uvw, suvw))


def prep_bwd(pts, M, ab, vr, shapes, raw, dloc, dloc2, dw, dw2, Q, H, L, P):
    """draw (R, H*L*P*3) and dpts (R, 3); torch.clamp passes the gradient on the closed interval [0, 1]."""
    R = np.shape(pts)[0]
    pj = _project(pts, M, ab, Q)
    vr, shapes = _d(vr).reshape(-1, L, 2)[pj["b"]], _d(shapes).reshape(L, 2)
    _, lg = _split_raw(raw, R, H, L, P)
    wh = np.stack([shapes[:, 1], shapes[:, 0]], -1)
    t = lg - lg.max(-1, keepdims=True)
    e = np.exp(t)
    w = e / e.sum(-1, keepdims=True)
    z = lambda a, b: (_d(a) + (0.0 if b is None else _d(b)), np.abs(_d(a)) + (0.0 if b is None else np.abs(_d(b))))
    DL, aDL = (a.reshape(R, H, L, P, 2) for a in z(dloc, dloc2))
    DW, aDW = (a.reshape(R, H, L * P) for a in z(dw, dw2))
    doff, sdoff = DL / wh[None, None, :, None, :], aDL / wh[None, None, :, None, :]
    dot, adot = (DW * w).sum(-1, keepdims=True), (aDW * w * (1 + np.abs(t))).sum(-1, keepdims=True)
    dlg, sdlg = w * (DW - dot), w * (aDW + adot) * (1 + np.abs(t))
    draw = np.concatenate([doff.reshape(R, -1), dlg.reshape(R, -1)], 1)
    sdraw = np.concatenate([sdoff.reshape(R, -1), sdlg.reshape(R, -1)], 1)
    duv = (DL * vr[:, None, :, None, :]).sum((1, 2, 3))                          # (R, 2)
    sduv = (aDL * vr[:, None, :, None, :]).sum((1, 2, 3))
    gate = np.stack([(pj["u0"] >= 0) & (pj["u0"] <= 1), (pj["v0"] >= 0) & (pj["v0"] <= 1)], -1)
    duv, sduv = duv * gate, sduv * gate
    a2 = pj["ab"][:, [0, 2]]
    gxy = duv * a2 / pj["pw"][:, None]
    sgxy = (sduv * np.abs(a2) / np.abs(pj["pw"])[:, None]) + np.abs(gxy) * (2.0 + pj["rpw"][:, None])
    xy = np.stack([pj["xw"], pj["yw"]], -1)
    gw = -(gxy * xy).sum(-1)
    sgw = (sgxy * np.abs(xy) + 2.0 * np.abs(gxy * xy)).sum(-1)
    g3, sg3 = np.concatenate([gxy, gw[:, None]], 1), np.concatenate([sgxy, sgw[:, None]], 1)
    M3 = pj["M"][:, :3, :3]                                                      # rows px, py, pw x columns x, y, z
    dpts = np.einsum("ri,rij->rj", g3, M3)
    sdpts = np.einsum("ri,rij->rj", sg3 + np.abs(g3), np.abs(M3))
    return dict(draw=(draw, sdraw), dpts=(dpts, sdpts))


# ---- row L2 normalisation and the vote tail -------------------------------------------------------------------------
def _l2(s):
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt((s * s).sum(-1, keepdims=True))
        return n, s / n


def l2norm_fwd(x):
    n, y = _l2(_d(x))
    return dict(y=(y, np.abs(y)), norm=(n[:, 0], n[:, 0]))


def _l2_bwd(s, g):
    n, y = _l2(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = (y * g).sum(-1, keepdims=True)
        return (g - y * dot) / n, (np.abs(g) + np.abs(y) * np.abs(y * g).sum(-1, keepdims=True)) / n


def l2norm_bwd(x, dy):
    return dict(dx=_l2_bwd(_d(x), _d(dy)))


def vote_fwd(rows, votes, seed_xyz):
    rows, votes, seed = _d(rows), _d(votes), _d(seed_xyz).reshape(-1, 3)
    n, y = _l2(rows + votes[:, 3:])
    return dict(vote_xyz=(seed + votes[:, :3], np.abs(seed) + np.abs(votes[:, :3])), y=(y, np.abs(y)), norm=(n[:, 0], n[:, 0]))


def vote_bwd(rows, votes, dy, dxyz):
    rows, votes = _d(rows), _d(votes)
    R = rows.shape[0]
    g = np.zeros_like(rows) if dy is None else _d(dy)
    dr, sdr = _l2_bwd(rows + votes[:, 3:], g)
    d3 = np.zeros((R, 3)) if dxyz is None else _d(dxyz).reshape(R, 3)
    return dict(drows=(dr, sdr), dvotes=(np.concatenate([d3, dr], 1), np.concatenate([np.zeros((R, 3)), sdr], 1)))
