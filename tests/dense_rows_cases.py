"""Inputs of the row-kernel edge tests (tests/test_gpu_dense_rows_edges.py), the torch compositions of the same
operations (float32 to measure what an fp32 evaluation costs, float64 to check the closed-form reference against
autograd) and the tolerance constants.  Not a test module.

Everything is built on the CPU as fp32 numpy arrays from seeded generators, so the GPU test, the fp64 reference and
the fp32 composition see identical numbers."""
import numpy as np
import torch
import torch.nn.functional as F

import dense_rows_reference as ref

SENTINEL = np.float32(-7777.25)
EPS = float(np.float32(1e-5))          # as the kernels receive it
RNG_SEED, RNG_STEP = 0x1234ABCD9E3779B1, 0x100000007       # both halves of both words carry bits
P_DROP = (0.0, 0.4)

# Tolerance constants, in units of 2^-24 * scale (scales: docstring of tests/dense_rows_reference.py).  Each is 4x
# the worst error of the fp32 torch composition below (on the CPU) against the fp64 reference over ALL the cases of
# this module, rounded up to a power of two; the factor covers the kernels' different summation order (wave
# butterfly, LDS fold, atomics) and __expf.
# tests/test_dense_rows_reference_host.py::test_fp32_composition_sets_the_constants re-measures the composition.
#                     fp32 composition   kernel (MI355X): worst output of the group, its case
C_LN_S = 8.0        # 1.23               1.23 (ln_fwd s, R1023_C256 p0.4)
C_LN_STATS = 16.0   # 2.47               1.64 (ln_fwd mean, R1024_C256 p0.4)
C_LN_Y = 16.0       # 3.67               3.62 (ln_fwd y, R1024_C256 p0.4)
C_LN_DS = 16.0      # 3.55               3.27 (ln_bwd dx, R1025_C1024 p0.4)
C_LN_DGB = 8.0      # 1.91               1.91 (ln_bwd dbeta, R5_C512 p0)
C_SM_FWD = 64.0     # 9.71               4.29 (softmax_fwd out, R2049_S1024 p0)
C_SM_BWD = 16.0     # 3.17               2.20 (softmax_bwd dscores, R1024_S129 p0.4)
C_PREP_LOC = 8.0    # 1.03               1.03 (prep_fwd loc, H8_L4_P2)
C_PREP_W = 16.0     # 2.82               2.82 (prep_fwd w, H3_L3_P5)
C_PREP_UVW = 8.0    # 1.41               1.41 (prep_fwd uvw, H64_L1_P1)
C_PREP_DRAW = 16.0  # 2.04               2.79 (prep_bwd draw, H8_L4_P2 all)
C_PREP_DPTS = 4.0   # 0.79               0.91 (prep_bwd dpts, H6_L8_P2 all)
C_L2_FWD = 32.0     # 4.16               3.73 (vote_fwd y, R1024_C256)
C_L2_BWD = 16.0     # 3.99               3.08 (l2_bwd dx, R1025_C256)
C_RLP = 16.0        # 3.51               3.35 (rows_ln_pos y, R1025 g1 r1 y1 yp1)

# output name -> constant, per operation
GROUPS = {
    "ln_fwd": dict(s=C_LN_S, mean=C_LN_STATS, rstd=C_LN_STATS, y=C_LN_Y),
    "ln_bwd": dict(ds=C_LN_DS, dx=C_LN_DS, dgamma=C_LN_DGB, dbeta=C_LN_DGB),
    "rows_ln_pos": dict(y=C_RLP, ypos=C_RLP),
    "softmax_fwd": dict(prob=C_SM_FWD, out=C_SM_FWD),
    "softmax_bwd": dict(dscores=C_SM_BWD),
    "prep_fwd": dict(loc=C_PREP_LOC, w=C_PREP_W, uvw=C_PREP_UVW),
    "prep_bwd": dict(draw=C_PREP_DRAW, dpts=C_PREP_DPTS),
    "l2_fwd": dict(y=C_L2_FWD, norm=C_L2_FWD),
    "l2_bwd": dict(dx=C_L2_BWD),
    "vote_fwd": dict(y=C_L2_FWD, norm=C_L2_FWD, vote_xyz=C_L2_FWD),
    "vote_bwd": dict(drows=C_L2_BWD, dvotes=C_L2_BWD),
}


def _g(seed):
    return np.random.default_rng(seed)


def _grid(rng, *shape):
    """Standard normal, clipped to +-4, on the 2^-10 grid."""
    return (np.round(np.clip(rng.standard_normal(shape), -4, 4) * 1024) / 1024).astype(np.float32)


def mask_for(op, n, p):
    return ref.dropout_scale(RNG_SEED, RNG_STEP, op, 0, n, p)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
# (R, C): every width at R = 1 and 5 (the 4-rows-per-block tail), every row count at C = 256; R > 1024 makes the
# backward's rows_per_wave 2 (1025) and 3 (2049), with trailing waves that own no row
LN_SHAPES = ([(1, c) for c in (64, 128, 256, 512, 1024)] + [(5, c) for c in (64, 128, 512, 1024)] +
             [(r, 256) for r in (3, 4, 5, 1023, 1024, 1025, 2049)] +
             [(2049, 64), (1023, 128), (1024, 512), (1025, 1024)])
LN_KINDS = ("unit", "m100", "m1000", "const", "spike")


def ln_case(R, C, seed=0):
    """Row i is of kind LN_KINDS[(i + R + log2(C / 64)) % 5]: unit-scale; m + z with m = 100 / 1000 and z on the 2^-10 grid
    (s exact in fp32 when p = 0: what separates a two-pass variance from a one-pass one); constant (variance exactly
    0); one spike of 2^20.  s = identity + x with both parts on the grid.  gamma has zero and negative entries."""
    rng = _g(1000 * seed + 7 * R + C)
    kind = (np.arange(R) + R + (C // 64).bit_length() - 1) % 5
    x = _grid(rng, R, C)
    ident = _grid(rng, R, C)
    ident[kind == 1] += 100.0
    ident[kind == 2] += 1000.0
    ident[kind == 3] = 100.0
    x[kind == 3] = 0.0                                   # (dropout keeps 0 at 0: constant under either p)
    spike = rng.integers(0, C, R)
    ident[kind == 4, spike[kind == 4]] = 2.0 ** 20
    x[kind == 4, spike[kind == 4]] = 0.0
    gamma = (rng.standard_normal(C) * 1.5).astype(np.float32)
    gamma[::7] = 0.0
    gamma[3] = -abs(gamma[3]) - 0.5
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(R=R, C=C, x=x, identity=ident, gamma=gamma, beta=r(C), dy=r(R, C), dy2=(0.5 * r(R, C)).astype(np.float32),
                ds_prev=r(R, C), dgamma0=(3 * r(C)).astype(np.float32), dbeta0=(3 * r(C)).astype(np.float32),
                kind=kind, op=3 + C // 64 + R)


def ln_cases():
    return {"R%d_C%d" % s: ln_case(*s) for s in LN_SHAPES}


def ln_composition(c, dtype, p, one_pass=False):
    """F.layer_norm over identity + mask * x with autograd -> dict of every forward and backward output (d = dy + dy2,
    ds on top of ds_prev, dgamma / dbeta on top of their prefill).  ``one_pass``: the deliberately wrong variance
    E[s^2] - E[s]^2 instead."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    R, C = c["R"], c["C"]
    mask = t(mask_for(c["op"], R * C, p)).view(R, C)
    x = t(c["x"]).requires_grad_()
    s = (t(c["identity"]) + mask * x)
    s.retain_grad()
    gamma, beta = t(c["gamma"]).requires_grad_(), t(c["beta"]).requires_grad_()
    mean = s.mean(-1)
    if one_pass:
        var = (s * s).mean(-1) - mean * mean
        rstd = 1.0 / torch.sqrt(var + EPS)
        y = (s - mean[:, None]) * rstd[:, None] * gamma + beta
    else:
        rstd = 1.0 / torch.sqrt(s.var(-1, unbiased=False) + EPS)
        y = F.layer_norm(s, (C,), gamma, beta, EPS)
    (y * (t(c["dy"]) + t(c["dy2"]))).sum().backward()
    n = lambda a: a.detach().numpy()
    return dict(s=n(s), mean=n(mean), rstd=n(rstd), y=n(y), ds=n(s.grad + t(c["ds_prev"])), dx=n(x.grad),
                dgamma=n(gamma.grad + t(c["dgamma0"])), dbeta=n(beta.grad + t(c["dbeta0"])))


def ln_reference(c, p):
    mask = mask_for(c["op"], c["R"] * c["C"], p)
    out = ref.ln_fwd(c["x"], c["identity"], c["gamma"], c["beta"], EPS, mask)
    out.update(ref.ln_bwd(c["dy"], c["dy2"], c["x"], c["identity"], c["gamma"], EPS, mask, c["ds_prev"], c["dgamma0"],
                          c["dbeta0"]))
    return out


# ---- rows_ln_pos (C = 256 only) -------------------------------------------------------------------------------------
RLP_ROWS = (1, 3, 4, 5, 1023, 1025)


def rlp_case(R):
    c = ln_case(R, 256, seed=5)
    return dict(R=R, C=256, x=c["x"], resid=c["identity"], gamma=c["gamma"], beta=c["beta"], pos=c["dy"], kind=c["kind"])


def rlp_cases():
    return {"R%d" % R: rlp_case(R) for R in RLP_ROWS}


def rlp_composition(c, dtype, with_gamma=True, with_resid=True):
    t = lambda a: torch.from_numpy(a).to(dtype)
    s = t(c["x"]) + t(c["resid"]) if with_resid else t(c["x"])
    y = F.layer_norm(s, (256,), t(c["gamma"]), t(c["beta"]), EPS) if with_gamma else s
    return dict(y=y.numpy(), ypos=(y + t(c["pos"])).numpy())


# ---- softmax --------------------------------------------------------------------------------------------------------
# (R, S): S around the lane count and the VPL = 1 / 2 / 4 / 8 / 16 instantiations, R around the 4-row block
SM_SHAPES = ((5, 1), (1, 63), (3, 64), (4, 65), (1023, 128), (1024, 129), (1025, 257), (5, 512), (3, 513), (4, 1000),
             (2049, 1024), (5, 1024))
SM_KINDS = ("random3", "max100", "equal", "gap60", "neg1e30")


def sm_case(R, S):
    """Row i is of kind SM_KINDS[(i + R) % 5]: logits at scale 3; one logit of 100 (overflows without the max
    subtraction); all equal; one logit 60 above the rest (the others underflow towards 0); one logit of -1e30."""
    rng = _g(31 * R + S)
    sc = (3 * rng.standard_normal((R, S))).astype(np.float32)
    kind = (np.arange(R) + R) % 5
    col = rng.integers(0, S, R)
    rows = np.arange(R)
    sc[rows[kind == 1], col[kind == 1]] = 100.0
    sc[kind == 2] = np.float32(1.75)
    sc[rows[kind == 3], col[kind == 3]] += 60.0
    sc[rows[kind == 4], col[kind == 4]] = -1e30
    return dict(R=R, S=S, scores=sc, dout=rng.standard_normal((R, S)).astype(np.float32), kind=kind, op=11 + S)


def sm_cases():
    return {"R%d_S%d" % s: sm_case(*s) for s in SM_SHAPES}


def sm_composition(c, dtype, p, no_max=False):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    mask = t(mask_for(c["op"], c["R"] * c["S"], p)).view(c["R"], c["S"])
    sc = t(c["scores"]).requires_grad_()
    if no_max:
        e = torch.exp(sc)
        prob = e / e.sum(-1, keepdim=True)
    else:
        prob = torch.softmax(sc, -1)
    out = prob * mask
    (out * t(c["dout"])).sum().backward()
    return dict(prob=prob.detach().numpy(), out=out.detach().numpy(), dscores=sc.grad.numpy())


def sm_reference(c, p):
    mask = mask_for(c["op"], c["R"] * c["S"], p)
    out = ref.softmax_fwd(c["scores"], mask)
    out.update(ref.softmax_bwd(c["scores"], c["dout"], mask))
    return out


# ---- L2 normalisation and the vote tail -----------------------------------------------------------------------------
L2_SHAPES = ([(1, c) for c in (64, 128, 256, 512, 1024)] + [(r, 256) for r in (3, 4, 5, 1023, 1024, 1025, 2049)] +
             [(5, 64), (1025, 128), (3, 512), (5, 1024)])
L2_ZERO_SHAPES = ((3, 64), (5, 256), (1025, 1024))          # an all-zero row in the middle


def l2_case(R, C, zero_row=False):
    """Rows scaled by 2^-40, 1, 2^40 in turn (the sum of squares stays normal in fp32).  For the vote tail the row is
    split as rows + votes[:, 3:].  ``zero_row``: row R // 2 is all zero (rows = -votes there)."""
    rng = _g(13 * R + C + (1 if zero_row else 0))
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    scale = np.float32(2.0) ** (40 * ((np.arange(R) + R) % 3 - 1)).astype(np.float32)
    x = r(R, C) * scale[:, None]
    rows = (0.5 * r(R, C) * scale[:, None]).astype(np.float32)
    votes = np.concatenate([r(R, 3), r(R, C) * scale[:, None]], 1).astype(np.float32)
    if zero_row:
        x[R // 2] = 0.0
        rows[R // 2] = -votes[R // 2, 3:]
    return dict(R=R, C=C, x=x, rows=rows, votes=votes, seed_xyz=(3 * r(R, 3)).astype(np.float32),
                dy=(r(R, C) / scale[:, None]).astype(np.float32), dxyz=r(R, 3), zero=R // 2 if zero_row else None)


def l2_cases():
    out = {"R%d_C%d" % s: l2_case(*s) for s in L2_SHAPES}
    out.update({"zero_R%d_C%d" % s: l2_case(*s, zero_row=True) for s in L2_ZERO_SHAPES})
    return out


def l2_composition(c, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    x = t(c["x"]).requires_grad_()
    n = x.norm(dim=-1, keepdim=True)
    y = x / n
    (y * t(c["dy"])).sum().backward()
    return dict(y=y.detach().numpy(), norm=n.detach().numpy()[:, 0], dx=x.grad.numpy())


def vote_composition(c, dtype, with_dy=True, with_dxyz=True):
    t = lambda a: torch.from_numpy(a).to(dtype)
    rows, votes = t(c["rows"]).requires_grad_(), t(c["votes"]).requires_grad_()
    xyz = t(c["seed_xyz"]) + votes[:, :3]
    s = rows + votes[:, 3:]
    n = s.norm(dim=-1, keepdim=True)
    y = s / n
    loss = (y * t(c["dy"])).sum() * (1.0 if with_dy else 0.0) + (xyz * t(c["dxyz"])).sum() * (1.0 if with_dxyz else 0.0)
    loss.backward()
    return dict(y=y.detach().numpy(), norm=n.detach().numpy()[:, 0], vote_xyz=xyz.detach().numpy(),
                drows=rows.grad.numpy(), dvotes=votes.grad.numpy())


def l2_reference(c):
    out = ref.l2norm_fwd(c["x"])
    out.update(ref.l2norm_bwd(c["x"], c["dy"]))
    return out


def vote_reference(c, with_dy=True, with_dxyz=True):
    out = ref.vote_fwd(c["rows"], c["votes"], c["seed_xyz"])
    out.update(ref.vote_bwd(c["rows"], c["votes"], c["dy"] if with_dy else None, c["dxyz"] if with_dxyz else None))
    return out


# ---- sampling-location preparation ----------------------------------------------------------------------------------
PREP_HLP = ((1, 1, 1), (2, 4, 2), (8, 4, 2), (8, 4, 4), (64, 1, 1), (3, 3, 5), (6, 8, 2))
PREP_B, PREP_Q = 3, 11      # R = 33: R * H is no multiple of 64 (but for H = 64, where it is no multiple of 256)
PIN = (0.0, 1.0, -2.0 ** -20, 1.0 + 2.0 ** -20, 0.5)
PREP_KINDS = ("random", "gap30", "equal")


def prep_case(H, L, P):
    """Three scenes with their own M, ab and valid ratios.  Scene 0: M = identity, ab = (1, 0, 1, 0) and z = 1, so
    that pw = 1 and u0 = x, v0 = y exactly; its points sit on PIN x PIN (the clamp gate's closed ends, one step
    outside them, the middle).  The other scenes keep u0 / v0 at least 2^-10 off 0 and 1 (a gate that a rounding
    could flip would test nothing) and pw in [0.6, 3.4].  Logits per (row, head): random, one 30 above the rest, all
    equal."""
    B, Q = PREP_B, PREP_Q
    R = B * Q
    rng = _g(100 * H + 10 * L + P)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    M = np.zeros((B, 4, 4), np.float32)
    M[:] = np.eye(4, dtype=np.float32)
    M[1:, :3, :] = (0.1 * r(B - 1, 3, 4)).astype(np.float32)
    M[1:, 0, 0] += 1.0
    M[1:, 1, 1] += 1.0
    M[1:, 2, 2] = 1.0
    M[1:, 2, 3] = 0.0
    M[1:, 2, :2] = np.float32(0.05)
    ab = np.array([[1, 0, 1, 0], [0.9, 0.45, 1.1, 0.5], [-0.7, 0.5, 0.8, 0.55]], np.float32)
    pts = np.empty((R, 3), np.float32)
    pts[:, :2] = (rng.uniform(-2, 2, (R, 2))).astype(np.float32)
    pts[:, 2] = rng.uniform(1.0, 3.0, R).astype(np.float32)
    for i in range(Q):
        pts[i] = (PIN[i % 5], PIN[(2 * i + i // 5) % 5], 1.0)
    vr = rng.uniform(0.6, 1.0, (B, L, 2)).astype(np.float32)
    shapes = np.array([[max(1, 45 >> l) + (l % 2), max(1, 61 >> l) + 2] for l in range(L)], np.int64)
    HLP = H * L * P
    raw = np.empty((R, HLP * 3), np.float32)
    raw[:, :HLP * 2] = 2 * r(R, HLP * 2)
    lg = r(R, H, L * P)
    kind = (np.arange(R)[:, None] + np.arange(H)[None, :]) % 3
    hot = rng.integers(0, L * P, (R, H))
    lg[kind == 2] = np.float32(0.375)
    rr, hh = np.nonzero(kind == 1)
    lg[rr, hh, hot[rr, hh]] += 30.0
    raw[:, HLP * 2:] = lg.reshape(R, HLP)
    c = dict(H=H, L=L, P=P, Q=Q, R=R, pts=pts, M=M.reshape(B, 16), ab=ab, vr=vr, shapes=shapes, raw=raw,
             dloc=r(R, H, L, P, 2), dloc2=(0.5 * r(R, H, L, P, 2)).astype(np.float32), dw=r(R, H, L, P),
             dw2=(0.5 * r(R, H, L, P)).astype(np.float32))
    uvw = ref.prep_fwd(pts, c["M"], ab, vr, shapes, raw, Q, H, L, P)["uvw"][0]
    for k in (0, 1):                                       # re-draw points whose u0 / v0 sits too near a gate end
        near = np.minimum(np.abs(uvw[Q:, k]), np.abs(uvw[Q:, k] - 1)) < 2.0 ** -10
        assert not near.any(), "prep_case(%d, %d, %d): a free point sits on a clamp end" % (H, L, P)
    return c


def prep_cases():
    return {"H%d_L%d_P%d" % s: prep_case(*s) for s in PREP_HLP}


def prep_reference(c, second=True):
    a = (c["pts"], c["M"], c["ab"], c["vr"], c["shapes"], c["raw"])
    k = (c["Q"], c["H"], c["L"], c["P"])
    out = ref.prep_fwd(*a, *k)
    out.update(ref.prep_bwd(*a, c["dloc"], c["dloc2"] if second else None, c["dw"], c["dw2"] if second else None, *k))
    return out


def prep_composition(c, dtype, second=True, strict_gate=False, drop_head=False):
    """Plain tensor arithmetic with autograd.  torch.clamp's own backward passes the gradient on [0, 1];
    ``strict_gate`` restates the clamp with a gate on the OPEN interval, ``drop_head`` leaves the last head out of the
    reference-point gradient: the two deliberately wrong forms."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    H, L, P, Q, R = (c[k] for k in "HLPQR")
    b = torch.arange(R) // Q
    pts = t(c["pts"]).requires_grad_()
    raw = t(c["raw"]).requires_grad_()
    M, ab, vr = t(c["M"]).view(-1, 4, 4)[b], t(c["ab"])[b], t(c["vr"])[b]
    hom = torch.cat([pts, torch.ones(R, 1, dtype=dtype)], 1)
    pr = torch.einsum("rij,rj->ri", M[:, :3], hom)
    xw, yw = pr[:, 0] / pr[:, 2], pr[:, 1] / pr[:, 2]
    uv0 = torch.stack([xw * ab[:, 0] + ab[:, 1], yw * ab[:, 2] + ab[:, 3]], -1)
    if strict_gate:
        inside = ((uv0 > 0) & (uv0 < 1)).to(dtype)
        uv = uv0 * inside + uv0.detach().clamp(0, 1) * (1 - inside)
    else:
        uv = uv0.clamp(0, 1)
    wh = torch.from_numpy(c["shapes"][:, ::-1].copy()).to(dtype)
    off = raw[:, :H * L * P * 2].view(R, H, L, P, 2)
    lg = raw[:, H * L * P * 2:].view(R, H, L * P)
    ref_pt = (uv[:, None] * vr)[:, None, :, None, :].expand(R, H, L, 1, 2)
    if drop_head:
        ref_pt = torch.cat([ref_pt[:, :H - 1], ref_pt[:, H - 1:].detach()], 1)
    loc = ref_pt + off / wh[None, None, :, None, :]
    w = torch.softmax(lg, -1).view(R, H, L, P)
    DL = t(c["dloc"]) + (t(c["dloc2"]) if second else 0)
    DW = t(c["dw"]) + (t(c["dw2"]) if second else 0)
    ((loc * DL).sum() + (w * DW).sum()).backward()
    n = lambda a: a.detach().numpy()
    return dict(loc=n(loc), w=n(w), uvw=n(torch.cat([uv0, xw[:, None], yw[:, None]], 1)), draw=n(raw.grad), dpts=n(pts.grad))


def worst(op, got, want, names=None):
    """{output: worst ratio} of ``got`` (dict of arrays) against ``want`` (dict of (value, scale))."""
    return {k: ref.units(got[k], *want[k]) for k in (names or GROUPS[op]) if k in got}


def over(op, ratios):
    """The outputs whose ratio exceeds their constant."""
    return {k: (v, GROUPS[op][k]) for k, v in ratios.items() if not v <= GROUPS[op][k]}
