"""The row kernels of csrc/dense.hip and rows_ln_pos_kernel (csrc/rows_gemm.hip), launched directly through
_ffi.call, against the float64 restatement of tests/dense_rows_reference.py: every width the dispatchers instantiate,
row counts around the 4-rows-per-block tail and the LayerNorm backward's rows_per_wave steps, every optional argument
present and null, accumulating outputs on top of a prefill, the dropout mask bit for bit against the host hash.

Pass rule, for EVERY element of every output: |got - ref64| <= C * 2^-24 * scale + 2^-126 (scales: docstring of
dense_rows_reference; constants and their measurement: tests/dense_rows_cases.py).  Every output lives between
sentinel guard bands of at least four rows, which must keep their bits; an output passed as null is allocated all the
same and must keep its sentinels too.  Every check prints its worst ratio per output before asserting."""
import functools

import numpy as np
import pytest
import torch

import dense_rows_cases as dc
import dense_rows_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
BAD_WIDTHS = (0, 32, 63, 65, 96, 127, 130, 192, 320, 1030, 1088, 2048)


def _call(name, *args):
    from demf_amd import _ffi
    _ffi.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rng_state():
    return _dev(np.array([dc.RNG_SEED, dc.RNG_STEP], np.uint64).view(np.int64))


class _Out:
    """``n`` floats between two sentinel bands of ``guard`` floats (the `_place` pattern of test_gpu_optim_edges):
    .ptr for the kernel (None when ``null``: allocated but not passed), .get() the values, .check() the bands."""

    def __init__(self, shape, pitch, fill=None, null=False):
        self.shape, self.n = shape, int(np.prod(shape))
        self.guard = max(4 * pitch, 16)
        host = np.full(self.guard + self.n + self.guard, dc.SENTINEL, F32)
        if fill is not None:
            host[self.guard:self.guard + self.n] = np.asarray(fill, F32).reshape(-1)
        self.before = host
        self.buf = _dev(host)
        self.null = null
        self.ptr = None if null else self.buf.data_ptr() + 4 * self.guard

    def get(self):
        return self.buf.cpu().numpy()[self.guard:self.guard + self.n].reshape(self.shape)

    def check(self, label):
        got = _bits(self.buf.cpu().numpy())
        want = _bits(self.before)
        inner = slice(self.guard, self.guard + self.n)
        assert np.array_equal(got[:self.guard], want[:self.guard]), label + ": band in front was written"
        assert np.array_equal(got[inner.stop:], want[inner.stop:]), label + ": band behind was written"
        if self.null:
            assert np.array_equal(got[inner], want[inner]), label + ": a null output was written"


def _judge(op, label, outs, want, extra=None):
    """outs: {name: _Out}; ``want``: {name: (value, scale)}.  Bands first, then every element of every output."""
    torch.cuda.synchronize()
    got = {}
    for k, o in outs.items():
        o.check("%s %s" % (label, k))
        if not o.null:
            got[k] = o.get()
    if extra:
        got.update(extra)
    ratios = dc.worst(op, got, want, names=list(got))
    print("dense-rows %-12s %-34s %s" % (op, label, "  ".join("%s %.2f (C %g)" % (k, v, dc.GROUPS[op][k])
                                                                 for k, v in ratios.items())))
    bad = dc.over(op, ratios)
    assert not bad, "%s %s: worst ratio over its constant: %s" % (op, label, bad)
    return got


# ---- demf_dropout_mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", dc.P_DROP)
@pytest.mark.parametrize("op,n", [(3, 1), (77, 255), (1001, 1000), (0x7FFFFFF1, 66_001)])
def test_dropout_mask_bit_exact(op, n, p):
    out = _Out((n,), 4)
    _call("demf_dropout_mask", n, float(p), _rng_state().data_ptr(), op, out.ptr)
    torch.cuda.synchronize()
    out.check("dropout_mask")
    want = ref.dropout_scale(dc.RNG_SEED, dc.RNG_STEP, op, 0, n, p)
    bad = np.flatnonzero(_bits(out.get()) != _bits(want))
    assert bad.size == 0, "op %d p %g: first wrong element %d of %d, %d wrong" % (op, p, bad[0], n, bad.size)
    if p > 0 and n >= 255:
        assert 0 < np.count_nonzero(want) < n


# ---- demf_add_dropout_ln_fwd / bwd ----------------------------------------------------------------------------------
LN_CASES = dc.ln_cases()
LN_FORM_CASES = ("R5_C64", "R1025_C256")


@functools.lru_cache(maxsize=4)
def _ln_ref(name, p, identity=True, dy2=True, accum=True, prefill=True):
    c = LN_CASES[name]
    x = c["x"] if identity else (c["x"] + c["identity"]).astype(F32)          # (on the grid: the sum is exact)
    ident = c["identity"] if identity else None
    if not identity:
        assert np.array_equal(x.astype(np.float64), c["x"].astype(np.float64) + c["identity"])
    mask = dc.mask_for(c["op"], c["R"] * c["C"], p)
    out = ref.ln_fwd(x, ident, c["gamma"], c["beta"], dc.EPS, mask)
    out.update(ref.ln_bwd(c["dy"], c["dy2"] if dy2 else None, x, ident, c["gamma"], dc.EPS, mask,
                          c["ds_prev"] if accum else None, c["dgamma0"] if prefill else None,
                          c["dbeta0"] if prefill else None))
    return x, out


def _run_ln_fwd(name, p, identity=True, keep=True, alias=False):
    c = LN_CASES[name]
    R, C = c["R"], c["C"]
    x, want = _ln_ref(name, p, identity)
    xin = _Out((R, C), C, fill=x)                                # (in a guarded buffer: it may double as s_out)
    outs = dict(y=_Out((R, C), C), s=xin if alias else _Out((R, C), C, null=not keep),
                stats=_Out((R, 2), 2, null=not keep))
    ident = _dev(c["identity"]) if identity else None
    gamma, beta, rng = _dev(c["gamma"]), _dev(c["beta"]), _rng_state()
    _call("demf_add_dropout_ln_fwd", R, C, xin.ptr, None if ident is None else ident.data_ptr(), gamma.data_ptr(),
          beta.data_ptr(), float(dc.EPS), float(p), rng.data_ptr() if p > 0 else None, c["op"], outs["s"].ptr,
          outs["y"].ptr, outs["stats"].ptr)
    torch.cuda.synchronize()
    label = "%s p%g%s%s%s" % (name, p, "" if identity else " id0", "" if keep else " nokeep", " alias" if alias else "")
    stats = outs.pop("stats")
    stats.check(label + " stats")
    extra = {} if stats.null else dict(mean=stats.get()[:, 0], rstd=stats.get()[:, 1])
    if not alias:
        xin.check(label + " x")
        assert np.array_equal(_bits(xin.get()), _bits(x)), label + ": x was written"
    got = _judge("ln_fwd", label, outs, want, extra)
    # a constant row (variance exactly 0): y is beta to the bit.  (Without an identity the constant sits in x, and
    # dropout breaks the row up: those runs are judged by the bound alone.)
    const = np.flatnonzero(c["kind"] == 3) if identity or p == 0 else np.zeros(0, np.int64)
    assert np.array_equal(_bits(got["y"][const]), _bits(np.broadcast_to(c["beta"], (const.size, C)))), label
    if "mean" in got:
        assert np.array_equal(got["mean"][const], np.full(const.size, 100.0, F32)), label


@pytest.mark.parametrize("name", list(LN_CASES))
def test_add_dropout_ln_fwd(name):
    for p in dc.P_DROP:
        _run_ln_fwd(name, p)


@pytest.mark.parametrize("form", ["null_identity", "null_s_out_and_stats", "s_out_aliases_x", "alias_null_identity"])
@pytest.mark.parametrize("name", LN_FORM_CASES)
def test_add_dropout_ln_fwd_forms(name, form):
    kw = dict(null_identity=dict(identity=False), null_s_out_and_stats=dict(keep=False), s_out_aliases_x=dict(alias=True),
              alias_null_identity=dict(alias=True, identity=False))[form]
    for p in dc.P_DROP:
        _run_ln_fwd(name, p, **kw)


def _run_ln_bwd(name, p, dy2=True, accum=True, prefill=True, ds=True, dx=True):
    """The kernel starts from the fp32 roundings of the reference's s and stats."""
    c = LN_CASES[name]
    R, C = c["R"], c["C"]
    _, want = _ln_ref(name, p, True, dy2, accum, prefill)
    s32 = want["s"][0].astype(F32)
    stats32 = np.stack([want["mean"][0], want["rstd"][0]], -1).astype(F32)
    g0 = c["dgamma0"] if prefill else np.zeros(C, F32)
    b0 = c["dbeta0"] if prefill else np.zeros(C, F32)
    outs = dict(ds=_Out((R, C), C, fill=c["ds_prev"] if accum else None, null=not ds), dx=_Out((R, C), C, null=not dx),
                dgamma=_Out((C,), C, fill=g0), dbeta=_Out((C,), C, fill=b0))
    ins = [_dev(a) for a in (c["dy"], c["dy2"], s32, stats32, c["gamma"])]
    rng = _rng_state()
    _call("demf_add_dropout_ln_bwd", R, C, ins[0].data_ptr(), ins[1].data_ptr() if dy2 else None, ins[2].data_ptr(),
          ins[3].data_ptr(), ins[4].data_ptr(), float(p), rng.data_ptr() if p > 0 else None, c["op"], outs["ds"].ptr,
          1 if accum else 0, outs["dx"].ptr, outs["dgamma"].ptr, outs["dbeta"].ptr)
    label = "%s p%g%s%s%s%s%s" % (name, p, "" if dy2 else " dy2=0", "" if accum else " store", "" if prefill else " from0",
                                  "" if ds else " ds=0", "" if dx else " dx=0")
    got = _judge("ln_bwd", label, outs, want)
    # the accumulating outputs, as increments over what they held
    for k, pre in (("dgamma", g0), ("dbeta", b0)):
        inc = ref.units(got[k].astype(np.float64) - pre, want[k][0] - pre, want[k][1])
        assert inc <= dc.C_LN_DGB, (label, k, "increment", inc)


@pytest.mark.parametrize("name", list(LN_CASES))
def test_add_dropout_ln_bwd(name):
    """dy + dy2, ds added onto what ds_out held, dx through the mask, dgamma / dbeta on top of a non-zero prefill."""
    for p in dc.P_DROP:
        _run_ln_bwd(name, p)


@pytest.mark.parametrize("form", ["no_dy2_store_from0", "null_ds_out", "null_dx_out", "null_ds_out_and_dx_out"])
@pytest.mark.parametrize("name", LN_FORM_CASES)
def test_add_dropout_ln_bwd_forms(name, form):
    kw = dict(no_dy2_store_from0=dict(dy2=False, accum=False, prefill=False), null_ds_out=dict(ds=False),
              null_dx_out=dict(dx=False), null_ds_out_and_dx_out=dict(ds=False, dx=False))[form]
    for p in dc.P_DROP:
        _run_ln_bwd(name, p, **kw)


# ---- demf_rows_ln_pos_f32 -------------------------------------------------------------------------------------------
RLP_CASES = dc.rlp_cases()


def _run_rlp(name, gamma=True, resid=True, y=True, ypos=True):
    c = RLP_CASES[name]
    R = c["R"]
    want = ref.rows_ln_pos(c["x"], c["resid"] if resid else None, c["gamma"] if gamma else None,
                           c["beta"] if gamma else None, dc.EPS, c["pos"])
    outs = dict(y=_Out((R, 256), 256, null=not y), ypos=_Out((R, 256), 256, null=not ypos))
    ins = {k: _dev(c[k]) for k in ("x", "resid", "gamma", "beta", "pos")}
    _call("demf_rows_ln_pos_f32", R, 256, ins["x"].data_ptr(), ins["resid"].data_ptr() if resid else None,
          ins["gamma"].data_ptr() if gamma else None, ins["beta"].data_ptr() if gamma else None, float(dc.EPS),
          ins["pos"].data_ptr(), outs["y"].ptr, outs["ypos"].ptr)
    _judge("rows_ln_pos", "%s g%d r%d y%d yp%d" % (name, gamma, resid, y, ypos), outs, want)


@pytest.mark.parametrize("name", list(RLP_CASES))
def test_rows_ln_pos(name):
    _run_rlp(name)


@pytest.mark.parametrize("form", ["null_gamma", "null_y", "null_ypos", "null_resid", "null_gamma_and_resid"])
@pytest.mark.parametrize("name", ["R5", "R1025"])
def test_rows_ln_pos_forms(name, form):
    _run_rlp(name, **dict(null_gamma=dict(gamma=False), null_y=dict(y=False), null_ypos=dict(ypos=False),
                          null_resid=dict(resid=False), null_gamma_and_resid=dict(gamma=False, resid=False))[form])


# ---- demf_softmax_dropout_fwd / bwd ---------------------------------------------------------------------------------
SM_CASES = dc.sm_cases()


@pytest.mark.parametrize("name", list(SM_CASES))
def test_softmax_dropout_fwd_bwd(name):
    c = SM_CASES[name]
    R, S = c["R"], c["S"]
    sc, rng = _dev(c["scores"]), _rng_state()
    for p in dc.P_DROP:
        want = dc.sm_reference(c, p)
        outs = dict(prob=_Out((R, S), S), out=_Out((R, S), S))
        _call("demf_softmax_dropout_fwd", R, S, sc.data_ptr(), float(p), rng.data_ptr() if p > 0 else None, c["op"],
              outs["prob"].ptr, outs["out"].ptr)
        _judge("softmax_fwd", "%s p%g" % (name, p), outs, want)
        prob32 = _dev(want["prob"][0].astype(F32))
        dio = _Out((R, S), S, fill=c["dout"])
        _call("demf_softmax_dropout_bwd", R, S, prob32.data_ptr(), float(p), rng.data_ptr() if p > 0 else None, c["op"],
              dio.ptr)
        _judge("softmax_bwd", "%s p%g" % (name, p), dict(dscores=dio), want)


@pytest.mark.parametrize("S", sorted({s for _, s in dc.SM_SHAPES}))
def test_softmax_forward_and_backward_draw_the_host_mask(S):
    """All-zero logits make out = mask / S; prob = 2^-20 everywhere and dout = 1 make the backward's result positive
    exactly where the element was kept (dot <= 1024 * 2^-20 * 5/3 < 1).  Both against the ONE host mask."""
    R, p, op = 5, 0.4, 900 + S
    keep = ref.dropout_keep(dc.RNG_SEED, dc.RNG_STEP, op, 0, R * S, p).reshape(R, S)
    rng = _rng_state()
    prob, out = _Out((R, S), S), _Out((R, S), S)
    _call("demf_softmax_dropout_fwd", R, S, _dev(np.zeros((R, S), F32)).data_ptr(), p, rng.data_ptr(), op, prob.ptr, out.ptr)
    dio = _Out((R, S), S, fill=np.ones((R, S), F32))
    _call("demf_softmax_dropout_bwd", R, S, _dev(np.full((R, S), 2.0 ** -20, F32)).data_ptr(), p, rng.data_ptr(), op, dio.ptr)
    torch.cuda.synchronize()
    for o in (prob, out, dio):
        o.check("S%d" % S)
    assert np.array_equal(out.get() != 0, keep), "forward mask, S %d" % S
    assert np.array_equal(dio.get() > 0, keep), "backward mask, S %d" % S


# ---- demf_msda_prep_fwd / bwd ---------------------------------------------------------------------------------------
PREP_CASES = dc.prep_cases()


def _prep_inputs(c):
    return [_dev(c[k]) for k in ("pts", "M", "ab", "vr", "shapes")]


@pytest.mark.parametrize("name", list(PREP_CASES))
def test_msda_prep_fwd(name):
    c = PREP_CASES[name]
    R, Q, H, L, P = (c[k] for k in "RQHLP")
    want = dc.prep_reference(c)
    ins, raw = _prep_inputs(c), _dev(c["raw"])
    outs = dict(loc=_Out((R, H, L, P, 2), H * L * P * 2), w=_Out((R, H, L, P), H * L * P), uvw=_Out((R, 4), 4))
    _call("demf_msda_prep_fwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], raw.data_ptr(), outs["loc"].ptr,
          outs["w"].ptr, outs["uvw"].ptr)
    got = _judge("prep_fwd", name, outs, want)
    q = slice(0, Q)                                   # the pinned scene: u0 = x and v0 = y to the bit
    assert np.array_equal(_bits(got["uvw"][q, :2]), _bits(c["pts"][q, :2])), name


@pytest.mark.parametrize("form", ["all", "null_dpts", "null_dloc2_dw2", "null_dpts_dloc2_dw2"])
@pytest.mark.parametrize("name", list(PREP_CASES))
def test_msda_prep_bwd(name, form):
    """w and uvw arrive as the fp32 roundings of the reference's; on the pinned scene uvw holds 0, 1 and their
    neighbours exactly, so the clamp gate is judged on its closed ends."""
    c = PREP_CASES[name]
    R, Q, H, L, P = (c[k] for k in "RQHLP")
    second, with_dpts = "dloc2" not in form, "dpts" not in form
    want = dc.prep_reference(c, second=second)
    ins = _prep_inputs(c)
    w32, uvw32 = _dev(want["w"][0].astype(F32)), _dev(want["uvw"][0].astype(F32))
    g = {k: _dev(c[k]) for k in ("dloc", "dloc2", "dw", "dw2")}
    outs = dict(draw=_Out((R, H * L * P * 3), H * L * P * 3), dpts=_Out((R, 3), 3, null=not with_dpts))
    _call("demf_msda_prep_bwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], w32.data_ptr(), uvw32.data_ptr(),
          g["dloc"].data_ptr(), g["dloc2"].data_ptr() if second else None, g["dw"].data_ptr(),
          g["dw2"].data_ptr() if second else None, outs["draw"].ptr, outs["dpts"].ptr)
    got = _judge("prep_bwd", "%s %s" % (name, form), outs, want)
    if with_dpts:                                     # outside the closed interval nothing passes: exact zeros
        u0, v0 = want["uvw"][0][:, 0], want["uvw"][0][:, 1]
        dead = ((u0 < 0) | (u0 > 1)) & ((v0 < 0) | (v0 > 1))
        assert dead[:Q].any() and not got["dpts"][dead].any(), name


# ---- demf_l2norm_rows_fwd / bwd, demf_vote_combine_fwd / bwd --------------------------------------------------------
L2_CASES = dc.l2_cases()


def _only_the_zero_row_is_non_finite(c, arr, label):
    fin = np.isfinite(arr.reshape(c["R"], -1)).all(-1)
    want = np.ones(c["R"], bool)
    if c["zero"] is not None:
        want[c["zero"]] = False
    assert np.array_equal(fin, want), label


@pytest.mark.parametrize("name", list(L2_CASES))
def test_l2norm_rows_fwd_bwd(name):
    c = L2_CASES[name]
    R, C = c["R"], c["C"]
    want = dc.l2_reference(c)
    x = _dev(c["x"])
    outs = dict(y=_Out((R, C), C), norm=_Out((R,), 1))
    _call("demf_l2norm_rows_fwd", R, C, x.data_ptr(), outs["y"].ptr, outs["norm"].ptr)
    got = _judge("l2_fwd", name, outs, want)
    _only_the_zero_row_is_non_finite(c, got["y"], name + " y")
    assert np.isfinite(got["norm"]).all()
    y32, n32, dy = _dev(want["y"][0].astype(F32)), _dev(want["norm"][0].astype(F32)), _dev(c["dy"])
    outs = dict(dx=_Out((R, C), C))
    _call("demf_l2norm_rows_bwd", R, C, y32.data_ptr(), n32.data_ptr(), dy.data_ptr(), outs["dx"].ptr)
    got = _judge("l2_bwd", name, outs, want)
    _only_the_zero_row_is_non_finite(c, got["dx"], name + " dx")


@pytest.mark.parametrize("name", list(L2_CASES))
def test_vote_combine_fwd(name):
    c = L2_CASES[name]
    R, C = c["R"], c["C"]
    want = dc.vote_reference(c)
    ins = [_dev(c[k]) for k in ("rows", "votes", "seed_xyz")]
    outs = dict(vote_xyz=_Out((R, 3), 3), y=_Out((R, C), C), norm=_Out((R,), 1))
    _call("demf_vote_combine_fwd", R, C, *[t.data_ptr() for t in ins], outs["vote_xyz"].ptr, outs["y"].ptr,
          outs["norm"].ptr)
    got = _judge("vote_fwd", name, outs, want)
    _only_the_zero_row_is_non_finite(c, got["y"], name + " y")
    assert np.isfinite(got["vote_xyz"]).all() and np.isfinite(got["norm"]).all()


@pytest.mark.parametrize("name,form", [(n, "all") for n in L2_CASES] +
                         [(n, f) for n in ("R5_C64", "R1025_C128", "zero_R5_C256", "R1_C1024") for f in ("null_dy", "null_dxyz")])
def test_vote_combine_bwd(name, form):
    c = L2_CASES[name]
    R, C = c["R"], c["C"]
    with_dy, with_dxyz = form != "null_dy", form != "null_dxyz"
    want = dc.vote_reference(c, with_dy, with_dxyz)
    y32, n32 = _dev(want["y"][0].astype(F32)), _dev(want["norm"][0].astype(F32))
    dy, dxyz = _dev(c["dy"]), _dev(c["dxyz"])
    outs = dict(dvotes=_Out((R, C + 3), C + 3), drows=_Out((R, C), C))
    _call("demf_vote_combine_bwd", R, C, y32.data_ptr(), n32.data_ptr(), dy.data_ptr() if with_dy else None,
          dxyz.data_ptr() if with_dxyz else None, outs["dvotes"].ptr, outs["drows"].ptr)
    got = _judge("vote_bwd", "%s %s" % (name, form), outs, want)
    _only_the_zero_row_is_non_finite(c, got["drows"], name + " drows")
    want3 = c["dxyz"] if with_dxyz else np.zeros((R, 3), F32)
    assert np.array_equal(got["dvotes"][:, :3], want3), name                 # copied (or zero-filled), not computed
    assert np.array_equal(_bits(got["dvotes"][:, 3:]), _bits(got["drows"])), name


# ---- widths that are no multiple of 64 ------------------------------------------------------------------------------
def _width_call(entry, R, C, n):
    """-> (argument tuple, outputs) with every buffer at the full max(R * C, 1) (+ 3 per row for the vote rows), so
    that a launch that did go out would stay in bounds."""
    i = lambda m=n: _dev(np.full(max(m, 1), 0.5, F32))
    o = lambda m=n: _Out((max(m, 1),), max(C, 4))
    if entry == "demf_add_dropout_ln_fwd":
        ins, outs = [i(), i(), i(), i()], [o(), o(), o(2 * R)]
        args = (ins[0], ins[1], ins[2], ins[3], float(dc.EPS), 0.0, None, 1, outs[0], outs[1], outs[2])
    elif entry == "demf_add_dropout_ln_bwd":
        ins, outs = [i(), i(), i(), i(2 * R), i()], [o(), o(), o(), o()]
        args = (ins[0], ins[1], ins[2], ins[3], ins[4], 0.0, None, 1, outs[0], 0, outs[1], outs[2], outs[3])
    elif entry == "demf_l2norm_rows_fwd":
        ins, outs = [i()], [o(), o(R)]
        args = (ins[0], outs[0], outs[1])
    elif entry == "demf_l2norm_rows_bwd":
        ins, outs = [i(), i(R), i()], [o()]
        args = (ins[0], ins[1], ins[2], outs[0])
    elif entry == "demf_vote_combine_fwd":
        ins, outs = [i(), i(n + 3 * R), i(3 * R)], [o(3 * R), o(), o(R)]
        args = (ins[0], ins[1], ins[2], outs[0], outs[1], outs[2])
    else:
        ins, outs = [i(), i(R), i(), i(3 * R)], [o(n + 3 * R), o()]
        args = (ins[0], ins[1], ins[2], ins[3], outs[0], outs[1])
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a.ptr if isinstance(a, _Out) else a
    return tuple(ptr(a) for a in args), outs, ins


@pytest.mark.parametrize("C", BAD_WIDTHS)
@pytest.mark.parametrize("entry", ["demf_add_dropout_ln_fwd", "demf_add_dropout_ln_bwd", "demf_l2norm_rows_fwd",
                                   "demf_l2norm_rows_bwd", "demf_vote_combine_fwd", "demf_vote_combine_bwd"])
def test_row_kernels_reject_other_widths(entry, C):
    """Only 64 / 128 / 256 / 512 / 1024 channels have a kernel: anything else raises and writes nothing - a width
    between two of them must not round down to the narrower kernel (wrong row pitch, silent garbage)."""
    R = 8
    args, outs, ins = _width_call(entry, R, C, R * C)
    with pytest.raises(RuntimeError, match="channels unsupported"):
        _call(entry, R, C, *args)
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        out.check("%s C %d output %d" % (entry, C, k))
        assert np.array_equal(_bits(out.buf.cpu().numpy()), _bits(out.before)), (entry, C, k)


@pytest.mark.parametrize("C", [96, 130])
def test_ops_surface_the_width_error(C):
    from demf_amd import ops
    g = torch.Generator().manual_seed(C)
    R = 8
    with pytest.raises(RuntimeError, match="channels unsupported"):
        ops.l2norm_rows(torch.randn(R, C, generator=g).cuda())
    with pytest.raises(RuntimeError, match="channels unsupported"):
        ops.vote_combine(torch.randn(R, C, generator=g).cuda(), torch.randn(R, C + 3, generator=g).cuda(),
                         torch.randn(1, R, 3, generator=g).cuda())
