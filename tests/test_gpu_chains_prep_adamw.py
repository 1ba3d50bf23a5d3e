"""The float4 forms of the sampling-preparation kernels (csrc/dense.hip, taken at H = 8, L = 4, P = 2 on 16-byte
aligned rows) and the leading-element peel of adamw_state_k (csrc/optim.hip), under the references, bounds and
constants of tests/test_gpu_dense_rows_edges.py and tests/test_gpu_optim_edges.py, whose helpers are reused as they
stand (dense_rows_cases.GROUPS, optim_cases.C_P / C_M / C_V: unchanged).

Sampling preparation: the fast form runs one wave per workgroup, one (row, head) item per lane.  The cases of
dense_rows_cases (33 rows: 264 items at H = 8, past four workgroups and one partial) already pass through it in the
existing test; here: ONE row (8 items, 56 dead lanes whose groups of 8 must stay out of the sum over heads), 8 and 9
rows (exactly one workgroup; one item group past it), the same inputs on rows that are NOT 16-byte aligned (the
present kernel must take them), a non-power-of-two head count and R * H = 1 cut the same way.  Inputs, clamp ends
included, are those of dense_rows_cases.prep_case.

AdamW: a segment whose four pointers share a residue r mod 16 bytes peels (4 - r / 4) % 4 elements; a gradient on
another residue keeps the scalar branch."""
import numpy as np
import pytest

import dense_rows_cases as dc
import optim_cases as oc
import test_gpu_dense_rows_edges as de
import test_gpu_optim_edges as oe

pytestmark = pytest.mark.gpu
F32 = np.float32


# ---- demf_msda_prep_fwd / bwd -------------------------------------------------------------------------------------
def _cut(c, R):
    """The first R rows of a prep_case as scenes of ONE row (Q = 1; the case has three scenes, so R <= 3), or - for
    more rows - the whole first scene followed by rows of the others, Q rows each (R a multiple of Q)."""
    out = dict(c)
    if R <= 3:
        rows = np.array([0, c["Q"], 2 * c["Q"]])[:R]            # one row of every scene: the pinned one first
        out["Q"] = 1
    else:
        q = R // 3
        assert R == 3 * q and q <= c["Q"]
        rows = np.concatenate([np.arange(q) + b * c["Q"] for b in range(3)])
        out["Q"] = q
    out["R"] = R
    for k in ("pts", "raw", "dloc", "dloc2", "dw", "dw2"):
        out[k] = np.ascontiguousarray(c[k][rows])
    return out


def _prep_case(H, L, P, R):
    return _cut(dc.prep_case(H, L, P), R)


def _shifted(a, floats):
    """``a`` on the device at ``floats`` past a 16-byte boundary."""
    base = de._dev(np.concatenate([np.zeros(floats, F32), np.asarray(a, F32).reshape(-1)]))
    view = base[floats:]
    assert view.data_ptr() % 16 == 4 * floats
    return view


class _ShiftedOut(de._Out):
    """de._Out with the output (and its guard bands) moved one float off the 16-byte grid."""

    def __init__(self, shape, pitch, null=False):
        super().__init__(shape, pitch, null=null)
        self.buf = _shifted(self.before, 1)
        self.ptr = None if null else self.buf.data_ptr() + 4 * self.guard


PREP = [(8, 4, 2, 1, 0), (8, 4, 2, 3, 0), (8, 4, 2, 24, 0), (8, 4, 2, 27, 0), (8, 4, 2, 3, 1), (8, 4, 2, 27, 1),
        (6, 8, 2, 1, 0), (3, 3, 5, 3, 0), (1, 1, 1, 1, 0)]
PREP_IDS = ["H%d_L%d_P%d_R%d%s" % (h, l, p, r, "_unaligned" if s else "") for h, l, p, r, s in PREP]


@pytest.mark.parametrize("H,L,P,R,shift", PREP, ids=PREP_IDS)
def test_msda_prep_fwd_fast_form_edges(H, L, P, R, shift):
    c = _prep_case(H, L, P, R)
    Q = c["Q"]
    want = dc.prep_reference(c)
    ins = de._prep_inputs(c)
    raw = _shifted(c["raw"], shift)
    Out = _ShiftedOut if shift else de._Out
    outs = dict(loc=Out((R, H, L, P, 2), H * L * P * 2), w=Out((R, H, L, P), H * L * P), uvw=de._Out((R, 4), 4))
    de._call("demf_msda_prep_fwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], raw.data_ptr(), outs["loc"].ptr,
             outs["w"].ptr, outs["uvw"].ptr)
    got = de._judge("prep_fwd", PREP_IDS[PREP.index((H, L, P, R, shift))], outs, want)
    q = slice(0, Q)                                   # the pinned scene: u0 = x and v0 = y to the bit
    assert np.array_equal(de._bits(got["uvw"][q, :2]), de._bits(c["pts"][q, :2]))


@pytest.mark.parametrize("form", ["all", "null_dpts", "null_dloc2_dw2", "null_dpts_dloc2_dw2"])
@pytest.mark.parametrize("H,L,P,R,shift", PREP, ids=PREP_IDS)
def test_msda_prep_bwd_fast_form_edges(H, L, P, R, shift, form):
    c = _prep_case(H, L, P, R)
    Q = c["Q"]
    second, with_dpts = "dloc2" not in form, "dpts" not in form
    want = dc.prep_reference(c, second=second)
    ins = de._prep_inputs(c)
    w32, uvw32 = de._dev(want["w"][0].astype(F32)), de._dev(want["uvw"][0].astype(F32))
    g = {k: _shifted(c[k], shift) for k in ("dloc", "dloc2", "dw", "dw2")}
    Out = _ShiftedOut if shift else de._Out
    outs = dict(draw=Out((R, H * L * P * 3), H * L * P * 3), dpts=de._Out((R, 3), 3, null=not with_dpts))
    de._call("demf_msda_prep_bwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], w32.data_ptr(), uvw32.data_ptr(),
             g["dloc"].data_ptr(), g["dloc2"].data_ptr() if second else None, g["dw"].data_ptr(),
             g["dw2"].data_ptr() if second else None, outs["draw"].ptr, outs["dpts"].ptr)
    de._judge("prep_bwd", "%s %s" % (PREP_IDS[PREP.index((H, L, P, R, shift))], form), outs, want)


def test_msda_prep_fast_form_and_present_kernel_agree_to_the_bit():
    """Same arithmetic term by term: the aligned call (fast form) and the call on rows one float off the grid (the
    present kernel) return the same bits, forward and backward."""
    H, L, P, R = 8, 4, 2, 27
    c = _prep_case(H, L, P, R)
    Q = c["Q"]
    ins = de._prep_inputs(c)
    want = dc.prep_reference(c)
    w32, uvw32 = de._dev(want["w"][0].astype(F32)), de._dev(want["uvw"][0].astype(F32))
    got = []
    for shift in (0, 1):
        Out = _ShiftedOut if shift else de._Out
        raw = _shifted(c["raw"], shift)
        g = {k: _shifted(c[k], shift) for k in ("dloc", "dloc2", "dw", "dw2")}
        o = dict(loc=Out((R, H, L, P, 2), 128), w=Out((R, H, L, P), 64), uvw=de._Out((R, 4), 4),
                 draw=Out((R, 192), 192), dpts=de._Out((R, 3), 3))
        de._call("demf_msda_prep_fwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], raw.data_ptr(), o["loc"].ptr,
                 o["w"].ptr, o["uvw"].ptr)
        de._call("demf_msda_prep_bwd", R, Q, H, L, P, *[t.data_ptr() for t in ins], w32.data_ptr(), uvw32.data_ptr(),
                 g["dloc"].data_ptr(), g["dloc2"].data_ptr(), g["dw"].data_ptr(), g["dw2"].data_ptr(), o["draw"].ptr,
                 o["dpts"].ptr)
        got.append({k: de._bits(v.get()) for k, v in o.items()})
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


# ---- demf_adamw_state_f32 -------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024, 1025)


@pytest.mark.parametrize("res", [0, 1, 2, 3])
def test_state_adamw_peel_geometry(res):
    """One segment that starts ``res`` floats past a 16-byte boundary of all four buffers, every length around the
    peel (1-9: shorter than the peel, the peel alone, peel + one float4, + tail) and around one workgroup; sentinel
    floats in front of and behind the segment keep their bits (checked by _check_step)."""
    for n in LENGTHS:
        start = 4 + res
        segs = [(start, n, oe.LRS[0], oe.WDS[0])]
        oe._run_state("peel_r%d_n%d" % (res, n), segs, start + n + 5, seed=100 * res + n)


@pytest.mark.parametrize("res", [1, 3])
def test_state_adamw_peel_on_shifted_buffers(res):
    """The residue from the buffers' own base, not from the segment start: all four at +res floats, segments at
    multiples of four and off them."""
    segs, total = oe._segments((7, 1025, 1024), "contiguous")
    oe._run_state("peel_bases_%d" % res, segs, total, seed=7 + res, offs=(res, res, res, res))


@pytest.mark.parametrize("offs", [(0, 1, 0, 0), (0, 0, 2, 0), (3, 3, 3, 0)], ids=["g", "m", "v"])
def test_state_adamw_mixed_residues_keep_the_scalar_path(offs):
    segs = [(3, 1025, oe.LRS[0], oe.WDS[0]), (3 + 1025 + 2, 9, oe.LRS[1], oe.WDS[1])]
    oe._run_state("mixed_%d%d%d%d" % offs, segs, 3 + 1025 + 2 + 9 + 3, seed=21, offs=offs)


def test_state_adamw_model_pair():
    """The full model's two groups by their numbers: 1 150 679 elements, then 1 039 296 that start 3 mod 4."""
    n0, n1 = 1_150_679, 1_039_296
    assert n0 % 4 == 3
    segs = [(0, n0, 0.008, 0.01), (n0, n1, 0.0004, 0.01)]
    oe._run_state("model_pair", segs, n0 + n1, seed=78)
