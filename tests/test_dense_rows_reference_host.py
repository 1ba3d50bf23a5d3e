"""The fp64 row-kernel reference (tests/dense_rows_reference.py) on the CPU: its closed-form backward formulas against
torch autograd in float64, the measurement of what an fp32 evaluation of the same operations costs (the number the
GPU tests' constants are derived from), four deliberately wrong fp32 restatements that the chosen inputs must expose,
and the host restatement of csrc/rng.h against keep bits recorded from the library."""
import json
import os

import numpy as np
import pytest
import torch

import dense_rows_cases as dc
import dense_rows_reference as ref

F64, F32 = torch.float64, torch.float32
# fp64 autograd against the fp64 closed forms: 2^-20 of a unit of 2^-24 * scale (~ 2^-44 relative, 500 fp64 roundings)
EXACT = 2.0 ** -20


@pytest.fixture(scope="module")
def refs():
    """(operation, case name, variant) -> (case, reference outputs); computed once, never modified."""
    out = {}
    for n, c in dc.ln_cases().items():
        for p in dc.P_DROP:
            out["ln", n, p] = (c, dc.ln_reference(c, p))
    for n, c in dc.rlp_cases().items():
        out["rlp", n, None] = (c, ref.rows_ln_pos(c["x"], c["resid"], c["gamma"], c["beta"], dc.EPS, c["pos"]))
    for n, c in dc.sm_cases().items():
        for p in dc.P_DROP:
            out["sm", n, p] = (c, dc.sm_reference(c, p))
    for n, c in dc.l2_cases().items():
        out["l2", n, None] = (c, dc.l2_reference(c))
        out["vote", n, None] = (c, dc.vote_reference(c))
    for n, c in dc.prep_cases().items():
        out["prep", n, None] = (c, dc.prep_reference(c))
    return out


def _compose(kind, c, variant, dtype):
    """-> [(operation of dc.GROUPS, composition outputs)]"""
    if kind == "ln":
        o = dc.ln_composition(c, dtype, variant)
        return [("ln_fwd", o), ("ln_bwd", o)]
    if kind == "rlp":
        return [("rows_ln_pos", dc.rlp_composition(c, dtype))]
    if kind == "sm":
        o = dc.sm_composition(c, dtype, variant)
        return [("softmax_fwd", o), ("softmax_bwd", o)]
    if kind == "l2":
        o = dc.l2_composition(c, dtype)
        return [("l2_fwd", o), ("l2_bwd", o)]
    if kind == "vote":
        o = dc.vote_composition(c, dtype)
        return [("vote_fwd", o), ("vote_bwd", o)]
    o = dc.prep_composition(c, dtype)
    return [("prep_fwd", o), ("prep_bwd", o)]


def test_closed_forms_match_autograd_fp64(refs):
    for (kind, name, variant), (c, want) in refs.items():
        for op, got in _compose(kind, c, variant, F64):
            for k, v in dc.worst(op, got, want).items():
                assert v <= EXACT, (kind, name, variant, op, k, v)


def test_reference_variants_match_autograd_fp64():
    """The argument forms the GPU tests use beyond the default: no second gradient in the sampling preparation, a
    null dy / dxyz in the vote tail, rows_ln_pos without gamma or residual."""
    for n, c in dc.prep_cases().items():
        got = dc.prep_composition(c, F64, second=False)
        for k, v in dc.worst("prep_bwd", got, dc.prep_reference(c, second=False)).items():
            assert v <= EXACT, (n, k, v)
    c = dc.l2_case(5, 64)
    for with_dy, with_dxyz in ((False, True), (True, False)):
        got = dc.vote_composition(c, F64, with_dy, with_dxyz)
        for k, v in dc.worst("vote_bwd", got, dc.vote_reference(c, with_dy, with_dxyz)).items():
            assert v <= EXACT, (with_dy, with_dxyz, k, v)
    c = dc.rlp_case(5)
    for with_gamma, with_resid in ((False, True), (True, False), (False, False)):
        want = ref.rows_ln_pos(c["x"], c["resid"] if with_resid else None, c["gamma"] if with_gamma else None,
                               c["beta"] if with_gamma else None, dc.EPS, c["pos"])
        for k, v in dc.worst("rows_ln_pos", dc.rlp_composition(c, F64, with_gamma, with_resid), want).items():
            assert v <= EXACT, (with_gamma, with_resid, k, v)


def test_special_rows_of_the_reference(refs):
    """A constant LayerNorm row gives y == beta and rstd == 1 / sqrt(eps); an all-zero L2 row is non-finite, its
    neighbours are finite."""
    c, want = refs["ln", "R5_C256", 0.0]
    i = int(np.flatnonzero(c["kind"] == 3)[0])
    assert np.array_equal(want["y"][0][i], c["beta"].astype(np.float64))
    assert want["rstd"][0][i] == 1.0 / np.sqrt(float(np.float32(dc.EPS)))
    for kind in ("l2", "vote"):
        c, want = refs[kind, "zero_R5_C256", None]
        fin = np.isfinite(want["y"][0]).all(-1)
        assert not fin[c["zero"]] and fin.sum() == c["R"] - 1


def test_fp32_composition_sets_the_constants(refs):
    """What ANY fp32 evaluation costs, in units of 2^-24 * scale: the torch composition in float32 on the CPU
    against the fp64 reference, over every case.  The constants of dense_rows_cases are 4x this, rounded up to a
    power of two, so the composition has to stay within a quarter of each."""
    w = {}
    for (kind, name, variant), (c, want) in refs.items():
        for op, got in _compose(kind, c, variant, F32):
            for k, v in dc.worst(op, got, want).items():
                key = (op, k)
                if v > w.get(key, (-1.0, None))[0]:
                    w[key] = (v, name)
    for (op, k), (v, name) in sorted(w.items()):
        print("fp32 composition %-12s %-8s %8.2f of %6g  (%s)" % (op, k, v, dc.GROUPS[op][k], name))
    bad = {key: v for key, (v, _) in w.items() if not v <= dc.GROUPS[key[0]][key[1]] / 4}
    assert not bad, bad


def test_wrong_restatements_exceed_their_bounds(refs):
    """Each fault below, restated in fp32, must exceed its bound on at least one case - the inputs can see it."""
    hit = lambda op, kinds, make, names: any(
        dc.over(op, dc.worst(op, make(c, v), want, names)) for (k, _, v), (c, want) in refs.items() if k == kinds)
    assert hit("ln_fwd", "ln", lambda c, p: dc.ln_composition(c, F32, p, one_pass=True), ("y",)), "one-pass variance"
    assert hit("softmax_fwd", "sm", lambda c, p: dc.sm_composition(c, F32, p, no_max=True), ("prob",)), "no max subtraction"
    assert hit("prep_bwd", "prep", lambda c, _: dc.prep_composition(c, F32, strict_gate=True), ("dpts",)), "strict clamp gate"
    # the strict gate must be caught by the pinned points alone: every case, rows of scene 0 only
    for (k, name, _), (c, want) in refs.items():
        if k != "prep":
            continue
        got = dc.prep_composition(c, F32, strict_gate=True)
        q = slice(0, c["Q"])
        assert ref.units(got["dpts"][q], want["dpts"][0][q], want["dpts"][1][q]) > dc.C_PREP_DPTS, name
        got = dc.prep_composition(c, F32, drop_head=True)
        assert dc.over("prep_bwd", dc.worst("prep_bwd", got, want, ("dpts",))), (name, "heads reduced over H - 1")


def test_pinned_points_sit_on_the_gate(refs):
    for (k, name, _), (c, want) in refs.items():
        if k != "prep":
            continue
        uvw = want["uvw"][0][:c["Q"]]
        assert np.array_equal(uvw[:, 0], c["pts"][:c["Q"], 0].astype(np.float64)), name        # u0 = x exactly
        assert np.array_equal(uvw[:, 1], c["pts"][:c["Q"], 1].astype(np.float64)), name
        for col in (0, 1):
            assert set(dc.PIN) <= set(uvw[:, col].tolist()), (name, col)
        assert (c["R"] * c["H"]) % 64 != 0 or c["H"] == 64, name


def test_case_shapes_reach_the_launch_edges():
    rpw = lambda R: max(1, -(-R // 1024))               # demf_add_dropout_ln_bwd: cdiv(R, 256 blocks * 4 waves)
    assert {rpw(R) for R, _ in dc.LN_SHAPES} == {1, 2, 3}
    for R, _ in dc.LN_SHAPES:
        if rpw(R) > 1:
            assert -(-R // (4 * rpw(R))) * 4 * rpw(R) - R >= rpw(R), R      # at least one wave owns no row
    assert {c for _, c in dc.LN_SHAPES} == {c for _, c in dc.L2_SHAPES} == {64, 128, 256, 512, 1024}
    vpl = lambda S: 1 if S <= 64 else 2 if S <= 128 else 4 if S <= 256 else 8 if S <= 512 else 16
    assert {vpl(S) for _, S in dc.SM_SHAPES} == {1, 2, 4, 8, 16}
    for n, c in dc.ln_cases().items():
        if c["R"] >= 5:
            assert set(c["kind"].tolist()) == set(range(5)), n
    assert {int(c["kind"][0]) for c in dc.ln_cases().values() if c["R"] == 1} == set(range(5))


def test_host_hash_reproduces_recorded_keep_bits(golden_dir):
    """tests/golden/dropout_keep_table.json: keep bits of demf_dropout_mask recorded on an MI355X."""
    with open(os.path.join(golden_dir, "dropout_keep_table.json")) as f:
        table = json.load(f)
    assert table["entries"]
    for e in table["entries"]:
        bits = np.unpackbits(np.frombuffer(bytes.fromhex(e["keep_hex"]), np.uint8))[:e["n"]].astype(bool)
        got = ref.dropout_keep(int(e["seed"]), int(e["step"]), e["op"], 0, e["n"], e["p"])
        assert np.array_equal(got, bits), (e["op"], e["p"], int(np.flatnonzero(got != bits)[0]))
        if e["p"] == 0:
            assert bits.all()
        else:
            assert abs(bits.mean() - (1 - e["p"])) < 0.05
