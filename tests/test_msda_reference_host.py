"""tests/msda_cases.py and tests/msda_reference.py checked on the CPU: the cases hold what they promise, the raw front
end and the numpy cell equal independent float64 statements, the bounds are loose enough (the float32 oracle stays
inside every one of them on every case) and tight enough (every mutation of MUTATIONS leaves them in every case class
where the mutation changes an output).  No GPU."""
import functools

import numpy as np
import pytest
import torch

import msda_cases as mc
import msda_reference as ref
from oracle import kernels as ok

F32, F64 = np.float32, np.float64
TABLES = dict(direct=mc.DIRECT, bf16=mc.BF16, raw=mc.RAW, head=mc.HEAD, xcd=mc.XCD)
CLASSES = {
    "direct": [("direct", n) for n in mc.DIRECT if not n.startswith("gen_")],
    "generic": [("direct", n) for n in mc.DIRECT if n.startswith("gen_")],
    "bf16": [("bf16", n) for n in mc.BF16],
    "raw_wave": [("raw", n) for n in mc.RAW if n.startswith("wave_")],
    "raw_lane": [("raw", n) for n in mc.RAW if n.startswith("lane_")],
    "raw_detector": [("raw", n) for n in mc.RAW if n.startswith("detr_")],
    "head": [("head", n) for n in mc.HEAD],
    "xcd": [("xcd", n) for n in mc.XCD],
}
ALL = [(t, n) for t, table in TABLES.items() for n in table]


def _is_direct(table):
    return table in ("direct", "bf16")


@functools.lru_cache(maxsize=None)
def _built(table, name):
    c = TABLES[table][name][0]
    if _is_direct(table):
        d = mc.direct_inputs(name, c)
        j = ref.judge(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], d["gout"], d["prefill"], d["eps"])
    else:
        d = mc.raw_inputs(name, c)
        j = ref.judge(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], eps=d["eps"], attw_err=d["attw_err"])
    return c, d, j


def test_tables_have_every_row_the_dispatch_asks_for():
    D = {n: c for n, (c, _) in mc.DIRECT.items()}
    fast = {(c["Dh"] // 4, (c["L"], c["P"]) if (c["L"], c["P"]) in ((4, 2), (4, 4)) else "runtime")
            for c in D.values() if mc.form_of(c)[0].startswith("msda_fwd_kernel")}
    assert fast == {(g, lp) for g in (1, 2, 4, 8, 16, 32, 64) for lp in ((4, 2), (4, 4), "runtime")}
    assert {(c["L"], c["P"]) for c in D.values()} >= set(mc.RUNTIME_LP)
    assert {c["Dh"] for n, c in D.items() if n.startswith("gen_")} >= {5, 12, 20, 512, 32}
    assert mc.form_of(D["gen_value_off"]) == ["msda_fwd_generic", "msda_bwd_generic"] == mc.form_of(D["gen_out_off"])
    assert {(c["H"], c["Dh"]) for c in D.values()} >= {(1, 256), (1, 4), (8, 32)}
    threads = {c["B"] * c["Q"] * c["H"] * (c["Dh"] // 4) for c in D.values()}
    assert threads >= {255, 256, 257, 8} and any(c["B"] == 3 for c in D.values())
    for table in (mc.DIRECT, mc.BF16):
        assert {c["gv"] for c, _ in table.values()} == set(mc.GV_MODES)
    assert {c["Dh"] // 4 for c, _ in mc.BF16.values() if c["Dh"] % 16 == 0 or c["Dh"] == 4} == {1, 8, 64}
    R = {n: c for n, (c, _) in mc.RAW.items()}
    assert {(c["P"], c["B"] * c["Q"]) for n, c in R.items() if n.startswith("wave_")} == {(p, r) for p in (2, 4) for r in (1, 3, 4, 5, 37)}
    assert {(c["P"], c["B"] * c["Q"]) for c, _ in mc.XCD.values()} == {(p, r) for p in (2, 4) for r in (1, 5, 37, 130)}
    for n in R:
        assert (mc.form_of(R[n])[0].startswith("msda_fwd_raw_kernel")) == n.startswith("lane_"), n
    assert R["lane_H4"]["H"] == 4 and R["lane_ldraw_odd"]["ldraw"] % 2 and R["lane_off_col_odd"]["off_col0"] % 2
    assert R["lane_raw_off"]["raw_shift"] == 1 and R["lane_ref_off"]["ref_shift"] == 1
    for li, n in ((0, "detr_li0"), (5, "detr_li5")):
        c = R[n]
        assert (c["Q"], c["vpitch"], c["v_off"], c["off_col0"]) == (13, 1536, 256 * li, 2)
        assert c["lgt_col0"] > c["off_col0"] + 2 * 128 and c["ldraw"] > c["lgt_col0"] + 128
    Hd = [c for c, _ in mc.HEAD.values()]
    assert {(c["P"], c["first"], c["B"]) for c in Hd} == {(p, f, b) for p in (2, 4) for f in (2, 3) for b in (1, 32)}
    assert {(c["Q"], c["B"]) for c in Hd} == {(q, b) for q in (1, 8, 63, 64, 65, 130) for b in (1, 32)}
    assert {c["vpitch"] for c in Hd} == {256, 1536}
    big = [c for c in Hd if c["Q"] == 130]
    assert {mc.head_chunks(c) for c in big} == {(3, 64, 1), (1, 192, 3)}
    for c in Hd:                                   # a one-pixel-wide level in memory and one staged
        shapes = mc.pyramid(c["pyr"], 4)
        assert any(1 in s for s in shapes[:c["first"]])
        assert any(1 in s for s in shapes[c["first"]:])
    for t, n in ALL:
        c = TABLES[t][n][0]
        S = sum(h * w for h, w in mc.pyramid(c["pyr"], c["L"]))
        assert S <= 320 and c["Q"] <= 130 and c["B"] <= 32, n


def test_form_of_reaches_every_instantiation():
    seen = set()
    for t, n in ALL:
        seen.update(mc.form_of(TABLES[t][n][0], mc.CHILD_SWITCHES if t == "xcd" else mc.DEFAULT_SWITCHES))
    assert seen == set(mc.FORMS), (sorted(set(mc.FORMS) - seen), sorted(seen - set(mc.FORMS)))
    assert len(set(mc.FORMS)) == len(mc.FORMS)
    lanes = dict(mc.DEFAULT_SWITCHES, DEMF_MSDA_RAW_LANES=1)
    assert mc.form_of(mc.RAW["wave_P4_rows5"][0], lanes) == ["msda_fwd_raw_kernel<8,4,4>"]


@pytest.mark.parametrize("table,name", ALL, ids=[n for _, n in ALL])
def test_case_meets_its_construction_conditions(table, name):
    c, d, j = _built(table, name)
    shapes = [tuple(s) for s in d["shapes"]]
    loc = np.asarray(d["loc"], F64)
    assert ref.robust(shapes, loc, *d["eps"]).all(), "a sample within 8 eps_loc of an integer"
    x, y = ref.pixel(shapes, loc)
    assert np.isfinite(loc).all() and np.abs(x).max() < 2.0 ** 31 and np.abs(y).max() < 2.0 ** 31
    if c["Q"] >= 2:
        assert j.out_zero[:, 0].all() and not j.out_zero[:, 1:].all(), "query 0, and only it, has every sample outside"
    if mc.is_exact(c["pyr"]):
        near = (np.abs(x) < 64) & (np.abs(y) < 64)
        assert not d["eps"][0][near].any() and not d["eps"][1][near].any(), "the coordinate arithmetic is exact"
        samples = c["B"] * (c["Q"] - 1) * c["H"] * c["P"]
        for l, (Hl, Wl) in enumerate(shapes):
            have = set(zip(x[:, 1:, :, l].reshape(-1), y[:, 1:, :, l].reshape(-1)))
            pairs = set(mc.edge_pairs(Hl, Wl))
            assert have <= pairs
            if samples >= 2 * len(pairs) or "edges" in name:
                assert have == pairs, (l, sorted(pairs - have))
    else:
        assert (d["eps"][0] > 0).any()
    if not _is_direct(table):
        assert (d["raw"] == mc.GARBAGE).sum() == d["raw"].size - 3 * c["H"] * 4 * c["P"] * d["raw"].shape[0]
        kinds = c["B"] * c["Q"] * c["H"]
        assert kinds < 4 or all((d["lgt"] == v).all(-1).any() for v in (F32(0.7), F32(-1e4)))
    else:
        w = d["attw"]
        assert (w == 0).any() and (w < 0).any() and (np.abs(w).max() > 20 or w.size < 40)


def test_raw_front_end_against_torch_and_the_explicit_formula():
    for name in ("wave_P4_rows37", "lane_H4", "detr_li0", "wave_P2_rows3"):
        c, d, _ = _built("raw", name)
        off, lgt = ref.raw_columns(d["raw"], c["H"], 4, c["P"], c["off_col0"], c["lgt_col0"])
        assert np.array_equal(off, d["off"]) and np.array_equal(lgt, d["lgt"])
        loc, attw = ref.raw_front_end(off, lgt, d["ref"], d["shapes"])
        want = torch.softmax(torch.from_numpy(lgt).double(), -1).numpy().reshape(attw.shape)
        assert np.allclose(attw, want, rtol=1e-13, atol=1e-300)
        for l, (Hl, Wl) in enumerate(d["shapes"]):
            for p in range(c["P"]):
                assert np.array_equal(loc[:, :, l, p, 0], d["ref"][:, None, l, 0].astype(F64) + off[:, :, l, p, 0].astype(F64) / Wl)
                assert np.array_equal(loc[:, :, l, p, 1], d["ref"][:, None, l, 1].astype(F64) + off[:, :, l, p, 1].astype(F64) / Hl)


@pytest.mark.parametrize("table,name", [("direct", "G8_L4P2"), ("direct", "G2_L1P3"), ("direct", "gen_Dh20"),
                                        ("direct", "prod_H8_Dh32_thin_edges"), ("raw", "wave_P4_rows37"), ("head", "head_P2_LS3_Q8_B32")])
def test_numpy_cell_equals_the_oracle(table, name):
    """The restatement behind the magnitudes, the counts and the mutations is the operation the oracle computes."""
    c, d, j = _built(table, name)
    e = j.numpy
    close = lambda a, b: np.allclose(a, b, rtol=1e-11, atol=1e-12)
    assert close(e.out, j.out)
    assert not e.out[j.out_zero].any() and not j.out[j.out_zero].view(np.uint64).any()
    if _is_direct(table):
        assert close(e.gattw, j.gattw) and close(e.gloc, j.gloc) and close(e.gvalue.value, j.gvalue.value)
        assert not j.gloc[j.dead].any() and not j.gattw[j.dead].any()
        none = e.gvalue.hits == 0
        pre = 0.0 if d["prefill"] is None else d["prefill"].astype(F64)
        assert none.any() and np.array_equal(j.gvalue.value[none], np.broadcast_to(pre, none.shape)[none])
        assert (e.gloc_mag >= np.abs(e.gloc) - 1e-12).all()


def _f32_results(table, c, d):
    """The operation in float32 on the CPU: the C oracle with dtype float32, behind a numpy float32 front end for the
    raw forms."""
    if _is_direct(table):
        out = ok.msda_fwd(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], dtype=F32)
        gv, gloc, gattw = ok.msda_bwd(d["value"], d["shapes"], d["lsi"], d["loc"], d["attw"], d["gout"], dtype=F32)
        if d["prefill"] is not None:
            gv = gv + d["prefill"]
        return dict(out=out, gloc=gloc, gattw=gattw, gvalue=gv)
    loc, attw = ref.raw_front_end(d["off"], d["lgt"], d["ref"], d["shapes"], dtype=F32)
    shp = (c["B"], c["Q"]) + loc.shape[1:4]
    return dict(out=ok.msda_fwd(d["value"], d["shapes"], d["lsi"], loc.reshape(shp + (2,)), attw.reshape(shp), dtype=F32))


def _ratios(j, got):
    r = {"out": np.abs(got["out"].astype(F64) - j.out) / j.out_bound}
    if "gloc" in got:
        r["gloc"] = np.abs(got["gloc"].astype(F64) - j.gloc) / j.gloc_bound
        r["gattw"] = np.abs(got["gattw"].astype(F64) - j.gattw) / j.gattw_bound
        r["gvalue"] = np.abs(got["gvalue"].astype(F64) - j.gvalue.value) / j.gvalue_bound
    return r


def test_bounds_hold_the_float32_oracle_on_every_case():
    worst, where = {}, {}
    for table, name in ALL:
        c, d, j = _built(table, name)
        got = _f32_results(table, c, d)
        assert not got["out"][j.out_zero].view(np.uint32).any(), name + ": an output with no valid term is not +0.0"
        for k, r in _ratios(j, got).items():
            key = (table, k)
            if r.size and r.max() > worst.get(key, -1.0):
                worst[key], where[key] = float(r.max()), name
    for key in sorted(worst):
        print("msda-host float32 oracle  %-7s %-7s worst |err| / bound %.3f  (%s)" % (key + (worst[key], where[key])))
    assert all(v <= 1.0 for v in worst.values()), "a bound is wrong: " + str({k: v for k, v in worst.items() if v > 1.0})


def test_measured_exp_error_sets_E():
    args = np.concatenate([ref.exp_arguments(_built(t, n)[1]["lgt"]).reshape(-1) for t, n in ALL if not _is_direct(t)])
    worst = ref.exp_ulp_error(args)
    print("msda-host numpy float32 exp on the cases' %d arguments: worst %.3f ulp -> E = 4 x = %.2f (EXP_ULP = %.2f)" % (
        args.size, worst, 4 * worst, ref.EXP_ULP))
    assert (args <= 0).all() and args.min() <= -160
    assert 4 * worst <= ref.EXP_ULP + 0.01, "EXP_ULP is 4 x the error measured when the bound was written"


def _mutated(table, c, d, mut):
    if mut in ref.FRONT_END_MUTATIONS:
        loc, attw = ref.raw_front_end(d["off"], d["lgt"], d["ref"], d["shapes"], mut=mut)
        shp = (c["B"], c["Q"]) + loc.shape[1:4]
        e = ref.evaluate(d["value"], d["shapes"], d["lsi"], loc.reshape(shp + (2,)), attw.reshape(shp))
    else:
        e = ref.evaluate(d["value"], d["shapes"], d["lsi"], np.asarray(d["loc"], F64), np.asarray(d["attw"], F64),
                         d.get("gout"), d.get("prefill"), mut=mut)
    got = dict(out=e.out)
    if e.gvalue is not None:
        got.update(gloc=e.gloc, gattw=e.gattw, gvalue=e.gvalue.value)
    return got


def _applies(mut, cls):
    if mut in ref.FRONT_END_MUTATIONS:
        return cls not in ("direct", "generic", "bf16")
    if mut == "nonstrict_border":
        # at pixel -1 the only corners in range have weight exactly 0, at pixel H_l none is in range: no forward
        # changes.  grad_loc does (the one-sided derivative at -1 is not 0), so the classes with a backward see it.
        return cls in ("direct", "generic", "bf16")
    return True


def test_every_mutation_leaves_the_bounds_in_every_class():
    table_out = []
    for mut in ref.MUTATIONS:
        for cls, members in CLASSES.items():
            if not _applies(mut, cls):
                continue
            caught = None
            for table, name in members:
                c, d, j = _built(table, name)
                if mut == "head_plus_one" and c["H"] == 1:
                    continue
                if c["B"] * c["Q"] > 600:                 # (the small members of a class are tried first and suffice)
                    continue
                over = {k: float(r.max()) for k, r in _ratios(j, _mutated(table, c, d, mut)).items() if r.size and r.max() > 1.0}
                if over:
                    caught = (name, over)
                    break
            table_out.append((mut, cls, caught))
    for mut, cls, caught in table_out:
        print("msda-host mutation %-22s class %-13s %s" % (mut, cls, "caught by %s: %s" % (
            caught[0], ", ".join("%s x%.3g" % kv for kv in caught[1].items())) if caught else "NOT CAUGHT"))
    assert all(c for _, _, c in table_out), [(m, k) for m, k, c in table_out if not c]
