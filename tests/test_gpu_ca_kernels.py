"""The distance-form kernels of the points-only baseline, called directly (ops.ca_head_loss / ops.ca_detect_decode),
against the float64 reference of tests/ca_loss_reference.py: the method of tests/test_gpu_loss_edges.py.

Tolerances: |got - ref64| <= C * 2^-24 * scale, scale = A (sum of |row contributions|) for a loss value, T (sum of the
|additive terms|) for a gradient element, scale7 for a decoded box element and 1 for a probability; the constants C_*
and how they were measured are in tests/ca_loss_cases.py.  "Exactly" means ==.  Inputs live on a 2^-10 grid.  Every
test prints its worst error in those units before asserting."""
import pytest
import torch

import ca_loss_cases as cc
import ca_loss_reference as cr
import loss_reference as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def head_cases():
    return cc.head_cases()


@pytest.fixture(scope="module")
def head_refs(head_cases):
    """name -> (sums, A, grads, T) for the upstream gradient cc.GOUT: computed once, never modified."""
    return {n: cr.head_loss_ref(c["cls"], c["reg"], c["ref"], hyper, *[c[k] for k in cc.CA_KEYS[2:]], gout=cc.GOUT,
                                dir_t=c["dir_t"]) for n, (c, hyper) in head_cases.items()}


@pytest.fixture(scope="module")
def decode_cases():
    return cc.decode_cases()


def _head_gpu(case, hyper, gout=cc.GOUT, backward=True):
    from demf_amd import ops
    t = {k: case[k].cuda() for k in cc.CA_KEYS + ("ref", "dir_t")}
    leaves = [t[k].requires_grad_() for k in ("cls", "reg", "ref")]
    out = ops.ca_head_loss(*leaves[:2], hyper, *[t[k] for k in cc.CA_KEYS[2:]], ref_points=leaves[2], dir_t=t["dir_t"])
    if not backward:
        return out.detach().cpu(), None
    g = torch.autograd.grad(out, leaves, grad_outputs=gout.cuda())
    for k in cc.CA_KEYS + ("ref", "dir_t"):                 # the kernels read their inputs only
        assert torch.equal(t[k].detach().cpu(), case[k]), k
    return out.detach().cpu(), [x.cpu() for x in g]


def _check_head(name, case, hyper, ref):
    sums, A, g, T = ref
    got, gg = _head_gpu(case, hyper)
    uf = [lr.error_units(got[i], sums[i], A[i]) for i in range(7)]
    uc, ur, up = (lr.error_units(a, b, t) for a, b, t in zip(gg, g, T))
    print("ca head %-10s fwd units %s  grad units cls %.2f reg %.2f ref %.2f"
          % (name, " ".join("%.2f" % u for u in uf), uc, ur, up))
    assert max(uf) <= cc.C_F_CA, (name, uf)
    assert max(uc, ur, up) <= cc.C_G_CA, (name, uc, ur, up)
    assert float(got[4]) == 0.0                               # the centre slot: exact 0
    # rows without a box weight: exact zeros in every box column; the residual block follows dir_class_t
    pos = case["box_w"] != 0
    assert float(gg[1][~pos].abs().max() if (~pos).any() else 0.0) == 0.0, name
    assert float(gg[2][~pos].abs().max() if (~pos).any() else 0.0) == 0.0, name
    assert float(gg[0][~pos][:, 2:].abs().max() if (~pos).any() else 0.0) == 0.0, name
    allowed = torch.nn.functional.one_hot(case["dir_class_t"], 12).bool() & pos.unsqueeze(1)
    assert not bool((gg[1][:, 18:30] != 0)[~allowed].any()), name
    d = case["reg"][:, 18:30].gather(1, case["dir_class_t"].view(-1, 1)).squeeze(1) - case["dir_res_t"]
    hit = gg[1][:, 18:30].gather(1, case["dir_class_t"].view(-1, 1)).squeeze(1) != 0
    assert torch.equal(hit, pos & (d != 0)), name
    return got, gg


@pytest.mark.parametrize("R", cc.HEAD_ROWS)
def test_ca_head_loss_row_counts(R, head_cases, head_refs):
    """1 .. 2049 rows: below / at / above one workgroup, two full workgroups plus a tail, 2048 and one more; ~30 %
    positive rows, ~20 % without objectness weight, ~5 % of the distance targets negative (clamped in the kernel)."""
    name = "R%d" % R
    case, hyper = head_cases[name]
    assert int(case["obj_t"].sum()) >= 1
    got, _ = _check_head(name, case, hyper, head_refs[name])
    if R <= 256:                    # one workgroup: one tree, one atomic per slot on a zeroed output
        again, _ = _head_gpu(case, hyper, backward=False)
        assert torch.equal(got, again)


def test_ca_head_loss_without_positive_rows(head_cases, head_refs):
    case, hyper = head_cases["nopos257"]
    assert float(case["box_w"].abs().max()) == 0.0
    got, gg = _check_head("nopos257", case, hyper, head_refs["nopos257"])
    assert float(got[0]) > 0.0 and bool(torch.isfinite(got).all())
    assert float(got[1:].abs().max()) == 0.0                 # every box loss exactly 0
    assert float(gg[1].abs().max()) == 0.0 and float(gg[2].abs().max()) == 0.0     # and every box gradient
    assert float(gg[0][:, 2:].abs().max()) == 0.0
    assert bool(torch.isfinite(gg[0]).all())


def test_ca_head_loss_with_zero_objectness_weights(head_cases, head_refs):
    case, hyper = head_cases["objw0_513"]
    off = case["obj_w"] == 0
    assert 0.4 < float(off.float().mean()) < 0.8
    _, gg = _check_head("objw0_513", case, hyper, head_refs["objw0_513"])
    assert float(gg[0][off][:, 0:2].abs().max()) == 0.0      # no objectness gradient without weight


def test_ca_head_loss_branch_edges(head_cases, head_refs):
    """The rows of ca_loss_cases._edge_rows (SmoothL1 exactly at beta = 2^-3, ties, clamped targets, zero target
    volume, clamped union, saturated cross entropies) in the first workgroup and again at the end of the second, under
    the common bound - which a tie weight other than 0.5 or a SmoothL1 branch taken on the wrong side exceeds by
    orders of magnitude - and hard numbers on the rows where they exist."""
    case, hyper = head_cases["edges300"]
    _check_head("edges300", case, hyper, head_refs["edges300"])
    e6 = torch.zeros(7)
    e6[6] = 1.0
    _, gi = _head_gpu(case, hyper, gout=e6)                   # the IoU term alone
    e3 = torch.zeros(7)
    e3[3] = 1.0
    _, gs = _head_gpu(case, hyper, gout=e3)                   # the SmoothL1 of the distances alone
    _, placed = cc.head_edge_case()
    seen = set()
    for p, s in placed:
        t = s.get("t")
        if s.get("lg") == (0.0,) * 6 and t == (1.0,) * 6:     # identical boxes: IoU 1, every pair of paths cancels
            assert not gi[1][p, 0:6].any() and not gs[1][p, 0:6].any(), p
            seen.add("identical")
        elif t == (0.0,) * 6 and s.get("lg") == (0.0,) * 6:   # a point target: overlap 0, IoU 0 whatever the box
            assert not gi[1][p, 0:6].any(), p
            seen.add("point")
        elif s.get("lg") == (-8.0,) * 6 and t == (0.0,) * 6:  # union below 1e-6: clamped, nothing flows
            assert not gi[1][p, 0:6].any(), p
            seen.add("clamped_union")
        elif t is not None and t[0] == 1 - cc.BETA_EDGE and t[1] == 1 + cc.BETA_EDGE:
            # d = 1: |d - t| == beta takes the LINEAR branch (diff < beta is false): gradient sign(d - t) * w * bw * d
            w = torch.tensor(hyper[5]) * case["box_w"][p]
            assert torch.equal(gs[1][p, 0:3], torch.stack([w, -w, torch.zeros(())])), p
            seen.add("beta")
    assert seen == {"identical", "point", "clamped_union", "beta"}


def test_ca_head_loss_without_reference_points(head_cases):
    """ref_points=None: the targets are constants, nothing but cls / reg gets a gradient - the same numbers."""
    from demf_amd import ops
    case, hyper = head_cases["R257"]
    _, want = _head_gpu(case, hyper)
    t = {k: case[k].cuda() for k in cc.CA_KEYS}
    leaves = [t[k].requires_grad_() for k in ("cls", "reg")]
    out = ops.ca_head_loss(*leaves, hyper, *[t[k] for k in cc.CA_KEYS[2:]])
    g = torch.autograd.grad(out, leaves, grad_outputs=cc.GOUT.cuda())
    assert torch.equal(g[0].cpu(), want[0]) and torch.equal(g[1].cpu(), want[1])


def test_ca_head_loss_rejects_wrong_shapes():
    from demf_amd import ops
    c, hyper = cc.head_case(8, 1), cc.HYPER
    t = {k: c[k].cuda() for k in cc.CA_KEYS}
    t["distance_t"] = t["distance_t"][:7].contiguous()
    with pytest.raises(ValueError, match="distance_t"):
        ops.ca_head_loss(t["cls"], t["reg"], hyper, *[t[k] for k in cc.CA_KEYS[2:]])


# ---- decode ---------------------------------------------------------------------------------------------------------
def _check_decode(name, case, rot, views=False):
    from demf_amd import ops
    reg, cls, ref = (case[k].cuda() for k in ("reg", "cls", "ref"))
    if views:            # column slices of wider buffers: strides are passed, nothing is copied
        B, K = reg.shape[:2]
        wide = torch.full((B, K, 50), float("nan"), device="cuda")
        wide[..., 3:33], wide[..., 36:48] = reg, cls
        reg, cls = wide[..., 3:33], wide[..., 36:48]
    box7, cosy, siny, obj, sem, classes = ops.ca_detect_decode(reg, cls, ref, 12, rot)
    r = cr.decode_ref(case["reg"], case["cls"], case["ref"], 12, rot)
    ub = [lr.error_units(box7[..., i].cpu(), r["box7"][..., i], r["scale7"][..., i]) for i in range(7)]
    us = max(lr.error_units(obj.cpu(), r["obj"], torch.ones_like(r["obj"])),
             lr.error_units(sem.cpu(), r["sem"], torch.ones_like(r["sem"])))
    ut = max(lr.error_units(cosy.cpu(), r["cos"], torch.ones_like(r["cos"])),
             lr.error_units(siny.cpu(), r["sin"], torch.ones_like(r["sin"])))
    print("ca decode %-8s rot %d views %d  box units %s  score %.2f  cos/sin %.2f"
          % (name, rot, views, " ".join("%.2f" % u for u in ub), us, ut))
    assert max(ub) <= cc.C_BOX_CA, (name, ub)
    assert us <= cc.C_SCORE_CA, (name, us)
    # cos / sin of the kernel's own yaw: 1-Lipschitz in the yaw, whose error is <= C_BOX units of 2^-24 * its scale
    # (< 13), plus the rounding of cosf / sinf themselves (a few units of 2^-24).  A derived bound (108 units), not one
    # of the composition's: the worst the kernel read on an MI355X is 8.39 (K = 1024).
    assert ut <= cc.C_BOX_CA * 13 + 4, (name, ut)
    assert classes.dtype == torch.int64 and torch.equal(classes.cpu(), r["classes"]), name
    assert torch.equal(torch.argmax(sem, -1), classes)
    yaw = box7[..., 6]
    assert float(yaw.min()) >= 0.0 and float(yaw.max()) < 6.2831855
    if not rot:
        assert float(yaw.abs().max()) == 0.0 and float((cosy - 1).abs().max()) == 0.0 and float(siny.abs().max()) == 0.0
    return box7.cpu(), r


@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("K", cc.DECODE_K)
def test_ca_detect_decode(K, rot, decode_cases):
    """K = 1 .. 1024 proposals in 2 scenes (one lane each: below / at / above one workgroup, the 1024 limit), the edge
    rows of ca_loss_cases._decode_edge_rows at the start of scene 0 and the end of scene 1."""
    box7, r = _check_decode("K%d" % K, decode_cases["K%d" % K], rot)
    if K >= 64:
        size = box7[..., 3:6]
        clamped = r["scale7"][..., 3:6] == 0
        assert int(clamped.sum()) >= 8 and bool((size[clamped] == torch.tensor(0.1)).all())     # float32(0.1), exactly
        if rot:
            assert float(box7[0, 0, 6]) == 0.0                                    # bin 0, residual 0
            assert 6.28 < float(box7[0, 1, 6]) < 6.2831855                        # just below 2 pi


def test_ca_detect_decode_single_row_below_two_pi(decode_cases):
    box7, _ = _check_decode("K1_rowE", decode_cases["K1_rowE"], True)
    assert box7.shape == (1, 1, 7) and 6.28 < float(box7[0, 0, 6]) < 6.2831855


def test_ca_detect_decode_reads_strided_views(decode_cases):
    _check_decode("K255", decode_cases["K255"], True, views=True)


def test_ca_detect_decode_limits():
    from demf_amd import ops
    z = lambda *s: torch.zeros(s, device="cuda")                             # noqa: E731
    with pytest.raises(RuntimeError, match="exceeds 1024"):
        ops.ca_detect_decode(z(1, 1025, 30), z(1, 1025, 12), z(1, 1025, 3), 12)
    with pytest.raises(ValueError, match="ref_points"):
        ops.ca_detect_decode(z(1, 8, 30), z(1, 8, 12), z(1, 7, 3), 12)
    out = ops.ca_detect_decode(z(2, 0, 30), z(2, 0, 12), z(2, 0, 3), 12)
    assert out[0].shape == (2, 0, 7)
