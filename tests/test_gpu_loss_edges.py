"""The loss kernels of csrc/loss.hip, called directly (ops.head_loss / vote_loss / loss_total / query_pos_rows /
target_weights), against the float64 reference of tests/loss_reference.py at workgroup edges (one 256-row
workgroup, a full one plus a tail, the bench's 2048 rows, the vote kernel's 8-way unrolled counting loop with
scene boundaries inside one step) and ON the branch points (SmoothL1 at beta, IoU boxes that touch / tie /
contain each other, signed and clamped unions, saturated cross entropies).

Tolerances: |got - ref64| <= C * 2^-24 * scale, scale = A (sum of |row contributions|) for a loss value, T (sum of
the |additive terms|) for a gradient element; the constants C_* and how they were measured are in
tests/loss_cases.py.  "Exactly" means ==.  Inputs live on a 2^-10 grid (loss_cases._q), so the comparison
measures the kernel's arithmetic and not the conditioning of its inputs.  Every test prints its worst error in
those units before asserting."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_reference as lr

pytestmark = pytest.mark.gpu
NAMES = ("cls", "reg", "base")


@pytest.fixture(scope="module")
def head_cases():
    return lc.head_cases()


@pytest.fixture(scope="module")
def head_refs(head_cases):
    """name -> (sums, A, grads, T) for the upstream gradient lc.GOUT: computed once, never modified."""
    return {n: lr.head_loss_ref(*[c[k] for k in lc.HEAD_KEYS[:3]], lc.HYPER, *[c[k] for k in lc.HEAD_KEYS[3:]],
                                gout=lc.GOUT) for n, c in head_cases.items()}


@pytest.fixture(scope="module")
def vote_cases():
    return lc.vote_cases()


@pytest.fixture(scope="module")
def vote_refs(vote_cases):
    return {n: lr.vote_loss_ref(c["vote"], c["seed"], c["seed_idx"], c["masks"], c["vote_targets"], 3,
                                lc.VOTE_DST_WEIGHT, lc.VOTE_GOUT) for n, c in vote_cases.items()}


def _head_gpu(case, gout=lc.GOUT, backward=True):
    from demf_amd import ops
    t = {k: case[k].cuda() for k in lc.HEAD_KEYS}
    leaves = [t[k].requires_grad_() for k in NAMES]
    out = ops.head_loss(*leaves, lc.HYPER, *[t[k] for k in lc.HEAD_KEYS[3:]])
    if not backward:
        return out.detach().cpu(), None
    g = torch.autograd.grad(out, leaves, grad_outputs=gout.cuda())
    for k in lc.HEAD_KEYS:                                  # the kernels read their inputs only
        assert torch.equal(t[k].detach().cpu(), case[k]), k
    return out.detach().cpu(), [x.cpu() for x in g]


def _check_head(name, case, ref):
    sums, A, g, T = ref
    got, gg = _head_gpu(case)
    uf = [lr.error_units(got[i], sums[i], A[i]) for i in range(7)]
    ug = [lr.error_units(a, b, t) for a, b, t in zip(gg, g, T)]
    print("head %-10s fwd units %s  grad units cls %.2f reg %.2f base %.2f"
          % (name, " ".join("%.2f" % u for u in uf), *ug))
    assert max(uf) <= lc.C_F_HEAD, (name, uf)
    for n, u in zip(NAMES, ug):
        assert u <= lc.C_G_HEAD, (name, n, u)
    # the residual block of the reg gradient follows dir_class_t: column 18 + dt of a positive row, nothing else
    pos = case["box_w"] != 0
    allowed = torch.nn.functional.one_hot(case["dir_class_t"], 12).bool() & pos.unsqueeze(1)
    assert not bool((gg[1][:, 18:30] != 0)[~allowed].any()), name
    d = case["reg"][:, 18:30].gather(1, case["dir_class_t"].view(-1, 1)).squeeze(1) - case["dir_res_t"]
    hit = gg[1][:, 18:30].gather(1, case["dir_class_t"].view(-1, 1)).squeeze(1) != 0
    assert torch.equal(hit, pos & (d != 0)), name
    assert torch.equal(gg[2], gg[1][:, 0:3]), name            # centre = base + offset: the same gradient, exactly
    return got, gg


@pytest.mark.parametrize("R", lc.HEAD_ROWS)
def test_head_loss_row_counts(R, head_cases, head_refs):
    """1 .. 2049 rows: below / at / above one workgroup, two full workgroups plus a tail, the bench's 2048 and
    one more; ~30 % positive rows, ~20 % without objectness weight."""
    name = "R%d" % R
    case = head_cases[name]
    assert int(case["obj_t"].sum()) >= 1 and (R < 64 or 0.2 < float(case["obj_t"].float().mean()) < 0.4)
    got, _ = _check_head(name, case, head_refs[name])
    if R <= 256:                    # one workgroup: one tree, one atomic per slot on a zeroed output
        again, _ = _head_gpu(case, backward=False)
        assert torch.equal(got, again)


def test_head_loss_without_positive_rows(head_cases, head_refs):
    case = head_cases["nopos257"]
    assert float(case["box_w"].abs().max()) == 0.0
    got, gg = _check_head("nopos257", case, head_refs["nopos257"])
    assert float(got[0]) > 0.0
    assert float(got[1:].abs().max()) == 0.0                 # every box loss exactly 0
    assert float(gg[1].abs().max()) == 0.0 and float(gg[2].abs().max()) == 0.0
    assert float(gg[0][:, 2:].abs().max()) == 0.0            # semantic columns


def test_head_loss_with_zero_objectness_weights(head_cases, head_refs):
    case = head_cases["objw0_513"]
    off = case["obj_w"] == 0
    assert 0.4 < float(off.float().mean()) < 0.8
    _, gg = _check_head("objw0_513", case, head_refs["objw0_513"])
    assert float(gg[0][off][:, 0:2].abs().max()) == 0.0      # no objectness gradient without weight


def test_head_loss_branch_edges(head_cases, head_refs):
    """The rows of loss_cases._edge_rows, in the first workgroup and again at the end of the second one (the
    last on row R - 1), against the reference under the common bound - which a gradient missing on touching boxes
    (-0.5 w_iou bw gout on c_x, half of it on s_x) or a tie weight other than 0.5 exceeds by orders of magnitude."""
    case = head_cases["edges300"]
    _check_head("edges300", case, head_refs["edges300"])
    # the IoU loss alone: hard expected numbers on the rows whose SmoothL1 terms would otherwise be added in
    e6 = torch.zeros(7)
    e6[6] = 1.0
    _, gg = _head_gpu(case, gout=e6)
    _, placed = lc.head_edge_case()
    w = np.float32(lc.HYPER[8])
    seen = set()
    for p, s in placed:
        bw = case["box_w"][p].numpy()
        row = gg[1][p].numpy()
        if s.get("ct") == (3, 0, 0):                          # disjoint on x
            assert not row.any(), p
            seen.add("disjoint")
        elif s.get("ct") == (1.5, .5, .5):                    # touching on x: clamp(min=0) passes the gradient at 0
            want = np.zeros(30, np.float32)
            want[0], want[3] = np.float32(-0.5) * w * bw, np.float32(-0.25) * w * bw
            np.testing.assert_allclose(row, want, rtol=4 * 2.0 ** -24, atol=0, err_msg=str(p))
            seen.add("touch_x")
        elif s.get("ct") == (.5, -.5, .5):                    # touching on y, target below
            want = np.zeros(30, np.float32)
            want[1], want[4] = np.float32(0.5) * w * bw, np.float32(-0.25) * w * bw
            np.testing.assert_allclose(row, want, rtol=4 * 2.0 ** -24, atol=0, err_msg=str(p))
            seen.add("touch_y")
        elif s.get("siz") == (1, 1.5, .5):                    # identical boxes: the centre gets 0.5 - 0.5
            assert not row[0:3].any(), p
            seen.add("identical")
        elif s.get("siz") == (-2, 1, 1):                      # union < 0: clamped, no overlap, nothing flows
            assert not row.any(), p
            seen.add("negative_union")
    assert seen == {"disjoint", "touch_x", "touch_y", "identical", "negative_union"}


# ---- vote loss ------------------------------------------------------------------------------------------------
def _vote_gpu(c):
    from demf_amd import ops
    vote = c["vote"].cuda().requires_grad_()
    v = ops.vote_loss(vote, c["seed"].cuda(), c["seed_idx"].cuda(), c["masks"].cuda(), c["vote_targets"].cuda(), 3,
                      lc.VOTE_DST_WEIGHT)
    (g,) = torch.autograd.grad(v * lc.VOTE_GOUT, vote)
    return v.detach().cpu(), g.cpu()


def _check_vote(name, c, ref):
    v, count, gv, contrib = ref
    got, gg = _vote_gpu(c)
    uf = lr.error_units(got, v, contrib.sum())
    ug = lr.error_units(gg, gv, gv.abs())                     # a zero of the reference (mask or sign 0): exactly 0
    print("vote %-16s count %5d  fwd units %.2f  grad units %.2f" % (name, count, uf, ug))
    assert uf <= lc.C_F_VOTE, (name, uf)
    assert ug <= lc.C_G_VOTE, (name, ug)
    on = torch.gather(c["masks"], 1, c["seed_idx"]).bool()
    assert int(on.sum()) == count
    assert float(gg[~on].abs().max() if (~on).any() else 0.0) == 0.0, name       # seeds on a masked-off point
    # the count, exactly, through the backward: |gvote| = gout * (1 / (count + 1e-6) * dst_weight) in fp32
    step = np.float32(lc.VOTE_GOUT) * (np.float32(1.0) / (np.float32(count) + np.float32(1e-6))
                                       * np.float32(lc.VOTE_DST_WEIGHT))
    live = on.unsqueeze(-1) & (gv != 0)
    assert np.array_equal(gg[live].abs().numpy(), np.full(int(live.sum()), step, np.float32)), \
        (name, count, float(step), np.unique(gg[live].abs().numpy())[:4])
    return got, gg, live


@pytest.mark.parametrize("shape", lc.VOTE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_vote_loss_block_edges_and_count(shape, vote_cases, vote_refs):
    """B*S from 1 to 8192: the scalar tail alone (< 2048 seeds), the unrolled loop alone (2048), both (2049,
    4105), scene boundaries inside one unrolled step (S = 683, 821) with unequal positive fractions per scene."""
    name = "%dx%dx%d" % shape
    c = vote_cases[name]
    _, _, live = _check_vote(name, c, vote_refs[name])
    assert int(live.sum()) > 0
    if shape[0] > 2:                                         # the scenes' positive fractions do differ
        per = torch.gather(c["masks"], 1, c["seed_idx"]).float().mean(1)
        assert float(per.max() - per.min()) > 0.3


def test_vote_loss_without_positive_seed(vote_cases, vote_refs):
    name = "nopos_3x100x50"
    got, gg, live = _check_vote(name, vote_cases[name], vote_refs[name])
    assert float(got) == 0.0 and float(gg.abs().max()) == 0.0 and int(live.sum()) == 0


def test_vote_loss_sign_zero_components(vote_cases, vote_refs):
    name = "sign0_2x300x40"
    c = vote_cases[name]
    _, gg, live = _check_vote(name, c, vote_refs[name])
    on = torch.gather(c["masks"], 1, c["seed_idx"]).bool().unsqueeze(-1)
    zero = on & ~live                                        # positive seed, vote == target + seed on that component
    assert int(zero[..., 0].sum()) >= 20 and int(zero[..., 2].sum()) >= 20
    assert float(gg[zero].abs().max()) == 0.0


# ---- loss_total / query_pos_rows / target_weights ---------------------------------------------------------------
@pytest.mark.parametrize("with_vote", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_loss_total_bit_exact(n, with_vote):
    from demf_amd import ops
    rng = np.random.default_rng(10 * n + with_vote)
    vecs = [(rng.standard_normal(7) * 3).astype(np.float32) for _ in range(n)]
    vote = np.float32(rng.standard_normal() * 2) if with_vote else None
    g8 = rng.standard_normal(8).astype(np.float32)
    tv = [torch.from_numpy(v).cuda().requires_grad_() for v in vecs]
    tvote = torch.tensor(vote).cuda().requires_grad_() if with_vote else None
    out = ops.loss_total(tv, tvote)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), lr.loss_total_np(vecs, vote))
    out.backward(torch.from_numpy(g8).cuda())
    gv, gvote = lr.loss_total_bwd_np(g8, n, with_vote)
    for j in range(n):
        np.testing.assert_array_equal(tv[j].grad.cpu().numpy(), gv[j])
    if with_vote:
        assert tvote.grad.cpu().numpy().reshape(()) == gvote
    for j in range(n):
        np.testing.assert_array_equal(tv[j].detach().cpu().numpy(), vecs[j])


@pytest.mark.parametrize("B,Q", [(1, 1), (1, 255), (2, 128), (1, 257), (8, 256)])
def test_query_pos_rows_bit_exact(B, Q):
    from demf_amd import ops
    g = torch.Generator().manual_seed(B * Q)
    reg = torch.randn(B, Q, 30, generator=g)
    base = torch.randn(B, Q, 3, generator=g) * 2
    dreg, dbase = reg.cuda(), base.cuda()
    out = ops.query_pos_rows(dreg, dbase)
    assert out.shape == (B * Q, 8) and out.dtype == torch.float32
    np.testing.assert_array_equal(out.cpu().numpy(), lr.query_pos_rows_np(reg.numpy(), base.numpy()))
    assert torch.equal(dreg.cpu(), reg) and torch.equal(dbase.cpu(), base)


@pytest.mark.parametrize("R", [1, 64, 1023, 1024, 1025, 2049])
def test_target_weights_block_edges(R):
    """One 1024-thread workgroup striding over R: below, at and above one stride, and the one-row case."""
    from demf_amd import ops
    g = torch.Generator().manual_seed(R)
    m = (torch.rand(R, generator=g) < 0.6).float()
    o = (torch.rand(R, generator=g) < 0.3).long()
    m[R // 2], o[R // 2] = 1.0, 1
    ow, bw = ops.target_weights(m.cuda(), o.cuda())
    np.testing.assert_allclose(ow.cpu().numpy(), (m.double() / (m.double().sum() + 1e-6)).numpy(), rtol=1e-6)
    np.testing.assert_allclose(bw.cpu().numpy(), (o.double() / (o.double().sum() + 1e-6)).numpy(), rtol=1e-6)
    z = torch.zeros(R, device="cuda")
    ow, bw = ops.target_weights(z, z.long())
    assert float(ow.abs().max()) == 0.0 and float(bw.abs().max()) == 0.0
