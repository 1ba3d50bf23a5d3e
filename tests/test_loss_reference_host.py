"""The fp64 loss reference (tests/loss_reference.py) against the project's torch losses
(demf_amd/modules/losses.py, VoteModule.get_loss) and the oracle's loss classes (oracle/deps.py), all in
float64 on the CPU, plus hard expected values at the IoU's touching / tie points - what makes the reference
trustworthy before a GPU test leans on it.  The last test measures what an fp32 evaluation costs, the
number the GPU tests' tolerance constants are derived from."""
from unittest import mock

import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_reference as lr

F64 = torch.float64
REL = 1e-12


def _ref(case, gout=lc.GOUT):
    return lr.head_loss_ref(*[case[k] for k in lc.HEAD_KEYS[:3]], lc.HYPER, *[case[k] for k in lc.HEAD_KEYS[3:]],
                            gout=gout)


def _vref(c):
    return lr.vote_loss_ref(c["vote"], c["seed"], c["seed_idx"], c["masks"], c["vote_targets"], 3,
                            lc.VOTE_DST_WEIGHT, lc.VOTE_GOUT)


def _within(got, ref, scale, rel=REL):
    return bool(((got.to(F64) - ref).abs() <= rel * scale).all())


@pytest.fixture(scope="module")
def head():
    return {n: (c, _ref(c)) for n, c in lc.head_cases().items()}


@pytest.fixture(scope="module")
def vote():
    return {n: (c, _vref(c)) for n, c in lc.vote_cases().items()}


def _f64_everywhere():
    """``Tensor.float()`` -> float64: the vote losses cast the gathered mask with .float(), which would round
    the weight mask / (count + 1e-6) to fp32 in an otherwise float64 run."""
    return mock.patch.object(torch.Tensor, "float", lambda self: self.double())


def test_reference_matches_project_functions_fp64(head):
    for name, (case, (sums, A, g, T)) in head.items():
        s, gs = lc.head_composition(case, F64)
        assert _within(s, sums, A), name
        for a, b, t, n in zip(gs, g, T, ("cls", "reg", "base")):
            assert _within(a, b, t), (name, n)
            assert bool((b.abs() <= t * (1 + 1e-12)).all()), (name, n)      # T bounds the gradient it scales


def _oracle_composition(case):
    """The seven sums through the ORACLE's loss classes, float64."""
    from oracle import deps
    h = lr.hyper_dict(lc.HYPER)
    d = lambda k: case[k].to(F64)
    cls, reg, base = (d(k).clone().requires_grad_() for k in ("cls", "reg", "base"))
    cen, siz, bw = base + reg[:, 0:3], reg[:, 3:6], d("box_w")
    w3 = bw.unsqueeze(-1).repeat(1, 3)
    corners = lambda c, s: torch.cat([c - s / 2, c + s / 2], dim=-1)
    ce = lambda w, cw=None: deps.CrossEntropyLoss(class_weight=cw, reduction="sum", loss_weight=w)
    sl1 = lambda w, beta: deps.SmoothL1Loss(beta=beta, reduction="sum", loss_weight=w)
    res = reg[:, 18:30].gather(1, case["dir_class_t"].view(-1, 1)).squeeze(1)
    sums = torch.stack([
        ce(h["w_obj"], [h["cw0"], h["cw1"]])(cls[:, 0:2], case["obj_t"], weight=d("obj_w")),
        ce(h["w_dircls"])(reg[:, 6:18], case["dir_class_t"], weight=bw),
        sl1(h["w_dirres"], h["beta_dirres"])(res, d("dir_res_t"), weight=bw),
        sl1(h["w_size"], h["beta_size"])(siz, d("size_t"), weight=w3),
        sl1(h["w_center"], h["beta_center"])(cen, d("center_t"), weight=w3),
        ce(h["w_sem"])(cls[:, 2:12], case["sem_t"], weight=bw),
        deps.AxisAlignedIoULoss(reduction="sum", loss_weight=h["w_iou"])(
            corners(cen, siz), corners(d("center_t"), d("size_t")), weight=bw)])
    return sums.detach(), torch.autograd.grad((lc.GOUT.to(F64) * sums).sum(), (cls, reg, base))


def test_reference_matches_oracle_losses_fp64(head):
    for name in ("R257", "R2049", "objw0_513", "edges300"):
        case, (sums, A, g, T) = head[name]
        with _f64_everywhere():                          # CrossEntropyLoss: loss * weight.float()
            s, gs = _oracle_composition(case)
        assert _within(s, sums, A), name
        for a, b, t, n in zip(gs, g, T, ("cls", "reg", "base")):
            assert _within(a, b, t), (name, n)


def test_vote_reference_matches_project_and_oracle_fp64(vote):
    from oracle import deps
    om = deps.VoteModule(8, gt_per_seed=3, vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                                                          loss_dst_weight=lc.VOTE_DST_WEIGHT))
    for name, (c, (v, count, gv, contrib)) in vote.items():
        A = contrib.sum()
        with _f64_everywhere():
            pv, pg = lc.vote_composition(c, F64)
            vp = c["vote"].to(F64).clone().requires_grad_()
            ov = om.get_loss(c["seed"].to(F64), vp, c["seed_idx"], c["masks"], c["vote_targets"].to(F64))
            (og,) = torch.autograd.grad(ov * lc.VOTE_GOUT, vp)
        assert count == int(torch.gather(c["masks"], 1, c["seed_idx"]).sum()), name
        for val, grad, who in ((pv, pg, "project"), (ov.detach(), og, "oracle")):
            assert _within(val, v, A), (name, who)
            assert _within(grad, gv, gv.abs()), (name, who)


def test_vote_reference_matches_chamfer_distance_fp64(vote):
    """The per-seed contribution against the oracle's chamfer_distance (l1, no reduction) fed the weights."""
    from oracle import deps
    for name in ("3x683x500", "sign0_2x300x40"):
        c, (v, count, gv, contrib) = vote[name]
        B, S = c["seed_idx"].shape
        m = torch.gather(c["masks"], 1, c["seed_idx"]).to(F64)
        gt = torch.gather(c["vote_targets"].to(F64), 1, c["seed_idx"].unsqueeze(-1).expand(-1, -1, 9))
        gt = gt + c["seed"].to(F64).repeat(1, 1, 3)
        w = m / (m.sum() + 1e-6)
        _, ld, _, _ = deps.chamfer_distance(c["vote"].to(F64).view(B * S, 1, 3), gt.view(B * S, 3, 3),
                                            dst_weight=w.view(B * S, 1), criterion_mode="l1", reduction="none")
        per_seed = lc.VOTE_DST_WEIGHT * ld.min(dim=1).values.view(B, S)
        assert _within(per_seed, contrib, contrib + 1e-300), name


def _one_row(cen, siz, ct, st):
    """A single positive row, box weight 1, zeros elsewhere -> reference outputs with gout = ones."""
    f = lambda v: torch.tensor([v], dtype=torch.float32)
    reg = torch.zeros(1, 30)
    reg[0, 0:3], reg[0, 3:6] = torch.tensor(cen), torch.tensor(siz)
    return lr.head_loss_ref(torch.zeros(1, 12), reg, torch.zeros(1, 3), lc.HYPER, f(ct), f(st),
                            torch.zeros(1, dtype=torch.long), torch.zeros(1), torch.zeros(1, dtype=torch.long),
                            torch.ones(1, dtype=torch.long), torch.ones(1), torch.ones(1),
                            gout=torch.tensor([0, 0, 0, 0, 0, 0, 1.0]))


def test_touching_boxes_pass_the_gradient():
    """Prediction [0,0,0,1,1,1], target [1,0,0,2,1,1]: the extent on x is exactly 0, clamp(min=0) passes the
    gradient there (its mask is x >= min), so d loss / d (max-x corner) = -0.5 * w_iou * bw.  In centre / size
    form the max-x corner is c_x + s_x / 2: d/d c_x = -0.5 w, d/d s_x = -0.25 w."""
    w = lc.HYPER[8]
    sums, A, g, T = _one_row((.5, .5, .5), (1., 1., 1.), (1.5, .5, .5), (1., 1., 1.))
    assert float(sums[6]) == w                                            # IoU 0
    want = torch.zeros(30, dtype=F64)
    want[0], want[3] = -0.5 * w, -0.25 * w
    assert torch.equal(g[1][0], want)
    assert torch.equal(g[2][0], want[:3])
    # the project's function and the oracle's class on the corners themselves
    from demf_amd.modules import losses as L
    from oracle import deps
    for fn in (lambda p, t: L.axis_aligned_iou_loss_sum(p, t, torch.ones(1, dtype=F64), w),
               lambda p, t: deps.AxisAlignedIoULoss(reduction="sum", loss_weight=w)(p, t, torch.ones(1, dtype=F64))):
        p = torch.tensor([[0., 0, 0, 1, 1, 1]], dtype=F64, requires_grad=True)
        fn(p, torch.tensor([[1., 0, 0, 2, 1, 1]], dtype=F64)).backward()
        assert torch.equal(p.grad[0], torch.tensor([0, 0, 0, -0.5 * w, 0, 0], dtype=F64))
    # disjoint by any margin: nothing
    _, _, g, _ = _one_row((.5, .5, .5), (1., 1., 1.), (1.625, .5, .5), (1., 1., 1.))
    assert float(g[1].abs().max()) == 0.0


def test_identical_boxes_split_every_tie():
    """Identical boxes: min and max tie on all six faces and every corner gets half the gradient.  With the
    overlap = both volumes = V, d iou / d (size k) through the overlap is 2/V * (V/s_k) * 0.5 and through the
    prediction's volume -1/V * (V/s_k): they cancel exactly, and the centre gets 0.5 - 0.5."""
    w = lc.HYPER[8]
    siz = (1.0, 1.5, 0.5)
    sums, A, g, T = _one_row((.25, .5, .75), siz, (.25, .5, .75), siz)
    assert float(sums[6]) == 0.0
    assert float(g[1].abs().max()) == 0.0 and float(g[2].abs().max()) == 0.0
    for k in range(3):                                                    # the scale keeps both paths
        assert float(T[1][0, 3 + k]) == pytest.approx(2 * w / siz[k], rel=1e-12)
        assert float(T[1][0, k]) == 0.0
    # a tie on one face only (max-x faces coincide, prediction inside elsewhere): half of the un-tied weight
    sums, A, g, T = _one_row((.5, 0., 0.), (1., .5, .5), (0., 0., 0.), (2., 2., 2.))
    ov, uni = 0.25, 8.0
    d_hi = -w * (1 / uni + ov / uni ** 2) * 0.25 * 0.5                    # via the overlap, tie weight 0.5
    d_lo = -w * (1 / uni + ov / uni ** 2) * 0.25 * -1.0                   # min-x face: the prediction's alone
    d_a1 = w * ov / uni ** 2 * 0.25                                       # via a1, on d/d s_x
    assert float(g[1][0, 0]) == pytest.approx(d_hi + d_lo, rel=1e-12)
    assert float(g[1][0, 3]) == pytest.approx(0.5 * d_hi - 0.5 * d_lo + d_a1, rel=1e-12)


def test_edge_batch_sits_on_both_workgroups():
    case, placed = lc.head_edge_case()
    rows = [p for p, _ in placed]
    assert min(rows) == 0 and max(rows) == 299 and sum(p >= 256 for p in rows) == len(rows) // 2
    assert int(case["obj_t"].sum()) > len(rows) // 2


def test_loss_total_and_query_pos_restatements():
    rng = np.random.default_rng(3)
    vecs = [rng.standard_normal(7).astype(np.float32) for _ in range(3)]
    out = lr.loss_total_np(vecs, np.float32(0.5))
    np.testing.assert_allclose(out[:7], np.mean(np.stack(vecs).astype(np.float64), 0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(out[7], out[:7].astype(np.float64).sum() + 0.5, rtol=1e-6)
    gv, gvote = lr.loss_total_bwd_np(np.arange(8, dtype=np.float32), 3, True)
    assert gv.shape == (3, 7) and gvote == np.float32(7) and gv[2, 1] == np.float32(8) / np.float32(3)
    reg = rng.standard_normal((2, 5, 30)).astype(np.float32)
    base = rng.standard_normal((2, 5, 3)).astype(np.float32)
    q = lr.query_pos_rows_np(reg, base)
    assert q.shape == (10, 8) and q.dtype == np.float32 and not q[:, 6:].any()
    np.testing.assert_array_equal(q[7, :6], np.concatenate([base[1, 2] + reg[1, 2, :3], reg[1, 2, 3:6]]))


def test_fp32_composition_sets_the_constants(head, vote):
    """What ANY fp32 evaluation costs, in units of 2^-24 * scale: the project's torch composition in float32 on
    the CPU against the fp64 reference, over every case.  The constants of loss_cases are 4x this, rounded up to
    a power of two, so the composition has to stay within a quarter of each."""
    wf = wg = 0.0
    for name, (case, (sums, A, g, T)) in head.items():
        s, gs = lc.head_composition(case, torch.float32)
        wf = max(wf, lr.error_units(s, sums, A))
        wg = max(wg, max(lr.error_units(a, b, t) for a, b, t in zip(gs, g, T)))
    vf = vg = 0.0
    for name, (c, (v, count, gv, contrib)) in vote.items():
        s, gs = lc.vote_composition(c, torch.float32)
        vf = max(vf, lr.error_units(s, v, contrib.sum()))
        vg = max(vg, lr.error_units(gs, gv, gv.abs()))
    print("fp32 composition, units of 2^-24 * scale: head fwd %.2f grad %.2f, vote fwd %.2f grad %.2f"
          % (wf, wg, vf, vg))
    assert wf <= lc.C_F_HEAD / 4 and wg <= lc.C_G_HEAD / 4
    assert vf <= lc.C_F_VOTE / 4 and vg <= lc.C_G_VOTE / 4
