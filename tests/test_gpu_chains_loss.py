"""The reworked head-loss and vote-loss kernels of csrc/loss.hip at the edges of THEIR tiling, against the float64
reference of tests/loss_reference.py under the bounds and constants of tests/test_gpu_loss_edges.py (whose checks
are reused as they stand: C_F_HEAD / C_G_HEAD / C_F_VOTE / C_G_VOTE of tests/loss_cases.py, unchanged).

Head losses: a wave owns 64 rows (T = 64); up to 256 rows run as ONE workgroup of four waves, more as one wave per
workgroup.  Rows 1, T-1, T, T+1, 2T+1 fall into the first form, 256 / 257 / 321 / 513 sit on and past the switch
(257 = four full waves and a one-row tile, 513 = 2 * 256 + 1).  Positives only in the last partial tile, no positive at
all past the switch, and every target direction class on the first or last bin (the residual column is read from
LDS at a run-time index: columns 18 and 29 of the row are its ends).

Vote loss: a workgroup owns 256 seeds, a wave 64; the count and the unscaled sum are combined over the workgroups by
the last one to arrive.  B*S of 1, 255 (three scenes of 85: scene boundaries inside waves 1 and 2), 257 (one workgroup
and one seed), 8 223 = 3 * 2 741 (33 workgroups, the last one partial, boundaries inside waves); an all-zero mask (one
workgroup, and many: the last workgroup scales a zero sum by 1 / 1e-6) and a mask with one positive point."""
import pytest
import torch

import loss_cases as lc
import loss_reference as lr
import test_gpu_loss_edges as le

pytestmark = pytest.mark.gpu

T = 64
HEAD_ROWS = (1, T - 1, T, T + 1, 2 * T + 1, 256, 257, 321, 513)


def _head_ref(case):
    return lr.head_loss_ref(*[case[k] for k in lc.HEAD_KEYS[:3]], lc.HYPER, *[case[k] for k in lc.HEAD_KEYS[3:]],
                            gout=lc.GOUT)


def _positives_at(case, rows):
    R = case["obj_t"].numel()
    case["obj_t"] = torch.zeros(R, dtype=torch.long)
    case["obj_t"][rows] = 1
    case["box_w"] = lc._weights(torch.ones(R), case["obj_t"])[1]
    return case


@pytest.fixture(scope="module")
def head_cases():
    out = {"R%d" % R: lc.head_case(R, 11) for R in HEAD_ROWS}
    out["nopos321"] = lc.head_case(321, 12, pos_frac=0.0)
    out["lastwave_193"] = _positives_at(lc.head_case(193, 13), [192])            # four-wave form: its last, one-row wave
    out["lasttile_321"] = _positives_at(lc.head_case(321, 14), [320])            # one-wave form: its last, one-row tile
    out["lasttile_383"] = _positives_at(lc.head_case(383, 15), list(range(320, 383)))
    for R in (130, 300):
        c = lc.head_case(R, 16, pos_frac=0.6)
        c["dir_class_t"] = torch.where(torch.arange(R) % 2 == 0, 0, 11)
        out["dirends_%d" % R] = c
    return out


@pytest.fixture(scope="module")
def head_refs(head_cases):
    return {n: _head_ref(c) for n, c in head_cases.items()}


@pytest.mark.parametrize("R", HEAD_ROWS)
def test_head_loss_tile_edges(R, head_cases, head_refs):
    name = "R%d" % R
    got, _ = le._check_head(name, head_cases[name], head_refs[name])
    if R <= 256:                                     # one workgroup, one atomic per output: the same bits again
        again, _ = le._head_gpu(head_cases[name], backward=False)
        assert torch.equal(got, again)


def test_head_loss_no_positive_row_past_the_switch(head_cases, head_refs):
    case = head_cases["nopos321"]
    assert float(case["box_w"].abs().max()) == 0.0
    got, gg = le._check_head("nopos321", case, head_refs["nopos321"])
    assert float(got[0]) > 0.0 and float(got[1:].abs().max()) == 0.0
    assert float(gg[1].abs().max()) == 0.0 and float(gg[2].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["lastwave_193", "lasttile_321", "lasttile_383"])
def test_head_loss_positives_only_in_the_last_partial_tile(name, head_cases, head_refs):
    case = head_cases[name]
    first = int(case["obj_t"].nonzero()[0])
    assert first % T == 0 and first + T > case["obj_t"].numel()
    got, gg = le._check_head(name, case, head_refs[name])
    assert float(got[1:].abs().min()) > 0.0          # every box loss saw the tile
    assert float(gg[1][:first].abs().max()) == 0.0 and float(gg[1][first:].abs().max()) > 0.0


@pytest.mark.parametrize("R", [130, 300])
def test_head_loss_direction_class_on_the_first_and_last_bin(R, head_cases, head_refs):
    name = "dirends_%d" % R
    case = head_cases[name]
    assert set(case["dir_class_t"].tolist()) == {0, 11}
    le._check_head(name, case, head_refs[name])      # (it also pins the residual gradient to column 18 + dt)


# ---- vote loss ------------------------------------------------------------------------------------------------
VOTE_SHAPES = ((1, 1, 7), (3, 85, 60), (1, 257, 100), (3, 2741, 500))


def _single_positive(c):
    k = int(c["seed_idx"][1, 40])
    c["masks"] = torch.zeros_like(c["masks"])
    c["masks"][1, k] = 1
    c["vote_targets"] = c["vote_targets"] * c["masks"].unsqueeze(-1).float()
    return c


@pytest.fixture(scope="module")
def vote_cases():
    out = {"%dx%dx%d" % s: lc.vote_case(*s, seed=30 + i) for i, s in enumerate(VOTE_SHAPES)}
    out["nopos_3x85x60"] = lc.vote_case(3, 85, 60, seed=40, positive=False)
    out["nopos_3x2741x500"] = lc.vote_case(3, 2741, 500, seed=41, positive=False)
    out["onepos_3x85x600"] = _single_positive(lc.vote_case(3, 85, 600, seed=42))
    return out


@pytest.fixture(scope="module")
def vote_refs(vote_cases):
    return {n: lr.vote_loss_ref(c["vote"], c["seed"], c["seed_idx"], c["masks"], c["vote_targets"], 3,
                                lc.VOTE_DST_WEIGHT, lc.VOTE_GOUT) for n, c in vote_cases.items()}


@pytest.mark.parametrize("shape", VOTE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_vote_loss_pass_and_wave_edges(shape, vote_cases, vote_refs):
    name = "%dx%dx%d" % shape
    _, _, live = le._check_vote(name, vote_cases[name], vote_refs[name])   # the count, exactly, through the backward
    assert int(live.sum()) > 0
    B, S, _ = shape
    assert B == 1 or any((b * S) % 64 for b in range(1, B)), "no scene boundary inside a wave"


@pytest.mark.parametrize("name", ["nopos_3x85x60", "nopos_3x2741x500"])
def test_vote_loss_all_zero_mask(name, vote_cases, vote_refs):
    got, gg, live = le._check_vote(name, vote_cases[name], vote_refs[name])
    assert float(got) == 0.0 and float(gg.abs().max()) == 0.0 and int(live.sum()) == 0


def test_vote_loss_single_positive_point(vote_cases, vote_refs):
    name = "onepos_3x85x600"
    c = vote_cases[name]
    assert int(c["masks"].sum()) == 1
    count = vote_refs[name][1]
    assert 1 <= count <= 3                           # the seeds that sit on the one positive point
    le._check_vote(name, c, vote_refs[name])


# ---- vote targets: the staged, contiguous stores ----------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (2, 255), (2, 256), (3, 513)])
def test_vote_targets_bit_exact_around_one_workgroup(B, N):
    """demf_vote_targets against its torch specification (DeMFVoteHead.vote_targets on the CPU), bit for bit, at
    point counts around the 256-point workgroup: the last workgroup of a scene stores a partial run, and the next
    scene's rows start right behind it - the stores' addresses are what changed."""
    import numpy as np
    from demf_amd import ops
    from demf_amd.modules.head import DeMFVoteHead
    rng = np.random.default_rng(1000 * B + N)
    pts = rng.uniform([-3, -3, 0, 0], [3, 3, 3, 3], size=(B, N, 4)).astype(np.float32)
    G = 5
    gt = np.zeros((B, G, 7), np.float32)
    gt[..., :3] = rng.uniform([-2.5, -2.5, 0], [2.5, 2.5, 1.5], size=(B, G, 3))
    gt[..., 3:6] = rng.uniform(2.0, 5.0, size=(B, G, 3))             # big boxes: 0, 1, 2 and >= 3 hits per point
    gt[..., 6] = rng.uniform(-np.pi, np.pi, size=(B, G))
    head = DeMFVoteHead.__new__(DeMFVoteHead)                        # vote_targets uses no state
    boxes = [torch.from_numpy(gt[b][:G - b]) for b in range(B)]      # unequal box counts: padded slots exist
    labels = [torch.zeros(len(bx), dtype=torch.long) for bx in boxes]
    spec = DeMFVoteHead.vote_targets(head, torch.from_numpy(pts), boxes, labels)
    g_pad, _, v_pad = DeMFVoteHead.pad_gt(boxes, labels, torch.device("cpu"))
    vt, mask = ops.vote_targets(torch.from_numpy(pts).cuda(), g_pad.cuda(), v_pad.cuda())
    np.testing.assert_array_equal(mask.cpu().numpy(), spec["vote_target_masks"].numpy())
    np.testing.assert_array_equal(vt.cpu().numpy(), spec["vote_targets"].numpy())
    assert N == 1 or 0 < int(spec["vote_target_masks"].sum()) < B * N
