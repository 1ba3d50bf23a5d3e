"""Inputs of the loss-kernel edge tests (tests/test_gpu_loss_edges.py) and of the CPU measurement of what an
fp32 evaluation of the same losses costs (tests/test_loss_reference_host.py).  Not a test module.

Everything is built on the CPU as fp32 / int64 tensors - the kernels' own row-form inputs - from seeded
generators, so the GPU test, the fp64 reference and the fp32 torch composition see identical numbers."""
import types

import numpy as np
import torch

_f = lambda v: float(np.float32(v))
# cw0, cw1, w_obj, w_dircls, w_dirres, w_size, w_center, w_sem, w_iou, beta_dirres, beta_size, beta_center
# (the head's configuration, demf_amd/config.py), as the fp32 numbers the kernel receives
HYPER = tuple(_f(v) for v in (0.2, 0.8, 5.0, 1.0, 10.0, 10.0, 10.0, 1.0, 12.0 / 3.0, 1.0, 0.0625, 1.0 / 9.0))
B9 = HYPER[11]                                   # fp32(1/9)
GOUT = torch.tensor([0.75 * (i + 1) for i in range(7)], dtype=torch.float32)    # a swapped slot shows
HEAD_KEYS = ("cls", "reg", "base", "center_t", "size_t", "dir_class_t", "dir_res_t", "sem_t", "obj_t", "obj_w",
             "box_w")
HEAD_ROWS = (1, 63, 64, 255, 256, 257, 513, 2048, 2049)
VOTE_GOUT = 1.7
VOTE_DST_WEIGHT = 10.0
VOTE_SHAPES = ((1, 1, 7), (1, 255, 100), (2, 128, 300), (1, 2047, 500), (8, 256, 400), (1, 2049, 600),
               (3, 683, 500), (5, 821, 300), (8, 1024, 4096))

# Tolerance constants, in units of 2^-24 * scale (scales A and T of tests/loss_reference.py).  Each is 4x the
# worst error of the project's fp32 torch composition (head_composition / vote_composition below, on the CPU)
# against the fp64 reference over ALL the cases of this module, rounded up to a power of two; the factor covers
# the kernels' different summation order (256-wide tree + atomics) and their fast exp / log intrinsics.
# tests/test_loss_reference_host.py::test_fp32_composition_sets_the_constants re-measures the composition.
#                     fp32 composition   kernel (MI355X)
C_F_HEAD = 16.0     # 2.31               2.90
C_G_HEAD = 64.0     # 9.50               21.03 (rows with a logit gap of 30: __expf)
C_F_VOTE = 8.0      # 1.52               1.95
C_G_VOTE = 8.0      # 1.72               1.72


def _q(t):
    """Onto the 2^-10 grid.  Coordinates, sizes and residuals (|x| < 16) and their targets live on it, so that
    every DIFFERENCE of inputs the losses start from (centre - target, corner - corner, vote - target) is exact
    in fp32 and in fp64 alike: the tolerances then measure the arithmetic of the loss, not the conditioning of
    subtracting two nearly equal inputs, which no kernel can do anything about."""
    return torch.round(t * 1024) / 1024


def _weights(obj_mask, obj_t):
    ow = obj_mask / (obj_mask.sum() + 1e-6)
    bw = obj_t.float() / (obj_t.sum().float() + 1e-6)
    return ow.float(), bw.float()


def head_case(R, seed, pos_frac=0.3, mask_frac=0.8):
    """Random rows; about ``pos_frac`` positive (at least one when pos_frac > 0), ``mask_frac`` of the rows
    carry an objectness weight."""
    g = torch.Generator().manual_seed(1000 * seed + R)
    r = lambda *s: torch.randn(*s, generator=g)
    base = _q(r(R, 3) * 2)
    obj_t = (torch.rand(R, generator=g) < pos_frac).long()
    if pos_frac > 0:
        obj_t[R // 2] = 1
    obj_mask = (torch.rand(R, generator=g) < mask_frac).float()
    ow, bw = _weights(obj_mask, obj_t)
    reg = r(R, 30) * 0.7
    # positive predicted sizes: a negative one can bring the union a1 + a2 - overlap next to 0, where the IoU
    # is ill-conditioned in ANY fp32 evaluation (d iou ~ 1 / union^2) and a tolerance says nothing about the
    # kernel.  Signed volumes are pinned by exact rows of the edge batch instead.
    reg[:, 3:6] = torch.rand(R, 3, generator=g) + 0.3
    reg[:, 0:6] = _q(reg[:, 0:6])
    reg[:, 18:30] = _q(reg[:, 18:30])
    return dict(cls=r(R, 12), reg=reg, base=base, center_t=_q(base + 0.3 * r(R, 3)),
                size_t=_q(torch.rand(R, 3, generator=g) + 0.4), dir_class_t=torch.randint(0, 12, (R,), generator=g),
                dir_res_t=_q(r(R) * 0.3), sem_t=torch.randint(0, 10, (R,), generator=g), obj_t=obj_t, obj_w=ow,
                box_w=bw)


def _edge_rows():
    """Rows that sit ON the branch points.  Every number is a multiple of 1/8 (or fp32(1/9), the centre
    beta, against zeros), so fp32 and fp64 arithmetic agree on every comparison.  Keys: cen / siz (predicted
    centre and size; reg[0:3] = cen - base), base, ct / st (target centre / size), dirlog (12), dt, res (the
    residual AT column dt), rt (its target), sem (10), semt, obj (2), ot."""
    rows = []
    add = lambda **kw: rows.append(kw)
    # SmoothL1, direction residual (beta 1): |d| below / at / above beta, d = 0, both signs
    for d in (0.5, 1.0, 1.5, 0.0, -0.5, -1.0, -1.5):
        add(res=d + 0.25, rt=0.25, dt=len(rows) % 12)
    # SmoothL1, size (beta 1/16): three differences per row
    for d in ((1 / 32, 1 / 16, 1 / 8), (0.0, -1 / 32, -1 / 8), (-1 / 16, 1 / 16, 0.0)):
        add(siz=tuple(1.0 + x for x in d), st=(1.0, 1.0, 1.0))
    # SmoothL1, centre (beta fp32(1/9)): base 0 and target 0, so the difference IS the stored number
    for d in ((1 / 16, B9, 1 / 8), (0.0, -1 / 16, -1 / 8), (-B9, B9, 0.0)):
        add(cen=d, ct=(0.0, 0.0, 0.0), base=(0.0, 0.0, 0.0))
    b = (1.0, -2.0, 0.5)
    one = (1.0, 1.0, 1.0)
    add(cen=(0, 0, 0), siz=one, ct=(3, 0, 0), st=one, base=b)                          # disjoint on x
    add(cen=(.5, .5, .5), siz=one, ct=(1.5, .5, .5), st=one, base=b)                  # touching on x only
    add(cen=(.5, .5, .5), siz=one, ct=(.5, -.5, .5), st=one, base=b)                  # touching on y only
    add(cen=(0, 0, 0), siz=(.5, .5, .5), ct=(.125, 0, 0), st=(2, 2, 2), base=b)       # prediction inside target
    add(cen=(.125, 0, 0), siz=(2, 2, 2), ct=(0, 0, 0), st=(.5, .5, .5), base=b)       # target inside prediction
    add(cen=(.25, .5, .75), siz=(1, 1.5, .5), ct=(.25, .5, .75), st=(1, 1.5, .5), base=b)   # identical: six ties
    add(cen=(0, 0, 0), siz=(1, 1, 1), ct=(.5, 0, 0), st=(2, 1, 1.5))                  # ties on four faces
    add(cen=(0, 0, 0), siz=(-.5, 1, 1), ct=(0, 0, 0), st=one)                         # signed a1 < 0, union > 0
    add(cen=(0, 0, 0), siz=(-.5, -1, 1), ct=(0, 0, 0), st=one)                        # two negative sizes
    t = 2.0 ** -8
    add(cen=(0, 0, 0), siz=(t, t, t), ct=(t / 4, 0, 0), st=(t, t, t), base=(0.0, 0.0, 0.0))   # union < 1e-6
    add(cen=(0, 0, 0), siz=(-2, 1, 1), ct=(0, 0, 0), st=one)                          # union < 0
    # cross entropies
    z12, z10 = [0.0] * 12, [0.0] * 10
    add(dirlog=[30.0] + z12[1:], dt=0, sem=[30.0] + z10[1:], semt=0, obj=(0.0, 30.0))     # target dominates
    add(dirlog=z12[:11] + [-30.0], dt=11, sem=z10[:9] + [-30.0], semt=9, obj=(0.0, -30.0))  # target at -30
    add(dirlog=[1.5] * 12, dt=5, sem=[-2.0] * 10, semt=9, obj=(0.25, 0.25))              # all equal
    add(dirlog=z12[:11] + [30.0], dt=11, sem=z10[:9] + [30.0], semt=9)                    # last index dominates
    add(dirlog=[-30.0] + z12[1:], dt=0, sem=[-30.0] + z10[1:], semt=0)
    add(ot=0, obj=(30.0, 0.0))                                                         # negatives: objectness only
    add(ot=0, obj=(-30.0, 0.0))
    add(ot=0, obj=(0.5, 0.5))
    return rows


def head_edge_case(R=300, seed=7):
    """The edge rows inside a random batch of ``R`` rows: once from row 0 on (first workgroup) and once at the end
    (second workgroup), the last edge row on row R - 1.  -> (case, positions of the copies: list of (row, spec))."""
    c = head_case(R, seed, pos_frac=0.3, mask_frac=1.0)
    obj_mask = torch.ones(R)
    rows = _edge_rows()
    E = len(rows)
    assert 256 + E <= R
    placed = []
    res_fill = torch.tensor([(3 * k % 7 - 3) / 8 + (0.125 if (3 * k % 7 - 3) == 0 else 0.0) for k in range(12)])
    for start in (0, R - E):
        for i, s in enumerate(rows):
            p = start + i
            base = torch.tensor(s.get("base", (0.0, 0.0, 0.0)), dtype=torch.float32)
            cen = torch.tensor(s.get("cen", (0.0, 0.0, 0.0)), dtype=torch.float32)
            dt = int(s.get("dt", 3))
            c["base"][p] = base
            c["reg"][p, 0:3] = cen - base
            c["reg"][p, 3:6] = torch.tensor(s.get("siz", (1.0, 1.0, 1.0)), dtype=torch.float32)
            c["reg"][p, 6:18] = torch.tensor(s.get("dirlog", [0.0] * 12), dtype=torch.float32)
            c["reg"][p, 18:30] = res_fill                  # every residual column non-zero: only dt may count
            c["reg"][p, 18 + dt] = float(s.get("res", 0.5))
            c["center_t"][p] = torch.tensor(s.get("ct", (0.25, -0.125, 0.0)), dtype=torch.float32)
            c["size_t"][p] = torch.tensor(s.get("st", (1.0, 1.25, 0.75)), dtype=torch.float32)
            c["dir_class_t"][p] = dt
            c["dir_res_t"][p] = float(s.get("rt", 0.25))
            c["cls"][p, 0:2] = torch.tensor(s.get("obj", (0.0, 0.0)), dtype=torch.float32)
            c["cls"][p, 2:12] = torch.tensor(s.get("sem", [0.0] * 10), dtype=torch.float32)
            c["sem_t"][p] = int(s.get("semt", 4))
            c["obj_t"][p] = int(s.get("ot", 1))
            placed.append((p, s))
    c["obj_w"], c["box_w"] = _weights(obj_mask, c["obj_t"])
    return c, placed


def head_cases():
    """name -> case: every row count of HEAD_ROWS, no positive row, zero objectness weights, the edge batch."""
    out = {"R%d" % R: head_case(R, 1) for R in HEAD_ROWS}
    out["nopos257"] = head_case(257, 2, pos_frac=0.0)
    out["objw0_513"] = head_case(513, 3, mask_frac=0.4)
    out["edges300"] = head_edge_case()[0]
    return out


def head_composition(case, dtype, hyper=HYPER, gout=GOUT):
    """The project's torch composition (demf_amd/modules/losses.py, combined as DeMFVoteHead._loss combines
    them) on the row form, in ``dtype`` on the CPU -> (sums (7,), (gcls, greg, gbase))."""
    from demf_amd.modules import losses as L
    h = dict(zip(("cw0", "cw1", "w_obj", "w_dircls", "w_dirres", "w_size", "w_center", "w_sem", "w_iou",
                  "beta_dirres", "beta_size", "beta_center"), hyper))
    fl = lambda k: case[k].to(dtype)
    cls, reg, base = (fl(k).clone().requires_grad_() for k in ("cls", "reg", "base"))
    cen, siz = base + reg[:, 0:3], reg[:, 3:6]
    bw = fl("box_w")
    w3 = bw.unsqueeze(-1).repeat(1, 3)
    corners = lambda c, s: torch.cat([c - s / 2.0, c + s / 2.0], dim=-1)
    one_hot = torch.nn.functional.one_hot(case["dir_class_t"], 12).to(dtype)
    res = torch.sum(reg[:, 18:30] * one_hot, -1)
    sums = torch.stack([
        L.cross_entropy_sum(cls[:, 0:2], case["obj_t"], fl("obj_w"), torch.tensor([h["cw0"], h["cw1"]], dtype=dtype),
                            h["w_obj"]),
        L.cross_entropy_sum(reg[:, 6:18], case["dir_class_t"], bw, None, h["w_dircls"]),
        L.smooth_l1_sum(res, fl("dir_res_t"), bw, h["beta_dirres"], h["w_dirres"]),
        L.smooth_l1_sum(siz, fl("size_t"), w3, h["beta_size"], h["w_size"]),
        L.smooth_l1_sum(cen, fl("center_t"), w3, h["beta_center"], h["w_center"]),
        L.cross_entropy_sum(cls[:, 2:12], case["sem_t"], bw, None, h["w_sem"]),
        L.axis_aligned_iou_loss_sum(corners(cen, siz), corners(fl("center_t"), fl("size_t")), bw, h["w_iou"])])
    grads = torch.autograd.grad((gout.to(dtype) * sums).sum(), (cls, reg, base))
    return sums.detach(), grads


# ---- vote loss ------------------------------------------------------------------------------------------------
def vote_case(B, S, N, seed, positive=True, exact_zero=False):
    """Vote targets in the form vote_targets_k writes: zeros off the boxes, three copies of one vote on most
    points inside, three distinct votes on about one in ten.  The positive fraction differs per scene (0.1 ..
    0.7, about 0.4 overall), so a seed counted in the wrong scene changes the count.  ``exact_zero``: some seeds
    get vote == target + seed exactly on components 0 and 2 (multiples of 1/8, exact in fp32 and fp64)."""
    g = torch.Generator().manual_seed(77 * seed + B * S)
    r = lambda *s: torch.randn(*s, generator=g)
    frac = torch.linspace(0.1, 0.7, B).view(B, 1) if B > 1 else torch.full((1, 1), 0.4)
    masks = (torch.rand(B, N, generator=g) < frac).long() if positive else torch.zeros(B, N, dtype=torch.long)
    v1 = _q(r(B, N, 3))
    vt = v1.repeat(1, 1, 3)
    distinct = torch.rand(B, N, generator=g) < 0.1
    vt = torch.where(distinct.unsqueeze(-1), _q(r(B, N, 9)), vt) * masks.unsqueeze(-1).float()
    seed_idx = torch.randint(0, N, (B, S), generator=g)
    if positive and B * S <= 2:
        masks[:, seed_idx.view(-1)] = 1                                   # a lone seed: make it count
    seed_pts = _q(r(B, S, 3))
    tgt = torch.gather(vt, 1, seed_idx.unsqueeze(-1).expand(-1, -1, 9))[..., :3]
    vote = _q(seed_pts + tgt + 0.2 * r(B, S, 3))
    if exact_zero:
        for b in range(B):
            for s in range(0, S, 5):
                k = int(seed_idx[b, s])
                if not masks[b, k]:
                    continue
                e = torch.tensor([(s % 9 - 4) / 8, 0.375, ((s // 3) % 7 - 3) / 8])
                vt[b, k] = e.repeat(3)
        snap = torch.round(seed_pts * 8) / 8
        for b in range(B):
            for s in range(0, S, 5):
                k = int(seed_idx[b, s])
                if masks[b, k]:
                    seed_pts[b, s] = snap[b, s]
        tgt = torch.gather(vt, 1, seed_idx.unsqueeze(-1).expand(-1, -1, 9))[..., :3]
        for b in range(B):
            for s in range(0, S, 5):
                if masks[b, int(seed_idx[b, s])]:
                    vote[b, s, 0] = tgt[b, s, 0] + seed_pts[b, s, 0]
                    vote[b, s, 2] = tgt[b, s, 2] + seed_pts[b, s, 2]
    return dict(vote=vote.contiguous(), seed=seed_pts.contiguous(), seed_idx=seed_idx, masks=masks,
                vote_targets=vt.contiguous())


def vote_cases():
    out = {"%dx%dx%d" % s: vote_case(*s, seed=i) for i, s in enumerate(VOTE_SHAPES)}
    out["nopos_3x100x50"] = vote_case(3, 100, 50, seed=20, positive=False)
    out["sign0_2x300x40"] = vote_case(2, 300, 40, seed=21, exact_zero=True)
    return out


def vote_composition(case, dtype, gout=VOTE_GOUT):
    """demf_amd VoteModule.get_loss in ``dtype`` on the CPU -> (value, grad wrt vote)."""
    from demf_amd.modules.vote import VoteModule
    me = types.SimpleNamespace(gt_per_seed=3, vote_loss_dst_weight=VOTE_DST_WEIGHT)
    vote = case["vote"].to(dtype).clone().requires_grad_()
    v = VoteModule.get_loss(me, case["seed"].to(dtype), vote, case["seed_idx"], case["masks"],
                            case["vote_targets"].to(dtype))
    (gv,) = torch.autograd.grad(v * gout, vote)
    return v.detach(), gv
