"""float64 restatement of the DISTANCE form of the head loss and of the test-time decode: the check of
ca_head_loss_fwd_k / ca_head_loss_bwd_k (csrc/loss.hip) and ca_detect_decode_k (csrc/detect.hip), beside
tests/loss_reference.py, whose helpers and conventions it shares.

Not a test module.  Written from the formulas of CAVoteHead.loss (class_agnostic_vote_head.py:40-121) and
ClassAgnosticBBoxCoder.split_pred / decode / decode_corners (class_agnostic_bbox_coder.py:42-137) on the kernels'
own row-form inputs, torch float64 on the CPU; tests/test_ca_reference_host.py holds it to the real reference classes'
output (tests/golden/ref_cavotehead.npz).

The scales are those of loss_reference.py: ``A[i]`` = sum over rows of |row contribution to loss i|; ``T`` per gradient
element = the sum of the absolute values of the additive terms that form it.  On the six log-distance columns
three terms meet: the SmoothL1 derivative (itself two terms inside the quadratic zone, see below), the IoU's path
through the overlap and its path through the predicted volume (each times d distance / d reg = distance).

The IoU is evaluated as the reference does, on corners that include the reference point: (ref - d[3:6], ref + d[0:3])
against the same from the targets.  Both boxes hang on the same point, so the loss VALUE does not depend on it, and with
constant targets (``ref_grad=False``) the gradient float64 autograd returns for ``ref`` is rounding noise.  The reference
does not hold the targets constant: it computes them from the proposal point without detaching it, and the point gets
a gradient through them (``ref_grad=True``, the default; see head_loss_ref).
"""
import numpy as np
import torch

import loss_reference as lr

F64 = torch.float64
NBINS, NSEM = lr.NBINS, lr.NSEM


def _iou_corners(lo1, hi1, lo2, hi2):
    """mmdet3d axis_aligned_bbox_overlaps_3d(is_aligned=True) on corners -> (iou, overlap, a1): extent clamped at 0
    (clamp passes the gradient AT 0), union floored at 1e-6, binary torch.max / torch.min (0.5 / 0.5 on a tie)."""
    e1, e2 = hi1 - lo1, hi2 - lo2
    a1 = e1[:, 0] * e1[:, 1] * e1[:, 2]
    a2 = e2[:, 0] * e2[:, 1] * e2[:, 2]
    ext = (torch.min(hi1, hi2) - torch.max(lo1, lo2)).clamp(min=0)
    ov = ext[:, 0] * ext[:, 1] * ext[:, 2]
    return ov / (a1 + a2 - ov).clamp(min=1e-6), ov, a1


def _local(ref, dir_t):
    """Rz(-yaw) ref: the part of the canonical coordinates (class_agnostic_vote_head.py:271-277) that depends on the
    proposal point, with mmdet3d's rotation_3d_in_axis convention; dir_t None: no rotation."""
    if dir_t is None:
        return ref
    c, s = torch.cos(-dir_t), torch.sin(-dir_t)
    return torch.stack([ref[:, 0] * c + ref[:, 1] * s, -ref[:, 0] * s + ref[:, 1] * c, ref[:, 2]], -1)


def head_loss_ref(cls, reg, ref, hyper12, distance_t, dir_class_t, dir_res_t, sem_t, obj_t, obj_w, box_w,
                  gout=None, dir_t=None, ref_grad=True):
    """-> (sums (7,), A (7,), (gcls, greg, gref) | None, (Tcls, Treg, Tref) | None), all float64, in
    ops.HEAD_LOSS_NAMES order with slot 4 (the centre loss this head does not have) 0; ``distance_t`` unclamped, as
    demf_proposal_targets writes it.  hyper12[6] and hyper12[11] are not read.
    ``ref_grad``: the distance targets carry their dependence on the reference point, as in the reference
    (:271-294: t = dims / 2 -+ Rz(-yaw) (point - centre), not detached): d t[0:3] = -Rz(-yaw) d ref, d t[3:6] = +Rz(-yaw)
    d ref, ``dir_t`` (R) the assigned boxes' yaw (None: no rotation).  False: the targets are constants."""
    h = lr.hyper_dict(hyper12)
    cls, reg, ref = (lr._f64(t).clone().requires_grad_() for t in (cls, reg, ref))
    raw_t = lr._f64(distance_t)
    if ref_grad:
        lin = _local(ref, None if dir_t is None else lr._f64(dir_t))
        lin = torch.cat([-lin, lin], -1)
        raw_t = raw_t + (lin - lin.detach())                                 # the value of distance_t, the slope of :279-284
    dist_t = raw_t.clamp(min=0)                                              # class_agnostic_vote_head.py:301
    dir_res_t, obj_w, box_w = map(lr._f64, (dir_res_t, obj_w, box_w))
    dt, st, ot = lr._i64(dir_class_t), lr._i64(sem_t), lr._i64(obj_t)
    R = cls.shape[0]
    assert cls.shape == (R, 2 + NSEM) and reg.shape == (R, 6 + 2 * NBINS) and ref.shape == (R, 3)
    d = torch.exp(reg[:, 0:6])
    cw = torch.where(ot != 0, torch.full((R,), h["cw1"], dtype=F64), torch.full((R,), h["cw0"], dtype=F64))
    ce_obj, p_obj = lr._ce_rows(cls[:, 0:2], ot)
    ce_dir, p_dir = lr._ce_rows(reg[:, 6:6 + NBINS], dt)
    ce_sem, p_sem = lr._ce_rows(cls[:, 2:2 + NSEM], st)
    res = reg[:, 6 + NBINS:].gather(1, dt.view(-1, 1)).squeeze(1)
    # decode_corners: (ref - d[3:6], ref + d[0:3])
    iou, ov, a1 = _iou_corners(ref - d[:, 3:6], ref + d[:, 0:3], ref - dist_t[:, 3:6], ref + dist_t[:, 0:3])
    w_obj_row = h["w_obj"] * obj_w * cw
    zero = torch.zeros(R, dtype=F64)
    rows = [w_obj_row * ce_obj,
            h["w_dircls"] * box_w * ce_dir,
            h["w_dirres"] * box_w * lr._smooth_l1(res - dir_res_t, h["beta_dirres"]),
            h["w_size"] * box_w * lr._smooth_l1(d - dist_t, h["beta_size"]).sum(1),
            zero,
            h["w_sem"] * box_w * ce_sem,
            h["w_iou"] * box_w * (1 - iou)]
    sums = torch.stack([r.sum() for r in rows])
    A = torch.stack([r.detach().abs().sum() for r in rows])
    if gout is None:
        return sums.detach(), A, None, None
    g = lr._f64(gout)
    leaves = (cls, reg, ref)

    def grads(out, seed=None):
        gs = torch.autograd.grad(out, leaves, grad_outputs=seed, retain_graph=True, allow_unused=True)
        return [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, gs)]

    total = grads((g * sums).sum())
    T = [torch.zeros_like(l) for l in leaves[:2]]
    for t, x in zip(T, grads(g[2] * sums[2])):            # SmoothL1 of the residual: one additive term per element
        t += x.abs()
    # SmoothL1 of the distances.  d = exp(reg) is a ROUNDED number in fp32 (the inputs of the other SmoothL1 terms lie
    # on the grid), so inside the quadratic zone the derivative (d - t) / beta is the sum of two terms, d / beta and
    # -t / beta, that nearly cancel when the prediction is good; outside it is the sign.  Times d (= d distance / d reg).
    dd, tt = d.detach(), dist_t.detach()
    inside = (dd - tt).abs() < h["beta_size"]
    sl1 = (g[3] * h["w_size"] * box_w).abs().unsqueeze(1) * \
        torch.where(inside, (dd + tt) / h["beta_size"], (dd != tt).to(F64))
    T[1][:, 0:6] += sl1 * dd
    G6 = sl1 * (lr._f64(distance_t) >= 0).to(F64)         # |terms| behind d total / d raw target (clamp passes AT 0)
    oh = lambda t, k: torch.nn.functional.one_hot(t, k).to(F64)             # noqa: E731
    T[0][:, 0:2] += (g[0] * w_obj_row).abs().unsqueeze(1) * (p_obj.detach() + oh(ot, 2))
    T[1][:, 6:6 + NBINS] += (g[1] * h["w_dircls"] * box_w).abs().unsqueeze(1) * (p_dir.detach() + oh(dt, NBINS))
    T[0][:, 2:2 + NSEM] += (g[5] * h["w_sem"] * box_w).abs().unsqueeze(1) * (p_sem.detach() + oh(st, NSEM))
    # IoU: through the overlap and through the predicted volume, separately.  The paths are taken from the
    # DISTANCES on (d ov / d ref and d a1 / d ref cancel term against term and are no part of the scale)
    d_ov, d_a1 = torch.autograd.grad(g[6] * sums[6], (ov, a1), retain_graph=True)
    for out, seed in ((ov, d_ov), (a1, d_a1)):
        (gd,) = torch.autograd.grad(out, d, grad_outputs=seed, retain_graph=True)
        T[1][:, 0:6] += (gd * d.detach()).abs()
    Tref = torch.zeros_like(ref)
    if ref_grad:
        # the reference point's gradient: the targets' side of the SmoothL1 term and of the IoU (through the overlap and
        # through the TARGET's volume, which sits in the union), rotated back: |Rz|^T applied to the per-face sums
        # (d iou / d a2 = d iou / d a1: both volumes enter through the union)
        (g_ov,) = torch.autograd.grad(ov, raw_t, grad_outputs=d_ov, retain_graph=True)
        t_side = dist_t[:, 0:3] + dist_t[:, 3:6]
        a2 = t_side[:, 0] * t_side[:, 1] * t_side[:, 2]
        (g_a2,) = torch.autograd.grad(a2, raw_t, grad_outputs=d_a1, retain_graph=True, allow_unused=True)
        G6 = G6 + g_ov.abs() + (torch.zeros_like(G6) if g_a2 is None else g_a2.abs())
        per_axis = G6[:, 0:3] + G6[:, 3:6]
        if dir_t is None:
            Tref = per_axis
        else:
            c, s = torch.cos(lr._f64(dir_t)).abs(), torch.sin(lr._f64(dir_t)).abs()
            Tref = torch.stack([per_axis[:, 0] * c + per_axis[:, 1] * s, per_axis[:, 0] * s + per_axis[:, 1] * c,
                                per_axis[:, 2]], -1)
    return sums.detach(), A, tuple(total), (T[0], T[1], Tref.detach())


def decode_ref(reg_rows, cls_rows, ref, num_dir_bins=NBINS, with_rot=True):
    """ClassAgnosticBBoxCoder.decode + the scoring of VoteHead.get_bboxes on the raw rows (B, K, .) in float64.
    -> dict(box7, cos, sin, obj, sem, classes, scale7): ``scale7`` (B, K, 7) is the sum of the absolute additive
    terms behind every box element -
      size   d_k + d_3+k; an element the 0.1 clamp replaces is the float32 number 0.1 exactly (scale 0);
      yaw    2 pi + |class angle| + |residual|;
      centre |ref_k| + the distances of its axis / 2 (z), and for x / y, where the yaw enters,
             |ref_k| + 8 * (d_0 + d_3 + d_1 + d_4) / 2: a yaw off by u units of 2^-24 * 2 pi moves the rotated offset by
             at most (|x| + |y|) * 2 pi * u * 2^-24, and 1 + 2 pi < 8."""
    reg, cls, ref = lr._f64(reg_rows), lr._f64(cls_rows), lr._f64(ref)
    nb = num_dir_bins
    d = torch.exp(reg[..., 0:6])
    if with_rot:
        best = torch.argmax(reg[..., 6:6 + nb], -1)
        res = reg[..., 6 + nb:6 + 2 * nb].gather(-1, best.unsqueeze(-1)).squeeze(-1) * (np.pi / nb)
        cls_angle = best.to(F64) * (2 * np.pi / nb)
        angle = cls_angle + res
        angle = torch.where(angle > np.pi, angle - 2 * np.pi, angle)
        yaw = torch.remainder(angle, 2 * np.pi)
        yaw_scale = 2 * np.pi + cls_angle.abs() + res.abs()
    else:
        yaw = torch.zeros(reg.shape[:-1], dtype=F64)
        yaw_scale = torch.zeros_like(yaw)
    raw = d[..., 0:3] + d[..., 3:6]
    clamp = float(np.float32(0.1))
    size = torch.where(raw < clamp, torch.full_like(raw, clamp), raw)
    size_scale = torch.where(raw < clamp, torch.zeros_like(raw), raw)
    x, y, z = ((d[..., 3 + k] - d[..., k]) / 2 for k in range(3))
    c, s = torch.cos(yaw), torch.sin(yaw)
    centre = torch.stack([ref[..., 0] - (x * c + y * s), ref[..., 1] - (-x * s + y * c), ref[..., 2] - z], -1)
    half = raw / 2
    xy = 8 * (half[..., 0] + half[..., 1])
    centre_scale = ref.abs() + torch.stack([xy, xy, half[..., 2]], -1)
    sem = torch.softmax(cls[..., 2:], -1)
    return dict(box7=torch.cat([centre, size, yaw.unsqueeze(-1)], -1), cos=c, sin=s,
                obj=torch.softmax(cls[..., 0:2], -1)[..., 1], sem=sem, classes=torch.argmax(sem, -1),
                scale7=torch.cat([centre_scale, size_scale, yaw_scale.unsqueeze(-1)], -1))
