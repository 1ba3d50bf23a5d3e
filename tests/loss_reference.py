"""float64 restatement of the head losses, the vote loss, ``loss_total`` and ``query_pos_rows``: the check
of the fused kernels in csrc/loss.hip.

Not a test module.  Written from the formulas ([dep-recall]: mmdet CrossEntropyLoss / SmoothL1Loss, mmdet3d
AxisAlignedIoULoss and VoteModule.get_loss with reduction='sum', as restated in oracle/deps.py), on the
kernels' own row-form inputs, torch float64 on the CPU.  None of demf_amd/modules/losses.py is used here;
tests/test_loss_reference_host.py compares the two (and the oracle's classes) to 1e-12.

Besides values and autograd gradients the functions return the SCALES the tolerances of the GPU tests are
expressed in:

* ``A[i]``: sum over rows of |row contribution to loss i|.  An fp32 evaluation of a sum of R terms is off by
  some multiple of 2^-24 * sum |term|, whatever the order of the summation.
* ``T``, per gradient element: the sum of the absolute values of the additive terms that form it.  A term is
  what an fp32 evaluation has to add: for a cross entropy the softmax and the one-hot term (|g| * (p_i +
  [i == target]); when the target logit dominates, p_t - 1 cancels to ~1e-12 and no fp32 code can resolve
  it), for SmoothL1 its derivative, for the IoU the part through the overlap and the part through the
  predicted box's volume (they cancel exactly for identical boxes).  On the centre / size columns the IoU
  terms meet the SmoothL1 term of the same column.
"""
import numpy as np
import torch

F64 = torch.float64
HYPER_NAMES = ("cw0", "cw1", "w_obj", "w_dircls", "w_dirres", "w_size", "w_center", "w_sem", "w_iou",
               "beta_dirres", "beta_size", "beta_center")
NBINS, NSEM = 12, 10


def _f64(t):
    return torch.as_tensor(t).detach().cpu().to(F64)


def _i64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.int64)


def error_units(got, ref, scale):
    """max over elements of |got - ref| / (2^-24 * scale); an element whose scale is 0 must match exactly
    (0 units if it does, inf if not)."""
    got, ref, scale = _f64(got).reshape(-1), _f64(ref).reshape(-1), _f64(scale).reshape(-1)
    err = (got - ref).abs()
    units = torch.where(scale > 0, err / (2.0 ** -24 * scale.clamp(min=1e-300)),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(units.max()) if units.numel() else 0.0


def hyper_dict(hyper12):
    """The twelve hyper-parameters as the kernel receives them: rounded to fp32."""
    assert len(hyper12) == 12
    return {n: float(np.float32(v)) for n, v in zip(HYPER_NAMES, hyper12)}


def _ce_rows(logits, target):
    """Per-row log-softmax cross entropy and the softmax: (n,), (n, K)."""
    m = logits.max(dim=1, keepdim=True).values.detach()
    lse = m.squeeze(1) + torch.log(torch.exp(logits - m).sum(1))
    return lse - logits.gather(1, target.view(-1, 1)).squeeze(1), torch.exp(logits - lse.unsqueeze(1))


def _smooth_l1(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta)


def _iou_parts(cen, siz, cen_t, siz_t):
    """Axis-aligned IoU of the boxes centre +- size/2 -> (iou, overlap, a1).  Signed a1 (a negative predicted
    size gives a negative volume), extent clamped at 0 (clamp passes the gradient AT 0), union floored at 1e-6,
    binary torch.max / torch.min (their backward gives 0.5 / 0.5 on a tie)."""
    lo1, hi1 = cen - siz / 2, cen + siz / 2
    lo2, hi2 = cen_t - siz_t / 2, cen_t + siz_t / 2
    e1, e2 = hi1 - lo1, hi2 - lo2
    a1 = e1[:, 0] * e1[:, 1] * e1[:, 2]
    a2 = e2[:, 0] * e2[:, 1] * e2[:, 2]
    ext = (torch.min(hi1, hi2) - torch.max(lo1, lo2)).clamp(min=0)
    ov = ext[:, 0] * ext[:, 1] * ext[:, 2]
    union = (a1 + a2 - ov).clamp(min=1e-6)
    return ov / union, ov, a1


def head_loss_ref(cls, reg, base, hyper12, center_t, size_t, dir_class_t, dir_res_t, sem_t, obj_t, obj_w,
                  box_w, gout=None):
    """-> (sums (7,), A (7,), (gcls, greg, gbase) | None, (Tcls, Treg, Tbase) | None), all float64, in
    ops.HEAD_LOSS_NAMES order; the gradients are those of ``(gout * sums).sum()``."""
    h = hyper_dict(hyper12)
    cls, reg, base = (_f64(t).clone().requires_grad_() for t in (cls, reg, base))
    center_t, size_t, dir_res_t, obj_w, box_w = map(_f64, (center_t, size_t, dir_res_t, obj_w, box_w))
    dt, st, ot = _i64(dir_class_t), _i64(sem_t), _i64(obj_t)
    R = cls.shape[0]
    assert cls.shape == (R, 2 + NSEM) and reg.shape == (R, 6 + 2 * NBINS) and base.shape == (R, 3)
    cen, siz = base + reg[:, 0:3], reg[:, 3:6]
    cw = torch.where(ot != 0, torch.full((R,), h["cw1"], dtype=F64), torch.full((R,), h["cw0"], dtype=F64))
    ce_obj, p_obj = _ce_rows(cls[:, 0:2], ot)
    ce_dir, p_dir = _ce_rows(reg[:, 6:6 + NBINS], dt)
    ce_sem, p_sem = _ce_rows(cls[:, 2:2 + NSEM], st)
    res = reg[:, 6 + NBINS:].gather(1, dt.view(-1, 1)).squeeze(1)
    iou, ov, a1 = _iou_parts(cen, siz, center_t, size_t)
    w_obj_row = h["w_obj"] * obj_w * cw
    rows = [w_obj_row * ce_obj,
            h["w_dircls"] * box_w * ce_dir,
            h["w_dirres"] * box_w * _smooth_l1(res - dir_res_t, h["beta_dirres"]),
            h["w_size"] * box_w * _smooth_l1(siz - size_t, h["beta_size"]).sum(1),
            h["w_center"] * box_w * _smooth_l1(cen - center_t, h["beta_center"]).sum(1),
            h["w_sem"] * box_w * ce_sem,
            h["w_iou"] * box_w * (1 - iou)]
    sums = torch.stack([r.sum() for r in rows])
    A = torch.stack([r.detach().abs().sum() for r in rows])
    if gout is None:
        return sums.detach(), A, None, None
    g = _f64(gout)
    leaves = (cls, reg, base)

    def grads(out, seed=None):
        gs = torch.autograd.grad(out, leaves, grad_outputs=seed, retain_graph=True, allow_unused=True)
        return [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, gs)]

    total = grads((g * sums).sum())
    T = [torch.zeros_like(l) for l in leaves]
    for i in (2, 3, 4):                                   # SmoothL1 terms: one additive term per element
        for t, x in zip(T, grads(g[i] * sums[i])):
            t += x.abs()
    # cross entropies: |upstream * row weight| * (softmax + one-hot)
    oh = lambda t, k: torch.nn.functional.one_hot(t, k).to(F64)
    T[0][:, 0:2] += (g[0] * w_obj_row).abs().unsqueeze(1) * (p_obj.detach() + oh(ot, 2))
    T[1][:, 6:6 + NBINS] += (g[1] * h["w_dircls"] * box_w).abs().unsqueeze(1) * (p_dir.detach() + oh(dt, NBINS))
    T[0][:, 2:2 + NSEM] += (g[5] * h["w_sem"] * box_w).abs().unsqueeze(1) * (p_sem.detach() + oh(st, NSEM))
    # IoU: the path through the overlap and the path through the predicted volume, separately
    d_ov, d_a1 = torch.autograd.grad(g[6] * sums[6], (ov, a1), retain_graph=True)
    via = [grads(ov, d_ov), grads(a1, d_a1)]
    for part in via:
        for t, x in zip(T, part):
            t += x.abs()
    direct = grads(g[6] * sums[6])
    for a, b, c in zip(direct, via[0], via[1]):           # the two paths ARE the IoU gradient
        assert bool(((a - (b + c)).abs() <= 1e-12 * (b.abs() + c.abs())).all())
    return sums.detach(), A, tuple(total), tuple(T)


def vote_loss_ref(vote, seed, seed_idx, masks, vote_targets, gt_per_seed, dst_weight, gout=1.0):
    """VoteModule.get_loss with one vote per seed: sum over seeds of min_j L1(vote - (target_j + seed)) *
    mask / (count + 1e-6) * dst_weight.  -> (value, count (int), grad wrt vote * gout, |contribution| (B, S))."""
    vote = _f64(vote).clone().requires_grad_()
    seed, vt = _f64(seed), _f64(vote_targets)
    idx, masks = _i64(seed_idx), _i64(masks)
    B, S = idx.shape
    m = torch.stack([masks[b][idx[b]] for b in range(B)])                       # (B, S)
    count = int(m.sum())
    tgt = torch.stack([vt[b][idx[b]] for b in range(B)]).view(B, S, gt_per_seed, 3) + seed.unsqueeze(2)
    w = m.to(F64) / (count + 1e-6) * float(dst_weight)
    d = (vote.unsqueeze(2) - tgt).abs().sum(-1) * w.unsqueeze(-1)               # (B, S, G)
    contrib = d.min(dim=2).values
    value = contrib.sum()
    (gv,) = torch.autograd.grad(value * float(gout), vote)
    return value.detach(), count, gv, contrib.detach().abs()


def loss_total_np(vecs, vote=None):
    """loss_total_k in fp32 numpy, in the kernel's stated order: per column the Python-sum order over the
    vectors, one division by n, then the sequential 7-element sum, then the vote loss."""
    vecs = [np.asarray(v, np.float32) for v in vecs]
    n = np.float32(len(vecs))
    out = np.zeros(8, np.float32)
    tot = np.float32(0)
    for i in range(7):
        m = vecs[0][i]
        for v in vecs[1:]:
            m = np.float32(m + v[i])
        m = np.float32(m / n)
        out[i] = m
        tot = m if i == 0 else np.float32(tot + m)
    out[7] = np.float32(tot + (np.float32(vote) if vote is not None else np.float32(0)))
    return out


def loss_total_bwd_np(g8, n, with_vote):
    """-> (gvecs (n, 7) fp32: (g8[t] + g8[7]) / n in every row, gvote (fp32 scalar) | None)."""
    g8 = np.asarray(g8, np.float32)
    row = ((g8[:7] + g8[7]).astype(np.float32) / np.float32(n)).astype(np.float32)
    return np.tile(row, (n, 1)), (g8[7] if with_vote else None)


def query_pos_rows_np(reg_rows, base_xyz):
    """(B, Q, nreg), (B, Q, 3) fp32 -> (B*Q, 8) fp32: [base + reg[:3] | reg[3:6] | 0 0]."""
    reg = np.asarray(reg_rows, np.float32).reshape(-1, reg_rows.shape[-1])
    base = np.asarray(base_xyz, np.float32).reshape(-1, 3)
    out = np.zeros((reg.shape[0], 8), np.float32)
    out[:, 0:3] = base + reg[:, 0:3]
    out[:, 3:6] = reg[:, 3:6]
    return out
