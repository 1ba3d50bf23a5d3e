"""fp64 restatement of the test side of Deformable DETR's decoder and head, written from the published algorithm
(mmdet DeformableDetrTransformerDecoder / DeformableDETRHead / _get_bboxes_single, mmcv MultiScaleDeformableAttention
and nn.MultiheadAttention; configs/deformdetr/imvotenet_image.py:21-80) - NOT from demf_amd.modules.  Everything reads
a state dict under the stage-1 checkpoint's key names.  mmdet / mmcv themselves are not available, so parity with
upstream binaries is not pinned by this file; it pins the formulas.

Plain torch / numpy, float64 throughout.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

HEAD = "img_bbox_head."
DEC = HEAD + "transformer.decoder.layers.%d."


def f64(sd):
    return {k: v.detach().double().cpu() for k, v in sd.items()}


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def attention(qkv, B, H):
    """qkv (B*Q, 3*H*Dh) packed [q | k | v] rows -> (B*Q, H*Dh): softmax(q k^T / sqrt(Dh)) v per (image, head)."""
    qkv = qkv.double()
    R, E3 = qkv.shape
    Q, E = R // B, E3 // 3
    Dh = E // H
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, Q, H, Dh).permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(Dh), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(R, E)


def msda(value, shapes, loc, w):
    """mmcv multi_scale_deformable_attn_pytorch: value (B,S,H,Dh), shapes [(h,w)], loc (B,Q,H,L,P,2) in [0,1] (x, y),
    w (B,Q,H,L,P) -> (B,Q,H*Dh).  Bilinear, zero padding, align_corners=False."""
    B, S, H, Dh = value.shape
    _, Q, _, L, P, _ = loc.shape
    grids = 2 * loc - 1
    out, start = [], 0
    for l, (h, ww) in enumerate(shapes):
        v = value[:, start:start + h * ww].permute(0, 2, 3, 1).reshape(B * H, Dh, h, ww)
        start += h * ww
        g = grids[:, :, :, l].permute(0, 2, 1, 3, 4).reshape(B * H, Q, P, 2)
        out.append(F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False))   # (BH,Dh,Q,P)
    samp = torch.stack(out, -2).flatten(-2)                                                          # (BH,Dh,Q,L*P)
    aw = w.permute(0, 2, 1, 3, 4).reshape(B * H, 1, Q, L * P)
    return (samp * aw).sum(-1).view(B, H, Dh, Q).permute(0, 3, 1, 2).reshape(B, Q, H * Dh)


def msda_function(value, shapes_t, lsi, loc, w, im2col_step=64):
    """The argument list of ops.MultiScaleDeformableAttnFunction.apply (a CPU stand-in for the module path)."""
    return msda(value, [tuple(int(v) for v in s) for s in shapes_t.tolist()], loc, w)


def decoder_layer(sd, li, x, pos, memory, mask, ref_in, shapes, H, L, P):
    """One DetrTransformerDecoderLayer (self_attn, norm, cross_attn, norm, ffn, norm) in eval mode, batch-major:
    x / pos (B,Q,E), memory (B,S,E), mask (B,S) True = padding, ref_in (B,Q,L,2)."""
    g = lambda name: sd[(DEC % li) + name]
    B, Q, E = x.shape
    # self-attention: q = k = x + pos, v = x (nn.MultiheadAttention with a packed in_proj)
    wi, bi = g("attentions.0.attn.in_proj_weight"), g("attentions.0.attn.in_proj_bias")
    qk = (x + pos) @ wi[:2 * E].T + bi[:2 * E]
    v = x @ wi[2 * E:].T + bi[2 * E:]
    o = attention(torch.cat([qk, v], -1).reshape(B * Q, 3 * E), B, H).view(B, Q, E)
    o = o @ g("attentions.0.attn.out_proj.weight").T + g("attentions.0.attn.out_proj.bias")
    x = layer_norm(x + o, g("norms.0.weight"), g("norms.0.bias"))
    # deformable cross-attention over the memory
    qp = x + pos
    val = memory @ g("attentions.1.value_proj.weight").T + g("attentions.1.value_proj.bias")
    val = val.masked_fill(mask[..., None], 0.0).view(B, -1, H, E // H)
    off = (qp @ g("attentions.1.sampling_offsets.weight").T + g("attentions.1.sampling_offsets.bias")) \
        .view(B, Q, H, L, P, 2)
    aw = (qp @ g("attentions.1.attention_weights.weight").T + g("attentions.1.attention_weights.bias")) \
        .view(B, Q, H, L * P).softmax(-1).view(B, Q, H, L, P)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)           # (L,2) = (W_l, H_l)
    loc = ref_in[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    o = msda(val, shapes, loc, aw)
    o = o @ g("attentions.1.output_proj.weight").T + g("attentions.1.output_proj.bias")
    x = layer_norm(x + o, g("norms.1.weight"), g("norms.1.bias"))
    # FFN
    hdn = torch.relu(x @ g("ffns.0.layers.0.0.weight").T + g("ffns.0.layers.0.0.bias"))
    o = hdn @ g("ffns.0.layers.1.weight").T + g("ffns.0.layers.1.bias")
    return layer_norm(x + o, g("norms.2.weight"), g("norms.2.bias"))


def reference_points(sd, E):
    qe = sd[HEAD + "query_embedding.weight"]
    return torch.sigmoid(qe[:, :E] @ sd[HEAD + "transformer.reference_points.weight"].T
                         + sd[HEAD + "transformer.reference_points.bias"])


def decoder(sd, memory, mask, valid_ratios, shapes, num_layers, H=8, L=4, P=4):
    """-> (hs of every layer [(B,Q,E)], reference points (Q,2))."""
    sd = f64(sd) if next(iter(sd.values())).dtype != torch.float64 else sd
    memory, valid_ratios = memory.double().cpu(), valid_ratios.double().cpu()
    mask = mask.cpu()
    B, _, E = memory.shape
    qe = sd[HEAD + "query_embedding.weight"]
    pos, x = qe[:, :E].expand(B, -1, -1), qe[:, E:].expand(B, -1, -1)
    ref = reference_points(sd, E)
    ref_in = ref[None, :, None, :] * valid_ratios[:, None]
    hs = []
    for li in range(num_layers):
        x = decoder_layer(sd, li, x, pos, memory, mask, ref_in, shapes, H, L, P)
        hs.append(x)
    return hs, ref


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def head_tail(hs, hidden, w_cls, b_cls, w_reg, b_reg, ref):
    """hs / hidden (R,K) rows, ref (R,2) -> logits (R,C), boxes (R,4) normalised cxcywh."""
    hs, hidden, ref = hs.double(), hidden.double(), ref.double()
    logits = hs @ w_cls.double().T + b_cls.double()
    tmp = hidden @ w_reg.double().T + b_reg.double()
    tmp = torch.cat([tmp[:, :2] + inverse_sigmoid(ref), tmp[:, 2:]], 1)
    return logits, torch.sigmoid(tmp)


def branches(sd, hs_last, ref, lvl):
    """The prediction level's class and box branches on hs_last (B,Q,E) -> logits (B,Q,C), boxes (B,Q,4)."""
    sd = f64(sd) if next(iter(sd.values())).dtype != torch.float64 else sd
    B, Q, E = hs_last.shape
    x = hs_last.double().cpu().reshape(B * Q, E)
    r = lambda i: (sd[HEAD + "reg_branches.%d.%d.weight" % (lvl, i)], sd[HEAD + "reg_branches.%d.%d.bias" % (lvl, i)])
    h = torch.relu(x @ r(0)[0].T + r(0)[1])
    h = torch.relu(h @ r(2)[0].T + r(2)[1])
    logits, boxes = head_tail(x, h, sd[HEAD + "cls_branches.%d.weight" % lvl], sd[HEAD + "cls_branches.%d.bias" % lvl],
                              r(4)[0], r(4)[1], ref.double().cpu().repeat(B, 1))
    return logits.view(B, Q, -1), boxes.view(B, Q, 4)


def select(logits, boxes, meta, k, thr, rescale):
    """Per image: a stable sort on (-logit, flat index), the first min(k, Q*C) places, label = idx % C, query =
    idx // C, cxcywh -> xyxy, x * w, y * h, clamp, optional / scale_factor, score = sigmoid(logit), rows kept while
    score > thr (thr < 0: all).  logits (B,Q,C) and boxes (B,Q,4) of any float dtype (the ORDER is taken on the values
    as given, the arithmetic is fp64), meta (B,6) = [h, w, sf x4].
    -> list over images of dict(idx (kk,), rows (n,6) fp64, n, logit (kk,) the ordered logits as given)."""
    B, Q, C = logits.shape
    lg = logits.detach().cpu().numpy().reshape(B, Q * C)
    bx = boxes.detach().double().cpu().numpy()
    mt = meta.detach().double().cpu().numpy()
    out = []
    for b in range(B):
        v = lg[b]
        nan = np.isnan(v)
        order = np.lexsort((np.arange(v.size), np.where(nan, 0.0, -v.astype(np.float64)), nan))   # NaN after every number
        idx = order[:min(int(k), v.size)]
        score = 1.0 / (1.0 + np.exp(-v[idx].astype(np.float64)))
        q, c = idx // C, idx % C
        cx, cy, w, h = (bx[b, q, i] for i in range(4))
        ih, iw = mt[b, 0], mt[b, 1]
        xy = np.stack([np.clip((cx - 0.5 * w) * iw, 0, iw), np.clip((cy - 0.5 * h) * ih, 0, ih),
                       np.clip((cx + 0.5 * w) * iw, 0, iw), np.clip((cy + 0.5 * h) * ih, 0, ih)], 1)
        if rescale:
            xy = xy / mt[b, 2:6]
        keep = np.ones_like(score, dtype=bool) if thr < 0 else score > thr
        n = int(keep.sum())
        assert keep[:n].all(), "the threshold keeps a prefix of the order"
        rows = np.concatenate([xy, score[:, None], c[:, None].astype(np.float64)], 1)[:n]
        out.append(dict(idx=idx, rows=rows, n=n, logit=v[idx]))
    return out


THR_LOGIT = math.log(0.09 / 0.91)


def well_separated(logits, k, thr, margin=1e-3):
    """The conditions under which fp32 rounding cannot change what ``select`` returns: no logit within ``margin`` of
    the threshold's logit, and the k-th and (k+1)-th ordered logits either bit-equal or ``margin`` apart."""
    B = logits.shape[0]
    lg = logits.detach().double().cpu().reshape(B, -1)
    if thr >= 0 and bool(((lg - math.log(thr / (1 - thr))).abs() < margin).any()):
        return False
    if lg.shape[1] > k:
        s = torch.sort(lg, 1, descending=True)[0]
        gap = s[:, k - 1] - s[:, k]
        if bool(((gap != 0) & (gap < margin)).any()):
            return False
    return True
