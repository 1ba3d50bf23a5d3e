"""The image branch's 2D detector, test side: Deformable DETR as the reference trains it in stage 1.

``Detr2D`` is the ``ImVoteNet_Deformdetr`` of the image-only config (configs/deformdetr/imvotenet_image.py:1-80;
demf/modeling/detectors/imvotenet_deform.py): ResNet-50 -> ChannelMapper -> ``DeformableDETRHead`` (encoder, 300
learned queries through a 6-layer decoder, class and box branches) -> per-image top-100 boxes.  The mmdet / mmcv
classes are restated from their published algorithm with upstream's module names and state-dict keys, so a stage-1
checkpoint loads with ``strict=True``; parity with upstream BINARIES is not pinned (mmdet is not a dependency and
was not run against).

What DeMF keeps of that model - backbone, neck, encoder, level embeds - is the ``ImageStream`` this package already
has; the head uses that encoder (``DeformableDetrEncoder.forward_tokens``) rather than a copy, and the loader routes
``img_bbox_head.transformer.encoder.* / level_embeds`` to it.

Two paths compute the decoder and the head:

  * the MODULE path - ``DeformableDetrTransformerDecoder.forward`` over ``transformer.DetrTransformerDecoderLayer``
    - for any configuration, on ``ops.linear``; in eval mode on the device its self-attention runs on
    demf_attn_fwd_eval (``MultiheadAttention._attend``);
  * the KERNEL path (eval mode, device, the reference's layer shape: embed 256, 8 heads, 4 levels, P in {2, 4},
    post-norm order, 2-fc ReLU FFN): every projection on demf_rows_gemm_f32 with weights packed once per weight
    version, self-attention on demf_attn_fwd_eval, cross-attention on demf_msda_fwd_raw_f32, LayerNorm tails in the
    GEMM epilogues, branches' tail on demf_detr2d_head, top-k / decode / threshold on demf_detr2d_select.  What
    depends on the weights only - the reference points and layer 0's self-attention block, whose query is the
    learned embedding - is computed once per weight version.

Out of scope (follow-ups): stage-1 TRAINING (Hungarian matching, focal / L1 / GIoU losses, a backward through the
backbone), a 2D mAP, and the ImVoteNet fusion that consumes ``extract_bboxes_2d``.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops, switches
from .image_stream import ImageStream
from .transformer import FFN, DetrTransformerDecoderLayer, MultiheadAttention, MultiScaleDeformableAttention

# the decoder + head on the row-GEMM / attention / selection kernels; False / DEMF_DETR2D_FUSED=0: the module path
FUSED = bool(switches.env_int("DEMF_DETR2D_FUSED"))
# the six layers' value projections of the memory tokens as ONE launch (N = 6 * 256, one read of the tokens: 2.43 ms
# against 2.61 ms per batch at the reference size); 0: one launch per layer, which needs a sixth
# of the scratch (152 MB instead of 915 MB at B = 8)
VALUE_ONE_LAUNCH = bool(switches.env_int("DEMF_DETR2D_VALUE_ONE"))

SCORE_THR = 0.09            # ImVoteNet.filter (imvotenet_deform.py:181)


def inverse_sigmoid(x, eps=1e-5):
    """mmdet.models.utils.transformer.inverse_sigmoid."""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


class DeformableDetrTransformerDecoder(nn.Module):
    """mmdet DeformableDetrTransformerDecoder (imvotenet_image.py:40-59) without box refinement: ``num_layers`` x
    DetrTransformerDecoderLayer (self_attn, norm, cross_attn, norm, ffn, norm), the same
    ``reference_points[:, :, None] * valid_ratios[:, None]`` for every layer."""

    def __init__(self, num_layers=6, embed_dims=256, num_heads=8, num_levels=4, num_points=4, attn_dropout=0.1,
                 feedforward_channels=1024, ffn_dropout=0.1, return_intermediate=True):
        super().__init__()
        self.layers = nn.ModuleList([
            DetrTransformerDecoderLayer(embed_dims, num_heads, num_levels, num_points, attn_dropout,
                                        feedforward_channels, ffn_dropout) for _ in range(num_layers)])
        self.embed_dims, self.return_intermediate = embed_dims, return_intermediate

    def forward(self, query, value, query_pos=None, key_padding_mask=None, reference_points=None,
                spatial_shapes=None, level_start_index=None, valid_ratios=None):
        """query / query_pos (Q,B,C), value (S,B,C) the encoder memory, key_padding_mask (B,S), reference_points
        (B,Q,2) in [0,1], valid_ratios (B,L,2) -> (num_layers,Q,B,C) (``return_intermediate``) or (Q,B,C)."""
        assert reference_points.shape[-1] == 2, "box refinement / two-stage (4-d reference points) is not built"
        ref_in = reference_points[:, :, None] * valid_ratios[:, None]
        out, inter = query, []
        for layer in self.layers:
            out = layer(out, None, value, query_pos=query_pos, key_padding_mask=key_padding_mask,
                        reference_points=ref_in, spatial_shapes=spatial_shapes, level_start_index=level_start_index)
            if self.return_intermediate:
                inter.append(out)
        return torch.stack(inter) if self.return_intermediate else out


class _Transformer(nn.Module):
    """The parameter holder under upstream's ``img_bbox_head.transformer``: ``reference_points`` and ``decoder``
    (the encoder and ``level_embeds`` live in the detector's ``DeformableDetrEncoder``)."""

    def __init__(self, embed_dims, **decoder):
        super().__init__()
        self.decoder = DeformableDetrTransformerDecoder(embed_dims=embed_dims, **decoder)
        self.reference_points = nn.Linear(embed_dims, 2)


class DeformableDETRHead(nn.Module):
    """mmdet DeformableDETRHead (imvotenet_image.py:21-72; as_two_stage=False, with_box_refine=False), test side.
    ``cls_branches`` / ``reg_branches`` hold ONE module ``num_layers`` times, as upstream: the state dict carries all
    the ``.0`` .. ``.5`` keys and they are equal after a load."""

    def __init__(self, num_query=300, num_classes=10, embed_dims=256, num_layers=6, num_heads=8, num_levels=4,
                 num_points=4, feedforward_channels=1024, attn_dropout=0.1, ffn_dropout=0.1, max_per_img=100):
        super().__init__()
        self.num_query, self.num_classes, self.embed_dims = num_query, num_classes, embed_dims
        self.max_per_img = max_per_img
        self.query_embedding = nn.Embedding(num_query, 2 * embed_dims)
        self.transformer = _Transformer(embed_dims, num_layers=num_layers, num_heads=num_heads, num_levels=num_levels,
                                        num_points=num_points, attn_dropout=attn_dropout,
                                        feedforward_channels=feedforward_channels, ffn_dropout=ffn_dropout)
        fc_cls = nn.Linear(embed_dims, num_classes)
        reg_branch = nn.Sequential(nn.Linear(embed_dims, embed_dims), nn.ReLU(), nn.Linear(embed_dims, embed_dims),
                                   nn.ReLU(), nn.Linear(embed_dims, 4))
        self.cls_branches = nn.ModuleList([fc_cls for _ in range(num_layers)])
        self.reg_branches = nn.ModuleList([reg_branch for _ in range(num_layers)])
        self.init_weights()

    def init_weights(self):
        """DeformableDetrTransformer.init_weights + DeformableDETRHead.init_weights (focal-loss class bias, zero last
        box layer)."""
        for p in self.transformer.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.transformer.modules():
            if isinstance(m, MultiScaleDeformableAttention):
                m.init_weights()
        nn.init.xavier_uniform_(self.transformer.reference_points.weight)
        nn.init.constant_(self.transformer.reference_points.bias, 0.0)
        nn.init.constant_(self.cls_branches[0].bias, float(-np.log((1 - 0.01) / 0.01)))
        nn.init.constant_(self.reg_branches[0][-1].weight, 0.0)
        nn.init.constant_(self.reg_branches[0][-1].bias, 0.0)

    # ---- module path ------------------------------------------------------------------------------------------
    @staticmethod
    def _linear(x, m):
        return ops.linear(x, m.weight, m.bias) if x.is_cuda else F.linear(x, m.weight, m.bias)

    def reference(self):
        """(Q,2): sigmoid(Linear(query_pos)) - the same for every image."""
        C = self.embed_dims
        return self._linear(self.query_embedding.weight[:, :C], self.transformer.reference_points).sigmoid()

    def decode(self, memory, mask_flatten, valid_ratios, spatial_shapes, level_start_index):
        """DeformableDetrTransformer.forward behind the encoder: memory (B,S,C) -> hs (num_layers,B,Q,C) (one layer
        when the decoder does not return intermediates) and the reference points (Q,2)."""
        B, C = memory.shape[0], self.embed_dims
        qe = self.query_embedding.weight
        query_pos = qe[:, :C].unsqueeze(1).expand(-1, B, -1)
        query = qe[:, C:].unsqueeze(1).expand(-1, B, -1)
        ref = self.reference()
        hs = self.transformer.decoder(query, memory.permute(1, 0, 2), query_pos=query_pos,
                                      key_padding_mask=mask_flatten,
                                      reference_points=ref.unsqueeze(0).expand(B, -1, -1),
                                      spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                                      valid_ratios=valid_ratios)
        if hs.dim() == 3:
            hs = hs.unsqueeze(0)
        return hs.permute(0, 2, 1, 3), ref

    def branches(self, hs_last, ref):
        """The last prediction level's branches: hs_last (B,Q,C), ref (Q,2) -> logits (B,Q,num_classes), boxes (B,Q,4)
        normalised (cx, cy, w, h)."""
        lvl = len(self.cls_branches) - 1
        logits = self._linear(hs_last, self.cls_branches[lvl])
        reg = self.reg_branches[lvl]
        tmp = self._linear(F.relu(self._linear(F.relu(self._linear(hs_last, reg[0])), reg[2])), reg[4])
        tmp = torch.cat([tmp[..., :2] + inverse_sigmoid(ref), tmp[..., 2:]], -1)
        return logits, tmp.sigmoid()

    def forward_module(self, enc, st):
        """enc: ``DeformableDetrEncoder.forward_tokens``' dict, st: its ``_static`` -> (hs_last, logits, boxes)."""
        hs, ref = self.decode(enc["tokens"], enc["mask_flatten"], enc["valid_ratios"], st["spatial_shapes"],
                              st["level_start_index"])
        logits, boxes = self.branches(hs[-1], ref)
        return hs[-1], logits, boxes

    # ---- kernel path ------------------------------------------------------------------------------------------
    def fused_ok(self, tokens):
        """The kernel path hard-codes the reference's decoder layer (imvotenet_image.py:40-59): embed 256, 8 heads of
        32 channels, 4 levels, 2 or 4 points, post-norm order, a 2-fc ReLU FFN, LayerNorm(256), eval mode, and the
        limits of the three kernels of csrc/detr2d.hip.  Anything else takes the module path."""
        if not (FUSED and tokens.is_cuda and tokens.dtype == torch.float32 and self.embed_dims == 256
                and not self.training and 1 <= self.num_query <= ops.ATTN_EVAL_MAX_Q
                and self.num_classes <= ops.DETR2D_MAX_CLASSES and tokens.shape[1] * 1536 < 2 ** 31):
            return False
        for layer in self.transformer.decoder.layers:
            if not (type(layer) is DetrTransformerDecoderLayer and not layer.training):
                return False
            mha, a, f = layer.attentions[0], layer.attentions[1], layer.ffns[0]
            if not (type(mha) is MultiheadAttention and mha.attn.num_heads == 8 and mha.attn.embed_dim == 256
                    and mha.attn.in_proj_weight is not None and mha.attn.in_proj_bias is not None):
                return False
            if not (type(a) is MultiScaleDeformableAttention and a.num_heads == 8 and a.num_levels == 4
                    and a.num_points in (2, 4) and a.embed_dims == 256 and not a.batch_first):
                return False
            if not (type(f) is FFN and len(f.layers) == 3 and isinstance(f.layers[0][0], nn.Linear)
                    and isinstance(f.layers[0][1], nn.ReLU) and isinstance(f.layers[1], nn.Linear)
                    and f.layers[0][0].out_features % 128 == 0 and f.layers[1].out_features == 256):
                return False
            if not all(isinstance(n, nn.LayerNorm) and tuple(n.normalized_shape) == (256,) for n in layer.norms):
                return False
        return True

    def _pack(self, planes):
        """Every weight as the kernels take it, split into ``planes`` bf16 planes (ops.split_planes), and the two
        weight-only results: the reference points (Q,2) and layer 0's self-attention block LN(query + attn(query))
        (Q,256).  Cached per (weight versions, planes): a load_state_dict rebuilds it."""
        prm = list(self.parameters())
        key = (planes,) + tuple((q.data_ptr(), q._version) for q in prm)
        pk = self.__dict__.get("_pack_cache")
        if pk is not None and pk["key"] == key:
            return pk
        c = lambda t: t.detach().float().contiguous()
        sp = lambda t: ops.split_planes(c(t), planes)
        layers = []
        for layer in self.transformer.decoder.layers:
            mha, a, f, n = layer.attentions[0].attn, layer.attentions[1], layer.ffns[0], layer.norms
            fc0, fc1 = f.layers[0][0], f.layers[1]
            layers.append(dict(
                w_qkv=sp(mha.in_proj_weight), b_qkv=c(mha.in_proj_bias),
                w_ao=sp(mha.out_proj.weight), b_ao=c(mha.out_proj.bias),
                w_x=sp(torch.cat([c(a.sampling_offsets.weight), c(a.attention_weights.weight)], 0)),
                b_x=torch.cat([c(a.sampling_offsets.bias), c(a.attention_weights.bias)], 0),
                lgt0=a.sampling_offsets.out_features, P=a.num_points,
                w_v=sp(a.value_proj.weight), b_v=c(a.value_proj.bias),
                w_co=sp(a.output_proj.weight), b_co=c(a.output_proj.bias),
                w0=sp(fc0.weight), b0=c(fc0.bias), w1=sp(fc1.weight), b1=c(fc1.bias),
                ln=[(c(m.weight), c(m.bias), float(m.eps)) for m in n]))
        lvl = len(self.cls_branches) - 1
        reg, cls = self.reg_branches[lvl], self.cls_branches[lvl]
        pk = dict(key=key, layers=layers,
                  w_vall=ops.split_planes(torch.cat([c(l.attentions[1].value_proj.weight)
                                                     for l in self.transformer.decoder.layers], 0), planes),
                  b_vall=torch.cat([c(l.attentions[1].value_proj.bias) for l in self.transformer.decoder.layers], 0),
                  w_r0=sp(reg[0].weight), b_r0=c(reg[0].bias), w_r1=sp(reg[2].weight), b_r1=c(reg[2].bias),
                  w_r2=c(reg[4].weight), b_r2=c(reg[4].bias), w_c=c(cls.weight), b_c=c(cls.bias), tiled={})
        C = self.embed_dims
        qe = c(self.query_embedding.weight)
        pk["pos"], pk["query"] = qe[:, :C].contiguous(), qe[:, C:].contiguous()
        with torch.no_grad():
            pk["ref"] = self.reference().float().contiguous()
            pk["x1_0"] = self._self_attention(pk["query"], pk["pos"], layers[0], 1)
        self.__dict__["_pack_cache"] = pk
        return pk

    @staticmethod
    def _self_attention(x, pos, lp, B):
        """Rows x (B*Q,256) -> LN(x + out_proj(attention([x + pos | x + pos | x]))): three launches."""
        R = x.shape[0]
        new = lambda n: torch.empty((R, n), dtype=torch.float32, device=x.device)
        qkv = ops.rows_gemm(x, lp["w_qkv"], lp["b_qkv"], new(768), a2=pos, a2_cols=512)
        o = ops.attn_eval(qkv, B, 8)
        g, b, eps = lp["ln"][0]
        return ops.rows_gemm(o, lp["w_ao"], lp["b_ao"], new(256), ln=(x, g, b, eps))

    def forward_kernels(self, enc, st):
        """The decoder and the branches on this package's kernels -> (hs_last (B,Q,256), logits (B,Q,C), boxes
        (B,Q,4)).  Per batch: 1 launch for the layers' value projections (or one per layer), 5 for layer 0, 8 for
        every later layer, 3 for the branches (+ two small elementwise ones for the reference points x valid
        ratios)."""
        from .. import _ffi
        tokens = enc["tokens"]
        B, S, C = tokens.shape
        Q = self.num_query
        R = B * Q
        planes = 1 if ops.get_compute_dtype() == "bf16" else 3
        pk = self._pack(planes)
        if B not in pk["tiled"]:
            if len(pk["tiled"]) > 4:
                pk["tiled"].clear()
            pk["tiled"][B] = (pk["pos"].repeat(B, 1), pk["x1_0"].repeat(B, 1))
        pos, x1 = pk["tiled"][B]
        tok = tokens.reshape(B * S, C)
        mask = enc["mask_flatten"].reshape(B * S).contiguous()
        ref_in = (pk["ref"][None, :, None, :] * enc["valid_ratios"][:, None].float()).contiguous()    # (B,Q,L,2)
        new = lambda n, r=R: torch.empty((r, n), dtype=torch.float32, device=tokens.device)
        stream = torch.cuda.current_stream().cuda_stream
        nl = len(pk["layers"])
        vall = None
        if VALUE_ONE_LAUNCH:
            vall = ops.rows_gemm(tok, pk["w_vall"], pk["b_vall"], new(256 * nl, B * S), row_mask=mask, mask_col0=0)
        val = None if VALUE_ONE_LAUNCH else new(256, B * S)
        raw, samp, hid = new(384), new(256), None
        x = None
        for li, lp in enumerate(pk["layers"]):
            if li > 0:
                x1 = self._self_attention(x, pos, lp, B)
            n_x = lp["w_x"].shape[1]
            if raw.shape[1] != n_x:
                raw = new(n_x)
            ops.rows_gemm(x1, lp["w_x"], lp["b_x"], raw, a2=pos, a2_cols=n_x)
            if vall is None:
                ops.rows_gemm(tok, lp["w_v"], lp["b_v"], val, row_mask=mask, mask_col0=0)
                vptr, vpitch = val.data_ptr(), 256
            else:
                vptr, vpitch = vall.data_ptr() + 4 * 256 * li, 256 * nl
            _ffi.call("demf_msda_fwd_raw_f32", B, S, 8, 32, 4, Q, lp["P"], vptr, vpitch, st["spatial_shapes"].data_ptr(),
                      st["level_start_index"].data_ptr(), raw.data_ptr(), raw.stride(0), 0, lp["lgt0"],
                      ref_in.data_ptr(), samp.data_ptr(), stream)
            g, b, eps = lp["ln"][1]
            x2 = ops.rows_gemm(samp, lp["w_co"], lp["b_co"], new(256), ln=(x1, g, b, eps))
            if hid is None or hid.shape[1] != lp["w0"].shape[1]:
                hid = new(lp["w0"].shape[1])
            ops.rows_gemm(x2, lp["w0"], lp["b0"], hid, relu=True)
            g, b, eps = lp["ln"][2]
            x = ops.rows_gemm(hid, lp["w1"], lp["b1"], new(256), ln=(x2, g, b, eps))
        h = ops.rows_gemm(x, pk["w_r0"], pk["b_r0"], new(256), relu=True)
        h = ops.rows_gemm(h, pk["w_r1"], pk["b_r1"], new(256), relu=True)
        logits, boxes = ops.detr2d_head(x, h, pk["w_c"], pk["b_c"], pk["w_r2"], pk["b_r2"], pk["ref"])
        self.__dict__["_last_path"] = "kernels"
        return x.view(B, Q, C), logits.view(B, Q, -1), boxes.view(B, Q, 4)

    @torch.no_grad()
    def forward(self, enc, st):
        """-> (hs_last (B,Q,C), logits (B,Q,num_classes), boxes (B,Q,4) normalised cxcywh) on whichever path the
        configuration allows; ``last_path`` says which one ran."""
        if self.fused_ok(enc["tokens"]):
            return self.forward_kernels(enc, st)
        self.__dict__["_last_path"] = "modules"
        return self.forward_module(enc, st)

    @property
    def last_path(self):
        return self.__dict__.get("_last_path")


def meta_rows(img_metas):
    """Per-image [img h, img w, scale_factor x4] (B,6) fp32 on the host: what demf_detr2d_select decodes with."""
    rows = []
    for m in img_metas:
        sf = np.asarray(m.get("scale_factor", (1.0, 1.0, 1.0, 1.0)), np.float64).reshape(-1)
        if sf.size == 1:
            sf = np.repeat(sf, 4)
        rows.append([float(m["img_shape"][0]), float(m["img_shape"][1])] + [float(v) for v in sf[:4]])
    return torch.tensor(rows, dtype=torch.float32)


def select_host(logits, boxes, meta, k, thr, rescale):
    """demf_detr2d_select's contract in torch for tensors that are not on the device (the CPU module path): -> (rows
    (B,k,6), counts (B,) int32, selected flat indices (B, min(k, Q*C)) int64)."""
    B, Q, C = logits.shape
    flat = logits.reshape(B, Q * C)
    kk = min(int(k), Q * C)
    key = torch.where(torch.isnan(flat), torch.full_like(flat, -float("inf")), flat)
    idx = torch.sort(key, dim=1, descending=True, stable=True)[1][:, :kk]
    score = torch.gather(flat, 1, idx).sigmoid()
    q, c = idx // C, idx % C
    bx = torch.gather(boxes, 1, q[..., None].expand(-1, -1, 4))
    ih, iw = meta[:, 0:1].to(bx.dtype), meta[:, 1:2].to(bx.dtype)
    x1 = ((bx[..., 0] - 0.5 * bx[..., 2]) * iw).clamp(min=0).minimum(iw)
    y1 = ((bx[..., 1] - 0.5 * bx[..., 3]) * ih).clamp(min=0).minimum(ih)
    x2 = ((bx[..., 0] + 0.5 * bx[..., 2]) * iw).clamp(min=0).minimum(iw)
    y2 = ((bx[..., 1] + 0.5 * bx[..., 3]) * ih).clamp(min=0).minimum(ih)
    xy = torch.stack([x1, y1, x2, y2], -1)
    if rescale:
        xy = xy / meta[:, None, 2:6].to(bx.dtype)
    keep = (score > thr) if thr >= 0 else torch.ones_like(score, dtype=torch.bool)
    rows = torch.zeros((B, int(k), 6), dtype=boxes.dtype)
    rows[:, :kk] = torch.cat([xy, score[..., None], c[..., None].to(bx.dtype)], -1) * keep[..., None]
    return rows, keep.sum(1).to(torch.int32), idx


class Detr2D(nn.Module):
    """``ImVoteNet_Deformdetr`` of the image-only config: ``img_backbone``, ``img_neck``, the encoder
    (``img_encoder``: this package's ``DeformableDetrEncoder``, upstream's ``img_bbox_head.transformer.encoder`` +
    ``level_embeds``) and ``img_bbox_head``.  Test side only."""

    def __init__(self, num_query=300, num_classes=10, num_decoder_layers=6, max_per_img=100, num_points=4,
                 image_stream=None, **image_stream_kwargs):
        super().__init__()
        stream = image_stream if image_stream is not None else ImageStream(**image_stream_kwargs)
        self.__dict__["_stream"] = stream           # (not a sub-module: its three parts are registered below)
        self.img_backbone, self.img_neck, self.img_encoder = stream.img_backbone, stream.img_neck, stream.img_encoder
        enc = self.img_encoder
        a = enc.encoder.layers[0].attentions[0]
        ffn = enc.encoder.layers[0].ffns[0].layers[0][0].out_features
        self.img_bbox_head = DeformableDETRHead(num_query, num_classes, enc.embed_dims, num_decoder_layers,
                                                a.num_heads, a.num_levels, num_points, ffn,
                                                max_per_img=max_per_img)
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("Detr2D is the test side of the 2D detector: stage-1 training is not built")
        return super().train(False)

    # ---- checkpoints --------------------------------------------------------------------------------------------
    _ENC = (("img_bbox_head.transformer.encoder.", "img_encoder.encoder."),
            ("img_bbox_head.transformer.level_embeds", "img_encoder.level_embeds"))

    def load_state_dict(self, state_dict, strict=True, **kw):
        """A stage-1 checkpoint as published (``img_backbone.* / img_neck.* / img_bbox_head.*``): the encoder's keys
        are routed to ``img_encoder``; every other key is upstream's.  This module's own ``state_dict()`` loads too."""
        out = {}
        for key, v in state_dict.items():
            for up, own in self._ENC:
                if key.startswith(up):
                    key = own + key[len(up):]
                    break
            out[key] = v
        return super().load_state_dict(out, strict=strict, **kw)

    def stage1_state_dict(self):
        """The weights under the stage-1 checkpoint's names (what ``load_state_dict`` takes and
        ``DeMFVoteNet.load_state_dict`` remaps)."""
        out = {}
        for key, v in self.state_dict().items():
            for up, own in self._ENC:
                if key.startswith(own):
                    key = up + key[len(own):]
                    break
            out[key] = v
        return out

    # ---- forward ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract_img_feat(self, img, img_metas):
        """-> the encoder's token dict (``ImageStream.tokens``)."""
        return self.__dict__["_stream"].tokens(img, img_metas)

    @torch.no_grad()
    def forward_head(self, enc, img_metas):
        """enc: the encoder's token dict, or the neck's pyramid (list of (B,C,h,w)) -> (hs_last, logits, boxes)."""
        if not (isinstance(enc, dict) and "mask_flatten" in enc):
            enc = self.img_encoder.forward_tokens(enc, img_metas)
        st = self.img_encoder._static(img_metas, enc["spatial"], enc["tokens"].device)
        return self.img_bbox_head(enc, st)

    def _select(self, logits, boxes, img_metas, thr, rescale, store=None):
        """-> (rows (B,k,6), counts (B,)) - on the device appended to ``store`` without a host sync."""
        k = self.img_bbox_head.max_per_img
        meta = meta_rows(img_metas)
        if not logits.is_cuda:
            rows, counts, _ = select_host(logits, boxes, meta, k, thr, rescale)
            return rows, counts
        from ..detections import Detection2DStore
        B = logits.shape[0]
        if store is None:
            store = Detection2DStore(B, k, device=logits.device)
        first = store.reserve(B, k)
        rows, counts = store.rows[first:first + B], store.counts[first:first + B]
        ops.detr2d_select(logits.float().contiguous(), boxes.float().contiguous(),
                          meta.to(logits.device, non_blocking=True), k, thr, rescale, rows, counts, store.flag)
        return rows, counts

    @torch.no_grad()
    def simple_test_img_only(self, img, img_metas, rescale=False):
        """mmdet ``DeformableDETRHead.simple_test`` -> per image (det_bboxes (k,5) = [x1,y1,x2,y2,score], det_labels
        (k,) int64), k = min(max_per_img, Q*C) (_get_bboxes_single)."""
        _, logits, boxes = self.forward_head(self.extract_img_feat(img, img_metas), img_metas)
        rows, counts = self._select(logits, boxes, img_metas, -1.0, rescale)
        n = counts.tolist()
        return [(rows[i, :n[i], :5].clone(), rows[i, :n[i], 5].to(torch.int64)) for i in range(len(n))]

    @torch.no_grad()
    def extract_bboxes_2d(self, img, img_metas, train=False, bboxes_2d=None, **unused):
        """imvotenet_deform.py:188-239 at test time -> per image (n,6) rows [x1,y1,x2,y2,score,class] with score >
        0.09 in score order."""
        if train:
            raise NotImplementedError("extract_bboxes_2d(train=True) drops a random half of the boxes for stage-2 "
                                      "training of ImVoteNet: not built (test side only)")
        if bboxes_2d is not None:
            return [b.float() for b in bboxes_2d]
        _, logits, boxes = self.forward_head(self.extract_img_feat(img, img_metas), img_metas)
        rows, counts = self._select(logits, boxes, img_metas, SCORE_THR, False)
        return [rows[i, :n].clone() for i, n in enumerate(counts.tolist())]

    @torch.no_grad()
    def predict_into(self, store, img=None, img_metas=None, **unused):
        """``extract_bboxes_2d`` whose rows stay on the device: the batch's images are appended to ``store``
        (detections.Detection2DStore); nothing is returned and nothing waits for the GPU."""
        _, logits, boxes = self.forward_head(self.extract_img_feat(img, img_metas), img_metas)
        self._select(logits, boxes, img_metas, store.score_thr, False, store)
