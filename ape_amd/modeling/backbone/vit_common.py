"""What the three ViT backbones (vit_eva_clip.py, vit_eva.py, vit_eva02.py) share: how a ViT's weights are laid out for the kernels
and how images become the embedded token stream.

The helpers take values, never a model family's name: head widths, hidden widths, a token order.  The blocks themselves (rope,
relative-position channels, the post-norm stream, gathered 14 x 14 windows) stay with their families.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...packing import attach_cache, f32, pack_matrix, round_up
from ...stagetap import tap


class VisionRotaryEmbeddingFast(nn.Module):
    """Persistent cos/sin tables [ft*ft, 2*dim] (utils_eva02.py:307-344); applied inside the q|k GEMM epilogue."""

    def __init__(self, dim, pt_seq_len=16, ft_seq_len=None, theta=10000):
        super().__init__()
        freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: (dim // 2)].float() / dim))
        if ft_seq_len is None:
            ft_seq_len = pt_seq_len
        t = torch.arange(ft_seq_len) / ft_seq_len * pt_seq_len
        freqs = (t[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
        fh = freqs[:, None, :].expand(ft_seq_len, ft_seq_len, dim)
        fw = freqs[None, :, :].expand(ft_seq_len, ft_seq_len, dim)
        full = torch.cat((fh, fw), dim=-1)
        self.register_buffer("freqs_cos", full.cos().reshape(-1, 2 * dim))
        self.register_buffer("freqs_sin", full.sin().reshape(-1, 2 * dim))


class PatchEmbed(nn.Module):
    def __init__(self, kernel_size=(16, 16), stride=(16, 16), padding=(0, 0), in_chans=3, embed_dim=768):
        super().__init__()
        assert tuple(kernel_size) == (16, 16) and tuple(stride) == (16, 16) and in_chans == 3, "HIP patchify is 16x16/16, RGB"
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=kernel_size, stride=stride, padding=padding)


def padded_head_dim(hd):
    """the flash-attention kernel's head widths: 32 / 64 / 128; narrower heads are zero-padded by the weight packing (zero q / k
    columns add nothing to the scores, zero v columns produce zero outputs that meet zero columns of the out projection)"""
    for w in (32, 64, 128):
        if hd <= w:
            return w
    raise ValueError(f"ape_amd ViT: head width {hd} > 128")


def window_major_order(ht, wt, ws):
    """token order used inside the backbone: (window row, window col, row in window, col in window).
    returns (tok2raster int32 [N], raster2tok int32 [N])"""
    r = torch.arange(ht * wt).view(ht // ws, ws, wt // ws, ws).permute(0, 2, 1, 3).reshape(-1)
    inv = torch.empty_like(r)
    inv[r] = torch.arange(ht * wt)
    return r.to(torch.int32), inv.to(torch.int32)


def abs_pos_embed(pos_embed, has_cls, hw):
    """get_abs_pos (utils_eva02.py:158-187): drop cls, bicubic resize to the token grid -- a per-model constant.
    -> [hw * hw, C] fp32 in RASTER order; the caller indexes it with its own token order.  torch's bicubic arithmetic on purpose
    (packing.resize_pos_embed says why)."""
    pos = pos_embed.detach().float()
    if has_cls:
        pos = pos[:, 1:]
    size = int(math.sqrt(pos.shape[1]))
    if size != hw:
        pos = F.interpolate(pos.reshape(1, size, size, -1).permute(0, 3, 1, 2), size=(hw, hw), mode="bicubic",
                            align_corners=False).permute(0, 2, 3, 1)
    return pos.reshape(hw * hw, -1)


def pad_heads(w, nh, hd, hdp):
    """[nh * hd, ...] -> [nh * hdp, ...], zero rows behind every head (see padded_head_dim).  The out projection needs zero COLUMNS
    where the attention output is padding: pad_heads(w.t().contiguous(), ...).t().contiguous()"""
    if hdp == hd:
        return w
    out = torch.zeros((nh, hdp) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
    out[:, :hd] = w.reshape((nh, hd) + tuple(w.shape[1:]))
    return out.reshape((nh * hdp,) + tuple(w.shape[1:]))


def pack_swiglu_up(w1, b1, w2, b2, dt):
    """SwiGLU up-projection, (gate, up) rows interleaved for the fused epilogue: w1 / w2 [hid, E], b1 / b2 [hid] ->
    (w12 [2 * hid_pad, E] in dt, b12 fp32, hid, hid_pad).  Zero (gate, up) rows beyond 2 * hid: the fused SwiGLU epilogue writes
    exact zeros into the K padding of the down projection"""
    hid, E = w1.shape
    hid_pad = round_up(hid, 64)
    w12 = torch.zeros((2 * hid_pad, E), dtype=torch.float32, device=w1.device)
    b12 = torch.zeros((2 * hid_pad,), dtype=torch.float32, device=w1.device)
    for dst, gate, up in ((w12, w1, w2), (b12, b1, b2)):
        dst[0:2 * hid:2], dst[1:2 * hid:2] = gate, up
    return pack_matrix(w12, dt), b12, hid, hid_pad


def pack_padded_up(fc1, dt):
    """GELU MLP up-projection: nn.Linear fc1 -> (w1 [hid_pad, E] in dt, b1 fp32, hid, hid_pad)"""
    hid, E = fc1.weight.shape
    hid_pad = round_up(hid, 64)
    w1 = torch.zeros((hid_pad, E), dtype=torch.float32, device=fc1.weight.device)     # zero rows: gelu(0) = 0 exactly in the K padding
    w1[:hid] = fc1.weight.detach().float()
    b1 = torch.zeros((hid_pad,), dtype=torch.float32, device=fc1.weight.device)
    b1[:hid] = fc1.bias.detach().float()
    return pack_matrix(w1, dt), b1, hid, hid_pad


def fork_vt_then_qk(xn, P, vt_buf, rope=None):
    """-> (qk [rows, 2 * Ep], the V^T branch's handle: .join() gives V^T before the attention reads it)"""
    # V^T on a parallel graph branch: two M = 4096 GEMMs fill the chip better together than one after the other
    vjob = ops.fork(lambda: ops.gemm(xn, P["wv"], P["bv"], trans_out=True, out=vt_buf))
    if rope is not None:
        return ops.gemm(xn, P["wqk"], P["bqk"], rope=(rope[0], rope[1], rope[2], P["hd"], 2 * P["Ep"]) + tuple(rope[3:])), vjob
    return ops.gemm(xn, P["wqk"], P["bqk"]), vjob


class Backbone(nn.Module):
    """minimal stand-in for detectron2.modeling.backbone.Backbone (output_shape / size_divisibility contract)"""

    @property
    def size_divisibility(self):
        return 0

    @property
    def padding_constraints(self):
        return {}

    def output_shape(self):
        from types import SimpleNamespace
        return {n: SimpleNamespace(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n])
                for n in self._out_features}


class ViTBase(Backbone):
    """what every ViT constructor repeats, images -> embedded tokens, and the reference-signature forward.  A subclass calls
    _init_embed, registers its rope tables and blocks, then _init_tail: the registration order is the state dict's key order."""

    def _init_embed(self, img_size, patch_size, in_chans, embed_dim, window_size, pretrain_img_size, pretrain_use_cls_token):
        self.pretrain_use_cls_token = pretrain_use_cls_token
        self.img_size, self.patch_size, self.embed_dim, self.window_size = img_size, patch_size, embed_dim, window_size
        self.patch_embed = PatchEmbed(in_chans=in_chans, embed_dim=embed_dim)
        num_patches = (pretrain_img_size // patch_size) ** 2
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + (1 if pretrain_use_cls_token else 0), embed_dim))

    def _init_tail(self, out_feature):
        self._out_feature_channels = {out_feature: self.embed_dim}
        self._out_feature_strides = {out_feature: self.patch_size}
        self._out_features = [out_feature]
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.compute_dtype = torch.bfloat16
        attach_cache(self)

    def _packed_embed(self, dt, t2r=None):
        """the packed dict's entries of the embedding: grid side, position embedding in the token order t2r (None: raster), patch GEMM"""
        hw = self.img_size // self.patch_size
        pos = abs_pos_embed(self.pos_embed, self.pretrain_use_cls_token, hw)
        w = self.patch_embed.proj.weight
        return dict(hw=hw, pos=(pos if t2r is None else pos[t2r.long()]).contiguous(), wpe=pack_matrix(w.reshape(w.shape[0], -1), dt),
                    bpe=f32(self.patch_embed.proj.bias))

    def embed_images(self, P, t2r, image, mean, std, stages):
        """image [3,h,w] fp32 (h,w <= img_size) or a list of B such images (sizes may differ) -> (x [B * N, E] fp32: patch embedding +
        position embedding, tokens in the order t2r per image; B; N)"""
        dt = self.compute_dtype
        hw = P["hw"]
        n = hw * hw
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        B = len(images)
        if B == 1:
            patches = ops.patchify(images[0], t2r, hw, hw, mean, std, out_dtype=dt)
            pos = P["pos"]
        else:
            patches = torch.empty((B * n, 768), dtype=dt, device=images[0].device)
            for b, im in enumerate(images):
                ops.patchify(im, t2r, hw, hw, mean, std, out_dtype=dt, out=patches[b * n:(b + 1) * n])
            if ("pos", B) not in P:
                P[("pos", B)] = P["pos"].repeat(B, 1).contiguous()
            pos = P[("pos", B)]
        x = tap(stages, "vit_embed", ops.gemm(patches, P["wpe"], P["bpe"], residual=pos, out_dtype=torch.float32))
        return x, B, n

    def forward(self, x):
        """reference signature: normalised, padded NCHW batch -> {"last_feat": [B, E, h/16, w/16]}"""
        outs = []
        P = self.packed(self.compute_dtype)
        for b in range(x.shape[0]):
            t = self.forward_tokens(x[b].float().contiguous())
            if "r2t" in P:                               # the token order is not raster
                t = t[P["r2t"].long()]
            outs.append(t.float().reshape(P["hw"], P["hw"], -1).permute(2, 0, 1))
        return {self._out_features[0]: torch.stack(outs)}
