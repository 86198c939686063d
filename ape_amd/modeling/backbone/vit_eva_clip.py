"""EVA-02-CLIP ViT backbone on the HIP kernels (its SimpleFeaturePyramid: simple_feature_pyramid.py).

Host-side mirror of ape/modeling/backbone/vit_eva_clip.py (ViT :570-754, Block :505-523, Attention :218-268,
SwiGLU :125-132, SimpleFeaturePyramid :757-922) and the helpers it uses from utils_eva02.py (PatchEmbed :190-216,
get_abs_pos :158-187, window_partition :19-63, VisionRotaryEmbeddingFast :307-346): same class names, constructor
kwargs and state-dict keys, so the reference's LazyConfig (configs/common/backbone/vitl_eva02_clip.py) instantiates
it unchanged.  The arithmetic runs through ape_amd.ops (C-ABI -> HIP); there is no PyTorch fallback.  What the three ViT
families share (weight layouts, images -> embedded tokens) lives in vit_common.py and is re-exported here.

MI355X-first layout: tokens stay token-major [N, C] and in WINDOW-MAJOR order through all blocks, so window
partition / unpartition are free (global blocks just use a RoPE table permuted to the same order); q|k are one
GEMM with the RoPE rotation fused in its epilogue, V is produced transposed for the flash-attention kernel,
w1|w2 are one interleaved GEMM with the SwiGLU epilogue, and the FPN's deconvolutions / 1x1 / 3x3 convolutions are
GEMMs over token-major maps (the pixel-shuffle and window orders are folded into the 3x3 im2col gather).
"""
import os
from functools import partial

import torch
import torch.nn as nn

from ... import ops
from ...packing import attach_cache, f32, ln_params, pack_matrix, round_up
from ...stagetap import tap
from .simple_feature_pyramid import LastLevelMaxPool, SimpleFeaturePyramid  # noqa: F401
from .vit_common import (Backbone, PatchEmbed, ViTBase, VisionRotaryEmbeddingFast, fork_vt_then_qk, pack_padded_up,  # noqa: F401
                         pack_swiglu_up, pad_heads, padded_head_dim, window_major_order)

__all__ = ["ViT", "SimpleFeaturePyramid"]


class SwiGLU(nn.Module):
    def __init__(self, in_features, hidden_features, norm_layer, subln=True):
        super().__init__()
        self.w1 = nn.Linear(in_features, hidden_features)
        self.w2 = nn.Linear(in_features, hidden_features)
        self.ffn_ln = norm_layer(hidden_features) if subln else nn.Identity()
        self.w3 = nn.Linear(hidden_features, in_features)


class Mlp(nn.Module):
    """fc1 -> GELU -> (ffn_ln) -> fc2 (vit_eva_clip.py:67-98): the MLP of the non-SwiGLU configurations (ViT-e)"""

    def __init__(self, in_features, hidden_features, norm_layer, subln=False):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.ffn_ln = norm_layer(hidden_features) if subln else nn.Identity()
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, rope, norm_layer, subln=True, qkv_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.subln = subln
        if subln:
            self.q_proj = nn.Linear(dim, dim, bias=False)
            self.k_proj = nn.Linear(dim, dim, bias=False)
            self.v_proj = nn.Linear(dim, dim, bias=False)
        else:
            self.qkv = nn.Linear(dim, dim * 3, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.v_bias = nn.Parameter(torch.zeros(dim))
        else:
            self.q_bias = self.v_bias = None
        self.inner_attn_ln = norm_layer(dim) if subln else nn.Identity()
        self.proj = nn.Linear(dim, dim)
        self.rope = rope

    def qkv_weights(self):
        """(Wq, Wk, Wv [E, E], q bias, v bias [E] or None) of either parameterisation (vit_eva_clip.py:236-260)"""
        if self.subln:
            wq, wk, wv = self.q_proj.weight, self.k_proj.weight, self.v_proj.weight
        else:
            E = self.qkv.weight.shape[1]
            wq, wk, wv = self.qkv.weight[:E], self.qkv.weight[E:2 * E], self.qkv.weight[2 * E:]
        return wq.detach().float(), wk.detach().float(), wv.detach().float(), self.q_bias, self.v_bias


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, norm_layer, window_size, rope, postnorm=False, subln=True, naiveswiglu=True,
                 qkv_bias=True):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, rope, norm_layer, subln=subln, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(dim)
        hidden = int(dim * mlp_ratio)
        self.mlp = SwiGLU(dim, hidden, norm_layer, subln=subln) if naiveswiglu else Mlp(dim, hidden, norm_layer, subln=subln)
        self.window_size = window_size
        self.postnorm, self.subln, self.naiveswiglu = postnorm, subln, naiveswiglu
        attach_cache(self)

    def packed(self, dt):
        def build(dt):
            a, m = self.attn, self.mlp
            wq, wk, wv, qb, vb = a.qkv_weights()
            E = wq.shape[1]
            nh = a.num_heads
            hd = E // nh
            hdp = padded_head_dim(hd)
            dev = wq.device
            pad = partial(pad_heads, nh=nh, hd=hd, hdp=hdp)
            zeros = torch.zeros(E, dtype=torch.float32, device=dev)
            qb = qb.detach().float() if qb is not None else zeros
            vb = vb.detach().float() if vb is not None else zeros
            wproj = a.proj.weight.detach().float()
            if hdp != hd:                          # zero COLUMNS of the out projection where the attention output is padding
                wproj = pad(wproj.t().contiguous()).t().contiguous()
            P = dict(
                hd=hd, hdp=hdp, Ep=nh * hdp,
                wqk=pack_matrix(torch.cat([pad(wq), pad(wk)], 0), dt),
                bqk=torch.cat([pad(qb), torch.zeros(nh * hdp, dtype=torch.float32, device=dev)]).contiguous(),
                wv=pack_matrix(pad(wv), dt), bv=pad(vb).contiguous(),
                wproj=pack_matrix(wproj, dt), bproj=f32(a.proj.bias), n1=ln_params(self.norm1), n2=ln_params(self.norm2))
            if self.subln:
                P["nin"] = ln_params(a.inner_attn_ln)
                P["nffn"] = ln_params(m.ffn_ln)
                P.update(self._folded_inner_ln(a, dt, hd == hdp))
            if self.naiveswiglu:
                w12, b12, hid, hid_pad = pack_swiglu_up(m.w1.weight, m.w1.bias, m.w2.weight, m.w2.bias, dt)
                P.update(w12=w12, b12=b12, hid=hid, hid_pad=hid_pad,
                         w3=pack_matrix(m.w3.weight, dt, kpad=64), b3=f32(m.w3.bias), **self._folded_subln(m, dt))
            else:
                w1, b1, hid, hid_pad = pack_padded_up(m.fc1, dt)
                P.update(w1=w1, b1=b1, hid=hid, hid_pad=hid_pad,
                         w2=pack_matrix(m.fc2.weight, dt, kpad=64), b2=f32(m.fc2.bias))
            return P
        return self._pack.get(self, dt, build)

    @staticmethod
    def _folded_subln(m, dt):
        """bf16 production mode: the SwiGLU sub-LayerNorm (vit_eva_clip.py:129-131) is folded into the down projection,
        LN(h) W3^T = rstd (h W'^T) - rstd mean rowsum(W') + W3 b_ln  with  W' = W3 diag(gamma)  (ApeGemmArgs.rowscale ...):
        the 2730-wide activation is read once (statistics) instead of read + written + read again."""
        if dt not in ops.HALF16 or not isinstance(m.ffn_ln, nn.LayerNorm) or os.environ.get("APE_NO_LNFOLD") == "1":
            return {}
        w3 = m.w3.weight.detach().float()
        g, b = m.ffn_ln.weight.detach().float(), m.ffn_ln.bias.detach().float()
        w3f = pack_matrix(w3 * g[None, :], dt, kpad=64)
        return dict(w3f=w3f, c1=w3f.float().sum(dim=1).contiguous(),                 # row sums of the ROUNDED folded weight
                    c2=(w3 @ b + m.w3.bias.detach().float()).contiguous())

    @staticmethod
    def _folded_inner_ln(a, dt, unpadded):
        """16-bit production mode (round 6): the attention's inner LayerNorm (vit_eva_clip.py:258-262, `inner_attn_ln` between the
        attention and its output projection) folded into that projection exactly like the SwiGLU sub-LayerNorm below:
        LN(o) Wp^T + bp = rstd (o W'^T) - rstd mean rowsum(W') + (Wp b_ln + bp)  with  W' = Wp diag(gamma).  The row statistics of the
        stored attention output come from the projection's own launch (ops.gemm rowstats=): no LayerNorm launch, no second copy of o."""
        if dt not in ops.HALF16 or not unpadded or not isinstance(a.inner_attn_ln, nn.LayerNorm) or os.environ.get("APE_NO_LNFOLD") == "1":
            return {}
        wp = a.proj.weight.detach().float()
        g, b = a.inner_attn_ln.weight.detach().float(), a.inner_attn_ln.bias.detach().float()
        wpf = pack_matrix(wp * g[None, :], dt)
        return dict(wprojf=wpf, cp1=wpf.float().sum(dim=1).contiguous(),                 # row sums of the ROUNDED folded weight
                    cp2=(wp @ b + a.proj.bias.detach().float()).contiguous())

    def _attention(self, xn, P, rope, nwin, ntok_win, vt_buf, images):
        """the attention branch on the normalised (pre-norm) or raw (post-norm) tokens xn [rows, E] -> [rows, Ep]"""
        nh = self.attn.num_heads
        hd, hdp, Ep = P["hd"], P["hdp"], P["Ep"]
        qk, vjob = fork_vt_then_qk(xn, P, vt_buf, rope)
        vt = vjob.join()
        if self.window_size > 0:
            o = ops.attention(qk[:, :Ep], qk[:, Ep:], vt, batch=nwin, n=ntok_win, heads=nh, head_dim=hdp, scale=hd ** -0.5)
        else:
            o = ops.attention(qk[:, :Ep], qk[:, Ep:], vt, batch=images, n=xn.shape[0] // images, heads=nh, head_dim=hdp, scale=hd ** -0.5)
        if self.subln and "wprojf" not in P:
            o = ops.layernorm(o, P["nin"][0], P["nin"][1], P["nin"][2], out_dtype=xn.dtype)
        return o

    def _out_proj(self, o, P, residual, out_dtype):
        """the attention's output projection (+ residual), with the inner LayerNorm folded in when packed so"""
        if "wprojf" in P:
            return ops.gemm(o, P["wprojf"], P["cp2"], residual=residual, out_dtype=out_dtype, rowstats=(o.shape[1], P["nin"][2], P["cp1"]))
        return ops.gemm(o, P["wproj"], P["bproj"], residual=residual, out_dtype=out_dtype)

    def _mlp(self, xn, P, dt, residual, out_dtype):
        """the MLP branch: residual + mlp(xn) (residual None: mlp(xn) alone) in out_dtype"""
        hbuf = torch.empty((xn.shape[0], P["hid_pad"]), dtype=dt, device=xn.device)
        if self.naiveswiglu:
            ops.gemm(xn, P["w12"], P["b12"], act=ops.ACT_SWIGLU, out=hbuf)
            if "w3f" in P:
                # the row statistics of the stored hidden activation come from the down projection's own launch where the 256 x 128 tile
                # kernel runs it (ops.gemm rowstats=; else a row_stats launch as in rounds 3-5): the K padding of hbuf is exact zeros
                return ops.gemm(hbuf, P["w3f"], P["c2"], residual=residual, rowstats=(P["hid"], P["nffn"][2], P["c1"]), out_dtype=out_dtype)
            if self.subln:
                hbuf = ops.layernorm(hbuf[:, :P["hid"]], P["nffn"][0], P["nffn"][1], P["nffn"][2], out_dtype=dt, cpad=P["hid_pad"])
            return ops.gemm(hbuf, P["w3"], P["b3"], residual=residual, out_dtype=out_dtype)
        ops.gemm(xn, P["w1"], P["b1"], act=ops.ACT_GELU, out=hbuf)
        if self.subln:
            hbuf = ops.layernorm(hbuf[:, :P["hid"]], P["nffn"][0], P["nffn"][1], P["nffn"][2], out_dtype=dt, cpad=P["hid_pad"])
        return ops.gemm(hbuf, P["w2"], P["b2"], residual=residual, out_dtype=out_dtype)

    def forward_tokens(self, x, dt, rope, nwin, ntok_win, vt_buf, last=False, images=1):
        """pre-norm block (vit_eva_clip.py:519-523): x [images * N, E] fp32 residual stream (window-major per image).
        rope = (cos, sin, rows) or None; nwin = windows of ALL images.  Returns the new stream."""
        P = self.packed(dt)
        xn = ops.layernorm(x, P["n1"][0], P["n1"][1], P["n1"][2], out_dtype=dt)
        o = self._attention(xn, P, rope, nwin, ntok_win, vt_buf, images)
        x = self._out_proj(o, P, x, torch.float32)
        xn = ops.layernorm(x, P["n2"][0], P["n2"][1], P["n2"][2], out_dtype=dt)
        return self._mlp(xn, P, dt, x, dt if last else torch.float32)

    def forward_tokens_postnorm(self, x32, xb, dt, rope, nwin, ntok_win, vt_buf, images=1):
        """post-norm block (vit_eva_clip.py:505-517): x += norm1(attn(x)); x += norm2(mlp(x)).  x32: the fp32 residual stream,
        updated IN PLACE; xb: the same values in the GEMM operand type (x32 itself in fp32 mode).  Returns the new xb."""
        P = self.packed(dt)
        cdt = None if dt == torch.float32 else dt
        o = self._attention(xb, P, rope, nwin, ntok_win, vt_buf, images)
        t = self._out_proj(o, P, None, torch.float32)
        xb = ops.postnorm_residual(x32, t, P["n1"], copy_dtype=cdt)
        xb = x32 if xb is None else xb
        t = self._mlp(xb, P, dt, None, torch.float32)
        xb = ops.postnorm_residual(x32, t, P["n2"], copy_dtype=cdt)
        return x32 if xb is None else xb


def _with_packed(cos, sin, rows):
    """(cos, sin, rows[, packed]) -- packed = [rows, hd / 2, 2] (cos, sin) per rotate_half pair when both columns of every pair share
    an angle (VisionRotaryEmbeddingFast repeats each frequency twice, vit_eva_clip.py:179-216): the form the 256-row GEMM tile stages
    through LDS (ApeGemmArgs.rope_cs); checked, not assumed"""
    if torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2]):
        return (cos, sin, rows, torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1).contiguous())
    return (cos, sin, rows)


class ViT(ViTBase):
    def __init__(self, img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                 qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0,
                 norm_layer=partial(nn.LayerNorm, eps=1e-6), init_values=None, use_abs_pos=True, use_rel_pos=False,
                 rope=False, postnorm=False, pt_hw_seq_len=16, intp_freq=False, naiveswiglu=False, subln=False,
                 window_size=0, window_block_indexes=(), residual_block_indexes=(), use_act_checkpoint=False,
                 pretrain_img_size=224, pretrain_use_cls_token=True, out_feature="last_feat", xattn=False, frozen_stages=-1):
        super().__init__()
        # the HIP path implements the EVA-02-CLIP configurations of the APE configs: rope + sub-LN + SwiGLU + pre-norm (ViT-L,
        # vitl_eva02_clip.py:9-48) and packed-qkv + GELU MLP + post-norm without rope (ViT-e, vite_eva02_clip_1024.py:9-49)
        assert use_abs_pos and init_values is None, "ape_amd ViT: absolute position embedding, no layer scale (every APE config)"
        assert len(residual_block_indexes) == 0 and patch_size == 16
        assert not rope or intp_freq, "ape_amd ViT: rope tables are interpolated to the token grid (intp_freq=True) in the APE configs"
        assert (img_size // patch_size) % window_size == 0, "token grid must be a multiple of the window size"
        assert embed_dim <= 2048 or not postnorm, "ape_amd ViT: the post-norm residual kernel holds rows of <= 2048 channels"
        self._init_embed(img_size, patch_size, in_chans, embed_dim, window_size, pretrain_img_size, pretrain_use_cls_token)
        self.postnorm = postnorm
        half_head_dim = embed_dim // num_heads // 2
        hw = img_size // patch_size
        if rope:
            assert padded_head_dim(2 * half_head_dim) == 2 * half_head_dim, "ape_amd ViT: rope needs a head width of 32 / 64 / 128"
            self.rope_win = VisionRotaryEmbeddingFast(half_head_dim, pt_seq_len=pt_hw_seq_len, ft_seq_len=window_size)
            self.rope_glb = VisionRotaryEmbeddingFast(half_head_dim, pt_seq_len=pt_hw_seq_len, ft_seq_len=hw)
        else:
            self.rope_win = self.rope_glb = None
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, norm_layer, window_size if i in window_block_indexes else 0,
                  self.rope_win if i in window_block_indexes else self.rope_glb, postnorm=postnorm, subln=subln,
                  naiveswiglu=naiveswiglu, qkv_bias=qkv_bias) for i in range(depth)])
        self._init_tail(out_feature)

    def token_order(self, hw):
        """(tok2raster, raster2tok) of the feature this ViT hands to the pyramid: window-major order"""
        return window_major_order(hw, hw, self.window_size)

    def packed(self, dt):
        def build(dt):
            hw = self.img_size // self.patch_size
            dev = self.pos_embed.device
            t2r, r2t = window_major_order(hw, hw, self.window_size)
            t2r, r2t = t2r.to(dev), r2t.to(dev)
            return dict(
                self._packed_embed(dt, t2r), t2r=t2r, r2t=r2t,
                rope_win=None if self.rope_win is None else _with_packed(f32(self.rope_win.freqs_cos), f32(self.rope_win.freqs_sin), self.window_size ** 2),
                rope_glb=None if self.rope_glb is None else _with_packed(f32(self.rope_glb.freqs_cos)[t2r.long()].contiguous(),
                                                                         f32(self.rope_glb.freqs_sin)[t2r.long()].contiguous(), hw * hw),
            )
        return self._pack.get(self, dt, build)

    def forward_tokens(self, image, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), stages=None):
        """image [3,h,w] fp32 (h,w <= img_size) -> last feature [N, E] in the compute dtype, WINDOW-MAJOR token order.
        stages: optional dict / StageTap (stagetap.py) recording "vit_embed" and every block's output "vit_blk<i>".
        A list of B images (sizes may differ) runs as ONE pass over [B * N, E]: every linear sees B x 4096 rows (the big-tile
        GEMM kernels need that many to fill 256 CUs), windows / global attention stay per image.  Rows are independent in
        every op of the ViT, so each image's result is bit-identical to its own single-image pass."""
        dt = self.compute_dtype
        P = self.packed(dt)
        x, B, n = self.embed_images(P, P["t2r"], image, mean, std, stages)
        nwin = (P["hw"] // self.window_size) ** 2 * B
        Ep = self.blocks[0].packed(dt)["Ep"]
        vt_buf = ops.zeros((Ep, round_up(B * n, 64)), dt, x.device)
        if self.postnorm:
            # the fp32 stream is updated IN PLACE by the post-norm residual kernel: with taps, work on a private copy (a forced
            # tensor belongs to the teacher) and record copies
            x32 = x.clone() if stages is not None else x
            cdt = None if dt == torch.float32 else dt
            xb = x32 if cdt is None else ops.postnorm_residual(x32, None, None, copy_dtype=cdt)
            for i, blk in enumerate(self.blocks):
                rope = P["rope_win"] if blk.window_size > 0 else P["rope_glb"]
                xb = blk.forward_tokens_postnorm(x32, xb, dt, rope, nwin, self.window_size ** 2, vt_buf, images=B)
                if stages is not None:
                    rec = x32.clone()
                    forced = tap(stages, f"vit_blk{i}", rec)
                    if forced is not rec:                            # teacher forcing: the next block starts from the teacher's stream
                        x32 = forced.float().clone()
                        xb = x32 if cdt is None else ops.postnorm_residual(x32, None, None, copy_dtype=cdt)
            return xb
        for i, blk in enumerate(self.blocks):
            rope = P["rope_win"] if blk.window_size > 0 else P["rope_glb"]
            x = blk.forward_tokens(x, dt, rope, nwin, self.window_size ** 2, vt_buf, last=(i == len(self.blocks) - 1), images=B)
            x = tap(stages, f"vit_blk{i}", x)
        return x
