"""SimpleFeaturePyramid (ViTDet's pyramid: strides 4 / 8 / 16 / 32 from the ViT's single stride-16 feature, + p6) on the HIP kernels.

Host-side mirror of ape/modeling/backbone/vit_eva_clip.py :757-922 (identical in vit_eva02.py :637-804 and vit_eva.py of the
reference): same class name, constructor kwargs and state-dict keys.  Shared by the three ViT backbones.  The deconvolutions / 1x1 /
3x3 convolutions are GEMMs over token-major maps; the pixel-shuffle and the ViT's token order are folded into the 3x3 im2col gather.
"""
import math

import torch
import torch.nn as nn

from ... import ops
from ...packing import attach_cache, ln_params, pack_matrix
from .vit_common import Backbone

__all__ = ["SimpleFeaturePyramid", "LastLevelMaxPool"]


class _LN2d(nn.Module):
    """parameter holder for detectron2's channel LayerNorm (get_norm("LN"), eps 1e-6)"""

    def __init__(self, c, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.eps = eps


class _ConvLN(nn.Module):
    """detectron2 Conv2d(bias=False, norm=LN): holds weight [Cout,Cin,k,k] and norm.{weight,bias}"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        self.norm = _LN2d(cout)
        self.k = k


class LastLevelMaxPool(nn.Module):
    """detectron2 LastLevelMaxPool: p6 = p5[:, :, ::2, ::2] (max_pool2d kernel 1, stride 2)"""

    def __init__(self):
        super().__init__()
        self.num_levels = 1
        self.in_feature = "p5"


class SimpleFeaturePyramid(Backbone):
    def __init__(self, net, in_feature, out_channels, scale_factors, top_block=None, norm="LN", square_pad=0):
        super().__init__()
        assert tuple(scale_factors) == (4.0, 2.0, 1.0, 0.5) and norm == "LN", "ape_amd FPN: the ViTDet (4,2,1,0.5)/LN pyramid"
        self.scale_factors = scale_factors
        dim = net.embed_dim
        self.simfp_2 = nn.Sequential(nn.ConvTranspose2d(dim, dim // 2, 2, 2), _LN2d(dim // 2), nn.GELU(),
                                     nn.ConvTranspose2d(dim // 2, dim // 4, 2, 2), _ConvLN(dim // 4, out_channels, 1),
                                     _ConvLN(out_channels, out_channels, 3))
        self.simfp_3 = nn.Sequential(nn.ConvTranspose2d(dim, dim // 2, 2, 2), _ConvLN(dim // 2, out_channels, 1),
                                     _ConvLN(out_channels, out_channels, 3))
        self.simfp_4 = nn.Sequential(_ConvLN(dim, out_channels, 1), _ConvLN(out_channels, out_channels, 3))
        self.simfp_5 = nn.Sequential(nn.MaxPool2d(2, 2), _ConvLN(dim, out_channels, 1), _ConvLN(out_channels, out_channels, 3))
        self.net = net
        self.in_feature = in_feature
        self.top_block = top_block
        strides = [int(net.patch_size / s) for s in scale_factors]
        self._out_feature_strides = {f"p{int(math.log2(s))}": s for s in strides}
        if top_block is not None:
            last = int(math.log2(strides[-1]))
            self._out_feature_strides[f"p{last + 1}"] = 2 ** (last + 1)
        self._out_features = list(self._out_feature_strides.keys())
        self._out_feature_channels = {k: out_channels for k in self._out_features}
        self._size_divisibility = strides[-1]
        self._square_pad = square_pad
        self.out_channels = out_channels
        attach_cache(self)

    @property
    def padding_constraints(self):
        return {"size_divisiblity": self._size_divisibility, "square_size": self._square_pad}  # sic (vit_eva_clip.py:864-869)

    @property
    def compute_dtype(self):
        return self.net.compute_dtype

    @staticmethod
    def _deconv_matrix(m, dt):
        """ConvTranspose2d(k=2,s=2) weight [Cin,Cout,2,2] -> GEMM weight [(i*2+j)*Cout + co, ci], bias x4"""
        w = m.weight.detach().float()
        cin, cout = w.shape[0], w.shape[1]
        return pack_matrix(w.permute(2, 3, 1, 0).reshape(4 * cout, cin), dt), m.bias.detach().float().repeat(4).contiguous()

    @staticmethod
    def _conv_matrix(m, dt):
        """Conv2d weight [Cout,Cin,k,k] -> [Cout, (ky*k+kx)*Cin + ci] (matches ops.im2col3x3's column order)"""
        w = m.weight.detach().float()
        return pack_matrix(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), dt)

    def packed(self, dt):
        def build(dt):
            hw = self.net.img_size // self.net.patch_size
            dev = self.simfp_4[0].weight.device
            _, r2t = self.net.token_order(hw)          # vit_eva_clip: window-major, vit_eva02: raster
            r2t = r2t.long()
            # raster (Y,X) of the x2 / x4 maps -> row of the nested (token, i, j[, i2, j2]) layouts the deconv GEMMs produce
            Y2, X2 = torch.meshgrid(torch.arange(2 * hw), torch.arange(2 * hw), indexing="ij")
            p3 = (r2t[(Y2 // 2) * hw + X2 // 2] * 4 + (Y2 % 2) * 2 + X2 % 2).reshape(-1)
            Y4, X4 = torch.meshgrid(torch.arange(4 * hw), torch.arange(4 * hw), indexing="ij")
            p2 = ((r2t[(Y4 // 4) * hw + X4 // 4] * 4 + ((Y4 // 2) % 2) * 2 + (X4 // 2) % 2) * 4 + (Y4 % 2) * 2 + X4 % 2).reshape(-1)
            Y6, X6 = torch.meshgrid(torch.arange(0, hw // 2, 2), torch.arange(0, hw // 2, 2), indexing="ij")
            p6 = (Y6 * (hw // 2) + X6).reshape(-1)
            d = dict(hw=hw, perm4=r2t.to(torch.int32).to(dev), perm3=p3.to(torch.int32).to(dev), perm2=p2.to(torch.int32).to(dev),
                     idx6=p6.to(torch.int32).to(dev))
            d["s2_d0"] = self._deconv_matrix(self.simfp_2[0], dt)
            d["s2_ln"] = ln_params(self.simfp_2[1])
            d["s2_d1"] = self._deconv_matrix(self.simfp_2[3], dt)
            d["s3_d0"] = self._deconv_matrix(self.simfp_3[0], dt)
            for name, seq, i1, i3 in (("s2", self.simfp_2, 4, 5), ("s3", self.simfp_3, 1, 2), ("s4", self.simfp_4, 0, 1), ("s5", self.simfp_5, 1, 2)):
                d[name + "_c1"] = (self._conv_matrix(seq[i1], dt),) + ln_params(seq[i1].norm)
                d[name + "_c3"] = (self._conv_matrix(seq[i3], dt),) + ln_params(seq[i3].norm)
            return d
        return self._pack.get(self, dt, build)

    def _conv_ln_pair(self, x, perm, H, W, c1, c3, dt):
        """1x1 conv + LN (any row order), then 3x3 conv + LN through the gathering im2col -> raster [H*W, C]"""
        y = ops.layernorm(ops.gemm(x, c1[0], None), c1[1], c1[2], c1[3], out_dtype=dt)
        # large 256-channel maps (p2: 256 x 256 pixels): implicit GEMM, the im2col matrix (302 MB) is never written; else im2col + gemm
        return ops.layernorm(ops.conv3x3(y, perm, H, W, c3[0], None), c3[1], c3[2], c3[3], out_dtype=dt)

    def forward_tokens(self, image, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), vit_feat=None, stages=None):
        """-> dict name -> ([H*W, C] raster token-major map in the compute dtype, (H, W)).  vit_feat: this image's rows of a
        batched ViT pass (ViT.forward_tokens on a list) -- the pyramid then starts from them."""
        dt = self.compute_dtype
        P = self.packed(dt)
        hw = P["hw"]
        if vit_feat is not None:
            x = vit_feat
        elif stages is not None:
            x = self.net.forward_tokens(image, mean, std, stages=stages)
        else:
            x = self.net.forward_tokens(image, mean, std)                                             # [hw*hw, E] window-major
        out = {}
        # The four scales only share the ViT output: stride 8 / 16 / 32 run as parallel graph branches next to the heavy
        # stride-4 chain (their kernels are small launches that leave most of the chip idle).
        def s3():
            t = ops.gemm(x, P["s3_d0"][0], P["s3_d0"][1]).view(hw * hw * 4, -1)
            return self._conv_ln_pair(t, P["perm3"], 2 * hw, 2 * hw, P["s3_c1"], P["s3_c3"], dt)

        def s5():
            t = ops.maxpool2x2(x, P["perm4"], hw, hw)
            p5 = self._conv_ln_pair(t, None, hw // 2, hw // 2, P["s5_c1"], P["s5_c3"], dt)
            return p5, (ops.gather_rows(p5, P["idx6"]) if self.top_block is not None else None)

        j3 = ops.fork(s3)
        j4 = ops.fork(lambda: self._conv_ln_pair(x, P["perm4"], hw, hw, P["s4_c1"], P["s4_c3"], dt))
        j5 = ops.fork(s5)
        # stride 4: deconv -> LN -> GELU -> deconv -> 1x1+LN -> 3x3+LN   (rows stay in nested order until the im2col)
        t = ops.gemm(x, P["s2_d0"][0], P["s2_d0"][1])
        t = t.view(hw * hw * 4, -1)
        t = ops.layernorm(t, P["s2_ln"][0], P["s2_ln"][1], P["s2_ln"][2], out_dtype=dt, act=ops.ACT_GELU)
        t = ops.gemm(t, P["s2_d1"][0], P["s2_d1"][1]).view(hw * hw * 16, -1)
        out["p2"] = (self._conv_ln_pair(t, P["perm2"], 4 * hw, 4 * hw, P["s2_c1"], P["s2_c3"], dt), (4 * hw, 4 * hw))
        out["p3"] = (j3.join(), (2 * hw, 2 * hw))
        out["p4"] = (j4.join(), (hw, hw))
        p5, p6 = j5.join()
        out["p5"] = (p5, (hw // 2, hw // 2))
        if self.top_block is not None:
            out["p6"] = (p6, (hw // 4, hw // 4))
        return out

    def forward(self, x):
        """reference signature: NCHW batch -> {"p2".."p6": NCHW}"""
        res = {}
        for b in range(x.shape[0]):
            maps = self.forward_tokens(x[b].float().contiguous())
            for k, (t, (H, W)) in maps.items():
                res.setdefault(k, []).append(t.float().reshape(H, W, -1).permute(2, 0, 1))
        return {k: torch.stack(v) for k, v in res.items()}
