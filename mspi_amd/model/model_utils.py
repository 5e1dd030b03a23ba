"""Model assembly, multisensory fusion and decoder -- HIP-backed mirror of the reference's
model/model_utils.py (AudioVisualSaliencyModel :388-574, VisualSaliencyModel :576-702).

Sub-module names equal the reference's so that released MSPI checkpoints load with
`load_state_dict(strict=False)` (inference.py:186); torch layers hold parameters only and the
forward runs entirely on the C ABI (mspi_amd.engine).  Fusions applied here (all exact up to
fp32 rounding):
  * eval BatchNorm folded into the producing conv; bias/ReLU/GELU/sigmoid/residual in epilogues
  * every torch.cat replaced by producers writing into channel slices / token slabs
  * latlayer_k[0] (1x1x1) and latlayer_k[1] ((s,1,1) stride s), both linear with nothing in
    between, composed into one strided temporal conv (4x fewer rows, no 192-ch intermediate)
  * readout: the x4 trilinear up-sample is moved behind the (4,1,1)/4 temporal conv (both linear,
    bilinear weights sum to 1 so the bias commutes), ReLU applied in the up-sample epilogue
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import engine as E
from .._lib import MspiError
from ..autograd import Adapter as AdapterTrain
from ..autograd import (STAGE_NAMES, STAGES, SYNC_PREFIXES, ContrastHead, Fusion, LateralBlock, LateralEntry, ReadoutHead,
                        ReadoutTail, compose_lateral, convnext_block_forward, pack_convnext_block, pack_lateral_entry,
                        pack_readout_tail, r0_parts, reaches, readout_tail_forward, stage_rank, stages_upto, sync_block)
from ..backbones.convnext import ConvNeXtTinyFeatures
from ..backbones.resnet import get_resnet18
from ..module import HipModule, to_cl
from .get_video_backbones import video_motion_extractor


def get_sinusoid_encoding_table(n_position, d_hid):
    """Sinusoid position table [1, n_position, d_hid] (reference: model/model_utils.py:18-29)."""
    pos = np.arange(n_position, dtype=np.float64).reshape(-1, 1)
    hid = np.arange(d_hid).reshape(1, -1)
    ang = pos / np.power(10000, 2 * (hid // 2) / d_hid)
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return torch.tensor(ang, dtype=torch.float, requires_grad=False).unsqueeze(0)


def _f(t):
    return t.detach().float().contiguous()


# ------------------------------------------------------------------------------- SyncBlock
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(HipModule):
    """Pre-LN transformer block (model/model_utils.py:122-152): 7 launches."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = Attention(dim, num_heads=num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def _pack(self):
        a, m = self.attn, self.mlp
        return {"n1": (_f(self.norm1.weight), _f(self.norm1.bias)), "n2": (_f(self.norm2.weight), _f(self.norm2.bias)),
                "qkv": E.pack_conv(a.qkv.weight, a.qkv.bias), "proj": E.pack_conv(a.proj.weight, a.proj.bias),
                "fc1": E.pack_conv(m.fc1.weight, m.fc1.bias, act=E.ACT_GELU), "fc2": E.pack_conv(m.fc2.weight, m.fc2.bias)}

    def run(self, x, B, R):
        pk = self.pk
        dim = self.norm1.normalized_shape[0]
        h = E.layernorm_for_gemm(x, *pk["n1"], 1e-5, pk["qkv"])
        o = E.attention(E.conv(h, pk["qkv"]), B, R, self.attn.num_heads, dim // self.attn.num_heads, self.attn.scale,
                        slot=E.attn_slot(pk))
        x = E.conv(o, pk["proj"], res=x)
        return E.mlp_tail(x, ("split", pk["fc1"], pk["fc2"]), pk["n2"], 1e-5, res=x)

    def tensors(self):
        """The eleven tensors in the order of autograd.TransformerBlock's arguments (and of pack_transformer_block's)."""
        a, m = self.attn, self.mlp
        return (self.norm1.weight, self.norm1.bias, a.qkv.weight, a.proj.weight, a.proj.bias, self.norm2.weight, self.norm2.bias,
                m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)


class SyncBlock(HipModule):
    def __init__(self, num_blocks=3, num_vis_tokens=336, num_aud_tokens=36, vis_in_embed=1024, embed_dim=512):
        super().__init__()
        self.vis_pos_embed = get_sinusoid_encoding_table(num_vis_tokens, 512)
        self.aud_pos_embed = get_sinusoid_encoding_table(num_aud_tokens, 512)
        self.vis_proj = nn.Linear(vis_in_embed, 512)
        self.vis_norm = nn.LayerNorm(512)
        self.aud_norm = nn.LayerNorm(512)
        self.blocks = nn.ModuleList([Block(dim=embed_dim, num_heads=4) for _ in range(num_blocks)])
        for m in self.modules():  # model/model_utils.py:241-251
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def _pack(self):
        dev = self.vis_proj.weight.device
        return {"proj": E.pack_conv(self.vis_proj.weight, self.vis_proj.bias),
                "vn": (_f(self.vis_norm.weight), _f(self.vis_norm.bias)),
                "an": (_f(self.aud_norm.weight), _f(self.aud_norm.bias)),
                "vpos": self.vis_pos_embed[0].to(dev).contiguous(), "apos": self.aud_pos_embed[0].to(dev).contiguous()}

    def run(self, vis, aud):
        """vis CL [B,t,h,w,C4], aud CL [B,1,F,T',512] -> token slab CL [B, Rv+Ra, 1, 1, 512]."""
        pk = self.pk
        B, Rv, Ra = vis.N, vis.T * vis.H * vis.W, aud.T * aud.H * aud.W
        if Rv != pk["vpos"].shape[0] or Ra != pk["apos"].shape[0]:
            raise MspiError("SyncBlock: got %d visual / %d audio tokens but the positional tables hold %d / %d rows "
                            "-- set cfg.MODEL.NUM_VIS_TOKENS[name] / cfg.MODEL.NUM_AUD_TOKENS (reference: the add at "
                            "model/model_utils.py:273-274 fails the same way)" % (Rv, Ra, pk["vpos"].shape[0], pk["apos"].shape[0]))
        x = E.alloc(B, Rv + Ra, 1, 1, 512, vis.buf.device)
        E.layernorm(E.conv(vis, pk["proj"]), *pk["vn"], 1e-5, out=x.tokens(0, vis.T, vis.H, vis.W), table=pk["vpos"])
        E.layernorm(aud, *pk["an"], 1e-5, out=x.tokens(Rv, aud.T, aud.H, aud.W), table=pk["apos"])
        for blk in self.blocks:
            x = blk.run(x, B, Rv + Ra)
        return x

    def tensors(self):
        """The six embedding tensors in the order of autograd.SyncEmbed's arguments (the blocks' are Block.tensors())."""
        return (self.vis_proj.weight, self.vis_proj.bias, self.vis_norm.weight, self.vis_norm.bias, self.aud_norm.weight,
                self.aud_norm.bias)

    def forward(self, vis_fea, aud_fea):
        a = aud_fea[:, :, None] if aud_fea.dim() == 4 else aud_fea
        x = self.run(to_cl(vis_fea), to_cl(a))
        return x.as_rows().view(x.N, x.T, 512)


# ------------------------------------------------------------------------------- conv helpers (backbones/s3d.py:41-52,95-116)
class BasicConv3d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding=0):
        super().__init__()
        self.conv = nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm3d(out_planes, eps=1e-3, momentum=0.001, affine=True)
        self.relu = nn.ReLU()

    def packed(self):
        c = self.conv
        return E.pack_conv(c.weight, None, self.bn, c.stride, c.padding, E.ACT_RELU)


class SepConv3d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding=0):
        super().__init__()
        k, s, p = kernel_size, stride, padding
        self.conv_s = nn.Conv3d(in_planes, out_planes, (1, k, k), (1, s, s), (0, p, p), bias=False)
        self.bn_s = nn.BatchNorm3d(out_planes, eps=1e-3, momentum=0.001, affine=True)
        self.relu_s = nn.ReLU()
        self.conv_t = nn.Conv3d(out_planes, out_planes, (k, 1, 1), (s, 1, 1), (p, 0, 0), bias=False)
        self.bn_t = nn.BatchNorm3d(out_planes, eps=1e-3, momentum=0.001, affine=True)
        self.relu_t = nn.ReLU()

    def packed(self):
        cs, ct = self.conv_s, self.conv_t
        return (E.pack_conv(cs.weight, None, self.bn_s, cs.stride, cs.padding, E.ACT_RELU),
                E.pack_conv(ct.weight, None, self.bn_t, ct.stride, ct.padding, E.ACT_RELU))


class SA(HipModule):
    """x * sigmoid(conv(up(BasicConv3d(mask)))) + x (model/model_utils.py:155-170)."""

    def __init__(self, in_embed_dim=512, k=2):
        super().__init__()
        self.k = k
        self.up = nn.Upsample(scale_factor=(1, k, k), align_corners=False, mode="trilinear") if k != 1 else nn.Identity()
        self.conv_mask = nn.Sequential(
            BasicConv3d(in_embed_dim, in_embed_dim // 16, kernel_size=3, stride=1, padding=1),
            self.up,
            nn.Conv3d(in_embed_dim // 16, 1, kernel_size=(1, 3, 3), stride=1, padding=(0, 1, 1)),
            nn.Sigmoid(),
        )

    def tensors(self):
        """The five tensors in the order of autograd.Fusion's arguments and the BatchNorm buffer triple behind them."""
        b, c = self.conv_mask[0], self.conv_mask[2]
        return [b.conv.weight, b.bn.weight, b.bn.bias, c.weight, c.bias], (b.bn.running_mean, b.bn.running_var, b.bn.num_batches_tracked)

    def _pack(self):
        c = self.conv_mask[2]
        return self.conv_mask[0].packed(), E.pack_conv(c.weight, c.bias, None, (1, 1, 1), (0, 1, 1), E.ACT_SIGMOID)

    def run(self, x, mask, premask=None):
        """In place on x.  premask: this module's BasicConv3d output if the caller already computed it
        (the decoder runs the three SA modules' first convs, which share their input, as ONE conv)."""
        p0, p2 = self.pk
        m = E.conv(mask, p0) if premask is None else premask
        if self.k != 1:
            m = E.upsample(m, self.k)
        return E.rowgate(x, E.conv(m, p2))


class Inception(HipModule):
    def __init__(self, embed_dim=320 + 96):
        super().__init__()
        self.branch0 = nn.Sequential(BasicConv3d(embed_dim, 192, kernel_size=1, stride=1))
        self.branch1 = nn.Sequential(BasicConv3d(embed_dim, 96, kernel_size=1, stride=1),
                                     SepConv3d(96, 208, kernel_size=3, stride=1, padding=1))
        self.branch2 = nn.Sequential(BasicConv3d(embed_dim, 16, kernel_size=1, stride=1),
                                     SepConv3d(16, 48, kernel_size=3, stride=1, padding=1))
        self.branch3 = nn.Sequential(nn.MaxPool3d(kernel_size=(3, 3, 3), stride=1, padding=1),
                                     BasicConv3d(embed_dim, 64, kernel_size=1, stride=1))

    def _pack(self):
        return {"b0": self.branch0[0].packed(), "b1": (self.branch1[0].packed(),) + self.branch1[1].packed(),
                "b2": (self.branch2[0].packed(),) + self.branch2[1].packed(), "b3": self.branch3[1].packed()}

    def run(self, x):
        pk = self.pk
        out = E.alloc(x.N, x.T, x.H, x.W, 512, x.buf.device)
        E.conv(x, pk["b0"], out=out.slice(0, 192))
        E.conv(E.conv(E.conv(x, pk["b1"][0]), pk["b1"][1]), pk["b1"][2], out=out.slice(192, 208))
        E.conv(E.conv(E.conv(x, pk["b2"][0]), pk["b2"][1]), pk["b2"][2], out=out.slice(400, 48))
        E.conv(E.maxpool(x, (3, 3, 3), (1, 1, 1), (1, 1, 1)), pk["b3"], out=out.slice(448, 64))
        return out


class Adapter(HipModule):
    def __init__(self, embed_dim=320 + 96, num_frames=32, stride=8):
        super().__init__()
        self.num_frames = num_frames
        self.stride = stride
        self.pool_time = nn.MaxPool3d(kernel_size=(stride, 1, 1), stride=(stride, 1, 1))
        self.conv = Inception(embed_dim=embed_dim)
        self.up = nn.Upsample(scale_factor=(1, 2, 2), align_corners=False, mode="trilinear")

    def tensors(self):
        """The 24 tensors in the order of autograd.Adapter's arguments and the eight BatchNorm buffer triples behind them."""
        ts, bns = [], []
        for conv, bn in self.layers().values():
            ts += [conv.weight, bn.weight, bn.bias]
            bns.append((bn.running_mean, bn.running_var, bn.num_batches_tracked))
        return ts, bns

    def layers(self):
        """{name of the BatchNorm module below the adapter: (conv, bn)} in autograd.ADAPTER_LAYERS order."""
        c = self.conv
        b1, b2 = c.branch1, c.branch2
        return {"conv.branch0.0.bn": (c.branch0[0].conv, c.branch0[0].bn), "conv.branch1.0.bn": (b1[0].conv, b1[0].bn),
                "conv.branch1.1.bn_s": (b1[1].conv_s, b1[1].bn_s), "conv.branch1.1.bn_t": (b1[1].conv_t, b1[1].bn_t),
                "conv.branch2.0.bn": (b2[0].conv, b2[0].bn), "conv.branch2.1.bn_s": (b2[1].conv_s, b2[1].bn_s),
                "conv.branch2.1.bn_t": (b2[1].conv_t, b2[1].bn_t), "conv.branch3.1.bn": (c.branch3[1].conv, c.branch3[1].bn)}

    def run(self, o3, o2, features=False):
        """o3 CL [(b t),1,h,w,96], o2 CL [(b t),1,h/2,w/2,320] -> masks CL [B,T/stride,h,w,512]; features at the "adapter" stage
        stops in front of the Inception and returns its 416-wide input for autograd.Adapter."""
        T, s = self.num_frames, self.stride
        B = o3.N // T
        o3 = o3.reshape(B, T, o3.H, o3.W)
        o2 = o2.reshape(B, T, o2.H, o2.W)
        cat = E.alloc(B, T // s, o3.H, o3.W, o3.C + o2.C, o3.buf.device)
        E.maxpool(o3, (s, 1, 1), (s, 1, 1), (0, 0, 0), out=cat.slice(0, o3.C))
        E.upsample(E.maxpool(o2, (s, 1, 1), (s, 1, 1), (0, 0, 0)), 2, dst=cat.slice(o3.C, o2.C))
        return cat if reaches(features, "adapter") else self.conv.run(cat)


class LayerNorm3d(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)


class ConvNextBlock(HipModule):
    """dw(7,1,1) -> dw(1,7,7) -> channel LN -> 1x1x1 x4 + GELU -> 1x1x1 -> + input (model/model_utils.py:306-354)."""

    def __init__(self, dim, drop_path=0.0):
        super().__init__()
        self.dwconv_t = nn.Conv3d(dim, dim, kernel_size=(7, 1, 1), padding=(3, 0, 0), groups=dim)
        self.dwconv_s = nn.Conv3d(dim, dim, kernel_size=(1, 7, 7), padding=(0, 3, 3), groups=dim)
        self.norm = LayerNorm3d(dim)
        self.pwconv1 = nn.Conv3d(dim, 4 * dim, 1)
        self.act = nn.GELU()
        self.pwconv2 = nn.Conv3d(4 * dim, dim, 1)
        self.drop_path = nn.Identity()
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.constant_(m.bias, 0)

    def tensors(self):
        """The ten tensors in the order of autograd.LateralBlock's arguments (and of pack_convnext_block's)."""
        return (self.dwconv_t.weight, self.dwconv_t.bias, self.dwconv_s.weight, self.dwconv_s.bias, self.norm.norm.weight,
                self.norm.norm.bias, self.pwconv1.weight, self.pwconv1.bias, self.pwconv2.weight, self.pwconv2.bias)

    def _pack(self):
        return pack_convnext_block(*self.tensors())

    def run(self, x, out=None):
        return convnext_block_forward(x, self.pk, out=out)[0]


class StaticSaliencyModelConvNext(HipModule):
    """Per-frame ConvNeXt-T + two smoothing convs (model/model_utils.py:357-385)."""

    def __init__(self):
        super().__init__()
        self.encoder = ConvNeXtTinyFeatures()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)
        self.up4 = nn.Upsample(scale_factor=4, mode="bilinear", align_corners=False)
        self.up8 = nn.Upsample(scale_factor=8, mode="bilinear", align_corners=False)
        self.smooth_0 = nn.Sequential(nn.Conv2d(768, 320, 3, 1, 1), nn.BatchNorm2d(320), nn.ReLU())
        self.smooth_1 = nn.Sequential(nn.Conv2d(384, 96, 3, 1, 1), nn.BatchNorm2d(96), nn.ReLU())

    def _pack(self):
        return tuple(E.pack_conv(s[0].weight, s[0].bias, s[1], (1, 1, 1), (0, 1, 1), E.ACT_RELU)
                     for s in (self.smooth_0, self.smooth_1))

    def run(self, clips):
        s0, s1 = self.pk
        _, _, o1, o0 = self.encoder.forward_cl(clips)
        return E.conv(o1, s1), E.conv(o0, s0)

    def forward(self, x):
        o1, o0 = self.run(x)
        return o1.as_ncdhw().squeeze(2), o0.as_ncdhw().squeeze(2)


# ------------------------------------------------------------------------------- models
class _Fork:
    """Fork the current HIP stream into side streams for independent branches and join them on exit.
    MSPI_STREAMS=0 runs everything on the current stream."""
    ENABLED = os.environ.get("MSPI_STREAMS", "1") != "0"

    def __init__(self, owner, device):
        self.main = torch.cuda.current_stream(device)
        d = owner.__dict__
        if "_side_streams" not in d or d["_side_streams"][0].device != device:
            d["_side_streams"] = [torch.cuda.Stream(device) for _ in range(2)]
        self.side = d["_side_streams"]
        self.used = []
        self.kept = []

    def __enter__(self):
        self.start = torch.cuda.Event()
        self.start.record(self.main)
        return self

    def branch(self, i, refork=False):
        """Context manager that runs its body on side stream i.  refork=True: the branch starts from the main
        stream's CURRENT position (a second use of the stream, after an earlier join), not from the fork point."""
        if not self.ENABLED:
            return torch.cuda.stream(self.main)
        s = self.side[i]
        if refork:
            ev = torch.cuda.Event()
            ev.record(self.main)
            s.wait_event(ev)
        else:
            s.wait_event(self.start)
        if s not in self.used:
            self.used.append(s)
        return torch.cuda.stream(s)

    def keep(self, *objs):
        """Hold references until the join at exit: memory allocated on the main stream that a side-stream kernel reads
        would otherwise go back to the caching allocator when its last Python reference dies, and be handed to a later
        main-stream kernel while the side stream has not run yet."""
        self.kept.extend(objs)

    def join(self, i):
        """Make the main stream wait for branch i now (its results are needed before the others finish)."""
        s = self.side[i]
        if self.ENABLED and s in self.used:
            ev = torch.cuda.Event()
            ev.record(s)
            self.main.wait_event(ev)
            self.used.remove(s)

    def __exit__(self, *exc):
        for s in list(self.used):
            ev = torch.cuda.Event()
            ev.record(s)
            self.main.wait_event(ev)
        self.used = []
        self.kept = []
        return False


DECODER_FUSED = os.environ.get("MSPI_DECODER_FUSED", "1") != "0"   # A/B switch: r0 on the coarse maps, summed up-samples


def _compose_lateral(c0, c1):
    """The composed conv of two entry modules (autograd.compose_lateral)."""
    return compose_lateral(c0.weight, c0.bias, c1.weight)


class _SaliencyBase(HipModule):
    """Shared decoder: lateral layers, SA gating, top-down fusion, readout (model/model_utils.py:437-504,561-572)."""

    def _build_decoder(self, cfg, vis_embed_dims, extra_c4, de_embed_dim=192):
        d = de_embed_dim
        for k in range(4):
            cin = vis_embed_dims[k] + (extra_c4 if k == 3 else 0)
            layers = [nn.Conv3d(cin, d, 1, 1, 0)]
            if cfg.MODEL.LATERAL_BOOL[k]:
                s = cfg.MODEL.LATERAL_STRIDE[k]
                layers.append(nn.Conv3d(d, d, kernel_size=(s, 1, 1), stride=(s, 1, 1), bias=False))
            layers.append(ConvNextBlock(dim=d))
            setattr(self, "latlayer_%d" % k, nn.Sequential(*layers))
        self.upsample = nn.Upsample(scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
        self.upsample_4 = nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False)
        self.upsample_8 = nn.Upsample(scale_factor=(1, 8, 8), mode="trilinear", align_corners=False)
        self.readout = nn.Sequential(
            nn.Conv3d(d * 4, d, 1, 1, 0),
            nn.Conv3d(d, d, kernel_size=3, stride=1, padding=1),
            nn.BatchNorm3d(d),
            nn.ReLU(inplace=True),
            nn.Conv3d(d, 64, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
            nn.BatchNorm3d(64),
            nn.ReLU(inplace=True),
            nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False),
            nn.Conv3d(64, 32, kernel_size=(4, 1, 1), stride=(4, 1, 1), padding=0),
            nn.ReLU(inplace=True),
            nn.Conv3d(32, 32, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
            nn.ReLU(inplace=True),
            nn.Conv3d(32, 1, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
        )
        self.adapter = Adapter(num_frames=cfg.DATA.NUM_FRAMES, stride=cfg.DATA.NUM_FRAMES // 4)
        self.sa_0 = SA(512, k=4)
        self.sa_1 = SA(512, k=2)
        self.sa_2 = SA(512, k=1)

    def _pack_lateral(self, k, split=None):
        """Packed entry conv(s) of latlayer_k.  split = C4: the input arrives as two tensors
        (v4 | vis_sync, the torch.cat of model/model_utils.py:559), so the K range is cut in two."""
        seq = getattr(self, "latlayer_%d" % k)
        if len(seq) == 3:
            return pack_lateral_entry(seq[0].weight, seq[0].bias, seq[1].weight, tuple(seq[1].stride), split)
        return pack_lateral_entry(seq[0].weight, seq[0].bias, None, (1, 1, 1), split)

    def _pack_decoder(self, split=None):
        r = self.readout
        return {
            "sa_cat": self._pack_sa_cat(),
            "lat": [self._pack_lateral(k, split if k == 3 else None) for k in range(4)],
            "r0": E.pack_conv(r[0].weight, r[0].bias),
            "r0_parts": self._pack_r0_parts(r[0]),
            "r1": E.pack_conv(r[1].weight, r[1].bias, r[2], (1, 1, 1), (1, 1, 1), E.ACT_RELU),
            "r4": E.pack_conv(r[4].weight, r[4].bias, r[5], (1, 1, 1), (0, 1, 1), E.ACT_RELU),
            "r8": E.pack_conv(r[8].weight, r[8].bias, None, (4, 1, 1), (0, 0, 0), E.ACT_NONE),
            "r10": E.pack_conv(r[10].weight, r[10].bias, None, (1, 1, 1), (0, 1, 1), E.ACT_RELU),
            "r12": E.pack_conv(r[12].weight, r[12].bias, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE),
            "tail_key": self._tail_key(),
            "head_key": self._head_key(),
            "sa_key": self._sa_key(),
        }

    def _pack_sa_cat(self):
        """sa_0/1/2.conv_mask[0] are three 3x3x3 convs 512->32 over the SAME masks tensor: one conv 512->96."""
        sa_w, sa_b = zip(*[E.fold_bn(m.conv_mask[0].conv.weight, None, m.conv_mask[0].bn) for m in (self.sa_0, self.sa_1, self.sa_2)])
        return E.pack_conv(torch.cat(sa_w, 0), torch.cat(sa_b, 0), None, (1, 1, 1), (1, 1, 1), E.ACT_RELU)

    _r0_parts = staticmethod(r0_parts)      # the split of readout[0] over the coarse maps (autograd.r0_parts)

    def _pack_r0_parts(self, conv):
        return [E.pack_conv(w, b) for w, b in self._r0_parts(conv.weight, conv.bias)]

    def _lateral(self, pk, k, xs, out=None, features=False):
        """latlayer_k: the entry conv(s), then the ConvNextBlock -- left to autograd.LateralBlock from the "lateral_blocks" stage
        on; from "lateral_entries" on it stops in front of the entry conv(s) and returns the encoder map(s) for
        autograd.LateralEntry, split planes joined into fp32 rows."""
        if reaches(features, "lateral_entries"):
            return [E.join_planes(x) if isinstance(x, E.SP) else x for x in xs]
        y = E.conv(xs[0], pk["lat"][k][0])
        if len(xs) == 2:
            y = E.conv(xs[1], pk["lat"][k][1], res=y)
        if reaches(features, "lateral_blocks"):
            return y
        return getattr(self, "latlayer_%d" % k)[-1].run(y, out=out)

    def _laterals_012(self, pk, v1, v2, v3, features=False):
        """latlayer_0..2 need only the motion encoder's first three maps: they run while the image branch is still busy.
        MSPI_DECODER_FUSED=0: s0 is produced straight into its channel slice of the readout's 768-channel input."""
        if DECODER_FUSED:
            return (None,) + tuple(self._lateral(pk, k, [v], features=features) for k, v in enumerate((v1, v2, v3)))
        B = v1.N
        cat = E.alloc(B, max(1, v1.T // (self.cfg.MODEL.LATERAL_STRIDE[0] if self.cfg.MODEL.LATERAL_BOOL[0] else 1)),
                      v1.H, v1.W, 4 * 192, v1.buf.device)
        s0 = self._lateral(pk, 0, [v1], out=cat.slice(0, 192))
        return cat, s0, self._lateral(pk, 1, [v2]), self._lateral(pk, 2, [v3])

    @torch.no_grad()
    def encode_frames(self, frames):
        """Per-frame half of the image branch (ConvNeXt-T + the two smoothing convs, model/model_utils.py:357-385) for
        frames [N,3,H,W]: (f1 [N,h,w,96], f0 [N,h/2,w/2,320]) dense fp32 tensors.  Nothing in it mixes frames, so a
        frame's features are the same in every window that contains it: cache them and pass them to
        forward(..., frame_feats=...) -- the clip loop of inference.py does."""
        self._check_eval()
        with self.plans_checked():
            o1, o0 = self.image_encoder.run(frames.float()[:, :, None])
        return (o1.buf.view(o1.N, o1.H, o1.W, o1.ld)[..., :o1.C], o0.buf.view(o0.N, o0.H, o0.W, o0.ld)[..., :o0.C])

    @staticmethod
    def _wrap_frame_feats(frame_feats):
        outs = []
        for f in frame_feats:
            f = f.float().contiguous()
            n, h, w, c = f.shape
            outs.append(E.CL(f.view(-1), 0, n, 1, h, w, c, c))
        return outs

    def _premask(self, pk, masks):
        """The three SA modules' first convs (same input) as one 512->96 conv."""
        self._refresh_sa(pk)
        return E.conv(masks, pk["sa_cat"])

    def _fuse_readout(self, pk, cat, s0, s1, s2, s3, masks, pm, features=False):
        """SA gating, top-down fusion and readout (model/model_utils.py:566-572); features=True stops in front of readout[8]
        and returns y4 [B,4,h,w,64]; "maps" stops in front of readout[0]; "laterals" in front of the gating (pm is None then);
        "entries" likewise, s0..s3 then being the entry convs' outputs (_lateral); "inputs" likewise, s0..s3 being the lists of
        encoder maps the entry convs read."""
        if reaches(features, "fusion"):
            # trainable("adapter"): as "inputs", and masks is the Inception's input, for autograd.Adapter;
            # trainable("fusion"): autograd.Fusion takes over from here, then ReadoutHead; trainable("lateral_blocks"): s0..s3
            # are the entry convs' outputs, and autograd.LateralBlock comes first; trainable("lateral_entries"): the entry
            # convs' inputs, and autograd.LateralEntry comes before that
            return s0, s1, s2, s3, masks
        if not reaches(features, "readout"):      # "maps": ReadoutHead packs the live values itself
            self._refresh_head(pk)
        self.sa_2.run(s2, masks, pm.slice(64, 32))
        E.upsample(s3, 2, dst=s2, accumulate=True)
        self.sa_1.run(s1, masks, pm.slice(32, 32))
        if cat is None:
            # r0 on the coarse maps, up-sampled after it (_r0_parts): neither s0' nor the 768-channel concat is materialised
            E.upsample_sum(s1, [(s2, 2), (s3, 4)])
            self.sa_0.run(s0, masks, pm.slice(0, 32))
            if reaches(features, "readout"):      # trainable("readout"): autograd.ReadoutHead takes over from here
                return s0, s1, s2, s3
            p0, p1, p2, p3 = pk["r0_parts"]
            y = E.conv(s0, p0)
            E.upsample_sum(y, [(E.conv(s1, p1), 2), (E.conv(s2, p2), 4), (E.conv(s3, p3), 8)])
        else:
            E.upsample(s2, 2, dst=s1, accumulate=True)
            E.upsample(s3, 4, dst=s1, accumulate=True)
            self.sa_0.run(s0, masks, pm.slice(0, 32))
            E.upsample(s1, 2, dst=s0, accumulate=True)
            E.upsample(s2, 4, dst=s0, accumulate=True)
            E.upsample(s3, 8, dst=s0, accumulate=True)
            E.upsample(s1, 2, dst=cat.slice(192, 192))
            E.upsample(s2, 4, dst=cat.slice(384, 192))
            E.upsample(s3, 8, dst=cat.slice(576, 192))
            y = E.conv(cat, pk["r0"])
        y4 = E.conv(E.conv(y, pk["r1"]), pk["r4"])
        return y4 if features else self._readout_tail(pk, y4)

    def _readout_tail(self, pk, y4):
        """readout[8], [10], [12] and the log-softmax on y4 [B,4,h,w,64]: four launches (autograd.readout_tail_forward; the
        trainable form of the same launches is autograd.ReadoutTail)."""
        self._refresh_tail(pk)
        return readout_tail_forward(y4, pk["r8"], pk["r10"], pk["r12"])[0]

    # The readout and the SA gates train (trainable()), so an optimiser moves them at every step: their packs follow the three
    # keys below and are replaced one group at a time, and the plan's own key (module.HipModule.pk) leaves their tensors out --
    # a step must not rebuild the laterals.  (The SA modules' own plans follow their own subtree keys.)
    _PK_SELF_KEYED = ("readout", "sa_0", "sa_1", "sa_2")

    def _refresh_sa(self, pk):
        key = self._sa_key()
        if pk["sa_key"] != key:        # an optimiser step, a training forward (running statistics) or a load has moved the SA fold
            pk["sa_cat"] = self._pack_sa_cat()
            pk["sa_key"] = key

    def _refresh_head(self, pk):
        key = self._head_key()
        if pk["head_key"] != key:      # an optimiser step or a load has moved readout[0..5] since the four were packed
            r = self.readout
            pk["r0"], pk["r0_parts"] = E.pack_conv(r[0].weight, r[0].bias), self._pack_r0_parts(r[0])
            pk["r1"] = E.pack_conv(r[1].weight, r[1].bias, r[2], (1, 1, 1), (1, 1, 1), E.ACT_RELU)
            pk["r4"] = E.pack_conv(r[4].weight, r[4].bias, r[5], (1, 1, 1), (0, 1, 1), E.ACT_RELU)
            pk["head_key"] = key

    def _refresh_tail(self, pk):
        key = self._tail_key()
        if pk["tail_key"] != key:      # an optimiser has moved the tail in place since the three were packed
            r = self.readout
            pk["r8"], pk["r10"], pk["r12"] = pack_readout_tail(r[8].weight, r[8].bias, r[10].weight, r[10].bias,
                                                               r[12].weight, r[12].bias)
            pk["tail_key"] = key

    def _pk_refresh(self, pk):
        """What a `pk` access outside a forward sees: the readout's packs and the SA fold at the present values, as the forward
        would make them.  In a forward that carries a graph the head is left alone (ReadoutHead packs the live values itself)"""
        grad_tail = self._training_tail()
        if [p for p, _ in self._sa_key()] != [p for p, _ in pk["sa_key"]]:
            # an SA tensor lies in other storage than at pack time (.to(), .double().float() on the sub-module): not a training
            # step, which writes in place.  As for any other sub-module, the whole plan is built again (`pk` packs when it is gone)
            self.__dict__.pop("_pk", None)
            return
        with torch.no_grad():
            if not reaches(grad_tail, "fusion"):       # ... autograd.Fusion for the SA fold, whose premask that forward does not launch
                self._refresh_sa(pk)
            if not reaches(grad_tail, "readout"):
                self._refresh_head(pk)
            if not grad_tail:          # ... and ReadoutTail does the same for the tail
                self._refresh_tail(pk)

    def _tail_key(self):
        """Identity and in-place version of the six tail tensors: what the packs r8, r10, r12 were built from."""
        r = self.readout
        # _version is torch's private in-place counter, the only record of optimiser steps and of load_state_dict (both write
        # in place and keep data_ptr); an assignment `p.data = ...` need not bump it but moves data_ptr, which is why the key holds that too
        return tuple((p.data_ptr(), p._version) for i in (8, 10, 12) for p in (r[i].weight, r[i].bias))

    def _head_key(self):
        """The same for what r0, r0_parts, r1 and r4 were built from: the weights and biases of readout[0], [1], [4] and the
        affine parameters and running statistics of the two BatchNorm layers folded into r1 and r4."""
        r = self.readout
        ts = [t for i in (0, 1, 4) for t in (r[i].weight, r[i].bias)]
        ts += [t for i in (2, 5) for t in (r[i].weight, r[i].bias, r[i].running_mean, r[i].running_var)]
        return tuple((t.data_ptr(), t._version) for t in ts)

    def _sa_key(self):
        """The same for what sa_cat was built from: the first conv of each SA module and the affine parameters and running
        statistics of the BatchNorm folded into it."""
        ts = []
        for m in (self.sa_0, self.sa_1, self.sa_2):
            b = m.conv_mask[0]
            ts += [b.conv.weight, b.bn.weight, b.bn.bias, b.bn.running_mean, b.bn.running_var]
        return tuple((t.data_ptr(), t._version) for t in ts)

    TAIL_PARAMS = STAGES[0].params

    def trainable(self, what, sync=False):
        """trainable("adapter"): on top of what "lateral_entries" trains, the adapter's Inception -- the eight conv -> BatchNorm3d
        -> ReLU layers of adapter.conv, 24 more tensors: 107 in all with the all-composed encoders, 105 with s3d, 103 with
        slowfast.  A forward with grad enabled stops the image branch IN FRONT of the Inception and hands its 416-wide input to
        autograd.Adapter (the eight layers on BATCH statistics, 13 such layers in all), whose masks carry a graph into
        autograd.Fusion, which then returns their gradient.  That input gets no gradient.  Still frozen: the SyncBlock, the
        contrastive projectors and every encoder.
        trainable("lateral_entries"): on top of what "lateral_blocks" trains, the laterals' entry convs -- latlayer_k[0]
        (1x1x1, weight and bias) and, where cfg.MODEL.LATERAL_BOOL[k] is set, latlayer_k[1] ((s,1,1) / stride (s,1,1), weight):
        12 more tensors with the all-composed encoders (83 in all), 10 with s3d (81), 8 with slowfast (79).  A forward with grad
        enabled stops each lateral IN FRONT of its entry conv(s) and hands the encoder maps to autograd.LateralEntry, then to
        autograd.LateralBlock, Fusion, ReadoutHead and ReadoutTail; the same five BatchNorm layers run on batch statistics.  The
        entry convs' inputs get no gradient: the adapter, the masks' gradient, the SyncBlock and every encoder stay frozen.
        trainable("lateral_blocks"): on top of what "fusion" trains, the ConvNextBlock at the end of each lateral -- the 40
        tensors of latlayer_k[-1] (dwconv_t, dwconv_s, norm.norm, pwconv1, pwconv2; weight and bias each), 71 in all.  A forward
        with grad enabled stops each lateral behind its entry conv and hands the four entry outputs to autograd.LateralBlock,
        then to autograd.Fusion, ReadoutHead and ReadoutTail.  The entry convs latlayer_k[0] / [1], the adapter, the SyncBlock
        and every encoder stay frozen.
        trainable("fusion"): the SA gates and the whole readout train -- the 15 tensors of sa_0, sa_1, sa_2 and the readout's
        16 get requires_grad; a forward with grad enabled runs the encoders, the adapter and the laterals as in inference and
        hands the four lateral outputs and the adapter's masks to autograd.Fusion (the three gates with their BatchNorm on BATCH
        statistics, the top-down sums), then to autograd.ReadoutHead and autograd.ReadoutTail.  The laterals, the adapter and
        every encoder stay frozen.
        trainable("readout"): the whole readout Sequential trains -- all 16 of its tensors get requires_grad, a forward with
        grad enabled computes the four fused pyramid maps as in inference and hands them to autograd.ReadoutHead (readout[0],
        [1], [4] with readout[2] and [5] on BATCH statistics, which frozen_encoder() puts in train()) and then to
        autograd.ReadoutTail.  SA gating, the laterals, the fusion and every encoder stay frozen.
        trainable("readout_tail"): the three convs readout[8], readout[10], readout[12] become trainable on top of a frozen
        network -- every other parameter gets requires_grad_(False), and a forward with grad enabled computes the features in
        front of readout[8] as in inference (eval BatchNorm, folded) and hands them to autograd.ReadoutTail.
        trainable(None) switches back and restores the flags found at switch-on.  Off by default.
        sync=True, a switch BESIDE the ladder (the six stages stay six): on top of the stage's tensors the SyncBlock and the
        contrastive head train -- the 39 tensors of aud_vis_sync_block, the 12 each of vis_projector and aud_projector and the 6
        each of mlp_vis and mlp_aud, 75 more: 182 in all on "adapter" with the all-composed encoders (180 with s3d, 178 with
        slowfast), 158 on "lateral_entries".  Accepted only on AudioVisualSaliencyModel and only where `what` reaches
        "lateral_entries": the SyncBlock's only path to the map is latlayer_3's entry conv; anything else is refused by name.
        A forward with grad enabled then launches neither SyncBlock.run nor the contrastive side branch: v4 and the audio map
        go, as fp32 rows, to autograd.sync_block, whose slab hands its visual tokens to autograd.LateralEntry as x2 (which
        returns their gradient) and the whole of itself to autograd.ContrastHead, and forward returns (map, loss_av), BOTH
        carrying a graph -- engine_train.train_one_epoch's gamma * aux then trains the 36 tensors of the head, which nothing
        else reaches.  v4 and the audio map get no gradient: the three encoders stay frozen.  All added modules are LayerNorm
        and Linear, so none gains a mode.  Under torch.no_grad(), or without the keyword, nothing changes."""
        d = self.__dict__
        if sync:
            if not hasattr(self, "aud_vis_sync_block"):
                raise MspiError("trainable(%r, sync=True): %s has neither a SyncBlock nor a contrastive head; sync=True is for "
                                "AudioVisualSaliencyModel" % (what, type(self).__name__))
            if what is None or (what in STAGE_NAMES and not reaches(what, "lateral_entries")):
                raise MspiError("trainable(%r, sync=True): the SyncBlock reaches the map only through latlayer_3's entry conv, so "
                                "sync=True needs a stage that trains it: %s" % (what, " or ".join(repr(n) for n in STAGE_NAMES[4:])))
        if what is None:
            for p, flag in d.pop("_trainable_saved", []):
                p.requires_grad_(flag)
            d["_trainable"] = None
            d["_trainable_sync"] = False
            return self
        if what not in STAGE_NAMES:
            raise MspiError("trainable: %r is not a trainable part of this model (only %s and %r are)"
                            % (what, ", ".join(repr(n) for n in STAGE_NAMES[:-1]), STAGE_NAMES[-1]))
        if reaches(what, "readout") and not DECODER_FUSED:
            raise MspiError("trainable(%r) needs the fused decoder path: it is switched off by MSPI_DECODER_FUSED=0" % (what,))
        if d.get("_trainable") is None:
            d["_trainable_saved"] = [(p, p.requires_grad) for p in self.parameters()]
        d["_trainable"] = what
        d["_trainable_sync"] = bool(sync)
        prefixes = tuple(p.format(k=k, last=len(getattr(self, "latlayer_%d" % k)) - 1)
                         for st in stages_upto(what) for p in st.params for k in range(4)) + (SYNC_PREFIXES if sync else ())
        for name, p in self.named_parameters():
            p.requires_grad_(name.startswith(prefixes))
        return self

    def _batch_stat_modules(self):
        """{name: module} of the BatchNorm layers that run on batch statistics under the present switch."""
        return {n: self.get_submodule(n) for st in stages_upto(self.__dict__.get("_trainable")) for n in st.batch_stat}

    def _training_tail(self):
        """What _forward stops at when this forward carries a graph: True (the features y4, for autograd.ReadoutTail), "maps"
        (the four pyramid maps, for autograd.ReadoutHead and then ReadoutTail), "laterals" (the lateral outputs and the masks,
        for autograd.Fusion in front of those two), "entries" (the laterals' entry-conv outputs and the masks, for
        autograd.LateralBlock in front of those three), "inputs" (the encoder maps the entry convs read and the masks, for
        autograd.LateralEntry in front of those four), "cat" (the same with the Inception's input in the place of the masks, for
        autograd.Adapter beside those) or False."""
        what = self.__dict__.get("_trainable")
        return STAGES[stage_rank(what)].stop if what is not None and torch.is_grad_enabled() else False

    def _check_eval(self):
        """The forward's guard.  Under trainable("readout") exactly readout[2] and readout[5] may be in train() (they run on
        batch statistics in autograd.ReadoutHead), under trainable("fusion") also the three conv_mask[0].bn (autograd.Fusion);
        under trainable("lateral_blocks") and trainable("lateral_entries") the same five; any other module in train() is refused by name, as the model itself is."""
        super()._check_eval()
        what = self.__dict__.get("_trainable")
        if not reaches(what, "readout"):
            return
        allowed = {id(m) for m in self._batch_stat_modules().values()}
        for name, mod in self.named_modules():
            if mod.training and id(mod) not in allowed:
                raise MspiError("%s.%s is in train() mode: under trainable('%s') %s; call frozen_encoder()"
                                % (type(self).__name__, name, what, STAGES[stage_rank(what)].only))

    def _frozen_eval(self):
        """frozen_encoder() under a trainable switch: eval() everywhere (folded BatchNorm), except that the readout's two
        BatchNorm layers run on batch statistics when the whole readout trains.  True when a switch is on."""
        what = self.__dict__.get("_trainable")
        if what is None:
            return False
        self.eval()
        for mod in self._batch_stat_modules().values():
            mod.train()
        return True

    def _tail_with_grad(self, y):
        """The rest of a forward that carries a graph, from what _forward stopped at (_training_tail) to the map: the stages'
        autograd Functions on the live tensors, lowest part of the network first.  Returns (map, loss_av): loss_av carries the
        graph of autograd.ContrastHead under trainable(..., sync=True) and is None otherwise."""
        what = self.__dict__.get("_trainable")
        r = self.readout
        loss_av = None
        if reaches(what, "fusion"):
            idle = [n for n, m in self._batch_stat_modules().items() if not m.training]
            if idle:
                raise MspiError("trainable('%s'): a forward with grad runs %s on batch statistics, but in eval() mode the "
                                "no_grad forward folds the running ones; call frozen_encoder() (engine_train.train_one_epoch does)"
                                % (what, ", ".join(idle)))
            lats, m = list(y[:4]), y[4].as_nthwc()
            seqs = [getattr(self, "latlayer_%d" % k) for k in range(4)]
            if reaches(what, "lateral_entries"):      # the encoder maps: the entry convs run here and their outputs carry a graph
                lats = [[x.as_nthwc() for x in xs] for xs in lats]
                if self.__dict__.get("_trainable_sync"):
                    # lats[3] is (v4, the audio map): the SyncBlock runs here, its slab carries a graph over the 39 tensors,
                    # its visual tokens are latlayer_3's second input and the whole of it the contrastive head's
                    v4, aud = lats[3]
                    slab = sync_block(self.aud_vis_sync_block, v4, aud)
                    Rv = v4.shape[1] * v4.shape[2] * v4.shape[3]
                    lats[3] = [v4, slab[:, :Rv].view(v4.shape[:4] + (slab.shape[2],))]
                    loss_av = ContrastHead.apply(slab, Rv, *self._contrast_tensors())
                lats = [LateralEntry.apply(xs[0], xs[1] if len(xs) == 2 else None, seq[0].weight, seq[0].bias,
                                           seq[1].weight if len(seq) == 3 else None) for xs, seq in zip(lats, seqs)]
            else:
                lats = [s.as_nthwc() for s in lats]
            if reaches(what, "lateral_blocks"):       # the entry convs' outputs: the four ConvNextBlocks
                lats = [LateralBlock.apply(t, *seq[-1].tensors()) for t, seq in zip(lats, seqs)]
            if reaches(what, "adapter"):              # the Inception's input: its eight layers, and the masks carry a graph
                ts, bns = self.adapter.tensors()
                m = AdapterTrain.apply(m, *ts, *bns)
            sa, bns = zip(*[g.tensors() for g in (self.sa_0, self.sa_1, self.sa_2)])
            y = Fusion.apply(*lats, m, *sum(sa, []), *bns)      # hands ReadoutHead maps that carry a graph
        if reaches(what, "readout"):
            if not (r[2].training and r[5].training):
                # ReadoutHead normalises with BATCH statistics whatever the modules' mode; in eval() the no_grad forward of the
                # same model folds the RUNNING statistics, so the two maps would differ silently
                raise MspiError("trainable('readout'): a forward with grad runs readout.2 and readout.5 on batch statistics, "
                                "but they are in eval() mode; call frozen_encoder() (engine_train.train_one_epoch does)")
            ts, bns = self._head_tensors()
            y = ReadoutHead.apply(*[s if torch.is_tensor(s) else s.as_nthwc() for s in y], *ts, *bns)
        else:
            y = y.as_nthwc()
        return ReadoutTail.apply(y, *[self.get_parameter(n) for n in self.TAIL_PARAMS]), loss_av

    def _head_tensors(self):
        """The ten tensors of readout[0], [1], [2], [4], [5] in the order of autograd.ReadoutHead's arguments and the two BatchNorm
        buffer triples behind them."""
        r = self.readout
        return ([t for i in (0, 1, 2, 4, 5) for t in (r[i].weight, r[i].bias)],
                [(r[i].running_mean, r[i].running_var, r[i].num_batches_tracked) for i in (2, 5)])

    def _try_load(self, module_loader, path, what):
        if os.path.exists(path):
            module_loader(path)
        else:
            print("[mspi_amd] %s not found at %s: keeping random initialisation" % (what, path))

    def _pack_clips(self, clips):
        name = self.cfg.MODEL.MOTION_ENCODER
        if name == "slowfast4x16":  # model/model_utils.py:521-524: slow pathway = frames 0, 4, 12, last
            return [torch.stack([clips[:, :, 0], clips[:, :, 4], clips[:, :, 12], clips[:, :, -1]], dim=2), clips]
        if "swin" in name or "morph" in name or name == "s3d":
            return clips
        return [clips]


class AudioVisualSaliencyModel(_SaliencyBase):
    """forward(clips [B,3,T,H,W], audios [B,1,257,Wa]) -> (log-probability map [B,H,W], loss_av scalar)."""

    def __init__(self, cfg, vis_embed_dims=(96, 192, 384, 768), aud_embed_dim=512, de_embed_dim=192,
                 num_vis_tokens=4 * 7 * 7, norm=nn.LayerNorm):
        super().__init__()
        print("Motion Encoder is {}.".format(cfg.MODEL.MOTION_ENCODER))
        self.cfg = cfg
        vis_embed_dims = cfg.MODEL.MOTION_ENCODER_EMBEDS[cfg.MODEL.MOTION_ENCODER]
        num_vis_tokens = cfg.MODEL.NUM_VIS_TOKENS[cfg.MODEL.MOTION_ENCODER]
        self.audnet = get_resnet18(pretrained=False)
        self.image_encoder = StaticSaliencyModelConvNext()
        self.visnet = video_motion_extractor(cfg)
        self.aud_vis_sync_block = SyncBlock(num_blocks=3, num_vis_tokens=num_vis_tokens,
                                            num_aud_tokens=cfg.MODEL.get("NUM_AUD_TOKENS", 36),
                                            vis_in_embed=vis_embed_dims[-1], embed_dim=aud_embed_dim)
        self.aud_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.vis_pool = nn.AdaptiveAvgPool3d((1, 1, 1))
        h = 2048

        def projector():
            return nn.Sequential(nn.Linear(aud_embed_dim, h), norm(h), nn.ReLU(inplace=True), nn.Linear(h, h), norm(h),
                                 nn.ReLU(inplace=True), nn.Linear(h, h), norm(h))

        def predictor():
            return nn.Sequential(nn.Linear(h, 512), norm(512), nn.ReLU(), nn.Linear(512, h))

        self.vis_projector = projector()
        self.mlp_vis = predictor()
        self.aud_projector = projector()
        self.mlp_aud = predictor()
        self._build_decoder(cfg, vis_embed_dims, aud_embed_dim, de_embed_dim)
        # pretrained weights (model/model_utils.py:512-514); absent files keep the random init
        self._try_load(self.visnet.load_weight, cfg.MODEL.MOTION_ENCODER_WEIGHT, "motion encoder weights")
        self._try_load(lambda p: self.audnet.load_state_dict(torch.load(p, map_location="cpu")),
                       cfg.MODEL.AUDIO_ENCODER_WEIGHT, "audio encoder weights")
        self._try_load(lambda p: self.image_encoder.load_state_dict(torch.load(p, map_location="cpu"), strict=False),
                       cfg.MODEL.IMAGE_SALIENCY_ENCODER_WEIGHT, "image saliency encoder weights")

    def frozen_encoder(self):
        if self._frozen_eval():      # frozen means folded eval BatchNorm everywhere; the tail has neither BatchNorm nor dropout
            return
        self.audnet.eval()
        self.image_encoder.eval()

    def _pack(self):
        c4 = self.cfg.MODEL.MOTION_ENCODER_EMBEDS[self.cfg.MODEL.MOTION_ENCODER][-1]
        pk = self._pack_decoder(split=c4)

        def lin_ln(lin, ln):
            return E.pack_conv(lin.weight, lin.bias), _f(ln.weight), _f(ln.bias)

        for name in ("vis", "aud"):
            pr = getattr(self, name + "_projector")
            ml = getattr(self, "mlp_" + name)
            pk[name] = [lin_ln(pr[0], pr[1]), lin_ln(pr[3], pr[4]), lin_ln(pr[6], pr[7]), lin_ln(ml[0], ml[1]),
                        E.pack_conv(ml[3].weight, ml[3].bias)]
        return pk

    @staticmethod
    def _embed(p, x):
        """projector (Linear-LN-ReLU x2, Linear-LN) then predictor (Linear-LN-ReLU, Linear) on [B,512] rows."""
        for i, act in ((0, E.ACT_RELU), (1, E.ACT_RELU), (2, E.ACT_NONE)):
            x = E.layernorm(E.conv(x, p[i][0]), p[i][1], p[i][2], 1e-5, act=act)
        emb = x
        y = E.layernorm(E.conv(emb, p[3][0]), p[3][1], p[3][2], 1e-5, act=E.ACT_RELU)
        return emb, E.conv(y, p[4])

    def _contrast_tensors(self):
        """The 36 tensors of vis_projector, mlp_vis, aud_projector and mlp_aud, each in module order: autograd.ContrastHead's
        arguments."""
        return [t for m in (self.vis_projector, self.mlp_vis, self.aud_projector, self.mlp_aud) for t in m.parameters()]

    def forward(self, clips, audios, frame_feats=None):
        """frame_feats: optional (f1 [B*T,h,w,96], f0 [B*T,h/2,w/2,320]) from encode_frames() for the clips' frames in
        (b t) order -- the image branch then starts at the adapter (sliding-window inference re-uses 15 of 16 frames).
        After trainable("readout_tail") or trainable("readout") and with grad enabled, the map carries the graph of
        autograd.ReadoutTail (and autograd.ReadoutHead); after trainable(..., sync=True) loss_av carries one too."""
        tail = self._training_tail()
        with torch.no_grad():
            y, loss = self._forward(clips, audios, frame_feats, features=tail)
        if not tail:
            return y, loss
        out, loss_av = self._tail_with_grad(y)
        return out, (loss if loss_av is None else loss_av)

    def _forward(self, clips, audios, frame_feats, features):
        self._check_eval()
        pk = self.pk
        clips = clips.float()
        B, dev = clips.shape[0], clips.device
        # Three independent branches (image encoder + adapter | audio encoder | motion encoder) on three HIP streams:
        # the backbones' many small launches (X3D: ~330 kernels of 20-30 us with ragged tails) overlap the image
        # encoder's large GEMMs instead of each draining the chip alone.  Fork / join by events, so a hipGraph
        # capture records them as parallel branches.
        with _Fork(self, dev) as fk:
            with fk.branch(0):
                o1, o0 = self.image_encoder.run(clips) if frame_feats is None else self._wrap_frame_feats(frame_feats)
                masks = self.adapter.run(o1, o0, features)   # "cat": the Inception's input, for autograd.Adapter
                pm = None if reaches(features, "fusion") else self._premask(pk, masks)    # autograd.Fusion runs its own, unfolded
            with fk.branch(1):
                aud = self.audnet.forward_cl(audios.float())
            v1, v2, v3, v4 = self.visnet.forward_cl(self._pack_clips(clips))
            cat, s0, s1, s2 = self._laterals_012(pk, v1, v2, v3, features)
            fk.join(1)
            if features and self.__dict__.get("_trainable_sync"):
                # trainable(..., sync=True) in a forward that carries a graph: neither the SyncBlock nor the contrastive branch
                # is launched; v4 and the audio map travel as fp32 rows to _tail_with_grad (autograd.sync_block, ContrastHead)
                s3, loss = [E.join_planes(x) if isinstance(x, E.SP) else x for x in (v4, aud)], None
            else:
                s3, loss = self._sync_and_lateral3(pk, v4, aud, fk, features)
        return self._fuse_readout(pk, cat, s0, s1, s2, s3, masks, pm, features), loss

    def _sync_and_lateral3(self, pk, v4, aud, fk, features=False):
        B, dev = v4.N, v4.buf.device
        x = self.aud_vis_sync_block.run(v4, aud)
        Rv = v4.T * v4.H * v4.W
        vis_fea = x.tokens(0, v4.T, v4.H, v4.W)
        aud_fea = x.tokens(Rv, aud.T, aud.H, aud.W)
        # Contrastive branch: its value is the second return (model/model_utils.py:545-552), nothing on the map's path
        # reads it -- a dozen tiny launches (M = B rows) that go to the audio branch's now idle stream.
        fk.keep(x)   # main-stream memory read by the side stream: must not return to the allocator before the join
        with fk.branch(1, refork=True):
            pooled = torch.empty(2, B, 512, dtype=torch.float32, device=dev)
            E.mean_rows(vis_fea, B, Rv, pooled[0])
            E.mean_rows(aud_fea, B, aud.T * aud.H * aud.W, pooled[1])
            vis_emb, vis_pred = self._embed(pk["vis"], E.from_rows(pooled[0]))
            aud_emb, aud_pred = self._embed(pk["aud"], E.from_rows(pooled[1]))
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            E.neg_cosine(vis_pred, aud_emb, loss, 0.5, False)
            E.neg_cosine(aud_pred, vis_emb, loss, 0.5, True)
        return self._lateral(pk, 3, [v4, vis_fea], features=features), loss[0]


class VisualSaliencyModel(_SaliencyBase):
    """forward(clips) -> (log-probability map [B,H,W], 0)  (model/model_utils.py:576-702)."""

    def __init__(self, cfg, vis_embed_dims=(96, 192, 384, 768), aud_embed_dim=512, de_embed_dim=192,
                 num_vis_tokens=4 * 7 * 7, norm=nn.LayerNorm):
        super().__init__()
        print("Motion Encoder is {}.".format(cfg.MODEL.MOTION_ENCODER))
        self.cfg = cfg
        vis_embed_dims = cfg.MODEL.MOTION_ENCODER_EMBEDS[cfg.MODEL.MOTION_ENCODER]
        self.image_encoder = StaticSaliencyModelConvNext()
        self.visnet = video_motion_extractor(cfg)
        self._build_decoder(cfg, vis_embed_dims, 0, de_embed_dim)
        self._try_load(self.visnet.load_weight, cfg.MODEL.MOTION_ENCODER_WEIGHT, "motion encoder weights")
        self._try_load(lambda p: self.image_encoder.load_state_dict(torch.load(p, map_location="cpu"), strict=False),
                       cfg.MODEL.IMAGE_SALIENCY_ENCODER_WEIGHT, "image saliency encoder weights")

    def frozen_encoder(self):
        if self._frozen_eval():
            return
        self.image_encoder.eval()

    def _pack(self):
        return self._pack_decoder(split=None)

    def forward(self, clips, frame_feats=None):
        tail = self._training_tail()
        with torch.no_grad():
            y = self._forward(clips, frame_feats, features=tail)
        return (self._tail_with_grad(y)[0] if tail else y), 0

    def _forward(self, clips, frame_feats, features):
        self._check_eval()
        pk = self.pk
        clips = clips.float()
        with _Fork(self, clips.device) as fk:
            with fk.branch(0):
                o1, o0 = self.image_encoder.run(clips) if frame_feats is None else self._wrap_frame_feats(frame_feats)
                masks = self.adapter.run(o1, o0, features)   # "cat": the Inception's input, for autograd.Adapter
                pm = None if reaches(features, "fusion") else self._premask(pk, masks)    # autograd.Fusion runs its own, unfolded
            v1, v2, v3, v4 = self.visnet.forward_cl(self._pack_clips(clips))
            cat, s0, s1, s2 = self._laterals_012(pk, v1, v2, v3, features)
            s3 = self._lateral(pk, 3, [v4], features=features)
        return self._fuse_readout(pk, cat, s0, s1, s2, s3, masks, pm, features)
