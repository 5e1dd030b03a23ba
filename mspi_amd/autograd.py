"""torch.autograd surface of the hand-written backward kernels.

ReadoutTail: the decoder's last three convs and the log-softmax (readout[8], readout[10], readout[12] of
model/model_utils.py:403-409) as one autograd.Function over the features y4 that enter readout[8] and the six parameters.
Forward and backward run on the C ABI (mspi_amd.engine); the forward launches what the inference path launches.

ReadoutHead: the three convs in front of it (readout[0], readout[1] + BatchNorm readout[2], readout[4] + BatchNorm readout[5],
model/model_utils.py:490-497) with the BatchNorm layers on BATCH statistics, over the four fused pyramid maps.  Its output is
ReadoutTail's input, so the two together train the whole readout Sequential.

Fusion: the stage in front of that -- the three SA gates (model/model_utils.py:155-170) with their BatchNorm on BATCH
statistics and the top-down sums of model/model_utils.py:566-567 -- over the four lateral outputs and the adapter's masks.  Its
outputs are ReadoutHead's maps, whose gradients ReadoutHead computes when they are asked for.

LateralBlock: the ConvNextBlock at the end of each lateral (model/model_utils.py:306-354) over the entry conv's output and the
block's ten tensors.  Its output is one of Fusion's laterals.

LateralEntry: the entry conv(s) in front of that block -- latlayer_k[0], 1x1x1 C_k -> 192 with bias, and where present
latlayer_k[1], (s,1,1) / stride (s,1,1) 192 -> 192 without bias, run composed as one conv (compose_lateral) -- over the
encoder map(s).  Its output is LateralBlock's input, whose gradient LateralBlock computes when it is asked for.

TransformerBlock: one pre-LN transformer Block of the SyncBlock (model/model_utils.py:84-152) over its input tokens and its
eleven tensors.  SyncEmbed: the embedding in front of the blocks (vis_proj, vis_norm, aud_norm, the sinusoid tables as
constants); sync_block: the two chained, the whole SyncBlock over its 39 tensors.  ContrastHead: the contrastive head behind it
(the two pooled rows, projectors, predictors and the two negative cosines) over the slab and its 36 tensors.  No stage of the
ladder holds them: trainable(what, sync=True) switches them on beside a stage that reaches "lateral_entries".

X3DBlock: one stride-1 X3D residual block without branch1 (backbones/blocks3d.py: ResBlock over an X3DTransform) with its three
BatchNorm layers on BATCH statistics, over its input and 13 tensors; x3d_blocks chains it over the blocks of a ResStage.  No
model reaches them yet: the stage heads and the stem have no backward."""
import collections

import torch

from . import engine as E
from ._lib import MspiError

# The training stages, each on top of the one before: the one place a new stage is added.  stop: what _training_tail() answers
# and the forward stops at; params: the parameter-name prefixes the stage adds ({k}, {last}: each lateral and the index of its
# ConvNextBlock); batch_stat: the BatchNorm modules it puts on batch statistics; only: what _check_eval says may be in train().
Stage = collections.namedtuple("Stage", "name stop params batch_stat only")
_SA_BN = tuple("sa_%d.conv_mask.0.bn" % k for k in range(3))
_ADAPTER_BN = tuple("adapter.conv.branch%s" % n for n in ("0.0.bn", "1.0.bn", "1.1.bn_s", "1.1.bn_t", "2.0.bn", "2.1.bn_s", "2.1.bn_t",
                                                         "3.1.bn"))        # ADAPTER_LAYERS order
_ONLY5 = "only readout.2, readout.5 and the three sa_k.conv_mask.0.bn run on batch statistics"
STAGES = (
    Stage("readout_tail", True, tuple("readout.%d.%s" % (i, n) for i in (8, 10, 12) for n in ("weight", "bias")), (), None),
    Stage("readout", "maps", ("readout.",), ("readout.2", "readout.5"), "only readout.2 and readout.5 run on batch statistics"),
    Stage("fusion", "laterals", ("sa_0.", "sa_1.", "sa_2."), _SA_BN, _ONLY5),
    Stage("lateral_blocks", "entries", ("latlayer_{k}.{last}.",), (), _ONLY5 + " (the blocks' LayerNorm has no mode)"),
    Stage("lateral_entries", "inputs", ("latlayer_",), (),
          _ONLY5 + " (neither the entry convs nor the blocks' LayerNorm have a mode)"),
    Stage("adapter", "cat", ("adapter.",), _ADAPTER_BN,
          "only readout.2, readout.5, the three sa_k.conv_mask.0.bn and the eight BatchNorm layers of adapter.conv run on batch "
          "statistics"),
)
STAGE_NAMES = tuple(s.name for s in STAGES)


def stage_rank(x):
    """The ladder position of a stage name or of a stop value (what _training_tail() answers); -1 for None and False."""
    if x is None or x is False:
        return -1
    return next(i for i, s in enumerate(STAGES) if x == s.name or x == s.stop)


def reaches(x, name):
    """True where x, a stage name or a stop value, is the stage `name` or one above it."""
    return stage_rank(x) >= STAGE_NAMES.index(name)


def stages_upto(what):
    """The stages trainable(what) switches on, lowest first."""
    return STAGES[:stage_rank(what) + 1]


def _check_input(t, what=None, layout="[B,T,h,w,C]", beside=None):
    """The refusals a Function opens with: a tensor off the GPU (or `beside` on another device), and, with what = "Function:
    name", one that is not fp32 with five dimensions."""
    if not t.is_cuda or (beside is not None and beside.device != t.device):
        raise MspiError("mspi_amd runs on the GPU only (tensor on %s); there is no CPU fallback" % t.device)
    if what is not None and (t.dim() != 5 or t.dtype != torch.float32):
        raise MspiError("%s must be fp32 %s (channels-last), got %s %s" % (what, layout, t.dtype, tuple(t.shape)))


def _pack_dgrad(w, pad):
    """The data gradient of a stride-1 "same" conv is the same conv with w'[ci][-tap][co] (a flip over an extent of 1 is the
    identity, so one flip serves the (1,3,3) layers too).  On the fp32 MFMA path: the activation operand is a gradient, whose
    scale is the loss's (1e-5 and below with SalLoss at the training shape), and the f16x3 split of an activation is exact only
    while its largest entries stay above about 2^-5."""
    return E.pack_conv(w.detach().transpose(0, 1).flip(2, 3, 4), None, None, (1, 1, 1), pad, E.ACT_NONE, prec=E.PREC_F32)


def _pack_t(w):
    """The transposed 1x1x1 conv (or 2-D weight) for a data gradient, on the fp32 MFMA path as in _pack_dgrad."""
    return E.pack_conv(w.detach().flatten(1).t().contiguous(), None, prec=E.PREC_F32)


def pack_readout_tail(w8, b8, w10, b10, w12, b12):
    """The three packs of the tail, as _SaliencyBase._pack_decoder builds them."""
    return (E.pack_conv(w8, b8, None, (4, 1, 1), (0, 0, 0), E.ACT_NONE),
            E.pack_conv(w10, b10, None, (1, 1, 1), (0, 1, 1), E.ACT_RELU),
            E.pack_conv(w12, b12, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE))


def readout_tail_forward(y4, pk8, pk10, pk12):
    """y4: CL [B,4,h,w,64] -> (out [B,H,W] log-probabilities, u, y10): four launches.  u and y10 are the two post-ReLU
    activations the backward needs; inference drops them."""
    u = E.upsample(E.conv(y4, pk8), 4, act=E.ACT_RELU)      # == relu(conv(4,1,1)(upsample(y))) of the reference
    y10 = E.conv(u, pk10)
    z = E.conv(y10, pk12)                                    # [B,1,H,W,1], ld 1
    E.logsumexp_sub(z.buf, z.N, z.H * z.W)
    return z.buf.view(z.N, z.H, z.W), u, y10


class ReadoutTail(torch.autograd.Function):
    """out = ReadoutTail.apply(y4, w8, b8, w10, b10, w12, b12): y4 [B,4,h,w,64] channels-last fp32 on the GPU, the parameters in
    their nn.Conv3d layouts.  The packs are built from the parameters' present values at every call (an optimiser changes them
    in place).  Gradients: each parameter that needs one, y4 only when it requires grad.  No double backward."""

    @staticmethod
    def forward(ctx, y4, w8, b8, w10, b10, w12, b12):
        if y4.dim() != 5 or y4.shape[1] != 4 or y4.shape[4] != 64 or y4.dtype != torch.float32:
            raise MspiError("ReadoutTail: y4 must be fp32 [B,4,h,w,64] (channels-last), got %s" % (tuple(y4.shape),))
        _check_input(y4)
        y4 = y4.detach().contiguous()
        B, _, h, w, _ = y4.shape
        with torch.no_grad():
            pk8, pk10, pk12 = pack_readout_tail(w8, b8, w10, b10, w12, b12)
            out, u, y10 = readout_tail_forward(E.CL(y4.view(-1), 0, B, 4, h, w, 64, 64), pk8, pk10, pk12)
        ctx.save_for_backward(y4, u.buf, y10.buf, out, w8, w10, w12)
        ctx.geom, ctx.packs = (B, h, w), (pk8, pk10)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y4, ub, y10b, out, w8, w10, w12 = ctx.saved_tensors
        B, h, w = ctx.geom
        H, W = 4 * h, 4 * w
        need = ctx.needs_input_grad
        x4 = E.CL(y4.view(-1), 0, B, 4, h, w, 64, 64)
        u = E.CL(ub, 0, B, 1, H, W, 32, 32)
        y10 = E.CL(y10b, 0, B, 1, H, W, 32, 32)
        pk8, pk10 = ctx.packs
        dz = E.logsumexp_sub_bwd(out, g.float())
        d10, dw12, db12 = E.conv_c1_bwd(y10, dz, w12)
        grads = [None] * 7
        grads[5], grads[6] = (dw12 if need[5] else None), (db12 if need[6] else None)
        if not any(need[:5]):
            return tuple(grads)
        if need[3] or need[4]:
            dw10, db10 = E.conv_wgrad(u, d10, pk10)
            grads[3], grads[4] = (dw10 if need[3] else None), (db10 if need[4] else None)
        if not any(need[:3]):
            return tuple(grads)
        d8 = E.upsample_bwd(E.conv(d10, _pack_dgrad(w10, (0, 1, 1))), 4, u=u, act=E.ACT_RELU)
        if need[1] or need[2]:
            dw8, db8 = E.conv_wgrad(x4, d8, pk8)
            grads[1], grads[2] = (dw8 if need[1] else None), (db8 if need[2] else None)
        if need[0]:
            # d y4[b,t,h,w,ci] = sum_co d8[b,h,w,co] W8[co,ci,t]: one 32 -> 256 GEMM, columns (t, ci), then the t slabs moved out
            pk8t = E.pack_conv(w8.detach()[:, :, :, 0, 0].permute(2, 1, 0).reshape(256, 32), None, prec=E.PREC_F32)
            rows = E.conv(d8, pk8t)                                           # [B*h*w, 256]
            hw = h * w
            grads[0] = E.permute(rows, (B, 4, hw, 64), (hw * 256, 64, 256, 1)).view(B, 4, h, w, 64)
        return tuple(grads)


def r0_parts(weight, bias):
    """The readout's 1x1x1 conv over cat(s0', up2(s1'), up4(s2'), up8(s3)) with s0' = s0 + up2(s1') + up4(s2') + up8(s3):
    a 1x1x1 conv commutes with a per-channel bilinear up-sample, so with W = [W0|W1|W2|W3]
    r0(cat) = W0 s0 + b + up2((W0+W1) s1') + up4((W0+W2) s2') + up8((W0+W3) s3).  Returns [(w, b)] * 4, summed in fp32."""
    w = weight.detach().float().flatten(1)
    d = w.shape[1] // 4
    w0 = w[:, :d]
    return [(w0.contiguous(), bias.detach().float())] + [((w0 + w[:, j * d:(j + 1) * d]).contiguous(), None) for j in (1, 2, 3)]


BN_EPS, BN_MOMENTUM = 1e-5, 0.1          # nn.BatchNorm3d's defaults, which the readout's two layers are built with


def _bn_running(buffers, mean, var, M, momentum):
    """The running-stat update of nn.BatchNorm3d.train(): the UNBIASED variance into running_var, num_batches_tracked += 1
    (buffers None: skipped)."""
    if buffers is None:
        return
    rm, rv, nbt = buffers
    rm.mul_(1.0 - momentum).add_(mean, alpha=momentum)
    rv.mul_(1.0 - momentum).add_(var, alpha=momentum * M / (M - 1.0))
    nbt.add_(1)


BN_MAX_CH = 192                          # widest channel count the mspi_bn_* entry points take


def _bn_slices(c):
    """Channel slices the BatchNorm kernels take: the statistics are per channel, so a wider layer in slices is exact."""
    if c <= BN_MAX_CH:
        return [(0, c)]
    n = -(-c // BN_MAX_CH)
    step = (-(-c // n) + 3) // 4 * 4
    return [(c0, min(step, c - c0)) for c0 in range(0, c, step)]


def bn_relu_train(x, gamma, beta, eps, out=None):
    """BatchNorm on the batch statistics of the CL x, then ReLU, into out (None: a new CL like x): bn_stats and bn_apply over
    _bn_slices(x.C).  Returns (y, mean, biased var, rstd); where one slice covers the width the three are bn_stats' own vectors.
    The running statistics are the caller's (_bn_running)."""
    gamma, beta = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
    if out is None:
        out = E.alloc(x.N, x.T, x.H, x.W, x.C, x.buf.device)
    stats = []
    for c0, c in _bn_slices(x.C):
        xs = x.slice(c0, c)
        mean, var, rstd = E.bn_stats(xs, eps)
        E.bn_apply(xs, mean, rstd, gamma[c0:c0 + c], beta[c0:c0 + c], act=E.ACT_RELU, out=out.slice(c0, c))
        stats.append((mean, var, rstd))
    mean, var, rstd = stats[0] if len(stats) == 1 else (torch.cat(ts) for ts in zip(*stats))
    return out, mean, var, rstd


def _cl5(t):
    B, T, h, w, c = t.shape
    return E.CL(t.view(-1), 0, B, T, h, w, c, c)


class ReadoutHead(torch.autograd.Function):
    """y4 = ReadoutHead.apply(s0, s1, s2, s3, w0, b0, w1, b1, g2, be2, w4, b4, g5, be5, bn2, bn5)
    s0..s3: the four fused pyramid maps, channels-last fp32 [B,T,h,w,D], [B,T,h/2,w/2,D], [B,T,h/4,w/4,D], [B,T,h/8,w/8,D], as
    the default path of _SaliencyBase._fuse_readout holds them in front of its r0_parts launches (s0 SA-gated and not yet
    summed, s1 and s2 already summed top-down).  The ten parameters of readout[0], [1], [2], [4], [5] in their nn layouts;
    bn2 / bn5: (running_mean, running_var, num_batches_tracked) of readout[2] / readout[5], updated in place as
    nn.BatchNorm3d.train() updates them; None only skips that update -- the normalisation is on BATCH statistics either way,
    never on the running ones (the model refuses a grad forward with these two modules in eval()).  Returns y4 [B,T,h,w,C4], the input of ReadoutTail.
    Gradients: the ten parameters, and each of the four maps that requires grad (d s0 = W0^T dy0, d sj = (W0 + Wj)^T up_j^T dy0:
    four more 1x1x1 convs); with detached maps nothing more is launched than before.  No double backward."""

    @staticmethod
    def forward(ctx, s0, s1, s2, s3, w0, b0, w1, b1, g2, be2, w4, b4, g5, be5, bn2, bn5):
        maps = []
        for j, s in enumerate((s0, s1, s2, s3)):
            _check_input(s)
            if s.dim() != 5 or s.dtype != torch.float32 or s.shape[4] != s0.shape[4] or s.shape[:2] != s0.shape[:2] or \
                    (s.shape[2] << j, s.shape[3] << j) != tuple(s0.shape[2:4]):
                raise MspiError("ReadoutHead: s%d %s does not continue the pyramid of s0 %s (fp32 channels-last, each level "
                                "half the one before)" % (j, tuple(s.shape), tuple(s0.shape)))
            maps.append(s.detach().contiguous())
        with torch.no_grad():
            cls = [_cl5(s) for s in maps]
            parts = [E.pack_conv(w, b) for w, b in r0_parts(w0, b0)]
            y0 = E.conv(cls[0], parts[0])
            E.upsample_sum(y0, [(E.conv(cls[1], parts[1]), 2), (E.conv(cls[2], parts[2]), 4), (E.conv(cls[3], parts[3]), 8)])
            pk1 = E.pack_conv(w1, b1, None, (1, 1, 1), (1, 1, 1), E.ACT_NONE)
            pk4 = E.pack_conv(w4, b4, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE)
            x1 = E.conv(y0, pk1)
            a1, m2, v2, r2 = bn_relu_train(x1, g2, be2, BN_EPS)
            _bn_running(bn2, m2, v2, x1.M, BN_MOMENTUM)
            x4 = E.conv(a1, pk4)
            y4, m5, v5, r5 = bn_relu_train(x4, g5, be5, BN_EPS)
            _bn_running(bn5, m5, v5, x4.M, BN_MOMENTUM)
        ctx.save_for_backward(*maps, y0.buf, x1.buf, a1.buf, x4.buf, y4.buf, m2, r2, m5, r5, w1, g2, w4, g5, w0, b0)
        ctx.packs = (parts, pk1, pk4)
        return y4.as_nthwc()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s0, s1, s2, s3, y0b, x1b, a1b, x4b, y4b, m2, r2, m5, r5, w1, g2, w4, g5, w0, b0 = ctx.saved_tensors
        parts, pk1, pk4 = ctx.packs
        B, T, h, w, D = s0.shape
        c1, c4 = w1.shape[0], w4.shape[0]

        def cl(buf, c):
            return E.CL(buf, 0, B, T, h, w, c, c)
        y0, x1, a1, x4, y4 = cl(y0b, c1), cl(x1b, c1), cl(a1b, c1), cl(x4b, c4), cl(y4b, c4)
        d4, dg5, dbe5 = E.bn_bwd(cl(g.float().contiguous().view(-1), c4), x4, m5, r5, g5.detach().contiguous(), y=y4)
        dw4, db4 = E.conv_wgrad_wide(a1, d4, pk4)
        d1, dg2, dbe2 = E.bn_bwd(E.conv(d4, _pack_dgrad(w4, (0, 1, 1))), x1, m2, r2, g2.detach().contiguous(), y=a1)
        dw1, db1 = E.conv_wgrad_wide(y0, d1, pk1)
        dy0 = E.conv(d1, _pack_dgrad(w1, (1, 1, 1)))
        # dW0 without the 768-channel concat: the adjoint of r0_parts.  y0 = W0 s0 + b + sum_j up_j((W0 + Wj) sj'), j = 1, 2, 3,
        # and <up_j(A s), dy0> = <A s, up_j^T dy0>, so with g_j = up_j^T dy0 (upsample_bwd) and G0 = dy0^T s0, G_j = g_j^T sj':
        #   dL/dW0 = G0 + G1 + G2 + G3 (W0 takes part in every term), dL/dWj = G_j, db0 = sum dy0
        G0, db0 = E.conv_wgrad_wide(_cl5(s0), dy0, parts[0])
        gs = [dy0] + [E.upsample_bwd(dy0, k) for k in (2, 4, 8)]
        Gs = [E.conv_wgrad_wide(_cl5(s), g, pk)[0] for s, g, pk in ((s1, gs[1], parts[1]), (s2, gs[2], parts[2]), (s3, gs[3], parts[3]))]
        dw0 = torch.cat([((G0 + Gs[0]) + Gs[1]) + Gs[2]] + Gs, dim=1)
        need = ctx.needs_input_grad
        # the maps' gradients, each only when asked for: d s0 = W0^T dy0, d sj = (W0 + Wj)^T g_j
        dmaps = [E.conv(gs[j], _pack_t(wj)).as_nthwc() if need[j] else None for j, (wj, _) in enumerate(r0_parts(w0, b0))]
        grads = dmaps + [dw0, db0, dw1, db1, dg2, dbe2, dw4, db4, dg5, dbe5, None, None]
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


SA_BN_EPS, SA_BN_MOMENTUM = 1e-3, 0.001  # BasicConv3d's BatchNorm3d(eps=1e-3, momentum=0.001) (backbones/s3d.py:45), SA's first layer
SA_FACTORS = (4, 2, 1)                   # sa_0, sa_1, sa_2 up-sample their premask by these (model/model_utils.py:500-502 upstream)
WGRAD_WIDE_MAX_CH = 192                  # widest stored channel count mspi_conv_wgrad_wide_fwd takes


def _geometry(k, pad, cin, cout, stride=(1, 1, 1)):
    """What conv_wgrad_wide / conv_wgrad_entry read of a pack (the layer's geometry), without packing any weights."""
    p = E.PackedConv()
    p.k, p.stride, p.pad, p.cin, p.cin_s, p.cout, p.cout_s = k, stride, pad, cin, cin, cout, cout
    return p


class Fusion(torch.autograd.Function):
    """s0, s1, s2, s3 = Fusion.apply(l0, l1, l2, l3, masks, *sa, bn_0, bn_1, bn_2): the decoder stage between the laterals and
    readout[0] -- the three SA gates (model/model_utils.py:155-170) and the top-down sums of model/model_utils.py:566-567 -- as
    the default path of _SaliencyBase._fuse_readout runs it, returning the four maps autograd.ReadoutHead takes.
    l0..l3: the lateral outputs, channels-last fp32 [B,T,h,w,D] .. [B,T,h/8,w/8,D]; masks: the adapter's [B,T,h/4,w/4,Cm].
    sa: for k = 0, 1, 2 (sa_0 gates l0 after a x4 up-sample, sa_1 l1 after x2, sa_2 l2) the five tensors conv_mask[0].conv.weight,
    conv_mask[0].bn.weight, conv_mask[0].bn.bias, conv_mask[2].weight, conv_mask[2].bias in their nn layouts.  bn_k:
    (running_mean, running_var, num_batches_tracked) of sa_k.conv_mask[0].bn, updated in place as nn.BatchNorm3d.train()
    with that layer's momentum 0.001 updates them, or None to skip that; the normalisation is on BATCH statistics either way.
    Gradients: the 15 SA tensors and each lateral that requires grad; masks when it requires grad (trainable("adapter")): the
    data gradient of the concatenated 3x3x3 conv, one more launch -- with detached masks nothing more is launched and every
    other gradient keeps its bits.  No double backward."""

    @staticmethod
    def forward(ctx, l0, l1, l2, l3, masks, *rest):
        if len(rest) != 18:
            raise MspiError("Fusion: expected 15 SA tensors and 3 BatchNorm buffer triples after masks, got %d arguments" % len(rest))
        sa, bns = [rest[5 * k:5 * k + 5] for k in range(3)], rest[15:]
        lats = []
        for j, t in enumerate((l0, l1, l2, l3)):
            _check_input(t)
            if t.dim() != 5 or t.dtype != torch.float32 or t.shape[4] != l0.shape[4] or t.shape[4] % 4 or t.shape[:2] != l0.shape[:2] or \
                    (t.shape[2] << j, t.shape[3] << j) != tuple(l0.shape[2:4]):
                raise MspiError("Fusion: l%d %s does not continue the pyramid of l0 %s (fp32 channels-last, a multiple of 4 wide, "
                                "each level half the one before)" % (j, tuple(t.shape), tuple(l0.shape)))
            lats.append(t.detach().contiguous())
        B, T, h, w, D = l0.shape
        mid, Cm = sa[0][0].shape[:2]
        if masks.dim() != 5 or masks.dtype != torch.float32 or tuple(masks.shape) != (B, T, h // 4, w // 4, Cm) or masks.device != l0.device:
            raise MspiError("Fusion: masks %s is not fp32 [B,T,h/4,w/4,%d] on the level of l2" % (tuple(masks.shape), Cm))
        for k, (wc, gam, bet, w2, b2) in enumerate(sa):
            if tuple(wc.shape) != (mid, Cm, 3, 3, 3) or gam.numel() != mid or bet.numel() != mid or tuple(w2.shape) != (1, mid, 1, 3, 3) or \
                    b2.numel() != 1 or mid % 32 or Cm % 32:
                raise MspiError("Fusion: the tensors of sa_%d are not a (3,3,3) conv %d -> %d (multiples of 32), its BatchNorm and a "
                                "(1,3,3) conv to 1" % (k, Cm, mid))
        masks = masks.detach().contiguous()
        with torch.no_grad():
            x = _cl5(masks)
            # the three first convs share their input: one conv Cm -> 3 mid, unfolded (no bias, no activation), then one BatchNorm
            pre = E.conv(x, E.pack_conv(torch.cat([p[0] for p in sa], 0), None, None, (1, 1, 1), (1, 1, 1), E.ACT_NONE))
            gamma = torch.cat([p[1].detach().float() for p in sa]).contiguous()
            beta = torch.cat([p[2].detach().float() for p in sa]).contiguous()
            pm, mean, var, rstd = bn_relu_train(pre, gamma, beta, SA_BN_EPS)
            for k, bn in enumerate(bns):
                _bn_running(bn, mean[k * mid:(k + 1) * mid], var[k * mid:(k + 1) * mid], pre.M, SA_BN_MOMENTUM)
            outs, ms, gates = [], [], []
            for k in (2, 1, 0):                       # the order of _fuse_readout
                m = pm.slice(k * mid, mid)
                if SA_FACTORS[k] != 1:
                    m = E.upsample(m, SA_FACTORS[k])
                gate = E.conv(m, E.pack_conv(sa[k][3], sa[k][4], None, (1, 1, 1), (0, 1, 1), E.ACT_SIGMOID))
                s = _cl5(lats[k].clone())             # the ungated l_k is what the backward reads
                E.rowgate(s, gate)
                if k == 2:
                    E.upsample(_cl5(lats[3]), 2, dst=s, accumulate=True)
                elif k == 1:
                    E.upsample_sum(s, [(outs[0], 2), (_cl5(lats[3]), 4)])
                outs.append(s)
                ms.append(m.buf)
                gates.append(gate.buf)
        s2, s1, s0 = outs
        ctx.save_for_backward(lats[0], lats[1], lats[2], masks, pre.buf, pm.buf, mean, rstd, gamma, *ms[::-1], *gates[::-1],
                              *[p[3] for p in sa], *[p[0] for p in sa])
        ctx.dims = (B, T, h, w, D, Cm, mid)
        return tuple(t.as_nthwc() for t in (s0, s1, s2)) + (lats[3].clone(),)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G0, G1, G2, G3):
        l0, l1, l2, masks, preb, pmb, mean, rstd, gamma, m0b, m1b, m2b, g0b, g1b, g2b, w20, w21, w22, wc0, wc1, wc2 = ctx.saved_tensors
        B, T, h, w, D, Cm, mid = ctx.dims
        need = ctx.needs_input_grad
        dev = l0.device
        hm, wm = h // 4, w // 4

        def grad(g, j):        # the incoming gradients are read only: an absent one is a zero map
            shape = (B, T, h >> j, w >> j, D)
            return _cl5(torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.float().contiguous())
        G = [grad(g, j) for j, g in enumerate((G0, G1, G2, G3))]
        # s2 = gate(l2) + up2(l3), s1 = gate(l1) + up2(s2) + up4(l3):  D2 = G2 + up2^T G1,  D3 = G3 + up4^T G1 + up2^T D2
        D2 = E.upsample_sum_bwd(_cl5(G[2].as_nthwc().clone()), [(G[1], 2)], accumulate=True)
        grads = [None] * 23
        if need[3]:
            grads[3] = E.upsample_sum_bwd(_cl5(G[3].as_nthwc().clone()), [(G[1], 4), (D2, 2)], accumulate=True).as_nthwc()
        sa_need = any(need[4:20])                # the gradient of masks runs through the three gates as well
        dp = E.alloc(B, T, hm, wm, 3 * mid, dev)
        for k, (Gk, lk, mb, gb, w2) in enumerate(((G[0], l0, m0b, g0b, w20), (G[1], l1, m1b, g1b, w21), (D2, l2, m2b, g2b, w22))):
            if not (need[k] or sa_need):
                continue
            f = SA_FACTORS[k]
            hk, wk = h >> k, w >> k
            dl, dz = E.rowgate_bwd(Gk, _cl5(lk), E.CL(gb, 0, B, T, hk, wk, 1, 1), need_dx=need[k])
            if need[k]:
                grads[k] = dl.as_nthwc()
            if not sa_need:
                continue
            # mspi_conv_c1_bwd masks its data gradient where its input y <= 0, and that is exact for all three gates.  sa_2
            # (f == 1): y is the post-ReLU premask, so the mask is the ReLU's.  sa_0, sa_1: y is a bilinear up-sample, with
            # non-negative weights, of the non-negative premask; it is 0 only where every source it taps with a positive weight
            # is 0, the gradient of such a cell goes to those sources alone, and bn_bwd's ReLU mask clears them anyway.
            # (T folds into N: a (1,3,3) conv does not mix frames.)
            m = E.CL(mb, 0, B * T, 1, hk, wk, mid, mid) if f != 1 else E.CL(mb, k * mid, B * T, 1, hk, wk, mid, 3 * mid)
            dm, dw2, db2 = E.conv_c1_bwd(m, dz.view(B * T, hk, wk), w2)
            grads[5 + 5 * k + 3], grads[5 + 5 * k + 4] = dw2, db2
            if f != 1:
                E.upsample_bwd(dm.reshape(B, T, hk, wk), f, dx=dp.slice(k * mid, mid))
            else:
                dp.buf.view(-1, 3 * mid)[:, k * mid:(k + 1) * mid].copy_(dm.buf.view(-1, mid))
        if not sa_need:
            return tuple(grads)
        pre, pm = E.CL(preb, 0, B, T, hm, wm, 3 * mid, 3 * mid), E.CL(pmb, 0, B, T, hm, wm, 3 * mid, 3 * mid)
        dpre, dgam, dbet = E.bn_bwd(dp, pre, mean, rstd, gamma, y=pm)
        # the (3,3,3) conv's weight gradient in input-channel slices the wide kernel takes (512 = 192 + 192 + 128)
        dW = wgrad_wide_sliced(_cl5(masks), dpre, (3, 3, 3), (1, 1, 1))[0]
        if need[4]:      # the data gradient of the concatenated (3,3,3) conv Cm -> 3 mid
            grads[4] = E.conv(dpre, _pack_dgrad(torch.cat([wc0, wc1, wc2], 0), (1, 1, 1))).as_nthwc()
        for k in range(3):
            sl = slice(k * mid, (k + 1) * mid)
            grads[5 + 5 * k], grads[5 + 5 * k + 1], grads[5 + 5 * k + 2] = dW[sl], dgam[sl], dbet[sl]
        return tuple(g if g is None or need[i] else None for i, g in enumerate(grads))


LN_EPS = 1e-5                            # nn.LayerNorm's default, which ConvNextBlock.norm is built with
MLP_FUSED_MIN_ROWS = 4096                # from here on the block's LN -> 1x1x1 -> GELU -> 1x1x1 -> +x runs as one launch (E.mlp)


def pack_convnext_block(wt, bt, ws, bs, gamma, beta, w1, b1, w2, b2):
    """The plan of a ConvNextBlock from its ten tensors in their nn layouts: what ConvNextBlock._pack holds and what
    LateralBlock.forward builds from the live values, so the two cannot drift."""
    d, hidden = w1.shape[1], w1.shape[0]
    return {"dt": E.pack_dwconv(wt, bt, None, (1, 1, 1), (3, 0, 0)),
            "ds": E.pack_dwconv(ws, bs, None, (1, 1, 1), (0, 3, 3)),
            "ln": (gamma.detach().float().contiguous(), beta.detach().float().contiguous()),
            "p1": E.pack_conv(w1, b1, act=E.ACT_GELU),
            "p2": E.pack_conv(w2, b2),
            # LN -> 1x1x1 -> GELU -> 1x1x1 -> +x in one launch where the fused kernel covers the width (dim 192)
            "fused": E.pack_mlp(w1.flatten(1), b1, w2.flatten(1), b2) if E.mlp_supported(d, hidden) else None}


def convnext_block_forward(x, pk, out=None):
    """ConvNextBlock.run on the plan pk: (y, a, b) with a = dw_t(x) and b = dw_s(a), which the backward reads."""
    a = E.dwconv(x, pk["dt"])
    b = E.dwconv(a, pk["ds"])
    if pk["fused"] is not None and b.M >= MLP_FUSED_MIN_ROWS:      # below that the two tiled GEMMs (split-K on the small maps) win
        return E.mlp(b, pk["fused"], res=x, ln=pk["ln"], eps=LN_EPS, out=out, split=(pk["p1"], pk["p2"])), a, b
    return E.conv(E.conv(E.layernorm(b, *pk["ln"], LN_EPS), pk["p1"]), pk["p2"], res=x, out=out), a, b


def _wide_cut(c):
    """Even channel slices of at most WGRAD_WIDE_MAX_CH, multiples of 32: 512 -> 192, 192, 128; 416 -> 160, 160, 96."""
    n = -(-c // WGRAD_WIDE_MAX_CH)
    step = -(-c // n // 32) * 32
    return [(c0, min(step, c - c0)) for c0 in range(0, c, step)]


def wgrad_wide_sliced(x, dy, k, pad):
    """Weight and bias gradient of a stride-1 conv from mspi_conv_wgrad_wide_fwd where both widths are multiples of 32, in
    slices (_wide_cut) of the channels of x, of dy or of both: a slice of the wider tensor as it stands where the kernel accepts
    its strides, a dense copy where it refuses; an operand one slice covers is the tensor itself and is never copied.  Returns
    (dW [Co,Ci,kt,kh,kw], db [Co]); every output slice's db comes with its first input slice."""
    def part(t, c0, c, dense):
        if c == t.C:
            return t
        return E.from_rows(t.as_rows()[:, c0:c0 + c].contiguous()).reshape(t.N, t.T, t.H, t.W) if dense else t.slice(c0, c)
    dWs, dbs = [], []
    for o0, oc in _wide_cut(dy.C):
        cols = []
        for c0, cc in _wide_cut(x.C):
            xs, ds, geo = part(x, c0, cc, False), part(dy, o0, oc, False), _geometry(k, pad, cc, oc)
            if E.conv_wgrad_wide_variant(xs, ds, geo) < 0:
                xs, ds = part(x, c0, cc, True), part(dy, o0, oc, True)
            cols.append(E.conv_wgrad_wide(xs, ds, geo))
        dWs.append(cols[0][0] if len(cols) == 1 else torch.cat([dW for dW, _ in cols], 1))
        dbs.append(cols[0][1])
    return (dWs[0], dbs[0]) if len(dWs) == 1 else (torch.cat(dWs, 0), torch.cat(dbs, 0))


class LateralBlock(torch.autograd.Function):
    """y = LateralBlock.apply(x, wt, bt, ws, bs, gamma, beta, w1, b1, w2, b2): the ConvNextBlock of a lateral on x, channels-last
    fp32 [B,T,h,w,D] on the GPU, D a multiple of 32 -- dwconv_t (7,1,1), dwconv_s (1,7,7), norm.norm, pwconv1 (D -> 4D, GELU) and
    pwconv2 with weight and bias each, in their nn layouts.  The forward launches what ConvNextBlock.run launches, from packs of
    the parameters' present values (pack_convnext_block), the switch at MLP_FUSED_MIN_ROWS rows included, so y has the bits of
    the inference path.  It keeps x, a = dw_t(x) and b = dw_s(a); the backward recomputes n = LN(b) and the 4D-wide
    z = W1 n + b1, which the fused kernel never stores.  Gradients: the ten tensors, and x only when it requires grad.  No
    double backward."""

    @staticmethod
    def forward(ctx, x, wt, bt, ws, bs, gamma, beta, w1, b1, w2, b2):
        _check_input(x, "LateralBlock: x", "[B,T,h,w,D]")
        D = x.shape[4]
        if D % 32:
            raise MspiError("LateralBlock: D = %d is not a multiple of 32 (D %% 32 != 0)" % D)
        want = ((D, 1, 7, 1, 1), (D,), (D, 1, 1, 7, 7), (D,), (D,), (D,), (4 * D, D, 1, 1, 1), (4 * D,), (D, 4 * D, 1, 1, 1), (D,))
        names = ("dwconv_t.weight", "dwconv_t.bias", "dwconv_s.weight", "dwconv_s.bias", "norm.norm.weight", "norm.norm.bias",
                 "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias")
        for name, t, shape in zip(names, (wt, bt, ws, bs, gamma, beta, w1, b1, w2, b2), want):
            if tuple(t.shape) != shape or t.device != x.device:
                raise MspiError("LateralBlock: %s is %s on %s, a ConvNextBlock of dim %d has %s on %s"
                                % (name, tuple(t.shape), t.device, D, shape, x.device))
        x = x.detach().contiguous()
        with torch.no_grad():
            pk = pack_convnext_block(wt, bt, ws, bs, gamma, beta, w1, b1, w2, b2)
            y, a, b = convnext_block_forward(_cl5(x), pk)
        ctx.save_for_backward(x, a.buf, b.buf, wt, ws, gamma, beta, w1, b1, w2)
        ctx.packs = (pk["dt"], pk["ds"])
        return y.as_nthwc()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        xb, ab, bb, wt, ws, gamma, beta, w1, b1, w2 = ctx.saved_tensors
        pdt, pds = ctx.packs
        B, T, h, w, D = xb.shape
        need = ctx.needs_input_grad

        def cl(buf):
            return E.CL(buf.view(-1), 0, B, T, h, w, D, D)
        x, a, b, Gc = cl(xb), cl(ab), cl(bb), cl(G.float().contiguous())
        gam = gamma.detach().float().contiguous()
        # the recompute works on activations, so the forward's f16x3 pack serves; the GELU is taken apart from it (z is needed)
        n = E.layernorm(b, gam, beta.detach().float().contiguous(), LN_EPS)
        z = E.conv(n, E.pack_conv(w1, b1))                                   # [M, 4D]
        dg = E.conv(Gc, _pack_t(w2))
        g, dz = E.gelu_bwd(z, dg, inplace=True)                              # g over z, dz over dg
        dw2, db2 = wgrad_wide_sliced(g, Gc, (1, 1, 1), (0, 0, 0))            # the 4D-wide side in slices: x here, dy below
        dw1, db1 = wgrad_wide_sliced(n, dz, (1, 1, 1), (0, 0, 0))
        dn = E.conv(dz, _pack_t(w1))
        db_, dgamma, dbeta = E.layernorm_bwd(dn, b, gam, LN_EPS)
        # padding 3 under kernel 7 is symmetric: the adjoint of a depthwise conv is the same conv on the flipped taps, no bias
        da = E.dwconv(db_, E.pack_dwconv(ws.detach().flip(2, 3, 4), None, None, (1, 1, 1), (0, 3, 3)))
        dws, dbs = E.dwconv_wgrad(a, db_, pds)
        dwt, dbt = E.dwconv_wgrad(x, da, pdt)
        dx = None
        if need[0]:
            dx = E.dwconv(da, E.pack_dwconv(wt.detach().flip(2, 3, 4), None, None, (1, 1, 1), (3, 0, 0)))
            E.add(dx.buf, Gc.buf, dx.buf)                                                # the residual
            dx = dx.as_nthwc()
        grads = (dx, dwt, dbt, dws, dbs, dgamma, dbeta, dw1, db1, dw2, db2)
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


# ------------------------------------------------------------------------------------------------ transformer Block (SyncBlock)
BLOCK_DIM, BLOCK_HEAD_DIM = 512, 128     # the SyncBlock's width and the one head dim mspi_attn_bwd is instantiated for
BLOCK_TENSORS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                 "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def pack_transformer_block(n1w, n1b, wqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2):
    """The plan of a transformer Block from its eleven tensors in their nn layouts (qkv has no bias): the dict Block._pack
    builds, here from the live values for TransformerBlock.forward.  Block._pack does not call it yet: routing the inference
    path's packs through it was taken out of the change that added this function (DESIGN.md section 7 says why)."""
    def f(t):
        return t.detach().float().contiguous()
    return {"n1": (f(n1w), f(n1b)), "n2": (f(n2w), f(n2b)),
            "qkv": E.pack_conv(wqkv, None), "proj": E.pack_conv(wproj, bproj),
            "fc1": E.pack_conv(w1, b1, act=E.ACT_GELU), "fc2": E.pack_conv(w2, b2)}


def transformer_block_forward(x, pk, B, R, heads, scale):
    """Block.run's launches on the plan pk, keeping what Block.run drops: (y, qkv, o, x1) with o the attention output and
    x1 = x + proj(o), which the backward reads."""
    dim = x.C
    h = E.layernorm_for_gemm(x, *pk["n1"], LN_EPS, pk["qkv"])
    qkv = E.conv(h, pk["qkv"])
    o = E.attention(qkv, B, R, heads, dim // heads, scale, slot=E.attn_slot(pk))
    x1 = E.conv(o, pk["proj"], res=x)
    return E.mlp_tail(x1, ("split", pk["fc1"], pk["fc2"]), pk["n2"], LN_EPS, res=x1), qkv, o, x1


def linear_wgrad_route(M, N, K):
    """"linear" or "sliced": where TransformerBlock.backward takes the weight gradient of a linear layer of M rows, K -> N wide.
    "linear" is one mspi_linear_wgrad launch pair on the operands as they lie; "sliced" is the path the Block had before,
    wgrad_wide_sliced on <= 192-wide channel slices (99 launch pairs a Block).  tools/sync_block_bench.py times both in one
    process by replacing this function; profiles/r22_sync_block.txt holds what was measured."""
    return "linear"


def block_linear_wgrad(x, dy, bias=True):
    """(dW [N, K], db [N] or None) of a linear layer of the Block by the route linear_wgrad_route names."""
    if linear_wgrad_route(x.M, dy.C, x.C) == "linear":
        return E.linear_wgrad(x, dy, bias=bias)
    dW, db = wgrad_wide_sliced(x, dy, (1, 1, 1), (0, 0, 0))
    return dW.flatten(1), (db if bias else None)


class TransformerBlock(torch.autograd.Function):
    """y = TransformerBlock.apply(x, n1w, n1b, wqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2): one pre-LN transformer Block on x,
    fp32 [B,R,512] on the GPU -- norm1, attn.qkv (no bias), attn.proj, norm2, mlp.fc1 (512 -> 2048, GELU) and mlp.fc2 in their nn
    layouts, 4 heads of 128.  The forward launches what Block.run launches, from packs of the parameters' present values
    (pack_transformer_block, the dict of Block._pack), the attention's precision slot decided on this call's data as a freshly packed Block decides it, so
    y has the bits of the inference path.  It keeps x, qkv, the attention output o and x1 = x + proj(o); the backward recomputes
    the two LayerNorms and the 2048-wide z = W1 n + b1.  Attention backward and every data gradient run on the fp32 MFMA
    (_pack_dgrad says why).  Gradients: the eleven tensors and x, each only when it requires grad.  No double backward."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, wqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2):
        _check_input(x)
        D, hd = BLOCK_DIM, BLOCK_HEAD_DIM
        if x.dim() != 3 or x.dtype != torch.float32 or x.shape[2] != D:
            raise MspiError("TransformerBlock: x must be fp32 [B,R,%d], got %s %s" % (D, x.dtype, tuple(x.shape)))
        want = ((D,), (D,), (3 * D, D), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,))
        for name, t, shape in zip(BLOCK_TENSORS, (n1w, n1b, wqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2), want):
            if tuple(t.shape) != shape or t.device != x.device:
                raise MspiError("TransformerBlock: %s is %s on %s, a Block of dim %d with heads of %d has %s on %s"
                                % (name, tuple(t.shape), t.device, D, hd, shape, x.device))
        x = x.detach().contiguous()
        B, R, _ = x.shape
        with torch.no_grad():
            pk = pack_transformer_block(n1w, n1b, wqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2)
            y, qkv, o, x1 = transformer_block_forward(E.CL(x.view(-1), 0, B, R, 1, 1, D, D), pk, B, R, D // hd, hd ** -0.5)
        ctx.save_for_backward(x, qkv.buf, o.buf, x1.buf, n1w, n1b, wqkv, wproj, n2w, n2b, w1, b1, w2)
        ctx.geom = (qkv.off, qkv.ld, o.off, o.ld, x1.off, x1.ld)
        return y.as_rows().view(B, R, D)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        xb, qkvb, ob, x1b, n1w, n1b, wqkv, wproj, n2w, n2b, w1, b1, w2 = ctx.saved_tensors
        B, R, D = xb.shape
        hd = BLOCK_HEAD_DIM
        need = ctx.needs_input_grad
        qoff, qld, ooff, old, xoff, xld = ctx.geom

        def cl(buf, c, off=0, ld=None):
            return E.CL(buf.view(-1), off, B, R, 1, 1, c, c if ld is None else ld)

        def f(t):
            return t.detach().float().contiguous()

        def lin(dW):
            return dW.flatten(1)
        x, qkv, o, x1, Gc = cl(xb, D), cl(qkvb, 3 * D, qoff, qld), cl(ob, D, ooff, old), cl(x1b, D, xoff, xld), cl(G.float().contiguous(), D)
        g1, g2 = f(n1w), f(n2w)
        # the recompute works on activations, so the forward's f16x3 pack serves; the GELU is taken apart from it (z is needed)
        n = E.layernorm(x1, g2, f(n2b), LN_EPS)
        z = E.conv(n, E.pack_conv(w1, b1))                                   # [M, 2048]
        dg = E.conv(Gc, _pack_t(w2))
        g, dz = E.gelu_bwd(z, dg, inplace=True)                              # g over z, dz over dg
        dw2, db2 = block_linear_wgrad(g, Gc)
        dw1, db1 = block_linear_wgrad(n, dz)
        dn = E.conv(dz, _pack_t(w1))
        dx1, dg2, dbt2 = E.layernorm_bwd_wide(dn, x1, g2, LN_EPS)
        E.add(dx1.buf, Gc.buf, dx1.buf)                                      # the MLP's residual
        dwp, dbp = block_linear_wgrad(o, dx1)
        do = E.conv(dx1, _pack_t(wproj))
        dqkv = E.attention_bwd(qkv, o, do, B, R, D // hd, hd, hd ** -0.5)
        h = E.layernorm(x, g1, f(n1b), LN_EPS)
        dwq, _ = block_linear_wgrad(h, dqkv, bias=False)                     # dqkv read in its slab
        dx = dg1 = dbt1 = None
        if need[0] or need[1] or need[2]:
            dh = E.conv(dqkv, _pack_t(wqkv))
            dxc, dg1, dbt1 = E.layernorm_bwd_wide(dh, x, g1, LN_EPS)
            E.add(dxc.buf, dx1.buf, dxc.buf)                                 # the attention's residual
            dx = dxc.as_rows().view(B, R, D)
        grads = (dx, dg1, dbt1, lin(dwq), lin(dwp), dbp, dg2, dbt2, lin(dw1), db1, lin(dw2), db2)
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


SYNC_EMBED_TENSORS = ("vis_proj.weight", "vis_proj.bias", "vis_norm.weight", "vis_norm.bias", "aud_norm.weight", "aud_norm.bias")


class SyncEmbed(torch.autograd.Function):
    """slab = SyncEmbed.apply(vis, aud, wp, bp, gv, bv, ga, ba, vpos, apos): the embedding in front of the SyncBlock's transformer
    blocks (model/model_utils.py:266-275 upstream) -- vis_norm(vis_proj(vis)) + vpos on the visual tokens, aud_norm(aud) + apos on
    the audio tokens, concatenated along the tokens.  vis fp32 [B,t,h,w,C4] and aud [B,1,F,T',512], channels-last on the GPU;
    wp [512,C4], bp, gv, bv, ga, ba [512] in their nn layouts; vpos [t h w, 512] and apos [F T', 512] the constant sinusoid tables
    (no gradient).  The forward runs SyncBlock.run's three embedding launches from packs of the live values, so the slab
    [B, Rv+Ra, 512] has the bits of the inference path.  It keeps vis, p = vis_proj(vis) and aud.  Backward, from the slab's
    gradient: layernorm_bwd_wide on each row range (a dense copy of each), the projection's weight gradient from
    engine.linear_wgrad and its data gradient on _pack_t at PREC_F32; each only when it is asked for.  No double backward."""

    @staticmethod
    def forward(ctx, vis, aud, wp, bp, gv, bv, ga, ba, vpos, apos):
        _check_input(vis, "SyncEmbed: vis", "[B,t,h,w,C4]", beside=aud)
        _check_input(aud, "SyncEmbed: aud", "[B,1,F,T',512]")
        D = BLOCK_DIM
        B, t, h, w, C4 = vis.shape
        if aud.shape[0] != B or aud.shape[4] != D:
            raise MspiError("SyncEmbed: aud is %s, expected [%d,1,F,T',%d] beside vis %s" % (tuple(aud.shape), B, D, tuple(vis.shape)))
        want = ((D, C4), (D,), (D,), (D,), (D,), (D,))
        for name, p, shape in zip(SYNC_EMBED_TENSORS, (wp, bp, gv, bv, ga, ba), want):
            if tuple(p.shape) != shape or p.device != vis.device:
                raise MspiError("SyncEmbed: %s is %s on %s, the embedding of %d-wide visual tokens has %s on %s"
                                % (name, tuple(p.shape), p.device, C4, shape, vis.device))
        Rv, Ra = t * h * w, aud.shape[1] * aud.shape[2] * aud.shape[3]
        if vpos.dim() != 2 or apos.dim() != 2 or Rv != vpos.shape[0] or Ra != apos.shape[0]:
            raise MspiError("SyncBlock: got %d visual / %d audio tokens but the positional tables hold %d / %d rows "
                            "-- set cfg.MODEL.NUM_VIS_TOKENS[name] / cfg.MODEL.NUM_AUD_TOKENS (reference: the add at "
                            "model/model_utils.py:273-274 fails the same way)" % (Rv, Ra, vpos.shape[0], apos.shape[0]))

        def f(p):
            return p.detach().float().contiguous()
        vis, aud = vis.detach().contiguous(), aud.detach().contiguous()
        with torch.no_grad():
            vc, ac = _cl5(vis), _cl5(aud)
            x = E.alloc(B, Rv + Ra, 1, 1, D, vis.device)
            p = E.conv(vc, E.pack_conv(wp, bp))
            E.layernorm(p, f(gv), f(bv), LN_EPS, out=x.tokens(0, vc.T, vc.H, vc.W), table=f(vpos).to(vis.device))
            E.layernorm(ac, f(ga), f(ba), LN_EPS, out=x.tokens(Rv, ac.T, ac.H, ac.W), table=f(apos).to(vis.device))
        ctx.save_for_backward(vis, p.buf, aud, wp, gv, ga)
        ctx.geom = (p.off, p.ld)
        return x.as_rows().view(B, Rv + Ra, D)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        vis, pb, aud, wp, gv, ga = ctx.saved_tensors
        need = ctx.needs_input_grad
        D = BLOCK_DIM
        B, t, h, w, C4 = vis.shape
        Rv, Ra = t * h * w, aud.shape[1] * aud.shape[2] * aud.shape[3]
        poff, pld = ctx.geom
        G = G.float()
        dvis = daud = dwp = dbp = dgv = dbv = dga = dba = None
        if any(need[i] for i in (0, 2, 3, 4, 5)):
            dyv = E.from_rows(G[:, :Rv].reshape(B * Rv, D).contiguous())
            p = E.CL(pb.view(-1), poff, B * Rv, 1, 1, 1, D, pld)
            dp, dgv, dbv = E.layernorm_bwd_wide(dyv, p, gv.detach().float().contiguous(), LN_EPS)
            if need[2] or need[3]:
                dwp, dbp = E.linear_wgrad(E.from_rows(vis.view(B * Rv, C4)), dp)
            if need[0]:
                dvis = E.conv(dp, _pack_t(wp)).as_rows().view(B, t, h, w, C4)
        if any(need[i] for i in (1, 6, 7)):
            dya = E.from_rows(G[:, Rv:].reshape(B * Ra, D).contiguous())
            da, dga, dba = E.layernorm_bwd_wide(dya, E.from_rows(aud.view(B * Ra, D)), ga.detach().float().contiguous(), LN_EPS)
            daud = da.as_rows().view(aud.shape)
        grads = (dvis, daud, dwp, dbp, dgv, dbv, dga, dba, None, None)
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


def sync_block(module, vis, aud):
    """The SyncBlock `module` as a differentiable unit: SyncEmbed on (vis, aud) and module.tensors(), then TransformerBlock on
    each of its blocks' tensors.  vis fp32 [B,t,h,w,C4] and aud [B,1,F,T',512], channels-last on the GPU.  Returns the slab
    [B, Rv+Ra, 512], the bits of module.forward, with a graph over all 39 tensors (and vis and aud where they require grad)."""
    dev = vis.device
    x = SyncEmbed.apply(vis, aud, *module.tensors(), module.vis_pos_embed[0].to(dev), module.aud_pos_embed[0].to(dev))
    for blk in module.blocks:
        x = TransformerBlock.apply(x, *blk.tensors())
    return x


# ------------------------------------------------------------------------------------------------ contrastive head
SYNC_PREFIXES = ("aud_vis_sync_block.", "vis_projector.", "mlp_vis.", "aud_projector.", "mlp_aud.")      # what sync=True adds
CONTRAST_DIM, CONTRAST_HIDDEN = 512, 2048    # the slab's width (and the predictor's waist) and the projectors' width
# one modality's 18 tensors in module order: projector [0] [1] [3] [4] [6] [7], predictor [0] [1] [3]; weight and bias each
CONTRAST_TENSORS = tuple("%s.%d.%s" % (m, i, n) for m, idx in (("projector", (0, 1, 3, 4, 6, 7)), ("mlp", (0, 1, 3)))
                         for i in idx for n in ("weight", "bias"))
_CONTRAST_ACTS = (E.ACT_RELU, E.ACT_RELU, E.ACT_NONE, E.ACT_RELU)      # behind the four LayerNorms


def pack_contrast_side(ts):
    """The plan of one modality's projector and predictor from its 18 tensors (CONTRAST_TENSORS order): four (Linear pack,
    LayerNorm weight, LayerNorm bias) and the last Linear's pack: the list AudioVisualSaliencyModel._pack holds as pk["vis"] /
    pk["aud"], here from the live values for ContrastHead.forward.  _pack does not call it: the inference path's text is left as
    it was (DESIGN.md section 7 says why), and tests/test_sync_train.py holds the two to the same bits."""
    def f(t):
        return t.detach().float().contiguous()
    return [(E.pack_conv(ts[4 * i], ts[4 * i + 1]), f(ts[4 * i + 2]), f(ts[4 * i + 3])) for i in range(4)] + \
        [E.pack_conv(ts[16], ts[17])]


def contrast_embed_forward(p, x):
    """projector (Linear-LN-ReLU x2, Linear-LN) then predictor (Linear-LN-ReLU, Linear) on the [B,512] rows x with the plan p
    (pack_contrast_side): (emb, pred, zs, ys) -- the embedding, the prediction, the four Linear outputs in front of a LayerNorm
    and the four rows behind them (ys[2] is emb), which the backward reads and inference drops."""
    zs, ys = [], []
    for i, act in enumerate(_CONTRAST_ACTS):
        zs.append(E.conv(x, p[i][0]))
        x = E.layernorm(zs[-1], p[i][1], p[i][2], LN_EPS, act=act)
        ys.append(x)
    return ys[2], E.conv(x, p[4]), zs, ys


def contrast_forward(vis_fea, aud_fea, pv, pa):
    """The launches of the contrastive side branch of AudioVisualSaliencyModel._sync_and_lateral3, restated, on the two token
    views of the slab and the two plans: (loss [1], pooled [2,B,512], the two contrast_embed_forward results)."""
    B, dev = vis_fea.N, vis_fea.buf.device
    pooled = torch.empty(2, B, CONTRAST_DIM, dtype=torch.float32, device=dev)
    E.mean_rows(vis_fea, B, vis_fea.T * vis_fea.H * vis_fea.W, pooled[0])
    E.mean_rows(aud_fea, B, aud_fea.T * aud_fea.H * aud_fea.W, pooled[1])
    vis = contrast_embed_forward(pv, E.from_rows(pooled[0]))
    aud = contrast_embed_forward(pa, E.from_rows(pooled[1]))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    E.neg_cosine(vis[1], aud[0], loss, 0.5, False)
    E.neg_cosine(aud[1], vis[0], loss, 0.5, True)
    return loss, pooled, vis, aud


class ContrastHead(torch.autograd.Function):
    """loss_av = ContrastHead.apply(slab, Rv, *36 tensors): the contrastive head (model/model_utils.py:545-552 upstream) on the
    SyncBlock's slab, fp32 [B, Rv+Ra, 512] on the GPU, its first Rv rows the visual tokens: the mean over each modality's tokens,
    projector and predictor, and 0.5 mean -cos(p_vis, z_aud) + 0.5 mean -cos(p_aud, z_vis), 0-dim.  The tensors: vis_projector,
    mlp_vis, aud_projector, mlp_aud, each in module order (CONTRAST_TENSORS).  The forward restates the contrastive launches of
    AudioVisualSaliencyModel._sync_and_lateral3 (contrast_forward) from packs of the live values (pack_contrast_side); the
    value has the bits of the inference path's second return.  It keeps the two pooled rows, every Linear output in front of a
    LayerNorm and the rows behind them.  The embeddings enter the loss only as the detached z (upstream's D(p, z.detach())), so
    the gradient flows through the two predictions alone.  Backward per modality: neg_cosine_bwd; through predictor and
    projector E.linear_wgrad for the five Linears, E.conv on _pack_t at PREC_F32 for their data gradients and
    layernorm_act_bwd for the four LayerNorms (three under the ReLU's mask); mean_rows_bwd into that modality's row range of one
    dslab.  Each gradient only when it is asked for.  No double backward."""

    @staticmethod
    def forward(ctx, slab, Rv, *ts):
        _check_input(slab)
        D, Hd = CONTRAST_DIM, CONTRAST_HIDDEN
        if slab.dim() != 3 or slab.dtype != torch.float32 or slab.shape[2] != D or not 0 < Rv < slab.shape[1]:
            raise MspiError("ContrastHead: slab must be fp32 [B, Rv+Ra, %d] with 0 < Rv = %s < Rv+Ra, got %s %s"
                            % (D, Rv, slab.dtype, tuple(slab.shape)))
        if len(ts) != 36:
            raise MspiError("ContrastHead: expected 36 tensors after Rv (vis_projector, mlp_vis, aud_projector, mlp_aud), got %d" % len(ts))
        want = ((Hd, D), (Hd,), (Hd,), (Hd,), (Hd, Hd), (Hd,), (Hd,), (Hd,), (Hd, Hd), (Hd,), (Hd,), (Hd,),
                (D, Hd), (D,), (D,), (D,), (Hd, D), (Hd,))
        for side, off in (("vis", 0), ("aud", 18)):
            for name, t, shape in zip(CONTRAST_TENSORS, ts[off:off + 18], want):
                if tuple(t.shape) != shape or t.device != slab.device:
                    raise MspiError("ContrastHead: %s %s is %s on %s, the head has %s on %s"
                                    % (side, name, tuple(t.shape), t.device, shape, slab.device))
        slab = slab.detach().contiguous()
        B, R, _ = slab.shape
        with torch.no_grad():
            x = E.CL(slab.view(-1), 0, B, R, 1, 1, D, D)
            loss, pooled, vis, aud = contrast_forward(x.tokens(0, Rv, 1, 1), x.tokens(Rv, R - Rv, 1, 1),
                                                      pack_contrast_side(ts[:18]), pack_contrast_side(ts[18:]))
        kept = [pooled]
        for emb, pred, zs, ys in (vis, aud):
            kept += [pred.buf] + [z.buf for z in zs] + [y.buf for y in ys]
        ctx.save_for_backward(*kept, *ts)
        ctx.geom = (B, R, Rv)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        saved = ctx.saved_tensors
        B, R, Rv = ctx.geom
        D = CONTRAST_DIM
        need = ctx.needs_input_grad
        pooled, kept, ts = saved[0], saved[1:19], saved[19:]
        g = G.detach().float().reshape(1).contiguous()
        grads = [None] * 38
        dslab = None
        if need[0]:
            dslab = E.alloc(B, R, 1, 1, D, pooled.device)
        for side, (r0, rows) in enumerate(((0, Rv), (Rv, R - Rv))):
            first = 2 + 18 * side                                       # this modality's tensors in the argument list
            w = ts[18 * side:18 * side + 18]
            asked = [need[first + 4 * i] or need[first + 4 * i + 1] for i in range(5)]       # the five Linears
            asked_ln = [need[first + 4 * i + 2] or need[first + 4 * i + 3] for i in range(4)]
            lo_lin = min([i for i in range(5) if asked[i]] + [9])       # the lowest Linear and LayerNorm asked for
            lo_ln = min([i for i in range(4) if asked_ln[i]] + [9])
            if not need[0] and lo_lin == lo_ln == 9:
                continue
            mine, other = kept[9 * side:9 * side + 9], kept[9 * (1 - side):9 * (1 - side) + 9]

            def rows_of(buf):
                return E.from_rows(buf.view(B, -1))
            pred, zs, ys = rows_of(mine[0]), [rows_of(t) for t in mine[1:5]], [rows_of(t) for t in mine[5:9]]
            xs = [rows_of(pooled[side])] + ys                           # the five Linears' inputs
            d = E.neg_cosine_bwd(pred, rows_of(other[7]), g, 0.5)       # other[7]: the other modality's embedding, detached
            for i in range(4, -1, -1):
                if asked[i]:
                    dW, db = E.linear_wgrad(xs[i], d)
                    grads[first + 4 * i], grads[first + 4 * i + 1] = dW, db
                if not (need[0] or lo_lin < i or lo_ln < i):            # nothing below this Linear is asked for
                    break
                d = E.conv(d, _pack_t(w[4 * i]))                        # the gradient of the Linear's input
                if i == 0:
                    E.mean_rows_bwd(d.as_rows(), dslab.tokens(r0, rows, 1, 1))
                    break
                d, dgam, dbet = E.layernorm_act_bwd(d, zs[i - 1], w[4 * i - 2].detach().float().contiguous(), LN_EPS,
                                                    y=ys[i - 1] if _CONTRAST_ACTS[i - 1] == E.ACT_RELU else None, inplace=True)
                grads[first + 4 * i - 2], grads[first + 4 * i - 1] = dgam, dbet
        if need[0]:
            grads[0] = dslab.as_rows().view(B, R, D)
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


def compose_lateral(w0, b0, w1):
    """(s,1,1)/s conv after a 1x1x1 conv, no nonlinearity between: one conv with
    W[co,ci,tap] = sum_m W1[co,m,tap] W0[m,ci],  b[co] = sum_{tap,m} W1[co,m,tap] b0[m], composed in fp64."""
    w0 = w0.detach().double().flatten(1)                         # [mid, cin]
    w1 = w1.detach().double()[:, :, :, 0, 0]                      # [co, mid, s]
    w = torch.einsum("omt,mi->oit", w1, w0)[:, :, :, None, None]  # [co, cin, s, 1, 1]
    b = torch.einsum("omt,m->o", w1, b0.detach().double())
    return w.float(), b.float()


def pack_lateral_entry(w0, b0, w1, stride, split=None):
    """The pack(s) of a lateral's entry conv(s) from the tensors in their nn layouts (w1 None: no second conv): what
    _SaliencyBase._pack_lateral holds and what LateralEntry.forward builds from the live values, so the two cannot drift.
    split = C4: the input arrives as two tensors, so the K range is cut in two, the bias on the first part."""
    if w1 is not None:
        w, b = compose_lateral(w0, b0, w1)
    else:
        w, b, stride = w0.detach().float(), b0.detach().float(), (1, 1, 1)
    if split is None:
        return (E.pack_conv(w, b, None, stride, (0, 0, 0)),)
    return (E.pack_conv(w[:, :split].contiguous(), b, None, stride, (0, 0, 0)),
            E.pack_conv(w[:, split:].contiguous(), None, None, stride, (0, 0, 0)))


def _cl_view(name, t):
    """A CL over the tensor t [B,T,h,w,C] as it lies in memory: frames, lines and positions nested (a channel slice of a wider
    buffer keeps its row stride), any sample stride (a token view into a slab)."""
    _check_input(t, "LateralEntry: %s" % name)
    B, T, h, w, c = t.shape
    sN, sT, sH, sW, sC = t.stride()
    if sC != 1 or sW % 4 or sW < c or sH != w * sW or sT != h * sH or sN % 4 or t.data_ptr() % 16:
        t = t.contiguous()
        sN, sW = T * h * w * c, c
    return E.CL(t, 0, B, T, h, w, c, sW, sN)


def _entry_dgrad(G, wc, c0, c, T):
    """The data gradient of the composed entry conv wc [Co, Cin, s, 1, 1] (kernel == stride along T) for its input channels
    [c0, c0 + c) from the output gradient G, a dense CL [B,T',h,w,Co]: dense fp32 [B,T,h,w,c], the frames beyond s T' zero."""
    Co, _, s = wc.shape[:3]
    if c % 4:
        raise MspiError("LateralEntry: the data gradient of an input of %d channels is not built (C %% 4 != 0)" % c)
    B, Tp, h, w = G.N, G.T, G.H, G.W
    hw = h * w
    rows = E.conv(G, E.pack_conv(wc[:, c0:c0 + c, :, 0, 0].permute(2, 1, 0).reshape(s * c, Co).contiguous(), None, prec=E.PREC_F32))
    if s == 1:                                                # rows (b, t, p) x ci: the gradient as it stands
        dx = rows.as_rows().view(B, Tp, h, w, c)
    else:                                                     # rows (b, t', p) x (tap, ci): the tap slabs to their frames
        dx = E.permute(rows, (B, Tp, s, hw, c), (Tp * hw * s * c, hw * s * c, c, s * c, 1)).view(B, Tp * s, h, w, c)
    if T == Tp * s:
        return dx
    out = torch.zeros(B, T, h, w, c, dtype=torch.float32, device=dx.device)
    out[:, :Tp * s] = dx
    return out


class LateralEntry(torch.autograd.Function):
    """y = LateralEntry.apply(x, x2, w0, b0, w1): the entry conv(s) of a lateral on x, channels-last fp32 [B,T,h,w,C] on the GPU
    (a channel slice of a wider buffer or a token view into a slab is read where it lies), and, x2 not None, on the concat
    [x | x2] without materialising it.  w0 [192,C(+C2),1,1,1] and b0 of latlayer_k[0]; w1 [192,192,s,1,1] of latlayer_k[1] or
    None, s in {1, 2, 4}.  The forward composes the two convs in fp64 from the live tensors, packs as _SaliencyBase._pack_lateral
    does and launches what _SaliencyBase._lateral launches, so y [B,T//s,h,w,192] has the bits of the inference path.  The
    backward takes dWc, dbc of the COMPOSED conv from mspi_conv_wgrad_entry and applies the chain rule through the composition
        dW1[co,m,t] = sum_ci dWc[co,ci,t] W0[m,ci] + dbc[co] b0[m]
        dW0[m,ci]   = sum_{co,t} W1[co,m,t] dWc[co,ci,t],   db0[m] = sum_{co,t} W1[co,m,t] dbc[co]
    as two GEMMs on the fp32 MFMA path (E.conv at PREC_F32), the bias terms riding as one more column / row; without w1,
    dW0 = dWc and db0 = dbc.  Gradients: w0, b0, w1, and x and x2 each only when it requires grad (x2 under
    trainable(..., sync=True), where it is the visual tokens of the SyncBlock's slab): kernel == stride along T, so
        dX[b, s t' + tap, p, ci] = sum_co G[b, t', p, co] Wc[co, ci, tap]
    is one GEMM of the rows (b, t', p) at PREC_F32 with the s C columns (tap, ci), whose s tap slabs E.permute then moves to
    their frames (as ReadoutTail does for d y4); frames beyond s floor(T / s) are zero.  A dense [B,T,h,w,C] tensor is returned
    and torch's view backward places x2's into the slab.  With both inputs detached nothing more is launched and dW0, db0, dW1
    keep their bits.  No double backward."""

    @staticmethod
    def forward(ctx, x, x2, w0, b0, w1):
        _check_input(x, beside=x2)
        xc = _cl_view("x", x.detach())
        xc2 = None if x2 is None else _cl_view("x2", x2.detach())
        cin = xc.C + (xc2.C if xc2 is not None else 0)
        mid = w0.shape[0]
        if w0.dim() != 5 or tuple(w0.shape[1:]) != (cin, 1, 1, 1) or tuple(b0.shape) != (mid,) or w0.device != x.device:
            raise MspiError("LateralEntry: latlayer[0] is %s / %s on %s, the input has %d channels on %s"
                            % (tuple(w0.shape), tuple(b0.shape), w0.device, cin, x.device))
        s = 1
        if w1 is not None:
            s = w1.shape[2] if w1.dim() == 5 else 0
            if w1.dim() != 5 or tuple(w1.shape) != (w1.shape[0], mid, s, 1, 1) or s not in (1, 2, 4) or w1.device != x.device:
                raise MspiError("LateralEntry: latlayer[1] is %s, not an (s,1,1) conv over %d channels with s in {1, 2, 4}"
                                % (tuple(w1.shape), mid))
        if xc2 is not None and (xc2.N, xc2.T, xc2.H, xc2.W) != (xc.N, xc.T, xc.H, xc.W):
            raise MspiError("LateralEntry: x2 %s does not have the extent of x %s" % (tuple(x2.shape), tuple(x.shape)))
        if xc.T < s:
            raise MspiError("LateralEntry: %d frames under a temporal kernel of %d" % (xc.T, s))
        with torch.no_grad():
            pks = pack_lateral_entry(w0, b0, w1, (s, 1, 1), None if xc2 is None else xc.C)
            y = E.conv(xc, pks[0])
            if xc2 is not None:
                y = E.conv(xc2, pks[1], res=y)
        views = [xc] + ([] if xc2 is None else [xc2])
        ctx.save_for_backward(*[v.buf for v in views], w0, b0, *([] if w1 is None else [w1]))
        ctx.dims = [(v.N, v.T, v.H, v.W, v.C, v.ld, v.sN) for v in views]
        ctx.has1 = w1 is not None
        ctx.geoms = [_geometry((s, 1, 1), (0, 0, 0), p.cin, p.cout_s, (s, 1, 1)) for p in pks]
        return y.as_nthwc()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        saved = list(ctx.saved_tensors)
        views = [E.CL(saved.pop(0), 0, *dims) for dims in ctx.dims]
        xc, xc2, has2, has1 = views[0], views[-1], len(views) == 2, ctx.has1
        w0, b0 = saved[0], saved[1]
        w1 = saved[2] if has1 else None
        need = ctx.needs_input_grad
        if not any(need):
            return None, None, None, None, None
        Gc = _cl5(G.float().contiguous())
        dxs = [None, None]
        if need[0] or (has2 and need[1]):
            wc = compose_lateral(w0, b0, w1)[0] if has1 else w0.detach().float()
            if need[0]:
                dxs[0] = _entry_dgrad(Gc, wc, 0, xc.C, xc.T)
            if has2 and need[1]:
                dxs[1] = _entry_dgrad(Gc, wc, xc.C, xc2.C, xc2.T)
        if not any(need[2:]):
            return dxs[0], dxs[1], None, None, None
        # raw [Co][s][Ci] blocks of the composed conv's gradient, the two inputs' column blocks side by side; dbc once
        dWc, dbc = E.conv_wgrad_entry(xc, Gc, ctx.geoms[0])
        if has2:
            dWc = torch.cat([dWc, E.conv_wgrad_entry(xc2, Gc, ctx.geoms[1])[0]], dim=1)
        if not has1:
            return dxs[0], dxs[1], (dWc.contiguous() if need[2] else None), (dbc if need[3] else None), None
        Co, Ci, s = dWc.shape[:3]
        mid = w0.shape[0]
        dev = dWc.device
        rows = dWc[:, :, :, 0, 0].permute(0, 2, 1)                                    # [Co, s, Ci]
        dw0 = db0 = dw1 = None
        if need[4]:
            # rows (co, t), K = Ci and one more column for the bias term (padded to four), N = mid
            a = torch.zeros(Co * s, Ci + 4, dtype=torch.float32, device=dev)
            a[:, :Ci] = rows.reshape(Co * s, Ci)
            a[:, Ci] = dbc.repeat_interleave(s)
            wb = torch.zeros(mid, Ci + 4, dtype=torch.float32, device=dev)
            wb[:, :Ci] = w0.detach().float().flatten(1)
            wb[:, Ci] = b0.detach().float()
            out = E.conv(E.from_rows(a), E.pack_conv(wb, None, prec=E.PREC_F32))      # [Co s, mid]
            dw1 = out.as_rows(mid).reshape(Co, s, mid).permute(0, 2, 1)[:, :, :, None, None]
        if need[2] or need[3]:
            # rows ci and one more for db0, K = (co, t), N = mid
            a = torch.empty(Ci + 1, Co * s, dtype=torch.float32, device=dev)
            a[:Ci] = rows.permute(2, 0, 1).reshape(Ci, Co * s)
            a[Ci] = dbc.repeat_interleave(s)
            wt = w1.detach().float()[:, :, :, 0, 0].permute(1, 0, 2).reshape(mid, Co * s).contiguous()
            out = E.conv(E.from_rows(a), E.pack_conv(wt, None, prec=E.PREC_F32)).as_rows(mid)      # [Ci + 1, mid]
            dw0, db0 = out[:Ci].t()[:, :, None, None, None], out[Ci]
        grads = (dxs[0], dxs[1], dw0, db0, dw1)
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))


ADAPTER_LAYERS = ("b0", "b1a", "b1s", "b1t", "b2a", "b2s", "b2t", "b3")      # branch0 | branch1: 1x1x1, conv_s, conv_t | branch2 | branch3
_ADAPTER_KERNEL = {"s": ((1, 3, 3), (0, 1, 1)), "t": ((3, 1, 1), (1, 0, 0))}
_ADAPTER_CHAINS = (("b0",), ("b1a", "b1s", "b1t"), ("b2a", "b2s", "b2t"), ("b3",))


def adapter_wgrad_route(rows, cin, cout):
    """"t16" or "wide": which kernel adapter_wgrad calls.  Measured on one MI355X (tools/adapter_bench.py,
    profiles/r20_adapter.txt): at 2 688 rows (two clips) mspi_conv_wgrad_t16 is the faster on all three layers the wide kernel
    takes (416 -> 192: 0.087 against 0.095 ms, 416 -> 96: 0.068 / 0.092, 416 -> 64: 0.060 / 0.099); at 10 752 rows (eight clips)
    it LOSES on all three (0.165 / 0.110, 0.129 / 0.099, 0.114 / 0.101).  The switch sits at the row count from which the new
    kernel takes its longest slices, between the two measured points; nothing in between was measured.  The other five layers
    have widths the wide kernel refuses and go to the new kernel at every size."""
    wide_takes = cin % 32 == 0 and cout % 32 == 0 and cout <= WGRAD_WIDE_MAX_CH
    return "wide" if wide_takes and rows >= E.WGRAD_T16_ROWS[1] else "t16"


def adapter_wgrad(x, dz, geo):
    """The weight gradient of one adapter layer (no bias), by the route adapter_wgrad_route names."""
    if adapter_wgrad_route(x.M, geo.cin, geo.cout) == "wide":
        return wgrad_wide_sliced(x, dz, geo.k, geo.pad)[0]
    return E.conv_wgrad_t16(x, dz, geo)[0]


class Adapter(torch.autograd.Function):
    """masks = Adapter.apply(cat, *tensors, *bns): the adapter's Inception (Adapter.conv, backbones/s3d.py upstream) on cat, the
    416-wide input Adapter.run assembles, channels-last fp32 [B,T,h,w,Cin] on the GPU.  tensors: for each of the eight layers in
    ADAPTER_LAYERS order conv.weight, bn.weight, bn.bias in their nn layouts (24); bns: for each layer (running_mean,
    running_var, num_batches_tracked), updated in place as nn.BatchNorm3d.train() with momentum 0.001 updates them, or None to
    skip that; the normalisation is on BATCH statistics either way (eps 1e-3).  Every width a multiple of 16, Cin <= 416, the
    others <= 208.  The forward runs, per layer, the unfolded conv, bn_stats and bn_apply with its ReLU -- layers wider than the
    BatchNorm kernels take in channel slices of a strided view -- the four branches writing their slices of one output
    [B,T,h,w,c0+c1+c2+c3]; branch3's 3x3x3 max-pool is forward only.  Backward per layer: bn_bwd under the ReLU mask, the weight
    gradient (adapter_wgrad: mspi_conv_wgrad_t16, or from 8192 rows on mspi_conv_wgrad_wide_fwd on the three layers it takes and was
    measured faster on), and through conv_t and conv_s the data gradient as the same conv on the flipped weights at
    PREC_F32.  Gradients: the 24 tensors.  cat gets NONE: the image encoder is frozen, as upstream.  No double backward."""

    @staticmethod
    def forward(ctx, cat, *rest):
        if len(rest) != 32:
            raise MspiError("Adapter: expected 24 tensors and 8 BatchNorm buffer triples after cat, got %d arguments" % len(rest))
        _check_input(cat, "Adapter: cat")
        ps = {l: rest[3 * i:3 * i + 3] for i, l in enumerate(ADAPTER_LAYERS)}
        bns = dict(zip(ADAPTER_LAYERS, rest[24:]))
        B, T, h, w, cin = cat.shape
        geos, src = {}, {}
        for chain in _ADAPTER_CHAINS:
            c = cin
            for l in chain:
                k, pad = _ADAPTER_KERNEL.get(l[2:], ((1, 1, 1), (0, 0, 0)))
                wl, gam, bet = ps[l]
                co = wl.shape[0] if wl.dim() == 5 else -1
                if wl.dim() != 5 or tuple(wl.shape) != (co, c) + k or gam.numel() != co or bet.numel() != co or wl.device != cat.device:
                    raise MspiError("Adapter: layer %s has conv.weight %s, BatchNorm %d / %d on %s; it reads %d channels through a "
                                    "%s kernel on %s" % (l, tuple(wl.shape), gam.numel(), bet.numel(), wl.device, c, k, cat.device))
                if c % 16 or co % 16 or c > E.WGRAD_T16_MAX_CIN or co > E.WGRAD_T16_MAX_COUT:
                    raise MspiError("Adapter: layer %s is %d -> %d wide; the widths must be multiples of 16, at most %d in and %d out"
                                    % (l, c, co, E.WGRAD_T16_MAX_CIN, E.WGRAD_T16_MAX_COUT))
                geos[l], src[l] = (k, pad, c, co), (None if l == chain[0] else prev)
                c, prev = co, l
        widths = [geos[chain[-1]][3] for chain in _ADAPTER_CHAINS]
        cat = cat.detach().contiguous()
        saved, stats = [cat], {}
        with torch.no_grad():
            x0 = _cl5(cat)
            pooled = E.maxpool(x0, (3, 3, 3), (1, 1, 1), (1, 1, 1))
            out = E.alloc(B, T, h, w, sum(widths), cat.device)
            ys, c0 = {}, 0
            for chain, cw in zip(_ADAPTER_CHAINS, widths):
                for l in chain:
                    k, pad, _, co = geos[l]
                    x = (pooled if l == "b3" else x0) if src[l] is None else ys[src[l]]
                    z = E.conv(x, E.pack_conv(ps[l][0], None, None, (1, 1, 1), pad, E.ACT_NONE))
                    y = out.slice(c0, co) if l == chain[-1] else E.alloc(B, T, h, w, co, cat.device)
                    _, mean, var, rstd = bn_relu_train(z, ps[l][1], ps[l][2], SA_BN_EPS, out=y)
                    _bn_running(bns[l], mean, var, z.M, SA_BN_MOMENTUM)
                    ys[l], stats[l] = y, (z.buf, mean, rstd, ps[l][1].detach().float().contiguous())
                c0 += cw
        for l in ADAPTER_LAYERS:
            saved += [stats[l][0], ys[l].buf, stats[l][1], stats[l][2], stats[l][3], ps[l][0]]
        ctx.save_for_backward(*saved, pooled.buf)
        ctx.dims, ctx.geos, ctx.widths = (B, T, h, w), geos, widths
        return out.as_nthwc()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        saved = list(ctx.saved_tensors)
        B, T, h, w = ctx.dims
        geos, widths = ctx.geos, ctx.widths
        need = ctx.needs_input_grad
        grads = [None] * 33
        if not any(need[1:25]):
            return tuple(grads)
        cat, pooled = saved[0], saved[-1]
        Cm = sum(widths)

        def cl(buf, c, ld=None, off=0):
            return E.CL(buf.view(-1), off, B, T, h, w, c, c if ld is None else ld)
        Gc = cl(G.float().contiguous(), Cm)
        t = {l: saved[1 + 6 * i:7 + 6 * i] for i, l in enumerate(ADAPTER_LAYERS)}
        c0 = 0
        for chain, cw in zip(_ADAPTER_CHAINS, widths):
            dy = Gc.slice(c0, cw)
            for j in range(len(chain) - 1, -1, -1):
                l = chain[j]
                i = ADAPTER_LAYERS.index(l)
                k, pad, c, co = geos[l]
                zb, yb, mean, rstd, gam, wl = t[l]
                z = cl(zb, co)
                y = cl(yb, co, Cm, c0) if j == len(chain) - 1 else cl(yb, co)       # a branch's last output lies in its slice of masks
                if not any(need[1 + 3 * i2] or need[2 + 3 * i2] or need[3 + 3 * i2] for i2 in (ADAPTER_LAYERS.index(q) for q in chain[:j + 1])):
                    break                                                           # nothing further down this branch is asked for
                dz = E.alloc(B, T, h, w, co, cat.device)
                dgam, dbet = (torch.empty(co, dtype=torch.float32, device=cat.device) for _ in range(2))
                for s0, sc in _bn_slices(co):
                    _, dg, dbt = E.bn_bwd(dy.slice(s0, sc), z.slice(s0, sc), mean[s0:s0 + sc].contiguous(), rstd[s0:s0 + sc].contiguous(),
                                          gam[s0:s0 + sc].contiguous(), y=y.slice(s0, sc), dx=dz.slice(s0, sc))
                    dgam[s0:s0 + sc], dbet[s0:s0 + sc] = dg, dbt
                if j == 0:
                    x = cl(pooled, c) if l == "b3" else cl(cat, c)
                else:
                    x = cl(t[chain[j - 1]][1], c)
                grads[1 + 3 * i] = adapter_wgrad(x, dz, _geometry(k, pad, c, co)).contiguous()
                grads[2 + 3 * i], grads[3 + 3 * i] = dgam, dbet
                if j:
                    dy = E.conv(dz, _pack_dgrad(wl, pad))
            c0 += cw
        return tuple(g if g is None or need[i] else None for i, g in enumerate(grads))


# ------------------------------------------------------------------------------------------------ X3D residual block
X3D_BLOCK_TENSORS = ("a.weight", "a_bn.weight", "a_bn.bias", "b.weight", "b_bn.weight", "b_bn.bias", "se.fc1.weight", "se.fc1.bias",
                     "se.fc2.weight", "se.fc2.bias", "c.weight", "c_bn.weight", "c_bn.bias")


def _bn_stats_sliced(x, eps):
    """(mean, biased var, rstd) of the CL x over _bn_slices(x.C)."""
    stats = [E.bn_stats(x.slice(c0, c), eps) for c0, c in _bn_slices(x.C)]
    return stats[0] if len(stats) == 1 else tuple(torch.cat(ts) for ts in zip(*stats))


def _bn_bwd_sliced(dy, x, mean, rstd, gamma, y=None):
    """E.bn_bwd over _bn_slices(x.C): (dx, a new CL like x, dgamma, dbeta)."""
    dev = x.buf.device
    dx = E.alloc(x.N, x.T, x.H, x.W, x.C, dev)
    dgam, dbet = (torch.empty(x.C, dtype=torch.float32, device=dev) for _ in range(2))
    for c0, c in _bn_slices(x.C):
        _, dg, db = E.bn_bwd(dy.slice(c0, c), x.slice(c0, c), mean[c0:c0 + c].contiguous(), rstd[c0:c0 + c].contiguous(),
                             gamma[c0:c0 + c].contiguous(), y=None if y is None else y.slice(c0, c), dx=dx.slice(c0, c))
        dgam[c0:c0 + c], dbet[c0:c0 + c] = dg, db
    return dx, dgam, dbet


def _bn_relu_sliced(x, mean, rstd, gamma, beta):
    """relu(bn(x)) on given statistics by bn_relu_train's launches: E.bn_apply over _bn_slices(x.C), the forward's bits."""
    out = E.alloc(x.N, x.T, x.H, x.W, x.C, x.buf.device)
    for c0, c in _bn_slices(x.C):
        E.bn_apply(x.slice(c0, c), mean[c0:c0 + c].contiguous(), rstd[c0:c0 + c].contiguous(), gamma[c0:c0 + c].contiguous(),
                   beta[c0:c0 + c].contiguous(), act=E.ACT_RELU, out=out.slice(c0, c))
    return out


class X3DBlock(torch.autograd.Function):
    """y = X3DBlock.apply(x, wa, ga, ba, wb, gb, bb, w1, b1, w2, b2, wc, gc, bc, bn_a, bn_b, bn_c): one stride-1 X3D residual
    block without branch1 (SlowFast/resnet_helper.py:213-360, 490-616 upstream) with its three BatchNorm layers on BATCH
    statistics (eps 1e-5):
        z_a = a(x); t = relu(bn_a(z_a)); v0 = b(t); v = bn_b(v0); g = sigmoid(fc2(relu(fc1(mean_THW(v))))); s = swish(v g);
        z_c = c(s); y = relu(x + bn_c(z_c)).
    x fp32 channels-last [B,T,h,w,dim_out] on the GPU; the tensors in their nn layouts, X3D_BLOCK_TENSORS order; w1, b1, w2, b2
    None for a block without `se` (g = 1).  bn_*: (running_mean, running_var, num_batches_tracked), updated in place as
    nn.BatchNorm3d.train() with momentum 0.1 updates them, or None to skip that.  dim_out a multiple of 32 and dim_inner of 4
    (what mspi_linear_wgrad takes), at least two rows.  The forward runs the unfolded convs on packs of the live values, bn_stats
    over _bn_slices, and keeps x, the pre-norm z_a, v0, z_c, the output y, the statistics and the SE's p, h, gate; t and s are
    computed again in the backward.  Backward: bn_bwd under y's mask, linear_wgrad for `c` and (operands exchanged, then
    transposed: dim_inner need not be a multiple of 32) for `a`, the data gradients on _pack_t at PREC_F32, gate_swish_bwd,
    se_train_bwd and mean_rows_bwd, dwconv3_wgrad, the depthwise conv on the flipped taps, relu_mask_add for the skip path.
    Gradients: x and the 13 tensors, each only when it requires grad.  No double backward."""

    @staticmethod
    def forward(ctx, x, wa, ga, ba, wb, gb, bb, w1, b1, w2, b2, wc, gc, bc, bn_a, bn_b, bn_c):
        if x.dim() != 5 or x.dtype != torch.float32:
            raise MspiError("X3DBlock: x must be fp32 [B,T,h,w,dim_out] (channels-last), got %s %s" % (x.dtype, tuple(x.shape)))
        B, T, h, w, D = x.shape
        Ci = wa.shape[0] if wa.dim() == 5 else -1
        se = [t is not None for t in (w1, b1, w2, b2)]
        if any(se) != all(se):
            raise MspiError("X3DBlock: se.fc1 / se.fc2 must be given whole (four tensors) or not at all (four None)")
        se = all(se)
        F = b1.numel() if se else 0
        want = ((Ci, D, 1, 1, 1), (Ci,), (Ci,), (Ci, 1, 3, 3, 3), (Ci,), (Ci,), (F, Ci, 1, 1, 1), (F,), (Ci, F, 1, 1, 1), (Ci,),
                (D, Ci, 1, 1, 1), (D,), (D,))
        for name, t, shape in zip(X3D_BLOCK_TENSORS, (wa, ga, ba, wb, gb, bb, w1, b1, w2, b2, wc, gc, bc), want):
            if t is not None and (tuple(t.shape) != shape or t.device != x.device):
                raise MspiError("X3DBlock: %s is %s on %s, a block %d -> %d -> %d wide%s has %s on %s"
                                % (name, tuple(t.shape), t.device, D, Ci, D, " with an SE of %d" % F if se else "", shape, x.device))
        if D % 32 or Ci % 4 or Ci <= 0:
            raise MspiError("X3DBlock: dim_out / dim_inner = %d / %d: dim_out must be a multiple of 32 and dim_inner of 4 "
                            "(X3D-L stages 4 and 5: 96 / 216, 192 / 432)" % (D, Ci))
        if se and not 0 < F <= E.SE_TRAIN_MAX_F:
            raise MspiError("X3DBlock: se.fc1 has %d output channels, at most %d" % (F, E.SE_TRAIN_MAX_F))
        M = B * T * h * w
        if M < 2:
            raise MspiError("X3DBlock: BatchNorm on batch statistics needs more than one row (B T h w = %d), as torch refuses it" % M)
        _check_input(x)

        def f(t):
            return t.detach().float().contiguous()
        x = x.detach().contiguous()
        dev = x.device
        with torch.no_grad():
            xc = _cl5(x)
            z_a = E.conv(xc, E.pack_conv(wa, None, None, (1, 1, 1), (0, 0, 0), E.ACT_NONE))
            t, ma, va, ra = bn_relu_train(z_a, ga, ba, BN_EPS)
            _bn_running(bn_a, ma, va, M, BN_MOMENTUM)
            v0 = E.dwconv(t, E.pack_dwconv(wb, None, None, (1, 1, 1), (1, 1, 1), E.ACT_NONE))
            mb, vb, rb = _bn_stats_sliced(v0, BN_EPS)
            _bn_running(bn_b, mb, vb, M, BN_MOMENTUM)
            p = hid = gate = None
            if se:
                pool0 = E.mean_rows(v0, B, T * h * w, torch.empty(B, Ci, dtype=torch.float32, device=dev))
                p, hid, gate = E.se_train_fwd(pool0, mb, rb, f(gb), f(bb), f(w1), f(b1), f(w2), f(b2))
            s = E.bn_gate_act(v0, mb, rb, f(gb), f(bb), gate=gate, act=E.ACT_SWISH)
            z_c = E.conv(s, E.pack_conv(wc, None, None, (1, 1, 1), (0, 0, 0), E.ACT_NONE))
            mc, vc, rc = _bn_stats_sliced(z_c, BN_EPS)
            _bn_running(bn_c, mc, vc, M, BN_MOMENTUM)
            y = E.bn_gate_act(z_c, mc, rc, f(gc), f(bc), res=xc, act=E.ACT_RELU)
        ctx.se = se
        ctx.save_for_backward(x, z_a.buf, v0.buf, z_c.buf, y.buf, ma, ra, mb, rb, mc, rc, wa, ga, ba, wb, gb, bb, wc, gc,
                              *((p, hid, gate, w1, w2) if se else ()))
        ctx.geom = tuple((c.off, c.ld) for c in (z_a, v0, z_c, y))
        return y.as_nthwc()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        saved = ctx.saved_tensors
        x, zab, v0b, zcb, yb, ma, ra, mb, rb, mc, rc, wa, ga, ba, wb, gb, bb, wc, gc = saved[:19]
        B, T, h, w, D = x.shape
        Ci = wa.shape[0]
        need = ctx.needs_input_grad
        grads = [None] * 17
        if not any(need[:14]):
            return tuple(grads)

        def f(t):
            return t.detach().float().contiguous()

        def cl(buf, c, geom=None):
            off, ld = (0, c) if geom is None else geom
            return E.CL(buf.view(-1), off, B, T, h, w, c, ld)
        z_a, v0, z_c, y = (cl(b, c, g) for b, c, g in zip((zab, v0b, zcb, yb), (Ci, Ci, D, D), ctx.geom))
        xc, Gc = cl(x, D), cl(G.float().contiguous(), D)
        gate = saved[21] if ctx.se else None
        dz_c, grads[12], grads[13] = _bn_bwd_sliced(Gc, z_c, mc, rc, f(gc), y=y)                 # the block's output is the mask
        if need[11]:
            s = E.bn_gate_act(v0, mb, rb, f(gb), f(bb), gate=gate, act=E.ACT_SWISH)
            grads[11] = E.linear_wgrad(s, dz_c, bias=False)[0].view(D, Ci, 1, 1, 1)
        if any(need[:11]):
            ds = E.conv(dz_c, _pack_t(wc))
            dv, dgate = E.gate_swish_bwd(ds, v0, mb, rb, f(gb), f(bb), gate=gate, inplace=True)
            if ctx.se:
                p, hid, _, w1, w2 = saved[19:]
                grads[7], grads[8], grads[9], grads[10], dp = E.se_train_bwd(dgate, gate, hid, p, f(w1), f(w2))
                E.mean_rows_bwd(dp, dv, accumulate=True)                                         # completes dv
        if any(need[:7]):
            dv0, grads[5], grads[6] = _bn_bwd_sliced(dv, v0, mb, rb, f(gb))
        if any(need[:5]):
            t = _bn_relu_sliced(z_a, ma, ra, f(ga), f(ba))
            if need[4]:
                grads[4] = E.dwconv3_wgrad(t, dv0)[0]
        if any(need[:4]):
            dt = E.dwconv(dv0, E.pack_dwconv(wb.detach().flip(2, 3, 4), None, None, (1, 1, 1), (1, 1, 1), E.ACT_NONE))
            dz_a, grads[2], grads[3] = _bn_bwd_sliced(dt, z_a, ma, ra, f(ga), y=t)
            if need[1]:
                # operands exchanged: [dim_out][dim_inner] = dW_a^T, the same sums; 432 is no multiple of 32, 192 and 96 are
                grads[1] = E.linear_wgrad(dz_a, xc, bias=False)[0].t().contiguous().view(Ci, D, 1, 1, 1)
            if need[0]:
                dx = E.conv(dz_a, _pack_t(wa))
                grads[0] = E.relu_mask_add(dx, Gc, y).as_nthwc()                                 # the skip path
        return tuple(g if g is None or need[i] else None for i, g in enumerate(grads))


def x3d_blocks(stage, x, start=1, stop=None):
    """Blocks start .. stop - 1 (None: to the end) of the single pathway of the ResStage `stage`, chained as X3DBlock on
    ResBlock.tensors(): x fp32 channels-last [B,T,h,w,dim_out] on the GPU.  The stage's first block (stride-2 `b`, branch1) has
    no backward yet and is refused by name, like any other block with branch1 or a stride.  Returns the last block's output
    with a graph over every tensor of the blocks (and x where it requires grad)."""
    if stage.num_pathways != 1:
        raise MspiError("x3d_blocks: the stage has %d pathways, X3D has one" % stage.num_pathways)
    blocks = stage.blocks(0)
    stop = len(blocks) if stop is None else stop
    if not 0 <= start < stop <= len(blocks):
        raise MspiError("x3d_blocks: blocks %d .. %d of a stage of %d" % (start, stop - 1, len(blocks)))
    for i in range(start, stop):
        blk = blocks[i]
        tr = blk.branch2
        if hasattr(blk, "branch1") or tuple(tr.a.stride) != (1, 1, 1) or tuple(tr.b.stride) != (1, 1, 1):
            raise MspiError("x3d_blocks: pathway0_res%d has %s: only stride-1 blocks without branch1 have a backward (the stage "
                            "heads are still frozen)" % (i, "branch1" if hasattr(blk, "branch1") else "a stride of %s" % (tuple(tr.b.stride),)))
        x = X3DBlock.apply(x, *blk.tensors())
    return x
