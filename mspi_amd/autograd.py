"""torch.autograd surface of the hand-written backward kernels.

ReadoutTail: the decoder's last three convs and the log-softmax (readout[8], readout[10], readout[12] of
model/model_utils.py:403-409) as one autograd.Function over the features y4 that enter readout[8] and the six parameters.
Forward and backward run on the C ABI (mspi_amd.engine); the forward launches what the inference path launches.

ReadoutHead: the three convs in front of it (readout[0], readout[1] + BatchNorm readout[2], readout[4] + BatchNorm readout[5],
model/model_utils.py:490-497) with the BatchNorm layers on BATCH statistics, over the four fused pyramid maps.  Its output is
ReadoutTail's input, so the two together train the whole readout Sequential."""
import torch

from . import engine as E
from ._lib import MspiError


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
        if not y4.is_cuda:
            raise MspiError("mspi_amd runs on the GPU only (tensor on %s); there is no CPU fallback" % y4.device)
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
        # data gradient of a stride-1 "same" conv: the same conv with w'[ci][-tap][co].  Both data-gradient convs run on the
        # fp32 MFMA path: their activation operand is a gradient, whose scale is the loss's (1e-5 and below with SalLoss at the
        # training shape), and the f16x3 split of an activation is exact only while its largest entries stay above about 2^-5
        pk10t = E.pack_conv(w10.detach().transpose(0, 1).flip(3, 4), None, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE,
                            prec=E.PREC_F32)
        d8 = E.upsample_bwd(E.conv(d10, pk10t), 4, u=u, act=E.ACT_RELU)
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


def _bn_train(x, gamma, beta, buffers):
    """BatchNorm on batch statistics + ReLU, and the running-stat update of nn.BatchNorm3d.train(): momentum 0.1, the
    UNBIASED variance into running_var, num_batches_tracked += 1.  Returns (y, mean, rstd)."""
    mean, var, rstd = E.bn_stats(x, BN_EPS)
    y = E.bn_apply(x, mean, rstd, gamma.detach().contiguous(), beta.detach().contiguous(), act=E.ACT_RELU)
    if buffers is not None:
        rm, rv, nbt = buffers
        rm.mul_(1.0 - BN_MOMENTUM).add_(mean, alpha=BN_MOMENTUM)
        rv.mul_(1.0 - BN_MOMENTUM).add_(var, alpha=BN_MOMENTUM * x.M / (x.M - 1.0))
        nbt.add_(1)
    return y, mean, rstd


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
    Gradients: the ten parameters.  The maps get none: everything in front of the readout is frozen.  No double backward."""

    @staticmethod
    def forward(ctx, s0, s1, s2, s3, w0, b0, w1, b1, g2, be2, w4, b4, g5, be5, bn2, bn5):
        maps = []
        for j, s in enumerate((s0, s1, s2, s3)):
            if not s.is_cuda:
                raise MspiError("mspi_amd runs on the GPU only (tensor on %s); there is no CPU fallback" % s.device)
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
            a1, m2, r2 = _bn_train(x1, g2, be2, bn2)
            x4 = E.conv(a1, pk4)
            y4, m5, r5 = _bn_train(x4, g5, be5, bn5)
        ctx.save_for_backward(*maps, y0.buf, x1.buf, a1.buf, x4.buf, y4.buf, m2, r2, m5, r5, w1, g2, w4, g5)
        ctx.packs = (parts, pk1, pk4)
        return y4.buf.view(y4.N, y4.T, y4.H, y4.W, y4.ld)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s0, s1, s2, s3, y0b, x1b, a1b, x4b, y4b, m2, r2, m5, r5, w1, g2, w4, g5 = ctx.saved_tensors
        parts, pk1, pk4 = ctx.packs
        B, T, h, w, D = s0.shape
        c1, c4 = w1.shape[0], w4.shape[0]

        def cl(buf, c):
            return E.CL(buf, 0, B, T, h, w, c, c)
        y0, x1, a1, x4, y4 = cl(y0b, c1), cl(x1b, c1), cl(a1b, c1), cl(x4b, c4), cl(y4b, c4)
        d4, dg5, dbe5 = E.bn_bwd(cl(g.float().contiguous().view(-1), c4), x4, m5, r5, g5.detach().contiguous(), y=y4)
        dw4, db4 = E.conv_wgrad_wide(a1, d4, pk4)
        # data gradient of a stride-1 "same" conv: the same conv with w'[ci][-tap][co], on the fp32 MFMA path (ReadoutTail.backward)
        pk4t = E.pack_conv(w4.detach().transpose(0, 1).flip(3, 4), None, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE, prec=E.PREC_F32)
        d1, dg2, dbe2 = E.bn_bwd(E.conv(d4, pk4t), x1, m2, r2, g2.detach().contiguous(), y=a1)
        dw1, db1 = E.conv_wgrad_wide(y0, d1, pk1)
        pk1t = E.pack_conv(w1.detach().transpose(0, 1).flip(2, 3, 4), None, None, (1, 1, 1), (1, 1, 1), E.ACT_NONE, prec=E.PREC_F32)
        dy0 = E.conv(d1, pk1t)
        # dW0 without the 768-channel concat: the adjoint of r0_parts.  y0 = W0 s0 + b + sum_j up_j((W0 + Wj) sj'), j = 1, 2, 3,
        # and <up_j(A s), dy0> = <A s, up_j^T dy0>, so with g_j = up_j^T dy0 (upsample_bwd) and G0 = dy0^T s0, G_j = g_j^T sj':
        #   dL/dW0 = G0 + G1 + G2 + G3 (W0 takes part in every term), dL/dWj = G_j, db0 = sum dy0
        G0, db0 = E.conv_wgrad_wide(_cl5(s0), dy0, parts[0])
        Gs = [E.conv_wgrad_wide(_cl5(s), E.upsample_bwd(dy0, k), pk)[0] for s, k, pk in ((s1, 2, parts[1]), (s2, 4, parts[2]), (s3, 8, parts[3]))]
        dw0 = torch.cat([((G0 + Gs[0]) + Gs[1]) + Gs[2]] + Gs, dim=1)
        grads = [None] * 4 + [dw0, db0, dw1, db1, dg2, dbe2, dw4, db4, dg5, dbe5, None, None]
        need = ctx.needs_input_grad
        return tuple(gr if need[i] else None for i, gr in enumerate(grads))
