"""torch.autograd surface of the hand-written backward kernels.

ReadoutTail: the decoder's last three convs and the log-softmax (readout[8], readout[10], readout[12] of
model/model_utils.py:403-409) as one autograd.Function over the features y4 that enter readout[8] and the six parameters.
Forward and backward run on the C ABI (mspi_amd.engine); the forward launches what the inference path launches."""
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
