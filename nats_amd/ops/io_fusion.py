"""Autograd wrappers for the glue kernels (ops/hip/io_fusion.hip).

Under bf16 autocast the torch expressions around the scan kernels make
value-identity passes over the largest tensors of the step: ``x @ W + b``
writes an fp32 sum that the consuming kernel rounds straight back to bf16,
its backward casts the bf16 gradient to fp32, column-sums that copy and
casts it to bf16 again for the GEMMs; the encoder context is cast to
bf16 twice, and its gradient is cast, accumulated, sliced and flipped.
The Functions here keep the GEMMs in torch (same shapes and leading
dimensions, so the tuned-GEMM table still applies) and do each remaining
piece in one kernel pass.
"""

import torch

from . import _hip_ext, eager
from .gru import _load_opt, _save_opt

BF16 = torch.bfloat16


class LinearBiasFn(torch.autograd.Function):
    """y = bf16(x.bf16 @ W.bf16 + b): the rounding ``(x @ W + b).to(bf16)``
    makes under autocast, without the fp32 intermediate."""

    @staticmethod
    def forward(ctx, x, W, b):
        ext = _hip_ext()
        K, N = W.shape
        x2 = x.reshape(-1, K).to(BF16)
        Wb = W.to(BF16)
        y = ext.bias_cast_(x2 @ Wb, b.float().contiguous())
        ctx.save_for_backward(x2, Wb)
        ctx.x_shape, ctx.dtypes = x.shape, (x.dtype, W.dtype, b.dtype)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        ext = _hip_ext()
        x2, Wb = ctx.saved_tensors
        xd, Wd, bd = ctx.dtypes
        N = Wb.shape[1]
        # dpre slices of the scans arrive as bf16 views with a row stride
        # of 4H: the column sum reads them in place
        dy2 = dy.to(BF16).reshape(-1, N)
        if dy2.stride(1) != 1 and N > 1:
            dy2 = dy2.contiguous()
        db = ext.colsum_bf16(dy2)
        # the GEMMs take one contiguous bf16 copy, the operand layout the
        # tuned-GEMM table was recorded for
        dyc = dy2.contiguous()
        dx = dW = None
        if ctx.needs_input_grad[0]:
            dx = (dyc @ Wb.t()).view(ctx.x_shape).to(xd)
        if ctx.needs_input_grad[1]:
            dW = (x2.t() @ dyc).to(Wd)
        return dx, dW, db.to(bd)


def linear_bias_hip(x, W, b):
    return LinearBiasFn.apply(x, W, b)


class EncoderHeadFn(torch.autograd.Function):
    """(h_f, h_r, mask, Wc_att, b_att) -> (ctx_bf, ctx_mean, pctx) with
    the bf16 ctx = [h_f | flip(h_r)] written straight from the scan
    outputs; no fp32 ctx, and no fp32 ctx gradient, is kept."""

    @staticmethod
    def forward(fctx, h_f, h_r, mask, Wc_att, b_att):
        ext = _hip_ext()
        T, B, H = h_f.shape
        fctx.dtypes = (h_f.dtype, h_r.dtype, Wc_att.dtype, b_att.dtype)
        h_f, h_r = h_f.float().contiguous(), h_r.float().contiguous()
        ctx_bf = ext.ctx_head_fwd(h_f, h_r)
        # the mean stays torch's own reduction over the fp32 context: the
        # decoder's initial state is rounded to bf16 from it, and another
        # summation order flips some of those roundings
        ctx_mean = eager.context_mean(
            torch.cat([h_f, h_r.flip(0)], dim=-1), mask)
        cnt = (mask.sum(0) if mask is not None
               else h_f.new_full((B,), float(T)))
        Wb = Wc_att.to(BF16)
        pctx = (ctx_bf.view(T * B, 2 * H) @ Wb).view(T, B, -1) + b_att
        fctx.save_for_backward(ctx_bf, Wb, _save_opt(mask), cnt)
        return ctx_bf, ctx_mean, pctx

    @staticmethod
    def backward(fctx, dctx, dmean, dpctx):
        ext = _hip_ext()
        ctx_bf, Wb, mask, cnt = fctx.saved_tensors
        mask = _load_opt(mask)
        T, B, C = ctx_bf.shape
        A = Wb.shape[1]
        hfd, hrd, Wd, bd = fctx.dtypes
        db_att = dpctx.reshape(T * B, A).sum(0)
        dpb = dpctx.to(BF16).reshape(T * B, A)
        dWc = ctx_bf.view(T * B, C).t() @ dpb
        dproj = (dpb @ Wb.t()).view(T, B, C)
        dh_f, dh_r = ext.ctx_head_bwd(
            dctx.to(BF16), dproj, dmean.float().contiguous(), mask, cnt)
        return dh_f.to(hfd), dh_r.to(hrd), None, dWc.to(Wd), db_att.to(bd)


def encoder_head_hip(h_f, h_r, x_mask, Wc_att, b_att):
    if x_mask is not None:
        x_mask = x_mask.float().contiguous()
    return EncoderHeadFn.apply(h_f, h_r, x_mask, Wc_att, b_att)
