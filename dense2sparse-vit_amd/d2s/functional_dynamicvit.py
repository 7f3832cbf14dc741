"""The DynamicViT baseline's predictor and keep decision (vit_models/default_dynamic_vit.py:304-330, :452-459 of the reference):
LN -> Linear(D,D) -> GELU, policy-weighted pooling of the upper half, Linear(D,D/2) -> GELU -> Linear(D/2,D/4) -> GELU -> Linear(D/4,2);
the 2-way LogSoftmax is fused into the Gumbel keep kernel behind it.  LayerNorm / GEMM launches are the library's existing ones."""
import torch

from . import ops
from .functional import layernorm_backward, mode_recorded, wants_grad


@mode_recorded
class DynPredictorFn(torch.autograd.Function):
    """x [B, n, D] (CLS row skipped in place), policy [B, N] -> raw 2-way logits z [B * N, 2].
    params: ln_w, ln_b, in_w, in_b, w1, b1, w2, b2, w3, b3."""

    @staticmethod
    def forward(ctx, x, policy, *params):
        B, n, D = x.shape
        N = n - 1
        M = B * N
        x = x.contiguous()
        policy = policy.contiguous()
        lnw, lnb, w0, b0, w1, b1, w2, b2, w3, b3 = params
        train = wants_grad(ctx)
        dev = x.device
        h0, mean0, rstd0 = ops.layernorm_fwd(x, ops.skip_cls_map(n, D), lnw, lnb, M, D, 1e-5, stats=train)
        z0 = torch.empty((M, w0.shape[0]), dtype=torch.float32, device=dev) if train else None
        a0 = ops.linear_fwd(h0, w0, b0, epi=ops.EPI_BIAS_GELU, aux_out=z0)
        C = a0.shape[1]
        c0, psum, glob = ops.policy_pool_fwd(a0, policy, B, N, C)
        z1 = torch.empty((M, w1.shape[0]), dtype=torch.float32, device=dev) if train else None
        a1 = ops.linear_fwd(c0, w1, b1, epi=ops.EPI_BIAS_GELU, aux_out=z1)
        z2 = torch.empty((M, w2.shape[0]), dtype=torch.float32, device=dev) if train else None
        a2 = ops.linear_fwd(a1, w2, b2, epi=ops.EPI_BIAS_GELU, aux_out=z2)
        with ops.gemm_mode(ops.GEMM_EXACT):      # the decision's logits stay exact fp32 in every GEMM arithmetic mode, like the student's tail
            z = ops.linear_fwd(a2, w3, b3)
        if train:
            ctx.save_for_backward(x, policy, h0, mean0, rstd0, z0, a0, psum, glob, c0, z1, a1, z2, a2, *params)
            ctx.dims = (B, n, D, C)
        return z

    @staticmethod
    def backward(ctx, gz):
        x, policy, h0, mean0, rstd0, z0, a0, psum, glob, c0, z1, a1, z2, a2 = ctx.saved_tensors[:14]
        lnw, lnb, w0, b0, w1, b1, w2, b2, w3, b3 = ctx.saved_tensors[14:]
        B, n, D, C = ctx.dims
        N = n - 1
        M = B * N
        want = [ctx.needs_input_grad[2 + i] for i in range(10)]
        g = [None] * 10
        gz = gz.contiguous()
        with ops.gemm_mode(ops.GEMM_EXACT):
            g[8], g[9] = ops.linear_param_grads(gz, a2, w3, b3, want[8], want[9])
            d2 = ops.linear_dgrad(gz, w3, epi=ops.EPI_MUL_GELU_GRAD, aux=z2)
        g[6], g[7] = ops.linear_param_grads(d2, a1, w2, b2, want[6], want[7])
        d1 = ops.linear_dgrad(d2, w2, epi=ops.EPI_MUL_GELU_GRAD, aux=z1)
        g[4], g[5] = ops.linear_param_grads(d1, c0, w1, b1, want[4], want[5])
        dc0 = ops.linear_dgrad(d1, w1)
        da0, dpol = ops.policy_pool_bwd(dc0, a0, policy, psum, glob, B, N, C)
        dz0 = ops.act_grad(da0, z0, "gelu")
        g[2], g[3] = ops.linear_param_grads(dz0, h0, w0, b0, want[2], want[3])
        gx = None
        if ctx.needs_input_grad[0] or want[0] or want[1]:
            dh0 = ops.linear_dgrad(dz0, w0)
            gx, g[0], g[1] = layernorm_backward(x, ops.skip_cls_map(n, D), dh0, lnw, lnb, mean0, rstd0,
                                                torch.zeros((B, n, D), dtype=torch.float32, device=gz.device), M, D, want[0], want[1])
            if not ctx.needs_input_grad[0]:
                gx = None
        return (gx, dpol if ctx.needs_input_grad[1] else None) + tuple(g)


class GumbelKeepFn(torch.autograd.Function):
    """z [B * N, 2] raw logits, g [B, N, 2] Gumbel noise, prev [B, N] -> decision [B, N] = hard(log_softmax(z) + g) * prev with the
    straight-through backward of F.gumbel_softmax(hard=True) (tau = 1).  Also returns log_softmax(z) [B, N, 2] (non-differentiable)."""

    @staticmethod
    def forward(ctx, z, g, prev):
        B, N = prev.shape
        prev = prev.contiguous()
        logp, y0, hard, dec = ops.gumbel_keep_fwd(z.contiguous(), g.contiguous().view(B * N, 2), prev.view(-1))
        ctx.save_for_backward(prev, y0, hard)
        logp = logp.view(B, N, 2)
        ctx.mark_non_differentiable(logp)
        return dec.view(B, N), logp

    @staticmethod
    def backward(ctx, gd, _gl):
        prev, y0, hard = ctx.saved_tensors
        dz, dprev = ops.gumbel_keep_bwd(gd.contiguous().view(-1), prev.view(-1), y0, hard)
        return dz, None, dprev.view(prev.shape) if ctx.needs_input_grad[2] else None


class RatioLossFn(torch.autograd.Function):
    """decision [B, N], rho, denom -> sum_b (mean_j decision[b, j] - rho)^2 / denom: one stage of the DynamicViT ratio term (denom = B * S
    folds the batch mean and the mean over the S stages in)."""

    @staticmethod
    def forward(ctx, d, rho, denom):
        d = d.contiguous()
        loss_row, diff = ops.ratio_rows_fwd(d, rho)
        ctx.save_for_backward(diff)
        ctx.meta = (d.shape[1], 1.0 / float(denom))
        return ops.sum_scalar(loss_row, 1.0 / float(denom))

    @staticmethod
    def backward(ctx, g):
        (diff,) = ctx.saved_tensors
        N, scale = ctx.meta
        return ops.ratio_rows_bwd(diff, g.contiguous(), scale, N), None, None
