"""Token Merging (ToMe, Bolya et al. 2023): the launch sequence of one transformer block that merges r tokens between
its attention branch and its MLP - tome_block_forward for inference, ToMeBlockFn (the same launches, plus what a backward needs) to train
through the merge.

    LayerNorm -> qkv GEMM -> attention -> proj + residual -> match -> merge -> LayerNorm -> fc1 + GELU -> fc2 + residual

The match reads the keys of the qkv GEMM's output in place; the merge acts on x1 (after proj + residual), so the MLP half runs on n - r
rows.  Attention is the plain kernel while every token still stands for one patch (size is None) and the key-weighted one afterwards
(proportional attention).  The composite block call (ops.block_fwd) cannot serve here - the merge sits in the middle of the block - so the
launches are issued one by one, the same kernels in the same order as functional.block_forward_sequence: with r = 0 and no sizes the
result is bit for bit the dense block's.  The bf16 arithmetic mode is refused there (the key-weighted attention it calls is an fp32
kernel; the GEMM modes exact and split both run); tome_block_forward_bf16 is the same block on the bf16 data path, inference only:
LayerNorm and the GEMMs hand bf16 to each other, attention and the match read the bf16 qkv (ops.attn_keyw_fwd_bf16io,
ops.tome_match_bf16), the residual stream and therefore the merge stay fp32.

Training: the merge is a size-weighted average with a constant plan (the match reads K under no gradient, as the published
bipartite_soft_matching does), so its backward is one scaled row copy per input row (ops.tome_merge_bwd); the attention backward takes
the key weights where the forward did (ops.attn_keyw_bwd).  Everything else is BlockFn.backward's fp32 per-op sequence; the MLP half's
residual gradient lives on n - r rows, the attention half's on n.
"""
import torch

from . import ops
from .functional import _norm_linear, bf16_data_path, layernorm_backward, mode_recorded, wants_grad
from .lib import D2SError

_BF16_REFUSAL = "token merging runs in the fp32 arithmetic modes (exact, split): the key-weighted attention has no bf16 kernel"


def tome_block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn=True, plan=None):
    """x [B * n, D] tokens, size [B, n] patches per token or None (all ones), params as Block._params(), r the merge count asked for (clipped
    here to (n - 1) // 2).  plan: (unm_idx, src_idx, dst_idx) to merge by instead of matching (a replay).
    -> (y [B * (n - r), D], size_out [B, n - r] or None while nothing has merged, (unm_idx, src_idx, dst_idx) or None when r == 0)"""
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(_BF16_REFUSAL)
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = params
    rows, D = x.shape
    assert rows == B * n
    r = ops.tome_clip_r(r, n)
    cmap = ops.contiguous_map(rows, D)
    ln, _, _ = ops.layernorm_fwd(x, cmap, n1w, n1b, rows, D, eps, stats=False)
    qkv = ops.linear_fwd(ln, qkvw, qkvb)
    del ln
    if size is not None and prop_attn:
        ao, _ = ops.attn_keyw_fwd(qkv, size, B, n, heads, scale)
    else:
        ao, _, _ = ops.attn_fwd(qkv, B, n, heads, scale, want_cls=False)
    x1 = ops.linear_fwd(ao, projw, projb, epi=ops.EPI_BIAS_RESID, aux=x)
    del ao
    if r > 0:
        if plan is None:
            plan = ops.tome_match(qkv, B, n, heads, r)[2:]
        x1, size = ops.tome_merge(x1, size, *plan, B, n, D, r)
    else:
        plan = None
    del qkv
    rows = B * (n - r)
    ln, _, _ = ops.layernorm_fwd(x1, ops.contiguous_map(rows, D), n2w, n2b, rows, D, eps, stats=False)
    h = ops.linear_fwd(ln, fc1w, fc1b, epi=ops.EPI_BIAS_GELU)
    del ln
    y = ops.linear_fwd(h, fc2w, fc2b, epi=ops.EPI_BIAS_RESID, aux=x1)
    return y, size, plan


def tome_block_forward_bf16(x, size, params, B, n, heads, eps, scale, r, prop_attn=True, plan=None):
    """tome_block_forward on the bf16 data path (inference): the launches of functional.block_forward_sequence with io=True, train=False,
    and the match and the merge between proj and the second LayerNorm.  Same arguments, same shape of a result.  With r = 0 and no sizes:
    bit for bit the bf16 forward-only block."""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = params
    rows, D = x.shape
    assert rows == B * n
    if not bf16_data_path(x, D, fc1w.shape[0]):
        raise D2SError("tome_block_forward_bf16 needs the bf16 data path: the bf16 arithmetic mode (ops.gemm_mode(ops.GEMM_BF16)), "
                       "D2S_BF16_IO not 0, D and hidden multiples of 32 and device tensors")
    r = ops.tome_clip_r(r, n)
    _, qkv, _, _ = _norm_linear(x, ops.contiguous_map(rows, D), n1w, n1b, qkvw, qkvb, eps, True, False)
    if size is not None and prop_attn:
        _, _, ao16 = ops.attn_keyw_fwd_bf16io(qkv, size, B, n, heads, scale, want_f32=False)
    else:
        _, _, _, ao16 = ops.attn_fwd_bf16io(qkv, B, n, heads, scale, want_cls=False, want_f32=False)
    x1 = ops.linear_fwd(None, projw, projb, epi=ops.EPI_BIAS_RESID, aux=x, a16=ao16)
    del ao16
    if r > 0:
        if plan is None:
            plan = ops.tome_match_bf16(qkv, B, n, heads, r)[2:]
        x1, size = ops.tome_merge(x1, size, *plan, B, n, D, r)
    else:
        plan = None
    del qkv
    rows = B * (n - r)
    _, h16, _, _ = _norm_linear(x1, ops.contiguous_map(rows, D), n2w, n2b, fc1w, fc1b, eps, True, False, ops.EPI_BIAS_GELU)
    y = ops.linear_fwd(None, fc2w, fc2b, epi=ops.EPI_BIAS_RESID, aux=x1, a16=h16)
    return y, size, plan


@mode_recorded
class ToMeBlockFn(torch.autograd.Function):
    """tome_block_forward as a differentiable Function: x [B, n, D], size [B, n] or None, the 12 block parameters, heads, eps, scale, r,
    prop_attn, plan (unm_idx, src_idx, dst_idx as three inputs, or three None to match here)
    -> (y [B, n - r, D], size_out [B, n - r] or None, unm_idx, src_idx, dst_idx or None); only y is differentiable, in x and the parameters."""

    @staticmethod
    def forward(ctx, x, size, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b, heads, eps, scale, r, prop_attn,
                unm, src, dst):
        if ops.get_gemm_mode() == ops.GEMM_BF16:
            raise D2SError(_BF16_REFUSAL)
        train = wants_grad(ctx)
        B, n, D = x.shape
        x = x.contiguous()
        rows = B * n
        xf = x.view(rows, D)
        r = ops.tome_clip_r(r, n)
        keyw = size is not None and bool(prop_attn)
        ln1, mean1, rstd1 = ops.layernorm_fwd(xf, ops.contiguous_map(rows, D), n1w, n1b, rows, D, eps, stats=train)
        qkv = ops.linear_fwd(ln1, qkvw, qkvb)
        if keyw:
            ao, lse = ops.attn_keyw_fwd(qkv, size, B, n, heads, scale, want_lse=train)
        else:
            ao, lse, _ = ops.attn_fwd(qkv, B, n, heads, scale, want_cls=False)
        x1 = ops.linear_fwd(ao, projw, projb, epi=ops.EPI_BIAS_RESID, aux=xf)
        size_out, matched = size, False
        if r > 0:
            if unm is None:
                unm, src, dst = ops.tome_match(qkv, B, n, heads, r)[2:]
                matched = True
            x1, size_out = ops.tome_merge(x1, size, unm, src, dst, B, n, D, r)       # the unmerged x1 dies here: the backward needs the merged one
        else:
            unm = src = dst = None
        rows2 = B * (n - r)
        z = torch.empty((rows2, fc1w.shape[0]), dtype=torch.float32, device=x.device) if train else None
        ln2, mean2, rstd2 = ops.layernorm_fwd(x1, ops.contiguous_map(rows2, D), n2w, n2b, rows2, D, eps, stats=train)
        h = ops.linear_fwd(ln2, fc1w, fc1b, epi=ops.EPI_BIAS_GELU, aux_out=z)
        y = ops.linear_fwd(h, fc2w, fc2b, epi=ops.EPI_BIAS_RESID, aux=x1)
        if train:
            ctx.save_for_backward(x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b, mean1, rstd1, ln1, qkv, ao, lse,
                                  x1, mean2, rstd2, ln2, z, h)
            ctx.merge = (size, size_out, unm, src, dst)      # constants of the backward (no gradient reaches them)
            ctx.dims = (B, n, D, heads, float(scale), r, keyw)
        outs = (size_out if r > 0 else None,) + ((unm, src, dst) if matched else (None, None, None))
        ctx.mark_non_differentiable(*[t for t in outs if t is not None])
        return (y.view(B, n - r, D),) + outs

    @staticmethod
    def backward(ctx, gy, *_unused):
        (x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b, mean1, rstd1, ln1, qkv, ao, lse,
         x1, mean2, rstd2, ln2, z, h) = ctx.saved_tensors
        size, size_out, unm, src, dst = ctx.merge
        B, n, D, heads, scale, r, keyw = ctx.dims
        M, M2 = B * n, B * (n - r)
        dev = gy.device
        gy = gy.contiguous().view(M2, D)
        # input slots: x 0, size 1, then n1w n1b qkvw qkvb projw projb n2w n2b fc1w fc1b fc2w fc2b -> 2..13
        wants = [ctx.needs_input_grad[0]] + [ctx.needs_input_grad[i] for i in range(2, 14)]
        grads = [None] * 13
        # ---- MLP branch, on the n - r rows that left the merge ----
        grads[11], grads[12] = ops.linear_param_grads(gy, h, fc2w, fc2b, wants[11], wants[12])
        dz = ops.linear_dgrad(gy, fc2w, epi=ops.EPI_MUL_GELU_GRAD, aux=z)
        grads[9], grads[10] = ops.linear_param_grads(dz, ln2, fc1w, fc1b, wants[9], wants[10])
        dln2 = ops.linear_dgrad(dz, fc1w)
        g1, grads[7], grads[8] = layernorm_backward(x1, ops.contiguous_map(M2, D), dln2, n2w, n2b, mean2, rstd2,
                                                    torch.empty((M2, D), dtype=torch.float32, device=dev), M2, D, wants[7], wants[8], add_src=gy)
        # ---- the merge: every one of the n input rows takes its output row's gradient, scaled where it was averaged ----
        if r > 0:
            g1 = ops.tome_merge_bwd(g1, size, size_out, unm, src, dst, B, n, D, r)
        # ---- attention branch, on n rows ----
        grads[5], grads[6] = ops.linear_param_grads(g1, ao, projw, projb, wants[5], wants[6])
        dao = ops.linear_dgrad(g1, projw)
        if keyw:
            dqkv = ops.attn_keyw_bwd(qkv, size, ao, dao, lse, B, n, heads, scale)
        else:
            dqkv = ops.attn_bwd(qkv, ao, dao, lse, B, n, heads, scale)
        grads[3], grads[4] = ops.linear_param_grads(dqkv, ln1, qkvw, qkvb, wants[3], wants[4])
        gx = None
        if wants[0] or wants[1] or wants[2]:
            dln1 = ops.linear_dgrad(dqkv, qkvw)
            gx, grads[1], grads[2] = layernorm_backward(x, ops.contiguous_map(M, D), dln1, n1w, n1b, mean1, rstd1,
                                                        torch.empty((M, D), dtype=torch.float32, device=dev), M, D, wants[1], wants[2], add_src=g1)
            gx = gx.view(B, n, D) if wants[0] else None
        return (gx, None) + tuple(grads[1:]) + (None,) * 8


def tome_block_train(x, size, params, heads, eps, scale, r, prop_attn=True, plan=None):
    """ToMeBlockFn with tome_block_forward's shape of a result: x [B, n, D] -> (y [B, n - r, D], size_out or None, plan or None)"""
    from .functional import run
    n = x.shape[1]
    if ops.tome_clip_r(r, n) == 0:
        plan = None
    y, size_out, unm, src, dst = run(ToMeBlockFn, x, size, *params, heads, eps, scale, r, prop_attn, *(plan if plan is not None else (None,) * 3))
    if ops.tome_clip_r(r, n) == 0:
        return y, size, None
    return y, size_out, (plan if plan is not None else (unm, src, dst))
