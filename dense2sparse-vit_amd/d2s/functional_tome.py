"""Token Merging at inference (ToMe, Bolya et al. 2023): the launch sequence of one transformer block that merges r
tokens between its attention branch and its MLP.

    LayerNorm -> qkv GEMM -> attention -> proj + residual -> match -> merge -> LayerNorm -> fc1 + GELU -> fc2 + residual

The match reads the keys of the qkv GEMM's output in place; the merge acts on x1 (after proj + residual), so the MLP half runs on n - r
rows.  Attention is the plain kernel while every token still stands for one patch (size is None) and the key-weighted one afterwards
(proportional attention).  The composite block call (ops.block_fwd) cannot serve here - the merge sits in the middle of the block - so the
launches are issued one by one, the same kernels in the same order as functional.block_forward_sequence: with r = 0 and no sizes the
result is bit for bit the dense block's.  Forward only: nothing is kept for a backward, and the bf16 arithmetic mode is refused (the
key-weighted attention is an fp32 kernel; the GEMM modes exact and split both run).
"""
from . import ops
from .lib import D2SError


def tome_block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn=True, plan=None):
    """x [B * n, D] tokens, size [B, n] patches per token or None (all ones), params as Block._params(), r the merge count asked for (clipped
    here to (n - 1) // 2).  plan: (unm_idx, src_idx, dst_idx) to merge by instead of matching (a replay).
    -> (y [B * (n - r), D], size_out [B, n - r] or None while nothing has merged, (unm_idx, src_idx, dst_idx) or None when r == 0)"""
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError("token merging runs in the fp32 arithmetic modes (exact, split): the key-weighted attention has no bf16 kernel")
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
