"""Graph ranking (--graph-rank T; DESIGN.md section 29 - the build's own definition, PARITY UNPINNED): a stage of an attention-selecting
student ranks its tokens by T steps of PageRank over the attention graph of the block before it (ops.graph_rank, from that block's qkv and
the log-sum-exp its attention wrote) instead of by that block's CLS row alone.

GraphRankBlockFn is the block before such a stage: BlockFn's arithmetic through block_forward_sequence / block_backward_sequence (the
one-call composite never shows qkv and lse to Python), with the rank launched right after the attention forward as a non-differentiable
side output - the pattern of functional_ltp.LTPSoftBlockFn.  No hook sits between the halves, so stochastic depth works as in BlockFn.
Every other block of the model stays on BlockFn.

The bf16 arithmetic mode is refused (GRAPH_RANK_BF16_ERROR): there qkv exists in bf16 only and the rank kernel is built for fp32."""
import torch

from . import functional as DF
from . import ops
from .lib import D2SError

GRAPH_RANK_BF16_ERROR = ("graph ranking (graph_rank_iters > 0, --graph-rank) runs in the fp32 arithmetic modes (exact, split): the rank is "
                         "recomputed from the block's fp32 qkv and the fp32 attention's log-sum-exp, and in the bf16 arithmetic mode qkv "
                         "exists in bf16 only")


def refuse_bf16():
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(GRAPH_RANK_BF16_ERROR)


@DF.mode_recorded
class GraphRankBlockFn(torch.autograd.Function):
    """One pre-norm transformer block on [B, n, D] tokens that also ranks them: x, the 12 block parameters, heads, eps, want_cls, scale,
    iters, s_attn, s_mlp (the block's stochastic-depth rows [B] or None) -> (y [B, n, D], cls_row [B, H, n] or an empty tensor,
    rank [B, H, n]).  Differentiable in x and the parameters as BlockFn is; the CLS row and the rank carry no gradient."""

    @staticmethod
    def forward(ctx, x, *rest):
        params, (heads, eps, want_cls, scale, iters, s_attn, s_mlp) = rest[:12], rest[12:]
        refuse_bf16()
        train = DF.wants_grad(ctx)
        if not train:                     # only a forward that keeps something for a backward applies stochastic depth, as in BlockFn
            s_attn = s_mlp = None
        B, n, D = x.shape
        x = x.contiguous()
        scale = float(DF._DH) ** -0.5 if scale is None else float(scale)
        ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        side = {}

        def attn(qkv, io, want_f32):
            out = DF.attn_forward(qkv, B, n, heads, scale, want_cls, None, io)
            side["rank"] = ops.graph_rank(qkv, out[1], B, n, heads, scale, iters)      # qkv and lse exist here and nowhere later in eval
            return out

        y, cls_row, saved, _ = DF.block_forward_sequence(x.view(B * n, D), params, eps, False, train, attn, (), s_attn, s_mlp, n)
        if train:
            ctx.save_for_backward(x, *saved)
            ctx.drop_path = (s_attn, s_mlp)
            ctx.dims = (B, n, heads, scale)
        cls_row = DF.cls_or_empty(cls_row, x.device)
        ctx.mark_non_differentiable(cls_row, side["rank"])
        return y.view(B, n, D), cls_row, side["rank"]

    @staticmethod
    def backward(ctx, gy, _gcls, _grank):
        x, *saved = ctx.saved_tensors
        B, n, heads, scale = ctx.dims
        # input slots: x 0, the 12 parameters 1..12, heads eps want_cls scale iters s_attn s_mlp 13..19
        grads, _ = DF.block_backward_sequence(
            gy, x, saved, list(ctx.needs_input_grad[:13]), *ctx.drop_path, n,
            lambda qkv, ao, dao, lse, io, dqkvh, want_f32: DF.attn_backward(qkv, ao, dao, lse, B, n, heads, scale, None, None, io, dqkvh,
                                                                            want_f32))
        return tuple(grads) + (None,) * 7


def rank_block(x, params, heads, eps, scale, iters, want_cls=True, drop_path_rows=None):
    """GraphRankBlockFn on one block -> (y, cls_row or None, rank [B, H, n])"""
    s_attn, s_mlp = drop_path_rows if drop_path_rows is not None else (None, None)
    y, cls_row, rank = DF.run(GraphRankBlockFn, x, *params, heads, eps, bool(want_cls), scale, int(iters), s_attn, s_mlp)
    return y, (cls_row if want_cls else None), rank
