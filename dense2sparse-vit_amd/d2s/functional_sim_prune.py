"""Similarity pruning (--sim-prune R; DESIGN.md section 30 - the build's own definition, PARITY UNPINNED): a stage of an attention-selecting
student takes k + r candidates by importance and prunes the r that resemble a more important candidate most (ops.sim_prune), by the
cosine of the key metric of the block before it (ops.key_metric, from that block's qkv).

SimPruneBlockFn is the block before such a stage: BlockFn's arithmetic through block_forward_sequence / block_backward_sequence (the
one-call composite never shows qkv to Python), with the metric - and, when the stage also ranks by PageRank, the rank - launched right
after the attention forward as non-differentiable side outputs: GraphRankBlockFn's pattern, which stays as it is for a stage without
similarity pruning.  No hook sits between the halves, so stochastic depth works as in BlockFn.  Every other block stays on BlockFn.

The bf16 arithmetic mode is refused (SIM_PRUNE_BF16_ERROR): there qkv exists in bf16 only and the metric kernel is built for fp32."""
import torch

from . import functional as DF
from . import ops
from .lib import D2SError

SIM_PRUNE_BF16_ERROR = ("similarity pruning (sim_prune > 0, --sim-prune) runs in the fp32 arithmetic modes (exact, split): the key metric "
                        "is computed from the block's fp32 qkv, and in the bf16 arithmetic mode qkv exists in bf16 only")


def refuse_bf16():
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(SIM_PRUNE_BF16_ERROR)


@DF.mode_recorded
class SimPruneBlockFn(torch.autograd.Function):
    """One pre-norm transformer block on [B, n, D] tokens that also emits their key metric: x, the 12 block parameters, heads, eps,
    want_cls, scale, iters, s_attn, s_mlp (the block's stochastic-depth rows [B] or None) -> (y [B, n, D], cls_row [B, H, n] or an empty
    tensor, metric [B, n, 64], rank [B, H, n] or an empty tensor when iters == 0).  Differentiable in x and the parameters as BlockFn
    is; the CLS row, the metric and the rank carry no gradient."""

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
            side["metric"] = ops.key_metric(qkv, B, n, heads)                          # qkv exists here and nowhere later in eval
            if iters > 0:
                side["rank"] = ops.graph_rank(qkv, out[1], B, n, heads, scale, iters)
            return out

        y, cls_row, saved, _ = DF.block_forward_sequence(x.view(B * n, D), params, eps, False, train, attn, (), s_attn, s_mlp, n)
        if train:
            ctx.save_for_backward(x, *saved)
            ctx.drop_path = (s_attn, s_mlp)
            ctx.dims = (B, n, heads, scale)
        cls_row = DF.cls_or_empty(cls_row, x.device)
        rank = side["rank"] if iters > 0 else torch.empty(0, dtype=torch.float32, device=x.device)
        ctx.mark_non_differentiable(cls_row, side["metric"], rank)
        return y.view(B, n, D), cls_row, side["metric"], rank

    @staticmethod
    def backward(ctx, gy, _gcls, _gmetric, _grank):
        x, *saved = ctx.saved_tensors
        B, n, heads, scale = ctx.dims
        # input slots: x 0, the 12 parameters 1..12, heads eps want_cls scale iters s_attn s_mlp 13..19
        grads, _ = DF.block_backward_sequence(
            gy, x, saved, list(ctx.needs_input_grad[:13]), *ctx.drop_path, n,
            lambda qkv, ao, dao, lse, io, dqkvh, want_f32: DF.attn_backward(qkv, ao, dao, lse, B, n, heads, scale, None, None, io, dqkvh,
                                                                            want_f32))
        return tuple(grads) + (None,) * 7


def metric_block(x, params, heads, eps, scale, iters=0, want_cls=True, drop_path_rows=None):
    """SimPruneBlockFn on one block -> (y, cls_row or None, metric [B, n, 64], rank [B, H, n] or None)"""
    s_attn, s_mlp = drop_path_rows if drop_path_rows is not None else (None, None)
    y, cls_row, metric, rank = DF.run(SimPruneBlockFn, x, *params, heads, eps, bool(want_cls), scale, int(iters), s_attn, s_mlp)
    return y, (cls_row if want_cls else None), metric, (rank if int(iters) > 0 else None)
