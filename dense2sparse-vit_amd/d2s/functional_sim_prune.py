"""Similarity pruning (--sim-prune R; DESIGN.md section 30 - the build's own definition, PARITY UNPINNED): a stage of an attention-selecting
student takes k + r candidates by importance and prunes the r that resemble a more important candidate most (ops.sim_prune), by the
cosine of the key metric of the block before it (ops.key_metric, from that block's qkv).

metric_block is the block before such a stage: BlockFn's arithmetic through block_forward_sequence / block_backward_sequence (the
one-call composite never shows qkv to Python), with the metric - and, when the stage also ranks by PageRank, the rank - launched right
after the attention forward as non-differentiable side outputs: functional_graph_rank.rank_block with one more tap on its route.  No hook
sits between the halves, so stochastic depth works as in BlockFn.  Every other block stays on BlockFn.

The bf16 arithmetic mode is refused (SIM_PRUNE_BF16_ERROR): there qkv exists in bf16 only and the metric kernel is built for fp32."""
from . import functional as DF
from . import functional_graph_rank as GF
from . import ops
from .lib import D2SError

SIM_PRUNE_BF16_ERROR = ("similarity pruning (sim_prune > 0, --sim-prune) runs in the fp32 arithmetic modes (exact, split): the key metric "
                        "is computed from the block's fp32 qkv, and in the bf16 arithmetic mode qkv exists in bf16 only")


def refuse_bf16():
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(SIM_PRUNE_BF16_ERROR)


def _metric(route, qkv, lse, cinv):
    """DenseRoute's tap: the key metric, from the qkv the attention forward just read"""
    return ops.key_metric(qkv, *route.geom[:3])


def metric_block(x, params, heads, eps, scale, iters=0, want_cls=True, drop_path_rows=None):
    """One pre-norm transformer block on [B, n, D] tokens that also emits their key metric and, with iters > 0, their rank;
    drop_path_rows: the block's stochastic-depth rows (s_attn, s_mlp), [B] each or None.
    -> (y, cls_row [B, H, n] or None, metric [B, n, 64], rank [B, H, n] or None).  Differentiable in x and the parameters as BlockFn is;
    the CLS row, the metric and the rank carry no gradient."""
    B, n, _ = x.shape
    taps = (_metric, GF.rank_tap(int(iters))) if int(iters) > 0 else (_metric,)
    route = DF.DenseRoute(B, n, heads, scale, bool(want_cls), None, taps, drop_path_rows or (None, None), refuse_bf16)
    y, cls_row, metric, *rank = DF.run(DF.RouteBlockFn, x, *params, eps, route, None)
    return y, cls_row, metric, (rank[0] if rank else None)
