"""Graph ranking (--graph-rank T; DESIGN.md section 29 - the build's own definition, PARITY UNPINNED): a stage of an attention-selecting
student ranks its tokens by T steps of PageRank over the attention graph of the block before it (ops.graph_rank, from that block's qkv and
the log-sum-exp its attention wrote) instead of by that block's CLS row alone.

rank_block is the block before such a stage: BlockFn's arithmetic through block_forward_sequence / block_backward_sequence (the
one-call composite never shows qkv and lse to Python) - functional.RouteBlockFn on a functional.DenseRoute - with the rank a tap, launched
right after the attention forward as a non-differentiable side output.  No hook sits between the halves, so stochastic depth works as in
BlockFn.  Every other block of the model stays on BlockFn.

The bf16 arithmetic mode is refused (GRAPH_RANK_BF16_ERROR): there qkv exists in bf16 only and the rank kernel is built for fp32."""
from . import functional as DF
from . import ops
from .lib import D2SError

GRAPH_RANK_BF16_ERROR = ("graph ranking (graph_rank_iters > 0, --graph-rank) runs in the fp32 arithmetic modes (exact, split): the rank is "
                         "recomputed from the block's fp32 qkv and the fp32 attention's log-sum-exp, and in the bf16 arithmetic mode qkv "
                         "exists in bf16 only")


def refuse_bf16():
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(GRAPH_RANK_BF16_ERROR)


def rank_tap(iters):
    """DenseRoute's tap: the rank, from qkv and the log-sum-exp the attention forward just wrote"""
    return lambda route, qkv, lse, cinv: ops.graph_rank(qkv, lse, *route.geom, iters)


def rank_block(x, params, heads, eps, scale, iters, want_cls=True, drop_path_rows=None):
    """One pre-norm transformer block on [B, n, D] tokens that also ranks them; drop_path_rows: the block's stochastic-depth rows
    (s_attn, s_mlp), [B] each or None.  -> (y, cls_row [B, H, n] or None, rank [B, H, n]).  Differentiable in x and the parameters as
    BlockFn is; the CLS row and the rank carry no gradient."""
    B, n, _ = x.shape
    route = DF.DenseRoute(B, n, heads, scale, bool(want_cls), None, (rank_tap(int(iters)),), drop_path_rows or (None, None), refuse_bf16)
    return DF.run(DF.RouteBlockFn, x, *params, eps, route, None)
