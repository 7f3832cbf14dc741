"""Adaptive Token Sampling at inference (ATS, Fayyaz et al. 2022; DESIGN.md section 24 - the build's own definition, PARITY UNPINNED): a
block with a sampling stage between its attention half and its MLP half, on a ragged packed batch.

The block attends over every token it received; after the projection and the residual add only the sampled rows and CLS go on into the
MLP half and the later blocks (rows are independent after attention, so this equals attention for the sampled queries only).  The score
is the CLS softmax row the varlen attention already emits times the norm of the token's V, read from the block's own qkv; the count falls
out of the image (d2s_ats_select), so every image keeps its own number of tokens and the batch stays ragged.

ats_block_forward issues block_forward_sequence's launches with a hook between the halves: select (or replay a plan), the new offsets,
ONE host read of the new row total (it sizes every later launch, as at a threshold stage), the re-pack of the residual stream.  Both data
paths: fp32, and the bf16 path, where qkv exists in bf16 only and the kernel reads that; the residual stream and the re-pack are fp32."""
from . import functional as DF
from . import ops


def ats_block_forward(xp, cu, B, max_n, params, heads, eps, scale, K, N, row_src, plan=None):
    """xp [total, D] packed, cu [B+1], row_src [total] (original token index, 0 at CLS); at most K of an image's tokens survive.
    plan: (keep [total] float 0/1, counts [B] int32) of an earlier forward on the same batch, replayed instead of selecting.
    -> (y [total', D], cu' [B+1], row_src' [total'], max_n' = min(max_n, K + 1), (keep, counts), score [total] or None when replaying,
    dense_mask [B, N] or None when replaying).  Forward only."""
    io = DF.bf16_data_path(xp, xp.shape[1], params[8].shape[0])
    out = {}

    def sample(qkv, x1, cls_row):
        if plan is None:
            score, keep, counts, dense = ops.ats_select(cls_row, qkv, cu, row_src, K, N, B, heads, max_n)
        else:
            (keep, counts), score, dense = plan, None, None
        cu_new = ops.ragged_offsets(counts, extra=1)
        total = int(cu_new[-1])      # the one device sync of a stage: the packed row count sizes every later launch
        x1, src = ops.ragged_repack(x1, keep, cu, cu_new, row_src, total, B)
        out.update(cu=cu_new, row_src=src, plan=(keep, counts), score=score, dense=dense)
        return x1

    y, _, _, _ = DF.block_forward_sequence(xp, params, eps, io, False, DF._varlen_attn_forward, (cu, B, max_n, heads, scale, True),
                                           mid=sample, mid_cls=True)
    return y, out["cu"], out["row_src"], min(int(max_n), int(K) + 1), out["plan"], out["score"], out["dense"]
