"""Adaptive Token Sampling (ATS, Fayyaz et al. 2022; DESIGN.md section 24 - the build's own definition, PARITY UNPINNED): a block with a
sampling stage between its attention half and its MLP half, on a ragged packed batch - ats_block_forward for inference, RaggedBlockFn
(functional.RouteBlockFn run on a _Ragged) to train through the stages.

The block attends over every token it received; after the projection and the residual add only the sampled rows and CLS go on into the
MLP half and the later blocks (rows are independent after attention, so this equals attention for the sampled queries only).  The score
is the CLS softmax row the varlen attention already emits times the norm of the token's V, read from the block's own qkv; the count falls
out of the image (d2s_ats_select), so every image keeps its own number of tokens and the batch stays ragged.

The seven block launches are functional.block_forward_sequence's and their backward is functional.block_backward_sequence's; what is
stated here is what a ragged block adds (_Ragged, a functional.BlockRoute): its refusals, the attention of either direction on the
packed batch, and the hook between the halves with its backward - select (or replay a plan), the new offsets, ONE host read of the
new row total (it sizes every later launch, as at a threshold stage), the re-pack of the residual stream.  Inference runs on both data paths: fp32, and the bf16 path, where qkv
exists in bf16 only and the kernel reads that; the residual stream and the re-pack are fp32.

Training (RaggedBlockFn, fp32 data path): the selection is a constant of the backward - score, keep and counts carry no gradient - so the
hook's backward is one row move (ops.ragged_repack_bwd: a kept row takes the gradient of the row it became, a dropped row zeros) and a
dropped row is reached only as a key and a value of the stage's own attention, whose backward is the varlen one (ops.attn_varlen_bwd).
The MLP half's residual gradient lives on the rows that left the stage, the attention half's on the rows that entered it.

Training in the bf16 arithmetic mode (_Ragged(..., bf16=True)): a block without a stage runs the same sequence
on the bf16 data path, its attention and the backward on the bf16 matrix cores (ops.attn_varlen_fwd_lse_bf16io / attn_varlen_bwd_bf16io).
The flag, not the mode, selects the path: without it the bf16 mode is refused as before.  A block WITH a stage joins it under
_Ragged(..., bf16=True, stage_bf16=True): the selection reads the bf16 qkv, the re-pack moves the fp32 residual
stream, and the hook's backward (sample_bwd_bf16: ops.ragged_repack_bwd with g16) writes the gradient of the rows that entered the stage
in fp32 and in bf16 in one launch - block_backward_sequence's mid_bwd_bf16 convention."""
import torch

from . import functional as DF
from . import ops
from .lib import D2SError

_BF16_REFUSAL = "training through a ragged block runs in the fp32 arithmetic modes (exact, split): the varlen attention backward is an fp32 kernel"
_BF16_STAGE_REFUSAL = (_BF16_REFUSAL + ".  A block with a sampling stage stays there with bf16=True too: behind the hook between the halves "
                       "(sample_bwd) the bf16 shadow of the gradient would have to be made again")
_BF16_MODE_REFUSAL = "a ragged block with bf16=True runs in the bf16 arithmetic mode only (ops.gemm_mode(GEMM_BF16))"
_STAGE_BF16_NEEDS_BF16 = "a ragged block with stage_bf16=True needs bf16=True too: stage_bf16 only lets a block with a stage onto the bf16 data path"


class _Ragged(DF.BlockRoute):
    """What a ragged packed batch puts into one block's launch sequence, and the constants of its backward (no gradient reaches them):
    a functional.BlockRoute.
    cu [B+1], row_src [total] (original token index, 0 at CLS), max_n the longest image.  K: the stage's token limit, or None for a
    block without a stage; plan: (keep, counts) of an earlier forward on the same batch, replayed instead of selecting.  After a stage's
    forward: cu_new, row_src_new, plan, score / dense (None when replaying); max_n_out either way.
    bf16: train on the bf16 data path in the bf16 arithmetic mode (a block without a stage) - attn and attn_bwd then honour io,
    dqkv16 and want_f32 as attn_forward / attn_backward do.
    stage_bf16: with bf16, a block with a stage runs there too - the hook's backward is then sample_bwd_bf16."""

    def __init__(self, cu, B, max_n, heads, scale, row_src=None, K=None, N=0, plan=None, bf16=False, stage_bf16=False):
        self.cu, self.B, self.max_n, self.heads, self.scale = cu, int(B), int(max_n), heads, float(scale)
        self.bf16, self.stage_bf16 = bool(bf16), bool(stage_bf16)
        self.row_src, self.K, self.N, self.plan = row_src, K, N, plan
        self.cu_new = self.row_src_new = self.score = self.dense = None
        self.max_n_out = self.max_n if K is None else min(self.max_n, int(K) + 1)

    def begin(self, xp, params):
        if self.stage_bf16 and not self.bf16:
            raise D2SError(_STAGE_BF16_NEEDS_BF16)
        if ops.get_gemm_mode() == ops.GEMM_BF16:
            if not self.bf16:
                raise D2SError(_BF16_REFUSAL)
            if self.K is not None and not self.stage_bf16:
                raise D2SError(_BF16_STAGE_REFUSAL)
        elif self.bf16:
            raise D2SError(_BF16_MODE_REFUSAL)
        return self.data_path(xp, params)

    def data_path(self, xp, params):
        """bf16=True: the bf16 data path (every GEMM input in bf16 only, the residual stream fp32), as BlockFn runs a dense block in that mode"""
        io = self.bf16 and DF.bf16_data_path(xp, xp.shape[1], params[8].shape[0])
        if self.bf16:
            if not io:
                raise D2SError("a ragged block with bf16=True needs the bf16 data path: widths that are multiples of 32, D2S_BF16_IO not 0")
            ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        return io

    def attn(self, qkv, keep, io, want_f32):
        """attn_forward's shape.  keep: the log-sum-exp is kept for attn_bwd - the fp32 kernel, or (bf16, on the bf16 data path) the bf16
        one; a forward that keeps nothing takes the varlen kernel without it."""
        if not keep:
            return DF._varlen_attn_forward(qkv, self.cu, self.B, self.max_n, self.heads, self.scale, self.K is not None, io, want_f32)
        if self.bf16 and io:
            out, lse, cls_rows, out16 = ops.attn_varlen_fwd_lse_bf16io(qkv, self.cu, self.B, qkv.shape[0], self.max_n, self.heads, self.scale,
                                                                       want_cls=self.K is not None, want_f32=want_f32)
            return out, lse, None, cls_rows, out16
        out, lse, cls_rows = ops.attn_varlen_fwd_lse(qkv, self.cu, self.B, qkv.shape[0], self.max_n, self.heads, self.scale,
                                                     want_cls=self.K is not None)
        return out, lse, None, cls_rows, None

    def attn_bwd(self, qkv, ao, dao, lse, io, dqkv16, want_f32):
        """attn_backward's shape"""
        if self.bf16 and io:
            return ops.attn_varlen_bwd_bf16io(qkv, self.cu, ao, dao, lse, self.B, qkv.shape[0], self.max_n, self.heads, self.scale,
                                              dqkv16=dqkv16, want_f32=want_f32), None
        return ops.attn_varlen_bwd(qkv, self.cu, ao, dao, lse, self.B, qkv.shape[0], self.max_n, self.heads, self.scale), None

    def sample(self, qkv, x1, cls_row):
        """block_forward_sequence's hook (mid_cls): select on the CLS rows and qkv (fp32, or bf16 on the bf16 data path) unless a plan is
        replayed, re-pack"""
        if self.plan is None:
            self.score, keep, counts, self.dense = ops.ats_select(cls_row, qkv, self.cu, self.row_src, self.K, self.N, self.B, self.heads,
                                                                  self.max_n)
            self.plan = (keep, counts)
        keep, counts = self.plan
        self.cu_new = ops.ragged_offsets(counts, extra=1)
        total = int(self.cu_new[-1])      # the one device sync of a stage: the packed row count sizes every later launch
        self.total_in = x1.shape[0]
        x1, self.row_src_new = ops.ragged_repack(x1, keep, self.cu, self.cu_new, self.row_src, total, self.B)
        return x1

    def sample_bwd(self, g1):
        """block_backward_sequence's hook: the gradient on the rows that left the stage -> on the rows that entered it"""
        return ops.ragged_repack_bwd(g1, self.plan[0], self.cu, self.cu_new, self.total_in, self.B)

    def sample_bwd_bf16(self, g1, g1h):
        """the same hook on the bf16 data path (block_backward_sequence's mid_bwd_bf16): g1h, the bf16 shadow of the rows that left the
        stage, ends here; the row move writes both forms of the gradient on the rows that entered it, the bf16 one the fp32 one rounded once"""
        g16 = ops.bf16_buffer(self.total_in, g1.shape[1], g1.device)
        return ops.ragged_repack_bwd(g1, self.plan[0], self.cu, self.cu_new, self.total_in, self.B, g16=g16), g16


    def hook(self):
        return (self.sample, True) if self.K is not None else (None, False)

    def hook_bwd(self):
        """a stage on the bf16 data path: the hook hands on both forms of the gradient"""
        if self.K is None:
            return None, False
        return (self.sample_bwd_bf16, True) if self.bf16 else (self.sample_bwd, False)


def ats_block_forward(xp, cu, B, max_n, params, heads, eps, scale, K, N, row_src, plan=None):
    """xp [total, D] packed, cu [B+1], row_src [total] (original token index, 0 at CLS); at most K of an image's tokens survive.
    plan: (keep [total] float 0/1, counts [B] int32) of an earlier forward on the same batch, replayed instead of selecting.
    -> (y [total', D], cu' [B+1], row_src' [total'], max_n' = min(max_n, K + 1), (keep, counts), score [total] or None when replaying,
    dense_mask [B, N] or None when replaying).  Forward only."""
    io = DF.bf16_data_path(xp, xp.shape[1], params[8].shape[0])
    r = _Ragged(cu, B, max_n, heads, scale, row_src, K, N, plan)
    y, _, _, _ = DF.block_forward_sequence(xp, params, eps, io, False, r.attn, (False,), mid=r.sample, mid_cls=True)
    return y, r.cu_new, r.row_src_new, r.max_n_out, r.plan, r.score, r.dense


# One transformer block on a ragged packed batch as a differentiable Function, with or without a sampling stage: xp [total, D], the 12
# block parameters, eps, the block's _Ragged, None -> (y [total', D],) (total' = total without a stage)
RaggedBlockFn = DF.RouteBlockFn


def ragged_block_train(xp, params, eps, r):
    """RaggedBlockFn on the block described by r (a _Ragged) -> y; afterwards r holds cu_new / row_src_new / plan / score / dense of a stage"""
    return DF.run(RaggedBlockFn, xp, *params, eps, r, None)[0]


class ClsGatherFn(torch.autograd.Function):
    """The CLS rows of a ragged packed batch: xp [total, D], cu [B+1] -> [B, D]; the backward scatters (zeros for every other row)."""

    @staticmethod
    def forward(ctx, xp, cu):
        ctx.save_for_backward(cu)
        ctx.total = xp.shape[0]
        return ops.gather_rows_i32(xp.contiguous(), cu, cu.numel() - 1)

    @staticmethod
    def backward(ctx, g):
        (cu,) = ctx.saved_tensors
        return ops.ragged_cls_scatter(g.contiguous(), cu, ctx.total), None
