"""Token Merging (ToMe, Bolya et al. 2023): one transformer block that merges r tokens between its attention
branch and its MLP - tome_block_forward / tome_block_forward_bf16 for inference, ToMeBlockFn (functional.RouteBlockFn run on a
_Merging) to train through the merge.

    LayerNorm -> qkv GEMM -> attention -> proj + residual -> match -> merge -> LayerNorm -> fc1 + GELU -> fc2 + residual

The seven block launches are functional.block_forward_sequence's and their backward is functional.block_backward_sequence's; what is
stated here is what merging adds (_Merging, a functional.BlockRoute): its refusals, the hook between the halves, its backward, and the
attention of either direction.  The
match reads the keys of the qkv GEMM's output in place; the merge acts on x1 (after proj + residual), so the MLP half runs on n - r
rows.  Attention is the plain kernel while every token still stands for one patch (size is None) and the key-weighted one afterwards
(proportional attention).  The composite block call (ops.block_fwd) cannot serve here - the merge sits in the middle of the block: with
r = 0 and no sizes the result is bit for bit the per-op dense block's.  The bf16 arithmetic mode is refused by tome_block_forward and by
ToMeBlockFn without bf16 on its route (the key-weighted attention they call is an fp32 kernel; the GEMM modes exact and split both run);
tome_block_forward_bf16 is the same block on the bf16 data path at inference: LayerNorm and the GEMMs hand bf16 to each other,
attention and the match read the bf16 qkv (ops.attn_keyw_fwd_bf16io, ops.tome_match_bf16), the residual stream and therefore the merge
stay fp32.  ToMeBlockFn with bf16=True (tome_block_train(..., bf16=True)) trains on that data path.

Training: the merge is a size-weighted average with a constant plan (the match reads K under no gradient, as the published
bipartite_soft_matching does), so its backward is one scaled row copy per input row (ops.tome_merge_bwd); the attention backward takes
the key weights where the forward did (ops.attn_keyw_bwd).  The MLP half's residual gradient lives on n - r rows, the attention half's
on n.  On the bf16 data path the attention backward is ops.attn_keyw_bwd_bf16io (the bf16 matrix cores, dqkv in bf16 for the qkv
Linear's gradient GEMMs) and the merge backward also writes the bf16 form of the gradient it returns (ops.tome_merge_bwd with dx16), which
proj's two gradient GEMMs read: block_backward_sequence's mid_bwd_bf16 convention.
"""
import torch

from . import ops
from .functional import BlockRoute, RouteBlockFn, attn_backward, attn_forward, bf16_data_path, block_forward_sequence, run
from .lib import D2SError

_BF16_MODE_NEEDED = ("ToMeBlockFn with bf16=True trains on the bf16 data path: it needs the bf16 arithmetic mode "
                     "(ops.gemm_mode(ops.GEMM_BF16))")
_BF16_PATH_NEEDED = ("ToMeBlockFn with bf16=True needs the bf16 data path: D2S_BF16_IO not 0, D and hidden multiples of 32 and device "
                     "tensors")
_BF16_REFUSAL = "token merging runs in the fp32 arithmetic modes (exact, split): the key-weighted attention has no bf16 kernel"


class _Merging(BlockRoute):
    """What token merging puts into one block's launch sequence, and the constants of its backward (no gradient reaches them): a
    functional.BlockRoute.
    size [B, n] patches per token or None (all ones), r the merge count asked for (clipped here to (n - 1) // 2), plan (unm_idx, src_idx,
    dst_idx) to merge by instead of matching (a replay) or None, bf16: train on the bf16 data path (the bf16 arithmetic mode is then
    required, and widths that keep the data path on).  Afterwards: size_out [B, n - r] (size itself at r = 0), plan (None at r = 0),
    matched (the plan was made here)."""

    def __init__(self, size, B, n, D, heads, scale, r, prop_attn, plan, bf16=False):
        self.size, self.geom, self.heads, self.scale, self.bf16 = size, (B, n, D), heads, float(scale), bool(bf16)
        self.key_w = size if prop_attn else None
        self.r = ops.tome_clip_r(r, n)
        self.size_out, self.plan, self.matched = size, (plan if self.r > 0 else None), False

    def begin(self, x, params):
        if self.bf16:
            if ops.get_gemm_mode() != ops.GEMM_BF16:
                raise D2SError(_BF16_MODE_NEEDED)
            if not bf16_data_path(x, x.shape[2], params[8].shape[0]):
                raise D2SError(_BF16_PATH_NEEDED)
            ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        elif ops.get_gemm_mode() == ops.GEMM_BF16:
            raise D2SError(_BF16_REFUSAL)
        return self.bf16

    def attn(self, qkv, want_lse, io, want_f32):
        """attn_forward's shape: plain attention, or key-weighted once sizes exist and prop_attn is set"""
        B, n, _ = self.geom
        if self.key_w is None:
            return attn_forward(qkv, B, n, self.heads, self.scale, False, None, io, want_f32)
        if io:
            out, lse, out16 = ops.attn_keyw_fwd_bf16io(qkv, self.key_w, B, n, self.heads, self.scale, want_f32=want_f32)
            return out, lse, None, None, out16
        out, lse = ops.attn_keyw_fwd(qkv, self.key_w, B, n, self.heads, self.scale, want_lse=want_lse)
        return out, lse, None, None, None

    def attn_bwd(self, qkv, ao, dao, lse, io, dqkv16, want_f32):
        """attn_backward's shape, with the key weights where the forward took them"""
        B, n, _ = self.geom
        if self.key_w is None:
            return attn_backward(qkv, ao, dao, lse, B, n, self.heads, self.scale, None, None, io, dqkv16, want_f32)
        if io:
            return ops.attn_keyw_bwd_bf16io(qkv, self.key_w, ao, dao, lse, B, n, self.heads, self.scale, dqkv16=dqkv16, want_f32=want_f32), None
        return ops.attn_keyw_bwd(qkv, self.key_w, ao, dao, lse, B, n, self.heads, self.scale), None

    def merge(self, qkv, x1):
        """block_forward_sequence's hook: match on the keys of qkv (fp32, or bf16 on the bf16 data path) unless a plan is replayed, merge"""
        if self.r == 0:
            return x1
        if self.plan is None:
            match = ops.tome_match_bf16 if qkv.dtype == torch.bfloat16 else ops.tome_match
            self.plan, self.matched = match(qkv, *self.geom[:2], self.heads, self.r)[2:], True
        x1, self.size_out = ops.tome_merge(x1, self.size, *self.plan, *self.geom, self.r)
        return x1

    def merge_bwd(self, g1):
        """block_backward_sequence's hook: every one of the n input rows takes its output row's gradient, scaled where it was averaged"""
        if self.r == 0:
            return g1
        return ops.tome_merge_bwd(g1, self.size, self.size_out, *self.plan, *self.geom, self.r)

    def merge_bwd_bf16(self, g1, g1h):
        """the same hook on the bf16 data path (block_backward_sequence's mid_bwd_bf16): g1h, the bf16 shadow of the n - r rows, ends here;
        the merge backward writes the bf16 form of the n rows it returns in the same launch.  r = 0: both forms pass through."""
        if self.r == 0:
            return g1, g1h
        B, n, D = self.geom
        g1h = ops.bf16_buffer(B * n, D, g1.device)
        return ops.tome_merge_bwd(g1, self.size, self.size_out, *self.plan, B, n, D, self.r, dx16=g1h), g1h


    def hook(self):
        return self.merge, False

    def hook_bwd(self):
        return (self.merge_bwd_bf16, True) if self.bf16 else (self.merge_bwd, False)

    def side(self, cls_row):
        """(size_out or None while nothing has merged, unm_idx, src_idx, dst_idx of a plan matched here or None)"""
        return (self.size_out if self.r > 0 else None,) + (self.plan if self.matched else (None, None, None))


def _block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn, plan, io):
    rows, D = x.shape
    assert rows == B * n
    m = _Merging(size, B, n, D, heads, scale, r, prop_attn, plan)
    y, _, _, _ = block_forward_sequence(x, params, eps, io, False, m.attn, (False,), mid=m.merge)
    return y, m.size_out, m.plan


def tome_block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn=True, plan=None):
    """x [B * n, D] tokens, size [B, n] patches per token or None (all ones), params as Block._params(), r the merge count asked for (clipped
    here to (n - 1) // 2).  plan: (unm_idx, src_idx, dst_idx) to merge by instead of matching (a replay).
    -> (y [B * (n - r), D], size_out [B, n - r] or None while nothing has merged, (unm_idx, src_idx, dst_idx) or None when r == 0)"""
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(_BF16_REFUSAL)
    return _block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn, plan, False)


def tome_block_forward_bf16(x, size, params, B, n, heads, eps, scale, r, prop_attn=True, plan=None):
    """tome_block_forward on the bf16 data path (inference): block_forward_sequence with io=True, train=False.  Same arguments, same shape
    of a result.  With r = 0 and no sizes: bit for bit the bf16 forward-only block."""
    if not bf16_data_path(x, x.shape[1], params[8].shape[0]):
        raise D2SError("tome_block_forward_bf16 needs the bf16 data path: the bf16 arithmetic mode (ops.gemm_mode(ops.GEMM_BF16)), "
                       "D2S_BF16_IO not 0, D and hidden multiples of 32 and device tensors")
    return _block_forward(x, size, params, B, n, heads, eps, scale, r, prop_attn, plan, True)


# tome_block_forward as a differentiable Function: x [B, n, D], the 12 block parameters, eps, the block's _Merging, None
# -> (y [B, n - r, D], *_Merging.side(...)); only y is differentiable, in x and the parameters
ToMeBlockFn = RouteBlockFn


def tome_block_train(x, size, params, heads, eps, scale, r, prop_attn=True, plan=None, bf16=False):
    """ToMeBlockFn with tome_block_forward's shape of a result: x [B, n, D] -> (y [B, n - r, D], size_out or None, plan or None).
    bf16: train on the bf16 data path."""
    B, n, D = x.shape
    m = _Merging(size, B, n, D, heads, scale, r, bool(prop_attn), plan, bf16)
    y, size_out, unm, src, dst = run(ToMeBlockFn, x, *params, eps, m, None)
    if m.r == 0:
        return y, size, None
    return y, size_out, (plan if plan is not None else (unm, src, dst))
