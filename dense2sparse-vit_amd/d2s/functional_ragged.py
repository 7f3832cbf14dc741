"""A threshold stage on a ragged packed batch (inference with a dynamic keep ratio and more than one pruning stage, --ragged-cascade;
DESIGN.md section 10): the score predictor over all packed rows, forward only.

The reference cannot run a second threshold stage at inference (its stage scatters an n_kept-long mask into an N-long buffer,
vit_models/dynamic_vit.py:945-946), so this is the build's definition (PARITY UNPINNED): a stage scores, per image, the tokens that
survived the stages before it - the per-row layers per row, the "global half" (:540-544) the mean over that image's surviving non-CLS
tokens.  That is what the predictor gives on each image's kept subset alone.

ragged_predictor_forward runs the LayerNorm predictor's one launch sequence (functional.predictor_forward_sequence, large or
small_predictor=True) on the packed rows (functional.PredictorRows with cu): ALL packed rows go through it - the B CLS rows are computed
and ignored (B extra rows instead of a strip copy) - and d2s_half_mean_concat_varlen stands where d2s_half_mean_concat stands for dense
rows.

Training on the ragged batch (--ragged-train) makes that cascade differentiable: RaggedPackFn / RaggedRepackFn hand
the gradient back along the rows they moved (dropped rows get zeros), RaggedPredictorFn is the same sequence on the same rows with its
backward (functional.predictor_backward_sequence; fp32 data path, d2s_half_mean_concat_varlen_bwd and one d2s_act_grad where the dense
half-mean-concat backward stands), ragged_head the final LayerNorm and classifier, RaggedMaskLossFn the mask loss of a packed stage.  The selection carries no gradient.
In the bf16 arithmetic mode RaggedPredictorFn runs only when asked to (bf16=True), then on PredictorFn's data path."""
import torch

from . import ops
from .functional import (PredictorRows, mode_recorded, predictor_backward_sequence, predictor_bf16_data_path, predictor_forward_sequence,
                         wants_grad)

RAGGED_PREDICTOR_BN_ERROR = ("the BatchNorm score predictor (predictor_bn=True) is not built for a ragged packed batch: more than "
                             "one threshold stage at inference needs the LayerNorm predictor")


def ragged_predictor_forward(predictor, xp, cu, B):
    """predictor: a PredictorLG (LayerNorm variants); xp [total, D] packed; cu [B+1].  -> scores [total], one per packed row (the entry
    at an image's CLS row has no meaning).  Forward only.  bf16 arithmetic mode as in PredictorFn: the large predictor's bf16 LayerNorm
    outputs feed the GEMMs, its last two Linear layers stay exact fp32 (the softmax and the selection behind them are fp32 kernels)."""
    if predictor.use_bn:
        raise NotImplementedError(RAGGED_PREDICTOR_BN_ERROR)
    act = "gelu" if predictor.small_predictor else "relu"
    scores, _ = predictor_forward_sequence(xp, PredictorRows(xp, B, cu), predictor._params(), act, predictor_bf16_data_path(xp, act), False)
    return scores.view(xp.shape[0])


# ---- training the dynamic keep ratio on the ragged batch (--ragged-train) ----------------------------------------
# The inference cascade made differentiable: what moves rows (pack, re-pack) hands the gradient back along the same rows, dropped rows get
# zeros; the selection itself carries no gradient.


class RaggedPackFn(torch.autograd.Function):
    """The first threshold stage's pack: x [B, n, D], policy [B, n] (0/1, column 0 = CLS = 1; select_threshold(..., lead=1)), cu [B+1],
    total -> (packed [total, D], row_src [total]); rows and row_src are ops.ragged_pack's.  The backward is the re-pack backward on the
    uniform offsets cu_old[b] = b * n with the policy row as the keep vector."""

    @staticmethod
    def forward(ctx, x, policy, cu, total):
        B, n, D = x.shape
        x = x.contiguous()
        out, row_src = ops.ragged_pack(x, policy[:, 1:].contiguous(), cu, int(total))
        ctx.save_for_backward(policy.contiguous(), cu)
        ctx.dims = (B, n, D)
        ctx.mark_non_differentiable(row_src)
        return out, row_src

    @staticmethod
    def backward(ctx, g, _g_src):
        policy, cu = ctx.saved_tensors
        B, n, D = ctx.dims
        cu_old = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=g.device)
        gx = ops.ragged_repack_bwd(g.contiguous(), policy.view(B * n), cu_old, cu, B * n, B)
        return gx.view(B, n, D), None, None, None


class RaggedRepackFn(torch.autograd.Function):
    """A later stage's re-pack: xp [total, D], keep [total], cu_old, cu_new, row_src_old, total_new, B -> (packed [total_new, D],
    row_src_new); ops.ragged_repack, its backward ops.ragged_repack_bwd."""

    @staticmethod
    def forward(ctx, xp, keep, cu_old, cu_new, row_src_old, total_new, B):
        xp = xp.contiguous()
        out, row_src = ops.ragged_repack(xp, keep, cu_old, cu_new, row_src_old, int(total_new), int(B))
        ctx.save_for_backward(keep, cu_old, cu_new)
        ctx.dims = (xp.shape[0], int(B))
        ctx.mark_non_differentiable(row_src)
        return out, row_src

    @staticmethod
    def backward(ctx, g, _g_src):
        keep, cu_old, cu_new = ctx.saved_tensors
        total_old, B = ctx.dims
        return ops.ragged_repack_bwd(g.contiguous(), keep, cu_old, cu_new, total_old, B), None, None, None, None, None, None


@mode_recorded
class RaggedPredictorFn(torch.autograd.Function):
    """The LayerNorm score predictor (large: ReLU, or small_predictor: exact-erf GELU) over a packed batch as a differentiable Function:
    xp [total, D], cu [B+1], B, small, then the predictor's parameters -> scores [total].  ragged_predictor_forward's launch sequence on
    the fp32 data path - a training forward also keeps the LayerNorm statistics and, for the small predictor, the GELU pre-activations -
    and its backward.  A trailing True behind the parameters (as PredictorFn's trailing "gelu") selects the bf16 arithmetic mode: the
    sequence then runs with PredictorFn's data path (predictor_bf16_data_path: the large predictor's LayerNorms feed bf16 GEMMs, its tail
    stays exact fp32, the small predictor keeps fp32 activations; no bf16 form crosses the concat).  Without it that mode is refused."""

    @staticmethod
    def forward(ctx, xp, cu, B, small, *params):
        from .functional_ats import _BF16_MODE_REFUSAL, _BF16_REFUSAL
        from .lib import D2SError
        bf16 = bool(params) and params[-1] is True
        params = params[:len(params) // 4 * 4]
        if ops.get_gemm_mode() == ops.GEMM_BF16:
            if not bf16:
                raise D2SError(_BF16_REFUSAL)
        elif bf16:
            raise D2SError(_BF16_MODE_REFUSAL)
        xp = xp.contiguous()
        train = wants_grad(ctx)
        act = "gelu" if small else "relu"
        io = bf16 and predictor_bf16_data_path(xp, act)
        scores, saved = predictor_forward_sequence(xp, PredictorRows(xp, B, cu), params, act, io, train)
        if train:
            ctx.save_for_backward(cu, *saved, *params)          # saved[0] is xp
            ctx.meta = (int(B), act)
        return scores.view(xp.shape[0])

    @staticmethod
    def backward(ctx, gscores):
        B, act = ctx.meta
        np_ = (len(ctx.needs_input_grad) - 4) // 4 * 4
        cu, saved, params = ctx.saved_tensors[0], ctx.saved_tensors[1:-np_], ctx.saved_tensors[-np_:]
        grads = predictor_backward_sequence(gscores, PredictorRows(saved[0], B, cu), saved, params, act,
                                            ctx.needs_input_grad[:1] + ctx.needs_input_grad[4:4 + np_])
        return (grads[0], None, None, None) + tuple(grads[1:]) + (None,) * (len(ctx.needs_input_grad) - 4 - np_)


def ragged_predictor_train(predictor, xp, cu, B, bf16=False):
    """RaggedPredictorFn on a PredictorLG (LayerNorm variants) -> scores [total]; the BatchNorm predictor is refused as at inference.
    bf16: run in the bf16 arithmetic mode, on PredictorFn's data path (refused in an fp32 mode; without it the bf16 mode is refused)"""
    from . import functional as DF
    if predictor.use_bn:
        raise NotImplementedError(RAGGED_PREDICTOR_BN_ERROR)
    extra = (True,) if bf16 else ()
    return DF.run(RaggedPredictorFn, xp, cu, int(B), bool(predictor.small_predictor), *predictor._params(), *extra)


def ragged_head(xp, cu, norm, head):
    """Final LayerNorm over the packed rows, the CLS rows gathered, the classifier on them -> (logits [B, classes], normed [total, D]):
    a composition of LayerNormFn, ClsGatherFn and LinearFn"""
    from .functional import LinearFn
    from .functional_ats import ClsGatherFn
    from .functional_t2t import LayerNormFn
    xn = LayerNormFn.apply(xp, norm.weight, norm.bias, norm.eps)
    logits = LinearFn.apply(ClsGatherFn.apply(xn, cu), head.weight, head.bias, None)
    return logits, xn


class RaggedMaskLossFn(torch.autograd.Function):
    """The mask loss of a packed threshold stage: scores [total], target [B, N], cu, row_src, mode (ops.KL_PROB_TARGET | ops.MSE_TARGET),
    scale -> scale * sum_b loss_rows[b]; gradient to the scores only, exactly 0 at the CLS rows."""

    @staticmethod
    def forward(ctx, scores, target, cu, row_src, mode, scale):
        scores = scores.contiguous()
        loss_rows = ops.ragged_mask_loss_fwd(scores, target, cu, row_src, mode)
        ctx.save_for_backward(ops.ragged_mask_loss_bwd(scores, target, cu, row_src, mode, scale))
        return ops.sum_scalar(loss_rows, float(scale))

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return ops.scale_by_scalar(grad, g.contiguous(), 1.0), None, None, None, None, None
