"""A threshold stage on a ragged packed batch (inference with a dynamic keep ratio and more than one pruning stage, --ragged-cascade;
DESIGN.md section 10): the score predictor over all packed rows, forward only.

The reference cannot run a second threshold stage at inference (its stage scatters an n_kept-long mask into an N-long buffer,
vit_models/dynamic_vit.py:945-946), so this is the build's definition (PARITY UNPINNED): a stage scores, per image, the tokens that
survived the stages before it - the per-row layers per row, the "global half" (:540-544) the mean over that image's surviving non-CLS
tokens.  That is what the predictor gives on each image's kept subset alone.

ragged_predictor_forward issues the launch sequence of PredictorFn.forward (large LayerNorm predictor) or SmallPredictorFn.forward
(small_predictor=True) over ALL packed rows: the B CLS rows are computed and ignored (B extra rows instead of a strip copy), and
d2s_half_mean_concat_varlen stands where d2s_half_mean_concat stands in the dense sequence.

Training on the ragged batch (--ragged-train) makes that cascade differentiable: RaggedPackFn / RaggedRepackFn hand
the gradient back along the rows they moved (dropped rows get zeros), RaggedPredictorFn is the packed predictor with its backward,
ragged_head the final LayerNorm and classifier, RaggedMaskLossFn the mask loss of a packed stage.  The selection carries no gradient."""
import torch

from . import ops
from .functional import layernorm_backward, mode_recorded, wants_grad


def ragged_predictor_forward(predictor, xp, cu, B):
    """predictor: a PredictorLG (LayerNorm variants); xp [total, D] packed; cu [B+1].  -> scores [total], one per packed row (the entry
    at an image's CLS row has no meaning).  bf16 arithmetic mode follows PredictorFn: bf16 LayerNorm outputs feed the GEMMs, the last
    two Linear layers stay exact fp32 (the softmax and the selection behind them are fp32 kernels)."""
    if predictor.use_bn:
        raise NotImplementedError("the BatchNorm score predictor (predictor_bn=True) is not built for a ragged packed batch: more than "
                                  "one threshold stage at inference needs the LayerNorm predictor")
    params = predictor._params()
    total, D = xp.shape
    eps = 1e-5
    nl = (len(params) - 4) // 4
    cmap = ops.contiguous_map(total, D)
    if predictor.small_predictor:        # SmallPredictorFn.forward: fp32 activations, exact-erf GELU, current GEMM mode throughout
        h0, _, _ = ops.layernorm_fwd(xp, cmap, params[0], params[1], total, D, eps, stats=False)
        a1 = ops.linear_fwd(h0, params[2], params[3], epi=ops.EPI_BIAS_GELU)
        cur = ops.half_mean_concat_varlen(a1, cu, B)
        for j in range(nl):
            lw, lb, fw, fb = params[4 + 4 * j: 8 + 4 * j]
            width = cur.shape[1]
            ln, _, _ = ops.layernorm_fwd(cur, ops.contiguous_map(total, width), lw, lb, total, width, eps, stats=False)
            cur = ops.linear_fwd(ln, fw, fb) if j == nl - 1 else ops.linear_fwd(ln, fw, fb, epi=ops.EPI_BIAS_GELU)
        return cur.view(total)
    io = ops.bf16_io() and xp.is_cuda and D % 32 == 0
    if io:
        _, _, _, h0h = ops.layernorm_fwd_bf16(xp, cmap, params[0], params[1], total, D, eps, stats=False, want_f32=False)
        a1 = ops.linear_fwd(None, params[2], params[3], epi=ops.EPI_BIAS_RELU, a16=h0h)
    else:
        h0, _, _ = ops.layernorm_fwd(xp, cmap, params[0], params[1], total, D, eps, stats=False)
        a1 = ops.linear_fwd(h0, params[2], params[3], epi=ops.EPI_BIAS_RELU)
    cur = ops.half_mean_concat_varlen(a1, cu, B)
    for j in range(nl):
        lw, lb, fw, fb = params[4 + 4 * j: 8 + 4 * j]
        width = cur.shape[1]
        last = j == nl - 1
        exact_tail = j >= nl - 2
        if io and not exact_tail and width % 32 == 0:
            _, _, _, ln = ops.layernorm_fwd_bf16(cur, ops.contiguous_map(total, width), lw, lb, total, width, eps, stats=False, want_f32=False)
            cur = ops.linear_fwd(None, fw, fb, epi=ops.EPI_BIAS_RELU, a16=ln)
        else:
            ln, _, _ = ops.layernorm_fwd(cur, ops.contiguous_map(total, width), lw, lb, total, width, eps, stats=False)
            with ops.gemm_mode(ops.GEMM_EXACT if exact_tail else ops.get_gemm_mode()):
                cur = ops.linear_fwd(ln, fw, fb, epi=ops.EPI_BIAS if last else ops.EPI_BIAS_RELU)
    return cur.view(total)


# ---- training the dynamic keep ratio on the ragged batch (--ragged-train) ----------------------------------------
# The inference cascade made differentiable: what moves rows (pack, re-pack) hands the gradient back along the same rows, dropped rows get
# zeros; the selection itself carries no gradient.  The packed stage's predictor keeps what its backward needs and runs the backward of
# PredictorFn / SmallPredictorFn with d2s_half_mean_concat_varlen_bwd where the dense half-mean-concat backward stands.


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
    xp [total, D], cu [B+1], B, small, then the predictor's parameters -> scores [total].  The forward is ragged_predictor_forward's launch
    sequence on the fp32 data path (a training forward also keeps the LayerNorm statistics and, for the small predictor, the GELU
    pre-activations); the backward is PredictorFn's / SmallPredictorFn's over all packed rows."""

    @staticmethod
    def forward(ctx, xp, cu, B, small, *params):
        from .functional_ats import _BF16_REFUSAL
        from .lib import D2SError
        if ops.get_gemm_mode() == ops.GEMM_BF16:
            raise D2SError(_BF16_REFUSAL)
        total, D = xp.shape
        xp = xp.contiguous()
        eps = 1e-5
        train = wants_grad(ctx)
        nl = (len(params) - 4) // 4
        dev = xp.device
        h0, mean0, rstd0 = ops.layernorm_fwd(xp, ops.contiguous_map(total, D), params[0], params[1], total, D, eps, stats=train)
        if small:
            z1 = torch.empty((total, params[2].shape[0]), dtype=torch.float32, device=dev) if train else None
            a1 = ops.linear_fwd(h0, params[2], params[3], epi=ops.EPI_BIAS_GELU, aux_out=z1)
        else:
            a1 = ops.linear_fwd(h0, params[2], params[3], epi=ops.EPI_BIAS_RELU)
            z1 = a1                                       # the ReLU's backward reads its output
        cur = ops.half_mean_concat_varlen(a1, cu, B)
        saved = [xp, h0, mean0, rstd0, z1]
        for j in range(nl):
            lw, lb, fw, fb = params[4 + 4 * j: 8 + 4 * j]
            width = cur.shape[1]
            last = j == nl - 1
            ln, mean, rstd = ops.layernorm_fwd(cur, ops.contiguous_map(total, width), lw, lb, total, width, eps, stats=train)
            z = ln                                        # placeholder: a ReLU layer and the last layer keep no pre-activation
            if small:
                if last:
                    nxt = ops.linear_fwd(ln, fw, fb)
                else:
                    z = torch.empty((total, fw.shape[0]), dtype=torch.float32, device=dev) if train else ln
                    nxt = ops.linear_fwd(ln, fw, fb, epi=ops.EPI_BIAS_GELU, aux_out=z if train else None)
            else:
                with ops.gemm_mode(ops.GEMM_EXACT if j >= nl - 2 else ops.get_gemm_mode()):
                    nxt = ops.linear_fwd(ln, fw, fb, epi=ops.EPI_BIAS if last else ops.EPI_BIAS_RELU)
            saved += [cur, ln, mean, rstd, z]
            cur = nxt
        if train:
            ctx.save_for_backward(cu, *saved, *params)
            ctx.meta = (int(B), bool(small), total, D, nl, len(saved))
        return cur.view(total)

    @staticmethod
    def backward(ctx, gscores):
        B, small, total, D, nl, nsaved = ctx.meta
        cu = ctx.saved_tensors[0]
        saved = ctx.saved_tensors[1:1 + nsaved]
        params = ctx.saved_tensors[1 + nsaved:]
        xp, h0, mean0, rstd0, z1 = saved[:5]
        dev = gscores.device
        grads = [None] * len(params)
        want = [ctx.needs_input_grad[4 + i] for i in range(len(params))]
        d = gscores.contiguous().view(total, 1)
        for j in reversed(range(nl)):
            cur, ln, mean, rstd, _z = saved[5 + 5 * j: 10 + 5 * j]
            lw, lb, fw, fb = params[4 + 4 * j: 8 + 4 * j]
            base = 4 + 4 * j
            width = cur.shape[1]
            with ops.gemm_mode(ops.get_gemm_mode() if small or j < nl - 2 else ops.GEMM_EXACT):     # the arithmetic of this layer's forward
                grads[base + 2], grads[base + 3] = ops.linear_param_grads(d, ln, fw, fb, want[base + 2], want[base + 3])
                dln = ops.linear_dgrad(d, fw)
            # cur is the activation of layer j - 1 for j >= 1: the ReLU's backward folds into the LayerNorm backward, the GELU's is one
            # elementwise kernel on the saved pre-activation; for j == 0 cur is the split / mean / concat output
            d, grads[base], grads[base + 1] = layernorm_backward(cur, ops.contiguous_map(total, width), dln, lw, lb, mean, rstd,
                                                                 torch.empty((total, width), dtype=torch.float32, device=dev), total, width,
                                                                 want[base], want[base + 1], relu_mask=(not small and j >= 1))
            if small and j >= 1:
                d = ops.act_grad(d, saved[5 + 5 * (j - 1) + 4], "gelu")
        dz1 = ops.act_grad(ops.half_mean_concat_varlen_bwd(d, cu, B), z1, "gelu" if small else "relu")
        grads[2], grads[3] = ops.linear_param_grads(dz1, h0, params[2], params[3], want[2], want[3])
        gx = None
        if ctx.needs_input_grad[0] or want[0] or want[1]:
            dh0 = ops.linear_dgrad(dz1, params[2])
            gx, grads[0], grads[1] = layernorm_backward(xp, ops.contiguous_map(total, D), dh0, params[0], params[1], mean0, rstd0,
                                                        torch.empty((total, D), dtype=torch.float32, device=dev), total, D, want[0], want[1])
            if not ctx.needs_input_grad[0]:
                gx = None
        return (gx, None, None, None) + tuple(grads)


def ragged_predictor_train(predictor, xp, cu, B):
    """RaggedPredictorFn on a PredictorLG (LayerNorm variants) -> scores [total]; the BatchNorm predictor is refused as at inference"""
    from . import functional as DF
    if predictor.use_bn:
        raise NotImplementedError("the BatchNorm score predictor (predictor_bn=True) is not built for a ragged packed batch: more than "
                                  "one threshold stage at inference needs the LayerNorm predictor")
    return DF.run(RaggedPredictorFn, xp, cu, int(B), bool(predictor.small_predictor), *predictor._params())


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
