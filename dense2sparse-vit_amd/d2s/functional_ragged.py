"""A threshold stage on a ragged packed batch (inference with a dynamic keep ratio and more than one pruning stage, --ragged-cascade;
DESIGN.md section 10): the score predictor over all packed rows, forward only.

The reference cannot run a second threshold stage at inference (its stage scatters an n_kept-long mask into an N-long buffer,
vit_models/dynamic_vit.py:945-946), so this is the build's definition (PARITY UNPINNED): a stage scores, per image, the tokens that
survived the stages before it - the per-row layers per row, the "global half" (:540-544) the mean over that image's surviving non-CLS
tokens.  That is what the predictor gives on each image's kept subset alone.

ragged_predictor_forward issues the launch sequence of PredictorFn.forward (large LayerNorm predictor) or SmallPredictorFn.forward
(small_predictor=True) over ALL packed rows: the B CLS rows are computed and ignored (B extra rows instead of a strip copy), and
d2s_half_mean_concat_varlen stands where d2s_half_mean_concat stands in the dense sequence."""
from . import ops


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
