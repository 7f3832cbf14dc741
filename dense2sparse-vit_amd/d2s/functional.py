"""Autograd glue: one torch.autograd.Function per module of the hot path.  Forward and backward are explicit
sequences of C-ABI calls (d2s.ops); torch only owns the tensors and the graph.  No torch arithmetic runs here.

The transformer block's seven launches (LayerNorm, qkv GEMM, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual) are
written once, in block_forward_sequence, and their backward once, in block_backward_sequence.  What a block adds around them - its
refusals, its attention of either direction, taps behind the attention forward, a hook between the halves, stochastic-depth rows, side
outputs - is a BlockRoute: DenseRoute here, functional_ats._Ragged (and functional_ltp._RaggedLTP) for a ragged packed batch,
functional_tome._Merging for token merging.  The autograd glue around the sequences is written once too: route_forward / route_backward,
behind RouteBlockFn (any route: the graph-rank, similarity-pruning and LTP soft blocks, ragged and LTP stage blocks, the token-merging
block) and behind BlockFn's per-op branch (a DenseRoute without a tap).  The forward sequence's callers: route_forward and the forward-only
helpers ragged_block_forward, functional_ats.ats_block_forward and functional_tome._block_forward; the backward sequence's one caller:
route_backward.  In front of both BlockFn keeps the composite path (ops.block_fwd / block_bwd: one C-ABI call for the same launches on
the fp32 data path).  Which attention entry runs is decided in attn_forward /
attn_backward, for BlockFn and AttnCoreFn alike; xarg, cls_or_empty and layernorm_backward are the small shared pieces (the latter also
serves the predictor and Tokens-to-Token Functions of the neighbouring modules).

The LayerNorm score predictor is written once in the same way: predictor_forward_sequence / predictor_backward_sequence, parameterised by
where the rows are (PredictorRows: dense or packed), the activation (ReLU: large, exact-erf GELU: small), the bf16 data path and whether
anything is kept for a backward.  Callers: PredictorFn here (dense; both predictors) and, for a ragged packed batch, functional_ragged's
ragged_predictor_forward and RaggedPredictorFn.  The BatchNorm predictor (functional_bn) and the DynamicViT baseline's
(functional_dynamicvit) are sequences of their own.

Reference lines (relative to /root/reference):
  EmbedFn      vit_models/dynamic_vit.py:300-306, 820-823
  BlockFn      vit_models/dynamic_vit.py:263-269 (Block), :216-236 (Attention), :169-175 (Mlp)
  PredictorFn  vit_models/dynamic_vit.py:536-551 with layers :491-531 (large) and :409-426 (small, --small-predictor)
  GatherFn     vit_models/dynamic_vit.py:907-912
  HeadFn       vit_models/dynamic_vit.py:993-1006
"""
import threading
import weakref

import torch

from . import ops

_DH = 64


def _zeros_like_param(p):
    return torch.zeros_like(p)


def _need(ctx, i):
    return ctx.needs_input_grad[i]


_tls = threading.local()


def run(fn, *args):
    """fn.apply(*args) with the grad mode decided HERE: inside Function.forward grad mode is always off and ctx.needs_input_grad only
    reflects the inputs' requires_grad, so under torch.no_grad() a trainable model (the student in evaluate.py) would take the
    training path - LayerNorm statistics, the GELU pre-activation copy, save_for_backward.  The flag makes the forward-only fast paths
    of BlockFn / EmbedFn / PredictorFn / HeadFn the ones that run (the tensors themselves are passed unchanged: detached aliases would
    defeat the identity checks of the weight caches in d2s.ops)."""
    if torch.is_grad_enabled():
        return fn.apply(*args)
    prev = getattr(_tls, "no_grad", False)
    _tls.no_grad = True
    try:
        return fn.apply(*args)
    finally:
        _tls.no_grad = prev


def wants_grad(ctx):
    """Does this forward have to keep anything for a backward?"""
    return any(ctx.needs_input_grad) and not getattr(_tls, "no_grad", False)


def mode_recorded(cls):
    """Class decorator for Functions that launch GEMM / attention kernels: the forward records the arithmetic mode it ran in
    (ops.get_gemm_mode(): the process default or the caller's `with ops.gemm_mode(...)`), the backward - which autograd runs on its
    own thread, outside the caller's block - re-enters it, so forward and backward of one module always use the same arithmetic."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args):
        ctx.gmode = ops.get_gemm_mode()
        return fwd(ctx, *args)

    def backward(ctx, *grads):
        with ops.gemm_mode(ctx.gmode):
            return bwd(ctx, *grads)

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


# Teacher and student embed the SAME image batch (train.py:40,43): inside `shared_patch_columns()` the im2col matrix of an image
# tensor is built once and handed to every EmbedFn that asks for it (same tensor object, same version counter, same patch size,
# same stream).  The block is what bounds the cache's lifetime - nothing is kept once it exits.
_COLS = {"depth": 0, "entry": None}


class shared_patch_columns:
    def __enter__(self):
        _COLS["depth"] += 1
        return self

    def __exit__(self, *exc):
        _COLS["depth"] -= 1
        if _COLS["depth"] == 0:
            _COLS["entry"] = None
        return False


def _patch_columns(img, patch):
    if _COLS["depth"] == 0:
        return ops.im2col_patch(img, patch)
    stream = torch.cuda.current_stream(img.device).cuda_stream
    ent = _COLS["entry"]
    if ent is not None and ent[0]() is img and ent[1:3] == (img._version, patch) and ent[3] in (stream, None):
        return ent[4]
    col = ops.im2col_patch(img, patch)
    _COLS["entry"] = (weakref.ref(img), img._version, patch, stream, col)
    return col


def prime_patch_columns(img, patch):
    """Build the im2col matrix of `img` now, on the current stream, and mark it usable from ANY stream: for a caller that then forks
    work onto a second stream which first waits on this one (d2s.engine.TrainStep with the teacher on its own stream)."""
    if _COLS["depth"] == 0:
        return
    img = img.contiguous()
    _COLS["entry"] = (weakref.ref(img), img._version, patch, None, ops.im2col_patch(img, patch))


@mode_recorded
class EmbedFn(torch.autograd.Function):
    """img [B,3,H,W] -> tokens [B, T+1, D]  (conv-as-GEMM with the bias + pos_embed add fused in the epilogue)."""

    @staticmethod
    def forward(ctx, img, proj_w, proj_b, cls_token, pos_embed, patch):
        B = img.shape[0]
        D = proj_w.shape[0]
        col = _patch_columns(img.contiguous(), patch)
        T = col.shape[0] // B
        Kc = col.shape[1]
        tokens = torch.empty((B, T + 1, D), dtype=torch.float32, device=img.device)
        w2 = proj_w.reshape(D, Kc)
        pos = pos_embed.reshape(T + 1, D)
        ops.gemm(ops.NT, col, Kc, w2, Kc, tokens, D, B * T, D, Kc, ops.EPI_BIAS_ROWADD, proj_b, pos[1:], D, None, T, T, 1)
        ops.fill_cls(cls_token.reshape(D), pos, tokens)
        if wants_grad(ctx):       # forward-only callers (frozen teacher, eval) keep nothing
            ctx.save_for_backward(col, proj_w, proj_b, cls_token, pos_embed)
            ctx.dims = (B, T, D, Kc, tuple(proj_w.shape))
        return tokens

    @staticmethod
    def backward(ctx, g):
        col, proj_w, proj_b, cls_token, pos_embed = ctx.saved_tensors
        B, T, D, Kc, wshape = ctx.dims
        g = g.contiguous()
        dw = db = dcls = dpos = None
        if _need(ctx, 1) or _need(ctx, 2):
            gp = ops.copy_rows(g, ops.skip_cls_map(T + 1, D), B * T, D)
            db = ops.grad_buffer(proj_b) if _need(ctx, 2) else None
            if _need(ctx, 1):
                dw = ops.grad_buffer(proj_w)
                ops.linear_wgrad(gp, col, dw.view(D, Kc), db=db)
            elif db is not None:
                ops.colsum(gp, db)
        if _need(ctx, 3) or _need(ctx, 4):
            dpos = ops.grad_buffer(pos_embed)
            ops.batch_sum(g, dpos, B, (T + 1) * D, (T + 1) * D)
            if _need(ctx, 3):
                dcls = ops.batch_sum(g, ops.grad_buffer(cls_token), B, D, (T + 1) * D)
            if not _need(ctx, 4):
                dpos = None
        return None, dw, db, dcls, dpos, None


def bf16_data_path(t, D, hidden):
    """bf16 arithmetic mode with the bf16 data path on, for a block of these widths: every GEMM input exists in bf16 (section 7 of
    DESIGN.md); the kernels need multiples of 32."""
    return ops.bf16_io() and D % 32 == 0 and hidden % 32 == 0 and t.is_cuda


def xarg(t):
    """A saved layer input is fp32, or bf16 only on the bf16 data path -> the (x, x16) pair the GEMM wrappers take."""
    return (None, t) if t.dtype == torch.bfloat16 else (t, None)


def cls_or_empty(cls_row, device):
    """A Function returns a tensor in every slot: the placeholder for CLS rows that were not asked for."""
    return torch.empty((0,), device=device) if cls_row is None else cls_row


def layernorm_backward(x, rowmap, dy, w, b, mean, rstd, dx, rows, D, want_w, want_b, add_src=None, relu_mask=False, dx16=None):
    """ops.layernorm_bwd into `dx`.  The kernel produces the weight and the bias gradient together: both buffers are made when either is
    wanted.  -> (dx, dw if wanted else None, db if wanted else None)"""
    dw = ops.grad_buffer(w) if (want_w or want_b) else None
    db = ops.grad_buffer(b) if dw is not None else None
    ops.layernorm_bwd(x, rowmap, dy, w, mean, rstd, dx, add_src, dw, db, rows, D, relu_mask=relu_mask, dx16=dx16)
    return dx, (dw if want_w else None), (db if want_b else None)


def attn_forward(qkv, B, n, H, scale, want_cls, policy, io, want_f32=True, want_bf16=True):
    """The attention forward of a dense [B * n, 3 * H * 64] qkv: plain or softmax_with_policy (:195-214, fused), fp32 kernels or (io) the
    bf16 matrix cores, which take qkv in fp32 or bf16 and also (or only: want_f32 / want_bf16) write the bf16 form of the output.
    -> (out or None, lse, cinv or None, cls_row or None, out16 or None)"""
    if policy is None:
        if io:
            out, lse, cls_row, out16 = ops.attn_fwd_bf16io(qkv, B, n, H, scale, want_cls, want_f32=want_f32)
            return out, lse, None, cls_row, out16
        out, lse, cls_row = ops.attn_fwd(qkv, B, n, H, scale, want_cls)
        return out, lse, None, cls_row, None
    if io:
        return ops.attn_policy_fwd_bf16io(qkv, policy, B, n, H, scale, want_cls=want_cls, want_f32=want_f32, want_bf16=want_bf16)
    out, lse, cinv, cls_row = ops.attn_policy_fwd(qkv, policy, B, n, H, scale, want_cls=want_cls)
    return out, lse, cinv, cls_row, None


def attn_backward(qkv, out, dout, lse, B, n, H, scale, policy, cinv, io, dqkv16=None, want_f32=True, want_dpolicy=False):
    """Backward of attn_forward.  dqkv16 (bf16 kernels): bf16 buffer that receives a copy of dqkv, the only form written with
    want_f32=False.  A constant mask keeps its launches; a policy that is learnt through (DynamicViT baseline) costs one more column sum
    in the dK/dV pass.  -> (dqkv or None, dpolicy or None)"""
    if policy is None:
        return ops.attn_bwd(qkv, out, dout, lse, B, n, H, scale, dqkv16=dqkv16, want_f32=want_f32), None
    if io:
        return ops.attn_policy_bwd_bf16io(qkv, policy, out, dout, lse, cinv, B, n, H, scale, dqkv16=dqkv16, want_f32=want_f32,
                                          want_dpolicy=want_dpolicy)
    if want_dpolicy:
        return ops.attn_policy_bwd_dpol(qkv, policy, out, dout, lse, cinv, B, n, H, scale)
    return ops.attn_policy_bwd(qkv, policy, out, dout, lse, cinv, B, n, H, scale), None


def _varlen_attn_forward(qkv, cu, B, max_n, H, scale, want_cls, io, want_f32):
    """attn_forward's shape for a ragged packed batch (per image through cu_seqlens; forward only, no policy)"""
    if io:
        out, cls_rows, out16 = ops.attn_varlen_fwd_bf16io(qkv, cu, B, qkv.shape[0], max_n, H, scale, want_cls=want_cls, want_f32=want_f32)
        return out, None, None, cls_rows, out16
    out, cls_rows = ops.attn_varlen_fwd(qkv, cu, B, qkv.shape[0], max_n, H, scale, want_cls=want_cls)
    return out, None, None, cls_rows, None


def _norm_linear(x, cmap, nw, nb, w, b, eps, io, train, epi=None, aux_out=None):
    """LayerNorm and the Linear that reads it, each written in the one form the data path keeps: fp32, or (io) bf16 only - the bf16
    attention kernels and the next GEMM round their input to bf16 anyway.  Statistics only when training.
    -> (LayerNorm output if train else None, Linear output, mean, rstd)"""
    rows, D = x.shape
    if io:
        _, mean, rstd, ln = ops.layernorm_fwd_bf16(x, cmap, nw, nb, rows, D, eps, stats=train, want_f32=False)
        y = ops.bf16_buffer(rows, w.shape[0], x.device)
        ops.linear_fwd(None, w, b, epi=epi, aux_out=aux_out, a16=ln, c16=y, want_f32=False)
    else:
        ln, mean, rstd = ops.layernorm_fwd(x, cmap, nw, nb, rows, D, eps, stats=train)
        y = ops.linear_fwd(ln, w, b, epi=epi, aux_out=aux_out)
    return (ln if train else None), y, mean, rstd


def block_forward_sequence(x, params, eps, io, train, attn, attn_args, s_attn=None, s_mlp=None, rows_per_group=0, mid=None, mid_cls=False):
    """THE launch sequence of a pre-norm transformer block on [rows, D] tokens: LayerNorm, qkv GEMM, attention, proj + residual, LayerNorm,
    fc1 + GELU, fc2 + residual.  Callers: route_forward (BlockFn's per-op branch and RouteBlockFn, forward only and training) and the
    forward-only ragged_block_forward, functional_ats.ats_block_forward and functional_tome._block_forward.
    io: bf16 data path - every GEMM input exists in bf16 only, the residual stream stays fp32.
    train: keep the LayerNorm statistics, the GELU pre-activation and every layer input for block_backward_sequence; otherwise (the frozen
    teacher, eval) nothing is kept and each intermediate dies before the next allocation (the pre-activation alone is 155 MB per block at
    B = 128), on the bf16 data path not even the fp32 form of the attention output is written.
    attn(qkv, *attn_args, io, want_f32) is attn_forward or a function of its shape.  s_attn / s_mlp: stochastic-depth row scales of the
    two branches, one per rows_per_group rows.
    mid(qkv, x1) -> x1', the hook between the halves (token merging): x1' may have fewer rows than x1, the MLP half runs on them and only
    x1' is kept; qkv then lives until the hook has returned.  mid_cls: the hook is called mid(qkv, x1, cls_row) instead (adaptive token
    sampling scores by the CLS softmax row the attention emitted).
    -> (y, cls_row or None, what block_backward_sequence unpacks (None unless train), cinv)"""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = params
    rows, D = x.shape
    assert mid is None or (s_attn is None and s_mlp is None), "stochastic depth is not built for a block with a hook between its halves"
    ln1, qkv, mean1, rstd1 = _norm_linear(x, ops.contiguous_map(rows, D), n1w, n1b, qkvw, qkvb, eps, io, train)
    ao, lse, cinv, cls_row, aoh = attn(qkv, *attn_args, io, train)      # training keeps the fp32 output for the backward's delta
    if not train:
        del lse, cinv
        if mid is None:
            del qkv
    x1 = ops.linear_fwd(ao, projw, projb, epi=ops.EPI_BIAS_RESID, aux=x, a16=aoh, rowscale=s_attn, rows_per_group=rows_per_group)
    if not train:
        del ao, aoh
    if mid is not None:
        x1 = mid(qkv, x1, cls_row) if mid_cls else mid(qkv, x1)          # the x1 that went in dies here
        rows = x1.shape[0]
        if not train:
            del qkv
    # GELU pre-activation for the backward: fp32, or bf16 on the bf16 data path (what autocast keeps: fc1's output is bf16 there)
    z = torch.empty((rows, fc1w.shape[0]), dtype=torch.bfloat16 if io else torch.float32, device=x.device) if train else None
    ln2, h, mean2, rstd2 = _norm_linear(x1, ops.contiguous_map(rows, D), n2w, n2b, fc1w, fc1b, eps, io, train, ops.EPI_BIAS_GELU, z)
    hx, h16 = xarg(h)
    y = ops.linear_fwd(hx, fc2w, fc2b, epi=ops.EPI_BIAS_RESID, aux=x1, a16=h16, rowscale=s_mlp, rows_per_group=rows_per_group)
    if not train:
        return y, cls_row, None, None
    return y, cls_row, (n1w, qkvw, projw, n2w, fc1w, fc2w, mean1, rstd1, ln1, qkv, ao, lse, x1, mean2, rstd2, ln2, z, h,
                        n1b, qkvb, projb, n2b, fc1b, fc2b, aoh), cinv      # aoh: bf16 form of ao (bf16 attention only), proj's weight gradient


def block_backward_sequence(gy, x, saved, wants, s_attn, s_mlp, rows_per_group, attn_bwd, mid_bwd=None, mid_bwd_bf16=False):
    """The backward of block_forward_sequence (training; per-op, either data path).  gy: the gradient of y; x: the block's input as a
    [..., D] tensor; saved: what the forward sequence returned for this; wants: which of (x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b,
    fc1w, fc1b, fc2w, fc2b) take a gradient; s_attn / s_mlp: the forward's stochastic-depth row scales.
    attn_bwd(qkv, ao, dao, lse, io, dqkv16, want_f32) -> (dqkv or None, dpolicy or None) is attn_backward or a function of its shape.
    mid_bwd(g1) -> g1 on the rows of x, the backward of the forward's hook: the MLP half runs on the rows of gy, the attention half on the
    rows of x, and the first LayerNorm backward adds the gradient that left the hook.
    mid_bwd_bf16: the hook also delivers the bf16 form of the gradient it returns, which lets it run on the bf16 data path: it is called
    mid_bwd(g1, g1h) -> (g1, g1h) with the bf16 shadow of the MLP half's rows (LayerNorm-2's backward made it; it ends at the hook) and
    hands back both forms on the rows of x - the bf16 one feeds proj's two gradient GEMMs.  A hook without it stays on the fp32 data path.
    -> (the 13 gradients in wants' order, gx shaped like x, None where not wanted; dpolicy)"""
    (n1w, qkvw, projw, n2w, fc1w, fc2w, mean1, rstd1, ln1, qkv, ao, lse, x1, mean2, rstd2, ln2, z, h,
     n1b, qkvb, projb, n2b, fc1b, fc2b, aoh) = saved
    D = x.shape[-1]
    M = x.numel() // D
    dev = gy.device
    gy = gy.contiguous().view(-1, D)
    M2 = gy.shape[0]          # rows of the MLP half: M, or fewer behind a hook
    grads = [None] * 13

    # ---- MLP branch ----
    hx, h16 = xarg(h)
    # bf16 data path: every gradient that feeds an input-gradient GEMM is also produced in bf16 by the kernel that computes it
    io = bf16_data_path(gy, D, z.shape[1])
    # behind a hook the bf16 shadow of g1 would have to be made again for the rows of x, and the row scales' groups differ between the halves
    assert mid_bwd is None or ((not io or mid_bwd_bf16) and s_attn is None and s_mlp is None), \
        "a hook between the halves: fp32 data path, no stochastic depth"
    gyh = ops.shadow_take(gy) if io else None
    if gyh is not None:
        gyh = gyh.view(M2, D)
    # stochastic depth: the gradient that enters a branch is s[b] * g (one pass, ops.scale_rows); the residual path - the LayerNorm
    # backward's add_src - keeps the unscaled one.  The bf16 shadow of the unscaled gradient does not describe the scaled copy.
    g_res = gy
    if s_mlp is not None:
        gy, gyh = ops.scale_rows(g_res, s_mlp, rows_per_group), None
    # with both operands at hand in bf16 the weight-gradient kernel reads them where they lie (token-major, no transposing pass); the
    # bias gradient is then the sum of the bf16 gradient values, as under torch.autocast
    grads[11], grads[12] = ops.linear_param_grads(gy, hx, fc2w, fc2b, wants[11], wants[12], x16=h16, dy16=gyh if h16 is not None else None)
    dzh = ops.bf16_buffer(M2, z.shape[1], dev) if io else None
    l2x, l216 = xarg(ln2)
    # dz = (gy fc2w) * gelu'(z) feeds two bf16 GEMMs and nothing else: on the bf16 data path only its bf16 form is written (fc1's bias
    # gradient is then the fp32 sum of those bf16 values, as under torch.autocast)
    dz_bf16_only = dzh is not None and l216 is not None and wants[9]
    dz = ops.linear_dgrad(gy, fc2w, epi=ops.EPI_MUL_GELU_GRAD, aux=z, a16=gyh, c16=dzh, want_f32=not dz_bf16_only)
    del gyh
    grads[9], grads[10] = ops.linear_param_grads(dz, l2x, fc1w, fc1b, wants[9], wants[10], x16=l216, dy16=dzh if dz_bf16_only else None)
    dln2 = ops.linear_dgrad(dz, fc1w, a16=dzh)
    del dzh
    g1h = ops.bf16_buffer(M2, D, dev) if (io and s_attn is None) else None
    g1, grads[7], grads[8] = layernorm_backward(x1, ops.contiguous_map(M2, D), dln2, n2w, n2b, mean2, rstd2,
                                                torch.empty((M2, D), dtype=torch.float32, device=dev), M2, D, wants[7], wants[8],
                                                add_src=g_res, dx16=g1h)
    if mid_bwd is not None:
        g1, g1h = mid_bwd(g1, g1h) if (io and mid_bwd_bf16) else (mid_bwd(g1), None)
    # ---- attention branch ----
    ga = g1
    if s_attn is not None:
        ga, g1h = ops.scale_rows(g1, s_attn, rows_per_group), None
    grads[5], grads[6] = ops.linear_param_grads(ga, ao, projw, projb, wants[5], wants[6], x16=aoh, dy16=g1h if aoh is not None else None)
    dao = ops.linear_dgrad(ga, projw, a16=g1h)
    del g1h
    l1x, l116 = xarg(ln1)
    dqkvh = torch.empty(qkv.shape, dtype=torch.bfloat16, device=dev) if io else None
    dqkv_bf16_only = io and l116 is not None and wants[3]      # both consumers (weight gradient, input gradient) read the bf16 form
    dqkv, dpolicy = attn_bwd(qkv, ao, dao, lse, io, dqkvh, not dqkv_bf16_only)
    grads[3], grads[4] = ops.linear_param_grads(dqkv, l1x, qkvw, qkvb, wants[3], wants[4], x16=l116, dy16=dqkvh if dqkv_bf16_only else None)
    if wants[0] or wants[1] or wants[2]:
        dln1 = ops.linear_dgrad(dqkv, qkvw, a16=dqkvh)
        del dqkvh
        gxh = ops.bf16_buffer(M, D, dev) if (io and wants[0]) else None
        gx, grads[1], grads[2] = layernorm_backward(x, ops.contiguous_map(M, D), dln1, n1w, n1b, mean1, rstd1,
                                                    torch.empty((M, D), dtype=torch.float32, device=dev), M, D, wants[1], wants[2],
                                                    add_src=g1, dx16=gxh)
        if wants[0]:
            grads[0] = gx.view(x.shape)
        if gxh is not None:
            ops.shadow_put(grads[0], gxh)
    return grads, dpolicy


class BlockRoute:
    """What one block puts into the launch sequence around the seven launches, and the constants of its backward (no gradient reaches
    them).  RouteBlockFn runs any route, BlockFn a DenseRoute on its per-op branch; functional_ats._Ragged and functional_tome._Merging
    are the routes with a hook between the halves.  A route answers, and nothing more:
    begin(x, params) -> io: raises the refusals of the current arithmetic mode, in the route's own order; says whether the block runs on
    the bf16 data path; clears the gradient shadows where the route's backward may make new ones.
    attn(qkv, keep, io, want_f32): attn_forward's shape.  keep: this forward keeps something for a backward (a route may take a kernel
    without the log-sum-exp otherwise).  Taps - launches that read qkv and the log-sum-exp - follow the attention in here: in eval both
    exist nowhere later.
    attn_bwd(qkv, ao, dao, lse, io, dqkv16, want_f32): attn_backward's shape; want_dpolicy is set on the route before it is called.
    hook() -> (mid, mid_cls) and hook_bwd() -> (mid_bwd, mid_bwd_bf16): the hook between the halves and its backward, as
    block_forward_sequence and block_backward_sequence take them.
    drop_path, rows_per_group: the stochastic-depth rows (s_attn, s_mlp) and how many rows share one; only a forward that keeps something
    for a backward applies them, and a route with a hook has none (the sequence asserts it).
    side(cls_row) -> the non-differentiable outputs that follow y (a slot may be None)."""
    drop_path, rows_per_group, want_dpolicy = (None, None), 0, False

    def hook(self):
        return None, False

    def hook_bwd(self):
        return None, False

    def side(self, cls_row):
        return ()


class DenseRoute(BlockRoute):
    """A dense block on [B, n, D] tokens: plain attention or (policy [B, n]) softmax_with_policy, no hook, stochastic depth.
    taps: callables tap(route, qkv, lse, cinv) -> tensor, launched in this order right after the attention forward; their results follow
    the CLS row in side().  refuse: called first, raises where the arithmetic mode cannot run the block (a tap built for fp32 qkv), or None.
    always_f32: the fp32 form of the attention output is written on the bf16 data path in eval too."""
    always_f32 = False

    def __init__(self, B, n, heads, scale, want_cls=False, policy=None, taps=(), drop_path=(None, None), refuse=None):
        # Attention.scale = qk_scale or head_dim ** -0.5 (:188)
        self.geom = (B, n, heads, float(_DH) ** -0.5 if scale is None else float(scale))
        self.want_cls, self.policy, self.taps, self.drop_path, self.rows_per_group, self.refuse = want_cls, policy, taps, drop_path, n, refuse
        self.cinv, self.tapped = None, ()

    def begin(self, x, params):
        if self.refuse is not None:
            self.refuse()
        ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        return bf16_data_path(x, x.shape[-1], params[8].shape[0])

    def attn(self, qkv, keep, io, want_f32):
        out = attn_forward(qkv, *self.geom, self.want_cls, self.policy, io, want_f32 or self.always_f32)
        self.tapped = tuple(tap(self, qkv, out[1], out[2]) for tap in self.taps)
        if keep:
            self.cinv = out[2]
        return out

    def attn_bwd(self, qkv, ao, dao, lse, io, dqkv16, want_f32):
        return attn_backward(qkv, ao, dao, lse, *self.geom, self.policy, self.cinv, io, dqkv16, want_f32, self.want_dpolicy)

    def side(self, cls_row):
        tapped, self.tapped = self.tapped, ()
        return (cls_row, *tapped)


def route_forward(ctx, x, params, eps, route, io):
    """The forward of a Function that runs `route` on x [..., D]: block_forward_sequence over all rows, and what the backward needs kept on
    ctx when there is one to serve.  -> (y [rows', D], the route's side outputs)"""
    train = wants_grad(ctx)
    x = x.contiguous()
    s_attn, s_mlp = route.drop_path if train else (None, None)
    y, cls_row, saved, _ = block_forward_sequence(x if x.dim() == 2 else x.view(-1, x.shape[-1]), params, eps, io, train, route.attn, (train,),
                                                  s_attn, s_mlp, route.rows_per_group, *route.hook())
    if train:
        ctx.save_for_backward(x, *saved)
        ctx.route = route
    return y, route.side(cls_row)


def route_backward(ctx, gy, policy_slot):
    """The backward of route_forward.  -> one gradient per input of the Function: x and the 12 parameters in slots 0..12, the policy in
    policy_slot if the call had that many inputs and it takes one, None everywhere else"""
    x, *saved = ctx.saved_tensors
    r, need = ctx.route, ctx.needs_input_grad
    r.want_dpolicy = len(need) > policy_slot and need[policy_slot]
    grads, dpolicy = block_backward_sequence(gy, x, saved, list(need[:13]), *r.drop_path, r.rows_per_group, r.attn_bwd, *r.hook_bwd())
    grads += [None] * (len(need) - 13)
    if r.want_dpolicy:
        grads[policy_slot] = dpolicy
    return tuple(grads)


@mode_recorded
class RouteBlockFn(torch.autograd.Function):
    """One transformer block run by a route: x [..., D], the 12 block parameters, eps, the BlockRoute, the policy (the route's own, a
    tensor input only to receive its gradient; None otherwise) -> (y [total', D] of packed rows or [B, n', D], *route.side(...)).  Differentiable in x, the
    parameters and the policy; the side outputs carry no gradient.  What a stage or a merge decided is left on the route."""

    @staticmethod
    def forward(ctx, x, *rest):
        params, (eps, route, _policy) = rest[:12], rest[12:]
        y, side = route_forward(ctx, x, params, eps, route, route.begin(x, params))
        ctx.mark_non_differentiable(*(t for t in side if t is not None))
        return (y if x.dim() == 2 else y.view(x.shape[0], -1, x.shape[-1]), *side)

    @staticmethod
    def backward(ctx, gy, *_gside):
        return route_backward(ctx, gy, 15)


@mode_recorded
class BlockFn(torch.autograd.Function):
    """One pre-norm transformer block on a packed [B, n, D] token tensor; also returns the CLS row of the softmax."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b, heads, eps, want_cls, scale, *extra):
        policy = extra[0] if extra else None         # optional 18th input: keep policy [B, n] of the dynamic-keep-ratio path (or None)
        train = wants_grad(ctx)
        # optional 19th and 20th input, stochastic depth: the block's two rows [B] of the ops.drop_path_scales table (attention branch, MLP
        # branch; either may be None), non-differentiable.  Only a forward that keeps something for a backward applies them.
        s_attn, s_mlp = (extra[1], extra[2]) if (train and len(extra) >= 3) else (None, None)
        ctx.nextra = len(extra)
        B, n, D = x.shape
        x = x.contiguous()
        scale = float(_DH) ** -0.5 if scale is None else float(scale)     # Attention.scale = qk_scale or head_dim ** -0.5 (:188)
        hidden = fc1w.shape[0]
        params = (n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b)
        # bf16 arithmetic mode: LayerNorm, the attention forward and the fc1 epilogue emit the bf16 form of what the next GEMM multiplies,
        # and that GEMM reads it instead of converting an fp32 operand (no conversion passes on the forward path)
        # (a policy block too: policy attention has its bf16 kernels, d2s_attn_policy_fwd_bf16 / _bwd_bf16)
        io = bf16_data_path(x, D, hidden)
        ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        ctx.composite = policy is None and not io and ops.block_composite_ok(x, heads, hidden)
        if ctx.composite:
            # fp32 data path: the whole block is ONE C-ABI call (csrc/block.hip issues the same seven launches)
            y, cls_row, slab = ops.block_fwd(x, params, B, n, D, heads, hidden, eps, scale, want_cls, train, s_attn, s_mlp)
            ctx.hidden = hidden
            if train:
                ctx.save_for_backward(x, slab, *params)
                ctx.drop_path = (s_attn, s_mlp)
                ctx.dims = (B, n, D, heads, scale)
        else:
            y, (cls_row,) = route_forward(ctx, x, params, eps, DenseRoute(B, n, heads, scale, want_cls, policy, drop_path=(s_attn, s_mlp)), io)
            y = y.view(B, n, D)
        cls_row = cls_or_empty(cls_row, x.device)
        ctx.mark_non_differentiable(cls_row)
        return y, cls_row

    @staticmethod
    def _backward_composite(ctx, gy):
        x, slab = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        B, n, D, heads, scale = ctx.dims
        wants = [_need(ctx, i) for i in range(13)]
        dparams = [None] * 12
        for i in range(12):
            pair = i ^ 1 if i in (0, 1, 6, 7) else i          # a LayerNorm's weight and bias gradients are produced together
            if wants[1 + i] or wants[1 + pair]:
                dparams[i] = ops.grad_buffer(params[i])
        want_dx = wants[0] or dparams[0] is not None
        dx = ops.block_bwd(gy.contiguous(), x, slab, params, B, n, D, heads, ctx.hidden, scale, want_dx, dparams, *ctx.drop_path)
        grads = [dx if wants[0] else None] + [dparams[i] if wants[1 + i] else None for i in range(12)]
        return tuple(grads) + (None, None, None, None) + (None,) * ctx.nextra

    @staticmethod
    def backward(ctx, gy, _gcls):
        # the policy: input slot 17
        return BlockFn._backward_composite(ctx, gy) if ctx.composite else route_backward(ctx, gy, 17)


class PredictorRows:
    """Where the score predictor's rows are.  Dense (cu None): x [B, n, D], the rows x[:, 1:] read in place through skip_cls_map, the input
    gradient a [B, n, D] tensor whose CLS rows are zero.  Packed: x [total, D] of a ragged batch with the offsets cu [B+1]; the B CLS rows
    are computed and ignored (B extra rows instead of a strip copy), the token mean runs over each image's non-CLS rows."""

    def __init__(self, x, B, cu=None):
        self.B, self.cu, self.shape = int(B), cu, tuple(x.shape)
        if cu is None:
            self.T = x.shape[1] - 1
            self.count, self.in_map = self.B * self.T, ops.skip_cls_map(x.shape[1], x.shape[2])
        else:
            self.count, self.in_map = x.shape[0], ops.contiguous_map(*x.shape)

    def mean_concat(self, a):
        """the split / token mean / concat behind the first activation (:540-544)"""
        if self.cu is None:
            return ops.half_mean_concat(a, self.B, self.T, a.shape[1])
        return ops.half_mean_concat_varlen(a, self.cu, self.B)

    def mean_concat_backward(self, d, act, z):
        """d: the gradient of mean_concat's output -> the gradient of the first Linear's pre-activation; z: what the first activation's
        backward reads (the ReLU's output, the GELU's pre-activation).  Only the dense kernel can fold the ReLU mask in."""
        if self.cu is not None:
            return ops.act_grad(ops.half_mean_concat_varlen_bwd(d, self.cu, self.B), z, act)
        if act == "relu":
            return ops.half_mean_concat(d, self.B, self.T, d.shape[1], relu_mask_src=z)
        return ops.act_grad(ops.half_mean_concat(d, self.B, self.T, d.shape[1]), z, act)

    def input_grad_buffer(self, device):
        return (torch.zeros if self.cu is None else torch.empty)(self.shape, dtype=torch.float32, device=device)


def predictor_bf16_data_path(x, act):
    """bf16 arithmetic mode with the bf16 data path on, for the large predictor only: the small one keeps fp32 activations"""
    return act == "relu" and ops.bf16_io() and x.is_cuda and x.shape[-1] % 32 == 0


def _predictor_exact_from(nl, act):
    """the first layer of the large predictor's tail (its last two Linear layers, D/2 -> D/4 -> 1: 0.3 % of its FLOPs), which like the
    softmax and the selection behind it always runs in exact fp32 - also in the bf16 arithmetic mode (kept-id stability).  The
    small predictor has no such tail."""
    return nl - 2 if act == "relu" else nl


def predictor_forward_sequence(x, rows, params, act, io, train):
    """THE launch sequence of the LayerNorm score predictor (PredictorLG :409-426 small, :491-531 large, forward :536-551): LN -> Linear ->
    activation on every row, split / token mean / concat, then a stack of LN -> Linear -> activation whose last Linear is 1 wide and bare.
    Callers: PredictorFn (dense rows) and functional_ragged's ragged_predictor_forward and RaggedPredictorFn (packed rows).
    rows: a PredictorRows; params: (ln_w, ln_b, fc_w, fc_b) of the input layer, then of each layer behind the concat.
    act: "relu" - the large predictor, five layers behind the concat - or "gelu" - the small one, three layers, exact-erf GELU.
    io: bf16 data path (predictor_bf16_data_path) - the LayerNorm in front of a bf16-mode Linear writes only the bf16 form that GEMM
    multiplies, as in BlockFn; the weight gradients read it too.  The exact-fp32 tail keeps fp32 activations.
    train: keep the LayerNorm statistics, every layer input and what the activations' backward reads; otherwise nothing is kept.
    -> (scores [rows.count, 1], what predictor_backward_sequence unpacks, 5 entries per layer (None unless train))"""
    M, eps = rows.count, 1e-5
    nl = len(params) // 4
    act_epi = ops.EPI_BIAS_RELU if act == "relu" else ops.EPI_BIAS_GELU
    saved = []
    cur = x
    for j in range(nl):
        lw, lb, fw, fb = params[4 * j: 4 * j + 4]
        width = fw.shape[1]
        cmap = rows.in_map if j == 0 else ops.contiguous_map(M, width)
        last = j == nl - 1
        exact = j >= _predictor_exact_from(nl, act)
        z = None
        if io and not exact:
            _, mean, rstd, ln = ops.layernorm_fwd_bf16(cur, cmap, lw, lb, M, width, eps, stats=train, want_f32=False)
            nxt = ops.linear_fwd(None, fw, fb, epi=act_epi, a16=ln)
        else:
            ln, mean, rstd = ops.layernorm_fwd(cur, cmap, lw, lb, M, width, eps, stats=train)
            if train and act == "gelu" and not last:      # the GELU's backward reads the pre-activation: written only when training
                z = torch.empty((M, fw.shape[0]), dtype=torch.float32, device=x.device)
            with ops.gemm_mode(ops.GEMM_EXACT if exact else ops.get_gemm_mode()):
                nxt = ops.linear_fwd(ln, fw, fb, epi=ops.EPI_BIAS if last else act_epi, aux_out=z)
        if train:
            # a ReLU's backward reads its output: the next layer keeps that as its input, only the one in front of the concat is kept here
            saved += [cur, ln, mean, rstd, nxt if (act == "relu" and j == 0) else z]
        cur = rows.mean_concat(nxt) if j == 0 else nxt
    return cur, (saved if train else None)


def predictor_backward_sequence(gscores, rows, saved, params, act, wants):
    """The backward of predictor_forward_sequence.  gscores: the gradient of the scores; saved: what the forward sequence returned for
    this; wants: which of (x, *params) take a gradient.  -> the gradients in wants' order, None where not wanted"""
    M = rows.count
    nl = len(params) // 4
    dev = gscores.device
    relu = act == "relu"
    grads = [None] * (1 + len(params))
    io = ops.bf16_io() and gscores.is_cuda
    d = gscores.contiguous().view(M, 1)
    d16 = None                      # bf16 copy of d, written by the LayerNorm backward that produced it, when the next GEMMs run in bf16
    for j in reversed(range(nl)):
        cur, ln, mean, rstd, _ = saved[5 * j: 5 * j + 5]
        lw, lb, fw, fb = params[4 * j: 4 * j + 4]
        p = 1 + 4 * j                   # lw's slot in wants / grads
        width = fw.shape[1]
        lnx, ln16 = xarg(ln)            # bf16 on the bf16 data path
        # d is the gradient w.r.t. the pre-activation of layer j's Linear (the activation's backward was applied upstream)
        with ops.gemm_mode(ops.GEMM_EXACT if j >= _predictor_exact_from(nl, act) else ops.get_gemm_mode()):      # as this layer's forward
            grads[p + 2], grads[p + 3] = ops.linear_param_grads(d, lnx, fw, fb, wants[p + 2], wants[p + 3], x16=ln16)
            if j == 0 and not (wants[0] or wants[p] or wants[p + 1]):
                break
            dln = ops.linear_dgrad(d, fw, a16=d16 if ln16 is not None else None)
        # the layer below multiplies d in bf16 if it is a bf16-mode layer: its saved input is bf16 then (no bf16 form crosses the concat)
        d16 = ops.bf16_buffer(M, width, dev) if (io and j >= 2 and saved[5 * (j - 1) + 1].dtype == torch.bfloat16) else None
        dx = rows.input_grad_buffer(dev) if j == 0 else torch.empty((M, width), dtype=torch.float32, device=dev)
        # cur is the activation of layer j - 1 for j >= 2: the ReLU's backward folds into the LayerNorm backward, the GELU's is one
        # elementwise kernel on the saved pre-activation; for j == 1 cur is the split / mean / concat output
        d, grads[p], grads[p + 1] = layernorm_backward(cur, rows.in_map if j == 0 else ops.contiguous_map(M, width), dln, lw, lb, mean, rstd,
                                                       dx, M, width, wants[p], wants[p + 1], relu_mask=(relu and j >= 2), dx16=d16)
        if j >= 2 and not relu:
            d = ops.act_grad(d, saved[5 * (j - 1) + 4], "gelu")
        elif j == 1:
            d = rows.mean_concat_backward(d, act, saved[4])
        elif j == 0 and wants[0]:
            grads[0] = d
    return grads


@mode_recorded
class PredictorFn(torch.autograd.Function):
    """LayerNorm predictor (PredictorLG, topk_selection=True) on x[:, 1:] of a [B, n, D] tensor: the large one (ReLU), or - a trailing
    "gelu" behind the parameters - the small one (--small-predictor, exact-erf GELU).
    Returns (scores [B, n-1] differentiable, keep_probs [B, n-1] non-differentiable)."""

    @staticmethod
    def forward(ctx, x, *params):
        # params: in_ln_w, in_ln_b, in_fc_w, in_fc_b, then 5 (small: 3) x (ln_w, ln_b, fc_w, fc_b)
        ctx.act = params[-1] if isinstance(params[-1], str) else "relu"
        params = params[:len(params) // 4 * 4]
        B, n, D = x.shape
        x = x.contiguous()
        train = wants_grad(ctx)
        scores, saved = predictor_forward_sequence(x, PredictorRows(x, B), params, ctx.act, predictor_bf16_data_path(x, ctx.act), train)
        scores = scores.view(B, n - 1)
        probs = ops.softmax_rows(scores)
        if train:
            ctx.save_for_backward(*saved, *params)          # saved[0] is x
            ctx.B = B
        ctx.mark_non_differentiable(probs)
        return scores, probs

    @staticmethod
    def backward(ctx, gscores, _gprobs):
        np_ = (len(ctx.needs_input_grad) - 1) // 4 * 4
        saved, params = ctx.saved_tensors[:-np_], ctx.saved_tensors[-np_:]
        grads = predictor_backward_sequence(gscores, PredictorRows(saved[0], ctx.B), saved, params, ctx.act, ctx.needs_input_grad)
        return tuple(grads) + (None,) * (len(ctx.needs_input_grad) - len(grads))


class GatherFn(torch.autograd.Function):
    """Pack the surviving tokens: out[b] = x[b, [0, kept+1]]; backward scatters (zeros for dropped tokens)."""

    @staticmethod
    def forward(ctx, x, kept):
        ctx.save_for_backward(kept)
        ctx.n = x.shape[1]
        return ops.gather_pack(x.contiguous(), kept)

    @staticmethod
    def backward(ctx, g):
        (kept,) = ctx.saved_tensors
        return ops.scatter_unpack(g.contiguous(), kept, ctx.n), None


class GatherFuseFn(torch.autograd.Function):
    """GatherFn plus one package token per stage (fuse_dropped): x [B,n,D] whose last t rows are the package
    tokens of earlier stages, p [B,n-1-t] the stage's keep probabilities (KeepProbsFn), kept / dropped the ids of select_topk ->
    [B,k+t+2,D] = [CLS | kept | the t package rows | sum_{j in dropped} (p_j / S) x_j].  Returns (dx, dp, None, None, None): the task
    loss reaches the predictor through dp.  Like GatherFn it works on the fp32 residual stream in every GEMM arithmetic mode."""

    @staticmethod
    def forward(ctx, x, p, kept, dropped, t):
        x, p = x.contiguous(), p.contiguous()
        y, S = ops.gather_fuse_fwd(x, p, kept, dropped, t)
        ctx.save_for_backward(x, p, S, y, kept, dropped)
        ctx.t = int(t)
        return y

    @staticmethod
    def backward(ctx, g):
        x, p, S, y, kept, dropped = ctx.saved_tensors
        dx, dp = ops.gather_fuse_bwd(g.contiguous(), x, p, S, y, kept, dropped, ctx.t)
        return dx if _need(ctx, 0) else None, dp if _need(ctx, 1) else None, None, None, None


class GatherSqueezeFn(torch.autograd.Function):
    """GatherFn with every dropped token squeezed into the kept token it resembles most (squeeze_dropped):
    x [B,n,D] = [CLS | T scored], kept / dropped the selector's ids -> (y [B,k+1,D], dst, sim).  The plan (dst, sim) is matched here unless
    `plan` replays one; it is a constant of the backward (no gradient through the cosine) and comes back detached, for inspection.  Saves
    kept, dropped, dst, sim, Z - not x: the merge is linear in x for a fixed plan.  No host synchronisation, no read-back.  Like GatherFn it
    works on the fp32 residual stream in every GEMM arithmetic mode and sends no gradient to the selector.  k == 0 is GatherFn: there is
    nothing to squeeze into."""

    @staticmethod
    def forward(ctx, x, kept, dropped, plan=None):
        x = x.contiguous()
        ctx.n, ctx.k = x.shape[1], kept.shape[1]
        if ctx.k == 0:
            ctx.save_for_backward(kept)
            dst = torch.empty((x.shape[0], 0), dtype=torch.int32, device=x.device)
            y = ops.gather_pack(x, kept)
            sim = torch.empty((x.shape[0], 0), dtype=torch.float32, device=x.device)
        else:
            dst, sim = ops.squeeze_match(x, kept, dropped) if plan is None else plan
            y, Z = ops.gather_squeeze_fwd(x, kept, dropped, dst, sim)
            ctx.save_for_backward(kept, dropped, dst, sim, Z)
        ctx.mark_non_differentiable(dst, sim)
        return y, dst, sim

    @staticmethod
    def backward(ctx, g, _gdst, _gsim):
        if ctx.k == 0:
            (kept,) = ctx.saved_tensors
            return ops.scatter_unpack(g.contiguous(), kept, ctx.n), None, None, None
        kept, dropped, dst, sim, Z = ctx.saved_tensors
        return ops.gather_squeeze_bwd(g.contiguous(), kept, dropped, dst, sim, Z, ctx.n), None, None, None


@mode_recorded
class HeadFn(torch.autograd.Function):
    """Final LayerNorm + classifier head on the CLS row.  Returns (logits [B,C], features = normed tokens[:, 1:n - tail]); tail: the
    trailing package rows of a fuse_dropped student, which are normalised with the rest but are no token features."""

    @staticmethod
    def forward(ctx, x, nw, nb, hw, hb, eps, tail=0):
        B, n, D = x.shape
        M = B * n
        x = x.contiguous()
        train = wants_grad(ctx)
        xn, mean, rstd = ops.layernorm_fwd(x, ops.contiguous_map(M, D), nw, nb, M, D, eps, stats=train)
        C = hw.shape[0]
        logits = torch.empty((B, C), dtype=torch.float32, device=x.device)
        ops.gemm(ops.NT, xn, n * D, hw, D, logits, C, B, C, D, ops.EPI_BIAS, hb)   # A = CLS rows (row stride n*D)
        if train:
            ctx.save_for_backward(x, nw, hw, mean, rstd, xn, nb, hb)
            ctx.dims = (B, n, D, C)
        ctx.tail = int(tail)
        return logits, xn.view(B, n, D)[:, 1:n - int(tail)]

    @staticmethod
    def backward(ctx, glogits, gfeat):
        x, nw, hw, mean, rstd, xn, nb, hb = ctx.saved_tensors
        B, n, D, C = ctx.dims
        M = B * n
        dev = x.device
        gfull = torch.zeros((B, n, D), dtype=torch.float32, device=dev)
        nf = n - 1 - ctx.tail             # feature rows per image
        if gfeat is not None and nf > 0:
            gfeat = gfeat.contiguous()
            ops.copy_rows(gfeat, ops.contiguous_map(B * nf, D), B * nf, D, dst=gfull, dst_map=ops.skip_cls_map(n, D, ctx.tail))
        dhw = dhb = None
        if glogits is not None:
            glogits = glogits.contiguous()
            cls_g = ops.linear_dgrad(glogits, hw)
            ops.copy_rows(cls_g, ops.contiguous_map(B, D), B, D, dst=gfull, dst_map=(1, n * D, D, 0))
            cls_rows = ops.copy_rows(xn, (1, n * D, D, 0), B, D) if _need(ctx, 3) else None
            dhw, dhb = ops.linear_param_grads(glogits, cls_rows, hw, hb, _need(ctx, 3), _need(ctx, 4))
        gx, dnw, dnb = layernorm_backward(x, ops.contiguous_map(M, D), gfull.view(M, D), nw, nb, mean, rstd,
                                          torch.empty((M, D), dtype=torch.float32, device=dev), M, D, _need(ctx, 1), _need(ctx, 2))
        return gx.view(B, n, D) if _need(ctx, 0) else None, dnw, dnb, dhw, dhb, None, None


def as_policy(policy, B, n):
    """[B,n,1] / [B,n] keep policy of the reference (:892-894) -> contiguous fp32 [B,n] (no copy when it already is)."""
    p = policy.reshape(B, n)
    if p.dtype != torch.float32:
        p = p.float()
    return p.contiguous()


def ragged_block_forward(xp, cu, B, max_n, params, heads, eps, scale, want_cls=False):
    """One transformer block on a ragged packed batch [total, D] (inference with a dynamic keep ratio, :935-949: every image keeps its
    own number of tokens): block_forward_sequence, forward only, over all packed rows at once, with attention per image through
    cu_seqlens.  Returns (y [total, D], cls_rows [H, total] or None)."""
    io = bf16_data_path(xp, xp.shape[1], params[8].shape[0])
    y, cls_rows, _, _ = block_forward_sequence(xp, params, eps, io, False, _varlen_attn_forward, (cu, B, max_n, heads, scale, want_cls))
    return y, cls_rows


def rows_map_3d(t):
    """Row map (relative to t.data_ptr()) of a [B, R, C] tensor whose last dim is dense."""
    assert t.dim() == 3 and t.stride(2) == 1
    return (t.shape[1], t.stride(0), t.stride(1), 0)


class RowLossFn(torch.autograd.Function):
    """mean-over-`denom` of a per-row loss from d2s_kl_rows: cross entropy, KL between two log-softmaxes, or KL against a
    probability target (losses.py:94-95,196,198-203,220-225).  Gradient flows to `s` only (the targets are teacher
    outputs).  `s` is [rows, C] contiguous or a [B, R, C] view with a dense last dim."""

    @staticmethod
    def forward(ctx, s, mode, t, t_ids, labels, denom, *extra):
        row_weight = extra[0] if extra else None      # optional 7th input: per-row weights [rows]
        ctx.nextra = len(extra)
        if s.dim() == 3:
            smap = rows_map_3d(s)
            rows, C = s.shape[0] * s.shape[1], s.shape[2]
        else:
            s = s.contiguous()
            rows, C = s.shape
            smap = ops.contiguous_map(rows, C)
        tmap = (1, 0, 0, 0)
        tid = None
        if t is not None:
            if t_ids is not None:       # teacher tokens gathered by kept ids: row r -> t[b, ids[b, j]]
                assert t.dim() == 3 and t.stride(2) == 1
                tmap = (t_ids.shape[1], t.stride(0), t.stride(1), 0)
                tid = t_ids.contiguous().view(-1)
            elif t.dim() == 3:
                tmap = rows_map_3d(t)
            else:
                t = t.contiguous()
                tmap = ops.contiguous_map(rows, C)
        loss_row, grad = ops.kl_rows(s, smap, rows, C, mode, t=t, t_map=tmap, t_ids=tid, labels=labels, want_grad=True,
                                     row_weight=row_weight)
        ctx.save_for_backward(grad)
        ctx.meta = (tuple(s.shape), float(denom))
        return ops.sum_scalar(loss_row, 1.0 / float(denom))

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        shape, denom = ctx.meta
        gs = ops.scale_by_scalar(grad, g.contiguous(), 1.0 / denom)
        return (gs.view(shape), None, None, None, None, None) + (None,) * ctx.nextra


class AddClsPosFn(torch.autograd.Function):
    """tokens [B,T,D] -> [B,T+1,D]: prepend the CLS token and add the position table (t2t_vit.py:160-162)."""

    @staticmethod
    def forward(ctx, tok, cls_token, pos_embed):
        B, T, D = tok.shape
        out = torch.empty((B, T + 1, D), dtype=torch.float32, device=tok.device)
        lib_call = ops.lib.call
        lib_call("d2s_assemble_tokens", ops.lib.ptr(tok.contiguous()), ops.lib.ptr(cls_token), ops.lib.ptr(pos_embed), ops.lib.ptr(out),
                 B, T, D)
        ctx.save_for_backward(cls_token, pos_embed)
        ctx.dims = (B, T, D)
        return out

    @staticmethod
    def backward(ctx, g):
        cls_token, pos_embed = ctx.saved_tensors
        B, T, D = ctx.dims
        g = g.contiguous()
        dtok = ops.copy_rows(g, ops.skip_cls_map(T + 1, D), B * T, D).view(B, T, D) if ctx.needs_input_grad[0] else None
        dcls = ops.batch_sum(g, ops.grad_buffer(cls_token), B, D, (T + 1) * D) if ctx.needs_input_grad[1] else None
        dpos = ops.batch_sum(g, ops.grad_buffer(pos_embed), B, (T + 1) * D, (T + 1) * D) if ctx.needs_input_grad[2] else None
        return dtok, dcls, dpos


class PolicySoftmaxFn(torch.autograd.Function):
    """Attention.softmax_with_policy (dynamic_vit.py:195-214): attn [B,H,N,N], policy [B,N,1] or [B,N] -> probabilities."""

    @staticmethod
    def forward(ctx, attn, policy, eps):
        B, H, N, _ = attn.shape
        attn = attn.contiguous()
        pol = policy.reshape(B, N).contiguous().float()
        out = torch.empty_like(attn)
        ops.lib.call("d2s_softmax_policy_fwd", ops.lib.ptr(attn), ops.lib.ptr(pol), ops.lib.ptr(out), B, H, N, float(eps))
        ctx.save_for_backward(attn, pol)
        ctx.eps = float(eps)
        return out

    @staticmethod
    def backward(ctx, g):
        attn, pol = ctx.saved_tensors
        B, H, N, _ = attn.shape
        ga = torch.empty_like(attn)
        ops.lib.call("d2s_softmax_policy_bwd", ops.lib.ptr(attn), ops.lib.ptr(pol), ops.lib.ptr(g.contiguous()), ops.lib.ptr(ga), B, H, N,
                     ctx.eps)
        return ga, None, None


def select_topk(keep_probs, k):
    """Hard top-k of the keep probabilities (dynamic_vit.py:858-862): (kept, dropped) int64, each ascending."""
    return ops.select_topk(keep_probs.detach().contiguous(), k)


@mode_recorded
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) for the stand-alone Mlp / Attention modules (act: None | "gelu" | "relu")."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x = x.contiguous()
        z = None
        if act == "gelu":
            z = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
            y = ops.linear_fwd(x, w, b, epi=ops.EPI_BIAS_GELU, aux_out=z)
        elif act == "relu":
            y = ops.linear_fwd(x, w, b, epi=ops.EPI_BIAS_RELU)
            z = y
        else:
            y = ops.linear_fwd(x, w, b)
        ctx.act = act
        ctx.save_for_backward(x, w, z if z is not None else x)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, z = ctx.saved_tensors
        g = g.contiguous()
        if ctx.act == "gelu":     # dz = g * gelu'(z): identity-weight GEMMs are wasteful, so use the elementwise route
            g = ops.act_grad(g, z, "gelu")
        elif ctx.act == "relu":
            g = ops.act_grad(g, z, "relu")
        dx = ops.linear_dgrad(g, w) if ctx.needs_input_grad[0] else None
        db = torch.empty((w.shape[0],), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = ops.linear_wgrad(g, x, torch.empty_like(w), db=db)
        elif db is not None:
            ops.colsum(g, db)
        return dx, dw, db, None


@mode_recorded
class AttnCoreFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(dh)) v on the raw qkv Linear output [B*n, 3*H*64] (+ CLS softmax row); with a 7th input `policy` [B, n]
    the softmax is Attention.softmax_with_policy (:195-214), fused."""

    @staticmethod
    def forward(ctx, qkv, B, n, H, scale, want_cls, *extra):
        qkv = qkv.contiguous()
        policy = extra[0] if extra else None
        ctx.nextra = len(extra)
        # a policy takes the arithmetic of BlockFn's policy block in the bf16 mode (fp32 tensors in and out); plain attention stays fp32
        ctx.bf16 = policy is not None and ops.bf16_io() and qkv.is_cuda
        out, lse, cinv, cls_row, _ = attn_forward(qkv, B, n, H, scale, want_cls, policy, ctx.bf16, want_bf16=False)
        ctx.save_for_backward(qkv, out, lse, *(() if policy is None else (cinv, policy)))
        ctx.dims = (B, n, H, scale)
        cls_row = cls_or_empty(cls_row, qkv.device)
        ctx.mark_non_differentiable(cls_row)
        return out, cls_row

    @staticmethod
    def backward(ctx, g, _gc):
        B, n, H, scale = ctx.dims
        qkv, out, lse, *rest = ctx.saved_tensors
        cinv, policy = rest or (None, None)
        dqkv, dpol = attn_backward(qkv, out, g.contiguous(), lse, B, n, H, scale, policy, cinv, ctx.bf16,
                                   want_dpolicy=policy is not None and ctx.needs_input_grad[6])
        return (dqkv, None, None, None, None, None) + ((dpol,) + (None,) * (ctx.nextra - 1) if ctx.nextra else ())


class DropPathFn(torch.autograd.Function):
    """x [B, ...] * s[b] with s the drawn 0 / (1 / keep) vector (deit.py:69-77 with the draw as an input); the backward is the same scaling."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.save_for_backward(s)
        return ops.drop_path_fwd(x.contiguous(), s)

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return ops.drop_path_fwd(g.contiguous(), s), None


class PerturbedTopKFn(torch.autograd.Function):
    """vit_models/peturbed_topk.py:16-80 with the noise tensor as an explicit input."""

    @staticmethod
    def forward(ctx, x, noise, k, sigma):
        x, noise = x.contiguous(), noise.contiguous()
        ind = ops.perturbed_topk_fwd(x, noise, k, sigma)
        ctx.save_for_backward(x, noise)
        ctx.meta = (k, float(sigma))
        return ind

    @staticmethod
    def backward(ctx, g):
        x, noise = ctx.saved_tensors
        k, sigma = ctx.meta
        return ops.perturbed_topk_bwd(x, noise, g.contiguous(), k, sigma), None, None, None


@mode_recorded
class SoftGatherFn(torch.autograd.Function):
    """The soft token gather of the perturbed top-k training mode (dynamic_vit.py:896-900, stated there in comments):
    y[:, 0] = x[:, 0], y[:, 1:] = ind @ x[:, 1:] with ind [B, k, N] the PerturbedTopKFn indicators.  Returns (dx, dind).
    Selection stays fp32 in every GEMM arithmetic mode: the three products always run on the exact-fp32 MFMA and the output is the
    fp32 residual stream without a bf16 shadow (the mode is recorded like the neighbours', nothing here depends on it)."""

    @staticmethod
    def forward(ctx, x, ind):
        x, ind = x.contiguous(), ind.contiguous()
        ctx.save_for_backward(x, ind)
        return ops.soft_gather_fwd(x, ind)

    @staticmethod
    def backward(ctx, g):
        x, ind = ctx.saved_tensors
        g = g.contiguous()
        dx = ops.soft_gather_bwd_x(g, ind, x.shape[1]) if ctx.needs_input_grad[0] else None
        dind = ops.soft_gather_bwd_ind(g, x) if ctx.needs_input_grad[1] else None
        return dx, dind


class KeepProbsFn(torch.autograd.Function):
    """keep_probs = softmax(scores) (dynamic_vit.py:551) as a differentiable value.  The predictor Functions return their probabilities
    marked non-differentiable (the hard selection needs no gradient); the perturbed top-k mode repeats the same launch on the same
    scores - the same bits - and this backward carries d2s_perturbed_topk_bwd's gradient into the predictor's scores."""

    @staticmethod
    def forward(ctx, scores):
        probs = ops.softmax_rows(scores.contiguous())
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, g):
        (probs,) = ctx.saved_tensors
        return ops.softmax_rows_bwd(probs, g.contiguous())
