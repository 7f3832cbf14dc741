"""Learned Token Pruning (LTP, Kim et al. 2022; DESIGN.md section 27 - the build's own definition, PARITY UNPINNED): a token's importance
is the attention it receives in a block (ops.ltp_score, from that block's qkv and the log-sum-exp its attention wrote), and every pruning
block owns one learnable threshold.

Hard phase (eval always, training with ltp_phase == "hard"): the ragged packed batch of functional_ats.  A stage block is a ragged block
with a hook between its halves (_RaggedLTP): its attention always keeps the log-sum-exp, in eval as well, because the score needs it; the
hook compares the score with the threshold on the device (ops.ltp_select), reads the new offsets once on the host and re-packs the residual
stream.  The selection is a constant of the backward, as at an ATS stage: the hook's backward is functional_ats._Ragged.sample_bwd, and
the thresholds receive no gradient in this phase.

Soft phase (training with ltp_phase == "soft"): the batch stays dense and the soft mask acts where removal acts - on the token as a KEY
of every later block, through policy attention (LTPSoftBlockFn: block_forward_sequence with attn_forward(..., policy), the score launched
next to it as a non-differentiable side output; the backward asks attn_backward for dpolicy).  LTPSoftMaskFn is the mask of one stage,
M = sigmoid((score - theta_k) / tau), m <- m * M; the score carries no gradient, the threshold learns through M.

The bf16 arithmetic mode is refused (BF16_REFUSAL) unless asked for: _RaggedLTP(..., bf16=True) and soft_block(..., bf16=True) put a stage
block and a soft block on the bf16 data path - the ragged and the policy attention and their backwards on the bf16 matrix cores, the hook's
backward handing on both forms of the gradient (functional_ats._Ragged.sample_bwd_bf16) - and the score is then rebuilt from the bf16 qkv
and the log-sum-exp those kernels wrote (ops.ltp_score dispatches on qkv's dtype; csrc/ltp_bf16.hip).  The soft mask stays fp32."""
import torch

from . import functional as DF
from . import functional_ats as AF
from . import ops
from .lib import D2SError

BF16_REFUSAL = ("LTP runs in the fp32 arithmetic modes (exact, split): the score is recomputed from the fp32 attention's log-sum-exp and "
                "training through a ragged or a policy block with a learnt policy is built on the fp32 data path")


def refuse_bf16():
    if ops.get_gemm_mode() == ops.GEMM_BF16:
        raise D2SError(BF16_REFUSAL)


# ---- hard phase ----
class _RaggedLTP(AF._Ragged):
    """A stage block of the hard phase on the packed batch.  theta: a 1-element view of the threshold parameter (device; never read on the
    host); T: the number of patches of an image.  plan: (keep, counts) of an earlier forward on the same batch, replayed instead of
    deciding.  After the forward: cu_new, row_src_new, plan, rows (the new row count of every image, CLS included), max_n_out, and -
    unless replaying - score [total] and dense [B, T], the stage's kept patches in original coordinates."""

    def __init__(self, cu, B, max_n, heads, scale, row_src, theta, T, plan=None, bf16=False):
        # K: a stage without a token limit.  bf16: the stage on the bf16 data path in the bf16 arithmetic mode (stage_bf16: the hook's
        # backward hands on both forms of the gradient)
        super().__init__(cu, B, max_n, heads, scale, row_src, K=int(T), N=int(T), plan=plan, **(dict(bf16=True, stage_bf16=True) if bf16 else {}))
        self.theta, self.T, self.rows = theta, int(T), None

    def attn_train(self, qkv, io, want_f32):
        """The LSE form in training and in eval: the score is the column mean of the probabilities this very log-sum-exp normalises"""
        total = qkv.shape[0]
        if self.bf16 and io:
            # the bf16 kernels' log-sum-exp, of the bf16-rounded operands: the score is rebuilt from those (ops.ltp_score on the bf16 qkv)
            out, lse, _, out16 = ops.attn_varlen_fwd_lse_bf16io(qkv, self.cu, self.B, total, self.max_n, self.heads, self.scale, want_f32=want_f32)
            if self.plan is None:
                self.score = ops.ltp_score(qkv, lse, self.B, self.max_n, self.heads, self.scale, cu=self.cu, total=total)
            return out, lse, None, None, out16
        out, lse, _ = ops.attn_varlen_fwd_lse(qkv, self.cu, self.B, total, self.max_n, self.heads, self.scale)
        if self.plan is None:
            self.score = ops.ltp_score(qkv, lse, self.B, self.max_n, self.heads, self.scale, cu=self.cu, total=total)
        return out, lse, None, None, None

    def sample(self, qkv, x1, cls_row):
        if self.plan is None:
            keep, counts, self.dense = ops.ltp_select(self.score, self.cu, self.theta, self.B, row_src=self.row_src, T=self.T)
            self.plan = (keep, counts)
        keep, counts = self.plan
        self.cu_new = ops.ragged_offsets(counts, extra=1)
        off = self.cu_new.tolist()        # the one device sync of a stage: the packed row counts size every later launch
        self.rows = [b - a for a, b in zip(off, off[1:])]
        self.max_n_out = max(self.rows)
        self.total_in = x1.shape[0]
        x1, self.row_src_new = ops.ragged_repack(x1, keep, self.cu, self.cu_new, self.row_src, off[-1], self.B)
        return x1


@DF.mode_recorded
class LTPStageBlockFn(torch.autograd.Function):
    """A stage block of the hard phase: xp [total, D], the 12 block parameters, eps, the block's _RaggedLTP -> y [total', D].
    functional_ats.RaggedBlockFn with the attention of the LSE form whether or not a backward follows."""

    @staticmethod
    def forward(ctx, xp, *rest):
        params, (eps, r) = rest[:12], rest[12:]
        if r.bf16:
            if ops.get_gemm_mode() != ops.GEMM_BF16:
                raise D2SError(AF._BF16_MODE_REFUSAL)
        else:
            refuse_bf16()
        train = DF.wants_grad(ctx)
        xp = xp.contiguous()
        # bf16=True: the bf16 data path, as functional_ats.RaggedBlockFn runs a block with a stage there
        io = r.bf16 and DF.bf16_data_path(xp, xp.shape[1], params[8].shape[0])
        if r.bf16:
            if not io:
                raise D2SError("a ragged block with bf16=True needs the bf16 data path: widths that are multiples of 32, D2S_BF16_IO not 0")
            ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        y, _, saved, _ = DF.block_forward_sequence(xp, params, eps, io, train, r.attn_train, (), mid=r.sample, mid_cls=True)
        if train:
            ctx.save_for_backward(xp, *saved)
            ctx.ragged = r
        return y

    @staticmethod
    def backward(ctx, gy):
        xp, *saved = ctx.saved_tensors
        r = ctx.ragged
        grads, _ = DF.block_backward_sequence(gy, xp, saved, list(ctx.needs_input_grad[:13]), None, None, 0, r.attn_bwd,
                                              r.sample_bwd_bf16 if r.bf16 else r.sample_bwd, mid_bwd_bf16=r.bf16)
        return tuple(grads) + (None, None)


def stage_block(xp, params, eps, r):
    """LTPStageBlockFn on the block described by r (a _RaggedLTP) -> y; afterwards r holds what the stage decided"""
    return DF.run(LTPStageBlockFn, xp, *params, eps, r)


# ---- soft phase ----
@DF.mode_recorded
class LTPSoftBlockFn(torch.autograd.Function):
    """One dense block of the soft phase: x [B, n, D], the 12 block parameters, heads, eps, scale, policy ([B, n] fp32 or None: no stage
    passed yet, the plain softmax), want_score[, bf16] -> (y [B, n, D], score [B, n] or an empty tensor).  Differentiable in x, the parameters
    and the policy; the score is a side output without a gradient."""

    @staticmethod
    def forward(ctx, x, *rest):
        params, (heads, eps, scale, policy, want_score) = rest[:12], rest[12:17]
        bf16 = len(rest) > 17 and bool(rest[17])          # optional trailing input: the block may run in the bf16 arithmetic mode
        if not bf16:
            refuse_bf16()
        train = DF.wants_grad(ctx)
        B, n, D = x.shape
        x = x.contiguous()
        scale = float(scale)
        side = {}
        # bf16 and the bf16 mode on: the bf16 data path, policy attention on the bf16 matrix cores (d2s_attn_policy_fwd_bf16 / _bwd_bf16);
        # under an fp32 mode the keyword changes nothing
        io = bf16 and DF.bf16_data_path(x, D, params[8].shape[0])
        if bf16 and ops.get_gemm_mode() == ops.GEMM_BF16:
            if not io:      # the fp32 score kernel would meet a log-sum-exp of bf16-rounded operands
                raise D2SError("an LTP soft block with bf16=True needs the bf16 data path: widths that are multiples of 32, D2S_BF16_IO not 0")
            ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        ctx.nbf16 = len(rest) - 17

        def attn(qkv, io, want_f32):
            out = DF.attn_forward(qkv, B, n, heads, scale, False, policy, io)
            if want_score:
                side["score"] = ops.ltp_score(qkv, out[1], B, n, heads, scale, policy=policy, cinv=out[2]).view(B, n)
            return out

        y, _, saved, cinv = DF.block_forward_sequence(x.view(B * n, D), params, eps, io, train, attn, ())
        if train:
            ctx.save_for_backward(x, *saved)
            ctx.policy = (policy, cinv)
            ctx.dims = (B, n, heads, scale)
        score = side.get("score")
        if score is None:
            score = torch.empty(0, device=x.device)
        ctx.mark_non_differentiable(score)
        return y.view(B, n, D), score

    @staticmethod
    def backward(ctx, gy, _gscore):
        x, *saved = ctx.saved_tensors
        B, n, heads, scale = ctx.dims
        policy, cinv = ctx.policy
        want_dpolicy = policy is not None and ctx.needs_input_grad[16]
        # input slots: x 0, the 12 parameters 1..12, heads eps scale 13..15, policy 16, want_score 17
        grads, dpolicy = DF.block_backward_sequence(
            gy, x, saved, list(ctx.needs_input_grad[:13]), None, None, 0,
            lambda qkv, ao, dao, lse, io, dqkvh, want_f32: DF.attn_backward(qkv, ao, dao, lse, B, n, heads, scale, policy, cinv, io, dqkvh,
                                                                            want_f32, want_dpolicy))
        return tuple(grads) + (None, None, None, dpolicy, None) + (None,) * ctx.nbf16


def soft_block(x, params, heads, eps, scale, policy, want_score, bf16=False):
    """-> (y, score [B, n] or None).  bf16: the block follows the bf16 arithmetic mode onto the bf16 data path instead of refusing it"""
    y, score = DF.run(LTPSoftBlockFn, x, *params, heads, eps, scale, policy, bool(want_score), *((True,) if bf16 else ()))
    return y, (score if want_score else None)


class LTPSoftMaskFn(torch.autograd.Function):
    """The soft mask of stage k: score [B, N] (no gradient), m_in [B, N] or None (before the first stage: ones), the threshold parameter
    [S], k, tau -> (m_out = m_in * M [B, N], msum [B] = each image's sum of M over its patches, M [B, N] without a gradient).  The backward
    writes gm_in = g_out * M and a gradient for the whole parameter that is zero but at k, where one fixed-order reduction puts dtheta_k."""

    @staticmethod
    def forward(ctx, score, m_in, theta, k, tau):
        M, m_out, msum = ops.ltp_soft_mask_fwd(score.contiguous(), m_in, theta.detach()[k:k + 1], tau)
        ctx.save_for_backward(M, m_in)
        ctx.k, ctx.tau, ctx.S = int(k), float(tau), theta.numel()
        ctx.mark_non_differentiable(M)
        return m_out, msum, M

    @staticmethod
    def backward(ctx, g_out, g_msum, _gM):
        M, m_in = ctx.saved_tensors
        dtheta = torch.zeros((ctx.S,), dtype=torch.float32, device=M.device)
        if g_out is None:
            g_out = torch.zeros_like(M)
        want_gm = m_in is not None and ctx.needs_input_grad[1]
        _, gm_in = ops.ltp_soft_mask_bwd(g_out.contiguous(), M, m_in, ctx.tau, dtheta[ctx.k:ctx.k + 1],
                                         greg=None if g_msum is None else g_msum.contiguous(), want_gm=want_gm)
        return None, gm_in, (dtheta if ctx.needs_input_grad[2] else None), None, None


def soft_mask(score, m_in, theta, k, tau):
    return LTPSoftMaskFn.apply(score, m_in, theta, k, tau)
