"""Learned Token Pruning (LTP, Kim et al. 2022; DESIGN.md section 27 - the build's own definition, PARITY UNPINNED): a token's importance
is the attention it receives in a block (ops.ltp_score, from that block's qkv and the log-sum-exp its attention wrote), and every pruning
block owns one learnable threshold.

Hard phase (eval always, training with ltp_phase == "hard"): the ragged packed batch of functional_ats.  A stage block is a ragged block
with a hook between its halves (_RaggedLTP, run like every route by functional.RouteBlockFn): its attention always keeps the
log-sum-exp, in eval as well, because the score needs it; the hook compares the score with the threshold on the device
(ops.ltp_select), reads the new offsets once on the host and re-packs the residual stream.  The selection is a constant of the backward, as at an ATS stage: the hook's backward is functional_ats._Ragged.sample_bwd, and
the thresholds receive no gradient in this phase.

Soft phase (training with ltp_phase == "soft"): the batch stays dense and the soft mask acts where removal acts - on the token as a KEY
of every later block, through policy attention (_Soft: a functional.DenseRoute with attn_forward(..., policy), the score a tap launched
next to it, a non-differentiable side output; the backward asks attn_backward for dpolicy).  LTPSoftMaskFn is the mask of one stage,
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

    def begin(self, xp, params):
        if self.bf16:
            if ops.get_gemm_mode() != ops.GEMM_BF16:
                raise D2SError(AF._BF16_MODE_REFUSAL)
        else:
            refuse_bf16()
        return self.data_path(xp, params)

    def attn(self, qkv, keep, io, want_f32):
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


def stage_block(xp, params, eps, r):
    """A stage block of the hard phase, described by r (a _RaggedLTP): xp [total, D] -> y [total', D], differentiable in xp and the
    parameters; afterwards r holds what the stage decided"""
    return DF.run(DF.RouteBlockFn, xp, *params, eps, r, None)[0]


# ---- soft phase ----
def _score(route, qkv, lse, cinv):
    """DenseRoute's tap: the attention every token receives, under the block's policy"""
    B, n = route.geom[:2]
    return ops.ltp_score(qkv, lse, *route.geom, policy=route.policy, cinv=cinv).view(B, n)


class _Soft(DF.DenseRoute):
    """One dense block of the soft phase: policy attention under the mask so far ([B, n] fp32, or None: no stage passed yet, the plain
    softmax), the score a tap.  bf16: the block follows the bf16 arithmetic mode onto the bf16 data path - policy attention on the bf16
    matrix cores (d2s_attn_policy_fwd_bf16 / _bwd_bf16) - instead of refusing it; under an fp32 mode the keyword changes nothing."""
    always_f32 = True

    def __init__(self, B, n, heads, scale, policy, want_score, bf16):
        super().__init__(B, n, heads, float(scale), False, policy, (_score,) if want_score else ())
        self.bf16 = bool(bf16)

    def begin(self, x, params):
        if not self.bf16:
            refuse_bf16()
            return False
        io = DF.bf16_data_path(x, x.shape[-1], params[8].shape[0])
        if ops.get_gemm_mode() == ops.GEMM_BF16:
            if not io:      # the fp32 score kernel would meet a log-sum-exp of bf16-rounded operands
                raise D2SError("an LTP soft block with bf16=True needs the bf16 data path: widths that are multiples of 32, D2S_BF16_IO not 0")
            ops._SHADOW.clear()          # gradient shadows never outlive the backward pass that made them
        return io


def soft_block(x, params, heads, eps, scale, policy, want_score, bf16=False):
    """x [B, n, D] -> (y [B, n, D], score [B, n] or None), differentiable in x, the parameters and the policy; the score is a side output
    without a gradient"""
    B, n, _ = x.shape
    y, _, *score = DF.run(DF.RouteBlockFn, x, *params, eps, _Soft(B, n, heads, scale, policy, want_score, bf16), policy)
    return y, (score[0] if want_score else None)


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
