"""LTP baseline (Learned Token Pruning, Kim et al. 2022; DESIGN.md section 27 - the build's own definition, no counterpart in the
reference): the dense DeiT trunk in which the blocks at `pruning_loc` each own one learnable threshold.  A token's importance is the
attention it receives in that block - the mean, over heads and query rows, of its column of the softmax - and it leaves as soon as that
falls below the block's threshold, so every image has its own token count at every block.  No predictor and no ratio; the one new
parameter is ltp_threshold [S], and a DeiT checkpoint loads with exactly that key missing.

Two phases.  "soft" (training only, the default): the batch stays dense, M = sigmoid((score - theta) / tau) multiplies into a policy that
masks the token as a key of every later block, and the thresholds learn through M (the score itself carries no gradient - a deviation from
the paper, and this repository's rule for every selection).  "hard": the ragged packed batch, thresholds constant; eval() always runs it."""
import torch
import torch.nn as nn

from d2s import functional_ats as AF
from d2s import functional_ltp as LF
from d2s import ops
from .dynamic_vit import VisionTransformerTeacher, _GEOM, checkpoint_filter_fn

PHASES = ("soft", "hard")


class VisionTransformerLTP(VisionTransformerTeacher):
    """forward returns the logits.  pruning_loc: ascending 0-based block indices in 0 .. depth - 2; ltp_temperature: tau > 0;
    ltp_init_threshold: theta_init, the thresholds start at theta_init * (k + 1) / S; ltp_phase: "soft" or "hard" (what train() runs;
    eval() is always hard).  forward(x, plans=None): plans - per stage (keep, counts) of an earlier hard forward on the same batch, replayed
    instead of deciding.
    Afterwards: tokens_per_block - [L] ints, the rows block l ran on (soft: B * N throughout); tokens_per_block_counts - [L, B] int32
    (host), the same per image, CLS included; avg_tokens - their mean per image and block; ltp_kept - per stage a [B, T] 0/1 mask of the
    patches that went on, in original patch coordinates (soft: M >= 1/2; None when replaying); ltp_plans - per stage (keep, counts)
    (hard); ltp_scores - per stage the scores of the rows that entered it; ltp_reg - the regulariser R (0-d; differentiable in the
    soft phase, the kept fraction of the patches per stage in the hard one).
    train_bf16: every forward - soft, hard and eval() - also runs in the bf16 arithmetic mode, on the bf16 data path: the stage blocks as
    _RaggedLTP(bf16=True) with the score rebuilt on the bf16 matrix cores (ops.ltp_score on the bf16 qkv), the other ragged blocks as
    _Ragged(bf16=True), the soft blocks through the bf16 policy attention; the soft mask stays fp32.  Under an fp32 mode the keyword changes
    nothing; without it the bf16 mode is refused as before."""

    def __init__(self, *args, pruning_loc=(), ltp_temperature=1e-3, ltp_init_threshold=0.005, ltp_phase="soft", train_bf16=False, **kwargs):
        super().__init__(*args, **kwargs)
        depth = len(self.blocks)
        locs = [int(v) for v in pruning_loc]
        if not locs or any(v < 0 or v > depth - 2 for v in locs) or any(a >= b for a, b in zip(locs, locs[1:])):
            raise ValueError(f"pruning_loc: at least one strictly ascending block index in [0, {depth - 2}], got {pruning_loc!r}")
        if not float(ltp_temperature) > 0.0:
            raise ValueError(f"ltp_temperature: a value > 0, got {ltp_temperature!r}")
        if ltp_phase not in PHASES:
            raise ValueError(f"ltp_phase: one of {PHASES}, got {ltp_phase!r}")
        if float(getattr(self, "drop_path_rate", 0.0)) > 0.0:
            raise ValueError("drop_path_rate > 0: stochastic depth is not built for a ragged block or a block with a learnt policy")
        self.pruning_loc = locs
        self.ltp_temperature, self.ltp_init_threshold = float(ltp_temperature), float(ltp_init_threshold)
        self.train_bf16 = bool(train_bf16)
        S = len(locs)
        self.ltp_threshold = nn.Parameter(torch.tensor([self.ltp_init_threshold * (k + 1) / S for k in range(S)], dtype=torch.float32))
        self.set_phase(ltp_phase)
        self.grad_ready_hook = None          # set by a data-parallel TrainStep: called with i when block i's input gradient exists
        self._reset_records()

    def set_phase(self, phase):
        """hard: the thresholds are constants (requires_grad off); soft: they learn"""
        if phase not in PHASES:
            raise ValueError(f"ltp_phase: one of {PHASES}, got {phase!r}")
        self.ltp_phase = phase
        self.ltp_threshold.requires_grad_(phase == "soft")

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """A DeiT / teacher checkpoint loads with exactly ltp_threshold allowed to be missing (it keeps its initial value)"""
        result = super().load_state_dict(state_dict, strict=False, **kwargs)
        missing = [k for k in result.missing_keys if k != "ltp_threshold"]
        if strict and (missing or result.unexpected_keys):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing keys {missing}, unexpected keys "
                               f"{list(result.unexpected_keys)} (only ltp_threshold may be missing)")
        return result

    def _reset_records(self):
        self.tokens_per_block, self.tokens_per_block_counts, self.avg_tokens = [], None, None
        self.ltp_kept, self.ltp_plans, self.ltp_scores, self.ltp_reg = [], [], [], None

    def forward(self, x, plans=None):
        self._reset_records()
        if not self.train_bf16:
            LF.refuse_bf16()
        if plans is not None and len(plans) != len(self.pruning_loc):
            raise ValueError(f"plans: one (keep, counts) per stage, {len(self.pruning_loc)} of them, got {len(plans)}")
        if self.training and self.ltp_phase == "soft":
            if plans is not None:
                raise ValueError("plans replay the decisions of the hard phase; the soft phase decides nothing")
            return self._forward_soft(x)
        if self.training and torch.is_grad_enabled():
            return self._forward_hard(x, plans, True)
        with torch.no_grad():               # eval keeps nothing for a backward
            return self._forward_hard(x, plans, False)

    def _forward_hard(self, x, plans, train):
        x = self._embed(x)
        B, n, D = x.shape
        T = n - 1
        x = x.contiguous().view(B * n, D)
        cu = ops.ragged_offsets(torch.full((B,), T, dtype=torch.int32, device=x.device), extra=1)      # arange(B + 1) * N
        row_src = torch.arange(n, dtype=torch.int32, device=x.device).repeat(B)
        rows, per_block, stage = [n] * B, [], 0
        bf16 = dict(bf16=True) if (self.train_bf16 and ops.get_gemm_mode() == ops.GEMM_BF16) else {}
        for i, blk in enumerate(self.blocks):
            if train and self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            per_block.append(rows)
            a = blk.attn
            if stage < len(self.pruning_loc) and i == self.pruning_loc[stage]:
                r = LF._RaggedLTP(cu, B, n, a.num_heads, a.scale, row_src, self.ltp_threshold.detach()[stage:stage + 1], T,
                                  None if plans is None else plans[stage], **bf16)
                x = LF.stage_block(x, blk._params(), blk.norm1.eps, r)
                cu, row_src, n, rows = r.cu_new, r.row_src_new, r.max_n_out, r.rows
                self.ltp_plans.append(r.plan)
                self.ltp_scores.append(r.score)
                self.ltp_kept.append(r.dense)
                stage += 1
            elif train:
                x = AF.ragged_block_train(x, blk._params(), blk.norm1.eps, AF._Ragged(cu, B, n, a.num_heads, a.scale, **bf16))
            else:
                x = blk.forward_ragged(x, cu, B, n)
        self._record_counts(per_block)
        kept = [sum(c - 1 for c in per_block[l + 1]) for l in self.pruning_loc]
        self.ltp_reg = torch.tensor(sum(kept) / float(len(kept) * B * T), dtype=torch.float32, device=x.device)
        cls = AF.ClsGatherFn.apply(x, cu)
        return self._head(cls.view(B, 1, D))[0]

    def _forward_soft(self, x):
        x = self._embed(x)
        B, n, D = x.shape
        T, S = n - 1, len(self.pruning_loc)
        m, msums, stage = None, [], 0
        bf16 = dict(bf16=True) if self.train_bf16 else {}
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            here = stage < S and i == self.pruning_loc[stage]
            a = blk.attn
            x, score = LF.soft_block(x, blk._params(), a.num_heads, blk.norm1.eps, a.scale, m, here, **bf16)
            if here:
                m_new, msum, M = LF.soft_mask(score, m, self.ltp_threshold, stage, self.ltp_temperature)
                self.ltp_kept.append((M[:, 1:] >= 0.5).float())
                self.ltp_scores.append(score)
                msums.append(msum)
                m = m_new
                stage += 1
        self._record_counts([[n] * B] * len(self.blocks))
        self.ltp_reg = torch.stack(msums).sum() / float(S * B * T)
        return self._head(x)[0]

    def _record_counts(self, per_block):
        self.tokens_per_block = [sum(r) for r in per_block]
        self.tokens_per_block_counts = torch.tensor(per_block, dtype=torch.int32)
        self.avg_tokens = float(sum(self.tokens_per_block)) / float(len(per_block) * len(per_block[0]))


def _ltp(size, pruning_loc, checkpoint_path=None, **kwargs):
    model = VisionTransformerLTP(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, pruning_loc=pruning_loc, **_GEOM[size], **kwargs)
    if checkpoint_path is not None:
        sd = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        missing, unexpected = model.load_state_dict(checkpoint_filter_fn(sd, model), strict=True)
        ops.invalidate_bf16_weights()
        print('# missing keys=', missing)
        print('# unexpected keys=', unexpected)
    return model


def ltp_deit_tiny_patch16_224(pruning_loc=(3, 6, 9), checkpoint_path=None, **kwargs):
    return _ltp("tiny", pruning_loc, checkpoint_path, **kwargs)


def ltp_deit_small_patch16_224(pruning_loc=(3, 6, 9), checkpoint_path=None, **kwargs):
    return _ltp("small", pruning_loc, checkpoint_path, **kwargs)


def ltp_deit_base_patch16_224(pruning_loc=(3, 6, 9), checkpoint_path=None, **kwargs):
    return _ltp("base", pruning_loc, checkpoint_path, **kwargs)
