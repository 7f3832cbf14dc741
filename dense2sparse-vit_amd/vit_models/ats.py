"""Adaptive Token Sampling baseline (ATS, Fayyaz et al. 2022; DESIGN.md section 24 - no counterpart in the reference): an off-the-shelf
DeiT trunk in which the blocks at `ats_locs` sample, per image, the tokens that go on past their attention.  No predictor and no fixed
count: the model has the teacher's parameters and state-dict keys and loads any DeiT checkpoint, and every image keeps its own number of
tokens, so from the first stage on the batch is ragged and packed.  Off the shelf it is an inference model; train_sample=True opts into
training through the stages (d2s.functional_ats.RaggedBlockFn), as the paper's fine-tuned numbers do."""
import torch

from d2s import functional as DF
from d2s import functional_ats as AF
from d2s import ops
from .dynamic_vit import VisionTransformerTeacher, _GEOM, _load_local

ATS_TRAINING_ERROR = ("adaptive token sampling is built for inference only: a sampling stage has no backward (call model.eval(), or "
                      "construct with ats_locs=())")


class VisionTransformerATS(VisionTransformerTeacher):
    """The dense ViT with adaptive token sampling.  ats_locs: the block indices that hold a stage, strictly ascending.  ats_tokens: the
    most tokens (CLS not counted) an image keeps at a stage - one int for every stage, a list with one int per stage, or None for the
    number of patches.  forward (eval mode) returns the logits; afterwards, per stage, tokens_per_stage holds the kept counts ([B] int32 on
    the device, CLS not counted), ats_plans the (keep, counts) that plans= replays, cu_seqlens_per_stage / ragged_row_src_per_stage the
    packed batch that leaves the stage (row_src: ORIGINAL token index of every row, 0 at CLS), ats_scores the stage's scores over the
    rows that entered it and ats_masks the cumulative keep masks [B, N] (the last two None when replaying).
    train_sample: let the training-mode forward sample too - the blocks before the first stage are the dense differentiable ones, every
    block from the first stage on runs through RaggedBlockFn on the packed batch, the head reads the gathered CLS rows; the selection is
    the inference one and a constant of the backward (no gradient through score, keep or counts), the records above are filled as in eval
    mode and plans= replays.  fp32 data path unless train_bf16.  Off (the default), a model with a stage refuses to train.
    train_bf16: with train_sample, the training-mode forward also runs in the bf16 arithmetic mode - the ragged blocks on the bf16 data
    path (_Ragged(bf16=True), stage_bf16=True at a stage), the dense blocks in front as they run there anyway.  Under an fp32 mode the
    keyword changes nothing; without it the bf16 mode is refused as before."""

    def __init__(self, *args, ats_locs=(), ats_tokens=None, train_sample=False, train_bf16=False, **kwargs):
        super().__init__(*args, **kwargs)
        depth = len(self.blocks)
        locs = [int(v) for v in ats_locs]
        if any(v < 0 or v >= depth for v in locs) or any(a >= b for a, b in zip(locs, locs[1:])):
            raise ValueError(f"ats_locs: strictly ascending block indices in [0, {depth}), got {ats_locs!r}")
        N = self.patch_embed.num_patches
        if ats_tokens is None:
            toks = [N] * len(locs)
        elif isinstance(ats_tokens, int):
            toks = [int(ats_tokens)] * len(locs)
        else:
            toks = [int(v) for v in ats_tokens]
        if len(toks) != len(locs) or any(v < 1 for v in toks):
            raise ValueError(f"ats_tokens: None, one int >= 1 or a list of {len(locs)} of them (one per stage), got {ats_tokens!r}")
        self.ats_locs, self.ats_tokens = locs, toks
        self.train_sample = bool(train_sample)
        self.train_bf16 = bool(train_bf16)
        if self.train_bf16 and not self.train_sample:
            raise ValueError("train_bf16 without train_sample: it puts training through the sampling stages into the bf16 arithmetic mode")
        if self.train_sample and float(getattr(self, "drop_path_rate", 0.0)) > 0.0:
            raise ValueError("train_sample with drop_path_rate > 0: stochastic depth is not built for a ragged block")
        self.grad_ready_hook = None          # set by a data-parallel TrainStep: called with i when block i's input gradient exists
        self._reset_records()

    def _reset_records(self):
        self.tokens_per_stage, self.ats_plans, self.ats_scores, self.ats_masks = [], [], [], []
        self.cu_seqlens_per_stage, self.ragged_row_src_per_stage = [], []

    def forward(self, x, plans=None):
        """plans: per stage (keep, counts) of an earlier forward on the same batch, to replay instead of selecting."""
        self._reset_records()
        if self.training and self.ats_locs and self.train_sample:
            return self._forward_train_sample(x, plans)
        if self.training:
            if self.ats_locs:
                raise NotImplementedError(ATS_TRAINING_ERROR)
            x = self._embed(x)                  # no stage: the dense, differentiable trunk
            for blk in self.blocks:
                x = blk(x)
            return self._head(x)[0]
        if not self.ats_locs:
            return super().forward(x)[0]
        self._check_plans(plans)
        with torch.no_grad():
            x = self._embed(x)
            B, n, D = x.shape
            N = n - 1
            cu = row_src = None
            stage = 0
            for i, blk in enumerate(self.blocks):
                if stage < len(self.ats_locs) and i == self.ats_locs[stage]:
                    if cu is None:              # the first stage packs the batch: every image still has all its rows
                        x = x.contiguous().view(B * n, D)
                        cu = ops.ragged_offsets(torch.full((B,), N, dtype=torch.int32, device=x.device), extra=1)
                        row_src = torch.arange(n, dtype=torch.int32, device=x.device).repeat(B)
                    a = blk.attn
                    x, cu, row_src, n, plan, score, dense = AF.ats_block_forward(
                        x, cu, B, n, blk._params(), a.num_heads, blk.norm1.eps, a.scale, self.ats_tokens[stage], N, row_src,
                        None if plans is None else plans[stage])
                    self._record(plan, score, dense, cu, row_src)
                    stage += 1
                elif cu is None:
                    x = blk(x)
                else:
                    x = blk.forward_ragged(x, cu, B, n)
            total = x.shape[0]
            xn, _, _ = ops.layernorm_fwd(x, ops.contiguous_map(total, D), self.norm.weight, self.norm.bias, total, D, self.norm.eps, stats=False)
            return ops.linear_fwd(ops.gather_rows_i32(xn, cu, B), self.head.weight, self.head.bias)

    def _check_plans(self, plans):
        if plans is not None and len(plans) != len(self.ats_locs):
            raise ValueError(f"plans: one (keep, counts) per stage, {len(self.ats_locs)} of them, got {len(plans)}")

    def _record(self, plan, score, dense, cu, row_src):
        self.tokens_per_stage.append(plan[1])
        self.ats_plans.append(plan)
        self.ats_scores.append(score)
        self.ats_masks.append(dense)
        self.cu_seqlens_per_stage.append(cu)
        self.ragged_row_src_per_stage.append(row_src)

    def _forward_train_sample(self, x, plans):
        """The eval forward's launches with everything a backward needs kept: dense BlockFn blocks up to the first stage, the pack (a view),
        one RaggedBlockFn per block from there on, the CLS rows gathered in front of the final LayerNorm (row-wise, so the same function
        as normalising every row first) and HeadFn on them."""
        self._check_plans(plans)
        bf16 = ops.get_gemm_mode() == ops.GEMM_BF16
        if bf16 and not self.train_bf16:
            raise NotImplementedError("train_sample in the bf16 arithmetic mode: training through a sampling stage is built on the fp32 data "
                                      "path only (gemm modes exact and split)")
        x = self._embed(x)
        B, n, D = x.shape
        N = n - 1
        cu = row_src = None
        stage = 0
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            here = stage < len(self.ats_locs) and i == self.ats_locs[stage]
            if cu is None and not here:
                x = blk(x)
                continue
            if cu is None:                      # the first stage packs the batch: every image still has all its rows
                x = x.contiguous().view(B * n, D)
                cu = ops.ragged_offsets(torch.full((B,), N, dtype=torch.int32, device=x.device), extra=1)
                row_src = torch.arange(n, dtype=torch.int32, device=x.device).repeat(B)
            a = blk.attn
            if here:
                r = AF._Ragged(cu, B, n, a.num_heads, a.scale, row_src, self.ats_tokens[stage], N, None if plans is None else plans[stage],
                               **(dict(bf16=True, stage_bf16=True) if bf16 else {}))
            else:
                r = AF._Ragged(cu, B, n, a.num_heads, a.scale, **(dict(bf16=True) if bf16 else {}))
            x = AF.ragged_block_train(x, blk._params(), blk.norm1.eps, r)
            if here:
                cu, row_src, n = r.cu_new, r.row_src_new, r.max_n_out
                self._record(r.plan, r.score, r.dense, cu, row_src)
                stage += 1
        cls = AF.ClsGatherFn.apply(x, cu)
        return self._head(cls.view(B, 1, D))[0]


def _ats(size, ats_locs, ats_tokens, checkpoint_path=None, **kwargs):
    model = VisionTransformerATS(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, ats_locs=ats_locs, ats_tokens=ats_tokens,
                                 **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=True)


def ats_deit_tiny_patch16_224(ats_locs=(), ats_tokens=None, checkpoint_path=None, **kwargs):
    return _ats("tiny", ats_locs, ats_tokens, checkpoint_path, **kwargs)


def ats_deit_small_patch16_224(ats_locs=(), ats_tokens=None, checkpoint_path=None, **kwargs):
    return _ats("small", ats_locs, ats_tokens, checkpoint_path, **kwargs)


def ats_deit_base_patch16_224(ats_locs=(), ats_tokens=None, checkpoint_path=None, **kwargs):
    return _ats("base", ats_locs, ats_tokens, checkpoint_path, **kwargs)
