"""Adaptive Token Sampling baseline (ATS, Fayyaz et al. 2022; DESIGN.md section 24 - no counterpart in the reference): an off-the-shelf
DeiT trunk in which the blocks at `ats_locs` sample, per image, the tokens that go on past their attention.  No predictor and no fixed
count: the model has the teacher's parameters and state-dict keys and loads any DeiT checkpoint, and every image keeps its own number of
tokens, so from the first stage on the batch is ragged and packed.  Inference only."""
import torch

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
    rows that entered it and ats_masks the cumulative keep masks [B, N] (the last two None when replaying)."""

    def __init__(self, *args, ats_locs=(), ats_tokens=None, **kwargs):
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
        self._reset_records()

    def _reset_records(self):
        self.tokens_per_stage, self.ats_plans, self.ats_scores, self.ats_masks = [], [], [], []
        self.cu_seqlens_per_stage, self.ragged_row_src_per_stage = [], []

    def forward(self, x, plans=None):
        """plans: per stage (keep, counts) of an earlier forward on the same batch, to replay instead of selecting."""
        self._reset_records()
        if self.training:
            if self.ats_locs:
                raise NotImplementedError(ATS_TRAINING_ERROR)
            x = self._embed(x)                  # no stage: the dense, differentiable trunk
            for blk in self.blocks:
                x = blk(x)
            return self._head(x)[0]
        if not self.ats_locs:
            return super().forward(x)[0]
        if plans is not None and len(plans) != len(self.ats_locs):
            raise ValueError(f"plans: one (keep, counts) per stage, {len(self.ats_locs)} of them, got {len(plans)}")
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
                    self.tokens_per_stage.append(plan[1])
                    self.ats_plans.append(plan)
                    self.ats_scores.append(score)
                    self.ats_masks.append(dense)
                    self.cu_seqlens_per_stage.append(cu)
                    self.ragged_row_src_per_stage.append(row_src)
                    stage += 1
                elif cu is None:
                    x = blk(x)
                else:
                    x = blk.forward_ragged(x, cu, B, n)
            total = x.shape[0]
            xn, _, _ = ops.layernorm_fwd(x, ops.contiguous_map(total, D), self.norm.weight, self.norm.bias, total, D, self.norm.eps, stats=False)
            return ops.linear_fwd(ops.gather_rows_i32(xn, cu, B), self.head.weight, self.head.bias)


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
