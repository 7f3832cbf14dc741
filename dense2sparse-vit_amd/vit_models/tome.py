"""Token Merging baseline (ToMe, Bolya et al. 2023; DESIGN.md section 22 - no counterpart in the reference): an off-the-shelf DeiT trunk
whose every block merges r tokens into their most similar partner between its attention branch and its MLP.  No predictor: the model has
the teacher's parameters and state-dict keys and loads any DeiT checkpoint.  Off the shelf it is an inference model; train_merge=True opts
into training through the merge (d2s.functional_tome.ToMeBlockFn), as the paper's fine-tuned numbers do; train_bf16=True puts that training
on the bf16 data path when the process runs in the bf16 arithmetic mode."""
import torch

from d2s import functional as DF
from d2s import functional_tome as TF
from d2s import ops
from .dynamic_vit import VisionTransformerTeacher, _GEOM, _load_local

TOME_TRAINING_ERROR = ("token merging is built for inference only: training through a merge needs the merge's backward and key weights in "
                       "both attention-backward kernels (call model.eval(), or construct with tome_r=0)")


class VisionTransformerToMe(VisionTransformerTeacher):
    """The dense ViT with token merging.  tome_r: tokens merged away per block, one int for every block or a list of `depth` ints; each
    block clips its count to (n - 1) // 2 of the n tokens it sees.  prop_attn: weight every key by the patches it stands for
    (proportional attention) once something has merged.  forward (eval mode) returns the logits; afterwards tokens_per_block[i] is the
    number of tokens (CLS included) that leave block i, and tome_plans[i] the block's (unm_idx, src_idx, dst_idx) or None.
    train_merge: let the training-mode forward merge too - every block runs through ToMeBlockFn, gradients flow through the merge (a
    size-weighted average with a constant plan) and the key-weighted attention; off (the default), a merging model refuses to train.
    bf16: run the eval forward on the bf16 data path (TF.tome_block_forward_bf16) inside ops.gemm_mode(ops.GEMM_BF16), whatever the
    ambient mode, which is restored afterwards; inference only, so it excludes train_merge.
    train_bf16 (needs train_merge): under the bf16 arithmetic mode the training-mode forward runs every block through ToMeBlockFn on the
    bf16 data path - the GEMMs, the (key-weighted) attention and both their backwards on the bf16 matrix cores, the residual stream and the
    merge in fp32 - and the eval forward takes the bf16=True route, so validation runs in the same process; under an fp32 mode it changes
    nothing."""

    def __init__(self, *args, tome_r=0, prop_attn=True, train_merge=False, bf16=False, train_bf16=False, **kwargs):
        super().__init__(*args, **kwargs)
        depth = len(self.blocks)
        rs = [int(tome_r)] * depth if isinstance(tome_r, int) else [int(v) for v in tome_r]
        if len(rs) != depth or any(v < 0 for v in rs):
            raise ValueError(f"tome_r: one non-negative int or a list of {depth} of them, got {tome_r!r}")
        self.tome_r = rs
        self.prop_attn = bool(prop_attn)
        self.train_merge = bool(train_merge)
        self.bf16 = bool(bf16)
        if self.bf16 and self.train_merge:
            raise ValueError("bf16 with train_merge: training through a merge is built in fp32 only (the bf16 merging trunk is inference only)")
        self.train_bf16 = bool(train_bf16)
        if self.train_bf16 and not self.train_merge:
            raise ValueError("train_bf16 without train_merge: it puts training through the merges on the bf16 data path (train_merge=True)")
        if self.train_merge and float(getattr(self, "drop_path_rate", 0.0)) > 0.0:
            raise ValueError("train_merge with drop_path_rate > 0: stochastic depth is not built for a merging block")
        self.grad_ready_hook = None          # set by a data-parallel TrainStep: called with i when block i's input gradient exists
        self.tokens_per_block = None
        self.tome_plans = None

    def forward(self, x, plans=None):
        """plans: per block (unm_idx, src_idx, dst_idx) or None, to replay instead of matching."""
        merging = any(v > 0 for v in self.tome_r)
        if self.training and self.train_merge:
            return self._forward_train_merge(x, plans)
        if self.training:
            if merging:
                raise NotImplementedError(TOME_TRAINING_ERROR)
            x = self._embed(x)                  # r = 0 everywhere: the dense, differentiable trunk
            for blk in self.blocks:
                x = blk(x)
            self.tokens_per_block, self.tome_plans = [x.shape[1]] * len(self.blocks), [None] * len(self.blocks)
            return self._head(x)[0]
        if self.bf16 or (self.train_bf16 and ops.get_gemm_mode() == ops.GEMM_BF16):
            with ops.gemm_mode(ops.GEMM_BF16):      # the context manager restores the ambient mode on return and on an exception
                return self._forward_eval(x, plans, TF.tome_block_forward_bf16)
        return self._forward_eval(x, plans, TF.tome_block_forward)

    def _forward_eval(self, x, plans, block_forward):
        with torch.no_grad():
            x = self._embed(x)
            B, n, D = x.shape
            x = x.view(B * n, D)
            size, counts, used = None, [], []
            for i, blk in enumerate(self.blocks):
                a = blk.attn
                x, size, plan = block_forward(x, size, blk._params(), B, n, a.num_heads, blk.norm1.eps, a.scale, self.tome_r[i],
                                              self.prop_attn, None if plans is None else plans[i])
                n = x.shape[0] // B
                counts.append(n)
                used.append(plan)
            self.tokens_per_block, self.tome_plans = counts, used
            return DF.run(DF.HeadFn, x.view(B, n, D), self.norm.weight, self.norm.bias, self.head.weight, self.head.bias, self.norm.eps, 0)[0]

    def _forward_train_merge(self, x, plans):
        """The eval forward's launches with everything a backward needs kept: one ToMeBlockFn per block, matching on the fly or replaying."""
        x = self._embed(x)
        size, counts, used = None, [], []
        bf16 = self.train_bf16 and ops.get_gemm_mode() == ops.GEMM_BF16
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            a = blk.attn
            x, size, plan = TF.tome_block_train(x, size, blk._params(), a.num_heads, blk.norm1.eps, a.scale, self.tome_r[i], self.prop_attn,
                                                None if plans is None else plans[i], **({"bf16": True} if bf16 else {}))
            counts.append(x.shape[1])
            used.append(plan)
        self.tokens_per_block, self.tome_plans = counts, used
        return self._head(x)[0]


def _tome(size, tome_r, checkpoint_path=None, **kwargs):
    model = VisionTransformerToMe(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, tome_r=tome_r, **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=True)


def tome_deit_tiny_patch16_224(tome_r=0, checkpoint_path=None, **kwargs):
    return _tome("tiny", tome_r, checkpoint_path, **kwargs)


def tome_deit_small_patch16_224(tome_r=0, checkpoint_path=None, **kwargs):
    return _tome("small", tome_r, checkpoint_path, **kwargs)


def tome_deit_base_patch16_224(tome_r=0, checkpoint_path=None, **kwargs):
    return _tome("base", tome_r, checkpoint_path, **kwargs)
