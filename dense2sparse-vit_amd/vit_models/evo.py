"""Evo-ViT baseline (Xu et al. 2022, slow-fast token evolution; DESIGN.md section 26 - the build's own definition, no counterpart in the
reference): the dense DeiT trunk in which no token is ever removed.  From block evo_start on a block runs on the k tokens of the highest
global score plus one representative row of the others, and the others are updated cheaply by the representative's residual; the global
score evolves from every block's CLS attention and ALL tokens are re-selected in every block.  No predictor and no new parameter: the
model has the teacher's state-dict keys and loads any DeiT checkpoint.  Every block sees a dense [B, k+2, D] batch of a fixed k: nothing
is read back on the host, all three arithmetic modes train, and the step can be captured."""
import torch

from d2s import functional_evo as EF
from d2s import ops
from .dynamic_vit import VisionTransformerTeacher, _GEOM, _load_local


class VisionTransformerEvo(VisionTransformerTeacher):
    """evo_start s: blocks 0 .. s-1 are dense (1 <= s <= depth; s = depth is the dense trunk); evo_keep: k = int(T * evo_keep) tokens take
    the slow path; evo_tradeoff tau: g[kept] = (1 - tau) g[kept] + tau * (mean over heads of the block's CLS attention).
    forward returns the logits, in train() and eval() mode by the same launches (eval keeps nothing for a backward).  Afterwards:
    evo_kept - one [B, k] int64 per slow-fast block, absolute patch ids (vit_models.patch_drop_mask applies); tokens - the final
    X [B, 1+T, D], the complete grid; global_score - g [B, T] after the last evolution; tokens_per_block - rows each block ran on."""

    def __init__(self, *args, evo_start=4, evo_keep=0.5, evo_tradeoff=0.5, **kwargs):
        super().__init__(*args, **kwargs)
        depth, T = len(self.blocks), self.patch_embed.num_patches
        self.evo_start, self.evo_keep, self.evo_tradeoff = int(evo_start), float(evo_keep), float(evo_tradeoff)
        if self.evo_start != evo_start or not 1 <= self.evo_start <= depth:
            raise ValueError(f"evo_start: an int in 1..{depth} (the depth), got {evo_start!r}")
        self.evo_k = int(T * self.evo_keep)
        if not 1 <= self.evo_k <= T - 1:
            raise ValueError(f"evo_keep {evo_keep!r}: k = int({T} * evo_keep) = {self.evo_k} must lie in 1..{T - 1}")
        if not 0.0 <= self.evo_tradeoff <= 1.0:
            raise ValueError(f"evo_tradeoff: a value in [0, 1], got {evo_tradeoff!r}")
        if float(getattr(self, "drop_path_rate", 0.0)) > 0.0:
            raise ValueError("drop_path_rate > 0: stochastic depth is not built for a slow-fast block")
        self.grad_ready_hook = None          # set by a data-parallel TrainStep: called with i when block i's input gradient exists
        self.evo_kept, self.tokens_per_block = [], []
        self.tokens = self.global_score = None

    def forward(self, x):
        x = self._embed(x)
        L, s, k, tau = len(self.blocks), self.evo_start, self.evo_k, self.evo_tradeoff
        kept_lists, counts = [], []
        g = kept = dropped = None
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda grad, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            if i < s:
                x, a = blk(x, return_cls_attn=True)             # the teacher's launches
                if i == s - 1:
                    g, kept, dropped = ops.evo_select(a.detach().contiguous(), k)
                counts.append(x.shape[1])
                continue
            x, a = EF.slow_fast_block(x, g, kept, dropped, lambda xc, blk=blk: blk(xc, return_cls_attn=True))
            kept_lists.append(kept)
            counts.append(k + 2)
            if i < L - 1:
                g, kept, dropped = ops.evo_select(a.detach().contiguous(), k, tau, g, kept)
        self.evo_kept, self.tokens_per_block = kept_lists, counts
        self.tokens, self.global_score = x.detach(), g
        return self._head(x)[0]


def _evo(size, checkpoint_path=None, **kwargs):
    model = VisionTransformerEvo(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=True)


def evo_deit_tiny_patch16_224(checkpoint_path=None, **kwargs):
    return _evo("tiny", checkpoint_path, **kwargs)


def evo_deit_small_patch16_224(checkpoint_path=None, **kwargs):
    return _evo("small", checkpoint_path, **kwargs)


def evo_deit_base_patch16_224(checkpoint_path=None, **kwargs):
    return _evo("base", checkpoint_path, **kwargs)
