"""MI355X-native counterpart of the reference's vit_models/default_dynamic_vit.py: the DynamicViT baseline the dense-to-sparse students
are measured against.  Same class names, constructor signatures, state-dict keys and forward return values; the arithmetic is the
library's HIP kernels.  Training is dense (no token is removed): every pruning stage draws a hard Gumbel keep decision per token,
multiplies it into the previous stage's decision, and from that stage on every block attends through softmax_with_policy with the
decision as key policy.  The predictors learn ONLY through that policy - the attention backward's policy gradient
(d2s_attn_policy_bwd_dpol_f32) - and through the policy-weighted pooling of the later stages' predictors.

Line references are to the reference's vit_models/default_dynamic_vit.py."""
from functools import partial

import torch
import torch.nn as nn

from d2s import functional as DF
from d2s.functional_dynamicvit import DynPredictorFn, GumbelKeepFn
from .dynamic_vit import (_ViTBase, _load_local, _GEOM, trunc_normal_, batch_index_select, resize_pos_embed, checkpoint_filter_fn,  # noqa: F401
                          Mlp, Attention, Block, PatchEmbed)
from .peturbed_topk import draw_seed


class PredictorLG(nn.Module):
    """:304-330.  Keys follow the nn.Sequential positions (in_conv.0/1, out_conv.0/2/4); the modules only hold the parameters."""

    def __init__(self, embed_dim=384):
        super().__init__()
        D = embed_dim
        self.in_conv = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, D), nn.GELU())
        self.out_conv = nn.Sequential(nn.Linear(D, D // 2), nn.GELU(), nn.Linear(D // 2, D // 4), nn.GELU(), nn.Linear(D // 4, 2),
                                      nn.LogSoftmax(dim=-1))

    def _params(self):
        ps = [self.in_conv[0].weight, self.in_conv[0].bias, self.in_conv[1].weight, self.in_conv[1].bias]
        for i in (0, 2, 4):
            ps += [self.out_conv[i].weight, self.out_conv[i].bias]
        return ps

    def raw_logits(self, x_with_cls, policy):
        """x [B, n, D] read in place behind its CLS row, policy [B, N] -> the 2-way logits BEFORE the LogSoftmax, [B * N, 2]"""
        return DF.run(DynPredictorFn, x_with_cls, policy, *self._params())

    def forward(self, x, policy):
        """Reference signature: x is the CLS-free token tensor [B, N, D], policy [B, N, 1] -> log-probabilities [B, N, 2].  Inference only:
        the model fuses the LogSoftmax into the Gumbel keep decision (raw_logits + GumbelKeepFn), which is the differentiable path; the
        kernels read the tokens behind a CLS row, so a row is put in front here."""
        from d2s import ops
        B, N, D = x.shape
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._params())):
            raise NotImplementedError("PredictorLG.forward is inference-only (call it under torch.no_grad()); training goes through "
                                      "raw_logits + GumbelKeepFn inside DefaultVisionTransformerDiffPruning")
        z = self.raw_logits(torch.cat([x.new_zeros((B, 1, D)), x], dim=1), DF.as_policy(policy, B, N))
        return ops.gumbel_keep_fwd(z.contiguous(), torch.zeros_like(z), torch.ones(B * N, dtype=torch.float32, device=x.device))[0].view(B, N, 2)


class DefaultVisionTransformerDiffPruning(_ViTBase):
    """:333-487.  init_n: the reference hard-codes 14 * 14 (:446); exposed as in VisionTransformerDiffPruning for other resolutions."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None,
                 pruning_loc=None, token_ratio=None, distill=False, init_n=14 * 14):
        super().__init__()
        self._build_trunk(img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale,
                          representation_size, drop_rate, attn_drop_rate, drop_path_rate, hybrid_backbone, norm_layer)
        self.pruning_loc, self.token_ratio = list(pruning_loc or []), list(token_ratio or [])
        self.score_predictor = nn.ModuleList([PredictorLG(embed_dim) for _ in self.pruning_loc])
        self.distill = distill
        self.init_n = init_n
        # injected Gumbel noise (tests, fixtures): a list of [B, N, 2] tensors, one per stage, used instead of the device stream until
        # set back to None
        self.gumbel_noise = None
        self.grad_ready_hook = None
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)

    def _noise(self, stage, B, N, device, seed):
        from d2s import ops
        if self.gumbel_noise is not None:
            g = self.gumbel_noise[stage].to(device=device, dtype=torch.float32).contiguous()
            assert tuple(g.shape) == (B, N, 2), f"gumbel_noise[{stage}] must be [B, N, 2] = {(B, N, 2)}"
            return g
        return ops.gumbel_noise((B, N, 2), (seed + 0x9E3779B97F4A7C15 * (stage + 1)) & 0xFFFFFFFFFFFFFFFF, device)

    def forward(self, x):
        B = x.shape[0]
        dp = self._drop_path_table(B, x.device)
        seed = draw_seed() if (self.training and self.gumbel_noise is None and self.pruning_loc) else None    # one draw per training forward
        x = self._embed(x)                                                      # :437-442
        init_n = self.init_n
        assert not self.training or x.shape[1] - 1 == init_n, f"training keeps all tokens: init_n = {init_n}, the image has {x.shape[1] - 1} patches"
        p_count = 0
        out_pred_prob = []
        prev_decision = torch.ones((B, init_n), dtype=torch.float32, device=x.device)      # :447
        policy = torch.ones((B, init_n + 1), dtype=torch.float32, device=x.device)         # :448
        ones_cls = policy[:, :1]
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            rows = self._drop_path.rows(dp, i)
            if i in self.pruning_loc:
                pred = self.score_predictor[p_count]
                if self.training:
                    z = pred.raw_logits(x, prev_decision)                                           # :452
                    noise = self._noise(p_count, B, init_n, x.device, seed)
                    prev_decision, _ = GumbelKeepFn.apply(z, noise, prev_decision)                  # :454 (tau = 1, hard) * prev_decision
                    out_pred_prob.append(prev_decision)                                             # :455
                    policy = torch.cat([ones_cls, prev_decision], dim=1)                            # :456-457
                    x = blk(x, policy=policy, drop_path_rows=rows)                                  # :458
                else:
                    from d2s import ops
                    n_now = x.shape[1] - 1
                    with torch.no_grad():
                        z = pred.raw_logits(x, torch.ones((B, n_now), dtype=torch.float32, device=x.device))
                        logp = ops.gumbel_keep_fwd(z.contiguous(), torch.zeros_like(z), torch.ones(B * n_now, dtype=torch.float32, device=x.device))[0]
                        score = logp.view(B, n_now, 2)[:, :, 0].contiguous()                        # :461
                    num_keep_node = int(init_n * self.token_ratio[p_count])                         # :462
                    kept, _ = DF.select_topk(score, num_keep_node)       # :463, ids ascending (attention is permutation-equivariant)
                    x = DF.GatherFn.apply(x, kept)                                                  # :464-466
                    x = blk(x)                                                                      # :468
                p_count += 1
            elif self.training:
                x = blk(x, policy=policy, drop_path_rows=rows)                                      # :472
            else:
                x = blk(x)                                                                          # :474
        logits, features = self._head(x)                                                            # :476-480
        if self.training:
            if self.distill:
                return logits, features, prev_decision.detach(), out_pred_prob                      # :483
            return logits, out_pred_prob                                                            # :485
        return logits                                                                               # :487


class DefaultVisionTransformerTeacher(_ViTBase):
    """:489-598 - the dense teacher: (logits, tokens)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None):
        super().__init__()
        self._build_trunk(img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale,
                          representation_size, drop_rate, attn_drop_rate, drop_path_rate, hybrid_backbone, norm_layer)
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)

    def forward(self, x):
        x = self._embed(x)
        for blk in self.blocks:
            x = blk(x)
        return self._head(x)


def _student(size, pruning_locs, keep_ratios, checkpoint_path=None, **kwargs):
    model = DefaultVisionTransformerDiffPruning(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, pruning_loc=pruning_locs,
                                                token_ratio=keep_ratios, distill=True, **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=False)


def _teacher(size, checkpoint_path=None):
    model = DefaultVisionTransformerTeacher(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, **_GEOM[size])
    return _load_local(model, checkpoint_path, strict=True)


def default_dynamic_vit_tiny_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("tiny", pruning_locs, keep_ratios, **kwargs)


def default_dynamic_vit_small_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("small", pruning_locs, keep_ratios, **kwargs)


def default_dynamic_vit_base_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("base", pruning_locs, keep_ratios, **kwargs)


def default_dynamic_vit_tiny_patch16_224_teacher(checkpoint_path=None):
    return _teacher("tiny", checkpoint_path)


def default_dynamic_vit_small_patch16_224_teacher(checkpoint_path=None):
    return _teacher("small", checkpoint_path)


def default_dynamic_vit_base_patch16_224_teacher(checkpoint_path=None):
    return _teacher("base", checkpoint_path)
