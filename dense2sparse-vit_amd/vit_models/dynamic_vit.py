"""MI355X-native counterpart of the reference's vit_models/dynamic_vit.py.

Same module-level names, constructor signatures, state-dict keys, forward return tuples and post-forward attributes as
the reference, so train.py / evaluate.py style callers run unchanged - but every arithmetic
operation is a hand-written HIP kernel reached through the C ABI (d2s.functional / d2s.ops).  nn.Linear / nn.LayerNorm /
nn.Conv2d objects are kept purely as parameter containers (they give the reference's state-dict key names); their own
forward is never called.  There is no CPU path: tensors must live on an MI355X and the library must be built.

Line references are to /root/reference/vit_models/dynamic_vit.py.
"""
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from d2s import functional as DF
from .peturbed_topk import PerturbedTopK, draw_seed


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def trunc_normal_(t, std=0.02):
    return nn.init.trunc_normal_(t, std=std, a=-2.0, b=2.0)


def batch_index_select(x, idx):
    """:39-60 - gather rows per batch element (kept for API parity; the model itself uses GatherFn)."""
    if x.dim() == 3:
        B, N, C = x.shape
        off = torch.arange(B, dtype=torch.long, device=x.device).view(B, 1) * N
        return x.reshape(B * N, C)[(idx + off).reshape(-1)].reshape(B, idx.size(1), C)
    if x.dim() == 2:
        B, N = x.shape
        off = torch.arange(B, dtype=torch.long, device=x.device).view(B, 1) * N
        return x.reshape(B * N)[(idx + off).reshape(-1)].reshape(B, idx.size(1))
    raise NotImplementedError


def patch_drop_mask(kept_token_indices, num_patches):
    """The kept / dropped mask reconstruction of the reference's visual outputs (visualizations.py:18-26: scatter ones for the kept
    ids, zeros for the dropped ones) for every stage, in the coordinates of the ORIGINAL patch grid: stage i's ids are relative to the
    tokens that survived stage i-1, so they are first composed with the previous stages' ids.
    kept_token_indices: list of int64 [B, k_i] (model.kept_token_indices) -> list of int64 [B, num_patches] 0/1 masks (1 = kept)."""
    from d2s import ops
    masks, absolute = [], None
    for ids in kept_token_indices:
        ids = ids.contiguous()
        absolute = ids if absolute is None else ops.compose_ids(absolute, ids)
        masks.append(ops.patch_keep_mask(absolute, num_patches))
    return masks



def _scores(predictor, x):
    """predictor.forward_tokens(x); the reference's predictor falls through and returns None without topk_selection (:537) and the
    caller then fails on the unpacking - same outcome here, with a message that says what to pass."""
    out = predictor.forward_tokens(x)
    if out is None:
        raise RuntimeError("the score predictor was built with topk_selection=False: the reference's PredictorLG.forward returns None on that "
                           "path (vit_models/dynamic_vit.py:537), so the pruning stages cannot run - pass --topk-selection / topk_selection=True")
    return out

DIFF_TOPK_THRESHOLD_ERROR = ("diff_topk (perturbed top-k soft gather) applies to the fixed-ratio path only: it cannot be combined with "
                             "patch_score_threshold")
DIFF_TOPK_OVERRIDE_ERROR = ("diff_topk cannot replay a recorded selection in training: kept_token_override fixes the ids, the soft gather "
                            "draws its own; set kept_token_override = None or call eval()")
FUSE_DROPPED_THRESHOLD_ERROR = ("fuse_dropped (one package token per pruning stage) applies to the fixed-ratio path only: with "
                                "patch_score_threshold no token is removed, there is nothing to fuse")
FUSE_DROPPED_TOPK_SELECTION_ERROR = ("fuse_dropped needs topk_selection=True: the package token is weighted by the score predictor's keep "
                                     "probabilities")
FUSE_DROPPED_DIFF_TOPK_ERROR = ("fuse_dropped cannot be combined with diff_topk: the perturbed top-k soft gather mixes every token into every "
                                "kept row and has no dropped set")
SQUEEZE_DROPPED_FUSE_ERROR = ("squeeze_dropped cannot be combined with fuse_dropped: a dropped token is either averaged into the stage's package "
                              "token or squeezed into its nearest kept token, not both")
SQUEEZE_DROPPED_DIFF_TOPK_ERROR = ("squeeze_dropped cannot be combined with diff_topk: the perturbed top-k soft gather mixes every token into "
                                   "every kept row and has no dropped set")
RAGGED_TRAIN_THRESHOLD_ERROR = ("ragged_train trains the dynamic keep ratio on the ragged packed batch: it needs patch_score_threshold (the "
                                "fixed-ratio path already trains on the kept tokens alone)")
RAGGED_BF16_ERROR = ("ragged_bf16 puts training on the ragged packed batch into the bf16 arithmetic mode: it needs ragged_train=True "
                     "(--ragged-train)")
RAGGED_TRAIN_DROP_PATH_ERROR = "ragged_train with drop_path_rate > 0: stochastic depth is not built for a ragged block"
RAGGED_CASCADE_BN_ERROR = ("ragged inference through more than one threshold stage is not built for the BatchNorm score predictor "
                           "(predictor_bn=True): a stage after the first scores a ragged packed batch, which needs the LayerNorm "
                           "predictor; one stage works with either")
SQUEEZE_DROPPED_THRESHOLD_ERROR = ("squeeze_dropped applies to the fixed-ratio path only: with patch_score_threshold no token is removed, there "
                                   "is nothing to squeeze")
SQUEEZE_DROPPED_TOPK_SELECTION_ERROR = ("squeeze_dropped needs topk_selection=True: the kept and dropped sets are those of the hard top-k of the "
                                        "fixed-ratio path")
ATTN_SELECTION_TOPK_SELECTION_ERROR = ("attn_selection needs topk_selection=True: the CLS attention is ranked by the hard top-k of the fixed-ratio "
                                       "path (the reference's recipe sets both, mask_predictor.py:147-148)")
ATTN_SELECTION_THRESHOLD_ERROR = ("attn_selection applies to the fixed-ratio path only: it cannot be combined with patch_score_threshold")
ATTN_SELECTION_DIFF_TOPK_ERROR = ("attn_selection cannot be combined with diff_topk: the perturbed top-k trains the score predictor, which "
                                  "attention selection never calls")
ATTN_SELECTION_BLOCK0_ERROR = ("attn_selection cannot prune at block 0: a stage is scored by the CLS attention of the block before it, and "
                               "there is no attention before block 0")
GRAPH_RANK_NEGATIVE_ERROR = "graph_rank_iters counts PageRank iterations over the block's attention graph: it cannot be negative"
GRAPH_RANK_ATTN_SELECTION_ERROR = ("graph_rank_iters > 0 needs attn_selection=True: graph ranking replaces the CLS attention row that "
                                   "attention selection ranks, and the score predictor has no use for it")
SIM_PRUNE_NEGATIVE_ERROR = "sim_prune counts the candidates a stage prunes for resembling a more important one: it cannot be negative"
SIM_PRUNE_ATTN_SELECTION_ERROR = ("sim_prune > 0 needs attn_selection=True: the similarity stage prunes among the candidates that attention "
                                  "selection ranks by importance, and the score predictor's stages have no such ranking to refine")


class DropPath(nn.Module):
    """Stochastic depth per sample (timm's DropPath as restated in vit_models/deit.py:69-89): identity in eval or at rate 0; in training
    x[b] * floor(keep + u[b]) / keep.  The draw is made on the device from a seed taken from torch's default CPU generator (draw_seed).
    Inside a Block the scaling is fused into the proj / fc2 GEMM epilogues (the model hands the block its rows of one per-step table);
    this forward serves stand-alone use."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def draw(self, B, device, seed=None):
        """-> s [B]: 0 or 1 / keep"""
        from d2s import ops
        rates = torch.full((1,), float(self.drop_prob), dtype=torch.float32, device=device)
        return ops.drop_path_scales(rates, B, draw_seed() if seed is None else seed)[0]

    def forward(self, x):
        if not self.drop_prob or not self.training:
            return x
        return DF.DropPathFn.apply(x, self.draw(x.shape[0], x.device))

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"


def drop_path_rates(drop_path_rate, depth):
    """dpr of the reference's trunks (:694): linspace(0, rate, depth) as Python floats"""
    return [x.item() for x in torch.linspace(0, drop_path_rate, depth)]


class _DropPathTable:
    """The per-step table of a model's stochastic-depth draws: [2 * depth, B] fp32 scales (row 2i: block i's attention branch, 2i + 1:
    its MLP branch) in ONE persistent buffer per batch size, filled by one launch at the start of a training forward.  Not a registered
    buffer: the state-dict keys are those of a model without stochastic depth."""

    def __init__(self, rates):
        self.rates = [float(r) for r in rates for _ in (0, 1)]
        self.active = any(r > 0. for r in self.rates)
        self._dev = {}      # (device, B) -> (rates tensor, table)

    def buffers(self, B, device):
        key = (str(device), B)
        ent = self._dev.get(key)
        if ent is None:
            if len(self._dev) >= 4:      # batch sizes come and go (a shorter last batch, evaluation): keep a handful of buffers, not a history
                self._dev.clear()
            ent = self._dev[key] = (torch.tensor(self.rates, dtype=torch.float32, device=device),
                                    torch.empty((len(self.rates), B), dtype=torch.float32, device=device))
        return ent

    def fill(self, B, device, masks=None, seed=None):
        """-> table [2 * depth, B].  masks: injected 0/1 draws [2 * depth, B] (tests, fixtures) used instead of the generator."""
        from d2s import ops
        rates, table = self.buffers(B, device)
        if masks is not None:
            assert tuple(masks.shape) == tuple(table.shape), f"drop_path_masks must be [2 * depth, B] = {tuple(table.shape)}"
            table.copy_(masks.to(device=device, dtype=torch.float32) / (1.0 - rates)[:, None])
        else:
            ops.drop_path_scales(rates, B, draw_seed() if seed is None else seed, out=table)
        return table

    def rows(self, table, i):
        """(s_attn, s_mlp) of block i; None where the block's rate is 0 (the block then issues its plain launches)"""
        if table is None or self.rates[2 * i] == 0.:
            return None
        return table[2 * i], table[2 * i + 1]


class _DropPathModel:
    """What a model with stochastic depth shares (mixed into _ViTBase and T2T_ViT): the rate, the per-block rates and the table."""

    def _init_drop_path(self, drop_path_rate, depth):
        """-> dpr, the per-block rates for the Block constructors"""
        assert 0. <= drop_path_rate < 1., "drop_path_rate is a probability below 1"
        self.drop_path_rate = float(drop_path_rate)
        dpr = drop_path_rates(drop_path_rate, depth)      # :694 stochastic depth decay rule
        self._drop_path = _DropPathTable(dpr)
        # injected draws (tests, fixtures): a 0/1 tensor [2 * depth, B] used instead of the generator until set back to None
        self.drop_path_masks = None
        return dpr

    def _drop_path_table(self, B, device):
        """The table of this forward's stochastic-depth draws, or None (eval, no gradient wanted, rate 0).  Each forward gets its OWN
        copy of the persistent buffer (12 KB at depth 12, B 128): the rows are kept for the backward, and a second training forward
        before the first one's backward (gradient accumulation, two forwards under one loss) refills the buffer."""
        t = self._drop_path
        if not (self.training and t.active and torch.is_grad_enabled()):
            return None
        return t.fill(B, device, masks=self.drop_path_masks).clone()


def block_drop_path_rows(block, x, rows):
    """The trailing BlockFn inputs of a block's stochastic depth: (policy slot, s_attn, s_mlp) or () - in eval, without gradients and at
    rate 0.  Without rows from a model's table (stand-alone use) the block makes its own two draws."""
    if not (block.training and isinstance(block.drop_path, DropPath) and torch.is_grad_enabled()):
        return None
    if rows is None:
        rows = (block.drop_path.draw(x.shape[0], x.device), block.drop_path.draw(x.shape[0], x.device))
    return tuple(rows)


class Mlp(nn.Module):
    """:159-175."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        assert drop == 0., "dropout is identity at the rates the reference uses (p=0)"
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        shape = x.shape
        h = DF.LinearFn.apply(x.reshape(-1, shape[-1]), self.fc1.weight, self.fc1.bias, "gelu")
        return DF.LinearFn.apply(h, self.fc2.weight, self.fc2.bias, None).reshape(*shape[:-1], -1)


class Attention(nn.Module):
    """:179-236.  policy / softmax_with_policy (:195-214) belongs to the patch_score_threshold path."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        assert dim % num_heads == 0 and dim // num_heads == 64, "the HIP attention kernels are specialised for head_dim 64"
        assert attn_drop == 0. and proj_drop == 0.
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def softmax_with_policy(self, attn, policy, eps=1e-6):
        """:195-214 on a materialised score tensor (stand-alone operator; Block / Attention.forward use the fused form)."""
        return DF.PolicySoftmaxFn.apply(attn, policy, eps)

    def forward(self, x, policy=None, return_cls_attn=False):
        B, N, C = x.shape
        qkv = DF.LinearFn.apply(x.reshape(B * N, C), self.qkv.weight, self.qkv.bias, None)
        if policy is not None:      # :229 softmax_with_policy, fused into the attention pass
            o, cls_row = DF.AttnCoreFn.apply(qkv, B, N, self.num_heads, self.scale, bool(return_cls_attn), DF.as_policy(policy, B, N))
        else:
            o, cls_row = DF.AttnCoreFn.apply(qkv, B, N, self.num_heads, self.scale, bool(return_cls_attn))
        o = DF.LinearFn.apply(o, self.proj.weight, self.proj.bias, None).reshape(B, N, C)
        return (o, cls_row) if return_cls_attn else o


class Block(nn.Module):
    """:240-283.  The whole block (LN, qkv, fused attention, proj+residual, LN, fc1+GELU, fc2+residual) is one Function."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        assert 0. <= drop_path < 1., "drop_path is a probability below 1"
        assert qkv_bias, "qkv_bias=True everywhere on the path"
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()      # :249
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def _params(self):
        a, m = self.attn, self.mlp
        return (self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias,
                self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)

    def forward(self, x, policy=None, return_cls_attn=False, drop_path_rows=None):
        """drop_path_rows: (s_attn, s_mlp), this block's rows [B] of the model's stochastic-depth table; without them a block in training
        mode with a rate above 0 makes its own two draws (stand-alone use)."""
        a = self.attn
        extra = () if policy is None else (DF.as_policy(policy, x.shape[0], x.shape[1]),)     # :263-283 with policy -> fused policy softmax
        rows = block_drop_path_rows(self, x, drop_path_rows)
        if rows is not None:
            extra = (extra[0] if extra else None,) + rows
        y, cls_row = DF.run(DF.BlockFn, x, *self._params(), a.num_heads, self.norm1.eps, bool(return_cls_attn), a.scale, *extra)
        return (y, cls_row) if return_cls_attn else y

    def forward_ranked(self, x, iters, drop_path_rows=None):
        """The block before a graph-ranked stage: forward(x, return_cls_attn=True) through the per-op launch
        sequence, which also ranks the block's n tokens by `iters` PageRank steps over its attention graph.
        -> (y, cls_row, rank [B, H, n] without a gradient)"""
        from d2s import functional_graph_rank as GF
        a = self.attn
        return GF.rank_block(x, self._params(), a.num_heads, self.norm1.eps, a.scale, iters, want_cls=True,
                             drop_path_rows=block_drop_path_rows(self, x, drop_path_rows))

    def forward_with_metric(self, x, iters=0, drop_path_rows=None):
        """The block before a stage with similarity pruning: forward(x, return_cls_attn=True) through the per-op
        launch sequence, which also emits the key metric of the block's n tokens and, with `iters` > 0, their PageRank as
        forward_ranked does.  -> (y, cls_row, metric [B, n, 64], rank [B, H, n] or None), the side outputs without a gradient"""
        from d2s import functional_sim_prune as SF
        a = self.attn
        return SF.metric_block(x, self._params(), a.num_heads, self.norm1.eps, a.scale, iters, want_cls=True,
                               drop_path_rows=block_drop_path_rows(self, x, drop_path_rows))

    def forward_ragged(self, xp, cu_seqlens, B, max_n, return_cls_attn=False):
        """The block on a ragged packed batch [total, D] (inference with a dynamic keep ratio, :935-949).  Forward only."""
        a = self.attn
        y, cls_rows = DF.ragged_block_forward(xp, cu_seqlens, B, max_n, self._params(), a.num_heads, self.norm1.eps, a.scale,
                                              want_cls=bool(return_cls_attn))
        return (y, cls_rows) if return_cls_attn else y


class PatchEmbed(nn.Module):
    """:286-306."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        img_size, patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

    def check(self, x):
        H, W = x.shape[2], x.shape[3]
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."

    def forward(self, x):
        """Patch tokens without CLS / pos (API parity); the models call EmbedFn which fuses those adds."""
        self.check(x)
        D = self.proj.weight.shape[0]
        T = self.num_patches
        zeros_pos = torch.zeros((1, T + 1, D), dtype=torch.float32, device=x.device)
        zeros_cls = torch.zeros((1, 1, D), dtype=torch.float32, device=x.device)
        return DF.run(DF.EmbedFn, x, self.proj.weight, self.proj.bias, zeros_cls, zeros_pos, self.patch_size[0])[:, 1:]


class BatchNormLayer(nn.Module):
    """:350-367: BatchNorm1d over all B * N token rows of a [B, N, D] tensor (the reference transposes around nn.BatchNorm1d).  Holds
    the parameters / running estimates under the reference's keys (`bn.weight`, `bn.running_mean`, ...); inside the predictor the
    arithmetic runs in d2s.functional_bn.PredictorBNFn, standalone use goes through the same kernels."""

    def __init__(self, input_dim=384):
        super().__init__()
        self.bn = nn.BatchNorm1d(input_dim)

    def forward(self, x):
        from d2s import ops
        B, N, D = x.shape
        if torch.is_grad_enabled() and (x.requires_grad or self.bn.weight.requires_grad):
            raise NotImplementedError("differentiable standalone BatchNormLayer: use it through PredictorLG (predictor_bn=True)")
        y, _, _ = ops.batchnorm_fwd(x.contiguous().view(B * N, D), self.bn.weight, self.bn.bias, self.bn.running_mean,
                                    self.bn.running_var, self.training, eps=self.bn.eps, momentum=self.bn.momentum)
        if self.training:
            self.bn.num_batches_tracked += 1
        return y.view(B, N, D)


class PredictorLG(nn.Module):
    """:370-560.  Large LayerNorm variant (:491-531) runs as one Function; keys follow the nn.Sequential positions."""

    def __init__(self, embed_dim=384, topk_selection=False, k=None, small_predictor=False, loss_type="kl_div", use_bn=False):
        super().__init__()
        self.small_predictor, self.k, self.topk_selection, self.loss_type, self.use_bn = small_predictor, k, topk_selection, loss_type, use_bn
        D = embed_dim
        relu = nn.ReLU()
        if use_bn and small_predictor:      # :383-400: small BatchNorm predictor (ReLU, unlike the small LayerNorm one which uses GELU)
            self.in_conv = nn.Sequential(BatchNormLayer(D), nn.Linear(D, D), relu)
            self.out_conv = nn.Sequential(BatchNormLayer(D), nn.Linear(D, D // 2), relu, BatchNormLayer(D // 2),
                                          nn.Linear(D // 2, D // 4), relu, BatchNormLayer(D // 4), nn.Linear(D // 4, 1),
                                          nn.Flatten(start_dim=-2, end_dim=-1))
            self.topk = PerturbedTopK(k)
            return
        if use_bn:               # :438-476: the large predictor with BatchNormLayer in place of every LayerNorm
            self.in_conv = nn.Sequential(BatchNormLayer(D), nn.Linear(D, D * 4), relu)
            self.out_conv = nn.Sequential(
                BatchNormLayer(D * 4), nn.Linear(D * 4, D * 2), relu,
                BatchNormLayer(D * 2), nn.Linear(D * 2, D), relu,
                BatchNormLayer(D), nn.Linear(D, D // 2), relu,
                BatchNormLayer(D // 2), nn.Linear(D // 2, D // 4), relu,
                BatchNormLayer(D // 4), nn.Linear(D // 4, 1), nn.Flatten(start_dim=-2, end_dim=-1))
            self.topk = PerturbedTopK(k)
            return
        if small_predictor:      # :409-426 (LayerNorm + GELU variant)
            self.in_conv = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, D), nn.GELU())
            self.out_conv = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, D // 2), nn.GELU(), nn.LayerNorm(D // 2),
                                          nn.Linear(D // 2, D // 4), nn.GELU(), nn.LayerNorm(D // 4), nn.Linear(D // 4, 1),
                                          nn.Flatten(start_dim=-2, end_dim=-1))
            self.topk = PerturbedTopK(k)
            return
        self.in_conv = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, D * 4), relu)
        self.out_conv = nn.Sequential(
            nn.LayerNorm(D * 4), nn.Linear(D * 4, D * 2), relu,
            nn.LayerNorm(D * 2), nn.Linear(D * 2, D), relu,
            nn.LayerNorm(D), nn.Linear(D, D // 2), relu,
            nn.LayerNorm(D // 2), nn.Linear(D // 2, D // 4), relu,
            nn.LayerNorm(D // 4), nn.Linear(D // 4, 1), nn.Flatten(start_dim=-2, end_dim=-1))
        self.topk = PerturbedTopK(k)

    def _params(self):
        norm = (lambda m: m.bn) if self.use_bn else (lambda m: m)
        ps = [norm(self.in_conv[0]).weight, norm(self.in_conv[0]).bias, self.in_conv[1].weight, self.in_conv[1].bias]
        for i in ((0, 3, 6) if self.small_predictor else (0, 3, 6, 9, 12)):
            ps += [norm(self.out_conv[i]).weight, norm(self.out_conv[i]).bias, self.out_conv[i + 1].weight, self.out_conv[i + 1].bias]
        return ps

    def _bn_layers(self):
        return [self.in_conv[0].bn] + [self.out_conv[i].bn for i in ((0, 3, 6) if self.small_predictor else (0, 3, 6, 9, 12))]

    def forward_tokens(self, x_with_cls):
        """Scores for x[:, 1:] of a [B, n, D] tensor, read in place (no slice copy).  -> (scores, keep_probs)."""
        if not self.topk_selection:
            return None  # the reference's forward falls through and returns None (:537)
        if self.loss_type not in ("kl_div", "mse"):
            raise NotImplementedError("sigmoid scores (bce loss type) are not on the accelerated hot path")
        if self.use_bn:
            from d2s.functional_bn import PredictorBNFn
            bns = self._bn_layers()
            running = [t for bn in bns for t in (bn.running_mean, bn.running_var)]
            out = DF.run(PredictorBNFn, x_with_cls, self.training, running, *self._params())
            if self.training:
                for bn in bns:
                    bn.num_batches_tracked += 1
            return out
        return DF.run(DF.PredictorFn, x_with_cls, *self._params(), *(("gelu",) if self.small_predictor else ()))

    def forward(self, x, policy=None, current_sigma=0.0005, cls_attn=None):
        """Reference signature: x is the CLS-free token tensor [B, N, D] (:855 passes x[:, 1:])."""
        B, N, D = x.shape
        pad = torch.zeros((B, 1, D), dtype=x.dtype, device=x.device)
        return self.forward_tokens(torch.cat([pad, x], dim=1))


class _ViTBase(_DropPathModel, nn.Module):
    def _build_trunk(self, img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale,
                     representation_size, drop_rate, attn_drop_rate, drop_path_rate, hybrid_backbone, norm_layer):
        assert hybrid_backbone is None, "HybridEmbed is not on the hot path"
        assert representation_size is None, "pre_logits representation layer is unused by the reference's factories"
        assert drop_rate == 0. and attn_drop_rate == 0., "dropout is 0 on the path"
        dpr = self._init_drop_path(drop_path_rate, depth)
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.pre_logits = nn.Identity()
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()

    def _init_weights(self, m):
        """:794-801."""
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def _embed(self, x):
        self.patch_embed.check(x)
        return DF.run(DF.EmbedFn, x, self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.cls_token, self.pos_embed,
                                self.patch_embed.patch_size[0])

    def _head(self, x, tail=0):
        """tail: trailing rows of x that are package tokens (fuse_dropped) - normalised with the rest, left out of the features"""
        return DF.run(DF.HeadFn, x, self.norm.weight, self.norm.bias, self.head.weight, self.head.bias, self.norm.eps, tail)


class VisionTransformerDiffPruning(_ViTBase):
    """:642-1015 - the student.  Hard top-k by score (argsort path, :858-862), kept-token gather (:907-912).

    attn_selection=True (the branch the reference names at :265 and never connects): the stage at block i ranks its
    tokens by the CLS attention row that block i - 1 of the same forward returned - max over heads, or the mean with mean_heads=True,
    renormalised over the stage's scored tokens - instead of by the score predictor.  `score_predictor` is still constructed (state-dict keys
    and checkpoints are unchanged) and never called; `pred_logits` then holds each stage's attention PROBABILITIES [B, T], detached (not
    logits: there is no predictor output), and no gradient reaches the attention row through the selection or the fused package token.

    graph_rank_iters=T > 0 (with attn_selection; the importance stage of Zero-TPrune, the build's own definition):
    the stage ranks by T steps of PageRank over the whole attention graph of block i - 1, s <- s P from s = 1 / n per head, instead of by
    that block's CLS row; the rank has the CLS row's layout and goes through the same reduction, renormalisation and top-k.
    `graph_ranks` holds each stage's rank [B, H, n] after a forward, detached.  T = 1 is the mean attention a token receives.

    sim_prune=R > 0 (with attn_selection; the similarity stage of Zero-TPrune, the build's own definition): the
    stage takes k + r candidates by importance (the CLS row, or the graph rank), r = min(R, k, T - k), and prunes the r of the less
    important half that have the highest cosine, between the key metrics of block i - 1, to a candidate of the more important half; it
    still keeps k tokens.  `sim_plans` holds each stage's (pruned, partner, sim) [B, r] after a forward, detached, and
    `sim_prune_counts` each stage's r.

    squeeze_dropped=True (pruning and squeezing, the build's own definition): a stage keeps the k tokens its selector
    chose and folds every token it drops into the kept token with the highest cosine, so the sequence lengths are those of plain pruning;
    `squeeze_plans` holds each stage's (dst, sim) after a forward."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None,
                 pruning_loc=None, token_ratio=None, distill=False, attn_selection=False, attn_selection_threshold=0.0,
                 topk_selection=False, early_exit=False, mean_heads=False, random_drop=False, small_predictor=False,
                 predictor_loss_type=False, predictor_bn=False, patch_score_threshold=None, fuse_dropped=False, squeeze_dropped=False,
                 ragged_train=False, ragged_bf16=False, graph_rank_iters=0, sim_prune=0, init_n=14 * 14, diff_topk=False,
                 topk_num_samples=500):
        super().__init__()
        if int(sim_prune) < 0:
            raise ValueError(SIM_PRUNE_NEGATIVE_ERROR)
        if int(sim_prune) > 0 and not attn_selection:
            raise ValueError(SIM_PRUNE_ATTN_SELECTION_ERROR)
        if int(graph_rank_iters) < 0:
            raise ValueError(GRAPH_RANK_NEGATIVE_ERROR)
        if int(graph_rank_iters) > 0 and not attn_selection:
            raise ValueError(GRAPH_RANK_ATTN_SELECTION_ERROR)
        if ragged_bf16 and not ragged_train:
            raise ValueError(RAGGED_BF16_ERROR)
        if ragged_train and patch_score_threshold is None:
            raise ValueError(RAGGED_TRAIN_THRESHOLD_ERROR)
        if ragged_train and float(drop_path_rate) > 0.0:
            raise ValueError(RAGGED_TRAIN_DROP_PATH_ERROR)
        if squeeze_dropped and fuse_dropped:
            raise ValueError(SQUEEZE_DROPPED_FUSE_ERROR)
        if squeeze_dropped and diff_topk:
            raise ValueError(SQUEEZE_DROPPED_DIFF_TOPK_ERROR)
        if squeeze_dropped and patch_score_threshold is not None:
            raise ValueError(SQUEEZE_DROPPED_THRESHOLD_ERROR)
        if squeeze_dropped and not topk_selection:
            raise ValueError(SQUEEZE_DROPPED_TOPK_SELECTION_ERROR)
        if fuse_dropped and patch_score_threshold is not None:
            raise ValueError(FUSE_DROPPED_THRESHOLD_ERROR)
        if fuse_dropped and diff_topk:
            raise ValueError(FUSE_DROPPED_DIFF_TOPK_ERROR)
        if fuse_dropped and not topk_selection:
            raise ValueError(FUSE_DROPPED_TOPK_SELECTION_ERROR)
        if diff_topk and patch_score_threshold is not None:
            raise ValueError(DIFF_TOPK_THRESHOLD_ERROR)
        if diff_topk and not topk_selection:
            raise ValueError("diff_topk needs topk_selection=True: the perturbed top-k acts on the score predictor's keep probabilities")
        if attn_selection:
            if not topk_selection:
                raise ValueError(ATTN_SELECTION_TOPK_SELECTION_ERROR)
            if patch_score_threshold is not None:
                raise ValueError(ATTN_SELECTION_THRESHOLD_ERROR)
            if diff_topk:
                raise ValueError(ATTN_SELECTION_DIFF_TOPK_ERROR)
            if 0 in list(pruning_loc or []):
                raise ValueError(ATTN_SELECTION_BLOCK0_ERROR)
        self._build_trunk(img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale,
                          representation_size, drop_rate, attn_drop_rate, drop_path_rate, hybrid_backbone, norm_layer)
        if early_exit:      # :752-758: the head is created (state-dict keys, 'early_exit' parameter group) but no forward path of the
            # reference ever calls it, so its parameters never receive a gradient and the optimiser never moves them
            self.early_exit_head = nn.Sequential((norm_layer or partial(nn.LayerNorm, eps=1e-6))(embed_dim),
                                                 nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity())
        pruning_loc = list(pruning_loc or [])
        token_ratio = list(token_ratio or [])
        isz = img_size if isinstance(img_size, int) else img_size[0]
        psz = patch_size if isinstance(patch_size, int) else patch_size[0]
        self.score_predictor = nn.ModuleList([
            PredictorLG(embed_dim, topk_selection=topk_selection, k=int(token_ratio[i] * (isz / psz) ** 2),
                        small_predictor=small_predictor, loss_type=predictor_loss_type, use_bn=predictor_bn)
            for i in range(len(pruning_loc))])
        self.num_kept_tokens = []
        self.attn_selection, self.attn_selection_threshold = attn_selection, attn_selection_threshold
        self.topk_selection = topk_selection
        if self.topk_selection:
            self.current_sigma = 0.05
        self.mean_heads, self.random_drop, self.current_score, self.early_exit = mean_heads, random_drop, None, early_exit
        self.cls_attns = []
        # graph ranking: PageRank iterations over the attention graph of the block before each stage (0: the CLS row ranks, as ever);
        # graph_ranks[s] = stage s's rank [B, H, n] after a forward, detached
        self.graph_rank_iters = int(graph_rank_iters)
        self.graph_ranks = []
        # similarity pruning: candidates a stage prunes for resembling a more important one (0: the importance ranking alone decides, as
        # ever); after a forward sim_plans[s] = stage s's (pruned, partner, sim) [B, r], detached, and sim_prune_counts[s] its r
        self.sim_prune = int(sim_prune)
        self.sim_plans, self.sim_prune_counts = [], []
        self.kept_token_indices = None
        self.dropped_token_indices = None
        self.pred_logits = []
        self.patch_score_threshold = patch_score_threshold
        self.keep_ratios = None          # :886 / :941 - per-image kept fraction of the last thresholded stage (device tensor)
        self.cu_seqlens = self.ragged_row_src = None     # ragged inference: packed-row offsets per image / ORIGINAL token of each row (last stage)
        self.cu_seqlens_per_stage, self.ragged_row_src_per_stage = [], []     # the same after every threshold stage
        # replay of a recorded selection (analysis / tests): a list of int64 [B, k_i] kept-id tensors, one per stage, used INSTEAD of the
        # top-k of this forward's scores (which are still computed and returned); None = normal operation
        self.kept_token_override = None
        # differentiable token selection (the "dense to sparse" scheme the reference states at :896-900 and never connects): in a training
        # forward every stage's kept-token gather becomes PerturbedTopK(keep_probs; k, topk_num_samples, current_sigma) @ tokens
        self.diff_topk = bool(diff_topk)
        self.topk_num_samples = int(topk_num_samples)       # peturbed_topk.py:6
        if self.topk_num_samples < 1:
            raise ValueError("topk_num_samples must be at least 1")
        # injected perturbation noise (tests, fixtures): a list of [B, topk_num_samples, N_i] tensors, one per stage, used instead of the
        # device stream until set back to None
        self.topk_noise = None
        # inspection (tests): with keep_topk_indicators set, the last soft forward's indicators [B, k_i, N_i] per stage stay referenced here
        # (detached) until the next forward; off by default so that nothing outlives the step
        self.keep_topk_indicators = False
        self.topk_indicators = []
        # token fusion (EViT's fused token / SPViT's package token, weighted by this selector's own keep probabilities): every stage
        # appends sum_{j in dropped} (p_j / sum p) x_j as one extra row, which later stages carry along unscored;
        # training and eval alike - the pruned inference model carries the package tokens too
        self.fuse_dropped = bool(fuse_dropped)
        # pruning and squeezing (TPS): every stage folds each token it drops into the kept token with the highest cosine, at weight
        # exp(cosine) against the kept token's own exp(1); the stage still hands on 1 + k rows; training and eval
        # alike.  squeeze_plans[s] = (dst, sim) of stage s after a forward, detached; squeeze_plan_override replays a list of such plans
        # (tests: the counterpart of kept_token_override)
        self.squeeze_dropped = bool(squeeze_dropped)
        self.squeeze_plans = []
        self.squeeze_plan_override = None
        # dynamic keep ratio only: a training forward runs the inference cascade, differentiable, on the ragged packed batch instead of
        # masking keys over all N tokens; eval() is untouched
        self.ragged_train = bool(ragged_train)
        # ... and does so in the bf16 arithmetic mode too: the flag, not the mode, selects the path - without it
        # that mode is refused; in an fp32 mode it changes nothing
        self.ragged_bf16 = bool(ragged_bf16)
        self.unpruned = False
        self.distill = distill
        self.pruning_loc, self.token_ratio = pruning_loc, token_ratio
        # the reference hard-codes init_n = 14*14 (:828,852); exposed so that 384x384 inputs can use int(N * ratio) instead
        self.init_n = init_n
        # optional callable(block_index): invoked from autograd when every parameter gradient of block i and of all later
        # layers is final (d2s.engine uses it to start the bucketed gradient all-reduce while backward continues)
        self.grad_ready_hook = None
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)

    # :887-889 / :942-944 read the minimum / mean / maximum kept fraction with three .item() calls (three device syncs per stage per
    # step); here they are derived from `keep_ratios` only when a caller looks at them
    @property
    def min_keep_ratio(self):
        return None if self.keep_ratios is None else float(self.keep_ratios.min())

    @property
    def avg_keep_ratio(self):
        return None if self.keep_ratios is None else float(self.keep_ratios.mean())

    @property
    def max_keep_ratio(self):
        return None if self.keep_ratios is None else float(self.keep_ratios.max())

    def forward(self, x, stacked_cls_attn_weights=None):
        if self.patch_score_threshold is not None:
            return self._forward_threshold(x)
        dp = self._drop_path_table(x.shape[0], x.device)
        soft = self._soft_selection()
        soft_seed = draw_seed() if (soft and self.topk_noise is None) else None     # one draw per training forward, mixed with the stage index
        self.topk_indicators = []
        x = self._embed(x)                                                  # :816-824
        self.num_kept_tokens, self.cls_attns, self.pred_logits = [], [], []
        self.kept_token_indices, self.dropped_token_indices = [], []
        self.squeeze_plans = []
        self.graph_ranks = []
        self.sim_plans, self.sim_prune_counts = [], []
        p_count = 0
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            if i in self.pruning_loc:
                num_keep_node = int(self.init_n * self.token_ratio[p_count])   # :852
                carried = p_count if self.fuse_dropped else 0                 # trailing package rows of earlier stages: never scored
                n_scored = x.shape[1] - 1 - carried
                if self.attn_selection:      # the CLS row block i - 1 just returned: reduce over heads, renormalise, rank - one launch
                    row = prev_cls_row
                    if self.graph_rank_iters > 0:      # ... or its tokens' PageRank over that block's attention graph, in the row's layout
                        row = prev_rank
                        self.graph_ranks.append(prev_rank)
                    # similarity pruning: r candidates more, of which the stage prunes the r that resemble a more important one most
                    sim_r = DF.ops.sim_prune_clip_r(self.sim_prune, num_keep_node, n_scored) if self.sim_prune > 0 else 0
                    pred_logits, kept, dropped = DF.ops.select_cls_attn(row.detach().contiguous(), 1, n_scored, num_keep_node + sim_r,
                                                                        self.mean_heads)
                    if self.sim_prune > 0:
                        self.sim_prune_counts.append(sim_r)
                    if sim_r > 0:
                        kept, dropped, *plan = DF.ops.sim_prune(prev_metric, pred_logits, kept, 1, sim_r)
                        self.sim_plans.append(tuple(t.detach() for t in plan))
                    elif self.sim_prune > 0:
                        self.sim_plans.append(tuple(torch.empty((x.shape[0], 0), dtype=dt, device=x.device)
                                                    for dt in (torch.int64, torch.int64, torch.float32)))
                else:
                    scored = x[:, :x.shape[1] - carried].contiguous() if carried else x
                    pred_logits, pred_score = _scores(self.score_predictor[p_count], scored)   # :855
                    kept, dropped = DF.select_topk(pred_score, num_keep_node)     # :858-862
                if self.kept_token_override is not None:
                    kept = self.kept_token_override[p_count].to(device=x.device, dtype=torch.int64).contiguous()
                    assert kept.shape == (x.shape[0], num_keep_node), "override ids must be [B, int(init_n * ratio)]"
                    keep_mask = DF.ops.patch_keep_mask(kept, n_scored)
                    dropped = torch.nonzero(keep_mask == 0)[:, 1].reshape(x.shape[0], -1)
                self.kept_token_indices.append(kept)
                self.dropped_token_indices.append(dropped)
                self.pred_logits.append(pred_logits)
                if soft:                                                     # :896-900
                    x = self._soft_gather(x, pred_logits, num_keep_node, p_count, soft_seed)
                elif self.fuse_dropped and self.attn_selection:      # the package token weighted by the attention probabilities, as a constant
                    x = DF.GatherFuseFn.apply(x, pred_logits, kept, dropped.contiguous(), carried)
                elif self.fuse_dropped:      # the bits of the predictor's own keep_probs, differentiable: the task loss reaches the scores
                    x = DF.GatherFuseFn.apply(x, DF.KeepProbsFn.apply(pred_logits), kept, dropped.contiguous(), carried)
                elif self.squeeze_dropped:   # the selection decides who survives; every dropped token goes into its nearest survivor
                    plan = None
                    if self.squeeze_plan_override is not None:
                        plan = (self.squeeze_plan_override[p_count][0].to(device=x.device, dtype=torch.int32).contiguous(),
                                self.squeeze_plan_override[p_count][1].to(device=x.device, dtype=torch.float32).contiguous())
                    x, dst, sim = DF.GatherSqueezeFn.apply(x, kept, dropped.contiguous(), plan)
                    self.squeeze_plans.append((dst.detach(), sim.detach()))
                else:
                    x = DF.GatherFn.apply(x, kept)                           # :907-912 / :954-960
                p_count += 1
            if self.sim_prune > 0 and (i + 1) in self.pruning_loc:      # the block before a similarity stage also emits its key metric
                x, cls_attn, prev_metric, prev_rank = blk.forward_with_metric(x, self.graph_rank_iters,
                                                                              drop_path_rows=self._drop_path.rows(dp, i))
                prev_metric = prev_metric.detach()
                prev_rank = prev_rank.detach() if prev_rank is not None else None
            elif self.graph_rank_iters > 0 and (i + 1) in self.pruning_loc:      # the block before a ranked stage also ranks its tokens
                x, cls_attn, prev_rank = blk.forward_ranked(x, self.graph_rank_iters, drop_path_rows=self._drop_path.rows(dp, i))
                prev_rank = prev_rank.detach()
            else:
                x, cls_attn = blk(x, return_cls_attn=True, drop_path_rows=self._drop_path.rows(dp, i))   # :924 / :985
            prev_cls_row = cls_attn
            self.cls_attns.append(cls_attn[:, :, 1:])
        logits, features = self._head(x, tail=p_count if self.fuse_dropped else 0)   # :993-1006
        if self.training:
            return logits, features, self.pred_logits, self.kept_token_indices   # :1013
        return logits, self.cls_attns, self.pred_logits, self.kept_token_indices  # :1015

    def _soft_selection(self):
        """Does this forward use the soft gather?  Only a training forward that keeps a graph does: eval(), torch.no_grad() and every
        forward-only branch keep the hard gather (the pruned inference model is what this training produces), and so does
        sigma <= 0, where the perturbed top-k IS the hard top-k and its gradient (1 / sigma) is undefined."""
        if not (self.diff_topk and self.training and torch.is_grad_enabled()):
            return False
        if self.kept_token_override is not None:
            raise RuntimeError(DIFF_TOPK_OVERRIDE_ERROR)
        return float(self.current_sigma) > 0.

    def _soft_gather(self, x, scores, k, stage, seed):
        """x [B, n, D] -> [B, k + 1, D]: CLS passes through, row 1 + i = sum_j ind[b, i, j] x[b, 1 + j] with ind the perturbed top-k
        indicators of the keep probabilities.  Row i of ind is the i-th selected id in ascending order - the order of `kept`."""
        from d2s import ops
        B, n, _ = x.shape
        probs = DF.KeepProbsFn.apply(scores)                                 # :551, the bits of the predictor's own keep_probs
        if self.topk_noise is not None:
            noise = self.topk_noise[stage].to(device=x.device, dtype=torch.float32).contiguous()
            assert tuple(noise.shape) == (B, self.topk_num_samples, n - 1), \
                f"topk_noise[{stage}] must be [B, topk_num_samples, N] = {(B, self.topk_num_samples, n - 1)}"
        else:
            noise = ops.normal_noise((B, self.topk_num_samples, n - 1), (seed + 0x9E3779B97F4A7C15 * (stage + 1)) & 0xFFFFFFFFFFFFFFFF, x.device)
        ind = DF.PerturbedTopKFn.apply(probs, noise, int(k), float(self.current_sigma))
        if self.keep_topk_indicators:
            self.topk_indicators.append(ind.detach())
        return DF.SoftGatherFn.apply(x, ind)

    def _forward_threshold(self, x):
        """Dynamic keep ratio (patch_score_threshold is set).

        Training (:880-894, :981-983, :1010-1011): no token is removed.  Each pruning stage turns its keep probabilities into a 0/1 mask
        (tokens whose ascending cumulative probability exceeds the threshold are kept), and that stage's block and every later block
        attend through Attention.softmax_with_policy with the mask as key policy; the blocks before the first stage use the all-ones
        policy, exactly as the reference does.  A later stage REPLACES the mask (the reference does not intersect them).
        Returns (logits, features [B,N,D], [pred_logits per stage], [keep mask [B,N] per stage]) - lists, where the reference returns the
        last stage's tensors only (:1011): the per-stage mask loss needs every stage.
        With ragged_train=True the training forward is the inference cascade below instead, differentiable
        (_forward_threshold_ragged_train).

        Inference (:935-949, with the reference's undefined `score` read as `pred_score`): the kept tokens of every image are packed
        into one ragged batch [total, D] (`cu_seqlens` [B+1] gives each image's rows) and the remaining blocks run on it - LayerNorm
        and GEMMs over all packed rows, attention per image.  A stage after the first (the reference's scatters an n_kept-long mask into
        an N-long buffer and cannot run; the build's definition) acts on the packed batch, per image: the score
        predictor runs over the image's surviving non-CLS tokens (its global half is their mean, its softmax runs over them), the
        threshold rule selects among them, the kept rows are packed again - what the remaining network gives on each image alone.
        Unlike training, where a later stage scores all N tokens and replaces the mask, a token dropped here is gone.
        Returns (logits, [cls rows: dense [B,H,N] before the first stage, packed [H,total_s] after stage s; a pruning block returns
        none], [pred_logits: dense [B,N] for the first stage, packed [total_{s-1}] for a later one (the CLS rows' entries have no
        meaning)], [cumulative keep mask [B,N] per stage, original patch coordinates]).  `cu_seqlens` / `ragged_row_src` (the ORIGINAL
        token index of every packed row, 0 for CLS) are the last stage's, `cu_seqlens_per_stage` / `ragged_row_src_per_stage` hold
        every stage's; `keep_ratios` = survivors of the last stage / N; `ragged_features` = the final LayerNorm of the last packed batch."""
        from d2s import ops
        from d2s.functional_ragged import ragged_predictor_forward
        thr = float(self.patch_score_threshold)
        dp = self._drop_path_table(x.shape[0], x.device)
        x = self._embed(x)
        B, n, D = x.shape
        N = n - 1
        self.num_kept_tokens, self.cls_attns, self.pred_logits = [], [], []
        self.kept_token_indices, self.dropped_token_indices = [], []       # here: per-stage keep masks / their complements
        self.cu_seqlens = self.ragged_row_src = None
        self.cu_seqlens_per_stage, self.ragged_row_src_per_stage = [], []
        p_count = 0
        if self.training and self.ragged_train:
            return self._forward_threshold_ragged_train(x, thr)
        if self.training:
            policy = torch.ones((B, n), dtype=torch.float32, device=x.device)       # :830,839
            for i, blk in enumerate(self.blocks):
                if self.grad_ready_hook is not None and x.requires_grad:
                    x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
                if i in self.pruning_loc:
                    pred_logits, pred_score = _scores(self.score_predictor[p_count], x)      # :855
                    policy, counts = ops.select_threshold(pred_score.detach().contiguous(), thr, lead=1)   # :881-893 -> [1, mask]
                    self.keep_ratios = counts.float() / N                                          # :886
                    self.pred_logits.append(pred_logits)
                    self.kept_token_indices.append(policy[:, 1:])
                    self.dropped_token_indices.append(1.0 - policy[:, 1:])
                    p_count += 1
                x = blk(x, policy=policy, drop_path_rows=self._drop_path.rows(dp, i))             # :894 / :983
            logits, features = self._head(x)
            return logits, features, self.pred_logits, self.kept_token_indices
        if len(self.pruning_loc) > 1 and any(p.use_bn for p in self.score_predictor):
            raise NotImplementedError(RAGGED_CASCADE_BN_ERROR)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("ragged inference is forward only: call it under torch.no_grad()")
        cu = None
        for i, blk in enumerate(self.blocks):
            if i in self.pruning_loc:
                if cu is None:
                    pred_logits, pred_score = _scores(self.score_predictor[p_count], x)
                    mask, counts = ops.select_threshold(pred_score.contiguous(), thr)              # :936-938 (score := pred_score)
                    cu = ops.ragged_offsets(counts, extra=1)
                    total = int(cu[-1])      # the one device sync of a stage: the packed row count sizes every later launch
                    x, self.ragged_row_src = ops.ragged_pack(x, mask, cu, total)                   # :947-948
                else:       # a later stage acts on the packed batch: per image, over the tokens that survived
                    pred_logits = ragged_predictor_forward(self.score_predictor[p_count], x, cu, B)          # packed [total]
                    keep, counts, mask, _ = ops.ragged_select_threshold(pred_logits, cu, self.ragged_row_src, thr, N, B)
                    cu_new = ops.ragged_offsets(counts, extra=1)
                    total = int(cu_new[-1])
                    x, self.ragged_row_src = ops.ragged_repack(x, keep, cu, cu_new, self.ragged_row_src, total, B)
                    cu = cu_new
                self.keep_ratios = counts.float() / N                                              # :941
                self.pred_logits.append(pred_logits)
                self.kept_token_indices.append(mask)
                self.dropped_token_indices.append(1.0 - mask)
                self.cu_seqlens = cu
                self.cu_seqlens_per_stage.append(cu)
                self.ragged_row_src_per_stage.append(self.ragged_row_src)
                x = blk.forward_ragged(x, cu, B, n)                                                # :949 blk(x)
                p_count += 1
            elif cu is None:
                x, cls_attn = blk(x, return_cls_attn=True)                                         # :987
                self.cls_attns.append(cls_attn[:, :, 1:])
            else:
                x, cls_rows = blk.forward_ragged(x, cu, B, n, return_cls_attn=True)
                self.cls_attns.append(cls_rows)             # packed [H, total]; image b's CLS row is columns cu[b] .. cu[b+1]
        if cu is None:
            logits, features = self._head(x)
            return logits, self.cls_attns, self.pred_logits, self.kept_token_indices
        total = x.shape[0]
        xn, _, _ = ops.layernorm_fwd(x, ops.contiguous_map(total, D), self.norm.weight, self.norm.bias, total, D, self.norm.eps, stats=False)
        cls_rows = ops.gather_rows_i32(xn, cu, B)                                                  # :996 x[:, 0] of every image
        logits = ops.linear_fwd(cls_rows, self.head.weight, self.head.bias)
        self.ragged_features = xn
        return logits, self.cls_attns, self.pred_logits, self.kept_token_indices

    def _forward_threshold_ragged_train(self, x, thr):
        """ragged_train=True, training mode (the build's own definition; PARITY UNPINNED): the inference cascade
        above made differentiable.  x [B, n, D] is the embedded batch.  Plain dense blocks up to the first stage; the first stage scores
        all N tokens with the dense predictor exactly as the policy-mode training forward does and packs the survivors (RaggedPackFn); its
        block and every later block is a RaggedBlockFn without a stage of its own; a later stage scores the packed rows
        (RaggedPredictorFn), selects per image among the survivors and packs again (RaggedRepackFn); the final LayerNorm runs over the
        packed rows, the head on the gathered CLS rows.  Selections carry no gradient; ONE host read of the new row total per stage.
        Returns (logits, the normed packed batch [total, D] with its CLS rows, [pred_logits: dense [B, N], then packed [total_{s-1}]],
        [cumulative dense [B, N] keep mask per stage]); cu_seqlens / ragged_row_src and the _per_stage lists are set as at inference."""
        from d2s import functional_ats as AF
        from d2s import functional_ragged as RF
        from d2s import ops
        from d2s.lib import D2SError
        bf16 = ops.get_gemm_mode() == ops.GEMM_BF16
        if bf16 and not self.ragged_bf16:
            raise D2SError(AF._BF16_REFUSAL)
        if len(self.pruning_loc) > 1 and any(p.use_bn for p in self.score_predictor):
            raise NotImplementedError(RAGGED_CASCADE_BN_ERROR)
        B, n, D = x.shape
        N = n - 1
        p_count = 0
        cu = row_src = None
        max_n = n
        for i, blk in enumerate(self.blocks):
            if self.grad_ready_hook is not None and x.requires_grad:
                x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
            if i in self.pruning_loc:
                if cu is None:
                    pred_logits, pred_score = _scores(self.score_predictor[p_count], x)
                    policy, counts = ops.select_threshold(pred_score.detach().contiguous(), thr, lead=1)
                    mask = policy[:, 1:]
                    cu = ops.ragged_offsets(counts, extra=1)
                    total = int(cu[-1])      # the one device sync of a stage: the packed row count sizes every later launch
                    x, row_src = RF.RaggedPackFn.apply(x, policy, cu, total)
                else:
                    pred_logits = RF.ragged_predictor_train(self.score_predictor[p_count], x, cu, B, bf16=bf16)          # packed [total]
                    keep, counts, mask, _ = ops.ragged_select_threshold(pred_logits.detach(), cu, row_src, thr, N, B)
                    cu_new = ops.ragged_offsets(counts, extra=1)
                    total = int(cu_new[-1])
                    x, row_src = RF.RaggedRepackFn.apply(x, keep, cu, cu_new, row_src, total, B)
                    cu = cu_new
                self.keep_ratios = counts.float() / N
                self.pred_logits.append(pred_logits)
                self.kept_token_indices.append(mask)
                self.dropped_token_indices.append(1.0 - mask)
                self.cu_seqlens, self.ragged_row_src = cu, row_src
                self.cu_seqlens_per_stage.append(cu)
                self.ragged_row_src_per_stage.append(row_src)
                p_count += 1
            if cu is None:
                x = blk(x)
            else:
                a = blk.attn
                x = AF.ragged_block_train(x, blk._params(), blk.norm1.eps, AF._Ragged(cu, B, max_n, a.num_heads, a.scale, bf16=bf16))
        if cu is None:       # no stage at all: the dense head
            logits, features = self._head(x)
            return logits, features, self.pred_logits, self.kept_token_indices
        logits, xn = RF.ragged_head(x, cu, self.norm, self.head)
        self.ragged_features = xn.detach()
        return logits, xn, self.pred_logits, self.kept_token_indices

    def forward_cls_attn(self, x):
        """:1018-1033."""
        x = self._embed(x)
        final = None
        for i, blk in enumerate(self.blocks):
            if i == len(self.blocks) - 1:
                _, final = blk(x, return_cls_attn=True)
            else:
                x = blk(x)
        return final


class VisionTransformerTeacher(_ViTBase):
    """:1036-1176 - dense frozen teacher; every block returns its (detached) CLS row."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None):
        super().__init__()
        self._build_trunk(img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale,
                          representation_size, drop_rate, attn_drop_rate, drop_path_rate, hybrid_backbone, norm_layer)
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(self._init_weights)

    def forward_cls_attention(self, x):
        """:1134-1148."""
        x = self._embed(x)
        rows = []
        for blk in self.blocks:
            x, cls_attns = blk(x, return_cls_attn=True)
            rows.append(cls_attns.detach())
        return torch.stack(rows, dim=1)

    def forward(self, x):
        """:1150-1176 -> (logits, tokens[B,N,D], cls_attn[B,depth,H,N+1])."""
        x = self._embed(x)
        rows = []
        for blk in self.blocks:
            x, cls_attns = blk(x, return_cls_attn=True)
            rows.append(cls_attns.detach())
        logits, tokens = self._head(x)
        return logits, tokens, torch.stack(rows, dim=1)


def resize_pos_embed(posemb, posemb_new):
    """Position-embedding table of a checkpoint trained at another resolution -> this model's grid (reference :1178-1195): the CLS
    row is kept, the square patch grid is resampled bilinearly (align_corners=False).  Host side, runs once at load time."""
    cls_row, grid = posemb[:, :1], posemb[0, 1:]
    side_old = int(math.sqrt(grid.shape[0]))
    side_new = int(math.sqrt(posemb_new.shape[1] - 1))
    dim = grid.shape[-1]
    grid = grid.t().reshape(1, dim, side_old, side_old)                               # [1, D, h, w]
    grid = F.interpolate(grid, size=(side_new, side_new), mode='bilinear')
    grid = grid.reshape(dim, side_new * side_new).t().unsqueeze(0)                    # [1, h'w', D]
    return torch.cat([cls_row, grid], dim=1)


def checkpoint_filter_fn(state_dict, model):
    """Make a DeiT-style checkpoint loadable (reference :1198-1213): unwrap {'model': ...}, give a patch-projection weight stored as a
    matrix its conv shape, and resample a position table of a different resolution."""
    source = state_dict.get('model', state_dict)
    conv_shape = model.patch_embed.proj.weight.shape

    def adapt(key, value):
        if 'patch_embed.proj.weight' in key and value.dim() < 4:
            return value.reshape(conv_shape[0], -1, conv_shape[2], conv_shape[3])
        if key == 'pos_embed' and value.shape != model.pos_embed.shape:
            return resize_pos_embed(value, model.pos_embed)
        return value

    return {key: adapt(key, value) for key, value in source.items()}


def _load_local(model, checkpoint_path, strict):
    """The reference's factories download DeiT weights (:1221 ff.); there is no network here, so a local file is
    the only source.  weights_only=True: nothing from the file is executed."""
    if checkpoint_path is None:
        return model
    sd = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    missing, unexpected = model.load_state_dict(checkpoint_filter_fn(sd, model), strict=strict)
    from d2s import ops
    ops.invalidate_bf16_weights()       # cached bf16 forms of frozen weights follow the version counter; a fresh load starts clean anyway
    print('# missing keys=', missing)
    print('# unexpected keys=', unexpected)
    return model


_GEOM = {"tiny": dict(embed_dim=192, num_heads=3), "small": dict(embed_dim=384, num_heads=6), "base": dict(embed_dim=768, num_heads=12)}


def _student(size, pruning_locs, keep_ratios, checkpoint_path=None, **kwargs):
    model = VisionTransformerDiffPruning(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, pruning_loc=pruning_locs,
                                         token_ratio=keep_ratios, distill=True, **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=False)


def _teacher(size, checkpoint_path=None):
    model = VisionTransformerTeacher(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, **_GEOM[size])
    return _load_local(model, checkpoint_path, strict=True)


def dynamic_vit_tiny_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("tiny", pruning_locs, keep_ratios, **kwargs)


def dynamic_vit_small_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("small", pruning_locs, keep_ratios, **kwargs)


def dynamic_vit_base_patch16_224_student(pruning_locs, keep_ratios, **kwargs):
    return _student("base", pruning_locs, keep_ratios, **kwargs)


def dynamic_vit_tiny_patch16_224_teacher(checkpoint_path=None):
    return _teacher("tiny", checkpoint_path)


def dynamic_vit_small_patch16_224_teacher(checkpoint_path=None):
    return _teacher("small", checkpoint_path)


def dynamic_vit_base_patch16_224_teacher(checkpoint_path=None):
    return _teacher("base", checkpoint_path)
