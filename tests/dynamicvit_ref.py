"""Plain torch (CPU) restatement of the DynamicViT baseline's forward with the Gumbel noise as an input, in the precision of the state
dict it is handed (fp32 or float64), and of the pieces the kernel tests compare against.  Test infrastructure; not part of oracle/."""
import torch
import torch.nn.functional as F

DH = 64


def policy_attention(qkv, policy, H, scale, eps=1e-6):
    """qkv [B, n, 3*H*64] (the qkv Linear's output), policy [B, n] -> [B, n, H*64]: Attention.forward with softmax_with_policy."""
    B, n, _ = qkv.shape
    q, k, v = qkv.reshape(B, n, 3, H, DH).permute(2, 0, 3, 1, 4)
    attn = (q @ k.transpose(-2, -1)) * scale
    m = policy.reshape(B, 1, 1, n)
    eye = torch.eye(n, dtype=qkv.dtype).view(1, 1, n, n)
    m = m + (1.0 - m) * eye
    attn = attn - attn.max(dim=-1, keepdim=True)[0].detach()
    attn = attn.exp() * m
    attn = (attn + eps / n) / (attn.sum(dim=-1, keepdim=True) + eps)
    return (attn @ v).transpose(1, 2).reshape(B, n, H * DH)


def policy_pool(x, p):
    """x [B, N, C], p [B, N] -> [B, N, C]: PredictorLG's local / policy-weighted global halves"""
    B, N, C = x.shape
    g = (x[:, :, C // 2:] * p[:, :, None]).sum(dim=1, keepdim=True) / p.sum(dim=1)[:, None, None]
    return torch.cat([x[:, :, :C // 2], g.expand(B, N, C // 2)], dim=-1)


def gumbel_keep(logp, g, prev):
    """F.gumbel_softmax(logp, tau=1, hard=True)[..., 0] * prev with the noise given.  -> (decision, hard, y0)"""
    y = F.softmax(logp + g, dim=-1)
    hard = F.one_hot(y.argmax(dim=-1), 2).to(y.dtype)
    st = hard - y.detach() + y
    return st[..., 0] * prev, hard[..., 0], y[..., 0]


def predictor(sd, pre, x, policy):
    g = lambda k: sd[pre + k]
    D = x.shape[-1]
    h = F.gelu(F.linear(F.layer_norm(x, (D,), g("in_conv.0.weight"), g("in_conv.0.bias"), 1e-5), g("in_conv.1.weight"), g("in_conv.1.bias")))
    h = policy_pool(h, policy)
    h = F.gelu(F.linear(h, g("out_conv.0.weight"), g("out_conv.0.bias")))
    h = F.gelu(F.linear(h, g("out_conv.2.weight"), g("out_conv.2.bias")))
    return F.log_softmax(F.linear(h, g("out_conv.4.weight"), g("out_conv.4.bias")), dim=-1)


def block(sd, pre, x, policy, H):
    g = lambda k: sd[pre + k]
    D = x.shape[-1]
    h = F.layer_norm(x, (D,), g("norm1.weight"), g("norm1.bias"), 1e-6)
    qkv = F.linear(h, g("attn.qkv.weight"), g("attn.qkv.bias"))
    pol = policy if policy is not None else torch.ones(x.shape[:2], dtype=x.dtype)
    if policy is None:
        B, n, _ = qkv.shape
        q, k, v = qkv.reshape(B, n, 3, H, DH).permute(2, 0, 3, 1, 4)
        a = ((q @ k.transpose(-2, -1)) * DH ** -0.5).softmax(dim=-1)
        o = (a @ v).transpose(1, 2).reshape(B, n, H * DH)
    else:
        o = policy_attention(qkv, pol, H, DH ** -0.5)
    x = x + F.linear(o, g("attn.proj.weight"), g("attn.proj.bias"))
    h = F.layer_norm(x, (D,), g("norm2.weight"), g("norm2.bias"), 1e-6)
    return x + F.linear(F.gelu(F.linear(h, g("mlp.fc1.weight"), g("mlp.fc1.bias"))), g("mlp.fc2.weight"), g("mlp.fc2.bias"))


def forward(sd, cfg, images, noise=None, training=True):
    """cfg: dict(patch, heads, depth, pruning_loc, token_ratio, init_n).  Training: noise = list of [B, N, 2] per stage; returns
    dict(logits, features, decisions [per stage], gaps [per stage: |(logp_0 + g_0) - (logp_1 + g_1)|]).  Eval: dict(logits, gaps)."""
    dt = sd["pos_embed"].dtype
    x = F.conv2d(images.to(dt), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=cfg["patch"]).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], dim=1) + sd["pos_embed"]
    init_n = cfg["init_n"]
    prev = torch.ones(B, init_n, dtype=dt)
    policy = torch.ones(B, init_n + 1, dtype=dt)
    decisions, gaps, p = [], [], 0
    for i in range(cfg["depth"]):
        pre = f"blocks.{i}."
        if i in cfg["pruning_loc"]:
            if training:
                logp = predictor(sd, f"score_predictor.{p}.", x[:, 1:], prev)
                a = logp + noise[p].to(dt)
                gaps.append((a[..., 0] - a[..., 1]).abs().min())
                prev, _, _ = gumbel_keep(logp, noise[p].to(dt), prev)
                decisions.append(prev)
                policy = torch.cat([torch.ones(B, 1, dtype=dt), prev], dim=1)
                x = block(sd, pre, x, policy, cfg["heads"])
            else:
                n_now = x.shape[1] - 1
                score = predictor(sd, f"score_predictor.{p}.", x[:, 1:], torch.ones(B, n_now, dtype=dt))[:, :, 0]
                k = int(init_n * cfg["token_ratio"][p])
                srt = torch.sort(score, dim=1, descending=True)
                if k < n_now:
                    gaps.append((srt.values[:, k - 1] - srt.values[:, k]).min())
                ids = torch.cat([torch.zeros(B, 1, dtype=torch.long), srt.indices[:, :k] + 1], dim=1)
                x = torch.gather(x, 1, ids[:, :, None].expand(-1, -1, x.shape[-1]))
                x = block(sd, pre, x, None, cfg["heads"])
            p += 1
        else:
            x = block(sd, pre, x, policy if training else None, cfg["heads"])
    x = F.layer_norm(x, (x.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-6)
    logits = F.linear(x[:, 0], sd["head.weight"], sd["head.bias"])
    return dict(logits=logits, features=x[:, 1:], decisions=decisions, gaps=gaps)


def probe(out, cfg):
    """A fixed linear probe of everything a training forward returns (deterministic weights): its gradient reaches every parameter, the
    predictors' through the policy of the masked softmax and the pooling only."""
    def w(t, seed):
        gen = torch.Generator().manual_seed(seed)
        return torch.randn(t.shape, generator=gen, dtype=torch.float64).to(dtype=t.dtype, device=t.device)
    s = (out["logits"] * w(out["logits"], 1)).sum() + (out["features"] * w(out["features"], 2)).sum() * 0.1
    for i, d in enumerate(out["decisions"]):
        s = s + (d * w(d, 10 + i)).sum() * 0.05
    return s


def loss(logits_s, feat_s, mask, decisions, logits_t, feat_t, labels, ratios, cls_weight=1.0, ratio_weight=2.0, dist_weight=0.5):
    """The DynamicViT objective (losses.DynamicViTLoss) written out term by term.  labels: int64 classes or [B, classes] soft targets;
    mask [B, N]: the final decision (no gradient); decisions: one [B, N] per stage.  -> dict(total, cls, ratio, kl, token)"""
    B = logits_s.shape[0]
    ls, lt = torch.log_softmax(logits_s, -1), torch.log_softmax(logits_t.detach(), -1)
    if labels.dtype == torch.long:
        cls = -ls.gather(1, labels[:, None]).sum() / B
    else:
        cls = -(labels.to(ls.dtype) * ls).sum() / B
    ratio = sum(((d.sum(1) / d.shape[1] - r) ** 2).sum() / B for d, r in zip(decisions, ratios)) / len(ratios)
    kl = (lt.exp() * (lt - ls)).sum() / B
    m = mask.detach()
    token = (m * ((feat_s - feat_t.detach()) ** 2).sum(-1) / feat_s.shape[-1]).sum() / m.sum()
    total = cls_weight * cls + ratio_weight * ratio + dist_weight * kl + dist_weight * token
    return dict(total=total, cls=cls, ratio=ratio, kl=kl, token=token)
