"""CPU restatement of the Evo-ViT baseline (the build's own definition, PARITY UNPINNED) as plain torch loops, in
float64 unless told otherwise: the selection rule, the four row operations of a slow-fast block with their closed-form backwards, and the
model composed from differentiable torch operations (no in-place write: every block builds a new X), so that autograd gives the gradients
the closed forms and the GPU are held to.  Imports nothing from the package.  No GPU."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32


# ---- the trunk ----
def embed(sd, images, cfg):
    t = F.conv2d(images, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=cfg["patch"]).flatten(2).transpose(1, 2)
    return torch.cat((sd["cls_token"].expand(t.shape[0], -1, -1), t), dim=1) + sd["pos_embed"]


def block(sd, i, x, cfg):
    """Block i on x [B, n, D] -> (y, the CLS row of the softmax [B, H, n])"""
    p = f"blocks.{i}."
    B, n, D = x.shape
    H, eps = cfg["heads"], cfg["ln_eps"]
    dh = D // H
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, n, 3, H, dh).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] @ qkv[1].transpose(-2, -1)) * (dh ** -0.5)).softmax(dim=-1)
    o = (a @ qkv[2]).transpose(1, 2).reshape(B, n, D)
    x = x + F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    z = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    z = F.linear(F.gelu(F.linear(z, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + z, a[:, :, 0, :]


# ---- the selection ----
def topk_rule(g, k):
    """g [B, T] -> (kept [B, k], dropped [B, T-k]) int64, both ascending: value descending, equal values lowest index first"""
    kept, dropped = [], []
    for row in g.detach().tolist():
        order = sorted(range(len(row)), key=lambda t: (-row[t], t))
        kept.append(sorted(order[:k]))
        dropped.append(sorted(order[k:]))
    return torch.tensor(kept, dtype=torch.int64).reshape(g.shape[0], k), torch.tensor(dropped, dtype=torch.int64).reshape(g.shape[0], -1)


def gap(g, k):
    """the smallest distance over the images between the k-th and the (k+1)-th largest value of g"""
    v = torch.sort(g.detach().double(), dim=1, descending=True)[0]
    return float((v[:, k - 1] - v[:, k]).min())


def head_mean(cls_row, lead, count):
    """(sum_h cls_row[b, h, lead + t]) / H, h ascending, t < count"""
    B, H, _ = cls_row.shape
    s = torch.zeros((B, count), dtype=cls_row.dtype)
    for h in range(H):
        s = s + cls_row[:, h, lead:lead + count]
    return s / H


def select(g_in, kept_prev, cls_row, tau, k):
    """-> (g_out, kept, dropped).  kept_prev None: the start from a [B, H, 1+T] row; else the evolution by a [B, H, k+2] row."""
    cls_row = cls_row.detach()
    if kept_prev is None:
        g = head_mean(cls_row, 1, cls_row.shape[2] - 1)
    else:
        g = g_in.detach().clone()
        a = head_mean(cls_row, 1, kept_prev.shape[1])
        for b in range(g.shape[0]):
            for i, t in enumerate(kept_prev[b].tolist()):
                g[b, t] = (1.0 - tau) * g_in[b, t] + tau * a[b, i]
    return (g,) + topk_rule(g, k)


# ---- the row operations of a slow-fast block (dtype follows the inputs) ----
def weights(g, dropped):
    """-> (w [B, m] = g_j / S, S [B]); 0 where S <= 0"""
    gd = torch.gather(g, 1, dropped)
    S = gd.sum(dim=1)
    return torch.where(S[:, None] > 0, gd / S[:, None], torch.zeros_like(gd)), S


def gather(X, g, kept, dropped):
    """-> xc [B, k+2, D] = [CLS | kept | r], r = sum_j (g_j / S) X[1 + dropped_j]"""
    B, _, D = X.shape
    w, _ = weights(g.to(X.dtype), dropped)
    rows = []
    for b in range(B):
        r = (w[b][:, None] * X[b, 1 + dropped[b]]).sum(dim=0, keepdim=True)
        rows.append(torch.cat((X[b, :1], X[b, 1 + kept[b]], r), dim=0))
    return torch.stack(rows)


def scatter_fwd(X, yc, xc, kept, dropped):
    """the write-back, out of place: CLS and kept rows from yc, dropped rows + (yc[k+1] - xc[k+1]) (one subtraction, then one addition)"""
    B = X.shape[0]
    k = kept.shape[1]
    out = []
    for b in range(B):
        d = yc[b, k + 1] - xc[b, k + 1]
        src = [None] * X.shape[1]
        src[0] = yc[b, 0]
        for i, t in enumerate(kept[b].tolist()):
            src[1 + t] = yc[b, 1 + i]
        for t in dropped[b].tolist():
            src[1 + t] = X[b, 1 + t] + d
        out.append(torch.stack(src))
    return torch.stack(out)


def scatter_bwd(dXn, kept, dropped):
    """dXn: the gradient of the written-back X -> dyc [B, k+2, D] (the last row is delta), float64"""
    dXn = dXn.double()
    B = dXn.shape[0]
    rows = []
    for b in range(B):
        delta = dXn[b, 1 + dropped[b]].sum(dim=0, keepdim=True)
        rows.append(torch.cat((dXn[b, :1], dXn[b, 1 + kept[b]], delta), dim=0))
    return torch.stack(rows)


def gather_bwd(dXn, dxc, delta, g, S, kept, dropped):
    """-> dX, float64: CLS and kept rows from dxc, dropped row j = dXn + (g_j / S) (dxc[k+1] - delta).  S as the forward produced it."""
    dXn, dxc, delta, g, S = dXn.double(), dxc.double(), delta.double(), g.double(), S.double()
    B = dXn.shape[0]
    k = kept.shape[1]
    out = dXn.clone()
    for b in range(B):
        out[b, 0] = dxc[b, 0]
        for i, t in enumerate(kept[b].tolist()):
            out[b, 1 + t] = dxc[b, 1 + i]
        for t in dropped[b].tolist():
            w = g[b, t] / S[b] if float(S[b]) > 0 else 0.0
            out[b, 1 + t] = dXn[b, 1 + t] + w * (dxc[b, k + 1] - delta[b])
    return out


def gather_bwd_bound(dXn, dxc, delta, g, S, dropped):
    """Elementwise bound [B, m, D] on the fp32 error of a dropped row of gather_bwd.  The fp32 result is fl(dXn + fl(w) * fl(dxc_r - delta))
    in at most four roundings (the weight's division, the subtraction, the product, the sum - three with a fused multiply-add), each of
    relative size U.  To first order the error is at most U |dxc_r - delta| w (the subtraction) + U w |e| (the weight) + U w |e| (the
    product) + U |result| (the sum), and |e| <= |dxc_r| + |delta|, |result| <= |dXn| + w (|dxc_r| + |delta|): in all at most
    4 U (|dXn| + w (|dxc_r| + |delta|)); the second-order terms are below U times that."""
    dXn, dxc, delta, g, S = dXn.double(), dxc.double(), delta.double(), g.double(), S.double()
    B = dXn.shape[0]
    out = []
    for b in range(B):
        w = torch.gather(g[b], 0, dropped[b]) / S[b]
        mag = dXn[b, 1 + dropped[b]].abs() + w[:, None] * (dxc[b, -1].abs() + delta[b].abs())[None, :]
        out.append(4 * U * (1 + U) * mag)
    return torch.stack(out)


# ---- the model ----
def forward(sd, images, cfg, start, keep, tau, dtype=torch.float64, kept_forced=None):
    """sd: {name: tensor} (tensors that require grad are differentiated through).  kept_forced: one [B, k] list per slow-fast block to replay
    instead of ranking g (the bf16 arithmetic mode's own selections).
    -> dict: logits, tokens (the final X), g (the final score), kept (one [B, k] per slow-fast block), gaps (gap(g, k) at every selection)"""
    X = embed(sd, images.to(dtype), cfg)
    L, T = cfg["depth"], X.shape[1] - 1
    k = int(T * keep)
    kept_all, gaps = [], []
    g = kept = dropped = None
    for i in range(L):
        if i < start:
            X, a = block(sd, i, X, cfg)
            if i == start - 1:
                g, kept, dropped = select(None, None, a, tau, k)
                gaps.append(gap(g, k))
            continue
        if kept_forced is not None:
            kept = kept_forced[i - start]
            dropped = torch.tensor([[t for t in range(T) if t not in set(row)] for row in kept.tolist()], dtype=torch.int64)
        xc = gather(X, g, kept, dropped)
        yc, a = block(sd, i, xc, cfg)
        X = scatter_fwd(X, yc, xc, kept, dropped)
        kept_all.append(kept)
        if i < L - 1:
            g, kept, dropped = select(g, kept, a, tau, k)
            gaps.append(gap(g, k))
    xn = F.layer_norm(X[:, 0], (X.shape[2],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return dict(logits=F.linear(xn, sd["head.weight"], sd["head.bias"]), tokens=X, g=g, kept=kept_all, gaps=gaps)
