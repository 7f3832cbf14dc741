"""Float64 restatement of token merging (ToMe, Bolya et al. 2023) as DESIGN.md section 22 defines it: the metric, the bipartite match under
the build's tie rules, the size-weighted merge, the key-weighted attention and a whole-model forward that can replay per-block plans.
Plain torch on the CPU; the tests compare the HIP kernels against it."""
import math

import torch
import torch.nn.functional as F


def clip_r(r, n):
    return max(0, min(int(r), (int(n) - 1) // 2))


def metric(qkv):
    """qkv [B,n,3,H,64] -> [B,n,64] float64: mean of the keys over the heads, divided by its L2 norm (a zero row is not special-cased)"""
    k = qkv[:, :, 1].double()
    m = k.sum(dim=2) / k.shape[2]
    return m / m.norm(dim=-1, keepdim=True)


def scores(qkv):
    m = metric(qkv)
    return m[:, 0::2] @ m[:, 1::2].transpose(-1, -2)           # [B, T_a, T_b]


def match(qkv, r):
    """-> (node_max [B,T_a] f64, node_idx [B,T_a], unm [B,T_a-r], src [B,r], dst [B,r]) int64; r is clipped to (n - 1) // 2.
    node_idx: lowest index attaining the maximum; CLS (A row 0): -inf / 0, never a source; sources: value descending, equal values lowest
    index first; unm and src ascending."""
    B, n = qkv.shape[:2]
    r = clip_r(r, n)
    s = scores(qkv)
    node_max = s.max(dim=-1).values
    node_idx = (s == node_max[..., None]).int().argmax(dim=-1)       # argmax of 0/1: the first maximal entry
    node_max[:, 0] = -math.inf
    node_idx[:, 0] = 0
    Ta = node_max.shape[1]
    unm, src = [], []
    for b in range(B):
        order = sorted(range(1, Ta), key=lambda i: (-float(node_max[b, i]), i))
        sb = sorted(order[:r])
        src.append(sb)
        unm.append([i for i in range(Ta) if i not in set(sb)])
    unm = torch.tensor(unm, dtype=torch.int64).reshape(B, Ta - r)
    src = torch.tensor(src, dtype=torch.int64).reshape(B, r)
    dst = torch.gather(node_idx, 1, src)
    return node_max, node_idx, unm, src, dst


def gaps(qkv, r):
    """The two margins a float32 kernel needs to reproduce match() exactly: (smallest best-minus-second-best score over the non-CLS A rows,
    the r-th minus the (r+1)-th largest node_max among them, smallest over the batch); inf where there is nothing to confuse."""
    B, n = qkv.shape[:2]
    r = clip_r(r, n)
    s = scores(qkv)[:, 1:]
    best = math.inf
    if s.shape[1] > 0 and s.shape[2] >= 2:
        top = s.topk(2, dim=-1).values
        best = float((top[..., 0] - top[..., 1]).min())
    rank = math.inf
    if 0 < r < s.shape[1]:
        nm = s.max(dim=-1).values.sort(dim=-1, descending=True).values
        rank = float((nm[:, r - 1] - nm[:, r]).min())
    return best, rank


def merge(x, size, unm, src, dst):
    """x [B,n,D], size [B,n] or None, a plan -> (x_out [B,n-r,D] f64, size_out [B,n-r] f64, group [B,n-r] rows merged into each output row
    (1 = copied), amax [B,n-r] largest |size * x| among a row's contributions)"""
    B, n, D = x.shape
    x = x.double()
    size = torch.ones((B, n), dtype=torch.float64) if size is None else size.double()
    Tb = n // 2
    xo, so, go, ao = [], [], [], []
    for b in range(B):
        rows, sizes, groups, amax = [], [], [], []
        for u in unm[b].tolist():
            rows.append(x[b, 2 * u]); sizes.append(size[b, 2 * u]); groups.append(1); amax.append(float((size[b, 2 * u] * x[b, 2 * u]).abs().max()))
        for j in range(Tb):
            t = 2 * j + 1
            num, den, g, am = size[b, t] * x[b, t], size[b, t].clone(), 1, float((size[b, t] * x[b, t]).abs().max())
            for p in range(src.shape[1]):
                if int(dst[b, p]) == j:
                    st = 2 * int(src[b, p])
                    num = num + size[b, st] * x[b, st]
                    den = den + size[b, st]
                    g += 1
                    am = max(am, float((size[b, st] * x[b, st]).abs().max()))
            rows.append(num / den if g > 1 else x[b, t]); sizes.append(den); groups.append(g); amax.append(am)
        xo.append(torch.stack(rows)); so.append(torch.stack(sizes)); go.append(groups); ao.append(amax)
    return torch.stack(xo), torch.stack(so), torch.tensor(go), torch.tensor(ao, dtype=torch.float64)


def keyw_attention(qkv, key_w, scale):
    """qkv [B,n,3,H,64], key_w [B,n] -> (out [B,n,H*64], lse [B,H,n]): e_ij = exp(S_ij - max_j S_ij) w_j, out = e v / sum_j e"""
    B, n, _, H, dh = qkv.shape
    q, k, v = (qkv[:, :, i].double().transpose(1, 2) for i in range(3))           # [B,H,n,dh]
    S = (q @ k.transpose(-1, -2)) * scale
    mx = S.max(dim=-1, keepdim=True).values
    e = torch.exp(S - mx) * key_w.double()[:, None, None, :]
    den = e.sum(dim=-1, keepdim=True)
    out = (e @ v) / den
    return out.transpose(1, 2).reshape(B, n, H * dh), (mx + torch.log(den)).squeeze(-1)


def model_forward(state_dict, images, r, plans=None, prop_attn=True, eps=1e-6):
    """The dense ViT of `state_dict` (DeiT key names; head dim 64) with token merging, in float64.  r: int or one int per block.  plans: per
    block (unm, src, dst) to replay, or None (entries or the whole list) to match here.  -> (logits, tokens leaving each block)"""
    sd = {k: torch.as_tensor(v).double() for k, v in state_dict.items()}
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    rs = [int(r)] * depth if isinstance(r, int) else [int(v) for v in r]
    w = sd["patch_embed.proj.weight"]
    D, P = w.shape[0], w.shape[-1]
    H = D // 64
    x = F.conv2d(images.double(), w, sd["patch_embed.proj.bias"], stride=P).flatten(2).transpose(1, 2)
    B = x.shape[0]
    x = torch.cat([sd["cls_token"].expand(B, -1, -1), x], dim=1) + sd["pos_embed"]
    size, counts = None, []
    for i in range(depth):
        p = lambda name: sd[f"blocks.{i}.{name}"]
        n = x.shape[1]
        ln = F.layer_norm(x, (D,), p("norm1.weight"), p("norm1.bias"), eps)
        qkv = F.linear(ln, p("attn.qkv.weight"), p("attn.qkv.bias")).reshape(B, n, 3, H, 64)
        kw = size if (size is not None and prop_attn) else torch.ones((B, n), dtype=torch.float64)
        ao, _ = keyw_attention(qkv, kw, 64 ** -0.5)
        x = x + F.linear(ao, p("attn.proj.weight"), p("attn.proj.bias"))
        re = clip_r(rs[i], n)
        if re > 0:
            plan = plans[i] if plans is not None and plans[i] is not None else match(qkv, re)[2:]
            x, size = merge(x, size, *[t.long() for t in plan])[:2]
        ln = F.layer_norm(x, (D,), p("norm2.weight"), p("norm2.bias"), eps)
        x = x + F.linear(F.gelu(F.linear(ln, p("mlp.fc1.weight"), p("mlp.fc1.bias"))), p("mlp.fc2.weight"), p("mlp.fc2.bias"))
        counts.append(x.shape[1])
    xn = F.layer_norm(x[:, 0], (D,), sd["norm.weight"], sd["norm.bias"], eps)
    return F.linear(xn, sd["head.weight"], sd["head.bias"]), counts
