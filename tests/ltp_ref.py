"""Plain torch restatement of the LTP kernels: the score - the attention a token receives - in its three forms as
loops over images and heads, the hard decision of a stage and the soft mask with its closed-form backward.  Nothing here imports the
package; the dtype of the inputs (float64 in the tests) is the dtype of every result."""
import torch


def softmax_rows(S):
    """plain softmax of S [n, n] -> (P, lse [n])"""
    lse = torch.logsumexp(S, dim=1)
    return torch.exp(S - lse[:, None]), lse


def policy_softmax_rows(S, m, eps):
    """softmax_with_policy as the policy attention defines it, S [n, n], m [n]: mk_ij = m_j off the diagonal and 1 on it,
    e_ij = exp(S_ij - max_j S_ij) mk_ij, P_ij = (e_ij + eps / n) / (sum_j e_ij + eps).
    -> (P, lse [n] = max + log(sum e + eps), cinv [n] = (eps / n) / (sum e + eps)), the two statistics the forward saves"""
    n = S.shape[0]
    mk = m[None, :].expand(n, n).clone()
    mk[torch.arange(n), torch.arange(n)] = 1.0
    mx = S.max(dim=1).values
    e = torch.exp(S - mx[:, None]) * mk
    l = e.sum(dim=1) + eps
    return (e + eps / n) / l[:, None], mx + torch.log(l), (eps / n) / l


def _scores(qkv_img, h, scale):
    """qkv_img [n, 3, H, 64] -> S [n, n] of head h"""
    return (qkv_img[:, 0, h] @ qkv_img[:, 1, h].T) * scale


def score_plain(qkv, B, n, H, scale):
    """qkv [B * n, 3, H, 64] -> s [B, n]: s[b, j] = (1 / (H n)) sum_h sum_i P[h, i, j]"""
    qkv = qkv.reshape(B, n, 3, H, 64)
    out = torch.zeros((B, n), dtype=qkv.dtype)
    for b in range(B):
        for h in range(H):
            P, _ = softmax_rows(_scores(qkv[b], h, scale))
            out[b] += P.sum(dim=0)
        out[b] /= H * n
    return out


def score_policy(qkv, policy, B, n, H, scale, eps):
    """policy [B, n] (entry 0, CLS, is 1) -> s [B, n]: s[b, j] = sum_h sum_i m_i P[h, i, j] / (H sum_i m_i), P the policy softmax"""
    qkv = qkv.reshape(B, n, 3, H, 64)
    out = torch.zeros((B, n), dtype=qkv.dtype)
    for b in range(B):
        m = policy[b]
        for h in range(H):
            P, _, _ = policy_softmax_rows(_scores(qkv[b], h, scale), m, eps)
            out[b] += (m[:, None] * P).sum(dim=0)
        out[b] /= H * m.sum()
    return out


def score_varlen(qkv, lens, H, scale):
    """qkv [total, 3, H, 64] packed, image b = the next lens[b] rows -> s [total]"""
    qkv = qkv.reshape(-1, 3, H, 64)
    out = torch.zeros((qkv.shape[0],), dtype=qkv.dtype)
    r0 = 0
    for n in lens:
        out[r0:r0 + n] = score_plain(qkv[r0:r0 + n], 1, n, H, scale)[0]
        r0 += n
    return out


def select(score, lens, theta):
    """-> (keep [total] 0/1 with 1 at every image's first row, counts: kept rows per image without CLS)"""
    keep = (score >= theta).to(score.dtype)
    counts, r0 = [], 0
    for n in lens:
        keep[r0] = 1.0
        counts.append(int(keep[r0 + 1:r0 + n].sum()))
        r0 += n
    return keep, counts


def soft_mask(score, m_in, theta, tau):
    """score, m_in [B, N] -> (M with 1 at CLS, m_out = m_in * M, msum [B] over the patches)"""
    M = torch.sigmoid((score - theta) / tau)
    M = torch.cat((torch.ones_like(M[:, :1]), M[:, 1:]), dim=1)
    return M, m_in * M, M[:, 1:].sum(dim=1)


def soft_mask_bwd(g_out, M, m_in, tau, greg_scaled):
    """The closed form of section 27: gM = g_out * m_in + greg_scaled at the patches (greg_scaled = dLoss/dR / (S B T)), 0 at CLS;
    gm_in = g_out * M; dtheta = -(1 / tau) sum over the patches of gM M (1 - M).  -> (gM, gm_in, dtheta, sum of |summands| of dtheta)"""
    gM = g_out * m_in + greg_scaled
    gM = torch.cat((torch.zeros_like(gM[:, :1]), gM[:, 1:]), dim=1)
    terms = (gM * M * (1.0 - M))[:, 1:]
    return gM, g_out * M, -terms.sum() / tau, terms.abs().sum() / tau


# ---- the model, restated the dense masked way (a full [B, N, D] batch in every block) ----
def _block(sd, i, x, cfg, P_of):
    """Block i on x [B, n, D]; P_of(S [B, H, n, n]) -> the attention probabilities.  -> (y, P)"""
    import torch.nn.functional as F
    from oracle import d2s_oracle as O
    p = f"blocks.{i}."
    B, n, D = x.shape
    H, eps = cfg["heads"], cfg["ln_eps"]
    dh = D // H
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, n, 3, H, dh).permute(2, 0, 3, 1, 4)
    P = P_of((qkv[0] @ qkv[1].transpose(-2, -1)) * (dh ** -0.5))
    o = (P @ qkv[2]).transpose(1, 2).reshape(B, n, D)
    x = x + F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    return x + O.mlp(sd, p + "mlp.", F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)), P


def _logits(sd, x, cfg):
    import torch.nn.functional as F
    xn = F.layer_norm(x[:, 0], (x.shape[-1],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return F.linear(xn, sd["head.weight"], sd["head.bias"])


def model_hard(sd, images, cfg, locs, theta, dtype=torch.float64, replay=None):
    """The hard forward: -inf on pruned keys, pruned rows skipped (they are never read again).  theta: S numbers.  replay: per stage a
    [B, N] bool mask of the rows that go on (the decisions of another run), taken instead of deciding.
    -> dict: logits, live (per stage, the [B, N] bool rows that go on), counts (per block [B] live rows), scores (per stage [B, N]),
    margin (the smallest |s - theta_k| / theta_k over the live patches of every stage; inf where theta_k = 0)"""
    from oracle import d2s_oracle as O
    x = O.embed_tokens(sd, images.to(dtype), cfg)
    B, N, _ = x.shape
    H = cfg["heads"]
    live = torch.ones((B, N), dtype=torch.bool)
    out = dict(live=[], counts=[], scores=[], margin=float("inf"))
    stage = 0
    for l in range(cfg["depth"]):
        out["counts"].append(live.sum(dim=1))
        keys = live
        x, P = _block(sd, l, x, cfg, lambda S: S.masked_fill(~keys[:, None, None, :], float("-inf")).softmax(dim=-1))
        if stage < len(locs) and l == locs[stage]:
            rows = live.to(dtype)
            s = (P.detach() * rows[:, None, :, None]).sum(dim=(1, 2)) / (H * rows.sum(dim=1, keepdim=True))
            th = float(theta[stage])
            patches = live.clone()
            patches[:, 0] = False
            if th > 0 and bool(patches.any()):
                out["margin"] = min(out["margin"], float(((s - th).abs() / th)[patches].min()))
            if replay is not None:
                keep = replay[stage]
            else:
                keep = live & (s >= torch.tensor(th, dtype=dtype))
                keep[:, 0] = True
            live = keep
            out["scores"].append(s)
            out["live"].append(live)
            stage += 1
    out["logits"] = _logits(sd, x, cfg)
    return out


def model_soft(sd, images, cfg, locs, theta, tau, eps=1e-6, dtype=torch.float64, binarise=False):
    """The soft forward: nothing is removed, the mask m acts on the token as a key of every later block through the policy softmax.
    theta: S 0-d tensors (differentiated through) or numbers.  binarise: every M replaced by [s >= theta] (with eps = 0 this is the hard
    forward).  -> dict: logits, M (per stage), m (per stage, the policy BEFORE the stage), scores, reg (R)"""
    from oracle import d2s_oracle as O
    x = O.embed_tokens(sd, images.to(dtype), cfg)
    B, N, _ = x.shape
    H = cfg["heads"]
    m = torch.ones((B, N), dtype=dtype)
    out = dict(M=[], m=[], scores=[])
    stage, reg = 0, 0.0
    eye = torch.eye(N, dtype=dtype)

    def policy_probs(S, m, first):
        if first:
            return S.softmax(dim=-1)
        mk = m[:, None, None, :] * (1.0 - eye) + eye
        e = torch.exp(S - S.max(dim=-1, keepdim=True).values.detach()) * mk
        return (e + eps / N) / (e.sum(dim=-1, keepdim=True) + eps)

    for l in range(cfg["depth"]):
        pol, first = m, stage == 0
        x, P = _block(sd, l, x, cfg, lambda S: policy_probs(S, pol, first))
        if stage < len(locs) and l == locs[stage]:
            s = ((P * m[:, None, :, None]).sum(dim=(1, 2)) / (H * m.sum(dim=1, keepdim=True))).detach()      # the score carries no gradient
            th = theta[stage]
            M = (s >= th).to(dtype) if binarise else torch.sigmoid((s - th) / tau)
            M = torch.cat((torch.ones_like(M[:, :1]), M[:, 1:]), dim=1)
            out["M"].append(M), out["m"].append(m), out["scores"].append(s)
            reg = reg + M[:, 1:].sum()
            m = m * M
            stage += 1
    out["logits"] = _logits(sd, x, cfg)
    out["reg"] = reg / (len(locs) * B * (N - 1))
    return out


def model_deleted(sd, image, cfg, locs, theta, dtype=torch.float64):
    """ONE image [1, 3, S, S] with its pruned tokens physically deleted (no mask anywhere) -> (logits [1, C], ids kept per stage)"""
    from oracle import d2s_oracle as O
    x = O.embed_tokens(sd, image.to(dtype), cfg)
    ids = torch.arange(x.shape[1])
    kept, stage = [], 0
    for l in range(cfg["depth"]):
        x, P = _block(sd, l, x, cfg, lambda S: S.softmax(dim=-1))
        if stage < len(locs) and l == locs[stage]:
            s = P[0].mean(dim=(0, 1))
            keep = s >= torch.tensor(float(theta[stage]), dtype=dtype)
            keep[0] = True
            x, ids = x[:, keep], ids[keep]
            kept.append(ids)
            stage += 1
    return _logits(sd, x, cfg), kept


def objective(logits, labels, reg, lam):
    """CE + lambda * R (no teacher: --dist-weight 0)"""
    import torch.nn.functional as F
    return F.cross_entropy(logits, labels) + lam * reg
