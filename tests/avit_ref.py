"""CPU restatement of the A-ViT baseline (the build's own definition, PARITY UNPINNED), written the DENSE MASKED
way - a full [B, N, D] batch in every block, -inf on halted keys - so that it shares nothing with the ragged implementation: the model
and the objective in fp32 or float64 with gradients from autograd (the halting layers are integers, detached by construction), the
closed-form gradient of a halting score, and the halting step of one block on a packed batch as plain loops.  No GPU."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O


def target(L, target_depth, dtype=torch.float64):
    t = torch.exp(-0.5 * (torch.arange(L, dtype=torch.float64) - float(target_depth)) ** 2)
    return (t / t.sum()).to(dtype)


def _block(sd, i, x, cfg, keymask):
    """Block i on x [B, n, D]; keymask [B, n] bool: the keys every query may attend to"""
    p = f"blocks.{i}."
    B, n, D = x.shape
    H, eps = cfg["heads"], cfg["ln_eps"]
    dh = D // H
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, n, 3, H, dh).permute(2, 0, 3, 1, 4)
    a = (qkv[0] @ qkv[1].transpose(-2, -1)) * (dh ** -0.5)
    a = a.masked_fill(~keymask[:, None, None, :], float("-inf")).softmax(dim=-1)
    o = (a @ qkv[2]).transpose(1, 2).reshape(B, n, D)
    x = x + F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    return x + O.mlp(sd, p + "mlp.", F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps))


def forward(sd, images, cfg, gamma, beta, eps_halt, dtype=torch.float64, n_forced=None):
    """sd: {name: tensor} (tensors that require grad are differentiated through).  n_forced [B, N]: halting layers to replay instead of
    deciding by the threshold (the bf16 arithmetic mode's own decisions; the margin is then not taken).
    -> dict: logits [B, C], acc [B, D], n [B, N] int64, R [B, N], h / live / ycls per layer, margin (the smallest |c_l - (1 - eps)| over
    the live tokens of every layer)"""
    x = O.embed_tokens(sd, images.to(dtype), cfg)
    B, N, D = x.shape
    L = cfg["depth"]
    thr = torch.tensor(1.0, dtype=dtype) - torch.tensor(float(eps_halt), dtype=dtype)
    c = torch.zeros((B, N), dtype=dtype)
    R = torch.zeros((B, N), dtype=dtype)
    n = torch.zeros((B, N), dtype=torch.int64)
    live = torch.ones((B, N), dtype=torch.bool)
    acc = torch.zeros((B, D), dtype=dtype)
    hs, lives, ycls = [], [], []
    margin = math.inf
    cls_col = torch.zeros((B, N), dtype=torch.bool)
    cls_col[:, 0] = True
    for l in range(1, L + 1):
        x = _block(sd, l - 1, x, cfg, live | cls_col)           # a finished image keeps its CLS key so that no row is all -inf
        h = torch.sigmoid(gamma * x[:, :, 0] - beta)
        c_new = c + h
        if bool(live.any()):
            margin = min(margin, float((c_new.detach() - thr).abs()[live].min()))
        if n_forced is not None:
            halt = live & (n_forced == l)
        else:
            halt = live & ((c_new.detach() > thr) | (l == L))
            halt = live & (halt | halt[:, :1])                  # the CLS token takes its image's live tokens with it
        R = torch.where(halt, 1.0 - c, R)
        n = torch.where(halt, torch.full_like(n, l), n)
        w = torch.where(halt[:, 0], 1.0 - c[:, 0], h[:, 0]) * live[:, 0].to(dtype)
        acc = acc + w[:, None] * x[:, 0, :]
        hs.append(h)
        lives.append(live)
        ycls.append(x[:, 0, :])
        c = torch.where(live, c_new, c)
        live = live & ~halt
    xn = F.layer_norm(acc, (D,), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    logits = F.linear(xn, sd["head.weight"], sd["head.bias"])
    return dict(logits=logits, acc=acc, n=n, R=R, h=hs, live=lives, ycls=ycls, margin=margin)


def forward_deleted(sd, image, cfg, gamma, beta, eps_halt, dtype=torch.float64):
    """ONE image [1, 3, S, S] with its halted tokens physically deleted after every block (no mask anywhere) -> (logits [1, C], n [N])"""
    x = O.embed_tokens(sd, image.to(dtype), cfg)
    N, D = x.shape[1], x.shape[2]
    L = cfg["depth"]
    thr = torch.tensor(1.0, dtype=dtype) - torch.tensor(float(eps_halt), dtype=dtype)
    ids = torch.arange(N)
    c = torch.zeros(N, dtype=dtype)
    n = torch.zeros(N, dtype=torch.int64)
    acc = torch.zeros((1, D), dtype=dtype)
    for l in range(1, L + 1):
        x = _block(sd, l - 1, x, cfg, torch.ones((1, x.shape[1]), dtype=torch.bool))
        h = torch.sigmoid(gamma * x[0, :, 0] - beta)
        c_new = c[ids] + h
        halt = (c_new > thr) | (l == L)
        halt = halt | halt[0]
        acc = acc + (1.0 - c[0] if bool(halt[0]) else h[0]) * x[:, 0, :]
        n[ids[halt]] = l
        c[ids] = c_new
        if bool(halt[0]):
            break
        x, ids = x[:, ~halt], ids[~halt]
    xn = F.layer_norm(acc, (D,), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return F.linear(xn, sd["head.weight"], sd["head.bias"]), n


def hbar(out):
    """[L]: the mean halting score over the rows live at every layer, 0 where nothing is live"""
    v = []
    for h, live in zip(out["h"], out["live"]):
        k = live.sum()
        v.append((h * live.to(h.dtype)).sum() / k if int(k) > 0 else torch.zeros((), dtype=h.dtype))
    return torch.stack(v)


def prior(hb, tgt):
    """P = sum_l tgt_l (log tgt_l - log p_l) / L, p = clamp(Hbar / sum Hbar, 0.01, 0.99)"""
    p = torch.clamp(hb / hb.sum(), 0.01, 0.99)
    return (tgt * (tgt.log() - p.log())).sum() / hb.numel()


def ponder(out):
    return (out["n"].to(out["R"].dtype) + out["R"]).mean()


def objective(out, labels, logits_t=None, cls_weight=1.0, dist_weight=0.5, ponder_scale=5e-4, prior_alpha=0.01, target_depth=7.0):
    """-> (loss, dict of the terms)"""
    logits = out["logits"]
    ce = F.cross_entropy(logits, labels)
    loss = cls_weight * ce
    kl = torch.zeros((), dtype=logits.dtype)
    if logits_t is not None and dist_weight != 0.0:
        kl = F.kl_div(F.log_softmax(logits, dim=-1), F.log_softmax(logits_t.to(logits.dtype), dim=-1), reduction="batchmean", log_target=True)
        loss = loss + dist_weight * kl
    pn = ponder(out)
    P = prior(hbar(out), target(len(out["h"]), target_depth, logits.dtype))
    loss = loss + ponder_scale * pn + prior_alpha * P
    return loss, dict(ce=ce, kl=kl, ponder=pn, prior=P)


def prior_grad_closed_form(hb, tgt):
    """dP/dHbar_k = a_k / S - (sum_l a_l Hbar_l) / S^2, a_l = -tgt_l / (L p_l) inside the clamp's range and 0 outside"""
    S = hb.sum()
    q = hb / S
    a = torch.where((q >= 0.01) & (q <= 0.99), -tgt / (hb.numel() * q), torch.zeros_like(q))
    return a / S - (a * hb).sum() / (S * S)


def gh_closed_form(out, dacc, ponder_scale, prior_alpha, target_depth):
    """The closed-form gradient of the loss in h_l[b, t] for the rows live at l (0 elsewhere), per layer [B, N]"""
    B, N = out["n"].shape
    L = len(out["h"])
    hb = hbar(out).detach()
    dP = prior_grad_closed_form(hb, target(L, target_depth, hb.dtype))
    n = out["n"]
    nc = n[:, 0]
    ysave = torch.stack([out["ycls"][int(nc[b]) - 1][b] for b in range(B)]).detach()
    s_n = (dacc * ysave).sum(-1)
    res = []
    for l in range(1, L + 1):
        live = out["live"][l - 1]
        lt = (n > l).to(dacc.dtype)
        g = -ponder_scale / (B * N) * lt
        g[:, 0] = g[:, 0] + lt[:, 0] * ((dacc * out["ycls"][l - 1].detach()).sum(-1) - s_n)
        k = int(live.sum())
        if k > 0:
            g = g + prior_alpha * dP[l - 1] / k
        res.append(g * live.to(dacc.dtype))
    return res


# ---- the halting step of one block on a packed batch, as plain loops (float64 sums; the decisions from the values given) ----
def halt_step(y, cu, row_src, st, layer, last, gamma, beta, eps_halt):
    """y [total, D] float64 numpy; st: dict of numpy arrays c, R [B, N] float64, nh [B, N] int, acc, ysave [B, D] float64, updated in
    place.  -> dict keep [total], counts [B], w [B], h [total], ycls [B, D], part [B, 3], margin, abs (per-output sums of |summands| for
    the error bounds: acc [B, D], part [B, 3])"""
    y = np.asarray(y, dtype=np.float64)
    total, D = y.shape
    B, N = st["c"].shape
    thr = 1.0 - eps_halt
    keep, h = np.zeros(total), np.zeros(total)
    counts, w, part = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros((B, 3))
    ycls = np.zeros((B, D))
    abs_acc, abs_part = np.abs(st["acc"]).copy(), np.zeros((B, 3))
    margin = math.inf
    for b in range(B):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        if r1 <= r0:
            continue
        keep[r0] = 1.0
        ycls[b] = y[r0]
        if st["nh"][b, 0] != 0:
            continue                                    # a finished image: a dead row
        cls_halt = False
        for r in range(r0, r1):
            t = int(row_src[r])
            hv = 1.0 / (1.0 + math.exp(-(gamma * y[r, 0] - beta)))
            c0 = st["c"][b, t]
            c1 = c0 + hv
            margin = min(margin, abs(c1 - thr))
            halts = bool(last) or c1 > thr or cls_halt
            if r == r0:
                cls_halt = halts
                w[b] = (1.0 - c0) if halts else hv
            st["c"][b, t] = c1
            h[r] = hv
            part[b, 0] += hv
            abs_part[b, 0] += hv
            part[b, 1] += 1
            if halts:
                st["nh"][b, t] = layer
                st["R"][b, t] = 1.0 - c0
                part[b, 2] += layer + (1.0 - c0)
                abs_part[b, 2] += layer + abs(1.0 - c0)
            elif r > r0:
                keep[r] = 1.0
                counts[b] += 1
        st["acc"][b] += w[b] * y[r0]
        abs_acc[b] += np.abs(w[b] * y[r0])
        if cls_halt:
            st["ysave"][b] = y[r0]
    return dict(keep=keep, counts=counts, w=w, h=h, ycls=ycls, part=part, margin=margin, abs_acc=abs_acc, abs_part=abs_part)


def repack(y, row_src, keep, cu):
    """numpy re-pack: -> (y', row_src', cu')"""
    rows, cu_new = [], [0]
    for b in range(len(cu) - 1):
        here = [r for r in range(int(cu[b]), int(cu[b + 1])) if r == int(cu[b]) or keep[r] != 0]
        rows += here
        cu_new.append(cu_new[-1] + len(here))
    rows = np.asarray(rows, dtype=np.int64)
    return y[rows], row_src[rows], np.asarray(cu_new, dtype=np.int32)


def halt_step_bwd(g, h, cu, row_src, nh, w, dacc, ycls, ysave, gsc, layer, gamma):
    """float64 numpy: g [total, D] (the arriving gradient, or zeros) -> (g + the step's own terms, the per-element sums of |summands|)"""
    g = np.array(g, dtype=np.float64)
    ab = np.abs(g)
    L = len(gsc) - 1
    for b in range(len(cu) - 1):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        if r1 <= r0 or nh[b, 0] < layer:
            continue
        s_l, s_n = float(dacc[b] @ ycls[b]), float(dacc[b] @ ysave[b])
        s_abs = float(np.abs(dacc[b] * ycls[b]).sum() + np.abs(dacc[b] * ysave[b]).sum())
        for r in range(r0, r1):
            t = int(row_src[r])
            lt = nh[b, t] > layer
            gh = ((s_l - s_n if t == 0 else 0.0) - gsc[L] if lt else 0.0) + gsc[layer - 1]
            gh_abs = ((s_abs if t == 0 else 0.0) + abs(gsc[L]) if lt else 0.0) + abs(gsc[layer - 1])
            f = gamma * h[r] * (1.0 - h[r])
            g[r, 0] += gh * f
            ab[r, 0] += gh_abs * abs(f)
        g[r0] += w[b] * dacc[b]
        ab[r0] += np.abs(w[b] * dacc[b])
    return g, ab
