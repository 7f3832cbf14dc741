"""Float64 restatement of graph ranking (DESIGN.md section 29 - the build's own definition): T steps of the unnormalised PageRank iteration
over the attention graph of one block, per image and head, on dense [n, n] matrices - nothing here shares code with the kernel or with
tests/ltp_ref.py - and the attention-selecting student that ranks by it, on the oracle's blocks."""
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O
from tests import attnsel_ref


def probabilities(qkv, B, n, H, scale):
    """qkv [B * n, 3, H, 64] float64 -> P [B, H, n, n], P[b, h, i, j] = exp(scale q_i . k_j - lse_i): every row sums to 1"""
    qkv = qkv.double().reshape(B, n, 3, H, 64)
    q, k = qkv[:, :, 0].permute(0, 2, 1, 3), qkv[:, :, 1].permute(0, 2, 1, 3)          # [B, H, n, 64]
    S = torch.matmul(q, k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, dim=-1, keepdim=True)
    return torch.exp(S - lse)


def iterate(P, iters, w0=None, trace=False):
    """P [B, H, n, n] -> s^iters [B, H, n] with s^0 = w0 or 1 / n and s^{t+1}_j = sum_i s^t_i P_ij; trace: the list s^1 .. s^iters"""
    B, H, n, _ = P.shape
    s = torch.full((B, H, n), 1.0 / n, dtype=torch.float64) if w0 is None else w0.double().reshape(B, H, n)
    steps = []
    for _ in range(int(iters)):
        s = torch.einsum("bhi,bhij->bhj", s, P)
        steps.append(s)
    return steps if trace else s


def rank(qkv, B, n, H, scale, iters, w0=None):
    return iterate(probabilities(qkv, B, n, H, scale), iters, w0)


def kth_gap(probs, k):
    """per image: the k-th largest probability minus the (k + 1)-th (k < T)"""
    v = torch.sort(probs, dim=1, descending=True)[0]
    return v[:, k - 1] - v[:, k]


def block_qkv(sd, i, x, cfg):
    """The qkv [B * n, 3, H, 64] block i computes from its input x [B, n, D]: LayerNorm 1 and the qkv projection, in x's precision"""
    p = f"blocks.{i}."
    D = cfg["dim"]
    ln = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], cfg["ln_eps"])
    qkv = F.linear(ln, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    return qkv.reshape(x.shape[0] * x.shape[1], 3, cfg["heads"], D // cfg["heads"])


def block_rank(sd, i, x, cfg, iters):
    """-> rank [B, H, n] float64 of block i's tokens from its input x"""
    B, n, D = x.shape
    return rank(block_qkv(sd, i, x.double(), cfg), B, n, cfg["heads"], (D // cfg["heads"]) ** -0.5, iters)


def model_forward(sd, images, cfg, iters, mean_heads=False):
    """The attention-selecting student without token fusion in float64 (the oracle's blocks): a stage at block i keeps by the rank of
    block i - 1 (iters > 0) or by that block's CLS row (iters == 0).
    -> dict(logits, ranks [per stage, B x H x n], probs, kept, dropped [per stage], inputs [the input of the block before each stage])"""
    sd = {k: v.double() for k, v in sd.items()}
    x = O.embed_tokens(sd, images.double(), cfg)
    out = dict(ranks=[], probs=[], kept=[], dropped=[], inputs=[])
    stage, row = 0, None
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            k = int(cfg["init_n"] * cfg["token_ratio"][stage])
            probs, kept, dropped = attnsel_ref.select(row, 1, x.shape[1] - 1, k, mean_heads)
            out["probs"].append(probs), out["kept"].append(kept), out["dropped"].append(dropped)
            x = O.gather_pack(x, kept)
            stage += 1
        if (i + 1) in cfg["pruning_loc"]:
            out["inputs"].append(x)
            if iters > 0:
                row = block_rank(sd, i, x, cfg, iters)
                out["ranks"].append(row)
        x, cls_row = O.block(sd, i, x, cfg)
        if iters == 0:
            row = cls_row
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    out["logits"] = F.linear(x[:, 0], sd["head.weight"], sd["head.bias"])
    return out
