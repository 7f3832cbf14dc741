"""Float64 restatement of the similarity stage after attention ranking (--sim-prune R; DESIGN.md section 30 - the build's own definition):
plain loops over one image at a time, nothing shared with the kernels, and the attention-selecting student that uses it, on the oracle's
blocks.

A comparison with NaN is false, as on the device: a NaN score never replaces the running best, so a zero key row is never a partner and
as a source keeps best = -inf with the lowest id of group B as its partner."""
import math

import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O
from tests import attnsel_ref
from tests import graph_rank_ref


def clip_r(R, k, T):
    return max(0, min(int(R), int(k), int(T) - int(k)))


def key_metric(qkv, B, n, H):
    """qkv [B * n, 3, H, 64] -> metric [B, n, 64] in qkv's precision (float64 when given float64): the mean of the keys over the heads,
    h ascending, divided by its L2 norm; a zero row gives NaN"""
    k = torch.as_tensor(qkv).reshape(B, n, 3, H, 64)[:, :, 1]
    m = k[:, :, 0].clone()
    for h in range(1, H):
        m = m + k[:, :, h]
    m = m / H
    return m / torch.sqrt((m * m).sum(dim=-1, keepdim=True))


def partition(probs, cand):
    """one image: probs [T], cand ascending ids -> (A ids ascending, B ids ascending): B the c - c // 2 most important candidates (probs
    descending, equal values lowest id first), A the others"""
    order = sorted((int(t) for t in cand), key=lambda t: (-float(probs[t]), t))
    c_b = len(order) - len(order) // 2
    return sorted(order[c_b:]), sorted(order[:c_b])


def match(metric, a_ids, b_ids):
    """one image: metric [T, 64] float64 rows of the scored tokens -> (best, second, partner) per A row; second is the largest score below
    best (for the gap checks; -inf when there is none)"""
    best, second, partner = [], [], []
    mb = metric[b_ids]
    for a in a_ids:
        v, v2, arg = -math.inf, -math.inf, b_ids[0]
        for b, s in zip(b_ids, (mb * metric[a]).sum(dim=-1).tolist()):      # score[a][b] = sum_d m_a[d] m_b[d], b ascending
            if s > v:
                v2, v, arg = v, s, b
            elif s > v2:
                v2 = s
        best.append(v), second.append(v2), partner.append(arg)
    return best, second, partner


def stage(metric, probs, cand, lead, r):
    """metric [B, n, 64], probs [B, T], cand [B, c] -> dict(kept [B, c - r], dropped [B, T - c + r], pruned / partner [B, r] int64,
    sim [B, r] float64, and per image the lists a_ids, b_ids, best, second)"""
    metric, probs = torch.as_tensor(metric).double(), torch.as_tensor(probs).double()
    cand = torch.as_tensor(cand)
    B, T = probs.shape
    out = dict(kept=[], dropped=[], pruned=[], partner=[], sim=[], a_ids=[], b_ids=[], best=[], second=[])
    for b in range(B):
        ids = [int(t) for t in cand[b]]
        a_ids, b_ids = partition(probs[b], ids)
        best, second, part = match(metric[b, lead:lead + T], a_ids, b_ids) if r > 0 else ([], [], [])
        chosen = sorted(sorted(range(len(best)), key=lambda p: (-best[p], a_ids[p]))[:r])      # positions in A, ascending = ids ascending
        gone = {a_ids[p] for p in chosen}
        kept = [t for t in ids if t not in gone]
        out["kept"].append(kept), out["dropped"].append([t for t in range(T) if t not in set(kept)])
        out["pruned"].append([a_ids[p] for p in chosen]), out["partner"].append([part[p] for p in chosen])
        out["sim"].append([best[p] for p in chosen])
        out["a_ids"].append(a_ids), out["b_ids"].append(b_ids), out["best"].append(best), out["second"].append(second)
    c = cand.shape[1]
    for key, width in (("kept", c - r), ("dropped", T - c + r), ("pruned", r), ("partner", r)):
        out[key] = torch.tensor(out[key], dtype=torch.int64).reshape(B, width)
    out["sim"] = torch.tensor(out["sim"], dtype=torch.float64).reshape(B, r)
    return out


def model_forward(sd, images, cfg, R, iters=0, mean_heads=False):
    """The attention-selecting student without token fusion in float64 (the oracle's blocks): a stage at block i takes k + r candidates by
    the CLS row of block i - 1 (iters == 0) or its graph rank, and prunes r of them by the key metric of that block (R > 0).
    -> dict(logits, probs, cand, r, stages [stage()'s dict, or None when r == 0], kept, dropped, metrics, inputs [the input of the block
    before each stage])"""
    sd = {k: v.double() for k, v in sd.items()}
    x = O.embed_tokens(sd, images.double(), cfg)
    out = dict(probs=[], cand=[], r=[], stages=[], kept=[], dropped=[], metrics=[], inputs=[])
    s, row, metric = 0, None, None
    H = cfg["heads"]
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            k, T = int(cfg["init_n"] * cfg["token_ratio"][s]), x.shape[1] - 1
            r = clip_r(R, k, T)
            probs, cand, dropped = attnsel_ref.select(row, 1, T, k + r, mean_heads)
            st, kept = None, cand
            if r > 0:
                st = stage(metric, probs, cand, 1, r)
                kept, dropped = st["kept"], st["dropped"]
            out["probs"].append(probs), out["cand"].append(cand), out["r"].append(r), out["stages"].append(st)
            out["kept"].append(kept), out["dropped"].append(dropped)
            x = O.gather_pack(x, kept)
            s += 1
        if (i + 1) in cfg["pruning_loc"]:
            out["inputs"].append(x)
            B, n, _ = x.shape
            qkv = graph_rank_ref.block_qkv(sd, i, x, cfg)
            metric = key_metric(qkv, B, n, H)
            out["metrics"].append(metric)
            if iters > 0:
                row = graph_rank_ref.rank(qkv, B, n, H, (cfg["dim"] // H) ** -0.5, iters)
        x, cls_row = O.block(sd, i, x, cfg)
        if iters == 0:
            row = cls_row
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    out["logits"] = F.linear(x[:, 0], sd["head.weight"], sd["head.bias"])
    return out
