"""CPU restatement of adaptive token sampling (the build's own definition, PARITY UNPINNED): the scores in float64,
the selection as the fp32 procedure operation for operation, and the model per image, dense, in float64, built from the oracle's own
embed_tokens and the arithmetic of its block.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O


def scores(cls_row, v, cu):
    """cls_row [H, total], v [total, H * 64] (what the kernel reads, already widened), cu [B+1] -> float64 [total]: per image
    a_j * ||v_j|| / sum over the image's non-CLS rows, 1 / T where that sum is not > 0 or not finite; 0 at the CLS rows."""
    a = np.asarray(cls_row, dtype=np.float64).sum(axis=0)
    nrm = np.sqrt((np.asarray(v, dtype=np.float64) ** 2).sum(axis=1))
    w = a * nrm
    out = np.zeros(w.shape[0], dtype=np.float64)
    cu = [int(c) for c in cu]
    for b in range(len(cu) - 1):
        lo, hi = cu[b] + 1, cu[b + 1]
        if hi <= lo:
            continue
        tot = w[lo:hi].sum()
        out[lo:hi] = w[lo:hi] / tot if (tot > 0 and np.isfinite(tot)) else 1.0 / (hi - lo)
    return out


def select(score_f32, K):
    """The selection on fp32 scores [T] -> keep [T] bool.  Stable ascending order, the running sum sequentially in fp32, K thresholds
    u_k * c_{T-1} with u_k = (float)(2k+1) / (float)(2K), for each the first position whose running sum reaches it; the picked set."""
    s = np.asarray(score_f32)
    assert s.dtype == np.float32 and s.ndim == 1 and K >= 1
    T = s.shape[0]
    keep = np.zeros(T, dtype=bool)
    if T == 0:
        return keep
    order = np.argsort(s, kind="stable")
    c = np.empty(T, dtype=np.float32)
    run = np.float32(0.0)
    for i in range(T):
        run = np.float32(run + s[order[i]])
        c[i] = run
    u = (2 * np.arange(K) + 1).astype(np.float32) / np.float32(2 * K)
    t = (u * c[-1]).astype(np.float32)
    reach = c[None, :] >= t[:, None]
    assert bool(reach[:, -1].all()), "the last position always qualifies"
    keep[order[np.argmax(reach, axis=1)]] = True
    return keep


def _block_halves(sd, i, x, cfg):
    """The attention half of block i on x [1, n, D] -> (x1 [1, n, D], CLS softmax rows [H, n], V [n, H * dh])"""
    p = f"blocks.{i}."
    D, eps, H = cfg["dim"], cfg["ln_eps"], cfg["heads"]
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    y, cls_row = O.attention(sd, p + "attn.", h, H)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    return x + y, cls_row[0], qkv[0, :, 2 * D:]


def _mlp_half(sd, i, x1, cfg):
    p = f"blocks.{i}."
    D, eps = cfg["dim"], cfg["ln_eps"]
    return x1 + O.mlp(sd, p + "mlp.", F.layer_norm(x1, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps))


def model_forward(sd, images, cfg, locs, kept_ids_per_stage=None, tokens=None):
    """Every image alone, dense, float64.  locs: the blocks that hold a stage.  kept_ids_per_stage[s][b]: the ORIGINAL token indices
    (int64, ascending, 0 = CLS first) that leave stage s of image b, replayed; None: the stage selects by its own float64 scores rounded
    to fp32, with at most tokens[s] tokens.  -> (logits [B, C] float64, the kept ids per stage per image as used)"""
    sd = {k: v.detach().double() for k, v in sd.items()}
    locs = list(locs)
    with torch.no_grad():
        x = O.embed_tokens(sd, images.double(), cfg)
        B = x.shape[0]
        used = [[] for _ in locs]
        logits = []
        for b in range(B):
            xb = x[b:b + 1]
            ids = torch.arange(xb.shape[1])
            for i in range(cfg["depth"]):
                if i not in locs:
                    xb, _ = O.block(sd, i, xb, cfg)
                    continue
                s = locs.index(i)
                x1, cls_row, v = _block_halves(sd, i, xb, cfg)
                if kept_ids_per_stage is not None:
                    new = torch.as_tensor(kept_ids_per_stage[s][b]).long()
                    pos = torch.searchsorted(ids, new)
                    assert int(new[0]) == 0 and torch.equal(ids[pos], new), "a replayed set holds CLS and only tokens that are still there"
                else:
                    sc = scores(cls_row.numpy(), v.numpy(), [0, xb.shape[1]])[1:].astype(np.float32)
                    keep = select(sc, int(tokens[s]))
                    pos = torch.cat((torch.zeros(1, dtype=torch.long), torch.nonzero(torch.from_numpy(keep)).flatten() + 1))
                    new = ids[pos]
                used[s].append(new)
                ids = new
                xb = _mlp_half(sd, i, x1[:, pos], cfg)
            xb = F.layer_norm(xb, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
            logits.append(F.linear(xb[:, 0], sd["head.weight"], sd["head.bias"]))
        return torch.cat(logits, dim=0), used
