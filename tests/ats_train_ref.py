"""CPU restatement of training through adaptive token sampling ("Training through the stages"): the varlen
attention and its gradient per image in float64 autograd, the closed-form backward of the re-pack and of the CLS gather (and their
index-based numpy statements), and the model per image, dense, in float64 autograd with the kept sets replayed - the selection is a
constant, a dropped token is reached only as a key and a value of the stage's own attention.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O
from tests import ats_ref as R


# ---- attention on a packed batch ----
def attention(qkv, scale):
    """qkv [n, 3, H, 64] of ONE image, any float dtype -> (out [n, H * 64], lse [H, n])"""
    n, _, H, dh = qkv.shape
    q, k, v = (qkv[:, i].transpose(0, 1) for i in range(3))          # [H, n, dh]
    S = (q @ k.transpose(-1, -2)) * scale
    return (torch.softmax(S, dim=-1) @ v).transpose(0, 1).reshape(n, H * dh), torch.logsumexp(S, dim=-1)


def varlen_attention(qkv, cu, H, scale):
    """qkv [total, 3 * H * 64] packed, cu [B+1] -> float64 (out [total, H * 64], lse [H, total], cls_row [H, total]), every image alone"""
    total = qkv.shape[0]
    out = torch.zeros((total, H * 64), dtype=torch.float64)
    lse = torch.zeros((H, total), dtype=torch.float64)
    cls_row = torch.zeros((H, total), dtype=torch.float64)
    cu = [int(c) for c in cu]
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        q = qkv[lo:hi].double().reshape(hi - lo, 3, H, 64)
        out[lo:hi], lse[:, lo:hi] = attention(q, scale)
        S0 = torch.einsum("hd,jhd->hj", q[0, 0], q[:, 1]) * scale
        cls_row[:, lo:hi] = torch.softmax(S0, dim=-1)
    return out, lse, cls_row


def varlen_attention_grad(qkv, cu, H, scale, dout):
    """d/dqkv of sum(varlen_attention(qkv)[0] * dout), float64 autograd, every image alone -> [total, 3 * H * 64]"""
    dq = torch.zeros(qkv.shape, dtype=torch.float64)
    cu = [int(c) for c in cu]
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        q = qkv[lo:hi].double().reshape(hi - lo, 3, H, 64).clone().requires_grad_(True)
        out, _ = attention(q, scale)
        out.backward(dout[lo:hi].double())
        dq[lo:hi] = q.grad.reshape(hi - lo, 3 * H * 64)
    return dq


# ---- the two row moves ----
def repack(x, keep, cu_old):
    """ragged_repack as plain indexing (differentiable in x): -> (out, cu_new, the old row of every new row)"""
    cu_old = [int(c) for c in cu_old]
    rows = []
    cu_new = [0]
    for b in range(len(cu_old) - 1):
        lo, hi = cu_old[b], cu_old[b + 1]
        here = [lo + i for i in range(hi - lo) if i == 0 or float(keep[lo + i]) != 0.0]
        rows += here
        cu_new.append(cu_new[-1] + len(here))
    idx = torch.tensor(rows, dtype=torch.long)
    return x[idx], cu_new, idx


def repack_backward(g_new, keep, cu_old, cu_new):
    """The closed form: row cu_old[b] + i of the result is row cu_new[b] + (number of kept rows of the image before i) of g_new when
    i == 0 or keep != 0, zeros otherwise.  numpy, the dtype of g_new."""
    g_new, keep = np.asarray(g_new), np.asarray(keep)
    cu_old, cu_new = [int(c) for c in cu_old], [int(c) for c in cu_new]
    g_old = np.zeros((cu_old[-1], g_new.shape[1]), dtype=g_new.dtype)
    for b in range(len(cu_old) - 1):
        j = cu_new[b]
        for i in range(cu_old[b + 1] - cu_old[b]):
            if i == 0 or keep[cu_old[b] + i] != 0:
                g_old[cu_old[b] + i] = g_new[j]
                j += 1
        assert j == cu_new[b + 1], "cu_new was not built from these flags"
    return g_old


def cls_scatter(g_cls, cu, total):
    """The backward of x[cu[:-1]]: row cu[b] = g_cls[b], zeros elsewhere.  numpy, the dtype of g_cls."""
    g_cls = np.asarray(g_cls)
    g = np.zeros((total, g_cls.shape[1]), dtype=g_cls.dtype)
    for b in range(g_cls.shape[0]):
        g[int(cu[b])] = g_cls[b]
    return g


# ---- the model ----
def model_grads(state_dict, images, cfg, locs, kept_ids_per_stage, logit_weight=None, loss_of=None):
    """ats_ref.model_forward with the kept sets replayed, under float64 autograd: every image alone, dense; at a stage the attention half
    runs on every token the image still has, only the kept rows go on.  The scalar that is differentiated is loss_of(logits) if given,
    else sum(logits * logit_weight), else sum(logits).  -> (logits [B, C], the scalar, {name: gradient or None})"""
    sd = {k: torch.as_tensor(v).detach().double().clone().requires_grad_(True) for k, v in state_dict.items()}
    locs = list(locs)
    x = O.embed_tokens(sd, images.double(), cfg)
    logits = []
    for b in range(x.shape[0]):
        xb = x[b:b + 1]
        ids = torch.arange(xb.shape[1])
        for i in range(cfg["depth"]):
            if i not in locs:
                xb, _ = O.block(sd, i, xb, cfg)
                continue
            x1, _, _ = R._block_halves(sd, i, xb, cfg)
            new = torch.as_tensor(kept_ids_per_stage[locs.index(i)][b]).long()
            pos = torch.searchsorted(ids, new)
            assert int(new[0]) == 0 and torch.equal(ids[pos], new), "a replayed set holds CLS and only tokens that are still there"
            ids = new
            xb = R._mlp_half(sd, i, x1[:, pos], cfg)
        xb = F.layer_norm(xb[:, 0], (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
        logits.append(F.linear(xb, sd["head.weight"], sd["head.bias"]))
    logits = torch.cat(logits, dim=0)
    if loss_of is not None:
        scalar = loss_of(logits)
    elif logit_weight is not None:
        scalar = (logits * torch.as_tensor(logit_weight).double()).sum()
    else:
        scalar = logits.sum()
    names = list(sd)
    grads = torch.autograd.grad(scalar, [sd[k] for k in names], allow_unused=True)
    return logits.detach(), scalar.detach(), dict(zip(names, grads))
