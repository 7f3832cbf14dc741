"""Token selection by the student's own CLS attention (attn_selection), restated in float64.  This is the definition (DESIGN.md section
21), the build's own: the reference names the branch (vit_models/dynamic_vit.py:265) and never connects it.

A stage receives the CLS softmax row cls_row [B, H, n] of the block before it.  Its T scored tokens are columns lead .. lead + T - 1
(lead = 1 skips the CLS column; trailing columns beyond lead + T belong to package tokens and are not scored).

    w[b, t]     = max_h cls_row[b, h, lead + t]            or the mean over h (mean_heads)
    probs[b, t] = w[b, t] / sum_t w[b, t]
    kept        = the ids of the k largest probs, equal values lowest index first, ascending;  dropped = the others, ascending
"""
import numpy as np
import torch


def reduce_heads(cls_row, lead, T, mean_heads=False):
    """-> w [B, T] float64"""
    a = torch.as_tensor(cls_row).double()[:, :, lead:lead + T]
    return a.mean(dim=1) if mean_heads else a.max(dim=1)[0]


def renormalise(w):
    return w / w.sum(dim=1, keepdim=True)


def stable_topk(p, k):
    """(kept [B, k], dropped [B, T - k]) int64: value descending, index ascending among equal values, each list sorted ascending"""
    p = torch.as_tensor(p)
    order = torch.argsort(p, dim=1, descending=True, stable=True)
    return torch.sort(order[:, :k], dim=1)[0].contiguous(), torch.sort(order[:, k:], dim=1)[0].contiguous()


def select(cls_row, lead, T, k, mean_heads=False):
    """-> (probs float64 [B, T], kept, dropped)"""
    probs = renormalise(reduce_heads(cls_row, lead, T, mean_heads))
    return (probs,) + stable_topk(probs, k)


def stage_loop(cls_rows, pruning_loc, ks, mean_heads=False, carried=None):
    """The model's stage loop over the per-block rows of ONE forward.  cls_rows[i]: block i's row WITHOUT its CLS column, [B, H, n_i - 1]
    (model.cls_attns).  The stage at block i reads cls_rows[i - 1]; carried[s] trailing columns (package rows under fuse_dropped) are not
    scored.  -> [(probs, kept, dropped)] per stage"""
    out = []
    for s, (loc, k) in enumerate(zip(pruning_loc, ks)):
        row = torch.as_tensor(cls_rows[loc - 1])
        c = 0 if carried is None else int(carried[s])
        out.append(select(row, 0, row.shape[-1] - c, k, mean_heads))
    return out


def mask_agreement(ids_a, ids_b, T):
    """fraction of the B * T token slots on which the two kept-id sets agree (losses.py:96 on 0/1 masks)"""
    ids_a, ids_b = torch.as_tensor(ids_a), torch.as_tensor(ids_b)
    B = ids_a.shape[0]
    ma = torch.zeros((B, T), dtype=torch.bool).scatter_(1, ids_a, True)
    mb = torch.zeros((B, T), dtype=torch.bool).scatter_(1, ids_b, True)
    return float((ma == mb).double().mean())


def teacher_target(cls_attn):
    """losses.py:76-79 on [B, L, H, n]: mean over layers, max over heads, drop the CLS column, renormalise -> float64 [B, n - 1]"""
    a = torch.as_tensor(cls_attn).double().mean(dim=1).max(dim=1)[0][:, 1:]
    return a / a.sum(dim=1, keepdim=True)


def gapped_rows(B, H, n, lead, T, mean_heads, seed):
    """Positive rows [B, H, n] fp32 whose reduced values are, per image, a permutation of the geometric grid g_j = r^j, r = 1 + max(2e-3,
    1 / T): values that are neighbours in rank differ by at least 2e-3 of the larger one, far beyond what fp32 rounding of the kernel's
    probabilities can reorder ((H + T + 2) 2^-24 each).  Head h holds scale_h * grid with scale_0 = 1 the largest, so the max over heads
    is head 0's row and the mean is mean(scale) * grid; columns outside [lead, lead + T) hold 0.5."""
    rng = np.random.default_rng(seed)
    grid = (1.0 + max(2e-3, 1.0 / T)) ** np.arange(T, dtype=np.float64)
    scale = np.array([1.0] + [0.9 - 0.05 * (h % 8) for h in range(1, H)])
    rows = np.full((B, H, n), 0.5, dtype=np.float64)
    for b in range(B):
        rows[b, :, lead:lead + T] = scale[:, None] * grid[rng.permutation(T)][None, :]
    return torch.from_numpy(rows.astype(np.float32))


def rank_gaps(w):
    """w [B, T] float64 reduced values -> (smallest gap between rank neighbours as a fraction of the larger value, the same as a fraction
    of the row sum), each the minimum over the batch"""
    v = torch.sort(torch.as_tensor(w).double(), dim=1)[0]
    if v.shape[1] < 2:
        return float("inf"), float("inf")
    gap = v[:, 1:] - v[:, :-1]
    return float((gap / v[:, 1:]).min()), float((gap / v.sum(dim=1, keepdim=True)).min())
