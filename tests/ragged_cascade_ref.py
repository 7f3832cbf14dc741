"""CPU restatement of ragged inference through every threshold stage (the eval-mode forward with patch_score_threshold set and any
number of pruning stages), built from the oracle's own embed_tokens, block, predictor(..., training=False) and
select_threshold_stable.

The definition: dense up to the first stage; from the first stage on EVERY IMAGE ALONE (B = 1) on its kept subset through all later
blocks and stages - a later stage's predictor sees that image's surviving non-CLS tokens only (its global half is their mean, its
softmax runs over them) and the threshold rule selects among them - then the final norm and the head.  PARITY UNPINNED: the reference's
second stage cannot run (vit_models/dynamic_vit.py:945-946)."""
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O


def cascade_forward(sd, x, cfg, threshold, dtype=torch.float32):
    """sd: state dict of tensors; x [B,3,H,W].  -> (logits [B,C], [normed tokens per image [n_b, D]], stages) with
    stages[s][b] = (T = non-CLS tokens image b brought to stage s, kept patch ids in ORIGINAL coordinates (int64, ascending),
    the stage's scores over those T tokens [T])."""
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    x = O.embed_tokens(sd, x.to(dtype), cfg)
    locs = list(cfg["pruning_loc"])
    first = locs[0]
    for i in range(first):
        x, _ = O.block(sd, i, x, cfg)
    B, n, _ = x.shape
    scores0, probs0 = O.predictor(sd, 0, x[:, 1:], cfg, training=False)
    mask0, _ = O.select_threshold_stable(probs0, threshold)
    stages = [[] for _ in locs]
    logits, feats = [], []
    for b in range(B):
        ids = torch.nonzero(mask0[b] > 0).flatten()
        stages[0].append((n - 1, ids, scores0[b]))
        xb = x[b:b + 1, torch.cat((torch.zeros(1, dtype=torch.long), ids + 1))]
        stage = 1
        for i in range(first, cfg["depth"]):
            if i in locs and i != first:
                T = xb.shape[1] - 1
                if T > 0:
                    sc, pr = O.predictor(sd, stage, xb[:, 1:], cfg, training=False)
                    m, _ = O.select_threshold_stable(pr, threshold)
                    keep = m[0] > 0
                    ids = ids[keep]
                    xb = xb[:, torch.cat((torch.ones(1, dtype=torch.bool), keep))]
                    sc = sc[0]
                else:       # only the CLS token is left: nothing to score
                    sc = torch.zeros(0, dtype=dtype)
                stages[stage].append((T, ids, sc))
                stage += 1
            xb, _ = O.block(sd, i, xb, cfg)
        xb = F.layer_norm(xb, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
        logits.append(F.linear(xb[:, 0], sd["head.weight"], sd["head.bias"]))
        feats.append(xb[0])
    return torch.cat(logits, dim=0), feats, stages


def dense_masks(stages, N):
    """-> per stage the cumulative [B, N] 0/1 mask (float32) in original patch coordinates"""
    out = []
    for per_image in stages:
        m = torch.zeros(len(per_image), N)
        for b, (_, ids, _) in enumerate(per_image):
            m[b, ids] = 1.0
        out.append(m)
    return out


def cu_seqlens(stages):
    """-> per stage the int32 [B+1] offsets of the packed batch the stage leaves (kept tokens + CLS per image)"""
    out = []
    for per_image in stages:
        lens = torch.tensor([int(ids.numel()) + 1 for _, ids, _ in per_image])
        out.append(torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0))).int())
    return out


# ---- the cases of the cascade tests (CPU and GPU tier) and their references, computed once per process ----
def cascade_cases():
    from tests import cases
    return {
        "micro_thr2": cases.THRESHOLD_CASES["micro_thr2"],
        "small_thr3": dict(cfg=O.make_cfg(dim=384, depth=6, heads=6, num_classes=100, pruning_loc=(1, 3, 4), token_ratio=(0.7, 0.5, 0.3)),
                           batch=3, seed=64, threshold=0.35),
        "micro_thr3s": dict(cfg=O.make_cfg(img_size=96, dim=128, depth=5, heads=2, num_classes=10, pruning_loc=(1, 2, 4),
                                           token_ratio=(0.7, 0.5, 0.3), small_predictor=True), batch=4, seed=65, threshold=0.3),
    }


_REFS = {}


def reference(name, dtype=torch.float32, threshold=None):
    """cascade_forward of a named case (cached; callers must not modify what they get)"""
    import numpy as np
    from tests import cases
    key = (name, dtype, threshold)
    if key not in _REFS:
        case = cascade_cases()[name]
        sd_s, _ = cases.make_weights(case)
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_s.items()}
        x = torch.from_numpy(np.ascontiguousarray(cases.make_images(case)))
        with torch.no_grad():
            _REFS[key] = cascade_forward(sd, x, case["cfg"], case["threshold"] if threshold is None else threshold, dtype)
    return _REFS[key]
