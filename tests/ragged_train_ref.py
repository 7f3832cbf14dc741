"""Float64 torch-autograd restatement of training the dynamic keep ratio on the ragged packed batch (ragged_train=True; DESIGN.md section
10.2 - the build's own definition, PARITY UNPINNED), built from the oracle's embed_tokens / block / predictor the way
tests/ragged_cascade_ref.py builds the inference cascade, and of the two loss terms a packed batch needs.  Nothing here imports the
package under test.

The definition: dense blocks up to the first stage; the first stage scores all N tokens; from there on EVERY IMAGE ALONE (B = 1) on its
kept subset through all later blocks and stages - a later stage's predictor sees that image's surviving non-CLS tokens only - then the
final norm and the head.  Selections carry no gradient.  `masks` replays a list of per-stage CUMULATIVE dense [B, N] keep masks instead
of selecting (the GPU tests hand in the GPU's own: the selection is discrete)."""
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O


def train_forward(sd, x, cfg, threshold, masks=None, dtype=torch.float64):
    """sd: state dict of tensors (leaves that require grad keep their graph when already of `dtype`); x [B, 3, H, W].
    -> dict: logits [B, C]; feats: per image the normed rows [n_b, D], CLS first; pred_logits: [dense [B, N], then per later stage a list
    per image of the scores [T_b] over the rows that image brought to the stage]; ids_in: per stage per image the ORIGINAL patch ids
    (int64, ascending) of the rows scored; ids: per stage per image the ids kept; masks: per stage the cumulative dense [B, N] mask;
    gaps: per stage the smallest |running sum - threshold| of its selections (inf where nothing was scored)."""
    sd = {k: (v if v.dtype == dtype else v.detach().to(dtype)) for k, v in sd.items()}
    x = O.embed_tokens(sd, x.to(dtype), cfg)
    locs = list(cfg["pruning_loc"])
    first = locs[0]
    for i in range(first):
        x, _ = O.block(sd, i, x, cfg)
    B, n, _ = x.shape
    N = n - 1
    S = len(locs)
    scores0, probs0 = O.predictor(sd, 0, x[:, 1:], cfg)
    gaps = [float("inf")] * S
    gaps[0] = _gap(probs0.detach(), threshold)
    mask0 = O.select_threshold_stable(probs0.detach(), threshold)[0] if masks is None else masks[0]
    out = dict(logits=[], feats=[], pred_logits=[scores0] + [[] for _ in locs[1:]], ids_in=[[] for _ in locs], ids=[[] for _ in locs])
    for b in range(B):
        ids = torch.nonzero(mask0[b] > 0).flatten()
        out["ids_in"][0].append(torch.arange(N))
        out["ids"][0].append(ids)
        xb = x[b:b + 1, torch.cat((torch.zeros(1, dtype=torch.long), ids + 1))]
        stage = 1
        for i in range(first, cfg["depth"]):
            if i in locs and i != first:
                T = xb.shape[1] - 1
                out["ids_in"][stage].append(ids)
                if T > 0:
                    sc, pr = O.predictor(sd, stage, xb[:, 1:], cfg)
                    gaps[stage] = min(gaps[stage], _gap(pr.detach(), threshold))
                    keep = (O.select_threshold_stable(pr.detach(), threshold)[0][0] if masks is None else masks[stage][b, ids]) > 0
                    ids = ids[keep]
                    xb = xb[:, torch.cat((torch.ones(1, dtype=torch.bool), keep))]
                    sc = sc[0]
                else:       # only the CLS token is left: nothing to score
                    sc = torch.zeros(0, dtype=dtype)
                out["pred_logits"][stage].append(sc)
                out["ids"][stage].append(ids)
                stage += 1
            xb, _ = O.block(sd, i, xb, cfg)
        xb = F.layer_norm(xb, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
        out["logits"].append(F.linear(xb[:, 0], sd["head.weight"], sd["head.bias"]))
        out["feats"].append(xb[0])
    out["logits"] = torch.cat(out["logits"], dim=0)
    out["masks"] = []
    for per_image in out["ids"]:
        m = torch.zeros(B, N)
        for b, ids in enumerate(per_image):
            m[b, ids] = 1.0
        out["masks"].append(m)
    out["gaps"] = gaps
    return out


def _gap(probs, threshold):
    """smallest |running sum - threshold| over the rows of probs [R, T], sums taken in the stable ascending order"""
    val, _ = torch.sort(probs, stable=True)
    return float((torch.cumsum(val, dim=-1) - threshold).abs().min())


# ---------------------------------------------------------------------------------------------------------------- the two loss terms
def packed_mask_term(scores, ids_in, target, loss_type):
    """The mask-loss term of a packed stage: scores / ids_in per image ([T_b] scores of the rows the image brought to the stage, their
    original patch ids), target [B, N] the teacher target.  q = target gathered at the ids and renormalised.
    kl_div: (1 / B) sum_b KL(q_b || softmax(scores_b)), a zero q contributing nothing, an image without rows 0;
    mse: 100 * sum (score - q)^2 / (number of scored rows)."""
    B = target.shape[0]
    total, rows = 0, 0
    for b in range(B):
        if scores[b].numel() == 0:
            continue
        g = target[b, ids_in[b]]
        q = g / g.sum() if float(g.sum()) > 0 else torch.zeros_like(g)
        if loss_type == "mse":
            total = total + ((scores[b] - q) ** 2).sum()
            rows += scores[b].numel()
        else:
            total = total + (torch.xlogy(q, q) - q * F.log_softmax(scores[b], dim=-1)).sum()
    if loss_type == "mse":
        return 100.0 * total / rows if rows else torch.zeros((), dtype=target.dtype)
    return total / B


def token_distill_term(feats, ids_last, token_t):
    """The token distillation on the last packed batch: the mean over all non-CLS packed rows of KL(softmax(token_t[b, j_r]) ||
    softmax(token_s[r])); feats per image [n_b, D] (CLS first), ids_last per image the original ids of its non-CLS rows."""
    total, rows = 0, 0
    for b, f in enumerate(feats):
        if ids_last[b].numel() == 0:
            continue
        ls, lt = F.log_softmax(f[1:], dim=-1), F.log_softmax(token_t[b, ids_last[b]], dim=-1)
        total = total + (lt.exp() * (lt - ls)).sum()
        rows += f.shape[0] - 1
    return total / rows if rows else torch.zeros((), dtype=token_t.dtype)


def losses(out, teacher_out, labels, cfg):
    """-> (mask_loss, backbone_loss, (cls, cls_kl, token_kl)) of a train_forward output against the teacher's (logits, tokens, cls_attn):
    the first stage's dense term is the policy-mode one, every later stage adds its packed term"""
    logits_t, token_t, cls_attn = teacher_out
    target = O.teacher_target(cls_attn)
    kind = cfg["loss_type"]
    s0 = out["pred_logits"][0]
    if kind == "mse":
        mask_loss = 100.0 * F.mse_loss(s0, target)
    else:
        mask_loss = F.kl_div(F.log_softmax(s0, dim=-1), torch.log(target), log_target=True, reduction="batchmean")
    for s in range(1, len(out["pred_logits"])):
        mask_loss = mask_loss + packed_mask_term(out["pred_logits"][s], out["ids_in"][s], target, kind)
    cls = F.cross_entropy(out["logits"], labels)
    cls_kl = F.kl_div(F.log_softmax(out["logits"], dim=-1), F.log_softmax(logits_t, dim=-1), reduction="batchmean", log_target=True)
    tok = token_distill_term(out["feats"], out["ids"][-1], token_t)
    return mask_loss, cls + cls_kl + tok, (cls, cls_kl, tok)


def packed(per_image):
    """per-image rows -> the packed tensor the GPU holds (concatenation in image order)"""
    return torch.cat(list(per_image), dim=0)


def packed_scores(scores):
    """a later stage's per-image scores -> the packed [total] vector with 0 at the CLS rows (whose entries have no meaning)"""
    return torch.cat([torch.cat((torch.zeros(1, dtype=s.dtype), s)) for s in scores])


# ---------------------------------------------------------------------------------------------------------------- the cases
def train_cases():
    """the geometries of the model tests: one stage, two stages, three stages with the small predictor"""
    from tests import cases
    from tests import ragged_cascade_ref as C
    return {"micro_thr1": cases.THRESHOLD_CASES["micro_thr1"], "micro_thr2": C.cascade_cases()["micro_thr2"],
            "micro_thr3s": C.cascade_cases()["micro_thr3s"]}


# smallest |running sum - threshold| of the fp32 restatement on each case, per stage (computed on the CPU by
# tests/test_ragged_train_cpu.py::test_selection_gaps_of_the_cases, which keeps these figures honest): all above section 14's margin
SELECTION_MARGIN = 2e-5


def case_tensors(name):
    """-> (case, student state dict, teacher state dict, images, labels) as torch tensors"""
    import numpy as np
    from tests import cases
    case = train_cases()[name]
    sd_s, sd_t = cases.make_weights(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return (case, {k: t(v) for k, v in sd_s.items()}, {k: t(v) for k, v in sd_t.items()}, t(cases.make_images(case)),
            t(cases.make_labels(case)))


def model_grads(name, masks=None, warmup=False, logit_weight=None):
    """float64 forward, losses and parameter gradients of a case.  logit_weight [B, C]: the objective is (logits * W).sum() instead of
    the training loss.  -> (out, loss, {name: grad or None}, (mask_loss, backbone_loss, terms))"""
    case, sd_s, sd_t, x, y = case_tensors(name)
    cfg = case["cfg"]
    sd = {k: v.double().requires_grad_(True) for k, v in sd_s.items()}
    out = train_forward(sd, x, cfg, case["threshold"], masks=masks)
    with torch.no_grad():
        teacher_out = O.teacher_forward({k: v.double() for k, v in sd_t.items()}, x.double(), cfg)
    mask_loss, backbone_loss, terms = losses(out, teacher_out, y, cfg)
    if logit_weight is not None:
        loss = (out["logits"] * logit_weight.double()).sum()
    else:
        loss = mask_loss if warmup else mask_loss + backbone_loss
    grads = torch.autograd.grad(loss, list(sd.values()), allow_unused=True)
    return out, loss.detach(), dict(zip(sd.keys(), grads)), (mask_loss.detach(), backbone_loss.detach(), terms)
