"""Float64 restatement of a transformer block with per-sample stochastic depth (the reference's Block.forward,
vit_models/dynamic_vit.py:263-269, with DropPath as vit_models/deit.py:69-77 and the draws given): the yardstick of
tests/test_droppath_gpu.py.  Plain torch on the CPU, autograd for the gradients; nothing here touches the HIP library."""
import math

import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O

# order of Block._params() in vit_models/dynamic_vit.py
PARAM_NAMES = ("n1w", "n1b", "qkvw", "qkvb", "projw", "projb", "n2w", "n2b", "fc1w", "fc1b", "fc2w", "fc2b")


def scales(masks, rates):
    """masks [R, B] of 0/1, rates [R] -> s = mask / keep in float64"""
    keep = 1.0 - torch.as_tensor(rates, dtype=torch.float64)
    return torch.as_tensor(masks, dtype=torch.float64) / keep[:, None]


def drop_path(x, mask, rate):
    """deit.py:69-77 with the Bernoulli draw given: x.div(keep) * mask[b]"""
    if rate == 0.:
        return x
    keep = 1.0 - rate
    return x.div(keep) * mask.to(x.dtype).view((x.shape[0],) + (1,) * (x.dim() - 1))


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def block(x, p, heads, eps, s_attn=None, s_mlp=None, scale=None):
    """x [B, n, D] float64, p: the 12 parameters (float64) in PARAM_NAMES order, s_attn / s_mlp: [B] scales (0 or 1 / keep) or None.
    y = x1 + s_mlp[b] * mlp(LN2 x1) with x1 = x + s_attn[b] * attn(LN1 x)."""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = p
    B, n, D = x.shape
    dh = D // heads
    scale = dh ** -0.5 if scale is None else scale
    h = layer_norm(x, n1w, n1b, eps)
    qkv = h @ qkvw.t()
    if qkvb is not None:
        qkv = qkv + qkvb
    q, k, v = qkv.reshape(B, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, n, D) @ projw.t() + projb
    if s_attn is not None:
        o = o * s_attn.view(B, 1, 1)
    x1 = x + o
    h = layer_norm(x1, n2w, n2b, eps)
    z = h @ fc1w.t() + fc1b
    g = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    m = g @ fc2w.t() + fc2b
    if s_mlp is not None:
        m = m * s_mlp.view(B, 1, 1)
    return x1 + m


def block_with_grads(x, params, heads, eps, gy, s_attn=None, s_mlp=None):
    """float32 inputs -> (y, dx, [12 parameter gradients]) in float64 for the upstream gradient gy"""
    xd = x.double().clone().requires_grad_(True)
    pd = [t.double().clone().requires_grad_(True) for t in params]
    sa = None if s_attn is None else s_attn.double()
    sm = None if s_mlp is None else s_mlp.double()
    y = block(xd, pd, heads, eps, sa, sm)
    grads = torch.autograd.grad(y, [xd] + pd, gy.double())
    return y.detach(), grads[0], list(grads[1:])


# ---- the whole student: the oracle's restatement of the reference's forward (oracle/d2s_oracle.py, pinned to the reference at rate 0 by
# tests/test_oracle_golden.py) with DropPath on both residual branches of every block; pinned to the reference's own run at rate 0.5 by
# tests/golden/droppath_micro.npz (tests/test_droppath_cpu.py) ----
def rates(cfg, drop_path_rate):
    """[2 * depth] per-row rates: dynamic_vit.py:695 for block i, twice (attention branch, MLP branch)"""
    return [p for p in (x.item() for x in torch.linspace(0, drop_path_rate, cfg["depth"])) for _ in (0, 1)]


def model_block(sd, i, x, cfg, masks, row_rates, policy=None):
    """Block.forward (dynamic_vit.py:263-269): x + drop_path(attn(LN1 x)), then + drop_path(mlp(LN2 .)); masks [2 * depth, B] of 0/1"""
    p = f"blocks.{i}."
    D, eps = cfg["dim"], cfg["ln_eps"]
    y, cls_row = O.attention(sd, p + "attn.", F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps), cfg["heads"], policy)
    x = x + drop_path(y, masks[2 * i], row_rates[2 * i])
    y = O.mlp(sd, p + "mlp.", F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps))
    return x + drop_path(y, masks[2 * i + 1], row_rates[2 * i + 1]), cls_row


def student_forward(sd, x, cfg, masks, drop_path_rate):
    """O.student_forward in training mode with stochastic depth -> (logits, features, [pred_logits], [kept])"""
    rr = rates(cfg, drop_path_rate)
    x = O.embed_tokens(sd, x, cfg)
    counts = O.keep_counts(cfg)
    pred_logits, kept_all, stage = [], [], 0
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            scores, probs = O.predictor(sd, stage, x[:, 1:], cfg)
            kept, _ = O.select_topk(probs, counts[stage])
            pred_logits.append(scores)
            kept_all.append(kept)
            x = O.gather_pack(x, kept)
            stage += 1
        x, _ = model_block(sd, i, x, cfg, masks, rr)
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return F.linear(x[:, 0], sd["head.weight"], sd["head.bias"]), x[:, 1:], pred_logits, kept_all


def student_forward_threshold_train(sd, x, cfg, threshold, masks, drop_path_rate):
    """O.student_forward_threshold_train (patch_score_threshold set: the keep mask is the attention policy, no token is removed) with
    stochastic depth -> (logits, features, [pred_logits per stage], [keep mask per stage])"""
    rr = rates(cfg, drop_path_rate)
    x = O.embed_tokens(sd, x, cfg)
    B, n, _ = x.shape
    policy = torch.ones(B, n, 1, dtype=x.dtype)
    pred_logits, keep, stage = [], [], 0
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            scores, probs = O.predictor(sd, stage, x[:, 1:], cfg)
            mask, _ = O.select_threshold(probs, threshold)
            mask = mask.to(x.dtype)
            policy = torch.cat((torch.ones(B, 1, dtype=x.dtype), mask), dim=1).unsqueeze(-1)
            pred_logits.append(scores)
            keep.append(mask)
            stage += 1
        x, _ = model_block(sd, i, x, cfg, masks, rr, policy=policy)
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return F.linear(x[:, 0], sd["head.weight"], sd["head.bias"]), x[:, 1:], pred_logits, keep


def probe_loss(tag, seed, logits, features, pred_logits):
    """the fixed linear probe of tools/gen_droppath_fixture.py (weights from d2s.synth)"""
    from d2s import synth
    t = lambda a: torch.from_numpy(a).to(logits.dtype)
    g1 = t(synth.normal(f"droppath/{tag}/g1", tuple(logits.shape), seed=seed))
    g2 = t(synth.normal(f"droppath/{tag}/g2", tuple(features.shape), seed=seed))
    out = (logits * g1).sum() + (features * g2).sum() / features.shape[1]
    for i, p in enumerate(pred_logits):
        out = out + (p * t(synth.normal(f"droppath/{tag}/g3/{i}", tuple(p.shape), seed=seed))).sum()
    return out


def fixture_case(g, prefix=""):
    """(case dict, tag, masks, rate) of a section of tests/golden/droppath_micro.npz"""
    from tests import cases
    if prefix:
        case, tag = cases.THRESHOLD_CASES["micro_thr1"], "micro_thr1"
    else:
        case, tag = dict(cases.MODEL_CASES["micro1"], batch=int(g["batch"])), "micro1"
    assert int(g[prefix + "batch"]) == case["batch"]
    return case, tag, torch.from_numpy(g[prefix + "masks"]), float(g[prefix + "rate"])


def run_fixture_case(g, prefix="", dtype=torch.float64):
    """the restatement on a fixture section -> dict(logits, features, pred_logits, sel, loss, grads{name: tensor})"""
    from d2s import synth
    from tests import cases
    case, tag, masks, rate = fixture_case(g, prefix)
    cfg = case["cfg"]
    sd_s, _ = cases.make_weights(case)
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd_s.items()}
    x = torch.from_numpy(synth.images(case["batch"], 3, cfg["img_size"], seed=case["seed"])).to(dtype)
    if prefix:
        lo, fe, pl, sel = student_forward_threshold_train(sd, x, cfg, case["threshold"], masks, rate)
        pl, sel = pl[-1:], sel[-1:]          # the reference returns the last stage's tensors only (:1011)
    else:
        lo, fe, pl, sel = student_forward(sd, x, cfg, masks, rate)
    loss = probe_loss(tag, case["seed"], lo, fe, pl)
    loss.backward()
    return dict(logits=lo.detach(), features=fe.detach(), pred_logits=[p.detach() for p in pl], sel=sel, loss=loss.detach(),
                grads={k: v.grad for k, v in sd.items()})
