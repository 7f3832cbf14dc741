"""Torch restatement of the differentiable token selection (the product vit_models/dynamic_vit.py:896-900 states in comments, with
pred_score := PerturbedTopKFunction(keep_probs), peturbed_topk.py:16-80) built on the oracle's functions: the yardstick of
tests/test_difftopk_cpu.py (pinned there to the reference's own run, tests/golden/difftopk_micro.npz) and tests/test_difftopk_gpu.py.
Plain torch on the CPU in the dtype of its inputs, autograd for the gradients; nothing here touches the HIP library."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O


class PerturbedTopK(torch.autograd.Function):
    """O.perturbed_topk_fwd with the backward of peturbed_topk.py:76-79 in the dtype of x (the oracle's backward is float32 only)"""

    @staticmethod
    def forward(ctx, x, noise, k, sigma):
        ind, ids = O.perturbed_topk_fwd(x, noise, k, sigma)
        ctx.save_for_backward(noise, ids)
        ctx.sigma = sigma
        return ind.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        noise, ids = ctx.saved_tensors
        onehot = F.one_hot(ids, num_classes=noise.shape[-1]).to(g.dtype)
        e = torch.einsum("bnkd,bnd->bkd", onehot, noise.to(g.dtype)) / noise.shape[1] / ctx.sigma
        return torch.einsum("bkd,bkd->bd", g, e), None, None, None


def soft_gather(x, ind):
    """:896-900: CLS passes through, spatial_x = ind @ x[:, 1:]"""
    return torch.cat((x[:, 0:1], ind @ x[:, 1:]), dim=1)


def margin(probs, noise, k, sigma):
    """smallest gap between the k-th and (k + 1)-th largest perturbed value over images and samples"""
    pert = torch.sort(probs.detach()[:, None, :] + noise * sigma, dim=-1, descending=True)[0]
    return float((pert[..., k - 1] - pert[..., k]).min())


def student_forward(sd, x, cfg, noises, sigma):
    """O.student_forward in training mode with the soft gather -> (logits, features, [pred_logits], [kept]), aux(probs, ind, x_in)"""
    x = O.embed_tokens(sd, x, cfg)
    counts = O.keep_counts(cfg)
    pred_logits, kept_all, probs_all, ind_all, x_in, stage = [], [], [], [], [], 0
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            x.retain_grad()
            x_in.append(x)
            scores, probs = O.predictor(sd, stage, x[:, 1:], cfg)
            kept, _ = O.select_topk(probs, counts[stage])
            ind = PerturbedTopK.apply(probs, noises[stage].to(x.dtype), counts[stage], sigma)
            pred_logits.append(scores)
            kept_all.append(kept)
            probs_all.append(probs)
            ind_all.append(ind)
            x = soft_gather(x, ind)
            stage += 1
        x, _ = O.block(sd, i, x, cfg)
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return (F.linear(x[:, 0], sd["head.weight"], sd["head.bias"]), x[:, 1:], pred_logits, kept_all), dict(probs=probs_all, ind=ind_all, x_in=x_in)


def probe_loss(tag, seed, logits, features):
    """the fixed linear probe of tools/gen_difftopk_fixture.py (weights from d2s.synth)"""
    from d2s import synth
    t = lambda a: torch.from_numpy(a).to(device=logits.device, dtype=logits.dtype)
    g1 = t(synth.normal(f"difftopk/{tag}/g1", tuple(logits.shape), seed=seed))
    g2 = t(synth.normal(f"difftopk/{tag}/g2", tuple(features.shape), seed=seed))
    return (logits * g1).sum() + (features * g2).sum() / features.shape[1]


SECTIONS = {"m1": "micro1", "m2": "micro2"}


def fixture_case(g, tag):
    """(case, [noise per stage], sigma) of a section of tests/golden/difftopk_micro.npz"""
    from tests import cases
    case = dict(cases.MODEL_CASES[SECTIONS[tag]], batch=int(g[f"{tag}_batch"]))
    noises = [torch.from_numpy(g[f"{tag}_noise_{i}"]) for i in range(int(g[f"{tag}_stages"]))]
    return case, noises, float(g[f"{tag}_sigma"])


def run_fixture_case(g, tag, dtype=torch.float64):
    """the restatement on a fixture section -> dict(logits, features, pred_logits, kept, probs, ind, grad_x, loss, grads{name: tensor})"""
    from d2s import synth
    from tests import cases
    case, noises, sigma = fixture_case(g, tag)
    cfg = case["cfg"]
    sd_s, _ = cases.make_weights(case)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in sd_s.items()}
    x = torch.from_numpy(synth.images(case["batch"], 3, cfg["img_size"], seed=case["seed"])).to(dtype)
    (lo, fe, pl, kept), aux = student_forward(sd, x, cfg, noises, sigma)
    loss = probe_loss(tag, case["seed"], lo, fe)
    loss.backward()
    return dict(logits=lo.detach(), features=fe.detach(), pred_logits=[p.detach() for p in pl], kept=kept,
                probs=[p.detach() for p in aux["probs"]], ind=[t.detach() for t in aux["ind"]], grad_x=[t.grad for t in aux["x_in"]],
                loss=loss.detach(), grads={k: v.grad for k, v in sd.items()})
