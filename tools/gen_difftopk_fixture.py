#!/usr/bin/env python3
"""Generate tests/golden/difftopk_micro.npz: the differentiable token selection the reference states at vit_models/dynamic_vit.py:896-900
(`spatial_x = pred_score @ spatial_x  # shape: (B, K, D)`, `x = torch.cat((cls_x, spatial_x), dim=1)`) and never connects, composed from
the REFERENCE's own live modules on the CPU: its patch embedding, PredictorLG, PerturbedTopKFunction (peturbed_topk.py:16-80), Blocks,
final norm and head, with pred_score := PerturbedTopKFunction.apply(keep_probs, k, nS, sigma).

Runs only where the reference exists (never on the GPU machine); the reference is loaded read-only the way tools/gen_golden.py loads it.
Outputs only.  Two sections: m1_ (tests/cases.py micro1, one stage: 16 -> 9 tokens) and m2_ (micro2, two stages: 16 -> 9 -> 5), both with
d2s.synth weights, B = 4, nS = 16, sigma = 0.05.  Per section: per stage the noise the reference drew, keep probabilities, indicators, kept ids
(:858-862), predictor logits and the gradient w.r.t. the stage input (norm + a slice); logits, features; the gradient of a fixed linear
probe of logits + features w.r.t. every predictor tensor (norm + leading elements); `margin`, the smallest gap between the k-th and the
(k + 1)-th largest perturbed value over all images, samples and stages.

Condition, not measurement: the torch seed (it decides the reference's torch.normal draw) is searched from SEED0 upwards until
margin >= MARGIN_MIN, and recorded together with how many seeds were tried.  MARGIN_MIN = 2e-5: the project's predictor-logit tolerance
(atol 1e-5) moves a probability of about 0.06 by about 6e-7, so the sample counts - integers - are then defined with a factor of 30 to
spare, independently of fp32 rounding order.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_difftopk_fixture.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402
from d2s import synth  # noqa: E402
from tests import cases  # noqa: E402

BATCH, NS, SIGMA = 4, 16, 0.05
SEED0 = 2026
MARGIN_MIN = 2e-5


def soft_forward(student, ptk, x, cfg, seed):
    """dynamic_vit.py:814-1013 in training mode with :896-900 in place of the gather (:907-912) -> outputs and per-stage records"""
    torch.manual_seed(seed)
    x = student.patch_embed(x)                                                    # :816
    B = x.shape[0]
    x = torch.cat((student.cls_token.expand(B, -1, -1), x), dim=1)                # :820-822
    x = student.pos_drop(x + student.pos_embed)                                   # :823-824
    init_n = 14 * 14                                                              # :828
    stages, p_count, margin = [], 0, float("inf")
    for i, blk in enumerate(student.blocks):
        if i in student.pruning_loc:
            x.retain_grad()
            k = int(init_n * student.token_ratio[p_count])                        # :852
            pred_logits, pred_score = student.score_predictor[p_count](x[:, 1:])  # :855
            order = torch.argsort(pred_score, dim=1, descending=True)             # :858-861
            kept = torch.sort(order[:, :k], dim=1)[0]
            ind = ptk.PerturbedTopKFunction.apply(pred_score, k, NS, SIGMA)       # :556 (commented out there)
            noise = ind.grad_fn.noise                                             # the draw of peturbed_topk.py:29
            pert = torch.sort(pred_score.detach()[:, None, :] + noise * SIGMA, dim=-1, descending=True)[0]
            margin = min(margin, float((pert[..., k - 1] - pert[..., k]).min()))
            spatial_x = ind @ x[:, 1:]                                            # :897  shape: (B, K, D)
            stages.append(dict(x_in=x, noise=noise, probs=pred_score, ind=ind, kept=kept, pred_logits=pred_logits))
            x = torch.cat((x[:, 0:1], spatial_x), dim=1)                          # :879, :900
            p_count += 1
        x, _ = blk(x, return_cls_attn=True)                                       # :924 / :985
    x = student.norm(x)                                                           # :993
    return student.head(student.pre_logits(x[:, 0])), x[:, 1:], stages, margin    # :994-1006


def run(dv, ptk, name, tag):
    case = dict(cases.MODEL_CASES[name], batch=BATCH)
    cfg = case["cfg"]
    student, _ = G.build_ref_models(dv, case)
    student.train()
    x = G._t(synth.images(BATCH, 3, cfg["img_size"], seed=case["seed"]))
    tried = 0
    for seed in range(SEED0, SEED0 + 1000):
        tried += 1
        logits, features, stages, margin = soft_forward(student, ptk, x.clone(), cfg, seed)
        if margin >= MARGIN_MIN:
            break
    assert margin >= MARGIN_MIN, "no seed gave the margin"
    g1 = G._t(synth.normal(f"difftopk/{tag}/g1", tuple(logits.shape), seed=case["seed"]))
    g2 = G._t(synth.normal(f"difftopk/{tag}/g2", tuple(features.shape), seed=case["seed"]))
    probe = (logits * g1).sum() + (features * g2).sum() / features.shape[1]
    student.zero_grad()
    probe.backward()
    out = {"seed": np.array(seed), "seeds_tried": np.array(tried), "batch": np.array(BATCH), "num_samples": np.array(NS),
           "sigma": np.array(SIGMA), "margin": np.array(margin, np.float64), "logits": G._np(logits), "features": G._np(features),
           "probe_loss": G._np(probe), "stages": np.array(len(stages))}
    for i, st in enumerate(stages):
        for key in ("noise", "probs", "ind", "kept", "pred_logits"):
            out[f"{key}_{i}"] = G._np(st[key])
        gx = st["x_in"].grad
        out[f"grad_x_norm_{i}"] = np.array(float(gx.double().norm()))
        out[f"grad_x_slice_{i}"] = G._np(gx[:, :, :8])
    names, norms, heads = [], [], []
    for n_, p in student.named_parameters():
        if not n_.startswith("score_predictor."):
            continue
        assert p.grad is not None, n_
        g = p.grad.detach().flatten()
        names.append(n_)
        norms.append(float(g.double().norm()))
        h = np.zeros(8, np.float32)
        h[: min(8, g.numel())] = G._np(g[:8])
        heads.append(h)
    out["grad_names"], out["grad_norms"], out["grad_heads"] = np.array(names), np.array(norms, np.float64), np.stack(heads)
    print(f"[golden] difftopk {tag}: seed {seed} after {tried} tried, margin {margin:.3e}, probe loss {float(probe.detach()):.6f}, "
          f"min predictor grad norm {min(norms):.3e}")
    return {f"{tag}_{k}": v for k, v in out.items()}


def seed_yield(dv, ptk, name, n=40):
    """how many of n seeds satisfy the margin (quoted in DESIGN.md section 14)"""
    case = dict(cases.MODEL_CASES[name], batch=BATCH)
    student, _ = G.build_ref_models(dv, case)
    student.train()
    x = G._t(synth.images(BATCH, 3, case["cfg"]["img_size"], seed=case["seed"]))
    return sum(soft_forward(student, ptk, x.clone(), case["cfg"], s)[3] >= MARGIN_MIN for s in range(SEED0, SEED0 + n))


def main():
    dv, _, ptk = G._load_reference()
    out = {}
    out.update(run(dv, ptk, "micro1", "m1"))
    out.update(run(dv, ptk, "micro2", "m2"))
    if "--yield" in sys.argv:
        print("[golden] seeds with margin >= 2e-5 out of 40:", seed_yield(dv, ptk, "micro1"), seed_yield(dv, ptk, "micro2"))
    path = os.path.join(G.OUT, "difftopk_micro.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 200 * 1024
    print(f"[golden] wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
