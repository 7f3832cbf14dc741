#!/usr/bin/env python3
"""Generate tests/golden/dynamicvit_micro.npz by running the REFERENCE's own DynamicViT baseline (vit_models/default_dynamic_vit.py) on
CPU with build-generated weights.  Runs where the reference checkout is (never on the GPU machine); the file holds data only.

The reference file is loaded by path like tools/gen_golden.py loads dynamic_vit.py (same five timm stand-ins).  Its forward hard-codes
init_n = 14 * 14 (:446), which cannot run the micro geometry (N = 16): that one assignment is read as `init_n = x.shape[1] - 1` when the
module is compiled in memory (nothing is written).  torch.nn.functional.gumbel_softmax is wrapped: the wrapper draws the noise the way
torch does (-log of an Exponential(1) sample), records it, and evaluates torch's documented formula with it.

Condition on the draw: a hard decision flips where |(logp_0 + g_0) - (logp_1 + g_1)| is within rounding, so the torch seed is searched
until the smallest such gap over all stages, and the eval top-k boundary gap, are at least MARGIN; the gap and the number of qualifying
seeds among the first 40 are recorded.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_dynamicvit_fixture.py
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden  # noqa: E402
from tests import dynamicvit_cases as DC  # noqa: E402
from tests import dynamicvit_ref as R  # noqa: E402

MARGIN = 2e-5
SEEDS = 40


def load_reference():
    import types
    gen_golden._install_standins()
    path = os.path.join(gen_golden.REF, "vit_models", "default_dynamic_vit.py")
    src = open(path).read()
    assert src.count("init_n = 14 * 14") == 1
    src = src.replace("init_n = 14 * 14", "init_n = x.shape[1] - 1")
    m = types.ModuleType("ref_default_dynamic_vit")
    exec(compile(src, path, "exec"), m.__dict__)
    return m


class Recorder:
    def __init__(self):
        self.noise = []

    def __call__(self, logits, tau=1, hard=False, eps=1e-10, dim=-1):
        g = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        self.noise.append(g.clone())
        y = ((logits + g) / tau).softmax(dim)
        if not hard:
            return y
        idx = y.max(dim, keepdim=True)[1]
        y_hard = torch.zeros_like(logits, memory_format=torch.legacy_contiguous_format).scatter_(dim, idx, 1.0)
        return y_hard - y.detach() + y


def run_case(ref, name):
    case = DC.CASES[name]
    cfg = case["cfg"]
    sd = {k: torch.from_numpy(v) for k, v in DC.make_weights(case).items()}
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref.DefaultVisionTransformerDiffPruning(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                                                        num_heads=cfg["heads"], num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
                                                        token_ratio=list(cfg["token_ratio"]), distill=True)
    assert set(model.state_dict()) == set(sd), sorted(set(model.state_dict()) ^ set(sd))
    model.load_state_dict(sd)
    x = torch.from_numpy(DC.make_images(case))
    sd64 = {k: v.double() for k, v in sd.items()}
    model.eval()
    with torch.no_grad():
        eval_logits = model(x)
    eval_gap = min([float(g) for g in R.forward(sd64, cfg, x, training=False)["gaps"]] or [float("inf")])
    assert eval_gap >= MARGIN, f"{name}: eval top-k boundary gap {eval_gap}"
    model.train()
    good, chosen = 0, None
    orig = F.gumbel_softmax
    for seed in range(SEEDS):
        rec = Recorder()
        F.gumbel_softmax = rec
        try:
            torch.manual_seed(seed)
            model.zero_grad()
            logits, feats, final, decs = model(x)
        finally:
            F.gumbel_softmax = orig
        gap = min(float(g) for g in R.forward(sd64, cfg, x, noise=[g.double() for g in rec.noise])["gaps"])
        if gap >= MARGIN:
            good += 1
            if chosen is None:
                out = dict(logits=logits, features=feats, decisions=list(decs))
                R.probe(out, cfg).backward()
                chosen = dict(seed=seed, gap=gap, noise=rec.noise, logits=logits, feats=feats, final=final, decs=decs,
                              grads={k: p.grad.clone() for k, p in model.named_parameters()})
    assert chosen is not None, f"{name}: no seed of {SEEDS} keeps every decision {MARGIN} away from a flip"
    o = {f"{name}/eval_logits": eval_logits.numpy(), f"{name}/eval_gap": np.float64(eval_gap), f"{name}/seed": np.int64(chosen["seed"]),
         f"{name}/gap": np.float64(chosen["gap"]), f"{name}/seeds_qualified": np.int64(good), f"{name}/seeds_tried": np.int64(SEEDS),
         f"{name}/logits": chosen["logits"].detach().numpy(), f"{name}/features": chosen["feats"].detach().numpy(),
         f"{name}/final_decision": chosen["final"].reshape(x.shape[0], -1).numpy()}
    for i, (g, d) in enumerate(zip(chosen["noise"], chosen["decs"])):
        o[f"{name}/noise{i}"] = g.numpy()
        o[f"{name}/decision{i}"] = d.detach().numpy().astype(np.uint8)
    # every parameter's probe gradient as its L2 norm and GRAD_SAMPLES evenly strided elements (the full tensors are 3.6 MB per case)
    names = sorted(chosen["grads"])
    o[f"{name}/grad_norm"] = np.array([float(chosen["grads"][k].double().norm()) for k in names], dtype=np.float64)
    o[f"{name}/grad_sample"] = np.stack([DC.grad_sample(chosen["grads"][k]).numpy() for k in names]).astype(np.float32)
    print(f"{name}: seed {chosen['seed']}, gap {chosen['gap']:.3e}, eval gap {eval_gap:.3e}, {good}/{SEEDS} seeds qualify")
    return o


def main():
    ref = load_reference()
    out = {}
    for name in DC.CASES:
        out.update(run_case(ref, name))
    path = os.path.join(REPO, "tests", "golden", "dynamicvit_micro.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
