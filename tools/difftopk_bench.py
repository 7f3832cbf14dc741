"""Cost of the differentiable token selection (perturbed top-k soft gather) on the training step, exact fp32 GEMMs, DeiT-S 224x224:
  headline  one stage at block 3, keep 0.5, batch 128
  config3   three stages at blocks 3 / 6 / 9, keep 0.7 / 0.5 / 0.3, batch 32 (BASELINE.json config 3's per-GPU batch)

Per configuration two TrainStep objects in one process (diff_topk off and on, same weights and batch), timed alternately in rounds of
STEPS steps with device events; prints one JSON line per configuration with the per-step times and their difference, the soft-gather
FLOPs (three products of 2 * B * k * N * D per stage) and the bytes the mode keeps per stage for the backward (indicators + noise).

Per-kernel figures (soft_gather_kernel<0,1> forward, <1,1> backward w.r.t. x, <0,0> backward w.r.t. the indicators, ptk_fwd_kernel,
ptk_bwd_kernel, normal_noise_kernel: calls, mean us) come from running this script under
`rocprofv3 --kernel-trace --stats -- python tools/difftopk_bench.py`.

usage: python tools/difftopk_bench.py [--samples 500] [--steps 10] [--rounds 3] [--configs headline config3]
"""
import argparse
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dense2sparse-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {"headline": ([3], [0.5], 128), "config3": ([3, 6, 9], [0.7, 0.5, 0.3], 32)}


def bench(name, a):
    import vit_models
    from d2s import synth
    from d2s.engine import TrainStep
    locs, ratios, batch = CONFIGS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    steps, base = {}, None
    for on in (False, True):
        student = vit_models.dynamic_vit_small_patch16_224_student(locs, ratios, topk_selection=True, predictor_loss_type="kl_div",
                                                                   diff_topk=on, topk_num_samples=a.samples)
        teacher = vit_models.dynamic_vit_small_patch16_224_teacher()
        if base is None:
            base = (student.state_dict(), teacher.state_dict())
        else:
            student.load_state_dict(base[0])
            teacher.load_state_dict(base[1])
        args = types.SimpleNamespace(keep_ratios=list(ratios), mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
        steps[on] = TrainStep(student.to(dev), teacher.to(dev), args, warmup_steps=0, graph=False)
    x = torch.from_numpy(synth.images(batch, 3, 224, seed=1)).to(dev)
    y = torch.from_numpy(synth.labels(batch, 1000, seed=1)).to(dev)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts(x, y)
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(a.rounds):
        for on, ts in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                ts(x, y)
            e1.record()
            torch.cuda.synchronize()
            ms[on].append(e0.elapsed_time(e1) / a.steps)
    n, flops, held = 196, 0, []
    for r in ratios:
        k = int(196 * r)
        flops += 3 * 2 * batch * k * n * 384
        held.append({"N": n, "k": k, "indicators_bytes": 4 * batch * k * n, "noise_bytes": 4 * batch * a.samples * n})
        n = k
    best = {r: min(v) for r, v in ms.items()}
    print(json.dumps({"tool": "difftopk_bench", "config": name, "batch": batch, "samples": a.samples,
                      "ms_per_step_off": [round(v, 3) for v in ms[False]], "ms_per_step_on": [round(v, 3) for v in ms[True]],
                      "delta_ms_best": round(best[True] - best[False], 3), "soft_gather_flops_per_step": flops, "held_per_stage": held}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    a = ap.parse_args()
    for name in a.configs:
        bench(name, a)


if __name__ == "__main__":
    main()
