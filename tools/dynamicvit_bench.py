"""Cost of the DynamicViT baseline step next to the d2s headline step: DeiT-S 224x224, batch 128, exact fp32 GEMMs (or --gemm-mode bf16:
the bf16 arithmetic mode, where the baseline's policy blocks attend through d2s_attn_policy_fwd_bf16 / _bwd_bf16).

Two TrainStep objects in one process - the d2s student (pruning at block 3, keep 0.5, top-k selection) and the DynamicViT baseline
(default_dynamic_vit_small_patch16_224_student, stages 3 / 6 / 9 at 0.7 / 0.49 / 0.343, dense training) - timed alternately in rounds of
STEPS steps with device events; prints one JSON line with the per-step times.  The baseline keeps all 197 tokens in every block and runs
policy attention from block 3 on, so it is expected to cost more than the d2s step, which halves the tokens after block 3.

Per-launch times of the attention backward's dK/dV kernel with and without the policy gradient come from running this script under
`rocprofv3 --kernel-trace --stats -- python tools/dynamicvit_bench.py --rounds 1`: the baseline's blocks 0-2 launch the mask-free
instantiation and blocks 3-11 the DPOL one, at the same (B, H, n) = (128, 6, 197).

usage: python tools/dynamicvit_bench.py [--batch 128] [--steps 10] [--rounds 4] [--gemm-mode exact|split|bf16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gemm-mode", choices=["exact", "split", "bf16"], default="exact")
    a = ap.parse_args()
    import vit_models
    from d2s import ops, synth
    ops.set_gemm_mode({"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}[a.gemm_mode])
    from d2s.engine import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    locs, ratios = [3, 6, 9], [0.7, 0.49, 0.343]
    d2s_args = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
    dyn_args = types.SimpleNamespace(keep_ratios=ratios, mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0,
                                     cls_weight=1.0, ratio_weight=2.0, dist_weight=0.5)
    steps = {
        "d2s": TrainStep(vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div").to(dev),
                         vit_models.dynamic_vit_small_patch16_224_teacher().to(dev), d2s_args, warmup_steps=0, graph=False),
        "dynamicvit": TrainStep(vit_models.default_dynamic_vit_small_patch16_224_student(locs, ratios).to(dev),
                                vit_models.default_dynamic_vit_small_patch16_224_teacher().to(dev), dyn_args, warmup_steps=0, graph=False),
    }
    x = torch.from_numpy(synth.images(a.batch, 3, 224, seed=1)).to(dev)
    y = torch.from_numpy(synth.labels(a.batch, 1000, seed=1)).to(dev)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts(x, y)
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, ts in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                ts(x, y)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps({"tool": "dynamicvit_bench", "batch": a.batch, "gemm_mode": a.gemm_mode, "ms_per_step_d2s": [round(v, 3) for v in ms["d2s"]],
                      "ms_per_step_dynamicvit": [round(v, 3) for v in ms["dynamicvit"]],
                      "ratio_best": round(best["dynamicvit"] / best["d2s"], 3),
                      "images_per_s_dynamicvit": round(a.batch / best["dynamicvit"] * 1e3, 1)}))


if __name__ == "__main__":
    main()
