"""Cost of stochastic depth on the headline step: DeiT-S 224x224, pruning at block 3 keep 0.5, batch 128, exact fp32 GEMMs.

Two TrainStep objects in one process (drop_path_rate 0 and RATE, same weights and batch), timed alternately in rounds of STEPS steps
with device events; prints one JSON line with the per-step times and their difference.  The byte-count estimate of the extra work is two
row-scaling passes per block with a non-zero rate (8 bytes per element and branch) plus one table fill per step.

Per-kernel figures (scale_rows_kernel, drop_path_scales_kernel: calls, mean us) come from running this script under
`rocprofv3 --kernel-trace --stats -- python tools/droppath_bench.py`; the achieved TB/s of scale_rows follows from 8 * B * n * D bytes
per launch.

usage: python tools/droppath_bench.py [--rate 0.1] [--batch 128] [--steps 10] [--rounds 4]
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
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import vit_models
    from d2s import synth
    from d2s.engine import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    steps = {}
    base = None
    for rate in (0.0, a.rate):
        student = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                                   drop_path_rate=rate)
        teacher = vit_models.dynamic_vit_small_patch16_224_teacher()
        if base is None:
            base = (student.state_dict(), teacher.state_dict())
        else:
            student.load_state_dict(base[0])
            teacher.load_state_dict(base[1])
        args = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
        steps[rate] = TrainStep(student.to(dev), teacher.to(dev), args, warmup_steps=0, graph=False)
    x = torch.from_numpy(synth.images(a.batch, 3, 224, seed=1)).to(dev)
    y = torch.from_numpy(synth.labels(a.batch, 1000, seed=1)).to(dev)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts(x, y)
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(a.rounds):
        for rate, ts in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                ts(x, y)
            e1.record()
            torch.cuda.synchronize()
            ms[rate].append(e0.elapsed_time(e1) / a.steps)
    n_tok = [197] * 3 + [99] * 9
    rated = [i for i in range(12) if i > 0]      # block 0 has rate 0
    extra_bytes = sum(2 * 8 * a.batch * n_tok[i] * 384 for i in rated)
    best = {r: min(v) for r, v in ms.items()}
    print(json.dumps({"tool": "droppath_bench", "batch": a.batch, "rate": a.rate, "ms_per_step_rate0": [round(v, 3) for v in ms[0.0]],
                      "ms_per_step_rate": [round(v, 3) for v in ms[a.rate]], "delta_ms_best": round(best[a.rate] - best[0.0], 3),
                      "scale_rows_bytes_per_step": extra_bytes, "estimate_ms_at_4TBs": round(extra_bytes / 4e12 * 1e3, 3)}))


if __name__ == "__main__":
    main()
