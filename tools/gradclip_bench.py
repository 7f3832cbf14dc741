"""Cost of global-norm clipping and of gradient accumulation on the headline step: DeiT-S 224x224, pruning at block 3 keep 0.5, batch 128,
exact fp32 GEMMs.

Three TrainStep objects in one process (default, clip_grad=M, accum_steps=A; same weights and batch), timed alternately in rounds of STEPS
calls with device events; prints one JSON line with the times per call (= per micro-step) and their differences.  From bytes alone an
accumulate moves 8 / 12 bytes per active element, the sum of squares 4, AdamW 28 as before.

Per-kernel figures (grad_accumulate_kernel<0|1|2>, grad_sumsq_kernel, grad_clip_fold_kernel, adamw_clip_kernel: calls, mean us) come from
running this script under `rocprofv3 --kernel-trace --stats -- python tools/gradclip_bench.py`.

usage: python tools/gradclip_bench.py [--clip 1.0] [--accum 4] [--batch 128] [--steps 8] [--rounds 4]
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
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=8, help="calls per timed round (a multiple of --accum)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if a.steps % a.accum or a.warmup % a.accum:
        raise SystemExit("--steps and --warmup must be multiples of --accum (a timed round holds whole windows)")
    import vit_models
    from d2s import synth
    from d2s.engine import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    steps = {}
    base = None
    for name, kw in (("off", {}), ("clip", dict(clip_grad=a.clip)), ("accum", dict(accum_steps=a.accum))):
        student = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div")
        teacher = vit_models.dynamic_vit_small_patch16_224_teacher()
        if base is None:
            base = (student.state_dict(), teacher.state_dict())
        else:
            student.load_state_dict(base[0])
            teacher.load_state_dict(base[1])
        args = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
        steps[name] = TrainStep(student.to(dev), teacher.to(dev), args, warmup_steps=0, graph=False, **kw)
    x = torch.from_numpy(synth.images(a.batch, 3, 224, seed=1)).to(dev)
    y = torch.from_numpy(synth.labels(a.batch, 1000, seed=1)).to(dev)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts(x, y)
    torch.cuda.synchronize()
    ms = {r: [] for r in steps}
    for _ in range(a.rounds):
        for name, ts in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                ts(x, y)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    ts = steps["off"]
    active = int(sum(sz for sz, g in zip(ts.arena.sizes, ts.opt.groups) if g is not None and g != "early_exit"))
    best = {r: min(v) for r, v in ms.items()}
    clip = steps["clip"].last_clip.tolist()
    print(json.dumps({"tool": "gradclip_bench", "batch": a.batch, "clip": a.clip, "accum": a.accum, "arena_elems": ts.arena.total,
                      "active_elems": active, "ms_per_call_off": [round(v, 3) for v in ms["off"]],
                      "ms_per_call_clip": [round(v, 3) for v in ms["clip"]], "ms_per_call_accum": [round(v, 3) for v in ms["accum"]],
                      "delta_ms_clip_best": round(best["clip"] - best["off"], 3), "delta_ms_accum_best": round(best["accum"] - best["off"], 3),
                      "last_norm": clip[0], "last_coef": clip[1],
                      "bytes_norm_pass": 4 * active, "estimate_us_norm_at_5TBs": round(4 * active / 5e12 * 1e6, 1),
                      "bytes_accumulate_modes": [8 * active, 12 * active, 12 * active]}))


if __name__ == "__main__":
    main()
