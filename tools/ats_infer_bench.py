"""Inference throughput of the Adaptive Token Sampling baseline (--method ats) next to the dense teacher: eval mode,
forward only, DeiT-S 224, B = 128, a sampling stage in each of blocks 3-11 with K = N (the paper's placement), in the exact and the bf16
arithmetic modes, the two models alternating for --rounds rounds of 30 forwards each.  Prints ms per batch (mean over the rounds, with the
spread between them) and images/s of both models and, for ATS, the mean number of tokens (CLS not counted) that leave
every stage - the figure means nothing without it: with seeded random weights attention is near uniform and ATS keeps almost everything,
a trained checkpoint (--student-checkpoint) keeps far fewer.  GPU box only.

  python tools/ats_infer_bench.py [--gemm-mode exact|bf16|split|all] [--ats-locs 3 4 ... 11] [--ats-tokens K] [--student-checkpoint deit_small.pth]
  python tools/ats_infer_bench.py --gemm-mode bf16 --no-teacher --rounds 1        (under a profiler: the ATS model alone)
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
import vit_models
from d2s import ops

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split"), "bf16": (ops.GEMM_BF16, "bf16 operands")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES) + ["all"], default="all", help="all: exact and bf16")
ap.add_argument("--ats-locs", type=int, nargs="+", default=list(range(3, 12)))
ap.add_argument("--ats-tokens", type=int, default=None, help="K of every stage (default: the number of patches)")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for both models (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-teacher", action="store_true", help="time the ATS model only")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 3, 30
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)


def timed(model, warm):
    with torch.no_grad():
        for _ in range(WARMUP if warm else 0):
            model(x)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(TIMED):
            model(x)
        e.record()
        torch.cuda.synchronize()
    return s.elapsed_time(e) / TIMED


for key in (["exact", "bf16"] if args.gemm_mode == "all" else [args.gemm_mode]):
    mode, mname = MODES[key]
    ops.set_gemm_mode(mode)
    torch.manual_seed(0)
    teacher = vit_models.dynamic_vit_small_patch16_224_teacher(checkpoint_path=args.student_checkpoint).to(dev).eval()
    torch.manual_seed(0)
    ats = vit_models.ats_deit_small_patch16_224(ats_locs=args.ats_locs, ats_tokens=args.ats_tokens,
                                                checkpoint_path=args.student_checkpoint).to(dev).eval()
    models = ([] if args.no_teacher else [teacher]) + [ats]
    times = {id(m): [] for m in models}
    for r in range(args.rounds):
        for m in models:
            times[id(m)].append(timed(m, r == 0))
    stat = lambda m: (sum(times[id(m)]) / args.rounds, max(times[id(m)]) - min(times[id(m)]))
    if not args.no_teacher:
        ms, spread = stat(teacher)
        print(f"{mname:14s} dense teacher                      {ms:7.2f} ms/batch (spread {spread:.2f})  {B / ms * 1e3:9.0f} images/s", flush=True)
    ms, spread = stat(ats)
    per = [c.float() for c in ats.tokens_per_stage]
    print(f"{mname:14s} ats @ blocks {args.ats_locs[0]}-{args.ats_locs[-1]} K = {ats.ats_tokens[0]:4d}       {ms:7.2f} ms/batch (spread {spread:.2f})  {B / ms * 1e3:9.0f} images/s   "
          f"tokens per stage: mean {[round(float(c.mean()), 1) for c in per]} min {[int(c.min()) for c in per]} max {[int(c.max()) for c in per]}",
          flush=True)
    del teacher, ats
ops.set_gemm_mode(ops.GEMM_EXACT)
