"""Eval forward and training step time of the Evo-ViT baseline (--method evo): DeiT-S 224, B = 128, seeded random
weights unless a checkpoint is given.  Two models, measured next to each other, alternating in one process for --rounds rounds of 10
iterations each:
  * the dense trunk: evo_start = depth, no slow-fast block (the teacher's launches plus one score launch);
  * the slow-fast trunk at --evo-start / --evo-keep / --evo-tradeoff (defaults 4 / 0.5 / 0.5).
For each: the eval forward (torch.no_grad) and one optimiser step through TrainStep's logits-only route (cross entropy, no teacher, fused
AdamW).  Prints ms per iteration (mean over the rounds, with the spread between them), images/s and the rows every block ran on.
GPU box only.

  python tools/evo_bench.py [--gemm-mode exact|split|bf16] [--evo-start 4] [--evo-keep 0.5] [--evo-tradeoff 0.5] [--graph]
                            [--student-checkpoint deit_small.pth]
"""
import argparse
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
import vit_models
from d2s import ops
from d2s.engine import TrainStep

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split"), "bf16": (ops.GEMM_BF16, "bf16")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES), default="exact")
ap.add_argument("--evo-start", type=int, default=4)
ap.add_argument("--evo-keep", type=float, default=0.5)
ap.add_argument("--evo-tradeoff", type=float, default=0.5)
ap.add_argument("--graph", action="store_true", help="capture the training step (TrainStep(graph=True))")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for both models (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 3, 10
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def evo(start):
    torch.manual_seed(0)
    return vit_models.evo_deit_small_patch16_224(evo_start=start, evo_keep=args.evo_keep, evo_tradeoff=args.evo_tradeoff,
                                                 checkpoint_path=args.student_checkpoint).to(dev)


def timed(fn, warm):
    for _ in range(WARMUP if warm else 0):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(TIMED):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / TIMED


def eval_of(model):
    model.eval()

    def run():
        with torch.no_grad():
            model(x)
    return run


def step_of(model):
    a = types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, step=0)
    ts = TrainStep(model.train(), None, a, lr=1e-5, graph=bool(args.graph))
    return lambda: ts(x, y)


runs = []
for name, start in (("dense (evo_start = depth)", 12), (f"evo start {args.evo_start} keep {args.evo_keep:g} tau {args.evo_tradeoff:g}", args.evo_start)):
    m_eval, m_train = evo(start), evo(start)
    runs.append((name, "eval forward", eval_of(m_eval), m_eval))
    runs.append((name, "train step" + (" (captured)" if args.graph else ""), step_of(m_train), m_train))
times = [[] for _ in runs]
for r in range(args.rounds):
    for i, (_, _, fn, _) in enumerate(runs):
        times[i].append(timed(fn, r == 0))
for (name, what, _, m), t in zip(runs, times):
    ms, spread = sum(t) / len(t), max(t) - min(t)
    print(f"{mname:12s} {name:34s} {what:22s} {ms:7.2f} ms (spread {spread:.2f})  {B / ms * 1e3:8.0f} images/s   rows per block {m.tokens_per_block}",
          flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
