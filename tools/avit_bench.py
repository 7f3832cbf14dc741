"""Training step time of the A-ViT baseline (--method avit): DeiT-S 224, B = 128, one optimiser step per batch
through TrainStep's logits-only route (cross entropy, the two penalty terms, no teacher, fused AdamW), seeded random weights unless a
checkpoint is given.  Measured next to each other, alternating in one process for --rounds rounds of 10 steps each:
  * the Adaptive Token Sampling student trained through a stage in block 0 with K = 196 (--method ats --ats-train): every later block is the
    same ragged block, with the few tokens that stage drops gone;
  * A-ViT with a gate centre so large that nothing halts (--no-halt-center): the same ragged blocks on every token, plus the halting step,
    the re-pack and the host read after each of the 12 blocks - the cost of the halting machinery;
  * A-ViT at every --gate-center given: the step with tokens leaving the batch.
Prints ms per step (mean over the rounds, with the spread between them), images/s, and for A-ViT the average depth and the rows of the
packed batch in every block of the last step - the figure means nothing without them.  GPU box only.

  python tools/avit_bench.py [--gemm-mode exact|split] [--gate-scale 10] [--gate-center C ...] [--student-checkpoint deit_small.pth]
  python tools/avit_bench.py --probe --gate-center C1 C2 ...      (one eval forward per centre: average depth and rows per block, no timing)
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

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES), default="exact")
ap.add_argument("--gate-scale", type=float, default=10.0)
ap.add_argument("--gate-center", type=float, nargs="+", default=[30.0], help="one A-ViT run per centre")
ap.add_argument("--no-halt-center", type=float, default=1e4, help="the centre of the run in which nothing halts")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for every model (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--probe", action="store_true", help="no timing: one eval forward per --gate-center, average depth and rows per block")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 2, 10
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def avit(center):
    torch.manual_seed(0)
    return vit_models.avit_deit_small_patch16_224(gate_scale=args.gate_scale, gate_center=center, checkpoint_path=args.student_checkpoint)


if args.probe:
    for c in args.gate_center:
        m = avit(c).to(dev).eval()
        with torch.no_grad():
            m(x)
        print(f"gate scale {args.gate_scale:g} centre {c:g}: average depth {float(m.avg_depth):.2f}, rows per block {m.tokens_per_layer}", flush=True)
    sys.exit(0)


def step_of(model):
    a = types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, step=0)
    return TrainStep(model.to(dev).train(), None, a, lr=1e-5, graph=False)


def timed(ts, warm):
    for _ in range(WARMUP if warm else 0):
        ts(x, y)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(TIMED):
        ts(x, y)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / TIMED


torch.manual_seed(0)
steps = [("ats stage in block 0, K = 196", step_of(vit_models.ats_deit_small_patch16_224(ats_locs=[0], ats_tokens=196, train_sample=True,
                                                                                         checkpoint_path=args.student_checkpoint))),
         (f"avit centre {args.no_halt_center:g} (nothing halts)", step_of(avit(args.no_halt_center)))]
for c in args.gate_center:
    steps.append((f"avit scale {args.gate_scale:g} centre {c:g}", step_of(avit(c))))
times = [[] for _ in steps]
for r in range(args.rounds):
    for i, (_, ts) in enumerate(steps):
        times[i].append(timed(ts, r == 0))
for (name, ts), t in zip(steps, times):
    ms, spread = sum(t) / len(t), max(t) - min(t)
    line = f"{mname:12s} {name:36s} {ms:7.2f} ms/step (spread {spread:.2f})  {B / ms * 1e3:8.0f} images/s"
    if ts.method.name == "avit":
        line += f"   average depth {float(ts.student.avg_depth):.2f}, rows per block {ts.student.tokens_per_layer}"
    else:
        line += f"   tokens after the stage: mean {float(ts.student.tokens_per_stage[0].float().mean()):.1f} of 196"
    print(line, flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
