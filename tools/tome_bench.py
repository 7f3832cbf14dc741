"""Inference throughput of the Token Merging baseline (--method tome): eval mode, forward only, DeiT-S 224, B = 128, fp32
exact GEMMs, seeded random weights, r in {0, 8, 13, 16} tokens merged per block, next to VisionTransformerTeacher.forward on the same
weights in the same process.  Every configuration is warmed up at its own shapes; the timed rounds alternate between the configurations
(so that a neighbour's load on the machine hits them alike), each round is a window of --iters forwards between two device events, and
the table reports the median images/s with the lowest and highest round.  GPU box only.

  python tools/tome_bench.py [--rounds 5] [--iters 10] [--r 0 8 13 16]
  rocprofv3 --kernel-trace --stats -d DIR -o tome -- python tools/tome_bench.py --no-teacher --r 13 --rounds 1      (kernel shares)
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
import vit_models
from d2s import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--r", type=int, nargs="+", default=[0, 8, 13, 16])
ap.add_argument("--no-teacher", action="store_true", help="leave the teacher forward out (a kernel trace of one merging configuration alone)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/tome_bench.py needs a GPU: nothing here is measured on the CPU")

dev = torch.device("cuda:0")
ops.set_gemm_mode(ops.GEMM_EXACT)
B = 128
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
teacher = vit_models.dynamic_vit_small_patch16_224_teacher().to(dev).eval()
weights = teacher.state_dict()
configs = [] if args.no_teacher else [("teacher forward", teacher)]
for r in args.r:
    m = vit_models.tome_deit_small_patch16_224(r)
    m.load_state_dict(weights)
    configs.append((f"tome r = {r}", m.to(dev).eval()))


def window(model, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        model(x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


with torch.no_grad():
    for _, model in configs:
        window(model, 3)                              # warm-up at this configuration's own shapes
    ms = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, model in configs:
            ms[name].append(window(model, args.iters))

print(f"DeiT-S 224, B = {B}, fp32 exact GEMMs, {args.rounds} rounds x {args.iters} forwards per configuration, rounds alternating")
print(f"{'configuration':16s} {'ms/batch':>9s} {'images/s (median)':>18s} {'min':>8s} {'max':>8s}   tokens leaving each block")
for name, model in configs:
    rate = sorted(B / t * 1e3 for t in ms[name])
    tokens = getattr(model, "tokens_per_block", None) or [197] * 12
    print(f"{name:16s} {statistics.median(ms[name]):9.2f} {statistics.median(rate):18.0f} {rate[0]:8.0f} {rate[-1]:8.0f}   "
          f"{' '.join(map(str, tokens))}", flush=True)
