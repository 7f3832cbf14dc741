"""Inference throughput of the Token Merging baseline (--method tome): eval mode, forward only, DeiT-S 224, B = 128, fp32
exact GEMMs, seeded random weights, r in {0, 8, 13, 16} tokens merged per block, next to VisionTransformerTeacher.forward on the same
weights in the same process.  Every configuration is warmed up at its own shapes; the timed rounds alternate between the configurations
(so that a neighbour's load on the machine hits them alike), each round is a window of --iters forwards between two device events, and
the table reports the median images/s with the lowest and highest round.  GPU box only.

--train: the same table for training through the merges (--tome-train): ms per d2s.engine.TrainStep call (forward, ToMeLoss without a
teacher - dist_weight 0 -, backward, fused AdamW) of a train_merge student, hard labels, same alternating rounds; read every row against
the r = 0 row of the same run.  --train --bf16: the steps of train_bf16 students under GEMM_BF16 (--tome-train-bf16); with --also-fp32
the fp32 steps stay in the same run, each step called under its own arithmetic mode.

--bf16: the same table with bf16=True models (--tome-bf16: the merging trunk on the bf16 data path) and the teacher row timed under
GEMM_BF16; --bf16 --also-fp32 keeps the fp32 rows in the same run, so that each bf16 row is read against the fp32 row of equal r.

  python tools/tome_bench.py [--rounds 5] [--iters 10] [--r 0 8 13 16] [--train] [--bf16 [--also-fp32]]
  python tools/tome_bench.py --train --bf16 --also-fp32      (training through the merges: bf16 rows against fp32 rows of equal r)
  rocprofv3 --kernel-trace --stats -d DIR -o tome -- python tools/tome_bench.py --no-teacher --r 13 --rounds 1      (kernel shares)
  rocprofv3 --kernel-trace --stats -d DIR -o tome -- python tools/tome_bench.py --bf16 --no-teacher --r 13 --rounds 1      (... on the bf16 data path)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tome -- python tools/tome_bench.py --train --r 13 --rounds 1     (... of a train step)
"""
import argparse
import os
import statistics
import sys
import types

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
ap.add_argument("--train", action="store_true", help="time a TrainStep of a train_merge student (no teacher, dist_weight 0) instead of the eval forward")
ap.add_argument("--bf16", action="store_true", help="bf16=True models (the bf16 data path); the teacher row runs under GEMM_BF16")
ap.add_argument("--also-fp32", action="store_true", help="with --bf16: keep the fp32 rows in the same run")
args = ap.parse_args()
if args.also_fp32 and not args.bf16:
    raise SystemExit("--also-fp32 goes with --bf16")
if not torch.cuda.is_available():
    raise SystemExit("tools/tome_bench.py needs a GPU: nothing here is measured on the CPU")

dev = torch.device("cuda:0")
ops.set_gemm_mode(ops.GEMM_EXACT)
B = 128
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
teacher = vit_models.dynamic_vit_small_patch16_224_teacher().to(dev).eval()
weights = teacher.state_dict()
if args.train:
    from d2s.engine import TrainStep
    y = torch.randint(0, 1000, (B,), device=dev)
    steps = []
    for bf16 in ([False] if not args.bf16 else [False, True] if args.also_fp32 else [True]):      # fp32 rows first when both are timed
        tag = " bf16" if bf16 else " fp32" if args.bf16 else ""
        for r in args.r:
            m = vit_models.tome_deit_small_patch16_224(r, train_merge=True, **({"train_bf16": True} if bf16 else {}))
            m.load_state_dict(weights)
            with ops.gemm_mode(ops.GEMM_BF16 if bf16 else ops.GEMM_EXACT):
                step = TrainStep(m.to(dev), None, types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, step=0))
            step.bench_mode = ops.GEMM_BF16 if bf16 else ops.GEMM_EXACT
            steps.append((f"tome r = {r}{tag}", step))
    del teacher

    def train_window(step, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with ops.gemm_mode(step.bench_mode):              # every step under its own arithmetic mode
            s.record()
            for _ in range(iters):
                step(x, y)
            e.record()
            torch.cuda.synchronize()
        return s.elapsed_time(e) / iters

    for _, step in steps:
        train_window(step, 3)                             # warm-up at this configuration's own shapes
    ms = {name: [] for name, _ in steps}
    for _ in range(args.rounds):
        for name, step in steps:
            ms[name].append(train_window(step, args.iters))
    gemms = "fp32 exact GEMMs" if not args.bf16 else "bf16 data path and fp32 exact GEMMs" if args.also_fp32 else "bf16 data path"
    print(f"DeiT-S 224, B = {B}, {gemms}, TrainStep (no teacher, dist_weight 0), {args.rounds} rounds x {args.iters} steps per "
          "configuration, rounds alternating")
    print(f"{'configuration':21s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'images/s (median)':>18s} {'min':>8s} {'max':>8s}   tokens leaving each block")
    for name, step in steps:
        t = sorted(ms[name])
        rate = sorted(B / v * 1e3 for v in t)
        print(f"{name:21s} {statistics.median(t):9.2f} {t[0]:8.2f} {t[-1]:8.2f} {statistics.median(rate):18.0f} {rate[0]:8.0f} {rate[-1]:8.0f}   "
              f"{' '.join(map(str, step.student.tokens_per_block))}", flush=True)
    sys.exit(0)

class TeacherBf16:
    """the teacher forward under GEMM_BF16 (a bf16=True merging model enters that mode itself)"""

    def __call__(self, x):
        with ops.gemm_mode(ops.GEMM_BF16):
            return teacher(x)


# (row name, model, called as); fp32 rows first when both data paths are timed
paths = ([False] if not args.bf16 else [False, True] if args.also_fp32 else [True])
configs = []
for bf16 in paths:
    tag = " bf16" if bf16 else " fp32" if args.bf16 else ""
    if not args.no_teacher:
        configs.append((f"teacher forward{tag}", teacher, TeacherBf16() if bf16 else teacher))
    for r in args.r:
        m = vit_models.tome_deit_small_patch16_224(r, bf16=bf16)
        m.load_state_dict(weights)
        m = m.to(dev).eval()
        configs.append((f"tome r = {r}{tag}", m, m))


def window(model, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        model(x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


with torch.no_grad():
    for _, _, run in configs:
        window(run, 3)                                # warm-up at this configuration's own shapes
    ms = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, _, run in configs:
            ms[name].append(window(run, args.iters))

gemms = "fp32 exact GEMMs" if not args.bf16 else "bf16 data path and fp32 exact GEMMs" if args.also_fp32 else "bf16 data path"
print(f"DeiT-S 224, B = {B}, {gemms}, {args.rounds} rounds x {args.iters} forwards per configuration, rounds alternating")
print(f"{'configuration':21s} {'ms/batch':>9s} {'images/s (median)':>18s} {'min':>8s} {'max':>8s}   tokens leaving each block")
for name, model, _ in configs:
    rate = sorted(B / t * 1e3 for t in ms[name])
    tokens = getattr(model, "tokens_per_block", None) or [197] * 12
    print(f"{name:21s} {statistics.median(ms[name]):9.2f} {statistics.median(rate):18.0f} {rate[0]:8.0f} {rate[-1]:8.0f}   "
          f"{' '.join(map(str, tokens))}", flush=True)
