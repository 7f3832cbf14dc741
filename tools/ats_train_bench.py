"""Training step time of the Adaptive Token Sampling baseline trained through its stages (--method ats --ats-train)
next to the same trunk without a stage: DeiT-S 224, B = 128, a sampling stage in each of blocks 3-11 with K = 196 / 98 / 49, one optimiser
step per batch through TrainStep's logits-only route (cross entropy, no teacher, fused AdamW), seeded random weights unless a checkpoint is
given.  The no-stage trunk is the same DeiT-S through the same route (VisionTransformerToMe with r = 0: the dense differentiable trunk,
BlockFn's composite blocks - what VisionTransformerATS(ats_locs=()) runs in training mode).  The models alternate in one process for
--rounds rounds of 10 steps each; prints ms per step (mean over the rounds, with the spread between them), images/s and, for ATS, the mean
number of tokens (CLS not counted) that leave every stage in the last step - the figure means nothing without it.  GPU box only.
--bf16: the same rows as train_bf16 students under GEMM_BF16 (--ats-train-bf16; the dense trunk: the bf16 step of the r = 0 merging
student); with --also-fp32 the fp32 rows stay in the same run, alternating with them, and every row prints the median of its rounds.

  python tools/ats_train_bench.py [--gemm-mode exact|split] [--ats-tokens 196 98 49] [--student-checkpoint deit_small.pth]
  python tools/ats_train_bench.py --bf16 [--also-fp32]
  python tools/ats_train_bench.py --kernels        (under rocprofv3 --kernel-trace --stats: the three varlen attention-backward launches on
                                                    128 images of 197 rows next to d2s_attn_bwd_f32 on the same data, alternating)
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
from d2s.engine import TrainStep

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES), default="exact")
ap.add_argument("--ats-locs", type=int, nargs="+", default=list(range(3, 12)))
ap.add_argument("--ats-tokens", type=int, nargs="+", default=[196, 98, 49], help="one run per K")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for every model (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernels", action="store_true", help="only the attention-backward kernels, varlen next to dense at equal length")
ap.add_argument("--bf16", action="store_true", help="time the train_bf16 students under GEMM_BF16 (--ats-train-bf16)")
ap.add_argument("--also-fp32", action="store_true", help="with --bf16: keep the fp32 rows in the same run")
args = ap.parse_args()
if args.also_fp32 and not args.bf16:
    raise SystemExit("--also-fp32 goes with --bf16")

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 2, 10
torch.manual_seed(0)

if args.kernels:
    n, H, reps = 197, 6, 20
    qkv = torch.randn(B * n, 3 * H * 64, device=dev)
    dout = torch.randn(B * n, H * 64, device=dev)
    cu = (torch.arange(B + 1, dtype=torch.int32) * n).to(dev)
    out, lse, _ = ops.attn_fwd(qkv, B, n, H, 0.125, want_cls=False)
    out_v, lse_v, _ = ops.attn_varlen_fwd_lse(qkv, cu, B, B * n, n, H, 0.125)
    for _ in range(reps):
        a = ops.attn_bwd(qkv, out, dout, lse, B, n, H, 0.125)
        b = ops.attn_varlen_bwd(qkv, cu, out_v, dout, lse_v, B, B * n, n, H, 0.125)
    torch.cuda.synchronize()
    print(f"{reps} x (d2s_attn_bwd_f32, d2s_attn_varlen_bwd_f32) on {B} x {n} rows, H = {H}: results bit-identical: {torch.equal(a, b)}")
    sys.exit(0)

x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def step_of(model, bf16=False):
    """the step and the arithmetic mode it is built and called in (a train_bf16 student under GEMM_BF16)"""
    a = types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, step=0)
    m = ops.GEMM_BF16 if bf16 else mode
    with ops.gemm_mode(m):
        return TrainStep(model.to(dev).train(), None, a, lr=1e-5, graph=False), m


def timed(step, warm):
    ts, m = step
    with ops.gemm_mode(m):
        return _timed(ts, warm)


def _timed(ts, warm):
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


steps = []
for bf16 in ([False] if not args.bf16 else [False, True] if args.also_fp32 else [True]):      # fp32 rows first when both are timed
    tag = " bf16" if bf16 else " fp32" if args.bf16 else ""
    kw = {"train_bf16": True} if bf16 else {}
    torch.manual_seed(0)
    steps.append(("no stage (dense trunk)" + tag,
                  step_of(vit_models.tome_deit_small_patch16_224(0, checkpoint_path=args.student_checkpoint,
                                                                 **({"train_merge": True, "train_bf16": True} if bf16 else {})), bf16)))
    for K in args.ats_tokens:
        torch.manual_seed(0)
        steps.append((f"ats @ blocks {args.ats_locs[0]}-{args.ats_locs[-1]} K = {K:3d}" + tag,
                      step_of(vit_models.ats_deit_small_patch16_224(ats_locs=args.ats_locs, ats_tokens=K, train_sample=True,
                                                                    checkpoint_path=args.student_checkpoint, **kw), bf16)))
times = [[] for _ in steps]
for r in range(args.rounds):
    for i, (_, step) in enumerate(steps):
        times[i].append(timed(step, r == 0))
for (name, (ts, _)), t in zip(steps, times):
    ms, spread = statistics.median(t) if args.bf16 else sum(t) / len(t), max(t) - min(t)      # --bf16: the median of the rounds
    line = f"{mname if not args.bf16 else '':12s} {name:35s} {ms:7.2f} ms/step (spread {spread:.2f})  {B / ms * 1e3:8.0f} images/s"
    if ts.method.name == "ats":
        per = [c.float() for c in ts.student.tokens_per_stage]
        line += f"   tokens per stage: mean {[round(float(c.mean()), 1) for c in per]} min {[int(c.min()) for c in per]} max {[int(c.max()) for c in per]}"
    print(line, flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
