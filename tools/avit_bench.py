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
--bf16: the same rows as train_bf16 students under GEMM_BF16 (--avit-bf16, --ats-train-bf16) and the dense bf16 step (the r = 0 merging
student) beside them; with --also-fp32 the fp32 rows stay in the same run, alternating with them; every row prints the median of its
rounds.  --boundary: the fused block-boundary backward alone (hip events) against the chain it replaces - d2s_ragged_repack_bwd, then
d2s_avit_halt_bwd, then the cast a block does when it finds no bf16 form of its gy - on B images of 197 rows, half of the tokens kept.

  python tools/avit_bench.py [--gemm-mode exact|split] [--gate-scale 10] [--gate-center C ...] [--student-checkpoint deit_small.pth]
  python tools/avit_bench.py --bf16 [--also-fp32] [--gate-center C ...]
  python tools/avit_bench.py --boundary
  python tools/avit_bench.py --probe --gate-center C1 C2 ...      (one eval forward per centre: average depth and rows per block, no timing)
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
ap.add_argument("--gate-scale", type=float, default=10.0)
ap.add_argument("--gate-center", type=float, nargs="+", default=[30.0], help="one A-ViT run per centre")
ap.add_argument("--no-halt-center", type=float, default=1e4, help="the centre of the run in which nothing halts")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for every model (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--probe", action="store_true", help="no timing: one eval forward per --gate-center, average depth and rows per block")
ap.add_argument("--bf16", action="store_true", help="time the train_bf16 students under GEMM_BF16 (--avit-bf16)")
ap.add_argument("--also-fp32", action="store_true", help="with --bf16: keep the fp32 rows in the same run")
ap.add_argument("--boundary", action="store_true", help="only the block-boundary backward: the fused launch against the chain it replaces")
args = ap.parse_args()
if args.also_fp32 and not args.bf16:
    raise SystemExit("--also-fp32 goes with --bf16")

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 2, 10
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def avit(center, **kw):
    torch.manual_seed(0)
    return vit_models.avit_deit_small_patch16_224(gate_scale=args.gate_scale, gate_center=center, checkpoint_path=args.student_checkpoint, **kw)


if args.boundary:
    n, D, L, layer, reps = 197, 384, 12, 6, 50
    total = B * n
    g = torch.Generator(device=dev).manual_seed(0)
    keep = (torch.rand(total, device=dev, generator=g) < 0.5).float()
    keep[::n] = 1.0
    counts = (keep.view(B, n)[:, 1:].sum(1)).int()
    cu = (torch.arange(B + 1, dtype=torch.int32) * n).to(dev)
    cu_new = ops.ragged_offsets(counts, extra=1)
    total_new = int(cu_new[-1])
    row_src = torch.arange(n, dtype=torch.int32, device=dev).repeat(B)
    st = ops.avit_state(B, n, D, L, dev)
    st["nh"].copy_(torch.where(keep.view(B, n) != 0, L, layer).int())
    st["ysave"].normal_(generator=g)
    h = torch.rand(total, device=dev, generator=g)
    w, dacc, ycls = torch.rand(B, device=dev, generator=g), torch.randn(B, D, device=dev, generator=g), torch.randn(B, D, device=dev, generator=g)
    gsc = 0.01 * torch.randn(L + 1, device=dev, generator=g)
    g_new = torch.randn(total_new, D, device=dev, generator=g)

    def chain():
        gy = ops.avit_halt_bwd(ops.ragged_repack_bwd(g_new, keep, cu, cu_new, total, B), h, cu, row_src, st, w, dacc, ycls, gsc, layer, 10.0)
        return gy, gy.bfloat16()

    def fused():
        return ops.avit_halt_repack_bwd_bf16io(g_new, keep, cu_new, h, cu, row_src, st, w, dacc, ycls, gsc, layer, 10.0)

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps * 1e3

    a, b = chain(), fused()
    same = torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    t = {"chain (repack_bwd, halt_bwd, cast)": [], "fused": []}
    for _ in range(max(args.rounds, 5)):
        t["chain (repack_bwd, halt_bwd, cast)"].append(window(chain))
        t["fused"].append(window(fused))
    print(f"block-boundary backward, {B} x {n} rows -> {total_new} kept, D = {D}, {reps} calls per window, windows alternating; "
          f"results bit-identical: {same}")
    for k, v in t.items():
        print(f"  {k:36s} {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})", flush=True)
    sys.exit(0)


if args.probe:
    for c in args.gate_center:
        m = avit(c).to(dev).eval()
        with torch.no_grad():
            m(x)
        print(f"gate scale {args.gate_scale:g} centre {c:g}: average depth {float(m.avg_depth):.2f}, rows per block {m.tokens_per_layer}", flush=True)
    sys.exit(0)


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
    if bf16:                                                 # the dense bf16 step: the r = 0 merging student on the same route
        steps.append(("dense trunk" + tag, step_of(vit_models.tome_deit_small_patch16_224(0, checkpoint_path=args.student_checkpoint,
                                                                                          train_merge=True, train_bf16=True), bf16)))
    steps.append(("ats stage in block 0, K = 196" + tag,
                  step_of(vit_models.ats_deit_small_patch16_224(ats_locs=[0], ats_tokens=196, train_sample=True,
                                                                checkpoint_path=args.student_checkpoint, **kw), bf16)))
    steps.append((f"avit centre {args.no_halt_center:g} (nothing halts)" + tag, step_of(avit(args.no_halt_center, **kw), bf16)))
    for c in args.gate_center:
        steps.append((f"avit scale {args.gate_scale:g} centre {c:g}" + tag, step_of(avit(c, **kw), bf16)))
times = [[] for _ in steps]
for r in range(args.rounds):
    for i, (_, step) in enumerate(steps):
        times[i].append(timed(step, r == 0))
for (name, (ts, _)), t in zip(steps, times):
    ms, spread = statistics.median(t) if args.bf16 else sum(t) / len(t), max(t) - min(t)      # --bf16: the median of the rounds
    line = f"{mname if not args.bf16 else '':12s} {name:41s} {ms:7.2f} ms/step (spread {spread:.2f})  {B / ms * 1e3:8.0f} images/s"
    if ts.method.name == "avit":
        line += f"   average depth {float(ts.student.avg_depth):.2f}, rows per block {ts.student.tokens_per_layer}"
    elif ts.method.name == "ats":
        line += f"   tokens after the stage: mean {float(ts.student.tokens_per_stage[0].float().mean()):.1f} of 196"
    print(line, flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
