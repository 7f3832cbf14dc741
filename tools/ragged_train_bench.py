"""Training step time of the dynamic keep ratio trained on the ragged packed batch (--patch-score-threshold --ragged-train, DESIGN.md
section 10.2) next to the policy-mode step on the same weights and batches: DeiT-S 224, B = 128, one optimiser step per batch through
TrainStep (both losses, the dense teacher, fused AdamW), seeded random weights unless checkpoints are given.  With a fresh predictor the
scores are near uniform, so a threshold t drops about the fraction t of the tokens at a stage.  The two steps alternate in one process for
--rounds rounds of 10 steps each; prints ms per step (mean over the rounds, with the spread between them), images/s, the mean kept
fraction after every stage in the last step - the figure means nothing without it - and the host reads per step (one per stage).  With one
stage it also prints the policy-versus-ragged differences of the first step's logits and gradient norms (recorded, not asserted: policy
attention carries eps terms the ragged definition does not have).  GPU box only.

--bf16: the policy-mode step in the bf16 arithmetic mode - how a threshold student trains in bf16 without
--ragged-bf16 - and the ragged step in that mode (ragged_bf16=True) alternate the same way, with the fp32 ragged step of --gemm-mode
beside them for orientation (every step runs in its own arithmetic mode, set before each of its timed blocks).

  python tools/ragged_train_bench.py [--gemm-mode exact|split] [--pruning-locs 3] [--threshold 0.5]
  python tools/ragged_train_bench.py --pruning-locs 3 6 9 --threshold 0.3
  python tools/ragged_train_bench.py --bf16 [--pruning-locs 3] [--threshold 0.5]
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
ap.add_argument("--pruning-locs", type=int, nargs="+", default=[3])
ap.add_argument("--threshold", type=float, default=0.5)
ap.add_argument("--batch-size", type=int, default=128)
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for both students (default: seeded random weights)")
ap.add_argument("--teacher-checkpoint", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--bf16", action="store_true", help="policy-mode step and ragged step in the bf16 arithmetic mode, the fp32 ragged step beside them")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, WARMUP, TIMED = args.batch_size, 2, 10
S = len(args.pruning_locs)
ratios = [round(0.7 ** (s + 1), 3) for s in range(S)]          # the keep_ratios list only sizes the per-stage metrics on this path
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def step_of(ragged, step_mode=mode):
    ops.set_gemm_mode(step_mode)
    torch.manual_seed(0)                                        # the same initial weights for both students
    kw = {"ragged_train": True} if ragged else {}
    if ragged and step_mode == ops.GEMM_BF16:
        kw["ragged_bf16"] = True
    student = vit_models.dynamic_vit_small_patch16_224_student(args.pruning_locs, ratios, topk_selection=True, predictor_loss_type="kl_div",
                                                               patch_score_threshold=args.threshold, checkpoint_path=args.student_checkpoint,
                                                               **kw)
    torch.manual_seed(1)
    teacher = vit_models.dynamic_vit_small_patch16_224_teacher(checkpoint_path=args.teacher_checkpoint)
    a = types.SimpleNamespace(keep_ratios=ratios, mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=args.threshold, step=0,
                              ragged_train=ragged)
    ts = TrainStep(student.to(dev).train(), teacher.to(dev), a, lr=1e-5, graph=False)
    ts.bench_mode = step_mode
    return ts


def grad_norms(ts):
    """L2 norm of the gradient arena per top-level module, after a step"""
    out = {}
    for n, p in ts.student.named_parameters():
        g = ops.grad_buffer(p)                                  # its slice of the gradient arena: still this step's gradient
        key = n.split(".")[0] + ("." + n.split(".")[1] if n.startswith(("blocks.", "score_predictor.")) else "")
        out[key] = out.get(key, 0.0) + float(g.double().pow(2).sum())
    return {k: v ** 0.5 for k, v in out.items()}


def timed(ts, warm):
    ops.set_gemm_mode(ts.bench_mode)
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


if args.bf16:
    steps = [("bf16: policy attention (all N tokens)", step_of(False, ops.GEMM_BF16)), ("bf16: ragged packed batch", step_of(True, ops.GEMM_BF16)),
             (f"{mname}: ragged packed batch", step_of(True))]
else:
    steps = [("policy attention (all N tokens)", step_of(False)), ("ragged packed batch", step_of(True))]
if S == 1:      # the first step of the first two, on identical weights: how far apart the two definitions are
    infos = []
    for _, ts in steps[:2]:
        ops.set_gemm_mode(ts.bench_mode)
        infos.append(ts(x, y))
    torch.cuda.synchronize()
    la, lb = (i["logits_s"].detach().double() for i in infos)
    print(f"one stage, first step, policy vs ragged: loss {float(infos[0]['loss']):.6f} vs {float(infos[1]['loss']):.6f}, "
          f"max |logits difference| {float((la - lb).abs().max()):.3e} (max |logit| {float(la.abs().max()):.3e}), "
          f"masks equal: {all(torch.equal(a, b) for a, b in zip(infos[0]['kept'], infos[1]['kept']))}")
    na, nb = (grad_norms(ts) for _, ts in steps[:2])
    worst = max(na, key=lambda k: abs(na[k] - nb.get(k, 0.0)) / max(na[k], 1e-30))
    print(f"  gradient norms per module: largest relative difference {abs(na[worst] - nb[worst]) / max(na[worst], 1e-30):.3e} at {worst} "
          f"({na[worst]:.6e} vs {nb[worst]:.6e})")
times = [[] for _ in steps]
for r in range(args.rounds):
    for i, (_, ts) in enumerate(steps):
        times[i].append(timed(ts, r == 0))
for (name, ts), t in zip(steps, times):
    ms, spread = sum(t) / len(t), max(t) - min(t)
    line = f"{mname if not args.bf16 else 'bf16 bench':12s} locs {args.pruning_locs} t {args.threshold}  {name:38s} {ms:7.2f} ms/step (spread {spread:.2f}; rounds {[round(v, 2) for v in t]})  {B / ms * 1e3:7.0f} images/s"
    kept = [float(m.mean()) for m in ts.student.kept_token_indices]
    line += f"   mean kept fraction per stage {[round(k, 3) for k in kept]}, host reads per step {S if ts.ragged_train else 0}"
    print(line, flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
