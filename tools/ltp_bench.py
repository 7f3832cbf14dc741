"""Training step time of the LTP baseline (--method ltp): DeiT-S 224, B = 128, stages at blocks 3 6 9, one optimiser
step per batch through TrainStep's logits-only route (cross entropy, no teacher, fused AdamW), seeded random weights unless a checkpoint is
given.  Measured next to each other, alternating in one process for --rounds rounds of 10 steps each:
  (a) the hard step with every threshold 0 (nothing leaves) against A-ViT with a gate centre so large that nothing halts: the same ragged
      blocks on every token - what differs is score + select + re-pack at 3 stages against the halting step + re-pack after 12 blocks;
  (b) the hard step at thresholds calibrated stage by stage to the median score of the live patches, so that every stage halves the batch
      and roughly half the token-blocks remain (random weights attend almost uniformly: no hand-set number would do);
  (c) the soft step (policy attention with a learnt policy in every block after the first stage) against the dense trunk's step (a Token
      Merging student with r = 0: the same logits-only route on dense blocks);
  (d) the score kernel's share of a stage block: ops.ltp_score alone on the full packed batch against one ragged block forward there.
Prints ms per step (mean over the rounds, with the spread between them), images/s and the rows of the packed batch in every block of the
last step - the figure means nothing without them.  GPU box only.
--bf16: the LTP rows and the dense trunk as train_bf16 students under GEMM_BF16 (--ltp-bf16; the dense trunk: the bf16 step of the r = 0
merging student), thresholds calibrated in that mode; with --also-fp32 the fp32 rows stay in the same run, alternating with them, and every
row prints the median of its rounds.  (d) then times the bf16 score kernel (the bf16 qkv, the bf16 varlen attention's log-sum-exp) against
that attention forward, next to the fp32 pair.

  python tools/ltp_bench.py [--gemm-mode exact|split] [--student-checkpoint deit_small.pth] [--rounds 3]
  python tools/ltp_bench.py --bf16 [--also-fp32]
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
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for every model (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--bf16", action="store_true", help="time the train_bf16 students under GEMM_BF16 (--ltp-bf16)")
ap.add_argument("--also-fp32", action="store_true", help="with --bf16: keep the fp32 rows in the same run")
args = ap.parse_args()
if args.also_fp32 and not args.bf16:
    raise SystemExit("--also-fp32 goes with --bf16")

dev = torch.device("cuda:0")
B, WARMUP, TIMED, LOCS = 128, 2, 10, (3, 6, 9)
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (B,), device=dev)
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def ltp(phase, theta, bf16=False):
    torch.manual_seed(0)
    m = vit_models.ltp_deit_small_patch16_224(pruning_loc=LOCS, ltp_phase=phase, checkpoint_path=args.student_checkpoint,
                                              **({"train_bf16": True} if bf16 else {}))
    with torch.no_grad():
        m.ltp_threshold.copy_(torch.tensor(theta, dtype=torch.float32))
    return m


def calibrate(bf16=False):
    """theta_k = the median score of the patches live at stage k, found stage by stage on the benchmark's own batch (eval forwards, in the
    arithmetic mode of the rows that use them)"""
    with ops.gemm_mode(ops.GEMM_BF16 if bf16 else mode):
        return _calibrate(bf16)


def _calibrate(bf16):
    theta = [0.0] * len(LOCS)
    m = ltp("hard", theta, bf16).to(dev).eval()
    for k in range(len(LOCS)):
        with torch.no_grad():
            m(x)
            s = m.ltp_scores[k]
            cu = torch.nn.functional.pad(torch.tensor(m.tokens_per_block_counts[LOCS[k]].tolist(), device=dev).cumsum(0), (1, 0))
            patch = torch.ones_like(s, dtype=torch.bool)
            patch[cu[:-1]] = False
            theta[k] = float(s[patch].median())
            m.ltp_threshold.copy_(torch.tensor(theta, dtype=torch.float32))
    return theta


def step_of(model, bf16=False):
    """the step and the arithmetic mode it is built and called in (a train_bf16 student under GEMM_BF16)"""
    a = types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, step=0, ltp_lambda=0.01)
    m = ops.GEMM_BF16 if bf16 else mode
    with ops.gemm_mode(m):
        return TrainStep(model.to(dev).train(), None, a, lr=1e-5, graph=False), m


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


steps = []
for bf16 in ([False] if not args.bf16 else [False, True] if args.also_fp32 else [True]):      # fp32 rows first when both are timed
    tag = " bf16" if bf16 else " fp32" if args.bf16 else ""
    half = calibrate(bf16)
    print(f"calibrated thresholds{tag} (median of the live patches' scores, stage by stage): {[round(t, 6) for t in half]}", flush=True)
    torch.manual_seed(0)
    if not args.bf16:
        steps.append(("(a) avit, nothing halts", step_of(vit_models.avit_deit_small_patch16_224(gate_scale=10.0, gate_center=1e4,
                                                                                                checkpoint_path=args.student_checkpoint))))
    steps += [("(a) ltp hard, thresholds 0" + tag, step_of(ltp("hard", [0.0] * len(LOCS), bf16), bf16)),
              ("(b) ltp hard, calibrated thresholds" + tag, step_of(ltp("hard", half, bf16), bf16)),
              ("(c) dense trunk (tome r = 0)" + tag,
               step_of(vit_models.tome_deit_small_patch16_224(0, checkpoint_path=args.student_checkpoint,
                                                              **({"train_merge": True, "train_bf16": True} if bf16 else {})), bf16)),
              ("(c) ltp soft" + tag, step_of(ltp("soft", half, bf16), bf16))]
times = [[] for _ in steps]
for r in range(args.rounds):
    for i, (_, (ts, m)) in enumerate(steps):
        with ops.gemm_mode(m):
            times[i].append(timed(lambda: ts(x, y), r == 0))
for (name, (ts, _)), t in zip(steps, times):
    ms, spread = statistics.median(t) if args.bf16 else sum(t) / len(t), max(t) - min(t)      # --bf16: the median of the rounds
    line = f"{mname if not args.bf16 else '':12s} {name:{43 if args.bf16 else 38}s} {ms:7.2f} ms/step (spread {spread:.2f})  {B / ms * 1e3:8.0f} images/s"
    rows = getattr(ts.student, "tokens_per_block", None) or getattr(ts.student, "tokens_per_layer", None)
    if rows:
        line += f"   rows per block {list(rows)}"
    print(line, flush=True)

# (d) the score kernel against one ragged block forward on the full packed batch
m = ltp("hard", [0.0] * len(LOCS)).to(dev).eval()
blk = m.blocks[LOCS[0]]
n, D, H = 197, 384, blk.attn.num_heads
xp = torch.randn(B * n, D, device=dev)
cu = (torch.arange(B + 1, dtype=torch.int32, device=dev) * n).contiguous()
qkv = torch.randn(B * n, 3 * D, device=dev)
mean = lambda t: sum(t) / len(t)
with torch.no_grad():
    _, lse, _ = ops.attn_varlen_fwd_lse(qkv, cu, B, B * n, n, H, blk.attn.scale)
    t_block, t_attn, t_score = [], [], []
    for r in range(args.rounds):
        t_block.append(timed(lambda: blk.forward_ragged(xp, cu, B, n), r == 0))
        t_attn.append(timed(lambda: ops.attn_varlen_fwd_lse(qkv, cu, B, B * n, n, H, blk.attn.scale), r == 0))
        t_score.append(timed(lambda: ops.ltp_score(qkv, lse, B, n, H, blk.attn.scale, cu=cu, total=B * n), r == 0))
print(f"{mname:12s} (d) ragged block forward {mean(t_block) * 1e3:7.1f} us, its attention {mean(t_attn) * 1e3:7.1f} us, "
      f"ltp_score {mean(t_score) * 1e3:7.1f} us = {100 * mean(t_score) / mean(t_block):.1f} % of the block, "
      f"{100 * mean(t_score) / mean(t_attn):.1f} % of its attention (B {B}, n {n}, H {H})", flush=True)
if args.bf16:
    qkv16 = qkv.bfloat16().contiguous()
    with torch.no_grad(), ops.gemm_mode(ops.GEMM_BF16):
        _, lse16, _, _ = ops.attn_varlen_fwd_lse_bf16io(qkv16, cu, B, B * n, n, H, blk.attn.scale)
        t_block16, t_attn16, t_score16 = [], [], []
        for r in range(args.rounds):
            t_block16.append(timed(lambda: blk.forward_ragged(xp, cu, B, n), r == 0))
            t_attn16.append(timed(lambda: ops.attn_varlen_fwd_lse_bf16io(qkv16, cu, B, B * n, n, H, blk.attn.scale), r == 0))
            t_score16.append(timed(lambda: ops.ltp_score(qkv16, lse16, B, n, H, blk.attn.scale, cu=cu, total=B * n), r == 0))
    med = statistics.median
    print(f"{'bf16':12s} (d) ragged block forward {med(t_block16) * 1e3:7.1f} us, its attention (LSE form) {med(t_attn16) * 1e3:7.1f} us, "
          f"ltp_score {med(t_score16) * 1e3:7.1f} us = {100 * med(t_score16) / med(t_block16):.1f} % of the block, "
          f"{100 * med(t_score16) / med(t_attn16):.1f} % of its attention, {100 * med(t_score16) / med(t_score):.1f} % of the fp32 score "
          f"kernel ({med(t_score) * 1e3:.1f} us)  (medians of {args.rounds} rounds; B {B}, n {n}, H {H})", flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
