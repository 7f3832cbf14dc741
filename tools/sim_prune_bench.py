"""The similarity stage after attention ranking (--sim-prune R): what it costs.  GPU box only.
  (a) the stage call: ops.key_metric on the block's qkv plus ops.sim_prune on the c = k + R candidates, for (B 128, H 6, n 197, k 98) and
      (B 64, H 12, n 577, k 288) at R 8 and 32, each part alone as well, next to ops.tome_match on a qkv of n = c + 1 tokens (the same
      number of 64-term pair scores, its metric computed inside) and d2s_select_cls_attn for the c candidates - alternating for --rounds
      rounds of 20 calls each; median and range of the rounds.
      Expectation, written down before the first run: the stage call (metric + stage) is no slower than tome_match beyond the spread of
      that kernel's own rounds - it reads the keys of all n tokens, not of c + 1, but spreads the match over (A tile, image) workgroups on
      the matrix pipe where tome_match runs one workgroup per image on the vector units.
  (b) the model: the eval forward of DeiT-S 224 at batch 128, one stage at block 3 that keeps half the patches, the same seeded weights
      in every row - --attn-selection, with --sim-prune 16, with --graph-rank 5, with both - alternating in the same way.

  python tools/sim_prune_bench.py [--rounds 7] [--gemm-mode exact|split] [--student-checkpoint deit_small.pth]
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

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES), default="exact")
ap.add_argument("--student-checkpoint", default=None, help="DeiT-S weights for every model (default: seeded random weights)")
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()

dev = torch.device("cuda:0")
WARMUP = 3
mode, mname = MODES[args.gemm_mode]
ops.set_gemm_mode(mode)


def timed(fn, warm, calls):
    for _ in range(WARMUP if warm else 0):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def alternate(rows, calls):
    """rows: [(name, fn)] -> {name: the per-call ms of every round}, the rows taking turns inside every round"""
    times = {name: [] for name, _ in rows}
    for r in range(args.rounds):
        for name, fn in rows:
            times[name].append(timed(fn, r == 0, calls))
    return times


def show(name, t, unit=1e3, what="us"):
    print(f"  {name:34s} median {statistics.median(t) * unit:9.1f} {what}  (range {min(t) * unit:.1f} .. {max(t) * unit:.1f})", flush=True)


# ---- (a) the stage call ----
for B, H, n, k in ((128, 6, 197, 98), (64, 12, 577, 288)):
    torch.manual_seed(0)
    T = n - 1
    qkv = torch.randn(B * n, 3 * H * 64, device=dev)
    _, _, cls_row = ops.attn_fwd(qkv, B, n, H, 0.125, True)
    metric = ops.key_metric(qkv, B, n, H)
    rows = []
    for R in (8, 32):
        c = k + R
        probs, cand, _ = ops.select_cls_attn(cls_row, 1, T, c)
        small = qkv[:B * (c + 1)].contiguous()                                    # a qkv of c + 1 tokens per image for tome_match

        def stage(R=R, probs=probs, cand=cand):
            return ops.sim_prune(ops.key_metric(qkv, B, n, H), probs, cand, 1, R)
        rows += [(f"R={R}: key_metric + sim_prune", stage),
                 (f"R={R}: sim_prune alone", (lambda R=R, probs=probs, cand=cand: ops.sim_prune(metric, probs, cand, 1, R))),
                 (f"R={R}: tome_match n={c + 1}", (lambda R=R, small=small, c=c: ops.tome_match(small, B, c + 1, H, R))),
                 (f"R={R}: select_cls_attn c={c}", (lambda c=c: ops.select_cls_attn(cls_row, 1, T, c)))]
    rows += [("key_metric alone", lambda: ops.key_metric(qkv, B, n, H)), (f"select_cls_attn k={k}", lambda: ops.select_cls_attn(cls_row, 1, T, k))]
    with torch.no_grad():
        t = alternate(rows, 20)
    print(f"(a) B {B}, H {H}, n {n}, k {k} ({args.rounds} alternating rounds of 20 calls; operator calls, allocations included)")
    for name, _ in rows:
        show(name, t[name])

# ---- (b) the model ----
B = 128
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)


def student(**kw):
    torch.manual_seed(0)
    m = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                         checkpoint_path=args.student_checkpoint, attn_selection=True, **kw)
    return m.to(dev).eval()


models = [("--attn-selection", student()), ("--sim-prune 16", student(sim_prune=16)), ("--graph-rank 5", student(graph_rank_iters=5)),
          ("--graph-rank 5 --sim-prune 16", student(graph_rank_iters=5, sim_prune=16))]
with torch.no_grad():
    t = alternate([(name, (lambda m=m: m(x))) for name, m in models], 10)
print(f"(b) DeiT-S 224 eval forward, batch {B}, one stage at block 3, keep 0.5, {mname} ({args.rounds} alternating rounds of 10 forwards)")
base = statistics.median(t["--attn-selection"])
for name, _ in models:
    show(name, t[name], unit=1.0, what="ms")
    print(f"  {'':34s} {B / statistics.median(t[name]) * 1e3:9.0f} images/s, {statistics.median(t[name]) - base:+.3f} ms against --attn-selection", flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
