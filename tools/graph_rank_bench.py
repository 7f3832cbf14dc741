"""Graph ranking (--graph-rank T): what the rank costs.  GPU box only.
  (a) the kernel: d2s_graph_rank_f32 at iters 1, 5 and 30 for (B 128, H 6, n 197) and (B 64, H 12, n 577), next to d2s_ltp_score_f32 on
      the same qkv and lse (one received-attention pass plus its head fold) and d2s_select_cls_attn on a row of the same shape (the
      stage's own launch, keep 0.5) - alternating for --rounds rounds of 20 calls each; median and range of the rounds, and the time of
      one further iteration, (t(30) - t(5)) / 25;
  (b) the model: the eval forward of DeiT-S 224 at batch 128, one stage at block 3 that keeps half the patches, the same seeded weights
      in every row - the score predictor, --attn-selection, --graph-rank 1, 5 and 30 - alternating in the same way.

  python tools/graph_rank_bench.py [--rounds 7] [--gemm-mode exact|split] [--student-checkpoint deit_small.pth]
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
WARMUP, ITERS = 3, (1, 5, 30)
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


# ---- (a) the kernel ----
for B, H, n in ((128, 6, 197), (64, 12, 577)):
    torch.manual_seed(0)
    scale = 0.125
    qkv = torch.randn(B * n, 3 * H * 64, device=dev)
    _, lse, cls_row = ops.attn_fwd(qkv, B, n, H, scale, True)
    rows = [(f"graph_rank iters={t}", (lambda t=t: ops.graph_rank(qkv, lse, B, n, H, scale, t))) for t in ITERS]
    rows += [("ltp_score (one pass + fold)", lambda: ops.ltp_score(qkv, lse, B, n, H, scale)),
             ("select_cls_attn (keep 0.5)", lambda: ops.select_cls_attn(cls_row, 1, n - 1, (n - 1) // 2))]
    with torch.no_grad():
        t = alternate(rows, 20)
    print(f"(a) B {B}, H {H}, n {n} ({args.rounds} alternating rounds of 20 calls; operator calls, allocations included)")
    for name, _ in rows:
        show(name, t[name])
    per = [(a - b) / (ITERS[2] - ITERS[1]) for a, b in zip(t[f"graph_rank iters={ITERS[2]}"], t[f"graph_rank iters={ITERS[1]}"])]
    show("one further iteration", per)
    # the share of the f32-input matrix pipe: 2 * 64 flop per P element over the kernel time
    print(f"  {'S = Q K^T of one iteration':34s} {2.0 * 64 * B * H * n * n / (statistics.median(per) * 1e-3) / 1e12:9.1f} TFLOP/s", flush=True)

# ---- (b) the model ----
B = 128
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)


def student(**kw):
    torch.manual_seed(0)
    m = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                         checkpoint_path=args.student_checkpoint, **kw)
    return m.to(dev).eval()


models = [("score predictor", student()), ("--attn-selection", student(attn_selection=True))]
models += [(f"--graph-rank {t}", student(attn_selection=True, graph_rank_iters=t)) for t in ITERS]
with torch.no_grad():
    t = alternate([(name, (lambda m=m: m(x))) for name, m in models], 10)
print(f"(b) DeiT-S 224 eval forward, batch {B}, one stage at block 3, keep 0.5, {mname} ({args.rounds} alternating rounds of 10 forwards)")
base = statistics.median(t["--attn-selection"])
for name, _ in models:
    show(name, t[name], unit=1.0, what="ms")
    print(f"  {'':34s} {B / statistics.median(t[name]) * 1e3:9.0f} images/s, {statistics.median(t[name]) - base:+.3f} ms against --attn-selection", flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
