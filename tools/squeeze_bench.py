"""Per-launch duration and achieved bytes/s of the three kernels of a squeezing stage (d2s_squeeze_match, d2s_gather_squeeze_fwd,
d2s_gather_squeeze_bwd) next to d2s_gather_pack_fwd / d2s_scatter_unpack_bwd and d2s_gather_fuse_fwd / _bwd at the
same shape, in the same process, in alternating rounds.  Outputs are preallocated and the C entries are called directly, launches back to
back (launch gaps included, the same for all); inputs rotate through more than 512 MB so that reads come from HBM, not from the 256 MB
Infinity Cache.  Each timing is preceded by 3 warm-up launches; a row is the median of ROUNDS rounds of ITERS launches.  Bytes are the
algorithm's: every row read or written once, plus ids and plan (the match reads x once and writes only the plan).  GPU box only.

With --step (a run of its own): the full train step at the headline configuration (DeiT-S, one stage at block 3, keep 0.5, batch 128,
fp32 GEMM mode, eager) with squeeze_dropped off and on, the same weights, alternating rounds of 10 steps after 3 warm-up steps each;
--step-only on|off runs one of the two alone for 12 steps (the form to put under a kernel trace).

  python tools/squeeze_bench.py
  python tools/squeeze_bench.py --step
"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
from d2s import lib, ops

dev = torch.device("cuda:0")
ROUNDS, ITERS = 5, 200


def timed(fn, nbuf):
    for i in range(3):
        fn(i % nbuf)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(ITERS):
        fn(i % nbuf)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / ITERS


def bench(B, T, k, D):
    n, m = T + 1, T - k
    nbuf = max(2, int(600e6 // (B * n * D * 4)) + 1)
    torch.manual_seed(0)
    # tokens from a 16-dimensional subspace plus noise: cosines spread the way those of token features do, several sources per kept row
    xs = [torch.randn(B, n, 16, device=dev) @ torch.randn(16, D, device=dev) + 0.1 * torch.randn(B, n, D, device=dev) for _ in range(nbuf)]
    p = ops.softmax_rows(torch.randn(B, T, device=dev))
    kept, dropped = ops.select_topk(p, k)
    gk = [torch.randn(B, k + 1, D, device=dev) for _ in range(nbuf)]
    gf = [torch.randn(B, k + 2, D, device=dev) for _ in range(nbuf)]
    dst, sim = torch.empty(B, m, dtype=torch.int32, device=dev), torch.empty(B, m, device=dev)
    y, Z = torch.empty(B, k + 1, D, device=dev), torch.empty(B, k, device=dev)
    yf, S = torch.empty(B, k + 2, D, device=dev), torch.empty(B, device=dev)
    dx, dp = torch.empty(B, n, D, device=dev), torch.empty(B, T, device=dev)
    P = lib.ptr
    fns = {
        "gather_pack_fwd": lambda i: lib.call("d2s_gather_pack_fwd", P(xs[i]), P(kept), P(y), B, n, k, D),
        "gather_fuse_fwd": lambda i: lib.call("d2s_gather_fuse_fwd", P(xs[i]), P(p), P(kept), P(dropped), P(yf), P(S), B, n, 0, k, D),
        "squeeze_match": lambda i: lib.call("d2s_squeeze_match", P(xs[i]), P(kept), P(dropped), B, n, k, D, P(dst), P(sim)),
        "gather_squeeze_fwd": lambda i: lib.call("d2s_gather_squeeze_fwd", P(xs[i]), P(kept), P(dropped), P(dst), P(sim), B, n, k, D, P(y), P(Z)),
        "scatter_unpack_bwd": lambda i: lib.call("d2s_scatter_unpack_bwd", P(gk[i]), P(kept), P(dx), B, n, k, D),
        "gather_fuse_bwd": lambda i: lib.call("d2s_gather_fuse_bwd", P(gf[i]), P(xs[i]), P(p), P(S), P(yf), P(kept), P(dropped), P(dx), P(dp),
                                              B, n, 0, k, D),
        "gather_squeeze_bwd": lambda i: lib.call("d2s_gather_squeeze_bwd", P(gk[i]), P(kept), P(dropped), P(dst), P(sim), P(Z), B, n, k, D,
                                                 P(dx)),
    }
    row = D * 4.0
    bytes_ = {
        "gather_pack_fwd": B * (2.0 * (k + 1) * row + 8.0 * k),
        "gather_fuse_fwd": B * ((1 + k + m) * row + (k + 2) * row + 8.0 * T + 4.0 * m + 4.0),
        "squeeze_match": B * (T * row + 8.0 * T + 8.0 * m),
        "gather_squeeze_fwd": B * (n * row + (k + 1) * row + 8.0 * T + 8.0 * m + 4.0 * k),
        "scatter_unpack_bwd": B * ((k + 1) * row + n * row + 8.0 * k),
        "gather_fuse_bwd": B * ((k + 2 + m + 1) * row + n * row + 8.0 * T + 4.0 * m + 4.0 * T + 4.0),
        "gather_squeeze_bwd": B * ((k + 1) * row + n * row + 8.0 * T + 8.0 * m + 4.0 * k),
    }
    # FLOPs of the match: the m x k dots over D (the squared norms that ride along are not counted)
    flops = 2.0 * B * m * k * D
    fns["gather_fuse_fwd"](0)           # yf, S and the plan of buffer 0 feed the backwards (they read other buffers: same traffic)
    fns["squeeze_match"](0)
    fns["gather_squeeze_fwd"](0)
    torch.cuda.synchronize()
    srcs = torch.bincount(dst.long().clamp_min(0).flatten() + k * torch.arange(B, device=dev).repeat_interleave(m), minlength=B * k)
    us = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            us[name].append(timed(fn, nbuf))
    med = {name: statistics.median(v) for name, v in us.items()}
    print(f"B={B} T={T} k={k} D={D}  ({nbuf} input buffers, {ROUNDS} rounds x {ITERS} launches, median of rounds; "
          f"sources per kept row: mean {m / k:.2f}, max {int(srcs.max())})")
    for name in fns:
        extra = f"  {flops / med[name] / 1e6:6.2f} TFLOP/s" if name == "squeeze_match" else ""
        print(f"  {name:20s} {med[name]:8.2f} us/launch  (min {min(us[name]):.2f} max {max(us[name]):.2f})  {bytes_[name] / 1e6:8.2f} MB"
              f"  {bytes_[name] / med[name] / 1e6:7.2f} TB/s{extra}")
    fwd, bwd = med["squeeze_match"] + med["gather_squeeze_fwd"], med["gather_squeeze_bwd"]
    print(f"  stage forward (match + merge) {fwd:.2f} us = x{fwd / med['gather_pack_fwd']:.2f} gather_pack_fwd, x{fwd / med['gather_fuse_fwd']:.2f} "
          f"gather_fuse_fwd; backward {bwd:.2f} us = x{bwd / med['scatter_unpack_bwd']:.2f} scatter_unpack_bwd, "
          f"x{bwd / med['gather_fuse_bwd']:.2f} gather_fuse_bwd")
    sys.stdout.flush()


def train_steps(only=None, B=128):
    import types
    import vit_models
    from d2s.engine import TrainStep
    steps = {}
    for name, flag in (("off", False), ("on", True)):
        if only not in (None, name):
            continue
        torch.manual_seed(0)
        student = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                                   squeeze_dropped=flag)
        teacher = vit_models.dynamic_vit_small_patch16_224_teacher()
        targs = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
        steps[name] = TrainStep(student.to(dev), teacher.to(dev), targs, lr=5e-4, min_lr=1e-5, weight_decay=0.05, epochs=25, warmup_steps=0,
                                graph=False)
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn((B, 3, 224, 224), device=dev, generator=g)
    labels = torch.randint(0, 1000, (B,), device=dev, generator=g)

    def run(ts, n):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            ts(images, labels)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n
    if only is not None:
        print(f"squeeze_dropped {only}: {run(steps[only], 12):.2f} ms/step over 12 steps (the first ones include warm-up)")
        return
    for ts in steps.values():
        run(ts, 3)
    ms = {name: [] for name in steps}
    for _ in range(ROUNDS):
        for name, ts in steps.items():
            ms[name].append(run(ts, 10))
    print(f"train step, DeiT-S, stage at block 3, keep 0.5, batch {B}, fp32 mode, eager ({ROUNDS} alternating rounds x 10 steps, median of rounds)")
    for name, v in ms.items():
        print(f"  squeeze_dropped {name:3s} {statistics.median(v):8.2f} ms/step  {B / statistics.median(v) * 1e3:8.1f} images/s  "
              f"(min {min(v):.2f} max {max(v):.2f})")
    print(f"  on / off = x{statistics.median(ms['on']) / statistics.median(ms['off']):.4f}")
    sys.stdout.flush()


if "--step-only" in sys.argv:
    train_steps(only=sys.argv[sys.argv.index("--step-only") + 1])
elif "--step" in sys.argv:
    train_steps()
else:
    bench(128, 196, 137, 384)
    bench(128, 137, 98, 384)
    bench(128, 196, 98, 384)
