"""Per-launch duration and achieved bytes/s of the token-fusion kernels (d2s_gather_fuse_fwd / d2s_gather_fuse_bwd)
next to d2s_gather_pack_fwd / d2s_scatter_unpack_bwd at the same shape, in the same process, in alternating rounds.  Outputs are
preallocated and the C entries are called directly, launches back to back (launch gaps included, the same for all four); inputs rotate
through more than 512 MB so that reads come from HBM, not from the 256 MB Infinity Cache.  Bytes are the algorithm's: every row read or
written once, plus ids and probabilities.  GPU box only.

  python tools/fuse_bench.py
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


def bench(B, n, k, D, t=0):
    T, m, R = n - 1 - t, n - 1 - t - k, k + t + 2
    nbuf = max(2, int(600e6 // (B * n * D * 4)) + 1)
    torch.manual_seed(0)
    xs = [torch.randn(B, n, D, device=dev) for _ in range(nbuf)]
    gs = [torch.randn(B, R, D, device=dev) for _ in range(nbuf)]
    p = ops.softmax_rows(torch.randn(B, T, device=dev))
    kept, dropped = ops.select_topk(p, k)
    y, S = torch.empty(B, R, D, device=dev), torch.empty(B, device=dev)
    dx, dp = torch.empty(B, n, D, device=dev), torch.empty(B, T, device=dev)
    out = torch.empty(B, k + 1, D, device=dev)
    gps = [torch.randn(B, k + 1, D, device=dev) for _ in range(nbuf)]
    P = lib.ptr
    fns = {
        "gather_fuse_fwd": lambda i: lib.call("d2s_gather_fuse_fwd", P(xs[i]), P(p), P(kept), P(dropped), P(y), P(S), B, n, t, k, D),
        "gather_pack_fwd": lambda i: lib.call("d2s_gather_pack_fwd", P(xs[i]), P(kept), P(out), B, n, k, D),
        "gather_fuse_bwd": lambda i: lib.call("d2s_gather_fuse_bwd", P(gs[i]), P(xs[i]), P(p), P(S), P(y), P(kept), P(dropped), P(dx), P(dp),
                                              B, n, t, k, D),
        "scatter_unpack_bwd": lambda i: lib.call("d2s_scatter_unpack_bwd", P(gps[i]), P(kept), P(dx), B, n, k, D),
    }
    row = D * 4.0
    bytes_ = {
        "gather_fuse_fwd": B * ((1 + k + t + m) * row + R * row + 8.0 * T + 4.0 * m + 4.0),
        "gather_pack_fwd": B * (2.0 * (k + 1) * row + 8.0 * k),
        "gather_fuse_bwd": B * ((R + m + 1) * row + n * row + 8.0 * T + 4.0 * m + 4.0 * T + 4.0),
        "scatter_unpack_bwd": B * ((k + 1) * row + n * row + 8.0 * k),
    }
    fns["gather_fuse_fwd"](0)           # y and S of buffer 0 feed the backward (the timed backward reads other x buffers: same traffic)
    us = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            us[name].append(timed(fn, nbuf))
    med = {name: statistics.median(v) for name, v in us.items()}
    print(f"B={B} n={n} t={t} k={k} D={D}  ({nbuf} input buffers, {ROUNDS} rounds x {ITERS} launches, median of rounds)")
    for name in fns:
        print(f"  {name:20s} {med[name]:8.2f} us/launch  (min {min(us[name]):.2f} max {max(us[name]):.2f})  {bytes_[name] / 1e6:8.2f} MB"
              f"  {bytes_[name] / med[name] / 1e6:7.2f} TB/s")
    for a, b in (("gather_fuse_fwd", "gather_pack_fwd"), ("gather_fuse_bwd", "scatter_unpack_bwd")):
        br, tr = bytes_[a] / bytes_[b], med[a] / med[b]
        print(f"  {a} / {b}: bytes x{br:.3f}  time x{tr:.3f}  time ratio / byte ratio {tr / br:.3f}  (expected <= 1.25)")
    sys.stdout.flush()


bench(128, 197, 98, 384)
bench(64, 577, 172, 768)
