"""Attention selection (d2s_select_cls_attn), two measurements in one process.  GPU box only.

(a) Per-stage selection cost at (B=128, H=6, n=197, k=98) and (B=64, H=12, n=577, k=172), in alternating rounds:
      fused        d2s_select_cls_attn                              one launch
      composed     d2s_teacher_target (L = 1) + d2s_select_topk     the same result from the two launches that existed before
      predictor    PredictorLG.forward_tokens (scores + softmax) + d2s_select_topk: the stage the flag replaces
    Outputs of the two kernel-only variants are preallocated and the C entries called directly, launches back to back; the predictor
    stage goes through its Function under no_grad.  The spread of the composed variant over the rounds is the margin the fused launch
    is judged by.
(b) Eval-forward images/s of DeiT-S (one stage at block 3, keep 0.5, batch 128, fp32 GEMM mode) with and without attn_selection, the
    same weights, alternating rounds.

  python tools/attnsel_bench.py
"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
import vit_models
from d2s import lib, ops
from vit_models.dynamic_vit import PredictorLG

dev = torch.device("cuda:0")
ROUNDS, ITERS = 7, 200


def timed(fn, iters=ITERS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters


def selection(B, H, n, k, D):
    T = n - 1
    torch.manual_seed(0)
    rows = torch.softmax(torch.randn(B, H, n, device=dev) * 2.0, dim=-1).contiguous()
    x = torch.randn(B, n, D, device=dev)
    pred = PredictorLG(D, topk_selection=True, k=k, loss_type="kl_div").to(dev).eval()
    probs, target = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    kept = torch.empty(B, k, dtype=torch.int64, device=dev)
    dropped = torch.empty(B, T - k, dtype=torch.int64, device=dev)
    P = lib.ptr

    def fused():
        lib.call("d2s_select_cls_attn", P(rows), B, H, n, 1, T, k, 0, P(probs), P(kept), P(dropped))

    def composed():
        lib.call("d2s_teacher_target", P(rows), P(target), B, 1, H, n)
        lib.call("d2s_select_topk", P(target), B, T, k, P(kept), P(dropped))

    def predictor():
        with torch.no_grad():
            _, keep_probs = pred.forward_tokens(x)
            ops.select_topk(keep_probs.contiguous(), k)

    fused()
    a = (probs.clone(), kept.clone(), dropped.clone())
    composed()
    torch.cuda.synchronize()
    same_ids = torch.equal(a[1], kept) and torch.equal(a[2], dropped)
    fns = {"fused": (fused, ITERS), "composed": (composed, ITERS), "predictor": (predictor, 20)}
    us = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, (fn, iters) in fns.items():
            us[name].append(timed(fn, iters))
    med = {name: statistics.median(v) for name, v in us.items()}
    print(f"(a) B={B} H={H} n={n} k={k} D={D}  ({ROUNDS} rounds, median of rounds; ids of fused and composed equal: {same_ids}; "
          f"largest |probs - target| {float((a[0] - target).abs().max()):.2e})")
    for name in fns:
        print(f"  {name:10s} {med[name]:9.2f} us/stage  (min {min(us[name]):.2f} max {max(us[name]):.2f})")
    spread = max(us["composed"]) - min(us["composed"])
    print(f"  fused - composed = {med['fused'] - med['composed']:+.2f} us; spread of composed over the rounds {spread:.2f} us; "
          f"fused is {'no slower than' if med['fused'] <= med['composed'] + spread else 'SLOWER than'} composed within that spread")
    print(f"  predictor stage / fused = x{med['predictor'] / med['fused']:.1f}")
    sys.stdout.flush()


def eval_forward(B=128):
    torch.manual_seed(0)
    models = {}
    for name, flag in (("predictor", False), ("attn_selection", True)):
        m = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div", attn_selection=flag)
        if models:
            m.load_state_dict(models["predictor"].state_dict())
        models[name] = m.to(dev).eval()
    x = torch.randn(B, 3, 224, 224, device=dev)

    def run(m):
        with torch.no_grad():
            m(x)
    ims = {name: [] for name in models}
    for _ in range(ROUNDS):
        for name, m in models.items():
            ims[name].append(B / (timed(lambda: run(m), 10) * 1e-6))
    print(f"(b) DeiT-S eval forward, one stage at block 3, keep 0.5, batch {B}, fp32 mode ({ROUNDS} rounds x 10 forwards, median of rounds)")
    for name, v in ims.items():
        print(f"  {name:15s} {statistics.median(v):9.1f} images/s  (min {min(v):.1f} max {max(v):.1f})")
    print(f"  attn_selection / predictor = x{statistics.median(ims['attn_selection']) / statistics.median(ims['predictor']):.3f}")
    sys.stdout.flush()


selection(128, 6, 197, 98, 384)
selection(64, 12, 577, 172, 768)
eval_forward()
