"""Inference throughput of the dynamic-keep-ratio student (--patch-score-threshold, DESIGN.md sections 10 and 19): eval mode, forward only,
DeiT-S 224, pruning stage at block 3, threshold 0.5, B = 128, seeded random weights.  Every block from the stage on runs on the ragged
packed batch (Block.forward_ragged); in the bf16 arithmetic mode that is the bf16 data path with d2s_attn_varlen_fwd_bf16.  Prints
ms per batch, images/s and how ragged the batch was (min / mean / max kept tokens per image, CLS included).  With several
--pruning-locs every stage after the first acts on the packed batch (the ragged cascade) and the packed length is
printed per stage.  GPU box only.

  python tools/ragged_infer_bench.py [--gemm-mode exact|split|bf16|all] [--pruning-locs 3 6 9]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
import torch
import vit_models
from d2s import ops

MODES = {"exact": (ops.GEMM_EXACT, "fp32 exact"), "split": (ops.GEMM_SPLIT, "bf16x3 split"), "bf16": (ops.GEMM_BF16, "bf16 operands")}
ap = argparse.ArgumentParser()
ap.add_argument("--gemm-mode", choices=list(MODES) + ["all"], default="all")
ap.add_argument("--pruning-locs", type=int, nargs="+", default=[3])
args = ap.parse_args()
LOCS = list(args.pruning_locs)

dev = torch.device("cuda:0")
B, WARMUP, TIMED = 128, 3, 20
torch.manual_seed(0)
x = torch.randn(B, 3, 224, 224, device=dev)
for key in (list(MODES) if args.gemm_mode == "all" else [args.gemm_mode]):
    mode, mname = MODES[key]
    ops.set_gemm_mode(mode)
    torch.manual_seed(0)
    m = vit_models.dynamic_vit_small_patch16_224_student(LOCS, [0.5] * len(LOCS), topk_selection=True, predictor_loss_type="kl_div",
                                                         patch_score_threshold=0.5).to(dev).eval()
    with torch.no_grad():
        for _ in range(WARMUP):
            m(x)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(TIMED):
            m(x)
        e.record()
        torch.cuda.synchronize()
    ms = s.elapsed_time(e) / TIMED
    cu = m.cu_seqlens.cpu()
    kept = (cu[1:] - cu[:-1]).float()
    print(f"{mname:14s} student threshold 0.5 @ block {' '.join(map(str, LOCS))}  {ms:7.2f} ms/batch  {B / ms * 1e3:9.0f} images/s   kept tokens per image "
          f"min {int(kept.min())} mean {float(kept.mean()):.1f} max {int(kept.max())} (total {int(cu[-1])} rows)", flush=True)
    for stage, cu_s in enumerate(m.cu_seqlens_per_stage):
        c = cu_s.cpu()
        ln = (c[1:] - c[:-1]).float()
        print(f"{'':14s} stage {stage} @ block {LOCS[stage]}: packed length per image mean {float(ln.mean()):.1f} min {int(ln.min())} "
              f"max {int(ln.max())}", flush=True)
ops.set_gemm_mode(ops.GEMM_EXACT)
