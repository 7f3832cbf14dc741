#!/usr/bin/env python3
"""Data-parallel correctness check: N ranks (each with batch B/N) must produce, after the bucketed all-reduce, the same
averaged gradients and the same updated parameters as one process with the concatenated batch B.

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 tools/ddp_check.py

Backend: RCCL ("nccl") when every rank has its own GPU, otherwise gloo on GPU tensors (rehearsal on a 1-GPU box: all ranks
share cuda:0).  Exit code 0 = pass.

D2S_DDP_DIFF_TOPK=1 runs the same check with the differentiable token selection on (diff_topk=True, 16 noise samples, sigma 0.05): one
noise tensor [B, 16, N_i] per stage is shared, every rank injects its own images' slice (student.topk_noise) and the single process the
whole tensor, so both sides perturb the same probabilities with the same numbers.  Epoch 0 is then the case in which the stage outputs
require a gradient although the backbone is frozen: the grad_ready hooks fire against the predictor-only live set.  The indicators are
integer sample counts: the comparison presupposes that no perturbed value sits within fp32 rounding of its selection boundary, so the
smallest gap between the k-th and (k + 1)-th largest perturbed value of the single-process run is printed and must be at least 2e-5 (the
condition of tests/golden/difftopk_micro.npz); a run that misses it exits with code 3 - a property of the noise seed, not a mismatch.

D2S_DDP_ACCUM=A (default 1) makes every optimiser step a window of A micro-batches (TrainStep accum_steps=A): each rank is given its
slice of every micro-batch, the single process the whole micro-batches in the same order; the comparison is made after the call that
steps, on the combined gradient.  D2S_DDP_CLIP=M adds clip_grad=M on both sides, prints the two pre-clip norms
and requires them to agree to 1e-4 relative, the gradient criterion.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dense2sparse-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

from tests import cases


DIFF_TOPK = os.environ.get("D2S_DDP_DIFF_TOPK") == "1"
NOISE_SAMPLES, NOISE_SEED, MARGIN_MIN = 16, 41, 2e-5
ACCUM = int(os.environ.get("D2S_DDP_ACCUM", "1"))
CLIP = float(os.environ["D2S_DDP_CLIP"]) if os.environ.get("D2S_DDP_CLIP") else None


def stage_noise(case, B):
    """one shared standard-normal tensor [B, NOISE_SAMPLES, N_i] per stage"""
    from d2s import synth
    cfg = case["cfg"]
    n, out = cfg["n_patches"], []
    for i, r in enumerate(cfg["token_ratio"]):
        out.append(torch.from_numpy(synth.normal(f"ddp_check/noise/{i}", (B, NOISE_SAMPLES, n), std=1.0, seed=NOISE_SEED)))
        n = int(cfg["init_n"] * r)
    return out


def selection_margin(student, noises):
    """smallest gap between the k-th and (k + 1)-th largest perturbed keep probability of the student's last forward"""
    worst = float("inf")
    for scores, kept, nz in zip(student.pred_logits, student.kept_token_indices, noises):
        k = kept.shape[1]
        pert = torch.sort(torch.softmax(scores.detach(), dim=-1)[:, None, :] + nz.to(scores.device) * float(student.current_sigma),
                          dim=-1, descending=True)[0]
        worst = min(worst, float((pert[..., k - 1] - pert[..., k]).min()))
    return worst


def build(case, dev):
    import vit_models
    cfg = case["cfg"]
    extra = dict(diff_topk=True, topk_num_samples=NOISE_SAMPLES) if DIFF_TOPK else {}
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                  num_heads=cfg["heads"], mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    s = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]),
                                                distill=True, topk_selection=True, predictor_loss_type="kl_div", **common, **extra)
    t = vit_models.VisionTransformerTeacher(**common)
    sd_s, sd_t = cases.make_weights(case)
    s.load_state_dict({k: torch.from_numpy(v) for k, v in sd_s.items()})
    t.load_state_dict({k: torch.from_numpy(v) for k, v in sd_t.items()})
    args = types.SimpleNamespace(keep_ratios=list(cfg["token_ratio"]), mask_loss_type="kl_div", mixup=0.0,
                                 patch_score_threshold=None, step=0)
    return s.to(dev), t.to(dev), args


def main():
    from d2s.engine import TrainStep
    from d2s import synth
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    ngpu = torch.cuda.device_count()
    own_gpu = ngpu >= world
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) if own_gpu else 0)
    torch.cuda.set_device(dev)
    if os.environ.get("D2S_FORCE_NCCL") == "1":      # rehearsal: RCCL with every rank on the same GPU (if the library allows it)
        own_gpu = True
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if own_gpu else "gloo", rank=rank, world_size=world)
    case = dict(cases.MODEL_CASES["micro2"])
    per = 2
    B = per * world
    xs = [torch.from_numpy(synth.images(B, 3, case["cfg"]["img_size"], seed=77 + 100 * i)) for i in range(ACCUM)]
    ys = [torch.from_numpy(synth.labels(B, case["cfg"]["num_classes"], seed=77 + 100 * i)) for i in range(ACCUM)]
    window = dict(accum_steps=ACCUM, clip_grad=CLIP) if (ACCUM > 1 or CLIP is not None) else {}
    # tiny bucket so that several all-reduces are launched from inside backward (exercises the hook path); warmup_steps=1: epoch 0
    # trains the predictors only (live gradient set = their slices, exchanged by finish()), epoch 1 everything (hooks + buckets)
    s, t, args = build(case, dev)
    ts = TrainStep(s, t, args, distributed=True, bucket_mb=0.25, warmup_steps=1, **window)
    ref = None
    if rank == 0:
        s1, t1, args1 = build(case, dev)
        ref = TrainStep(s1, t1, args1, distributed=False, warmup_steps=1, **window)
    noises = stage_noise(case, B) if DIFF_TOPK else None
    if DIFF_TOPK:
        s.topk_noise = [nz[rank * per:(rank + 1) * per] for nz in noises]
        if rank == 0:
            s1.topk_noise = noises
    ok, margin_ok = True, True
    for epoch in (0, 1):
        ts.set_epoch(epoch)
        live = list(ts.reducer.live)
        if epoch == 0:
            assert ts.reducer.live_elems() < ts.arena.total // 2, "warm-up epoch must only exchange the predictor slices"
        for x, y in zip(xs, ys):
            info = ts(x[rank * per:(rank + 1) * per].to(dev), y[rank * per:(rank + 1) * per].to(dev))
        assert info.get("stepped", True), "the last call of the window must have stepped"
        torch.cuda.synchronize()
        grads = ts.arena.grads.clone() / world
        params = ts.arena.params.clone()
        if rank == 0:
            ref.set_epoch(epoch)
            for x, y in zip(xs, ys):
                ref(x.to(dev), y.to(dev))
            torch.cuda.synchronize()
            sel = torch.cat([torch.arange(a, b) for a, b in live]).to(dev)       # the gradients the optimiser reads
            gd = float((grads[sel] - ref.arena.grads[sel]).norm() / ref.arena.grads[sel].norm())
            pd = float((params - ref.arena.params).abs().max())
            print(f"[ddp_check] world={world} backend={'nccl' if own_gpu else 'gloo'} epoch {epoch} live {len(sel)}/{ts.arena.total} "
                  f"rel grad diff {gd:.3e}  max param diff {pd:.3e}")
            ok = ok and gd < 1e-4 and pd < 2 * 2 * 5e-4 * 1.01
            if CLIP is not None:
                # the norm is taken from the exchanged sum: one taken before the exchange, or scaled by the wrong 1 / (c * world),
                # differs in the first digit, the summation orders of the two sides differ by rounding only
                nd = abs(float(ts.last_clip[0]) - float(ref.last_clip[0])) / float(ref.last_clip[0])
                ok = ok and nd < 1e-4
                print(f"[ddp_check] rel pre-clip norm diff {nd:.3e}")
                print(f"[ddp_check] accum {ACCUM} clip {CLIP}: pre-clip norm {float(ts.last_clip[0]):.6e} (coef {float(ts.last_clip[1]):.6f}), "
                      f"single process {float(ref.last_clip[0]):.6e} (coef {float(ref.last_clip[1]):.6f})")
            if DIFF_TOPK:
                margin = selection_margin(s1, noises)
                print(f"[ddp_check] diff_topk epoch {epoch}: selection margin of the single-process run {margin:.3e} (needs >= {MARGIN_MIN:.0e})")
                margin_ok = margin_ok and margin >= MARGIN_MIN
    flag = torch.tensor([(1 if ok else 0) + (0 if margin_ok else 2)])
    flag = flag.to(dev) if own_gpu else flag
    dist.broadcast(flag, src=0)
    dist.destroy_process_group()
    code = int(flag.item())
    sys.exit(3 if code & 2 else (0 if code & 1 else 1))


if __name__ == "__main__":
    main()
