"""Counterpart of the reference's entry script (mask_predictor.py:56-330): the same flags (utils.parse_args), the same sequence
- student / teacher from the arch factories (:170-202), parameter groups + AdamW (:213-230), optional backbone freeze
(:218-224), per epoch adjust_learning_rate -> train_one_epoch -> evaluate_performance (:295-310), best-accuracy tracking -
on the accelerated path, with synthetic batches by default or, with --data-source folder, the reference's ImageFolder split, training
transform and Mixup/CutMix on the GPU input pipeline (d2s.data, csrc/augment.hip); wandb / tensorboard tracking and visualisations
are outside the path.

    python dense2sparse-vit_amd/mask_predictor.py --arch deit_small --pruning-locs 3 --keep-ratios 0.5 --epochs 3 \\
        --warmup-steps 1 --batch-size 64 --steps-per-epoch 10
    python dense2sparse-vit_amd/mask_predictor.py --arch deit_small --pruning-locs 3 --keep-ratios 0.5 --topk-selection \\
        --data-source folder --imgnet-val-dir /path/to/imagefolder --batch-size 128
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        dense2sparse-vit_amd/mask_predictor.py --use-ddp ...        (one process per GPU, RCCL)
    python dense2sparse-vit_amd/mask_predictor.py ... --output-dir runs/a --model-ema      (runs/a/last.pt after every epoch, best.pt)
    python dense2sparse-vit_amd/mask_predictor.py ... --output-dir runs/a --resume runs/a/last.pt
    python dense2sparse-vit_amd/mask_predictor.py ... --eval-only --resume runs/a/best.pt
    python dense2sparse-vit_amd/mask_predictor.py ... --batch-size 64 --accum-steps 8 --clip-grad 1.0     (512 images per optimiser step)
    python dense2sparse-vit_amd/mask_predictor.py --method dynamicvit --arch deit_small --pruning-locs 3 6 9 --keep-ratios 0.7 0.49 0.343
    python dense2sparse-vit_amd/mask_predictor.py ... --topk-selection --attn-selection [--mean-heads] [--fuse-dropped]     (select by the CLS attention)
    python dense2sparse-vit_amd/mask_predictor.py ... --topk-selection --squeeze-dropped     (dropped tokens go into their nearest kept token)
    python dense2sparse-vit_amd/mask_predictor.py ... --topk-selection --patch-score-threshold 0.4 --pruning-locs 3 6 9 --keep-ratios 0.7 0.5 0.3 \
        --ragged-cascade                                                   (dynamic keep ratio, ragged inference through every stage)
    python dense2sparse-vit_amd/mask_predictor.py ... --topk-selection --patch-score-threshold 0.4 --pruning-locs 3 6 9 --keep-ratios 0.7 0.5 0.3 \
        --ragged-cascade --ragged-train                                    (... and training on the ragged batch as well)
    python dense2sparse-vit_amd/mask_predictor.py --method tome --tome-r 13 --arch deit_small --eval-only --student-checkpoint deit_small.pth
    python dense2sparse-vit_amd/mask_predictor.py --method tome --tome-r 13 --arch deit_small --eval-only --tome-bf16 --student-checkpoint deit_small.pth
    python dense2sparse-vit_amd/mask_predictor.py --method tome --tome-r 13 --arch deit_small --tome-train --student-checkpoint deit_small.pth \
        --teacher-checkpoint deit_small.pth --epochs 30                   (fine-tune through the merges; --dist-weight 0: no teacher)
    python dense2sparse-vit_amd/mask_predictor.py --method tome --tome-r 13 --arch deit_small --tome-train --tome-train-bf16 ...  (... in bf16)
    python dense2sparse-vit_amd/mask_predictor.py --method ats --pruning-locs 3 6 9 --ats-tokens 64 --arch deit_small --eval-only \
        --student-checkpoint deit_small.pth                               (adaptive token sampling: every image keeps its own count)
    python dense2sparse-vit_amd/mask_predictor.py --method avit --arch deit_small --student-checkpoint deit_small.pth --dist-weight 0
    python dense2sparse-vit_amd/mask_predictor.py --method ats --pruning-locs 3 6 9 --ats-tokens 64 --arch deit_small --ats-train \
        --student-checkpoint deit_small.pth --teacher-checkpoint deit_small.pth --epochs 30      (fine-tune through the sampling stages)
    python dense2sparse-vit_amd/mask_predictor.py --method ltp --pruning-locs 3 6 9 --arch deit_small --student-checkpoint deit_small.pth \
        --output-dir runs/soft                                            (learn the thresholds: soft masks on the dense batch)
    python dense2sparse-vit_amd/mask_predictor.py --method ltp --ltp-phase hard --pruning-locs 3 6 9 --arch deit_small \
        --student-checkpoint runs/soft/best.pt                            (fine-tune with the thresholds fixed: tokens leave the ragged batch)
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import methods                                       # noqa: E402
import utils                                         # noqa: E402
import vit_models                                    # noqa: E402
from d2s import ops                                  # noqa: E402
from d2s.engine import TrainStep                     # noqa: E402
from evaluate import evaluate_performance            # noqa: E402
from train import train_one_epoch                    # noqa: E402

_STUDENTS = {"deit_tiny": "dynamic_vit_tiny_patch16_224_student", "deit_small": "dynamic_vit_small_patch16_224_student",
             "deit_base": "dynamic_vit_base_patch16_224_student"}
_TEACHERS = {"deit_tiny": "dynamic_vit_tiny_patch16_224_teacher", "deit_small": "dynamic_vit_small_patch16_224_teacher",
             "deit_base": "dynamic_vit_base_patch16_224_teacher"}
# --method dynamicvit: flags of the d2s selection rules that the baseline's Gumbel keep decision has no counterpart for
_NOT_WITH_DYNAMICVIT = (("topk_selection", "--topk-selection"), ("diff_topk", "--diff-topk"), ("patch_score_threshold", "--patch-score-threshold"),
                        ("small_predictor", "--small-predictor"), ("predictor_bn", "--predictor-bn"), ("fuse_dropped", "--fuse-dropped"))
# --method ats: the selection rules of the dense-to-sparse student, which a sampling stage replaces
_NOT_WITH_ATS = (("topk_selection", "--topk-selection"), ("attn_selection", "--attn-selection"), ("fuse_dropped", "--fuse-dropped"),
                 ("squeeze_dropped", "--squeeze-dropped"), ("diff_topk", "--diff-topk"), ("patch_score_threshold", "--patch-score-threshold"))
_EVO_DEPTH, _EVO_PATCHES = 12, 196           # the factories' trunk: 12 blocks on the 14 x 14 patches of a 224 image


def _training_refusals(m, args, bad, warmup=True):
    """What no logits-only family trains with, under the family's own subject (m.cli) and in its own words."""
    if m.cli_bf16 and getattr(args, "gemm_mode", "exact") == "bf16" and not (m.cli_bf16[1] and args.eval_only):
        bad.append(f"{m.cli} with --gemm-mode bf16 ({m.cli_bf16[0]})")
    if getattr(args, "drop_path", 0.0) > 0.0:
        bad.append(f"{m.cli} with --drop-path {args.drop_path} (stochastic depth is not built for {m.block})")
    if args.torch_optim:
        bad.append(f"{m.cli} with --torch-optim ({m.optim_noun} trains through the fused step only)")
    if warmup and getattr(args, "warmup_steps_given", True) and args.warmup_steps > 0:
        bad.append(f"{m.cli} with --warmup-steps {args.warmup_steps} (the warm-up epochs train the score predictors only and "
                   f"{m.has_none}: pass 0 or leave it out)")


def _evo_ranges(args, bad):
    start = getattr(args, "evo_start", None)
    if start is not None and not 1 <= start <= _EVO_DEPTH:
        bad.append(f"--evo-start {start} (a block in 1..{_EVO_DEPTH}, the depth)")
    keep = getattr(args, "evo_keep", None)
    if keep is not None and not 1 <= int(_EVO_PATCHES * keep) <= _EVO_PATCHES - 1:
        bad.append(f"--evo-keep {keep} (k = int({_EVO_PATCHES} * keep) must lie in 1..{_EVO_PATCHES - 1})")
    tau = getattr(args, "evo_tradeoff", None)
    if tau is not None and not 0.0 <= tau <= 1.0:
        bad.append(f"--evo-tradeoff {tau} (0 <= tau <= 1)")


def _ltp_ranges(args, bad):
    locs = list(args.pruning_locs or [])
    if not locs or any(v < 0 or v > _EVO_DEPTH - 2 for v in locs) or any(a >= b for a, b in zip(locs, locs[1:])):
        bad.append(f"--method ltp with --pruning-locs {' '.join(str(v) for v in locs)} (ascending blocks in 0..{_EVO_DEPTH - 2}: a stage "
                   "acts on the blocks after it)")
    tau = getattr(args, "ltp_temperature", None)
    if tau is not None and not tau > 0.0:
        bad.append(f"--ltp-temperature {tau} (tau > 0)")
    lam = getattr(args, "ltp_lambda", None)
    if lam is not None and not lam >= 0.0:
        bad.append(f"--ltp-lambda {lam} (lambda >= 0)")


def check_supported(args):
    """Flags whose code path is outside the accelerated hot path fail here, loudly, instead of silently training something else."""
    bad = []
    method = getattr(args, "method", "d2s")
    if method == "dynamicvit":
        for attr, flag in _NOT_WITH_DYNAMICVIT:
            if getattr(args, attr, None) not in (None, False):
                bad.append(f"--method dynamicvit with {flag} (the baseline keeps tokens by its own Gumbel decision and predictor)")
    tome_r = getattr(args, "tome_r", 0)
    if tome_r < 0:
        bad.append(f"--tome-r {tome_r} (0 or more tokens per block)")
    tome_train = bool(getattr(args, "tome_train", False))
    if tome_train and method != "tome":
        bad.append(f"--tome-train with --method {method} (it trains the Token Merging baseline: --method tome)")
    if tome_train:
        _training_refusals(methods.by_name("tome"), args, bad, warmup=False)      # its warm-up is printed and zeroed below, not refused
    if bool(getattr(args, "tome_bf16", False)):
        if method != "tome":
            bad.append(f"--tome-bf16 with --method {method} (it puts the Token Merging baseline on the bf16 data path: "
                       "--method tome)")
        if tome_train:
            bad.append("--tome-bf16 with --tome-train (training through the merges is built in fp32 only)")
        if not args.eval_only:
            bad.append("--tome-bf16 without --eval-only (the bf16 merging trunk is built for inference)")
    tome_train_bf16 = bool(getattr(args, "tome_train_bf16", False))
    if tome_train_bf16:
        # the flag, not the mode, selects the path (as --ragged-bf16): it sets the bf16 arithmetic mode itself, --gemm-mode bf16 stays refused below
        if not tome_train:
            bad.append("--tome-train-bf16 without --tome-train (it puts training through the merges into the bf16 arithmetic mode)")
        if bool(getattr(args, "tome_bf16", False)):
            bad.append("--tome-train-bf16 with --tome-bf16 (--tome-bf16 is the inference-only trunk; validation under --tome-train-bf16 "
                       "runs on the bf16 data path already)")
        if getattr(args, "gemm_mode", "exact") == "split":
            bad.append("--tome-train-bf16 with --gemm-mode split (the flag sets the bf16 arithmetic mode itself: leave --gemm-mode at exact)")
    if method == "tome":
        if not args.eval_only and not tome_train:
            bad.append("--method tome without --eval-only (token merging is built for inference: training through a merge needs the merge's "
                       "backward and key weights in both attention-backward kernels)")
        if getattr(args, "gemm_mode", "exact") == "bf16":
            bad.append("--method tome with --gemm-mode bf16 (the key-weighted attention is an fp32 kernel; exact and split run)")
    elif tome_r > 0:
        bad.append(f"--tome-r {tome_r} with --method {method} (tokens are merged by --method tome only)")
    ats_tokens = getattr(args, "ats_tokens", None)
    ats_train = bool(getattr(args, "ats_train", False))
    if ats_train:
        if method != "ats":
            bad.append(f"--ats-train with --method {method} (it trains the Adaptive Token Sampling baseline: --method ats)")
        if args.eval_only:
            bad.append("--ats-train with --eval-only (evaluation runs the inference path: drop one of the two)")
        _training_refusals(methods.by_name("ats"), args, bad)
    ats_train_bf16 = bool(getattr(args, "ats_train_bf16", False))
    if ats_train_bf16:
        # the flag, not the mode, selects the path (as --tome-train-bf16): it sets the bf16 arithmetic mode itself, --gemm-mode bf16 stays refused
        if not ats_train:
            bad.append("--ats-train-bf16 without --ats-train (it puts training through the sampling stages into the bf16 arithmetic mode)")
        if getattr(args, "gemm_mode", "exact") == "split":
            bad.append("--ats-train-bf16 with --gemm-mode split (the flag sets the bf16 arithmetic mode itself: leave --gemm-mode at exact)")
    avit_bf16 = bool(getattr(args, "avit_bf16", False))
    if avit_bf16:
        if method != "avit":
            bad.append(f"--avit-bf16 with --method {method} (it puts training the A-ViT baseline into the bf16 arithmetic mode: --method avit)")
        if args.eval_only:
            bad.append("--avit-bf16 with --eval-only (--gemm-mode bf16 already evaluates the adaptive-depth trunk on the bf16 data path)")
        if getattr(args, "gemm_mode", "exact") == "split":
            bad.append("--avit-bf16 with --gemm-mode split (the flag sets the bf16 arithmetic mode itself: leave --gemm-mode at exact)")
    ltp_bf16 = bool(getattr(args, "ltp_bf16", False))
    if ltp_bf16:
        # the flag, not the mode, selects the path (as --avit-bf16): it sets the bf16 arithmetic mode itself, --gemm-mode bf16 stays refused
        if method != "ltp":
            bad.append(f"--ltp-bf16 with --method {method} (it puts the LTP baseline into the bf16 arithmetic mode: --method ltp)")
        if getattr(args, "gemm_mode", "exact") == "split":
            bad.append("--ltp-bf16 with --gemm-mode split (the flag sets the bf16 arithmetic mode itself: leave --gemm-mode at exact)")
    if method == "ats":
        if not args.eval_only and not ats_train:
            bad.append("--method ats without --eval-only (adaptive token sampling is built for inference: a sampling stage has no backward)")
        for attr, flag in _NOT_WITH_ATS:
            if getattr(args, attr, None) not in (None, False):
                bad.append(f"--method ats with {flag} ({methods.by_name('ats').cli_selection})")
        stages = len(args.pruning_locs or [])
        if ats_tokens is not None and len(ats_tokens) not in (1, stages):
            bad.append(f"--ats-tokens with {len(ats_tokens)} values for {stages} stages (one value for every stage, or one per --pruning-locs entry)")
        if ats_tokens is not None and any(v < 1 for v in ats_tokens):
            bad.append(f"--ats-tokens {' '.join(str(v) for v in ats_tokens)} (at least 1 token per stage)")
    elif ats_tokens is not None:
        bad.append(f"--ats-tokens with --method {method} (tokens are sampled by --method ats only)")
    for m in methods.METHODS:                # the families that --method alone selects and that bring flags of their own: avit, evo, ltp
        if not m.flags:
            continue
        if method != m.name:
            for attr, flag, _ in m.flags:
                if getattr(args, attr, None) is not None:
                    bad.append(f"{flag} with --method {method} (it sets the {m.title} baseline: --method {m.name})")
            continue
        for attr, flag in _NOT_WITH_ATS:
            if getattr(args, attr, None) not in (None, False):
                bad.append(f"{m.cli} with {flag} ({m.cli_selection})")
        _training_refusals(m, args, bad)
        if m.name == "evo":
            _evo_ranges(args, bad)
        if m.name == "ltp":
            _ltp_ranges(args, bad)
    if bool(getattr(args, "ragged_train", False)):
        if args.patch_score_threshold is None:
            bad.append("--ragged-train without --patch-score-threshold (it trains the dynamic keep ratio on the ragged packed batch; the "
                       "fixed-ratio path already trains on the kept tokens alone)")
        if method != "d2s":
            bad.append(f"--ragged-train with --method {args.method} (it trains the dense-to-sparse student's dynamic keep ratio: --method d2s)")
        if getattr(args, "gemm_mode", "exact") == "bf16":
            bad.append("--ragged-train with --gemm-mode bf16 (training through a ragged block is built on the fp32 data path; exact and split run)")
        if getattr(args, "drop_path", 0.0) > 0.0:
            bad.append(f"--ragged-train with --drop-path {args.drop_path} (stochastic depth is not built for a ragged block)")
        if args.torch_optim:
            bad.append("--ragged-train with --torch-optim (the packed outputs go through the fused step only)")
        if args.eval_only:
            bad.append("--ragged-train with --eval-only (evaluation runs the inference cascade either way: drop one of the two)")
    if bool(getattr(args, "ragged_bf16", False)):
        # the flag, not the mode, selects the path (as --tome-bf16): it sets the bf16 arithmetic mode itself, --gemm-mode bf16 stays refused above
        if not getattr(args, "ragged_train", False):
            bad.append("--ragged-bf16 without --ragged-train (it puts training on the ragged packed batch into the bf16 arithmetic mode)")
        if getattr(args, "gemm_mode", "exact") == "split":
            bad.append("--ragged-bf16 with --gemm-mode split (the flag sets the bf16 arithmetic mode itself: leave --gemm-mode at exact)")
    if args.patch_score_threshold is not None:
        print("Attention: --patch-score-threshold: the reference's losses and inference branch cannot run on this path (losses.py:81,216-218, "
              "dynamic_vit.py:936); this build follows its training forward line by line and the documented fix for the rest (DESIGN.md section 10)")
        if len(args.pruning_locs) > 1 and not getattr(args, "ragged_cascade", False):
            bad.append("--patch-score-threshold with more than one pruning stage (ragged inference supports one stage: the reference's "
                       "second stage cannot run, dynamic_vit.py:945-946); --ragged-cascade selects this build's definition of the later stages")
        elif len(args.pruning_locs) > 1 and args.predictor_bn:
            bad.append("--ragged-cascade with --predictor-bn and more than one pruning stage (a stage on a ragged packed batch needs the "
                       "LayerNorm predictor)")
        elif len(args.pruning_locs) > 1:
            print("Attention: --ragged-cascade: at inference every threshold stage after the first scores and selects, per image, among the "
                  "tokens that survived the stages before it and packs the batch again - this build's definition, the reference's second "
                  "stage cannot run (dynamic_vit.py:945-946; DESIGN.md section 10); a packed stage adds no mask-loss term at validation"
                  + (" (with --ragged-train it does)" if getattr(args, "ragged_train", False) else ""))
        if getattr(args, "ragged_train", False):
            print("Attention: --ragged-train: training follows the cascade definition too - the training forward packs every stage's "
                  "survivors and runs the later blocks on them alone (selection without gradient), a later stage scores the survivors only "
                  "and adds its own mask-loss term, in training and at validation (this build's definition; DESIGN.md section 10.2)")
        if getattr(args, "ragged_train", False) and getattr(args, "ragged_bf16", False):
            print("Attention: --ragged-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path - GEMMs, the ragged attention "
                  "and its backward on the bf16 matrix cores, the residual stream, the selection and the row moves in fp32 (DESIGN.md "
                  "section 10.3)")
    if tome_train_bf16 and tome_train and method == "tome":
        print("Attention: --tome-train-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path - GEMMs, the (key-weighted) "
              "attention and its backward on the bf16 matrix cores, the residual stream, the match and the merge in fp32; validation runs "
              "the bf16 merging trunk (DESIGN.md section 22)")
    if ats_train_bf16 and ats_train and method == "ats":
        print("Attention: --ats-train-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path - GEMMs, the ragged attention "
              "and its backward on the bf16 matrix cores, the residual stream, the selection and the row moves in fp32, a stage's backward "
              "handing on both forms of the gradient (DESIGN.md section 24)")
    if avit_bf16 and method == "avit" and not args.eval_only:
        print("Attention: --avit-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path - GEMMs, the ragged attention and "
              "its backward on the bf16 matrix cores, the residual stream, the halting step and the row moves in fp32, every block "
              "boundary's backward one launch that hands on both forms of the gradient (DESIGN.md section 25)")
    if ltp_bf16 and method == "ltp":
        print("Attention: --ltp-bf16: every phase and the evaluation run in the bf16 arithmetic mode on the bf16 data path - GEMMs, the "
              "ragged and the policy attention and their backwards on the bf16 matrix cores, the score rebuilt there from the bf16 qkv and "
              "the bf16 kernels' log-sum-exp; the residual stream, the thresholds' comparison, the soft mask and the row moves in fp32 "
              "(DESIGN.md section 27)")
    if args.early_exit:
        print("Attention: --early-exit creates the extra head but, as in the reference, nothing calls it (dynamic_vit.py:752-758)")
    if args.random_drop:
        # stored on the model and used for the job name only (dynamic_vit.py:748, mask_predictor.py:79-80): no effect on the forward
        print("Attention: --random-drop has no effect on the forward pass at this commit of the reference (attribute only)")
    if args.mask_loss_type not in ("kl_div", "mse"):
        bad.append(f"--mask-loss-type {args.mask_loss_type} (kl_div and mse are on the path; bce is broken in the reference)")
    if not 0.0 <= getattr(args, "drop_path", 0.0) < 1.0:
        bad.append(f"--drop-path {args.drop_path} (0 <= rate < 1)")
    if getattr(args, "diff_topk", False):
        if not args.topk_selection:
            bad.append("--diff-topk without --topk-selection (the perturbed top-k acts on the score predictor's keep probabilities)")
        if args.patch_score_threshold is not None:
            bad.append("--diff-topk with --patch-score-threshold (the soft gather applies to the fixed-ratio path only)")
        if getattr(args, "topk_samples", 500) < 1:
            bad.append(f"--topk-samples {args.topk_samples} (at least 1)")
    if getattr(args, "fuse_dropped", False):
        if not args.topk_selection:
            bad.append("--fuse-dropped without --topk-selection (the package token is weighted by the score predictor's keep probabilities)")
        if args.patch_score_threshold is not None:
            bad.append("--fuse-dropped with --patch-score-threshold (no token is removed there: nothing to fuse)")
        if getattr(args, "diff_topk", False):
            bad.append("--fuse-dropped with --diff-topk (the soft gather has no dropped set)")
    if getattr(args, "squeeze_dropped", False):
        if method in ("dynamicvit", "tome"):
            bad.append(f"--squeeze-dropped with --method {args.method} (dropped tokens are squeezed into kept ones in the dense-to-sparse "
                       "student only)")
        if not args.topk_selection:
            bad.append("--squeeze-dropped without --topk-selection (the kept and dropped sets are those of the hard top-k)")
        if getattr(args, "fuse_dropped", False):
            bad.append("--squeeze-dropped with --fuse-dropped (a dropped token goes into the package token or into its nearest kept token, "
                       "not both)")
        if getattr(args, "diff_topk", False):
            bad.append("--squeeze-dropped with --diff-topk (the soft gather has no dropped set)")
        if args.patch_score_threshold is not None:
            bad.append("--squeeze-dropped with --patch-score-threshold (no token is removed there: nothing to squeeze)")
    if getattr(args, "attn_selection", False):
        if method == "dynamicvit":
            bad.append("--method dynamicvit with --attn-selection (the baseline keeps tokens by its own Gumbel decision and predictor)")
        if not args.topk_selection:
            bad.append("--attn-selection without --topk-selection (the CLS attention is ranked by the hard top-k of the fixed-ratio path; "
                       "the reference's recipe sets both, mask_predictor.py:147-148)")
        if args.patch_score_threshold is not None:
            bad.append("--attn-selection with --patch-score-threshold (attention selection applies to the fixed-ratio path only)")
        if getattr(args, "diff_topk", False):
            bad.append("--attn-selection with --diff-topk (the perturbed top-k trains the score predictor, which attention selection never calls)")
        if 0 in list(args.pruning_locs or []):
            bad.append("--attn-selection with a pruning location of 0 (a stage is scored by the CLS attention of the block before it)")
    graph_rank = getattr(args, "graph_rank", 0)          # no attribute unless given
    if hasattr(args, "graph_rank"):
        if graph_rank < 1:
            bad.append(f"--graph-rank {graph_rank} (at least 1 PageRank iteration)")
        if method != "d2s":
            bad.append(f"--graph-rank with --method {method} (graph ranking is a rule of the dense-to-sparse student's attention selection)")
        elif not getattr(args, "attn_selection", False):
            bad.append("--graph-rank without --attn-selection (it replaces the CLS attention row that attention selection ranks)")
        if getattr(args, "gemm_mode", "exact") == "bf16":
            bad.append("--graph-rank with --gemm-mode bf16 (the rank is recomputed from the block's fp32 qkv; exact and split run)")
    sim_prune = getattr(args, "sim_prune", 0)            # no attribute unless given
    if hasattr(args, "sim_prune"):
        if sim_prune < 1:
            bad.append(f"--sim-prune {sim_prune} (at least 1 candidate pruned by similarity)")
        if method != "d2s":
            bad.append(f"--sim-prune with --method {method} (the similarity stage is a rule of the dense-to-sparse student's attention selection)")
        elif not getattr(args, "attn_selection", False):
            bad.append("--sim-prune without --attn-selection (it prunes among the candidates that attention selection ranks by importance)")
        if getattr(args, "gemm_mode", "exact") == "bf16":
            bad.append("--sim-prune with --gemm-mode bf16 (the key metric is computed from the block's fp32 qkv; exact and split run)")
    if getattr(args, "accum_steps", 1) < 1:
        bad.append(f"--accum-steps {args.accum_steps} (at least 1)")
    if getattr(args, "clip_grad", None) is not None and not args.clip_grad > 0:
        bad.append(f"--clip-grad {args.clip_grad} (a norm > 0)")
    if args.use_dp:
        bad.append("--use-dp (one process per GPU only: --use-ddp under torch.distributed.run)")
    folder = getattr(args, "data_source", "synthetic") == "folder"
    if folder:
        if not args.imgnet_val_dir:
            bad.append("--data-source folder needs --imgnet-val-dir DIR (an ImageFolder: one sub-directory per class)")
        if args.train_interpolation not in ("bilinear", "bicubic", "random"):
            bad.append(f"--train-interpolation {args.train_interpolation} (bilinear, bicubic and random are built)")
        if (args.cutmix > 0 or args.cutmix_minmax is not None) and not args.mixup > 0:
            bad.append("--cutmix without --mixup > 0 (BackboneLoss takes soft targets only when mixup > 0, as the reference does, and "
                       "would read the soft labels as hard ones)")
        if args.mixup_mode not in ("batch", "pair", "elem"):
            bad.append(f"--mixup-mode {args.mixup_mode} (batch, pair or elem)")
        if args.recount > 8:
            bad.append("--recount above 8 (erase boxes per image)")
        if not 0 <= args.num_workers <= 16:
            bad.append("--num-workers outside 0..16")
        try:
            from d2s import data
            data.parse_auto_augment(args.aa)
        except ValueError as e:
            bad.append(f"--aa: {e}")
        if args.color_jitter < 0:
            bad.append(f"--color-jitter {args.color_jitter} (a single non-negative strength)")
    if args.resume and args.torch_optim:
        bad.append("--resume with --torch-optim (a checkpoint restores the fused step's arenas; that recipe has none)")
    if args.model_ema and args.torch_optim:
        bad.append("--model-ema with --torch-optim (the moving average is kept inside the fused AdamW launch)")
    if args.model_ema and not 0.0 <= args.model_ema_decay < 1.0:
        bad.append(f"--model-ema-decay {args.model_ema_decay} (0 <= decay < 1)")
    if args.eval_only and not (args.resume or args.student_checkpoint):
        bad.append("--eval-only without weights to load (--resume FILE or --student-checkpoint FILE)")
    if args.save_every < 1:
        bad.append(f"--save-every {args.save_every} (at least 1)")
    if bad:
        raise SystemExit("not on the accelerated path: " + "; ".join(bad))
    if args.output_dir and args.torch_optim and not args.eval_only:
        print("Attention: --output-dir with --torch-optim saves the student's weights only ('model', epoch, best_acc): such a file "
              "loads through --student-checkpoint, it cannot be resumed")
    if methods.by_name(method).flags:
        args.warmup_steps = 0                # not given (refused above otherwise)
        for attr, value in methods.flag_values(methods.by_name(method), args).items():
            setattr(args, attr, value)
    if ats_train:
        args.warmup_steps = 0                # not given (refused above otherwise): the reference's default of 5 predictor-only epochs has no meaning here
    if tome_train and args.warmup_steps > 0:
        print("Attention: --tome-train trains a model without score predictors, so the predictor warm-up has no meaning "
              "(mask_predictor.py:300): --warmup-steps is set to 0")
        args.warmup_steps = 0
    if getattr(args, "attn_selection", False):
        print("Attention: --attn-selection selects tokens by the student's own CLS attention and never calls the score predictors, so the "
              "predictor warm-up has no meaning (mask_predictor.py:300): --warmup-steps is set to 0"
              + (" (--mean-heads: mean over heads instead of max)" if args.mean_heads else ""))
        args.warmup_steps = 0
        if graph_rank > 0:
            print(f"Attention: --graph-rank {graph_rank} ranks every stage's tokens by {graph_rank} PageRank iteration"
                  f"{'s' if graph_rank > 1 else ''} over the attention graph of the block before it instead of by that block's CLS row "
                  "(the importance stage of Zero-TPrune; DESIGN.md section 29)")
        if sim_prune > 0:
            print(f"Attention: --sim-prune {sim_prune} lets every stage rank {sim_prune} candidate{'s' if sim_prune > 1 else ''} more than it "
                  f"keeps and prunes, from the less important half, the {sim_prune} whose keys resemble a more important candidate most "
                  "(the similarity stage of Zero-TPrune; a stage clips the count to its k and to T - k; DESIGN.md section 30)")
    elif args.mean_heads:
        print("Attention: --mean-heads has no effect without --attn-selection (it chooses how attention selection aggregates the heads, "
              "losses.py:126)")
    if args.predictor_bn and args.use_ddp:
        print("Attention: --predictor-bn keeps per-rank batch statistics (not synchronised), exactly like the reference")
    if folder:
        return
    if args.mixup > 0 or args.cutmix > 0 or args.cutmix_minmax is not None:
        print("Attention: mixup/cutmix are not used (synthetic batches)")
    args.mixup, args.cutmix, args.cutmix_minmax = 0.0, 0.0, None


def build_models(args):
    """mask_predictor.py:170-202 (the arch switch), with local checkpoints instead of URL downloads."""
    arch = args.arch if args.arch in _STUDENTS else "deit_small"
    method = getattr(args, "method", "d2s")
    if method == "ats" and not getattr(args, "ats_train", False):
        return build_ats(args), None                 # inference only: no teacher
    ats_kw = {"train_bf16": True} if getattr(args, "ats_train_bf16", False) else {}
    build = {"ats": lambda a: build_ats(a, train_sample=True, **ats_kw), "avit": build_avit, "evo": build_evo, "ltp": build_ltp}.get(method)
    if build is not None:
        # the family's student from --student-checkpoint; the dense teacher as for the other methods, unless --dist-weight 0
        teacher = _teacher(args)
        return build(args), teacher
    if method == "dynamicvit":
        student = getattr(vit_models, "default_" + _STUDENTS[arch])(args.pruning_locs, args.keep_ratios,
                                                                    drop_path_rate=getattr(args, "drop_path", 0.0),
                                                                    checkpoint_path=args.student_checkpoint)
        teacher = getattr(vit_models, "default_" + _TEACHERS[arch])(checkpoint_path=args.teacher_checkpoint)
        return student.to(args.device), teacher.to(args.device)
    student = getattr(vit_models, _STUDENTS[arch])(args.pruning_locs, args.keep_ratios, topk_selection=args.topk_selection,
                                                   early_exit=args.early_exit, mean_heads=args.mean_heads,
                                                   random_drop=args.random_drop, small_predictor=args.small_predictor,
                                                   predictor_loss_type=args.mask_loss_type, predictor_bn=args.predictor_bn,
                                                   patch_score_threshold=args.patch_score_threshold,
                                                   drop_path_rate=getattr(args, "drop_path", 0.0),
                                                   diff_topk=getattr(args, "diff_topk", False),
                                                   topk_num_samples=getattr(args, "topk_samples", 500),
                                                   fuse_dropped=getattr(args, "fuse_dropped", False),
                                                   squeeze_dropped=getattr(args, "squeeze_dropped", False),
                                                   attn_selection=getattr(args, "attn_selection", False),
                                                   checkpoint_path=args.student_checkpoint,
                                                   **({"ragged_train": True} if getattr(args, "ragged_train", False) else {}),
                                                   **({"ragged_bf16": True} if getattr(args, "ragged_bf16", False) else {}),
                                                   **({"graph_rank_iters": int(args.graph_rank)} if getattr(args, "graph_rank", 0) else {}),
                                                   **({"sim_prune": int(args.sim_prune)} if getattr(args, "sim_prune", 0) else {}))
    teacher = getattr(vit_models, _TEACHERS[arch])(checkpoint_path=args.teacher_checkpoint)
    return student.to(args.device), teacher.to(args.device)


def _teacher(args):
    """The dense teacher of a logits-only student, or None under --dist-weight 0: such a student trains without one."""
    if args.dist_weight == 0:
        return None
    arch = args.arch if args.arch in _TEACHERS else "deit_small"
    return getattr(vit_models, _TEACHERS[arch])(checkpoint_path=args.teacher_checkpoint).to(args.device)


def _trunk(name, args, *a, **kw):
    """The family's factory for --arch, called with a and kw; weights as load_trunk finds them."""
    m = methods.by_name(name)
    model = getattr(vit_models, m.factory(args.arch if args.arch in _STUDENTS else "deit_small"))(*a, **kw)
    return load_trunk(args, model, m.name, m.no_predictor)


def build_tome(args):
    """--method tome: the dense DeiT trunk with token merging, weights from --student-checkpoint or the 'model' entry of a --resume file.  A
    dense-to-sparse student's checkpoint carries score predictors this model has no use for: they are ignored (strict=False)."""
    return _trunk("tome", args, args.tome_r, train_merge=bool(getattr(args, "tome_train", False)), bf16=bool(getattr(args, "tome_bf16", False)),
                  **({"train_bf16": True} if getattr(args, "tome_train_bf16", False) else {}))


def load_trunk(args, model, method, why):
    """Weights of a predictor-free baseline from --student-checkpoint or the 'model' entry of a --resume file.  A dense-to-sparse student's
    checkpoint carries score predictors such a model has no use for: they are counted and ignored (strict=False)."""
    path = args.student_checkpoint or args.resume
    if path is None:
        print(f"--method {method}: no --student-checkpoint, the trunk starts from its random initialisation")
        return model.to(args.device)
    sd = vit_models.checkpoint_filter_fn(torch.load(path, map_location="cpu", weights_only=True), model)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not (method == "ltp" and k == "ltp_threshold")]      # a DeiT checkpoint: the thresholds keep their initial values
    if missing:
        raise SystemExit(f"{path}: no weights for {len(missing)} tensors of the trunk, first {missing[0]}")
    pred = [k for k in unexpected if 'predictor' in k]
    print(f"--method {method}: trunk weights from {path}; ignored {len(pred)} predictor tensors" +
          (f" and {len(unexpected) - len(pred)} others, first {[k for k in unexpected if k not in pred][0]}" if len(unexpected) > len(pred) else "") +
          f" ({why})")
    return model.to(args.device)


def build_ats(args, **kw):
    """--method ats: the dense DeiT trunk with a sampling stage in every block of --pruning-locs, at most --ats-tokens tokens each.
    kw: train_sample=True under --ats-train (and train_bf16=True under --ats-train-bf16), nothing otherwise."""
    toks = getattr(args, "ats_tokens", None)
    if toks is not None and len(toks) == 1:
        toks = int(toks[0])
    return _trunk("ats", args, ats_locs=list(args.pruning_locs), ats_tokens=toks, **kw)


def build_avit(args):
    """--method avit: the dense DeiT trunk with per-token adaptive depth; the gate constants and the prior's target depth from --avit-*."""
    v = methods.flag_values(methods.by_name("avit"), args)
    return _trunk("avit", args, gate_scale=v["avit_gate_scale"], gate_center=v["avit_gate_center"], target_depth=v["avit_target_depth"],
                  **({"train_bf16": True} if getattr(args, "avit_bf16", False) else {}))


def build_evo(args):
    """--method evo: the dense DeiT trunk with the slow-fast token update from block --evo-start on."""
    return _trunk("evo", args, **methods.flag_values(methods.by_name("evo"), args))


def build_ltp(args):
    """--method ltp: the dense DeiT trunk with one learnable threshold per block of --pruning-locs; phase, temperature and the initial
    thresholds from --ltp-*.  A DeiT checkpoint has no ltp_threshold: the thresholds then keep their initial values; a checkpoint of an
    earlier LTP run (the soft phase's best.pt) brings its own."""
    v = methods.flag_values(methods.by_name("ltp"), args)
    return _trunk("ltp", args, pruning_loc=list(args.pruning_locs), ltp_temperature=v["ltp_temperature"],
                  ltp_init_threshold=v["ltp_init_threshold"], ltp_phase=v["ltp_phase"],
                  **({"train_bf16": True} if getattr(args, "ltp_bf16", False) else {}))


def folder_loaders(args, samples, split, epoch, rank, world):
    """The reference's ImageFolder loaders (mask_predictor.py:234-259, ddp_training.py:15-20) on the GPU input pipeline (d2s.data): the
    training subset in a new order per epoch, one DistributedSampler-style shard per rank; Mixup when the reference enables it."""
    from d2s import data
    train_idx, val_idx = split
    mix = None
    if args.mixup > 0 or args.cutmix > 0 or args.cutmix_minmax is not None:                                # :261-267
        mix = data.MixConfig(args.mixup, args.cutmix, tuple(args.cutmix_minmax) if args.cutmix_minmax else None, args.mixup_prob,
                             args.mixup_switch_prob, args.mixup_mode, args.smoothing, args.nb_classes)
    opts = data.AugmentOptions(args.train_interpolation, args.reprob, args.remode, args.recount, auto_augment=args.aa or "",
                               color_jitter=args.color_jitter)
    common = dict(seed=42, epoch=epoch, rank=rank, num_workers=args.num_workers)
    train = data.FolderLoader(samples, data.shard(data.epoch_order(train_idx, 42, epoch), rank, world), args.batch_size, args.device,
                              train=True, opts=opts, mix=mix, **common)
    val = data.FolderLoader(samples, data.shard(val_idx, rank, world), args.batch_size, args.device, train=False, **common)
    return train, val


def save_checkpoints(args, optim, student, epoch, best_acc, improved, first):
    """Rank 0, after an epoch: DIR/last.pt (every --save-every epochs and after the final one) and, when val_acc improved, DIR/best.pt.
    Each goes to a temporary name first (utils.atomic_save)."""
    last = (epoch + 1) % args.save_every == 0 or epoch == args.epochs - 1
    if not (last or improved):
        return first
    t0 = time.time()
    if args.torch_optim:
        sd = {"model": {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}, "epoch": epoch, "best_acc": float(best_acc)}
    else:
        sd = optim.state_dict(best_acc=best_acc, epoch=epoch)
    os.makedirs(args.output_dir, exist_ok=True)
    for name, wanted in (("last.pt", last), ("best.pt", improved)):
        if wanted:
            utils.atomic_save(sd, os.path.join(args.output_dir, name))
            if first:       # the cost of --save-every 1, once
                size = os.path.getsize(os.path.join(args.output_dir, name))
                print(f"checkpoint: state_dict + write of {name} took {time.time() - t0:.3f} s ({size / 1e6:.1f} MB)")
                first = False
    return first


def eval_tome(args, rank, world, distributed):
    """--method tome / --method ats --eval-only: no teacher pass, no TrainStep - the model, the validation loader, one evaluation."""
    model = build_ats(args) if args.method == "ats" else build_tome(args)
    if args.data_source == "folder":
        from d2s import data
        samples, classes = data.image_folder(args.imgnet_val_dir)
        if len(classes) > args.nb_classes:
            raise SystemExit(f"{len(classes)} classes in {args.imgnet_val_dir}, the heads have {args.nb_classes}")
        _, val_loader = folder_loaders(args, samples, data.split_indices(len(samples)), 0, rank, world)
    else:
        val_loader = utils.SyntheticLoader(args.val_steps, args.batch_size, 224, seed=777 + rank, device=args.device)
    metrics = evaluate_performance(args, model, torch.nn.Identity(), val_loader)
    if distributed:
        import torch.distributed as dist
        t = torch.tensor([metrics["val_acc"]], device=args.device)
        dist.all_reduce(t)
        metrics["val_acc"] = float(t / world)
        dist.destroy_process_group()
    if rank == 0 and args.method == "ats":
        per = [c.float() for c in model.tokens_per_stage]       # the last validation batch's
        print(f"eval only: --method ats --pruning-locs {' '.join(str(v) for v in model.ats_locs)} (gemm mode {args.gemm_mode}): "
              f"ats tokens per stage: mean {[round(float(c.mean()), 1) for c in per]} min {[int(c.min()) for c in per]} "
              f"max {[int(c.max()) for c in per]}, " + ", ".join(f"{k}={v:.4f}" for k, v in sorted(metrics.items()) if isinstance(v, float)))
    elif rank == 0:
        path_ran = "bf16 data path" if getattr(model, "bf16", False) else f"fp32 data path, gemm mode {args.gemm_mode}"
        print(f"eval only: --method tome --tome-r {args.tome_r} ({path_ran}): tokens per block {model.tokens_per_block}, " +
              ", ".join(f"{k}={v:.4f}" for k, v in sorted(metrics.items()) if isinstance(v, float)))
    return metrics["val_acc"]


def main(argv=None):
    args = utils.parse_args(argv)
    check_supported(args)
    if not torch.cuda.is_available():
        raise SystemExit("mask_predictor.py needs a GPU: the path has no CPU fallback")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = args.use_ddp and world > 1
    torch.cuda.set_device(local)
    args.device = torch.device("cuda", local)
    args.world_size, args.job_name, args.nb_classes, args.step = world, "synthetic_job", 1000, 0
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)          # RCCL
    # --ragged-bf16, --tome-train-bf16, --ats-train-bf16 and --avit-bf16 set the bf16 arithmetic mode themselves, as --gemm-mode bf16 would
    # (which stays refused with --ragged-train, with --method tome, with --ats-train and with training --method avit)
    own_bf16 = any(getattr(args, f, False) for f in ("ragged_bf16", "tome_train_bf16", "ats_train_bf16", "avit_bf16", "ltp_bf16"))
    ops.set_gemm_mode({"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}["bf16" if own_bf16 else args.gemm_mode])
    torch.manual_seed(42)                                                     # mask_predictor.py:43-44
    if (args.method == "ats" and not args.ats_train) or (args.method == "tome" and not args.tome_train):
        return eval_tome(args, rank, world, distributed)
    if args.method == "tome":
        # --tome-train: the merging student from --student-checkpoint; the dense teacher as for the other methods, unless --dist-weight 0
        student, teacher = build_tome(args), _teacher(args)
    else:
        student, teacher = build_models(args)
    if rank == 0:
        for key in sorted(vars(args), key=str.lower):
            print(f'{key}: {getattr(args, key)}')
    if args.freeze_backbone:                                                  # :218-224
        print('Freezing whole student, except predictor network')
        for n, p in student.named_parameters():
            p.requires_grad = 'predictor' in n
    step_teacher = teacher
    if teacher is not None:
        teacher.eval()
        for p in teacher.parameters():
            p.requires_grad = False
    else:
        teacher = torch.nn.Identity()        # what the evaluation of a logits-only model is handed (eval_tome does the same)
    if args.torch_optim:
        if distributed:
            raise SystemExit("--torch-optim is the single-process reference recipe; drop it for --use-ddp")
        optim = torch.optim.AdamW(utils.get_param_groups(student, args), lr=args.lr, weight_decay=args.weight_decay)   # :213,229-230
    else:
        optim = TrainStep(student, step_teacher, args, lr=args.lr, min_lr=args.min_lr, weight_decay=args.weight_decay, epochs=args.epochs,
                          warmup_steps=args.warmup_steps, distributed=distributed, accum_steps=args.accum_steps, clip_grad=args.clip_grad)
        if distributed:
            dist.broadcast(optim.arena.params, src=0)
    start_epoch, best_acc = 0, 0.0
    if not args.torch_optim:
        if args.model_ema:
            optim.enable_ema(args.model_ema_decay)
        if args.resume:                   # every rank reads the file; nothing from it is executed
            sd = torch.load(args.resume, map_location="cpu", weights_only=True)
            start_epoch = optim.load_state_dict(sd) + 1
            best_acc = float(sd["best_acc"])
            print(f"Resumed {args.resume}: epoch {start_epoch} is finished, best val acc so far {best_acc:4f}")
            del sd
    n_pred = sum(p.numel() for n, p in student.named_parameters() if 'predictor' in n and p.requires_grad)
    print(f'Total number of trainable parameters in predictor network in millions: {n_pred / 1e6}')
    folder = args.data_source == "folder"
    if folder:
        from d2s import data
        samples, classes = data.image_folder(args.imgnet_val_dir)
        if len(classes) > args.nb_classes:
            raise SystemExit(f"{len(classes)} classes in {args.imgnet_val_dir}, the heads have {args.nb_classes}")
        split = data.split_indices(len(samples))
        print(f"{len(samples)} images in {len(classes)} classes: {len(split[0])} train / {len(split[1])} val")
    img = 224
    if args.eval_only:
        if folder:
            _, val_loader = folder_loaders(args, samples, split, 0, rank, world)
        else:
            val_loader = utils.SyntheticLoader(args.val_steps, args.batch_size, img, seed=777 + rank, device=args.device)
        metrics = evaluate_performance(args, student, teacher, val_loader)
        if args.model_ema and args.resume:
            with optim.ema_weights():
                metrics["val_acc_ema"] = evaluate_performance(args, student, teacher, val_loader)["val_acc"]
        if distributed:
            keys = [k for k in ("val_acc", "val_acc_ema") if k in metrics]
            t = torch.tensor([metrics[k] for k in keys], device=args.device)
            dist.all_reduce(t)
            metrics.update(zip(keys, (t / world).tolist()))
            dist.destroy_process_group()
        if rank == 0:
            print("eval only: " + ", ".join(f"{k}={v:.4f}" for k, v in sorted(metrics.items()) if isinstance(v, float)))
        return metrics["val_acc"]
    print(f"Start training for {args.epochs} epochs, with batch size of {args.batch_size}")
    if args.accum_steps > 1 or args.clip_grad is not None:
        print(f"Optimiser step: {args.accum_steps} batch(es) x {args.batch_size} images x {world} rank(s) = "
              f"{args.accum_steps * args.batch_size * world} images"
              + (f", gradient clipped to norm {args.clip_grad}" if args.clip_grad is not None else ""))
    since = time.time()
    first_save = True
    for epoch in range(start_epoch, args.epochs):
        args.step = epoch
        print('Epoch {}/{}'.format(epoch + 1, args.epochs))
        print('-' * 50)
        if args.torch_optim:
            utils.adjust_learning_rate(optim.param_groups, args, epoch, student, warmup_predictor=False,
                                       warming_up_step=args.warmup_steps, base_multi=0.1)                  # :300-301
        else:
            optim.set_epoch(epoch)
        if args.topk_selection:
            args.current_sigma = utils.current_sigma(args, epoch)       # the fused step's schedule does not touch args
            student.current_sigma = args.current_sigma
            print(f"### current_sigma = {args.current_sigma:.6f}" + (" (perturbed top-k soft gather)" if getattr(args, "diff_topk", False) else ""))
        if folder:
            train_loader, val_loader = folder_loaders(args, samples, split, epoch, rank, world)
            n_images = len(train_loader.set.order)
        else:
            train_loader = utils.SyntheticLoader(args.steps_per_epoch, args.batch_size, img, seed=1000 * epoch + rank, device=args.device)
            val_loader = utils.SyntheticLoader(args.val_steps, args.batch_size, img, seed=777 + rank, device=args.device)
            n_images = args.steps_per_epoch * args.batch_size
        t0 = time.time()
        train_metrics = train_one_epoch(args, student, teacher, train_loader, optim, None)                  # :308
        torch.cuda.synchronize()
        dt = time.time() - t0
        val_metrics = evaluate_performance(args, student, teacher, val_loader)                              # :310
        epoch_metrics = dict(train_metrics, **val_metrics)
        if args.model_ema:                # the same student object scores its moving average: the arenas trade contents and trade back
            with optim.ema_weights():
                epoch_metrics["val_acc_ema"] = evaluate_performance(args, student, teacher, val_loader)["val_acc"]
        if distributed:                                                                                     # ddp_training.py:174-177,213
            keys = ["train_loss", "val_acc"] + (["val_acc_ema"] if args.model_ema else [])
            t = torch.tensor([epoch_metrics[k] for k in keys], device=args.device)
            dist.all_reduce(t)
            epoch_metrics.update(zip(keys, (t / world).tolist()))
            dist.barrier()
        if args.output_dir:
            # best.pt follows val_acc, as the reference tracks it: written after the first evaluated epoch whatever its accuracy, replaced
            # only by a strictly better one.  All ranks hold the same arenas after the reduced step, so rank 0 alone writes.
            improved = epoch_metrics['val_acc'] > best_acc or not os.path.exists(os.path.join(args.output_dir, "best.pt"))
            if distributed:
                flag = torch.tensor([1.0 if improved else 0.0], device=args.device)
                dist.broadcast(flag, src=0)          # only rank 0 looks at the directory
                improved = bool(flag.item())
        best_acc = max(best_acc, epoch_metrics['val_acc'])
        if args.output_dir:
            if rank == 0:
                first_save = save_checkpoints(args, optim, student, epoch, best_acc, improved, first_save)
            if distributed:
                dist.barrier()
        if rank == 0 and args.method == "tome":
            print(f"--method tome --tome-r {args.tome_r} --tome-train: tokens per block {student.tokens_per_block}")
        if rank == 0 and args.method == "ats":
            per = [c.float() for c in student.tokens_per_stage]       # the last validation batch's
            print(f"--method ats --pruning-locs {' '.join(str(v) for v in student.ats_locs)} --ats-train: ats tokens per stage: "
                  f"mean {[round(float(c.mean()), 1) for c in per]} min {[int(c.min()) for c in per]} max {[int(c.max()) for c in per]}")
        if rank == 0 and args.method == "avit":
            print(f"--method avit: tokens per layer {student.tokens_per_layer} (the last validation batch's), "
                  f"train_avg_depth={float(epoch_metrics['train_avg_depth']):.3f}, train_ponder_loss={float(epoch_metrics['train_ponder_loss']):.4f}, "
                  f"train_prior_loss={float(epoch_metrics['train_prior_loss']):.4f}")
        if rank == 0 and args.method == "ltp":
            print(f"--method ltp --ltp-phase {args.ltp_phase} --pruning-locs {' '.join(str(v) for v in student.pruning_loc)}: tokens per block "
                  f"{student.tokens_per_block} (the last validation batch's), thresholds "
                  f"{[round(v, 6) for v in student.ltp_threshold.detach().cpu().tolist()]}, train_ltp_reg={float(epoch_metrics['train_ltp_reg']):.4f}, "
                  f"train_avg_tokens={float(epoch_metrics['train_avg_tokens']):.1f}, val_avg_tokens={float(epoch_metrics['val_avg_tokens']):.1f}")
        if rank == 0 and args.method == "evo":
            print(f"--method evo --evo-start {args.evo_start} --evo-keep {args.evo_keep} --evo-tradeoff {args.evo_tradeoff}: "
                  f"tokens per block {student.tokens_per_block}")
        if rank == 0:
            print(f"epoch {epoch + 1}: {n_images * world / dt:.1f} train images/s, " +
                  ", ".join(f"{k}={v:.4f}" for k, v in sorted(epoch_metrics.items()) if isinstance(v, float)))
    elapsed = time.time() - since
    print(f'Training complete in {(elapsed // 60):.0f}m {(elapsed % 60):.0f}s')
    print(f'Best val acc: {best_acc:4f}')
    if distributed:
        dist.destroy_process_group()
    return best_acc


if __name__ == '__main__':
    main()
