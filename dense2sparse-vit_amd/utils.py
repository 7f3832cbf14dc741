"""Hot-path subset of the reference's utils.py: the optimiser parameter groups and the per-epoch learning-rate / freeze
schedule, with the reference's signatures (utils.py:67-147).  (The reference file itself needs torchvision and the whole model
zoo to import.)"""
import math

import torch


def get_param_groups(model, args):
    """utils.py:67-90."""
    decay, no_decay, predictor, early_exit = [], [], [], []
    for name, param in model.named_parameters():
        if 'predictor' in name or 'dist' in name:
            predictor.append(param)
        elif 'early_exit' in name:
            early_exit.append(param)
        elif not param.requires_grad:
            continue
        elif 'cls_token' in name or 'pos_embed' in name:
            continue
        elif len(param.shape) == 1 or name.endswith(".bias"):
            no_decay.append(param)
        else:
            decay.append(param)
    return [{'params': predictor, 'weight_decay': args.weight_decay, 'name': 'predictor'},
            {'params': no_decay, 'weight_decay': 0., 'name': 'base_no_decay'},
            {'params': decay, 'weight_decay': args.weight_decay, 'name': 'base_decay'},
            {'params': early_exit, 'weight_decay': args.weight_decay, 'name': 'early_exit'}]


def current_sigma(args, step):
    """The perturbation scale of epoch `step` (utils.py:95-96 of the reference): linear from --initial-sigma to 0 at step == epochs"""
    return max(0, (1 - step / args.epochs) * args.initial_sigma)


def adjust_learning_rate(param_groups, args, step, model, warming_up_step=2, warmup_predictor=False, base_multi=0.1):
    """utils.py:93-147 for torch.optim param groups (d2s.engine.adjust_learning_rate is the same schedule for FusedAdamW)."""
    if getattr(args, "topk_selection", False):
        args.current_sigma = current_sigma(args, step)
    cos_lr = (math.cos(step / args.epochs * math.pi) + 1) * 0.5
    cos_lr = args.min_lr + cos_lr * (args.lr - args.min_lr)
    for n, p in model.named_parameters():
        p.requires_grad_(True if ('dist' in n or 'predictor' in n) else step >= args.warmup_steps)
    predictor_lr = cos_lr
    backbone_lr = 0 if step < args.warmup_steps else min(args.lr * 0.01, cos_lr)
    print(f'### Using lr {backbone_lr:.7f} for BACKBONE, cosine lr = {predictor_lr:.7f} for PREDICTOR')
    for param_group in param_groups:
        if param_group['name'] == 'predictor':
            param_group['lr'] = predictor_lr
            for p in param_group['params']:
                p.requires_grad_(predictor_lr != 0)
        elif param_group['name'] != 'early_exit':
            param_group['lr'] = backbone_lr
            for p in param_group['params']:
                p.requires_grad_(backbone_lr != 0)


class SyntheticLoader:
    """Deterministic stand-in for the ImageFolder loaders of build_data_sets.py: `steps` batches of N(0,1) images."""

    def __init__(self, steps, batch, img_size=224, num_classes=1000, seed=0, device="cpu", last_batch=None):
        """last_batch: size of the final batch (the reference's loaders use drop_last=False, ddp_training.py:15-20, so an epoch usually
        ends on a shorter batch); None = as long as the others."""
        self.steps, self.batch, self.img, self.nc, self.seed, self.device = steps, batch, img_size, num_classes, seed, device
        self.last_batch = last_batch

    def __len__(self):
        return self.steps

    def __iter__(self):
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        for i in range(self.steps):
            b = self.last_batch if (self.last_batch and i == self.steps - 1) else self.batch
            yield (torch.randn((b, 3, self.img, self.img), generator=g, device=self.device),
                   torch.randint(0, self.nc, (b,), generator=g, device=self.device))


class _Unset(int):
    """An argparse default that can be told from the same number given on the command line (parse_args sets warmup_steps_given)."""


def parse_args(argv=None):
    """The reference's command line (utils.py:182-317): same flag names, types and defaults, so job scripts written for the
    reference run unchanged.  With the default --data-source synthetic the data-set / augmentation flags are accepted and ignored;
    with --data-source folder they drive d2s.data (the tracking flags are always ignored).  The run flags added at the end are not in
    the reference."""
    import argparse
    import methods
    p = argparse.ArgumentParser(description='Transformers')
    p.add_argument('--arch', default='deit_small', type=str)
    p.add_argument('--is-sbatch', action='store_true', default=False)
    p.add_argument('--wandb', action='store_true', default=False)
    p.add_argument('--save-path', default='test_imgs/')
    p.add_argument('--model-name', type=str, default='deit_small_patch16_224')
    p.add_argument('--patch-size', default=16)
    p.add_argument('--use-shape', action='store_true', default=False)
    p.add_argument('--batch-size', default=64, type=int)
    p.add_argument('--epochs', default=25, type=int)
    p.add_argument('--use-dp', action='store_true', default=False)
    p.add_argument('--use-ddp', action='store_true', default=False)
    p.add_argument('--imgnet-val-dir', type=str, default="")
    p.add_argument('--weight-decay', type=float, default=0.05)
    p.add_argument('--lr', type=float, default=5e-4)
    p.add_argument('--warmup-lr', type=float, default=1e-6)
    p.add_argument('--min-lr', type=float, default=1e-5)
    p.add_argument('--warmup-steps', default=_Unset(5), type=int)
    p.add_argument('--early-exit', action='store_true', default=False)
    p.add_argument('--pruning-locs', nargs='+', default=[3], type=int)
    p.add_argument('--keep-ratios', nargs='+', type=float, default=[0.3])
    p.add_argument('--softmax-temp', default=1.0, type=float)
    p.add_argument('--use-ratio-loss', action='store_true', default=False)
    p.add_argument('--ratio-weight', default=2.0, type=float)
    p.add_argument('--use-token-dist-loss', action='store_true', default=False)
    p.add_argument('--dist-weight', default=0.5, type=float)
    p.add_argument('--teacher-cls-loss', action='store_true', default=False)
    p.add_argument('--cls-weight', default=1.0, type=float)
    p.add_argument('--topk-selection', action='store_true', default=False)
    p.add_argument('--mean-heads', action='store_true', default=False)
    p.add_argument('--random-drop', action='store_true', default=False)
    p.add_argument('--initial-sigma', default=0.05, type=float)
    p.add_argument('--attn-selection', action='store_true', default=False)
    p.add_argument('--cls-from-teacher', action='store_true', default=False)
    p.add_argument('--freeze-backbone', action='store_true', default=False)
    p.add_argument('--visualize-patch-drop', action='store_true', default=False)
    p.add_argument('--visualize-cls-attn-evo', action='store_true', default=False)
    p.add_argument('--small-predictor', action='store_true', default=False)
    p.add_argument('--mask-loss-type', default='kl_div', type=str)
    p.add_argument('--predictor-bn', action='store_true', default=False)
    p.add_argument('--patch-score-threshold', default=None, type=float)
    p.add_argument('--color-jitter', type=float, default=0.4)
    p.add_argument('--aa', type=str, default='rand-m9-mstd0.5-inc1')
    p.add_argument('--smoothing', type=float, default=0.1)
    p.add_argument('--train-interpolation', type=str, default='bicubic')
    p.add_argument('--repeated-aug', action='store_true')
    p.add_argument('--no-repeated-aug', action='store_false', dest='repeated_aug')
    p.set_defaults(repeated_aug=True)
    p.add_argument('--reprob', type=float, default=0.25)
    p.add_argument('--remode', type=str, default='pixel')
    p.add_argument('--recount', type=int, default=1)
    p.add_argument('--resplit', action='store_true', default=False)
    p.add_argument('--drop-path', type=float, default=0.0, metavar='RATE',
                   help="stochastic depth rate of the student's last block (DeiT's flag; block i drops with linspace(0, RATE, depth)[i])")
    p.add_argument('--mixup', type=float, default=0.8)
    p.add_argument('--cutmix', type=float, default=1.0)
    p.add_argument('--cutmix-minmax', type=float, nargs='+', default=None)
    p.add_argument('--mixup-prob', type=float, default=1.0)
    p.add_argument('--mixup-switch-prob', type=float, default=0.5)
    p.add_argument('--mixup-mode', type=str, default='batch')
    # ---- additions for synthetic / offline runs (not in the reference) ----
    p.add_argument('--steps-per-epoch', type=int, default=20, help='synthetic training batches per epoch')
    p.add_argument('--val-steps', type=int, default=2, help='synthetic validation batches per epoch')
    p.add_argument('--student-checkpoint', type=str, default=None, help='local DeiT checkpoint for the student (weights_only load)')
    p.add_argument('--teacher-checkpoint', type=str, default=None, help='local DeiT checkpoint for the teacher (weights_only load)')
    p.add_argument('--torch-optim', action='store_true', default=False,
                   help="the reference's recipe (torch.optim.AdamW over get_param_groups) instead of the fused arena step")
    p.add_argument('--gemm-mode', choices=['exact', 'split', 'bf16'], default='exact')
    p.add_argument('--data-source', choices=['synthetic', 'folder'], default='synthetic',
                   help='synthetic N(0,1) batches, or an ImageFolder at --imgnet-val-dir (80/20 train/val split, GPU augmentation)')
    p.add_argument('--num-workers', type=int, default=8, help='JPEG-decoding DataLoader workers of --data-source folder (at most 16)')
    p.add_argument('--output-dir', type=str, default=None,
                   help='after every epoch rank 0 writes DIR/last.pt, and DIR/best.pt when val_acc improved (default: nothing is written)')
    p.add_argument('--save-every', type=int, default=1, help='write last.pt every N epochs, and always after the final one')
    p.add_argument('--resume', type=str, default=None, help='continue the run saved in FILE (a last.pt / best.pt) with the epoch after it')
    p.add_argument('--eval-only', action='store_true', default=False,
                   help='with --resume or --student-checkpoint: load, run the evaluation once, print, exit')
    p.add_argument('--model-ema', action='store_true', default=False,
                   help='keep an exponential moving average of the student inside the fused AdamW launch; adds val_acc_ema to the epoch metrics')
    p.add_argument('--model-ema-decay', type=float, default=0.99996, help="decay of --model-ema (DeiT's default)")
    p.add_argument('--method', default='d2s', choices=[m.name for m in methods.METHODS],
                   help="d2s: the dense-to-sparse student (default); dynamicvit: the DynamicViT baseline (Gumbel keep decisions through policy "
                        "attention, dense training) with --ratio-weight / --dist-weight / --cls-weight as the weights of its objective; "
                        "tome: the Token Merging baseline (--tome-r; no predictor; --eval-only, or --tome-train to train through the merges); "
                        "ats: the Adaptive Token Sampling baseline (stages at --pruning-locs, --ats-tokens; no predictor; --eval-only, or --ats-train to "
                        "train through the stages); "
                        "avit: the A-ViT baseline (per-token adaptive depth: every token halts by its own cumulative score and leaves the ragged "
                        "packed batch, in training too; no predictor; --avit-* set the gate and the two penalty terms); "
                        "evo: the Evo-ViT baseline (slow-fast token update: no token is removed, from block --evo-start on a block runs on the "
                        "--evo-keep share of the tokens with the highest global score plus one representative of the rest; no predictor); "
                        "ltp: the LTP baseline (learned token thresholds: the blocks at --pruning-locs each own one learnable threshold on the "
                        "attention a token receives; --ltp-phase soft trains the thresholds on the dense batch through a sigmoid mask, hard "
                        "prunes on the ragged packed batch with the thresholds fixed; evaluation is always hard; no predictor)")
    p.add_argument('--ltp-phase', choices=['soft', 'hard'], default=None,
                   help='with --method ltp: what training runs (default soft); go from soft to hard with --student-checkpoint, which loads the '
                        'weights including the thresholds')
    p.add_argument('--ltp-temperature', type=float, default=None, metavar='TAU',
                   help='with --method ltp: the soft mask is sigmoid((score - threshold) / TAU) (default 1e-3)')
    p.add_argument('--ltp-lambda', type=float, default=None, metavar='W',
                   help='with --method ltp: weight of the regulariser, the mean of every soft mask entry (default 0.01)')
    p.add_argument('--ltp-init-threshold', type=float, default=None, metavar='TH',
                   help='with --method ltp: stage k of S starts at TH * (k + 1) / S (default 0.005, about 1 / tokens at 224 x 224)')
    p.add_argument('--evo-start', type=int, default=None, metavar='S',
                   help='with --method evo: the first slow-fast block, 1..depth; the blocks before it are dense (default 4)')
    p.add_argument('--evo-keep', type=float, default=None, metavar='R',
                   help='with --method evo: a slow-fast block runs on k = int(patches * R) tokens (default 0.5)')
    p.add_argument('--evo-tradeoff', type=float, default=None, metavar='TAU',
                   help="with --method evo: a kept token's global score becomes (1 - TAU) * score + TAU * the block's CLS attention (default 0.5)")
    p.add_argument('--avit-gate-scale', type=float, default=None, metavar='G',
                   help='with --method avit: the halting score is sigmoid(G * channel 0 - C) (default 10)')
    p.add_argument('--avit-gate-center', type=float, default=None, metavar='C', help='with --method avit: see --avit-gate-scale (default 30)')
    p.add_argument('--avit-ponder-scale', type=float, default=None, metavar='W',
                   help='with --method avit: weight of the ponder term, the mean over all tokens of halting layer + remainder (default 5e-4)')
    p.add_argument('--avit-prior-alpha', type=float, default=None, metavar='A',
                   help='with --method avit: weight of the distribution prior, KL(target || mean halting score per layer) (default 0.01)')
    p.add_argument('--avit-target-depth', type=float, default=None, metavar='T',
                   help='with --method avit: centre of the Gaussian target of the distribution prior, in layers (default 7)')
    p.add_argument('--ats-tokens', nargs='+', type=int, default=None, metavar='K',
                   help='with --method ats: the most tokens an image keeps at a stage, one value for every stage or one per --pruning-locs '
                        'entry (default: the number of patches); how many of them an image keeps falls out of its own attention')
    p.add_argument('--ats-train', action='store_true', default=False,
                   help='with --method ats: train through the sampling stages on the ragged packed batch (varlen attention backward, re-pack '
                        'backward; the selection itself carries no gradient); the objective is --cls-weight * CE + --dist-weight * KL to the '
                        'dense teacher (--dist-weight 0: no teacher); --gemm-mode exact or split')
    p.add_argument('--tome-train', action='store_true', default=False,
                   help='with --method tome: train through the merges (merge backward, key-weighted attention backward); the objective is '
                        '--cls-weight * CE + --dist-weight * KL to the dense teacher (--dist-weight 0: no teacher)')
    p.add_argument('--tome-bf16', action='store_true', default=False,
                   help='with --method tome --eval-only: run the merging trunk on the bf16 data path (bf16 matrix cores for the GEMMs and the '
                        'key-weighted attention, the match on the bf16 qkv); --gemm-mode stays at exact or split')
    # no attribute unless given (argparse.SUPPRESS): every reader asks getattr(args, "tome_train_bf16", False)
    p.add_argument('--tome-train-bf16', action='store_true', default=argparse.SUPPRESS,
                   help='with --method tome --tome-train: train through the merges in the bf16 arithmetic mode (bf16 matrix cores for the '
                        'GEMMs, the key-weighted attention and its backward; the bf16 data path) - the flag sets that mode itself, '
                        '--gemm-mode stays at exact (its default); validation runs the bf16 merging trunk')
    p.add_argument('--ats-train-bf16', action='store_true', default=argparse.SUPPRESS,
                   help='with --method ats --ats-train: train through the sampling stages in the bf16 arithmetic mode (bf16 matrix cores for '
                        'the GEMMs, the ragged attention and its backward; the bf16 data path) - the flag sets that mode itself, --gemm-mode '
                        'stays at exact (its default)')
    p.add_argument('--avit-bf16', action='store_true', default=argparse.SUPPRESS,
                   help='with --method avit: train in the bf16 arithmetic mode (bf16 matrix cores for the GEMMs, the ragged attention and its '
                        'backward; the bf16 data path, every block boundary handing on the bf16 form of its gradient) - the flag sets that '
                        'mode itself, --gemm-mode stays at exact (its default); with --eval-only use --gemm-mode bf16')
    p.add_argument('--ltp-bf16', action='store_true', default=argparse.SUPPRESS,
                   help='with --method ltp: run both phases and the evaluation in the bf16 arithmetic mode (bf16 matrix cores for the GEMMs, '
                        'the ragged and the policy attention, their backwards and the score; the bf16 data path) - the flag sets that mode '
                        'itself, --gemm-mode stays at exact (its default)')
    p.add_argument('--graph-rank', type=int, default=argparse.SUPPRESS, metavar='T',
                   help='with --topk-selection --attn-selection: rank the tokens of every stage by T iterations of PageRank over the whole '
                        'attention graph of the block before it (s <- s P from s = 1/n per head; the importance stage of Zero-TPrune) instead '
                        'of by that block\'s CLS row; T = 1 is the mean attention a token receives; --gemm-mode exact or split')
    p.add_argument('--sim-prune', type=int, default=argparse.SUPPRESS, metavar='R',
                   help='with --topk-selection --attn-selection: every stage ranks R candidates more than it keeps, matches the less '
                        'important half of them against the more important half by the cosine of the previous block\'s keys and prunes the '
                        'R with the closest partner (the similarity stage of Zero-TPrune), so the kept tokens are not near-duplicates; '
                        'combines with --graph-rank; --gemm-mode exact or split')
    p.add_argument('--tome-r', type=int, default=0, metavar='R',
                   help='with --method tome: tokens merged away in every block (each block clips it to half of its non-CLS tokens)')
    p.add_argument('--diff-topk', action='store_true', default=False,
                   help='with --topk-selection: train through the perturbed top-k soft gather (sigma decays from --initial-sigma to 0 over '
                        'the epochs); evaluation and the trained model keep the hard top-k')
    p.add_argument('--topk-samples', type=int, default=500, metavar='N', help="noise samples of --diff-topk (the reference's PerturbedTopK default)")
    p.add_argument('--fuse-dropped', action='store_true', default=False,
                   help='with --topk-selection: every pruning stage fuses the tokens it drops, weighted by their keep probabilities, into one '
                        'package token that later stages carry along (training and evaluation alike; no new parameters)')
    p.add_argument('--squeeze-dropped', action='store_true', default=False,
                   help='with --topk-selection: every pruning stage folds each token it drops into the kept token it resembles most '
                        '(cosine), weighted by exp(cosine); the stage still keeps k tokens (training and evaluation alike; no new '
                        'parameters)')
    p.add_argument('--ragged-cascade', action='store_true', default=False,
                   help='with --patch-score-threshold and several --pruning-locs: at inference every threshold stage after the first scores '
                        'and selects, per image, among the tokens that survived, and packs the batch again (this build\'s definition: the '
                        'reference\'s second stage cannot run)')
    p.add_argument('--ragged-train', action='store_true', default=False,
                   help='with --patch-score-threshold: train on the ragged packed batch - the training forward runs the inference cascade, '
                        'differentiable (the survivors of every stage are packed and the later blocks run on them alone; the selection '
                        'carries no gradient), and a packed stage adds its own mask-loss term; several --pruning-locs still need '
                        '--ragged-cascade; --gemm-mode exact or split (this build\'s definition)')
    p.add_argument('--ragged-bf16', action='store_true', default=False,
                   help='with --ragged-train: train on the ragged packed batch in the bf16 arithmetic mode (bf16 matrix cores for the GEMMs, '
                        'the ragged attention and its backward; the bf16 data path) - the flag sets that mode itself, --gemm-mode stays at '
                        'exact (its default); --gemm-mode bf16 without this path stays refused')
    p.add_argument('--accum-steps', type=int, default=1, metavar='N',
                   help='one optimiser step per N batches (gradient = mean over the N; effective batch = N x --batch-size x ranks), '
                        'accumulated inside the fused arena step')
    p.add_argument('--clip-grad', type=float, default=None, metavar='NORM',
                   help="clip the gradient to this global L2 norm before the update (DeiT's flag; default: no clipping); the norm never "
                        "leaves the device, its epoch mean is reported as train_grad_norm")
    args = p.parse_args(argv)
    # --ats-train refuses a predictor warm-up that was asked for and takes the reference's default as "none"
    args.warmup_steps_given = not isinstance(args.warmup_steps, _Unset)
    args.warmup_steps = int(args.warmup_steps)
    return args


def atomic_save(obj, path, writer=torch.save):
    """writer(obj, file) into a temporary name in the directory of `path`, flushed to disk, then os.replace: whoever reads `path`
    finds the previous complete file or the new complete file, never a part of one - also when the job is killed mid-write."""
    import os
    tmp = os.path.join(os.path.dirname(os.path.abspath(path)), f".{os.path.basename(path)}.{os.getpid()}.tmp")
    try:
        with open(tmp, "wb") as f:
            writer(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def keep_ratio_summary(keep_ratio_batches):
    """min / avg / max of the per-image keep ratios collected over an epoch (train.py:67-70,77-80; evaluate.py:53-62).  The loaders use
    drop_last=False (ddp_training.py:15-20), so the last batch may be shorter than the others: the batches are concatenated, never
    stacked.  avg follows the reference: the mean of the per-batch means (sum(avg_keep_ratio) / len(loader)), min / max over all images."""
    import torch
    allr = torch.cat([r.reshape(-1) for r in keep_ratio_batches])
    avg = torch.stack([r.float().mean() for r in keep_ratio_batches]).mean()
    return float(allr.min()), float(avg), float(allr.max())
