"""Counterpart of the reference's losses.py: same classes, constructor arguments, forward signatures and metrics keys
(including the swapped train_token_kl_loss / train_cls_kl_loss keys of losses.py:238-239), computed by HIP kernels.

Differences that are deliberate and documented:
  * running statistics stay on the device (no .item() per step, losses.py:111,230-233 force a D2H sync every step);
    metrics values are 0-d tensors, `float(v)` reads them.
  * the kl_div and mse mask losses, hard-label and soft-target (mixup) cross entropy are on the accelerated path; the reference's bce
    branch is broken as written (undefined `args` / `self.mask_criterions`, losses.py:57-58).
  * dynamic keep ratio (args.patch_score_threshold set): the reference's losses cannot run on that path (MaskLoss iterates over the
    batch dimension of the mask tensor it is handed, losses.py:81; BackboneLoss indexes with a float row and an undefined `C`,
    :216-218).  The fix built here keeps their intent: no token is removed in training, so every stage's KL runs over all N tokens
    against the un-gathered teacher target and its accuracy compares the two THRESHOLD masks (student scores vs teacher target under
    the same cumulative rule); the token distillation term is the mean over the tokens the last stage's mask keeps.
  * dynamic keep ratio at validation with more than one stage (the ragged cascade): a stage after the first scores
    only the tokens that survived, so its pred_logits is the packed [total] vector.  mask_acc_i is computed for every stage, from the
    dense cumulative [B, N] masks against the teacher's threshold mask as above; the KL / MSE term is computed for a stage only when its
    pred_logits is the dense [B, N] tensor.  A packed stage contributes NO loss term: neither the reference nor the training-mode fix
    defines one (val_mask_loss of such a student is the first stage's term).
  * training the dynamic keep ratio on the ragged batch (args.ragged_train; the build's own definition): a packed
    stage s >= 1 DOES carry a term, in training and at validation alike.  For image b over its rows of the batch the stage scored, with
    original patch ids j_r = row_src[r] - 1: q_r = target[b, j_r] / sum_r target[b, j_r] - the gather_renorm(normalize=True) recursion
    of the fixed-ratio path - and the term is (1 / B) sum_b KL(q_b || softmax(pred_logits_b)) for kl_div, 100 * sum (pred_logit_r -
    q_r)^2 / (total_{s-1} - B) for mse; an image without a surviving token contributes 0.  The token distillation is the mean over the
    non-CLS rows of the last packed batch of KL(softmax(token_t[b, j_r]) || softmax(token_s[r])).  Without the flag nothing changes.
"""
import torch

from d2s import functional as DF
from d2s import ops


class MaskLoss(torch.nn.Module):
    def __init__(self, args, phase):
        super().__init__()
        self.phase = phase
        self.keep_ratios = args.keep_ratios
        self.loss_type = args.mask_loss_type
        if self.loss_type not in ("kl_div", "mse"):
            raise NotImplementedError("mask_loss_type 'kl_div' (losses.py:75-96) and 'mse' (:61-73) are on the accelerated path; the "
                                      "reference's 'bce' branch is broken as written (:57-58)")
        self.patch_score_threshold = getattr(args, "patch_score_threshold", None)
        self.ragged_train = bool(getattr(args, "ragged_train", False))
        self.count = 1
        self.running_loss = 0
        self.runnings_accs = [0 for _ in self.keep_ratios]

    def _packed_stage_term(self, scores, target, cu, row_src):
        """args.ragged_train: the term of a stage that scored the packed batch (cu, row_src), see the module docstring"""
        from d2s.functional_ragged import RaggedMaskLossFn
        B = target.shape[0]
        if self.loss_type == "mse":
            rows = scores.numel() - B
            return RaggedMaskLossFn.apply(scores, target, cu, row_src, ops.MSE_TARGET, 100.0 / rows if rows > 0 else 0.0)
        return RaggedMaskLossFn.apply(scores, target, cu, row_src, ops.KL_PROB_TARGET, 1.0 / B)

    def _forward_threshold(self, pred_logits, target, keep_masks, mask_accs, ragged=None):
        """Dynamic keep ratio: every stage scores all N tokens (nothing was gathered), see the module docstring.
        ragged (args.ragged_train only): ([cu_seqlens per stage], [row_src per stage]) of the forward that produced pred_logits."""
        B, T = target.shape
        packed_terms = self.ragged_train and ragged is not None
        mask_loss = 0
        with torch.no_grad():
            gt_mask, _ = ops.select_threshold(target, float(self.patch_score_threshold))
        for i in range(len(keep_masks)):
            dense = pred_logits[i].dim() == 2       # a packed stage of the ragged cascade hands over [total] scores: no loss term is defined
            if not dense and packed_terms:          # stage i scored the batch stage i - 1 packed
                mask_loss = mask_loss + self._packed_stage_term(pred_logits[i], target, ragged[0][i - 1], ragged[1][i - 1])
            if self.loss_type == "mse":
                if dense:
                    mask_loss = mask_loss + DF.RowLossFn.apply(pred_logits[i], ops.MSE_TARGET, target, None, None, B * T / 100.0)
                continue
            with torch.no_grad():
                mask_accs[i] = ops.sum_scalar(ops.dense_mask_agreement(keep_masks[i].contiguous(), gt_mask), 1.0 / float(B * T))
            if dense:
                mask_loss = mask_loss + DF.RowLossFn.apply(pred_logits[i], ops.KL_PROB_TARGET, target, None, None, B)
        return mask_loss

    def forward(self, pred_logits, cls_attn_weights, kept_token_idx, metrics, accumulate=True, attn_selection=False, ragged=None):
        """accumulate=False: only the loss of this batch is computed (its running mean / accuracies are NOT advanced); the caller hands
        `self.last` to accumulate() later - the split a captured (hipGraph) step needs: the kernels replay, the host-side running
        statistics of losses.py:105-119 are advanced once per replay (d2s.engine.TrainStep).
        attn_selection: the student selected by its own CLS attention - there is no predictor output to distil, so the
        KL / MSE term is exactly 0 without a gradient, and mask_acc_i is the agreement of the stage's kept ids with the teacher target's
        top-k (same recursion, same kernels; only where the student's ids come from differs)."""
        target = ops.teacher_target(cls_attn_weights.contiguous())             # losses.py:76-79
        B = target.shape[0]
        mask_loss = torch.zeros((), dtype=torch.float32, device=target.device) if attn_selection else 0
        mask_accs = [0 for _ in self.keep_ratios]
        if self.patch_score_threshold is not None:
            mask_loss = self._forward_threshold(pred_logits, target, kept_token_idx, mask_accs, ragged)
            kept_token_idx = []
        for i in range(len(kept_token_idx)):
            if i > 0:
                ratio = self.keep_ratios[i] / self.keep_ratios[i - 1]
                gt_vals = ops.gather_renorm(target, kept_token_idx[i - 1], normalize=False)   # :84-85
                target = ops.gather_renorm(target, kept_token_idx[i - 1], normalize=True)     # :89-90
            else:
                ratio = self.keep_ratios[i]
                gt_vals = target
            T = gt_vals.shape[1]
            nk = int(T * ratio)                                                               # :132,154
            if attn_selection:
                with torch.no_grad():
                    gt_ids, _ = ops.select_topk(gt_vals, nk)
                    pm_ids = kept_token_idx[i].contiguous()
                    if pm_ids.shape[1] != nk:      # init_n is not this model's token count (micro geometries): the same rule at the target's count
                        pm_ids, _ = ops.select_topk(pred_logits[i].detach().contiguous(), nk)
                    mask_accs[i] = ops.sum_scalar(ops.mask_agreement(pm_ids, gt_ids, T), 1.0 / float(B * T))
                continue
            if self.loss_type == "mse":      # :61-73: 100 * mean squared difference between the raw scores and the target; no accuracy
                mask_loss = mask_loss + DF.RowLossFn.apply(pred_logits[i], ops.MSE_TARGET, target, None, None, B * T / 100.0)
                continue
            with torch.no_grad():
                gt_ids, _ = ops.select_topk(gt_vals, nk)
                pm_ids, _ = ops.select_topk(ops.softmax_rows(pred_logits[i].detach().contiguous()), nk)
                agree = ops.mask_agreement(pm_ids, gt_ids, T)
                mask_accs[i] = ops.sum_scalar(agree, 1.0 / float(B * T))             # :96
            mask_loss = mask_loss + DF.RowLossFn.apply(pred_logits[i], ops.KL_PROB_TARGET, target, None, None, B)   # :94-95
        self.last = (mask_loss.detach(), mask_accs)
        if accumulate:
            self.accumulate(metrics, self.last)
        return mask_loss

    def accumulate(self, metrics, last):
        """Advance the running mean of the loss and of the per-stage mask accuracies by one batch (losses.py:105-119)."""
        mask_loss, mask_accs = last
        self.running_loss = self.running_loss + mask_loss
        metrics[f"{self.phase}_mask_loss"] = self.running_loss / self.count
        for i, _ in enumerate(self.keep_ratios):
            self.runnings_accs[i] = self.runnings_accs[i] + mask_accs[i]
            metrics[f"{self.phase}_mask_acc_{i}"] = self.runnings_accs[i] / self.count
        self.count += 1


class BackboneLoss(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.soft_targets = getattr(args, "mixup", 0.) > 0.      # losses.py:170-174: SoftTargetCrossEntropy under mixup, else hard labels
        self.patch_score_threshold = getattr(args, "patch_score_threshold", None)
        self.ragged_train = bool(getattr(args, "ragged_train", False))
        self.count = 1
        self.running_loss = 0
        self.running_cls_loss = 0
        self.running_token_kl_loss = 0
        self.running_token_dist_loss = 0
        self.runnings_acc = 0

    def forward(self, logits_s, token_s, logits_t, token_t, kept_token_idx, train_labels, metrics, accumulate=True, ragged=None):
        """accumulate: see MaskLoss.forward.  ragged (args.ragged_train only): (cu_seqlens, row_src) of the last packed batch, token_s then
        being its normed rows [total, D], CLS rows included."""
        B = logits_s.shape[0]
        if self.soft_targets:      # train_labels are [B, classes] probabilities produced by the caller's mixup_fn (train.py:29-30)
            cls_loss = DF.RowLossFn.apply(logits_s, ops.SOFT_CE, train_labels.float().contiguous(), None, None, B)
        else:
            cls_loss = DF.RowLossFn.apply(logits_s, ops.CE_LABEL, None, None, train_labels.contiguous(), B)      # :196
        cls_kl_loss = DF.RowLossFn.apply(logits_s, ops.KL_LOGIT_TARGET, logits_t.detach(), None, None, B)       # :198-203
        rows = token_s.shape[0] * token_s.shape[1]
        if self.ragged_train and ragged is not None and token_s.dim() == 2:
            # every packed row against the teacher's token at its original position, mean over the non-CLS rows (weights 1 / (total - B),
            # 0 at the CLS rows); for one stage: the mean over the rows the last mask keeps, as in the branch below
            t_rows, w = ops.ragged_teacher_rows(token_t.detach(), ragged[0], ragged[1])
            token_kl_loss = DF.RowLossFn.apply(token_s, ops.KL_LOGIT_TARGET, t_rows, None, None, 1.0, w)
        elif self.patch_score_threshold is not None:
            # the intent of losses.py:216-225: distil only the tokens the last stage keeps; student and teacher both still hold all N
            # tokens, so the pairing is positional and 'batchmean' becomes the mean over the kept rows (weights = mask / count)
            w = ops.mask_row_weights(kept_token_idx[-1].detach().contiguous())
            token_kl_loss = DF.RowLossFn.apply(token_s, ops.KL_LOGIT_TARGET, token_t.detach(), None, None, 1.0, w)
        else:
            # teacher tokens gathered with the LAST stage's stage-relative ids, exactly like losses.py:212
            token_kl_loss = DF.RowLossFn.apply(token_s, ops.KL_LOGIT_TARGET, token_t.detach(), kept_token_idx[-1], None, rows)   # :218-225
        backbone_loss = cls_loss + cls_kl_loss + token_kl_loss
        self.last = (backbone_loss.detach(), cls_loss.detach(), cls_kl_loss.detach(), token_kl_loss.detach())
        self.last_terms = self.last[1:]
        if accumulate:
            self.accumulate(metrics, self.last)
        return backbone_loss

    def accumulate(self, metrics, last):
        """Advance the running means by one batch (losses.py:228-241)."""
        backbone_loss, cls_loss, cls_kl_loss, token_kl_loss = last
        self.running_loss = self.running_loss + backbone_loss
        self.running_cls_loss = self.running_cls_loss + cls_loss
        self.running_token_dist_loss = self.running_token_dist_loss + cls_kl_loss
        self.running_token_kl_loss = self.running_token_kl_loss + token_kl_loss
        metrics["train_backbone_loss"] = self.running_loss / self.count
        metrics["train_cls_loss"] = self.running_cls_loss / self.count
        metrics["train_token_kl_loss"] = self.running_token_dist_loss / self.count      # sic: swapped in the reference
        metrics["train_cls_kl_loss"] = self.running_token_kl_loss / self.count          # (losses.py:238-239)
        self.count += 1


class DynamicViTLoss(torch.nn.Module):
    """The objective of the DynamicViT baseline (vit_models/default_dynamic_vit.py).  The reference ships no loss for this model - its
    --ratio-weight / --dist-weight / --cls-weight flags are read nowhere (mask_predictor.py:150-151) - so this is the DynamicViT paper's
    objective, and its parity with the reference is unpinned:

        L = cls_weight * CE(logits, y)                                   (soft-target CE under mixup, as BackboneLoss)
          + ratio_weight / S * sum_s mean_b (mean_j d_s[b, j] - rho_s)^2
          + dist_weight * KL(log_softmax(logits_s) || log_softmax(logits_t), batchmean, log_target)
          + dist_weight * sum(mask * mean_c (f_s - f_t)^2) / sum(mask)   (mask = the final decision, detached)

    Everything stays on the device: the running means are 0-d tensors, `float(v)` reads them."""

    def __init__(self, args):
        super().__init__()
        self.soft_targets = getattr(args, "mixup", 0.) > 0.
        self.keep_ratios = [float(r) for r in args.keep_ratios]
        self.cls_weight = float(getattr(args, "cls_weight", 1.0))
        self.ratio_weight = float(getattr(args, "ratio_weight", 2.0))
        self.dist_weight = float(getattr(args, "dist_weight", 0.5))
        self.count = 1
        self.running = [0, 0, 0, 0, 0]

    def forward(self, logits_s, token_s, mask, out_pred_prob, logits_t, token_t, train_labels, metrics, accumulate=True):
        """logits_s [B, classes], token_s / token_t [B, N, D], mask [B, N] (the final decision), out_pred_prob: one [B, N] decision per stage."""
        from d2s.functional_dynamicvit import RatioLossFn
        B = logits_s.shape[0]
        S = len(out_pred_prob)
        if S != len(self.keep_ratios):
            raise ValueError(f"{S} pruning stages, {len(self.keep_ratios)} keep ratios")
        if self.soft_targets:
            cls_loss = DF.RowLossFn.apply(logits_s, ops.SOFT_CE, train_labels.float().contiguous(), None, None, B)
        else:
            cls_loss = DF.RowLossFn.apply(logits_s, ops.CE_LABEL, None, None, train_labels.contiguous(), B)
        ratio_loss = 0
        for d, rho in zip(out_pred_prob, self.keep_ratios):
            ratio_loss = ratio_loss + RatioLossFn.apply(d, rho, B * S)
        cls_kl_loss = DF.RowLossFn.apply(logits_s, ops.KL_LOGIT_TARGET, logits_t.detach(), None, None, B)
        # w = mask / sum(mask): the weighted sum of the rows' squared differences, over D, is the mean over the kept tokens
        w = ops.mask_row_weights(mask.detach().contiguous())
        token_loss = DF.RowLossFn.apply(token_s, ops.MSE_TARGET, token_t.detach(), None, None, token_s.shape[-1], w)
        loss = self.cls_weight * cls_loss + self.ratio_weight * ratio_loss + self.dist_weight * cls_kl_loss + self.dist_weight * token_loss
        self.last = (loss.detach(), cls_loss.detach(), ratio_loss.detach(), cls_kl_loss.detach(), token_loss.detach())
        self.last_terms = self.last[1:]
        if accumulate:
            self.accumulate(metrics, self.last)
        return loss

    def accumulate(self, metrics, last):
        """Advance the running means by one batch."""
        self.running = [r + v for r, v in zip(self.running, last)]
        for key, r in zip(("train_dynamicvit_loss", "train_cls_loss", "train_ratio_loss", "train_cls_kl_loss", "train_token_mse_loss"), self.running):
            metrics[key] = r / self.count
        self.count += 1


class ToMeLoss(torch.nn.Module):
    """The objective of a Token Merging student that trains through its merges (the reference has no ToMe):

        L = cls_weight * CE(logits, y)                                   (soft-target CE under mixup, as BackboneLoss)
          + dist_weight * KL(log_softmax(logits_s) || log_softmax(logits_t), batchmean, log_target)

    The second term only with a teacher and dist_weight != 0.  The running means are 0-d device tensors, `float(v)` reads them."""

    def __init__(self, args):
        super().__init__()
        self.soft_targets = getattr(args, "mixup", 0.) > 0.
        self.cls_weight = float(getattr(args, "cls_weight", 1.0))
        self.dist_weight = float(getattr(args, "dist_weight", 0.5))
        self.count = 1
        self.running = [0, 0, 0]

    def forward(self, logits_s, logits_t, train_labels, metrics, accumulate=True):
        """logits_s [B, classes]; logits_t the teacher's, or None"""
        B = logits_s.shape[0]
        if self.soft_targets:
            cls_loss = DF.RowLossFn.apply(logits_s, ops.SOFT_CE, train_labels.float().contiguous(), None, None, B)
        else:
            cls_loss = DF.RowLossFn.apply(logits_s, ops.CE_LABEL, None, None, train_labels.contiguous(), B)
        loss = self.cls_weight * cls_loss
        if logits_t is not None and self.dist_weight != 0.0:
            cls_kl_loss = DF.RowLossFn.apply(logits_s, ops.KL_LOGIT_TARGET, logits_t.detach(), None, None, B)
            loss = loss + self.dist_weight * cls_kl_loss
            kl = cls_kl_loss.detach()
        else:
            kl = torch.zeros((), dtype=torch.float32, device=logits_s.device)
        self.last = (loss.detach(), cls_loss.detach(), kl)
        self.last_terms = self.last[1:]
        if accumulate:
            self.accumulate(metrics, self.last)
        return loss

    def accumulate(self, metrics, last):
        """Advance the running means by one batch."""
        self.running = [r + v for r, v in zip(self.running, last)]
        for key, r in zip(("train_tome_loss", "train_cls_loss", "train_cls_kl_loss"), self.running):
            metrics[key] = r / self.count
        self.count += 1


class AViTLoss(ToMeLoss):
    """The objective of the A-ViT baseline (the reference has no A-ViT): ToMeLoss's two terms plus the two penalty
    terms the model's forward leaves behind (VisionTransformerAViT.ponder_loss / prior_loss, computed by d2s_avit_penalty_fwd):

        L = cls_weight * CE + dist_weight * KL(student || teacher) + ponder_scale * mean_{b,t}(n + R) + prior_alpha * P

    The running means are 0-d device tensors, `float(v)` reads them."""

    def __init__(self, args):
        super().__init__(args)
        self.ponder_scale = float(getattr(args, "avit_ponder_scale", 5e-4))
        self.prior_alpha = float(getattr(args, "avit_prior_alpha", 0.01))
        self.running_avit = [0, 0, 0]

    def forward(self, logits_s, logits_t, train_labels, metrics, ponder, prior, avg_depth, accumulate=True):
        """ponder, prior: the model's two penalty terms (0-d, differentiable); avg_depth: its mean halting layer (0-d)"""
        loss = super().forward(logits_s, logits_t, train_labels, metrics, accumulate=False)
        loss = loss + self.ponder_scale * ponder + self.prior_alpha * prior
        self.last = (loss.detach(),) + tuple(self.last[1:])
        self.last_avit = (ponder.detach(), prior.detach(), avg_depth.detach())
        if accumulate:
            self.accumulate(metrics, self.last, self.last_avit)
        return loss

    def accumulate(self, metrics, last, last_avit):
        """Advance the running means by one batch."""
        self.running = [r + v for r, v in zip(self.running, last)]
        self.running_avit = [r + v for r, v in zip(self.running_avit, last_avit)]
        for key, r in zip(("train_avit_loss", "train_cls_loss", "train_cls_kl_loss"), self.running):
            metrics[key] = r / self.count
        for key, r in zip(("train_ponder_loss", "train_prior_loss", "train_avg_depth"), self.running_avit):
            metrics[key] = r / self.count
        self.count += 1


class LTPLoss(ToMeLoss):
    """The objective of the LTP baseline (the reference has no LTP): ToMeLoss's two terms plus the regulariser the
    model's forward leaves behind (VisionTransformerLTP.ltp_reg: the mean of every soft mask entry over stages, images and patches):

        L = cls_weight * CE + dist_weight * KL(student || teacher) + ltp_lambda * R

    In the hard phase R is a constant (the kept fraction) and only reported.  The running means are 0-d device tensors."""

    def __init__(self, args):
        super().__init__(args)
        lam = getattr(args, "ltp_lambda", None)
        self.ltp_lambda = 0.01 if lam is None else float(lam)
        self.running_ltp = [0, 0]

    def forward(self, logits_s, logits_t, train_labels, metrics, reg, avg_tokens, accumulate=True):
        """reg: the model's regulariser (0-d; differentiable in the soft phase); avg_tokens: its mean token count per image and block"""
        loss = super().forward(logits_s, logits_t, train_labels, metrics, accumulate=False)
        if reg.requires_grad:
            loss = loss + self.ltp_lambda * reg
        self.last = (loss.detach(),) + tuple(self.last[1:])
        self.last_ltp = (reg.detach(), torch.as_tensor(float(avg_tokens), dtype=torch.float32, device=logits_s.device))
        if accumulate:
            self.accumulate(metrics, self.last, self.last_ltp)
        return loss

    def accumulate(self, metrics, last, last_ltp):
        """Advance the running means by one batch."""
        self.running = [r + v for r, v in zip(self.running, last)]
        self.running_ltp = [r + v for r, v in zip(self.running_ltp, last_ltp)]
        for key, r in zip(("train_ltp_loss", "train_cls_loss", "train_cls_kl_loss"), self.running):
            metrics[key] = r / self.count
        for key, r in zip(("train_ltp_reg", "train_avg_tokens"), self.running_ltp):
            metrics[key] = r / self.count
        self.count += 1
