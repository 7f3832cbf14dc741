"""GPU tier of training the dynamic keep ratio on the ragged packed batch (ragged_train=True / --ragged-train): the
entries of csrc/ragged_threshold.hip on their own against float64, the Functions that move rows, the training-mode student against the
float64 restatement (tests/ragged_train_ref.py) with the GPU's own masks replayed, and TrainStep.

PARITY UNPINNED: the definition is the build's own.  The selection is discrete, so the float64 reference replays the masks the GPU chose;
separately the masks are asserted equal to the fp32 restatement's on cases whose smallest |running sum - threshold| is far above 2e-5
(tests/test_ragged_train_cpu.py records the gaps: 2.0e-3 at the least).

Tolerances.  Row moves, ids, masks, offsets: bit-exact.  The varlen split / mean / concat backward: the project's summation bound
(losspath_ref.sum_bound) over the segment - wave partial sums of ceil(n / 4) terms, two combine levels, one division.  The mask loss:
those of tests/test_loss_kernels_gpu.py (4 x the fp32 restatement, 3e-7, or kl_rows_error_bound - the kernel forms the same s - (max + log
sum)) plus 12 u for the renormalised target q, which the kernel forms in fp32 (a sum of depth 8 and a division) and the float64 reference
in float64: its relative error enters every loss term and gradient linearly.  The model: tests/test_ats_train_gpu.py's (logits rtol 1e-4 /
atol 2e-5; gradient norms rtol 1e-3 / atol 1e-6; leading elements rtol 5e-3, atol 5e-4 max|ref| + 2e-6; first-step loss rtol 1e-4)."""
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import losspath_ref as L
from tests import ragged_train_ref as R
from oracle import d2s_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)
U = L.F32_EPS
ROWS = (1, 2, 5, 130, 17)                      # rows per segment, CLS included: a CLS-only image, one token, fewer rows than waves, many, some


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cu(rows):
    return torch.tensor(np.concatenate([[0], np.cumsum(rows)]).astype(np.int32))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("C", [6, 64, 192, 384])
def test_half_mean_concat_varlen_bwd(C):
    """C = 6: the scalar form; 64, 192, 384: the 16-byte form, one and two column chunks per half"""
    from d2s import lib, ops
    B, half = len(ROWS), C // 2
    cu = _cu(ROWS)
    total = int(cu[-1])
    g = torch.randn((total, C), generator=torch.Generator().manual_seed(C))
    gd, cud = g.to(DEV), cu.to(DEV)
    out = _nan(total, C)
    lib.call("d2s_half_mean_concat_varlen_bwd", gd.data_ptr(), cud.data_ptr(), out.data_ptr(), B, C)
    again = ops.half_mean_concat_varlen_bwd(gd, cud, B)
    torch.cuda.synchronize()
    assert torch.equal(out, again), "two launches, the first into NaN: every element written, nothing read back"
    out = out.cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :half], g[:, :half]), "the first half is a copy"
    for b, n in enumerate(ROWS):
        r0, T = int(cu[b]), n - 1
        got = out[r0:r0 + n, half:].double()
        assert bool((got[0] == 0).all()), "the CLS row is no part of the mean"
        if T == 0:
            continue
        assert bool((got[1:] == got[1:2]).all()), "every non-CLS row takes the same value"
        seg = g[r0:r0 + n, half:].double()
        bound = torch.tensor([L.sum_bound((n + 3) // 4 + 2, float(a), extra_roundings=1) for a in seg.abs().sum(dim=0)]) / T
        err = (got[1] - seg.sum(dim=0) / T).abs()
        print(f"half-mean varlen bwd C {C} n {n}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (C, n)
    # it is the adjoint of the forward: <bwd(g), x> = <g, fwd(x)>
    x = torch.randn((total, C), generator=torch.Generator().manual_seed(C + 1))
    fwd = ops.half_mean_concat_varlen(x.to(DEV), cud, B).cpu().double()
    lhs, rhs = float((out.double() * x.double()).sum()), float((g.double() * fwd).sum())
    assert lhs == pytest.approx(rhs, rel=1e-5, abs=1e-4)


@pytest.mark.parametrize("C", [6, 64])
def test_half_mean_concat_varlen_bwd_against_the_dense_backward(C):
    """Equal lengths.  The dense backward (d2s_half_mean_concat applied to the gradient) runs over the T non-CLS rows only and its wave w
    starts at token w; the varlen backward sums the CLS row's gradient too and its wave w starts at ROW w, so the partial sums hold
    different rows and the orders do NOT match: the second half of both agrees with float64 within the summation bound, not with each
    other bit for bit.  What does match is asserted bit for bit: the first half."""
    from d2s import ops
    B, T, half = 3, 21, C // 2
    n = T + 1
    g = torch.randn((B, n, C), generator=torch.Generator().manual_seed(7 + C))
    g[:, 0] = 0.0                                                              # the CLS rows' gradient: what the dense form never sees
    cu = _cu([n] * B).to(DEV)
    got = ops.half_mean_concat_varlen_bwd(g.view(B * n, C).to(DEV), cu, B).cpu().view(B, n, C)
    dense = ops.half_mean_concat(g[:, 1:].contiguous().view(B * T, C).to(DEV), B, T, C).cpu().view(B, T, C)
    assert torch.equal(got[:, 1:, :half], dense[:, :, :half])
    want = g[:, :, half:].double().sum(dim=1) / T
    bound = torch.tensor([[L.sum_bound((n + 3) // 4 + 2, float(a), 1) for a in row] for row in g[:, :, half:].abs().double().sum(dim=1)]) / T
    assert bool(((got[:, 1, half:].double() - want).abs() <= bound).all()) and bool(((dense[:, 0, half:].double() - want).abs() <= bound).all())


def _mask_loss_case(N, seed):
    """segments with T = 0, 1, N and two in between; a target with exact zeros; ascending row_src subsets"""
    g = torch.Generator().manual_seed(seed)
    Ts = [0, 1, N, max(1, N // 3), N - 1]
    B = len(Ts)
    target = torch.rand((B, N), generator=g)
    target[:, ::5] = 0.0                                                       # zeros in the target, some of them among the survivors
    target = (target / target.sum(dim=1, keepdim=True)).float()
    ids = [torch.sort(torch.randperm(N, generator=g)[:T])[0] for T in Ts]
    row_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), i + 1)) for i in ids]).int()
    cu = _cu([T + 1 for T in Ts])
    scores = (torch.randn(int(cu[-1]), generator=g) * 1.5 + 20.0).float()      # an offset: a kernel that forgets the maximum loses digits
    return Ts, target, ids, row_src, cu, scores


def _mask_loss_ref(scores, target, ids, cu, mode, dtype):
    """per image (loss [B], d loss / d scores [total]) in `dtype`; autograd"""
    s = scores.to(dtype).clone().requires_grad_(True)
    tg = target.to(dtype)
    losses = []
    for b, i in enumerate(ids):
        sb = s[int(cu[b]) + 1:int(cu[b + 1])]
        if i.numel() == 0:
            losses.append(torch.zeros((), dtype=dtype))
            continue
        gq = tg[b, i]
        q = gq / gq.sum() if float(gq.sum()) > 0 else torch.zeros_like(gq)
        if mode == L.MSE_TARGET:
            losses.append(((sb - q) ** 2).sum())
        else:
            losses.append((torch.xlogy(q, q) - q * torch.log_softmax(sb, dim=-1)).sum())
    loss = torch.stack(losses)
    (grad,) = torch.autograd.grad(loss.sum(), s)
    return loss.detach(), grad


@pytest.mark.parametrize("mode", [L.KL_PROB_TARGET, L.MSE_TARGET], ids=["kl_div", "mse"])
@pytest.mark.parametrize("N", [16, 33, 196])
def test_ragged_mask_loss(N, mode):
    from d2s import lib, ops
    Ts, target, ids, row_src, cu, scores = _mask_loss_case(N, 100 + N)
    B, total = len(Ts), int(cu[-1])
    sd, td, cud, rd = scores.to(DEV), target.to(DEV), cu.to(DEV), row_src.to(DEV)
    loss, grad = _nan(B), _nan(total)
    scale = 0.37
    lib.call("d2s_ragged_mask_loss_fwd", sd.data_ptr(), td.data_ptr(), cud.data_ptr(), rd.data_ptr(), loss.data_ptr(), B, total, N, mode)
    lib.call("d2s_ragged_mask_loss_bwd", sd.data_ptr(), td.data_ptr(), cud.data_ptr(), rd.data_ptr(), grad.data_ptr(), B, total, N, mode, scale)
    loss2, grad2 = ops.ragged_mask_loss_fwd(sd, td, cud, rd, mode), ops.ragged_mask_loss_bwd(sd, td, cud, rd, mode, scale)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), "two launches, the first into NaN: every element written"
    loss, grad = loss.cpu(), grad.cpu()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    assert bool((grad[cu[:-1].long()] == 0).all()), "exactly 0 at every CLS row"
    assert float(loss[0]) == 0.0, "an image without a surviving token contributes 0"
    ref_l, ref_g = _mask_loss_ref(scores, target, ids, cu, mode, torch.float64)
    cpu_l, cpu_g = _mask_loss_ref(scores, target, ids, cu, mode, torch.float32)
    bl = bg = 0.0
    if mode == L.KL_PROB_TARGET:
        # the derived bound of the row kernel, over the longest segment's row (the other rows are shorter sums of the same form)
        b = 2
        q = (target[b, ids[b]].double() / target[b, ids[b]].double().sum()).clamp_min(1e-300)[None]
        bl, bg = L.kl_rows_error_bound(mode, scores[int(cu[b]) + 1:int(cu[b + 1])].double()[None], q)
    if mode == L.KL_PROB_TARGET:
        assert float(loss[1]) == pytest.approx(0.0, abs=1e-6), "one row: softmax of one score is 1 and q is 1"
    L.assert_close_as_fp32(f"ragged mask loss mode {mode} N {N} loss", loss, ref_l, cpu_l, bl + 12 * U)
    L.assert_close_as_fp32(f"ragged mask loss mode {mode} N {N} grad", grad, scale * ref_g, scale * cpu_g, bg + 12 * U)


def test_ragged_teacher_rows_is_indexing_bit_for_bit():
    from d2s import lib, ops
    g = torch.Generator().manual_seed(5)
    B, N, D = 4, 33, 132
    Ts = [0, 1, N, 7]
    ids = [torch.sort(torch.randperm(N, generator=g)[:T])[0] for T in Ts]
    row_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), i + 1)) for i in ids]).int()
    cu = _cu([T + 1 for T in Ts])
    total = int(cu[-1])
    full = torch.randn((B, N + 1, D), generator=g)                            # the teacher's normed tokens, CLS included
    want = torch.zeros(total, D)
    want_w = torch.zeros(total)
    for b, i in enumerate(ids):
        want[int(cu[b]) + 1:int(cu[b + 1])] = full[b, 1:][i]
        want_w[int(cu[b]) + 1:int(cu[b + 1])] = float(np.float32(1.0) / np.float32(total - B))
    fd, cud, rd = full.to(DEV), cu.to(DEV), row_src.to(DEV)
    view = fd[:, 1:]                                                          # the token view HeadFn returns: image stride (N + 1) * D
    out, w = _nan(total, D), _nan(total)
    lib.call("d2s_ragged_teacher_rows", view.data_ptr(), view.stride(0), cud.data_ptr(), rd.data_ptr(), out.data_ptr(), w.data_ptr(), B, total, N, D)
    out2, w2 = ops.ragged_teacher_rows(view, cud, rd)
    out3, w3 = ops.ragged_teacher_rows(view.contiguous(), cud, rd)
    torch.cuda.synchronize()
    for o, ww in ((out, w), (out2, w2), (out3, w3)):
        assert torch.equal(o.cpu(), want) and torch.equal(ww.cpu(), want_w)
    # every image is CLS only: no row to distil, every weight 0 (not a division by zero)
    cls_only = torch.arange(B + 1, dtype=torch.int32, device=DEV)
    o, ww = ops.ragged_teacher_rows(view, cls_only, torch.zeros(B, dtype=torch.int32, device=DEV))
    assert bool((o == 0).all()) and bool((ww == 0).all())


def test_error_returns_before_any_launch():
    from d2s import lib
    B, N, D, total = 2, 16, 8, 9
    cu = _cu([4, 5]).to(DEV)
    x, out = torch.zeros(total, D, device=DEV), torch.zeros(total, D, device=DEV)
    v, w = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
    lr = torch.zeros(B, device=DEV)
    tg, tok = torch.full((B, N), 1.0 / N, device=DEV), torch.zeros(B, N, D, device=DEV)
    src = torch.zeros(total, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()
    s = lib.stream()
    hmc, fwd, bwd, rows = (lib._fn(n) for n in ("d2s_half_mean_concat_varlen_bwd", "d2s_ragged_mask_loss_fwd", "d2s_ragged_mask_loss_bwd",
                                                "d2s_ragged_teacher_rows"))
    good = (P(x), P(cu), P(out), B, D)
    assert hmc(*good, s) == 0
    for bad in [good[:i] + (None,) + good[i + 1:] for i in range(3)] + [good[:3] + (0, D), good[:3] + (B, 0), good[:3] + (B, 7)]:
        assert hmc(*bad, s) == ERR_ARG, bad
    good = (P(v), P(tg), P(cu), P(src), P(lr), B, total, N, 1)
    assert fwd(*good, s) == 0 and bwd(*good[:4], P(w), *good[5:], 1.0, s) == 0
    bads = [good[:i] + (None,) + good[i + 1:] for i in range(5)]
    bads += [good[:5] + (0, total, N, 1), good[:5] + (B, 0, N, 1), good[:5] + (B, total, 0, 1), good[:5] + (B, total, 8193, 1),
             good[:5] + (B, total, N, 0), good[:5] + (B, total, N, 2)]
    for bad in bads:
        assert fwd(*bad, s) == ERR_ARG, bad
        assert bwd(*bad, 1.0, s) == ERR_ARG, bad
    good = (P(tok), N * D, P(cu), P(src), P(out), P(w), B, total, N, D)
    assert rows(*good, s) == 0
    bads = [good[:i] + (None,) + good[i + 1:] for i in (0, 2, 3, 4, 5)]
    bads += [good[:6] + (0, total, N, D), good[:6] + (B, 0, N, D), good[:6] + (B, total, 0, D), good[:6] + (B, total, N, 0),
             good[:6] + (B, total, N, 6), (P(tok), N * D + 2) + good[2:], (P(tok), -4) + good[2:], (P(tok) + 4,) + good[1:]]
    for bad in bads:
        assert rows(*bad, s) == ERR_ARG, bad
    torch.cuda.synchronize()


# ---- 2. the Functions that move rows, the packed predictor ----
def test_pack_function_is_ragged_pack_bit_for_bit_and_its_backward_moves_rows():
    from d2s import ops
    from d2s.functional_ragged import RaggedPackFn, RaggedRepackFn
    g = torch.Generator().manual_seed(11)
    B, n, D = 4, 17, 128
    x = torch.randn((B, n, D), generator=g).to(DEV).requires_grad_(True)
    probs = torch.softmax(torch.randn((B, n - 1), generator=g), dim=-1).to(DEV)
    policy, counts = ops.select_threshold(probs, 0.4, lead=1)
    cu = ops.ragged_offsets(counts, extra=1)
    total = int(cu[-1])
    out, src = RaggedPackFn.apply(x, policy, cu, total)
    want, want_src = ops.ragged_pack(x.detach(), policy[:, 1:].contiguous(), cu, total)
    assert torch.equal(out.detach(), want) and torch.equal(src, want_src) and out.requires_grad and not src.requires_grad
    gy = torch.randn((total, D), generator=g).to(DEV)
    (gx,) = torch.autograd.grad(out, x, gy)
    flat = torch.nonzero(policy.view(-1) > 0).flatten()                       # the kept rows of [B * n], in order: the packed rows
    ref = torch.zeros(B * n, D, device=DEV)
    ref[flat] = gy
    assert torch.equal(gx.view(B * n, D), ref), "a kept row takes the row it became, a dropped row zeros"
    # the re-pack: keep every second surviving token
    keep = torch.ones(total, device=DEV)
    keep[1::2] = 0.0
    keep[cu[:-1].long()] = 1.0
    cnt = torch.stack([keep[int(cu[b]) + 1:int(cu[b + 1])].sum() for b in range(B)]).int()
    cu2 = ops.ragged_offsets(cnt, extra=1)
    xp = out.detach().clone().requires_grad_(True)
    out2, src2 = RaggedRepackFn.apply(xp, keep, cu, cu2, src, int(cu2[-1]), B)
    w2, ws2 = ops.ragged_repack(xp.detach(), keep, cu, cu2, src, int(cu2[-1]), B)
    assert torch.equal(out2.detach(), w2) and torch.equal(src2, ws2)
    gy2 = torch.randn(tuple(out2.shape), generator=g).to(DEV)
    (gxp,) = torch.autograd.grad(out2, xp, gy2)
    ref2 = torch.zeros(total, D, device=DEV)
    ref2[torch.nonzero(keep > 0).flatten()] = gy2
    assert torch.equal(gxp, ref2)


def _student(case, **kw):
    import vit_models
    cfg = case["cfg"]
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    args = dict(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True,
                predictor_loss_type=cfg["loss_type"], small_predictor=cfg["small_predictor"], patch_score_threshold=case["threshold"])
    args.update(kw)
    student = vit_models.VisionTransformerDiffPruning(**args, **common)
    sd_s, sd_t = cases.make_weights(case)
    student.load_state_dict({k: _t(v) for k, v in sd_s.items()}, strict=True)
    teacher = vit_models.VisionTransformerTeacher(**common)
    teacher.load_state_dict({k: _t(v) for k, v in sd_t.items()}, strict=True)
    return student.to(DEV), teacher.to(DEV).eval()


@pytest.mark.parametrize("name", ["micro_thr2", "micro_thr3s"])
def test_packed_predictor_function_is_the_inference_launch_sequence(name):
    """RaggedPredictorFn's training forward gives ragged_predictor_forward's bits (large and small LayerNorm predictor): both run
    functional.predictor_forward_sequence, one keeping what the backward reads"""
    from d2s.functional_ragged import ragged_predictor_forward, ragged_predictor_train
    case = R.train_cases()[name]
    student, _ = _student(case)
    D = case["cfg"]["dim"]
    cu = _cu(ROWS).to(DEV)
    xp = torch.randn((int(cu[-1]), D), generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
    pred = student.score_predictor[1]
    got = ragged_predictor_train(pred, xp, cu, len(ROWS))
    with torch.no_grad():
        want = ragged_predictor_forward(pred, xp, cu, len(ROWS))
    assert got.requires_grad and torch.equal(got.detach(), want)


# ---- 3. the model against the float64 reference ----
def _args(case, **kw):
    cfg = case["cfg"]
    return types.SimpleNamespace(keep_ratios=list(cfg["token_ratio"]), mask_loss_type=cfg["loss_type"], mixup=0.0,
                                 patch_score_threshold=case["threshold"], ragged_train=True, step=0, **kw)


def _compare_grads(student, ref_grads, what):
    for k, p in student.named_parameters():
        want = ref_grads[k]
        if want is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        gf, wf = p.grad.detach().flatten().cpu(), want.flatten()
        np.testing.assert_allclose(float(gf.double().norm()), float(wf.norm()), rtol=1e-3, atol=1e-6, err_msg=f"{what} {k}")
        h = min(8, gf.numel())
        np.testing.assert_allclose(gf[:h].numpy(), wf[:h].numpy(), rtol=5e-3, atol=5e-4 * float(wf[:h].abs().max()) + 2e-6, err_msg=f"{what} {k}")


@pytest.mark.parametrize("warmup", [False, True], ids=["full", "warmup"])
@pytest.mark.parametrize("name,mode", [("micro_thr1", "exact"), ("micro_thr2", "exact"), ("micro_thr2", "split"), ("micro_thr3s", "exact")])
def test_model_forward_losses_and_gradients_against_float64(name, mode, warmup):
    """One training-mode forward, both losses and the backward; warm-up: the mask loss alone, which must still reach every predictor
    parameter of every stage - a later stage's through the packed blocks' activations."""
    from d2s import ops
    from losses import MaskLoss, BackboneLoss
    case, _, _, x, y = R.case_tensors(name)
    cfg = case["cfg"]
    B, N, S = case["batch"], cfg["n_patches"], len(cfg["pruning_loc"])
    student, teacher = _student(case, ragged_train=True)
    student.train()
    args = _args(case)
    with ops.gemm_mode({"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[mode]):
        with torch.no_grad():
            logits_t, token_t, cls_attn = teacher(x.to(DEV))
        logits, xn, pred_logits, masks = student(x.to(DEV))
        metrics = {}
        ragged = (list(student.cu_seqlens_per_stage), list(student.ragged_row_src_per_stage))
        mask_loss = MaskLoss(args, "train")(pred_logits, cls_attn, masks, metrics, ragged=ragged)
        backbone_loss = BackboneLoss(args)(logits, xn, logits_t, token_t, masks, y.to(DEV), metrics,
                                           ragged=(student.cu_seqlens, student.ragged_row_src))
        loss = mask_loss if warmup else mask_loss + backbone_loss
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    # the selection: the fp32 restatement's masks (gaps recorded on the CPU tier), offsets and row ids as at inference
    with torch.no_grad():
        ref32 = R.train_forward(R.case_tensors(name)[1], x, cfg, case["threshold"], dtype=torch.float32)
    gpu_masks = [m.detach().cpu() for m in masks]
    assert len(masks) == len(pred_logits) == len(student.cu_seqlens_per_stage) == S
    for s in range(S):
        assert tuple(masks[s].shape) == (B, N) and torch.equal(gpu_masks[s], ref32["masks"][s]), f"stage {s}"
        lens = torch.tensor([int(i.numel()) + 1 for i in ref32["ids"][s]])
        assert torch.equal(student.cu_seqlens_per_stage[s].cpu().long(), torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0))))
        want_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), i + 1)) for i in ref32["ids"][s]])
        assert torch.equal(student.ragged_row_src_per_stage[s].cpu().long(), want_src)
    assert student.cu_seqlens is student.cu_seqlens_per_stage[-1] and student.ragged_row_src is student.ragged_row_src_per_stage[-1]
    np.testing.assert_allclose(student.keep_ratios.cpu().numpy(), gpu_masks[-1].sum(dim=1).numpy() / N, rtol=1e-6)
    # float64 with the GPU's own masks
    out, want_loss, ref_grads, (want_mask, want_bb, _) = R.model_grads(name, masks=gpu_masks, warmup=warmup)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), out["logits"].detach().numpy(), rtol=1e-4, atol=2e-5)
    assert tuple(xn.shape) == (int(student.cu_seqlens[-1]), cfg["dim"])
    np.testing.assert_allclose(xn.detach().cpu().numpy(), R.packed(out["feats"]).detach().numpy(), rtol=1e-4, atol=3e-5)
    assert tuple(pred_logits[0].shape) == (B, N)
    np.testing.assert_allclose(pred_logits[0].detach().cpu().numpy(), out["pred_logits"][0].detach().numpy(), rtol=1e-4, atol=2e-5)
    for s in range(1, S):
        cu = student.cu_seqlens_per_stage[s - 1].cpu().long()
        assert tuple(pred_logits[s].shape) == (int(cu[-1]),)
        live = torch.ones(int(cu[-1]), dtype=torch.bool)
        live[cu[:-1]] = False                                                  # the CLS rows' entries have no meaning
        np.testing.assert_allclose(pred_logits[s].detach().cpu()[live].numpy(), R.packed_scores(out["pred_logits"][s]).detach()[live].numpy(),
                                   rtol=1e-4, atol=2e-5)
    print(f"{name} {mode} {'warm-up' if warmup else 'full'}: loss {float(loss.detach()):.7f} (float64 {float(want_loss):.7f}), mask {float(mask_loss.detach()):.7f} "
          f"({float(want_mask):.7f}), backbone {float(backbone_loss.detach()):.7f} ({float(want_bb):.7f}), rows per stage "
          f"{[int(c[-1]) for c in student.cu_seqlens_per_stage]}")
    np.testing.assert_allclose(float(mask_loss.detach()), float(want_mask), rtol=1e-4)
    np.testing.assert_allclose(float(backbone_loss.detach()), float(want_bb), rtol=1e-4)
    np.testing.assert_allclose(float(loss.detach()), float(want_loss), rtol=1e-4)
    _compare_grads(student, ref_grads, f"{name} {mode}")
    if warmup:
        for k, p in student.named_parameters():
            if "score_predictor" in k:
                assert p.grad is not None and float(p.grad.abs().max()) > 0, f"{k}: the mask loss alone must reach every predictor parameter"


def test_mse_mask_loss_on_the_packed_stages():
    """mask_loss_type mse: the packed stages' term 100 * sum (score - q)^2 / (total - B), forward and gradient to the predictors"""
    from d2s import ops
    from losses import MaskLoss
    name = "micro_thr2"
    case, _, _, x, y = R.case_tensors(name)
    case = dict(case, cfg=dict(case["cfg"], loss_type="mse"))
    student, teacher = _student(case, ragged_train=True)
    student.train()
    with torch.no_grad():
        cls_attn = teacher(x.to(DEV))[2]
    logits, xn, pred_logits, masks = student(x.to(DEV))
    mask_loss = MaskLoss(_args(case), "train")(pred_logits, cls_attn, masks, {},
                                               ragged=(student.cu_seqlens_per_stage, student.ragged_row_src_per_stage))
    mask_loss.backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    sd = {k: _t(v).double().requires_grad_(True) for k, v in cases.make_weights(case)[0].items()}
    out = R.train_forward(sd, x, case["cfg"], case["threshold"], masks=[m.detach().cpu() for m in masks])
    with torch.no_grad():
        teacher_out = O.teacher_forward({k: _t(v).double() for k, v in cases.make_weights(case)[1].items()}, x.double(), case["cfg"])
    want, _, _ = R.losses(out, teacher_out, y, case["cfg"])
    np.testing.assert_allclose(float(mask_loss.detach()), float(want.detach()), rtol=1e-4)
    grads = dict(zip(sd.keys(), torch.autograd.grad(want, list(sd.values()), allow_unused=True)))
    _compare_grads(student, grads, "mse")
    assert float(student.score_predictor[1].in_conv[1].weight.grad.abs().max()) > 0


def test_bf16_mode_is_refused_and_eval_is_untouched():
    from d2s import lib, ops
    from d2s.functional_ats import _BF16_REFUSAL
    case, _, _, x, _ = R.case_tensors("micro_thr2")
    on, _ = _student(case, ragged_train=True)
    off, _ = _student(case)
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            on.train()(x.to(DEV))
    assert str(e.value) == _BF16_REFUSAL
    with torch.no_grad():
        a, b = on.eval()(x.to(DEV)), off.eval()(x.to(DEV))
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
    assert torch.equal(on.ragged_features, off.ragged_features) and torch.equal(on.cu_seqlens, off.cu_seqlens)
    # and the policy-mode training forward of a student built without the keyword is what it was: all N tokens
    out = off.train()(x.to(DEV))
    assert tuple(out[1].shape) == (case["batch"], case["cfg"]["n_patches"], case["cfg"]["dim"])


# ---- 4. TrainStep ----
def _step(name="micro_thr2", **kw):
    from d2s.engine import TrainStep
    case = R.train_cases()[name]
    student, teacher = _student(case, ragged_train=True)
    return TrainStep(student, teacher, _args(case), lr=1e-3, **kw), case


def _batch(case):
    return _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)


def test_train_step_first_loss_two_runs_and_resume():
    from d2s import lib
    ts, case = _step()
    assert ts.ragged_train and ts.graph is False and not ts.logits_only
    x, y = _batch(case)
    info = ts(x, y)
    torch.cuda.synchronize()
    masks = [m.detach().cpu() for m in info["kept"]]
    _, want, _, _ = R.model_grads("micro_thr2", masks=masks)
    print(f"train step: loss {float(info['loss']):.7f}, float64 {float(want):.7f}")
    np.testing.assert_allclose(float(info["loss"]), float(want), rtol=1e-4)
    saved = ts.state_dict()
    assert saved["config"]["ragged_train"] is True
    l2 = float(ts(x, y)["loss"])
    torch.cuda.synchronize()
    two = ts.arena.params.clone()
    # a second run of two steps: bit-identical
    again, _ = _step()
    la = [float(again(x, y)["loss"]), float(again(x, y)["loss"])]
    torch.cuda.synchronize()
    assert la == [float(info["loss"]), l2] and torch.equal(again.arena.params, two)
    # save after step 1, resume, step 2: bit for bit
    resumed, _ = _step()
    assert resumed.load_state_dict(saved) == saved["epoch"]
    assert float(resumed(x, y)["loss"]) == l2
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, two)
    # a checkpoint with the other ragged_train value is refused, either way round
    from d2s.engine import TrainStep
    off_student, teacher = _student(case)
    off = TrainStep(off_student, teacher, types.SimpleNamespace(**{**vars(_args(case)), "ragged_train": False}), lr=1e-3)
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ragged_train"):
        off.load_state_dict(saved)
    old = dict(saved, config={k: v for k, v in saved["config"].items() if k != "ragged_train"})      # written before the key existed: off
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ragged_train"):
        resumed.load_state_dict(old)
    assert off.load_state_dict(old) == saved["epoch"]
    assert "train_mask_loss" in ts.metrics and float(ts.metrics["train_cls_loss"]) > 0


def test_train_step_warmup_accumulation_clipping_and_graph_refusal():
    from d2s import lib
    x, y = _batch(R.train_cases()["micro_thr3s"])
    ts, case = _step("micro_thr3s", warmup_steps=1, accum_steps=2, clip_grad=1.0)
    before = ts.arena.params.clone()
    old = {n: p.detach().clone() for n, p in ts.student.named_parameters()}
    a = ts(x, y)
    assert a["stepped"] is False and torch.equal(ts.arena.params, before)
    b = ts(x, y)
    torch.cuda.synchronize()
    assert b["stepped"] is True and float(b["grad_norm"]) > 0 and not torch.equal(ts.arena.params, before)
    assert float(a["loss"]) == float(a["mask_loss"].detach())                          # epoch 0 < warmup_steps: the mask loss alone
    moved = {n for n, p in ts.student.named_parameters() if not torch.equal(p.detach(), old[n])}
    assert moved and all("score_predictor" in n for n in moved), "warm-up trains the predictors only"
    assert any(n.startswith("score_predictor.2.") for n in moved), "a later stage's predictor moves in the warm-up"
    ts.set_epoch(1)
    c = ts(x, y)
    ts.flush()
    torch.cuda.synchronize()
    assert np.isfinite(float(c["loss"])) and float(c["loss"]) > float(c["mask_loss"].detach())
    with pytest.raises(lib.D2SError, match=r"graph=True\) with ragged_train"):
        _step(graph=True)


def test_validation_reports_the_packed_stage_term():
    """evaluate_performance with args.ragged_train adds the packed stages' term to val_mask_loss; without the flag it is the first stage's"""
    from evaluate import evaluate_performance
    case = R.train_cases()["micro_thr2"]
    student, teacher = _student(case, ragged_train=True)
    x, y = _batch(case)
    args = _args(case, device=torch.device(DEV))
    on = evaluate_performance(args, student, teacher, [(x, y)])
    args.ragged_train = False
    off = evaluate_performance(args, student, teacher, [(x, y)])
    assert float(on["val_mask_loss"]) > float(off["val_mask_loss"]) > 0
    assert float(on["val_mask_acc_1"]) == float(off["val_mask_acc_1"]) and on["val_acc"] == off["val_acc"]


# ---- 5. command line ----
def test_cli_trains_on_the_ragged_batch(tmp_path, capsys):
    import os
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    acc = mask_predictor.main(["--arch", "deit_tiny", "--topk-selection", "--patch-score-threshold", "0.4", "--pruning-locs", "3", "6",
                               "--keep-ratios", "0.7", "0.5", "--ragged-cascade", "--ragged-train", "--warmup-steps", "1", "--epochs", "2",
                               "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--teacher-checkpoint", path,
                               "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Attention: --ragged-train: training follows the cascade definition" in out and "Start training" in out and "val loss:" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert cfg["ragged_train"] is True and cfg["patch_score_threshold"] == 0.4 and cfg["pruning_loc"] == [3, 6]
