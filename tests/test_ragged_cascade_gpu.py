"""GPU tier of ragged inference through every threshold stage (--ragged-cascade): the three kernels of a stage on a
packed batch on their own (csrc/ragged.hip), the eval-mode student with two and three threshold stages against the per-image
restatement (tests/ragged_cascade_ref.py) in fp32 and against its own dense blocks per image in the bf16 arithmetic mode, the unchanged
one-stage launch sequence, and evaluate_performance on a two-stage student.

PARITY UNPINNED for every stage after the first: the reference's second stage cannot run (vit_models/dynamic_vit.py:945-946), so the
checks are against the build's own statement - each image alone through the remaining network.

Tolerances.  Ids, masks, offsets, packed row order, row copies: bit-exact (tests/test_ragged_cascade_cpu.py shows that fp32 and fp64
select the same ids on these cases).  Selection given the kernel's own probabilities: exactly the stable rule on the CPU.  The token
mean: any summation order of T fp32 values plus one division, (T + 1) 2^-24 sum|x| / T per column.  Floating point of the model: what
tests/test_threshold_gpu.py::test_ragged_inference_matches_oracle holds the same kernels to (rtol 1e-4, atol 2e-5 / 3e-5); bf16 mode:
rtol = atol = 3e-2 as tests/test_ragged_bf16_gpu.py."""
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import ragged_cascade_ref as R
from oracle import d2s_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)
NEW_ENTRIES = ("d2s_half_mean_concat_varlen", "d2s_ragged_select_threshold", "d2s_ragged_repack")
# non-CLS rows per image: a CLS-only image, the wave boundaries, the 256-thread chunk boundary, more than two chunks
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 577)
CASES = R.cascade_cases()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cu(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths) + 1)]).astype(np.int32)


def _normal(tag, shape, seed=1, std=1.0):
    from d2s import synth
    return _t(synth.normal(f"rc/{tag}", shape, std=std, seed=seed))


def _row_src(lengths, N, seed=5):
    """per image: 0 for CLS, then an ascending subset of 1..N (the original token index of every packed row)"""
    rng = np.random.RandomState(seed)
    return np.concatenate([np.concatenate([[0], 1 + np.sort(rng.permutation(N)[:T])]) for T in lengths]).astype(np.int32)


def _spy_calls(monkeypatch):
    from d2s import lib
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return names


# ---- 1. the kernels alone ----
def test_repack_is_numpy_indexing_bit_for_bit():
    from d2s import ops
    B, D, N = len(LENGTHS), 128, 600
    cu = _cu(LENGTHS)
    total = int(cu[-1])
    x = _normal("repack/x", (total, D))
    src = _row_src(LENGTHS, N)
    keep = (_normal("repack/keep", (total,), seed=2) > 0.1).float().numpy()
    keep[cu[5] + 1:cu[6]] = 1.0                # the 255-token image keeps everything
    keep[cu[6] + 1:cu[7]] = 0.0                # the 256-token image keeps nothing but its CLS token
    keep[cu[:-1]] = 1.0
    sel = np.nonzero(keep > 0)[0]
    counts = np.array([int(keep[cu[b] + 1:cu[b + 1]].sum()) for b in range(B)], dtype=np.int32)
    assert counts[0] == 0 and counts[5] == 255 and counts[6] == 0
    cu_new = ops.ragged_offsets(_t(counts).to(DEV), extra=1)
    want_cu = np.concatenate([[0], np.cumsum(counts + 1)])
    np.testing.assert_array_equal(cu_new.cpu().numpy(), want_cu)
    out, src_new = ops.ragged_repack(x.to(DEV), _t(keep).to(DEV), _t(cu).to(DEV), cu_new, _t(src).to(DEV), int(want_cu[-1]), B)
    torch.cuda.synchronize()
    assert out.shape == (len(sel), D)
    np.testing.assert_array_equal(out.cpu().numpy(), x.numpy()[sel])
    np.testing.assert_array_equal(src_new.cpu().numpy(), src[sel])


@pytest.mark.parametrize("C", [128, 20])
def test_half_mean_concat_varlen(C):
    """C = 128: the 16-byte form; C = 20: the scalar form"""
    from d2s import ops
    B = len(LENGTHS)
    cu = _cu(LENGTHS)
    total, half = int(cu[-1]), C // 2
    x = _normal(f"hmc/{C}", (total, C), seed=3)
    out = ops.half_mean_concat_varlen(x.to(DEV), _t(cu).to(DEV), B).cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :half], x[:, :half]), "the first half is a copy"
    for b, T in enumerate(LENGTHS):
        got = out[cu[b]:cu[b + 1], half:].double()
        assert bool((got == got[:1]).all()), "every row of a segment, the CLS row too, receives the same mean"
        if T == 0:
            assert bool((got == 0).all())
            continue
        seg = x[cu[b] + 1:cu[b + 1], half:].double()
        bound = (T + 1) * 2.0 ** -24 * seg.abs().sum(dim=0) / T
        err = (got[0] - seg.mean(dim=0)).abs()
        print(f"half-mean varlen C {C} T {T}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (C, T)


def test_ragged_select_threshold_is_the_stable_rule_per_segment():
    from d2s import lib
    B, N, th = len(LENGTHS), 600, 0.3
    cu = _cu(LENGTHS)
    total = int(cu[-1])
    scores = _normal("sel/scores", (total,), seed=4, std=1.5)
    src = _row_src(LENGTHS, N)
    nan = float("nan")
    probs, keep = torch.full((total,), nan, device=DEV), torch.full((total,), nan, device=DEV)
    dense = torch.full((B, N), nan, device=DEV)
    counts = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    cu_d, src_d, sc_d = _t(cu).to(DEV), _t(src).to(DEV), scores.to(DEV)
    lib.call("d2s_ragged_select_threshold", sc_d.data_ptr(), cu_d.data_ptr(), src_d.data_ptr(), th, N, probs.data_ptr(), keep.data_ptr(),
             counts.data_ptr(), dense.data_ptr(), B)
    torch.cuda.synchronize()
    probs, keep, dense, counts = probs.cpu(), keep.cpu(), dense.cpu(), counts.cpu()
    assert torch.isfinite(probs).all() and torch.isfinite(keep).all()
    assert torch.isfinite(dense).all(), "every dense_mask row is written in full"
    for b, T in enumerate(LENGTHS):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        assert keep[r0] == 1.0
        want_dense = torch.zeros(N)
        if T > 0:
            p = probs[r0 + 1:r1]
            np.testing.assert_allclose(p.numpy(), scores[r0 + 1:r1].double().softmax(dim=0).numpy(), rtol=1e-5)
            stable, scount = O.select_threshold_stable(p[None], th)
            assert torch.equal(keep[r0 + 1:r1], stable[0]), T
            assert int(counts[b]) == int(scount[0]) >= 1, T
            want_dense[_t(src[r0 + 1:r1]).long()[stable[0] > 0] - 1] = 1.0
        else:
            assert int(counts[b]) == 0
        assert torch.equal(dense[b], want_dense), T
    # probs == NULL: the same selection
    keep2, counts2 = torch.empty((total,), device=DEV), torch.empty((B,), dtype=torch.int32, device=DEV)
    dense2 = torch.empty((B, N), device=DEV)
    lib.call("d2s_ragged_select_threshold", sc_d.data_ptr(), cu_d.data_ptr(), src_d.data_ptr(), th, N, None, keep2.data_ptr(),
             counts2.data_ptr(), dense2.data_ptr(), B)
    assert torch.equal(keep2.cpu(), keep) and torch.equal(counts2.cpu(), counts) and torch.equal(dense2.cpu(), dense)


@pytest.mark.parametrize("T", [16, 196, 300])
def test_equal_lengths_are_the_dense_kernels_bit_for_bit(T):
    from d2s import ops
    B, th = 3, 0.35
    cu = _t(_cu([T] * B)).to(DEV)
    scores = _normal(f"eq/scores/{T}", (B, T), seed=6, std=1.5)
    packed = torch.cat((torch.full((B, 1), 1e9), scores), dim=1).reshape(-1)        # a value at the CLS slot that must not be read
    src = torch.arange(T + 1, dtype=torch.int32).repeat(B)
    keep, counts, dense, probs = ops.ragged_select_threshold(packed.to(DEV), cu, src.to(DEV), th, T, B, want_probs=True)
    dprobs = ops.softmax_rows(scores.to(DEV))
    dmask, dcounts = ops.select_threshold(dprobs, th)
    assert torch.equal(probs.view(B, T + 1)[:, 1:], dprobs)
    assert torch.equal(keep.view(B, T + 1)[:, 1:], dmask) and bool((keep.view(B, T + 1)[:, 0] == 1).all())
    assert torch.equal(counts, dcounts) and torch.equal(dense, dmask)
    assert 0 < int(counts.min()) and int(counts.max()) < T
    for C in (128, 20):
        x = _normal(f"eq/x/{T}/{C}", (B, T + 1, C), seed=7)
        out = ops.half_mean_concat_varlen(x.view(B * (T + 1), C).to(DEV), cu, B).view(B, T + 1, C)
        want = ops.half_mean_concat(x[:, 1:].contiguous().view(B * T, C).to(DEV), B, T, C).view(B, T, C)
        assert torch.equal(out[:, 1:], want), (T, C)


def test_argument_checks():
    """the error returns of the dense siblings, through the bound functions: a refused call launches nothing"""
    from d2s import lib
    B, D, N = 2, 128, 16
    cu = _t(_cu([3, 4])).to(DEV)
    total = 9
    x, out = torch.zeros(total, D, device=DEV), torch.zeros(total, D, device=DEV)
    v, keep = torch.zeros(total, device=DEV), torch.ones(total, device=DEV)
    src = torch.zeros(total, dtype=torch.int32, device=DEV)
    counts, dense = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, N, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    s = lib.stream()
    hmc, sel, rep = (lib._fn(n) for n in NEW_ENTRIES)
    assert hmc(P(x), P(cu), P(out), B, D, s) == 0
    for bad in ((None, P(cu), P(out), B, D), (P(x), None, P(out), B, D), (P(x), P(cu), None, B, D), (P(x), P(cu), P(out), 0, D),
                (P(x), P(cu), P(out), B, 0), (P(x), P(cu), P(out), B, 21)):
        assert hmc(*bad, s) == ERR_ARG, bad
    assert sel(P(v), P(cu), P(src), 0.3, N, None, P(keep), P(counts), P(dense), B, s) == 0
    for bad in ((None, P(cu), P(src), 0.3, N, None, P(keep), P(counts), P(dense), B), (P(v), None, P(src), 0.3, N, None, P(keep), P(counts), P(dense), B),
                (P(v), P(cu), None, 0.3, N, None, P(keep), P(counts), P(dense), B), (P(v), P(cu), P(src), 0.3, N, None, None, P(counts), P(dense), B),
                (P(v), P(cu), P(src), 0.3, N, None, P(keep), None, P(dense), B), (P(v), P(cu), P(src), 0.3, N, None, P(keep), P(counts), None, B),
                (P(v), P(cu), P(src), 0.3, 0, None, P(keep), P(counts), P(dense), B), (P(v), P(cu), P(src), 0.3, 8193, None, P(keep), P(counts), P(dense), B),
                (P(v), P(cu), P(src), 0.3, N, None, P(keep), P(counts), P(dense), 0)):
        assert sel(*bad, s) == ERR_ARG, bad
    cu_new = _t(_cu([3, 4])).to(DEV)
    srcn = torch.zeros(total, dtype=torch.int32, device=DEV)
    good = (P(x), P(keep), P(cu), P(cu_new), P(src), P(out), P(srcn), B, D)
    assert rep(*good, s) == 0
    for i in range(7):
        assert rep(*(good[:i] + (None,) + good[i + 1:]), s) == ERR_ARG, i
    for bad in (good[:7] + (0, D), good[:7] + (B, 0), good[:7] + (B, 126)):
        assert rep(*bad, s) == ERR_ARG, bad
    torch.cuda.synchronize()


# ---- 2. the model ----
def _student(case, **kw):
    import vit_models
    cfg = case["cfg"]
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    args = dict(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True,
                predictor_loss_type=cfg["loss_type"], small_predictor=cfg["small_predictor"], patch_score_threshold=case["threshold"])
    args.update(kw)
    student = vit_models.VisionTransformerDiffPruning(**args, **common)
    if not kw.get("predictor_bn"):
        sd_s, _ = cases.make_weights(case)
        student.load_state_dict({k: _t(v) for k, v in sd_s.items()}, strict=True)
    return student.to(DEV).eval()


def _packed_ids(per_image):
    return torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), ids + 1)) for _, ids, _ in per_image]).int()


@pytest.mark.parametrize("name", list(CASES))
def test_cascade_matches_the_per_image_restatement(name):
    case = CASES[name]
    cfg = case["cfg"]
    locs, N, S, B = list(cfg["pruning_loc"]), cfg["n_patches"], len(cfg["pruning_loc"]), case["batch"]
    rlogits, rfeats, stages = R.reference(name)
    ragged = [len(set(int(ids.numel()) for _, ids, _ in per_image)) > 1 for per_image in stages]
    assert any(ragged), "the case should be genuinely ragged at some stage"
    student = _student(case)
    x = _t(cases.make_images(case)).to(DEV)
    with torch.no_grad():
        logits, cls_attns, pred_logits, masks = student(x)
    torch.cuda.synchronize()
    assert len(masks) == len(pred_logits) == len(student.cu_seqlens_per_stage) == len(student.ragged_row_src_per_stage) == S
    want_masks, want_cu = R.dense_masks(stages, N), R.cu_seqlens(stages)
    for s in range(S):
        assert tuple(masks[s].shape) == (B, N)
        np.testing.assert_array_equal(masks[s].cpu().numpy(), want_masks[s].numpy(), err_msg=f"stage {s}")
        np.testing.assert_array_equal(student.cu_seqlens_per_stage[s].cpu().numpy(), want_cu[s].numpy(), err_msg=f"stage {s}")
        np.testing.assert_array_equal(student.ragged_row_src_per_stage[s].cpu().numpy(), _packed_ids(stages[s]).numpy(), err_msg=f"stage {s}")
    np.testing.assert_array_equal(student.cu_seqlens.cpu().numpy(), want_cu[-1].numpy())
    np.testing.assert_array_equal(student.ragged_row_src.cpu().numpy(), _packed_ids(stages[-1]).numpy())
    last = torch.tensor([float(ids.numel()) for _, ids, _ in stages[-1]])
    np.testing.assert_allclose(student.keep_ratios.cpu().numpy(), (last / N).numpy(), rtol=1e-6)
    np.testing.assert_allclose(logits.cpu().numpy(), rlogits.numpy(), rtol=1e-4, atol=2e-5)
    cu = want_cu[-1].numpy()
    assert tuple(student.ragged_features.shape) == (int(cu[-1]), cfg["dim"])
    for b, f in enumerate(rfeats):
        np.testing.assert_allclose(student.ragged_features[cu[b]:cu[b + 1]].cpu().numpy(), f.numpy(), rtol=1e-4, atol=3e-5)
    assert tuple(pred_logits[0].shape) == (B, N)
    np.testing.assert_allclose(pred_logits[0].cpu().numpy(), torch.stack([sc for _, _, sc in stages[0]]).numpy(), rtol=1e-4, atol=2e-5)
    for s in range(1, S):
        pc = want_cu[s - 1].numpy()
        assert tuple(pred_logits[s].shape) == (int(pc[-1]),)
        for b, (T, _, sc) in enumerate(stages[s]):
            assert T == pc[b + 1] - pc[b] - 1
            np.testing.assert_allclose(pred_logits[s][pc[b] + 1:pc[b + 1]].cpu().numpy(), sc.numpy(), rtol=1e-4, atol=2e-5)
    # CLS rows: dense before the first stage, none from a pruning block, packed [H, total_s] after stage s - each image's a probability row
    assert len(cls_attns) == cfg["depth"] - S
    it, stage, packed_seen = iter(cls_attns), -1, 0
    for i in range(cfg["depth"]):
        if i in locs:
            stage += 1
            continue
        rows = next(it)
        if stage < 0:
            assert tuple(rows.shape) == (B, cfg["heads"], N)
            continue
        c = want_cu[stage].numpy()
        assert tuple(rows.shape) == (cfg["heads"], int(c[-1])), (i, stage)
        for b in range(B):
            np.testing.assert_allclose(rows[:, c[b]:c[b + 1]].sum(dim=1).cpu().numpy(), 1.0, rtol=1e-5)
        packed_seen += 1
    assert packed_seen >= 1
    # threshold 0 keeps every token at every stage: the dense forward
    student.patch_score_threshold = 0.0
    with torch.no_grad():
        l0, _, _, m0 = student(x)
    assert all(bool((m == 1).all()) for m in m0) and len(m0) == S
    sd_s, _ = cases.make_weights(case)
    with torch.no_grad():
        dl, _, _ = O.teacher_forward({k: _t(v) for k, v in sd_s.items()}, _t(cases.make_images(case)), cfg)
    np.testing.assert_allclose(l0.cpu().numpy(), dl.numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("name", ["micro_thr2", "small_thr3"])
def test_cascade_in_bf16_mode_matches_the_dense_blocks_per_image(name, monkeypatch):
    """The per-stage masks are read back, then every image alone goes through the model's own dense blocks (bf16 mode, forward only) on the
    subsets those masks give, stage by stage."""
    from d2s import ops
    case = CASES[name]
    cfg = case["cfg"]
    locs, D, first = list(cfg["pruning_loc"]), cfg["dim"], cfg["pruning_loc"][0]
    student = _student(case)
    x = _t(cases.make_images(case)).to(DEV)
    B = x.shape[0]
    names = _spy_calls(monkeypatch)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        logits, _, _, masks = student(x)
        ragged_names = list(names)
        after = ragged_names[ragged_names.index("d2s_ragged_pack"):]
        attends = [s for s in after if s.startswith("d2s_attn_")]
        assert attends == ["d2s_attn_varlen_fwd_bf16"] * (cfg["depth"] - first), attends
        assert [s for s in NEW_ENTRIES if s not in after] == []
        cu = student.cu_seqlens.cpu().numpy()
        feats = student.ragged_features.clone()
        masks = [m.cpu() for m in masks]
        np.testing.assert_array_equal(cu, np.concatenate([[0], np.cumsum(masks[-1].sum(dim=1).int().numpy() + 1)]))
        for s in range(1, len(masks)):
            assert bool((masks[s] <= masks[s - 1]).all()), "a dropped token is gone"
        x0 = student._embed(x)
        for blk in student.blocks[:first]:
            x0 = blk(x0)
        for b in range(B):
            ids = torch.nonzero(masks[0][b] > 0).flatten()
            xb = x0[b].index_select(0, torch.cat((torch.zeros(1, dtype=torch.long), ids + 1)).to(DEV)).view(1, -1, D).contiguous()
            stage = 1
            for i in range(first, cfg["depth"]):
                if i in locs and i != first:
                    keep = masks[stage][b][ids] > 0
                    ids = ids[keep]
                    xb = xb[:, torch.cat((torch.ones(1, dtype=torch.bool), keep)).to(DEV)].contiguous()
                    stage += 1
                xb = student.blocks[i](xb)
            nb = xb.shape[1]
            assert nb == cu[b + 1] - cu[b]
            want_logits, _ = student._head(xb)
            want_feats, _, _ = ops.layernorm_fwd(xb.view(nb, D), ops.contiguous_map(nb, D), student.norm.weight, student.norm.bias, nb, D,
                                                 student.norm.eps, stats=False)
            err = float((feats[cu[b]:cu[b + 1]] - want_feats).abs().max())
            print(f"ragged cascade bf16 {name} image {b} ({nb} tokens): max abs feature difference {err:.3e}")
            np.testing.assert_allclose(feats[cu[b]:cu[b + 1]].cpu().numpy(), want_feats.cpu().numpy(), rtol=3e-2, atol=3e-2)
            np.testing.assert_allclose(logits[b].cpu().numpy(), want_logits[0].cpu().numpy(), rtol=3e-2, atol=3e-2)


def test_one_stage_model_issues_none_of_the_new_entries(monkeypatch):
    case = cases.THRESHOLD_CASES["micro_thr1"]
    student = _student(case)
    x = _t(cases.make_images(case)).to(DEV)
    names = _spy_calls(monkeypatch)
    with torch.no_grad():
        student(x)
    assert [s for s in NEW_ENTRIES if s in names] == [] and names.count("d2s_ragged_pack") == 1
    assert len(student.cu_seqlens_per_stage) == 1 and student.cu_seqlens_per_stage[0] is student.cu_seqlens
    assert len(student.ragged_row_src_per_stage) == 1 and student.ragged_row_src_per_stage[0] is student.ragged_row_src


def test_evaluate_performance_on_a_two_stage_threshold_student():
    import vit_models
    from evaluate import evaluate_performance
    from utils import SyntheticLoader
    case = CASES["micro_thr2"]
    cfg = case["cfg"]
    N = cfg["n_patches"]
    student = _student(case)
    teacher = vit_models.VisionTransformerTeacher(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                                                  num_heads=cfg["heads"], mlp_ratio=cfg["mlp_ratio"], qkv_bias=True,
                                                  num_classes=cfg["num_classes"])
    _, sd_t = cases.make_weights(case)
    teacher.load_state_dict({k: _t(v) for k, v in sd_t.items()}, strict=True)
    teacher = teacher.to(DEV).eval()
    args = types.SimpleNamespace(keep_ratios=list(cfg["token_ratio"]), mask_loss_type="kl_div", patch_score_threshold=case["threshold"],
                                 device=DEV)
    loader = SyntheticLoader(2, case["batch"], img_size=cfg["img_size"], num_classes=cfg["num_classes"], seed=7)
    metrics = evaluate_performance(args, student, teacher, loader)
    for key in ("val_mask_acc_0", "val_mask_acc_1"):
        assert 0.0 <= float(metrics[key]) <= 1.0, (key, float(metrics[key]))
    assert np.isfinite(float(metrics["val_mask_loss"]))
    ratios = []
    with torch.no_grad():
        for xb, _ in loader:
            _, _, _, masks = student(xb.to(DEV))
            ratios.append(float((masks[-1].sum(dim=1) / N).mean()))
    assert abs(float(metrics["val_avg_keep_ratio"]) - float(np.mean(ratios))) < 1e-6
    bn = _student(case, predictor_bn=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="BatchNorm"):
        bn(_t(cases.make_images(case)).to(DEV))
