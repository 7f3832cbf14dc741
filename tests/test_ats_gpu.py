"""Adaptive token sampling on the GPU: d2s_ats_select against tests/ats_ref.py - the scores against float64, the
selection bit for bit on the kernel's own emitted scores, on fp32 and bf16 qkv - the entry's refusals, the model against the float64
restatement with the GPU's kept sets replayed (fp32 modes and the bf16 data path), a batch whose images end with different token counts,
and the command line."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import ats_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


# ---- 1. the kernel ----
def _inputs(lens, H, seed, N=None):
    """A packed batch of images with lens[b] rows (CLS included): (cls_row [H,total], qkv [total, 3*H*64], cu, row_src, N)"""
    g = torch.Generator().manual_seed(seed)
    total = int(sum(lens))
    N = N or 2 * max(max(lens) - 1, 1)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    cls_row = torch.exp(1.5 * torch.randn((H, total), generator=g)) / 50.0
    qkv = torch.randn((total, 3 * H * 64), generator=g) * torch.exp(0.5 * torch.randn((total, 1), generator=g))
    row_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), torch.sort(torch.randperm(N, generator=g)[:n - 1])[0] + 1)) for n in lens])
    return cls_row, qkv, cu, row_src.int(), N


def _select(cls_row, qkv, cu, row_src, K, N, H, max_n):
    from d2s import ops
    out = ops.ats_select(cls_row.to(DEV), qkv.to(DEV).contiguous(), cu.to(DEV), row_src.to(DEV), K, N, cu.numel() - 1, H, max_n)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _check_selection(score, keep, counts, dense, cu, row_src, K, N):
    """keep / counts / dense_mask bit for bit what the fp32 procedure gives on the emitted scores; CLS entries"""
    cu = [int(c) for c in cu]
    for b in range(len(cu) - 1):
        lo, hi = cu[b] + 1, cu[b + 1]
        assert float(score[cu[b]]) == 0.0 and float(keep[cu[b]]) == 1.0
        want = R.select(score[lo:hi].numpy(), K)
        assert np.array_equal(keep[lo:hi].numpy(), want.astype(np.float32)), (b, K)
        assert int(counts[b]) == int(want.sum())
        assert (1 <= int(counts[b]) <= min(K, hi - lo)) or hi == lo
        row = np.zeros(N, dtype=np.float32)
        row[row_src[lo:hi].numpy()[want] - 1] = 1.0                         # dense_mask follows row_src: original patch coordinates
        assert np.array_equal(dense[b].numpy(), row)


# 301 rows: past the 64-lane boundary and the four-rows-per-wave passes of the norms; 1030 rows: past the 1024-thread chunk of every loop
KERNEL_CASES = [((17, 5, 2), 2, K) for K in (1, 4, 16, 40)] + [((301,), 3, 98), ((1030, 70), 1, 300), ((5, 1, 3), 2, 4), ((1,), 1, 3)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("lens,H,K", KERNEL_CASES, ids=str)
def test_select_against_the_reference(lens, H, K, bf16):
    cls_row, qkv, cu, row_src, N = _inputs(lens, H, seed=7 + len(lens) + K)
    if bf16:
        qkv = qkv.bfloat16()
    score, keep, counts, dense = _select(cls_row, qkv, cu, row_src, K, N, H, max(lens))
    assert score.dtype == keep.dtype == dense.dtype == torch.float32 and counts.dtype == torch.int32 and dense.shape == (len(lens), N)
    ref = R.scores(cls_row.numpy(), qkv.float().numpy()[:, 2 * H * 64:], cu)       # float64 of the same, widened inputs
    np.testing.assert_allclose(score.numpy(), ref, rtol=1e-5, atol=0)
    for b, n in enumerate(lens):
        lo, hi = int(cu[b]) + 1, int(cu[b + 1])
        if n > 1:
            assert abs(float(score[lo:hi].double().sum()) - 1.0) <= 1e-5
        else:
            assert int(counts[b]) == 0 and float(dense[b].sum()) == 0.0     # only the CLS row: the count, the CLS flag, an empty mask row
    _check_selection(score, keep, counts, dense, cu, row_src, K, N)
    again = _select(cls_row, qkv, cu, row_src, K, N, H, max(lens))
    assert all(torch.equal(a, b) for a, b in zip(again, (score, keep, counts, dense)))       # no atomics: bit-identical run to run
    if bf16:                                                                # widening is exact and the sums keep their order
        wide = _select(cls_row, qkv.float(), cu, row_src, K, N, H, max(lens))
        assert torch.equal(wide[0], score) and torch.equal(wide[1], keep)
    roomy = _select(cls_row, qkv, cu, row_src, K, N, H, max(lens) + 40)      # max_n is a bound, not a shape
    assert torch.equal(roomy[0], score) and torch.equal(roomy[1], keep)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_uniform_scores_keep_the_expected_index_sets(bf16):
    """A constant CLS row and constant-norm V: w_j = 1 exactly, so s_j = 1 / T; an all-zero CLS row takes the uniform fallback."""
    lens, H = (17, 5, 2), 2
    _, _, cu, row_src, N = _inputs(lens, H, seed=1)
    total = sum(lens)
    cls_row = torch.full((H, total), 0.25)                                  # a_j = 0.5
    qkv = torch.randn((total, 3 * H * 64), generator=torch.Generator().manual_seed(2))
    qkv[:, 2 * H * 64:] = 0.0
    qkv[torch.arange(total), 2 * H * 64 + (torch.arange(total) * 37) % (H * 64)] = 2.0      # ||V_j|| = 2, the one value anywhere in the row
    qkv = qkv.bfloat16() if bf16 else qkv
    T = [n - 1 for n in lens]
    uni = torch.cat([torch.cat((torch.zeros(1), torch.full((t,), 1.0) / torch.tensor(float(t)))) for t in T])
    for source in (cls_row, torch.zeros_like(cls_row)):
        for K, want in ((16, [list(range(16)), [0, 1, 2, 3], [0]]), (40, [list(range(16)), [0, 1, 2, 3], [0]]),
                        (8, [list(range(0, 16, 2)), [0, 1, 2, 3], [0]]), (2, [[3, 11], [0, 2], [0]]), (1, [[7], [1], [0]])):
            score, keep, counts, dense = _select(source, qkv, cu, row_src, K, N, H, 17)
            assert torch.equal(score, uni)
            got = [torch.nonzero(keep[int(cu[b]) + 1:int(cu[b + 1])]).flatten().tolist() for b in range(3)]
            assert got == want, (K, got)
            assert counts.tolist() == [len(w) for w in want]
            _check_selection(score, keep, counts, dense, cu, row_src, K, N)
    score, keep, _, _ = _select(torch.full((H, total), float("inf")), qkv, cu, row_src, 16, N, H, 17)      # a sum that is not finite
    assert torch.equal(score, uni) and bool((keep == 1).all())


def test_entry_refuses_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, H, total, N, K, max_n = 2, 2, 12, 16, 4, 8
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    cls_row, qkv = f(H, total), f(total, 3 * H * 64)
    cu = torch.tensor([0, 7, 12], dtype=torch.int32, device=DEV)
    row_src = torch.tensor(list(range(7)) + list(range(5)), dtype=torch.int32, device=DEV)
    score, keep, dense = f(total), f(total), f(B, N)
    counts = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    p, s = lib.ptr, lib.stream()

    def sel(c=cls_row, q=qkv, bf=0, cu_=cu, rs=row_src, K_=K, N_=N, B_=B, H_=H, t_=total, m_=max_n, sc=score, kp=keep, ct=counts, dm=dense):
        return lib._fn("d2s_ats_select")(p(c), p(q), bf, p(cu_), p(rs), K_, N_, B_, H_, t_, m_, p(sc), p(kp), p(ct), p(dm), s)

    bad = [sel(c=None), sel(q=None), sel(q=None, bf=1), sel(cu_=None), sel(rs=None), sel(sc=None), sel(kp=None), sel(ct=None),
           sel(B_=0), sel(B_=-1), sel(H_=0), sel(K_=0), sel(K_=-3), sel(K_=(1 << 22) + 1), sel(t_=0), sel(t_=-5), sel(m_=0), sel(m_=2050),
           sel(m_=1 << 20), sel(N_=0), sel(N_=8193)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    for t in (score, keep, dense, counts):                                  # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    assert sel(m_=2049) == 0 and sel(N_=8192, dm=f(B, 8192)) == 0 and sel(dm=None, N_=0) == 0      # the limits themselves; no dense mask
    torch.cuda.synchronize()
    assert counts.tolist() == [4, 4]                                       # constant inputs: uniform scores, K = 4 of 6 and of 4 tokens


# ---- 2. the model ----
_MODELS = {}


def _models(name):
    """(teacher, state dict as tensors, images, geometry) of a parity case, built once"""
    if name not in _MODELS:
        import vit_models
        case = cases.MODEL_CASES[name]
        cfg = case["cfg"]
        geom = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                    mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cases.make_weights(case)[1].items()}
        teacher = vit_models.VisionTransformerTeacher(**geom)
        teacher.load_state_dict(sd)
        images = torch.from_numpy(cases.make_images(case))
        _MODELS[name] = (teacher.to(DEV).eval(), sd, images, geom)
    return _MODELS[name]


def _ats(name, sd=None, **kw):
    import vit_models
    _, sd0, _, geom = _models(name)
    m = vit_models.VisionTransformerATS(**geom, **kw)
    m.load_state_dict(sd0 if sd is None else sd)
    return m.to(DEV).eval()


def _kept_sets(m, B):
    """per stage, per image: the ORIGINAL token indices (CLS = 0 first) that left the stage, read from the model's packed bookkeeping"""
    out = []
    for cu, src in zip(m.cu_seqlens_per_stage, m.ragged_row_src_per_stage):
        cu, src = cu.cpu().tolist(), src.cpu().long()
        out.append([src[cu[b]:cu[b + 1]] for b in range(B)])
    return out


def _sharpened(name, factor):
    """The case's state dict with the query and key rows of every block's qkv scaled: attention logits grow by factor ** 2"""
    _, sd, _, geom = _models(name)
    D = geom["embed_dim"]
    sd = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            sd[k][:2 * D] *= factor
    return sd


def _check_model(name, m, sd, images, mode, tol):
    """One forward in `mode`, its plans replayed (bit for bit), the float64 restatement with the GPU's kept sets, every image alone."""
    from d2s import ops
    cfg = cases.MODEL_CASES[name]["cfg"]
    B, n = images.shape[0], cfg["n_patches"] + 1
    gm = {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}[mode]
    with ops.gemm_mode(gm):
        logits = m(images.to(DEV))
        plans, cus = list(m.ats_plans), list(m.cu_seqlens_per_stage)
        counts = [c.cpu().tolist() for c in m.tokens_per_stage]
        kept = _kept_sets(m, B)
        scores = list(m.ats_scores)
        again = m(images.to(DEV), plans=plans)
        assert torch.equal(again, logits)                                  # replaying the model's own plans changes nothing
        assert m.ats_scores == [None] * len(plans) and [c.cpu().tolist() for c in m.tokens_per_stage] == counts
        alone = []
        cu_in = [torch.arange(B + 1, dtype=torch.int32) * n] + [c.cpu() for c in cus[:-1]]
        for b in range(B):                                                  # image b alone, its slice of every plan replayed
            pl = [(keep[int(ci[b]):int(ci[b + 1])].contiguous(), cnt[b:b + 1].contiguous()) for (keep, cnt), ci in zip(plans, cu_in)]
            alone.append(m(images[b:b + 1].to(DEV), plans=pl))
    assert len(plans) == len(m.ats_locs) and logits.shape == (B, cfg["num_classes"])
    for s, K in enumerate(m.ats_tokens):
        before = [n - 1] * B if s == 0 else counts[s - 1]
        assert all(1 <= c <= min(K, t) for c, t in zip(counts[s], before)), (s, counts)
        assert [len(ids) - 1 for ids in kept[s]] == counts[s] and all(int(ids[0]) == 0 for ids in kept[s])
        assert torch.diff(cus[s].cpu()).tolist() == [c + 1 for c in counts[s]]
        assert scores[s].shape[0] == sum(before) + B
    ref, _ = R.model_forward(sd, images, cfg, m.ats_locs, kept_ids_per_stage=kept)
    print(f"{name} locs {m.ats_locs} K {m.ats_tokens} {mode}: tokens per stage {counts}, "
          f"max |logits - ref| {float((logits.cpu().double() - ref).abs().max()):.3e}")
    np.testing.assert_allclose(logits.cpu().numpy(), ref.numpy(), rtol=tol[0], atol=tol[1])
    np.testing.assert_allclose(torch.cat(alone).cpu().numpy(), logits.cpu().numpy(), rtol=tol[0], atol=tol[1])     # cu indexing
    return counts


@pytest.mark.parametrize("name", ["micro1", "tiny32"])
def test_model_without_a_stage_is_the_teacher_bit_for_bit(name):
    teacher, _, images, _ = _models(name)
    m = _ats(name)
    with torch.no_grad():
        want = teacher(images.to(DEV))[0]
    assert torch.equal(m(images.to(DEV)), want)
    assert m.tokens_per_stage == [] and m.ats_plans == []


STAGE_CASES = [("micro1", [1, 2, 3], 16), ("micro1", [1, 2, 3], [12, 8, 4]), ("micro1", [0], 8), ("tiny32", list(range(3, 12)), 2)]


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("name,locs,K", STAGE_CASES, ids=str)
def test_model_against_float64_with_the_gpu_kept_sets_replayed(name, locs, K, mode):
    _, sd, images, _ = _models(name)
    _check_model(name, _ats(name, ats_locs=locs, ats_tokens=K), sd, images, mode, (1e-4, 2e-5))


@pytest.mark.parametrize("name,locs,K", STAGE_CASES, ids=str)
def test_model_on_the_bf16_data_path(name, locs, K):
    _, sd, images, _ = _models(name)
    _check_model(name, _ats(name, ats_locs=locs, ats_tokens=K), sd, images, "bf16", (3e-2, 3e-2))


def test_a_truly_ragged_batch():
    """Sharper attention makes the images of one batch end with different token counts.  The factor is chosen by the float64 reference
    alone, selecting by its own scores: the first one whose images end with more than one distinct count."""
    name, locs, K = "micro1", [1, 2, 3], 16
    cfg = cases.MODEL_CASES[name]["cfg"]
    _, _, images, _ = _models(name)
    for factor in (2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
        sd = _sharpened(name, factor)
        _, used = R.model_forward(sd, images, cfg, locs, tokens=[K] * len(locs))
        ref_counts = [len(ids) - 1 for ids in used[-1]]
        if len(set(ref_counts)) > 1:
            break
    print(f"factor {factor}: reference token counts after the last stage {ref_counts}")
    assert len(set(ref_counts)) > 1, "no factor made the reference ragged"
    m = _ats(name, sd=sd, ats_locs=locs, ats_tokens=K)
    for mode, tol in (("exact", (1e-4, 2e-5)), ("bf16", (3e-2, 3e-2))):
        counts = _check_model(name, m, sd, images, mode, tol)
        assert len(set(counts[-1])) > 1, counts                             # the batch that reached the head was ragged


def test_training_mode_with_stages_is_refused():
    from vit_models import ats
    _, _, images, _ = _models("micro1")
    m = _ats("micro1", ats_locs=[1], ats_tokens=8).train()
    with pytest.raises(NotImplementedError) as e:
        m(images.to(DEV))
    assert str(e.value) == ats.ATS_TRAINING_ERROR
    dense = _ats("micro1").train()                                          # no stage in training mode: the dense, differentiable trunk
    out = dense(images.to(DEV))
    out.sum().backward()
    assert dense.head.weight.grad is not None and out.shape == (images.shape[0], 10)


# ---- 3. command line ----
def test_cli_evaluates_a_checkpoint_with_predictor_keys(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    sd = vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()
    sd["score_predictor.0.in_conv.0.weight"] = torch.ones(192)               # a dense-to-sparse student's file carries predictors
    path = os.path.join(tmp_path, "student.pt")
    torch.save({"model": sd}, path)
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "ats", "--pruning-locs", "3", "6", "9", "--ats-tokens", "64", "--eval-only",
                               "--student-checkpoint", path, "--batch-size", "4", "--val-steps", "1"])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "ignored 1 predictor tensors" in out and "val loss:" in out and "ats tokens per stage: mean [" in out and " min [" in out and " max [" in out
    assert "Start training" not in out
