"""Training through adaptive token sampling on the GPU ("Training through the stages"): the varlen attention
forward with lse and its backward against float64 (tests/ats_train_ref.py) and against the dense kernels bit for bit, the re-pack and
CLS-scatter backward against their index-based statements, the entries' refusals, the train_sample model against float64 autograd with the
GPU's kept sets replayed (bit-identical to the eval forward where every block is ragged; a truly ragged batch; the embedding gradients),
the train step (loss, three steps, checkpoint) and the command line.

Tolerances are the project's: lse at tests/test_kernels_gpu.py:254 (rtol 1e-5 / atol 1e-5), the attention backward at
tests/test_kernels_gpu.py:257 (rtol 2e-4 / atol 5e-5); the model at tests/test_tome_train_gpu.py:285 (logits rtol 1e-4 / atol 2e-5),
:290 (gradient norms rtol 1e-3 / atol 1e-6) and :292 (leading elements rtol 5e-3, atol 5e-4 max|ref| + 2e-6); the first step's loss at
tests/test_tome_train_gpu.py:333 (rtol 1e-4).  Everything else is bit for bit."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import ats_ref as R
from tests import ats_train_ref as T
from tests.test_ats_train_cpu import RAGGED, ragged_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SCALE = 0.125


# ---- 1. varlen attention: forward with lse, backward ----
# (segment lengths, H, max_n): CLS-only images, the 32-key tile edge, a second 128-row tile for one image only, equal lengths, three tiles
ATTN_CASES = ([((17, 5, 2), H, 17) for H in (1, 2)] + [((1, 9, 1), H, 9) for H in (1, 2)] + [((33, 32, 31), H, 33) for H in (1, 2)]
              + [((130, 3), H, 130) for H in (1, 2)] + [((197, 197), H, 197) for H in (1, 2)] + [((301,), 3, 301)])
_ATTN = {}


def _attn_case(lens, H):
    """inputs and the float64 reference of a case, computed once and left unchanged"""
    key = (lens, H)
    if key not in _ATTN:
        g = torch.Generator().manual_seed(700 + 13 * sum(lens) + H)
        total = sum(lens)
        qkv = torch.randn((total, 3 * H * 64), generator=g)
        dout = torch.randn((total, H * 64), generator=g)
        cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
        out, lse, cls_row = T.varlen_attention(qkv, cu, H, SCALE)
        _ATTN[key] = dict(qkv=qkv, dout=dout, cu=cu, out=out, lse=lse, cls_row=cls_row, dqkv=T.varlen_attention_grad(qkv, cu, H, SCALE, dout))
    return _ATTN[key]


def _bwd_raw(qkv, cu, out, dout, lse, dqkv, delta, B, total, max_n, H):
    from d2s import lib
    p = lib.ptr
    return lib._fn("d2s_attn_varlen_bwd_f32")(p(qkv), p(cu), p(out), p(dout), p(lse), p(dqkv), p(delta), B, total, max_n, H,
                                              ctypes.c_float(SCALE), lib.stream())


@pytest.mark.parametrize("lens,H,max_n", ATTN_CASES, ids=str)
def test_varlen_forward_with_lse(lens, H, max_n):
    from d2s import ops
    c = _attn_case(lens, H)
    B, total = len(lens), sum(lens)
    qd, cud = c["qkv"].to(DEV), c["cu"].to(DEV)
    out0, cls0 = ops.attn_varlen_fwd(qd, cud, B, total, max_n, H, SCALE, want_cls=True)
    out, lse, cls_row = ops.attn_varlen_fwd_lse(qd, cud, B, total, max_n, H, SCALE, want_cls=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(cls_row, cls0)             # the existing entry's bits
    assert lse.shape == (H, total)
    print(f"varlen fwd lse {lens} H={H}: max |lse - ref| {float((lse.cpu().double() - c['lse']).abs().max()):.3e}")
    np.testing.assert_allclose(lse.cpu().numpy(), c["lse"].numpy(), rtol=1e-5, atol=1e-5)
    out1, lse1, cls1 = ops.attn_varlen_fwd_lse(qd, cud, B, total, max_n, H, SCALE, want_cls=False)
    assert cls1 is None and torch.equal(out1, out) and torch.equal(lse1, lse)


@pytest.mark.parametrize("lens,H,max_n", ATTN_CASES, ids=str)
def test_varlen_backward_against_float64_and_the_dense_kernels(lens, H, max_n):
    from d2s import ops
    c = _attn_case(lens, H)
    B, total = len(lens), sum(lens)
    qd, cud, dd = c["qkv"].to(DEV), c["cu"].to(DEV), c["dout"].to(DEV)
    out, lse, _ = ops.attn_varlen_fwd_lse(qd, cud, B, total, max_n, H, SCALE)
    # the raw entry into a NaN-filled dqkv followed by a guard band: every element written, nothing past the end
    buf = torch.full((total * 3 * H * 64 + 4096,), float("nan"), device=DEV)
    delta = torch.empty((H, total), device=DEV)
    assert _bwd_raw(qd, cud, out, dd, lse, buf, delta, B, total, max_n, H) == 0
    torch.cuda.synchronize()
    dqkv = buf[:total * 3 * H * 64].view(total, 3 * H * 64)
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isnan(buf[total * 3 * H * 64:]).all())
    got = dqkv.cpu()
    print(f"varlen bwd {lens} H={H}: max abs err {float((got.double() - c['dqkv']).abs().max()):.3e}, max |ref| {float(c['dqkv'].abs().max()):.3e}")
    np.testing.assert_allclose(got.numpy(), c["dqkv"].numpy(), rtol=2e-4, atol=5e-5)
    # two runs, and a larger grid bound: the same bits
    assert torch.equal(ops.attn_varlen_bwd(qd, cud, out, dd, lse, B, total, max_n, H, SCALE), dqkv)
    assert torch.equal(ops.attn_varlen_bwd(qd, cud, out, dd, lse, B, total, 300 if max_n < 300 else 400, H, SCALE), dqkv)
    # every image's rows: the dense backward on that image alone
    cu = c["cu"].tolist()
    for b, n in enumerate(lens):
        lo, hi = cu[b], cu[b + 1]
        alone = ops.attn_bwd(qd[lo:hi].contiguous(), out[lo:hi].contiguous(), dd[lo:hi].contiguous(), lse[:, lo:hi].contiguous().view(1, H, n),
                             1, n, H, SCALE)
        assert torch.equal(alone, dqkv[lo:hi]), (b, n)
    if len(set(lens)) == 1:                                                  # equal lengths: the batched dense call
        n = lens[0]
        lse_d = lse.view(H, B, n).transpose(0, 1).contiguous()
        assert torch.equal(ops.attn_bwd(qd, out, dd, lse_d, B, n, H, SCALE), dqkv)


def test_attention_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, H, total, max_n = 2, 2, 12, 8
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    qkv, out, dout, lse, cls_row, dqkv, delta = f(total, 3 * H * 64), f(total, H * 64), f(total, H * 64), f(H, total), f(H, total), f(total, 3 * H * 64), f(H, total)
    cu = torch.tensor([0, 7, 12], dtype=torch.int32, device=DEV)
    p, s, sc = lib.ptr, lib.stream(), ctypes.c_float(SCALE)

    def fwd(q=qkv, c=cu, o=out, l=lse, cr=cls_row, B_=B, t_=total, m_=max_n, H_=H):
        return lib._fn("d2s_attn_varlen_fwd_lse_f32")(p(q), p(c), p(o), p(l), p(cr), B_, t_, m_, H_, sc, s)

    def bwd(q=qkv, c=cu, o=out, g=dout, l=lse, dq=dqkv, ws=delta, B_=B, t_=total, m_=max_n, H_=H):
        return lib._fn("d2s_attn_varlen_bwd_f32")(p(q), p(c), p(o), p(g), p(l), p(dq), p(ws), B_, t_, m_, H_, sc, s)

    bad = [fwd(q=None), fwd(c=None), fwd(o=None), fwd(l=None), fwd(B_=0), fwd(t_=0), fwd(m_=0), fwd(m_=8193), fwd(H_=0), fwd(B_=-1),
           bwd(q=None), bwd(c=None), bwd(o=None), bwd(g=None), bwd(l=None), bwd(dq=None), bwd(ws=None), bwd(B_=0), bwd(t_=0), bwd(t_=-3),
           bwd(m_=0), bwd(m_=8193), bwd(H_=0), bwd(m_=8192, H_=2731)]         # the last: an image's panel past 32-bit element offsets
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    for t in (out, lse, cls_row, dqkv, delta):                              # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    assert fwd(cr=None) == 0 and bwd() == 0                                 # the CLS row is optional
    torch.cuda.synchronize()
    assert bool((cls_row == 7).all()) and bool((dqkv != 7).any(dim=1).all())


# ---- 2. re-pack backward, CLS scatter ----
def _flags(kind, total, g):
    return {"mixed": lambda: (torch.rand(total, generator=g) < 0.5).float(), "all": lambda: torch.ones(total), "none": lambda: torch.zeros(total)}[kind]()


ROW_CASES = [((17, 5, 2), k) for k in ("mixed", "all", "none")] + [((1030, 70), "mixed")]      # 1030 rows: past the 256-row chunk


@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("lens,kind", ROW_CASES, ids=str)
def test_repack_backward_and_cls_scatter_bit_exact(lens, kind, D):
    from d2s import lib, ops
    g = torch.Generator().manual_seed(40 + sum(lens) + D)
    B, total = len(lens), sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    keep = _flags(kind, total, g)
    x = torch.randn((total, D), generator=g)
    _, cu_new, idx = T.repack(x, keep, cu.tolist())
    counts = torch.tensor([cu_new[b + 1] - cu_new[b] - 1 for b in range(B)], dtype=torch.int32)
    cud, keepd = cu.to(DEV), keep.to(DEV)
    cund = ops.ragged_offsets(counts.to(DEV), extra=1)
    assert cund.cpu().tolist() == cu_new
    # the forward it inverts: the rows the reference indexing names
    row_src = torch.arange(total, dtype=torch.int32, device=DEV)
    y, _ = ops.ragged_repack(x.to(DEV), keepd, cud, cund, row_src, cu_new[-1], B)
    assert torch.equal(y.cpu(), x[idx])
    g_new = torch.randn((cu_new[-1], D), generator=g)
    buf = torch.full((total * D + 1024,), float("nan"), device=DEV)
    rc = lib._fn("d2s_ragged_repack_bwd")(lib.ptr(g_new.to(DEV)), lib.ptr(keepd), lib.ptr(cud), lib.ptr(cund), lib.ptr(buf), B, D, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(buf[total * D:]).all())
    want = T.repack_backward(g_new.numpy(), keep.numpy(), cu.tolist(), cu_new)
    assert np.array_equal(buf[:total * D].cpu().numpy().reshape(total, D), want)             # NaN anywhere would differ: fully overwritten
    assert torch.equal(ops.ragged_repack_bwd(g_new.to(DEV), keepd, cud, cund, total, B).cpu(), torch.from_numpy(want))
    # CLS scatter
    g_cls = torch.randn((B, D), generator=g)
    buf = torch.full((total * D + 1024,), float("nan"), device=DEV)
    rc = lib._fn("d2s_ragged_cls_scatter")(lib.ptr(g_cls.to(DEV)), lib.ptr(cud), lib.ptr(buf), B, total, D, lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(buf[total * D:]).all())
    want = T.cls_scatter(g_cls.numpy(), cu.tolist(), total)
    assert np.array_equal(buf[:total * D].cpu().numpy().reshape(total, D), want)
    assert torch.equal(ops.ragged_cls_scatter(g_cls.to(DEV), cud, total).cpu(), torch.from_numpy(want))
    assert torch.equal(ops.gather_rows_i32(ops.ragged_cls_scatter(g_cls.to(DEV), cud, total), cud, B).cpu(), g_cls)


def test_row_move_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, total, D = 2, 12, 64
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    g_new, keep, g_old, g_cls, g = f(total, D), f(total), f(total, D), f(B, D), f(total, D)
    cu = torch.tensor([0, 7, 12], dtype=torch.int32, device=DEV)
    p, s = lib.ptr, lib.stream()

    def rb(a=g_new, k=keep, co=cu, cn=cu, o=g_old, B_=B, D_=D):
        return lib._fn("d2s_ragged_repack_bwd")(p(a), p(k), p(co), p(cn), p(o), B_, D_, s)

    def cs(a=g_cls, c=cu, o=g, B_=B, t_=total, D_=D):
        return lib._fn("d2s_ragged_cls_scatter")(p(a), p(c), p(o), B_, t_, D_, s)

    bad = [rb(a=None), rb(k=None), rb(co=None), rb(cn=None), rb(o=None), rb(B_=0), rb(D_=0), rb(D_=66),
           cs(a=None), cs(c=None), cs(o=None), cs(B_=0), cs(t_=0), cs(D_=0), cs(D_=66)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert bool((g_old == 7).all()) and bool((g == 7).all())


# ---- 3. the model ----
_MODELS = {}


def _models(name):
    """(state dict as tensors, images, geometry) of a parity case, built once"""
    if name not in _MODELS:
        case = cases.MODEL_CASES[name]
        cfg = case["cfg"]
        geom = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                    mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cases.make_weights(case)[1].items()}
        _MODELS[name] = (sd, torch.from_numpy(cases.make_images(case)), geom)
    return _MODELS[name]


def _ats(name, sd=None, **kw):
    import vit_models
    sd0, _, geom = _models(name)
    m = vit_models.VisionTransformerATS(**geom, **kw)
    m.load_state_dict(sd0 if sd is None else sd)
    return m.to(DEV)


def _kept_sets(m, B):
    """per stage, per image: the ORIGINAL token indices (CLS = 0 first) that left the stage"""
    out = []
    for cu, src in zip(m.cu_seqlens_per_stage, m.ragged_row_src_per_stage):
        cu, src = cu.cpu().tolist(), src.cpu().long()
        out.append([src[cu[b]:cu[b + 1]] for b in range(B)])
    return out


def _mode(ops, name):
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[name]


def _train_and_compare(name, m, sd, images, mode):
    """One training-mode forward and backward in `mode` against the float64 reference with the GPU's kept sets replayed.
    -> (token counts per stage, kept sets, the reference's gradients)"""
    from d2s import ops
    cfg = cases.MODEL_CASES[name]["cfg"]
    B = images.shape[0]
    W = torch.randn((B, cfg["num_classes"]), generator=torch.Generator().manual_seed(77))
    m.train()
    with ops.gemm_mode(_mode(ops, mode)):
        logits = m(images.to(DEV))
        assert logits.requires_grad and logits.shape == (B, cfg["num_classes"])
        counts = [c.cpu().tolist() for c in m.tokens_per_stage]
        kept = _kept_sets(m, B)
        assert len(m.ats_plans) == len(m.ats_locs) == len(m.ats_scores) == len(m.ats_masks) and m.ats_scores[0] is not None
        (logits * W.to(DEV)).sum().backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    ref_logits, _, ref_grads = T.model_grads(sd, images, cfg, m.ats_locs, kept, logit_weight=W)
    print(f"{name} locs {m.ats_locs} K {m.ats_tokens} {mode}: tokens per stage {counts}, "
          f"max |logits - ref| {float((logits.detach().cpu().double() - ref_logits).abs().max()):.3e}")
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits.numpy(), rtol=1e-4, atol=2e-5)
    for k, p in m.named_parameters():
        want = ref_grads[k]
        assert p.grad is not None and want is not None, k
        gf, wf = p.grad.detach().flatten().cpu(), want.flatten()
        np.testing.assert_allclose(float(gf.double().norm()), float(wf.norm()), rtol=1e-3, atol=1e-6, err_msg=k)
        h = min(8, gf.numel())
        np.testing.assert_allclose(gf[:h].numpy(), wf[:h].numpy(), rtol=5e-3, atol=5e-4 * float(wf[:h].abs().max()) + 2e-6, err_msg=k)
    return counts, kept, ref_grads


LAYOUTS = [([1, 2, 3], [12, 8, 4]), ([0], 8)]


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("locs,K", LAYOUTS, ids=str)
@pytest.mark.parametrize("name", ["micro1", "tiny32"])
def test_model_logits_and_gradients_against_float64(name, locs, K, mode):
    sd, images, _ = _models(name)
    m = _ats(name, ats_locs=locs, ats_tokens=K, train_sample=True)
    counts, kept, ref_grads = _train_and_compare(name, m, sd, images, mode)
    n = cases.MODEL_CASES[name]["cfg"]["n_patches"] + 1
    for s, k in enumerate(m.ats_tokens):
        assert all(1 <= c <= min(k, n - 1) for c in counts[s])
    # the embedding takes gradients, and a token the FIRST stage dropped (in as many images as possible) takes its position gradient
    # through that stage's keys and values only: the row of pos_embed's gradient against the reference's
    for k in ("pos_embed", "cls_token", "patch_embed.proj.weight", "patch_embed.proj.bias"):
        assert float(dict(m.named_parameters())[k].grad.abs().max()) > 0, k
    dropped = torch.zeros(n, dtype=torch.long)
    for ids in kept[0]:
        gone = torch.ones(n, dtype=torch.bool)
        gone[ids] = False
        dropped += gone.long()
    if int(dropped.max()) > 0:                                               # tiny32 keeps all 4 tokens when K >= 4
        t = int(torch.argmax(dropped))
        got, want = m.pos_embed.grad[0, t].cpu(), ref_grads["pos_embed"][0, t]
        print(f"  token {t}, dropped at the first stage in {int(dropped[t])} of {len(kept[0])} images: |pos_embed grad| {float(got.norm()):.3e} "
              f"(float64 {float(want.norm()):.3e})")
        assert float(want.norm()) > 0
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=5e-3, atol=5e-4 * float(want.abs().max()) + 2e-6)
    else:
        assert name == "tiny32"


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("name,locs,K", [("micro1", [0, 2], [8, 4]), ("tiny32", [0, 5], [3, 2])], ids=str)
def test_training_forward_is_the_eval_forward_when_every_block_is_ragged(name, locs, K, mode):
    from d2s import ops
    _, images, _ = _models(name)
    m = _ats(name, ats_locs=locs, ats_tokens=K, train_sample=True)
    x = images.to(DEV)
    with ops.gemm_mode(_mode(ops, mode)):
        m.train()
        logits = m(x)
        plans = list(m.ats_plans)
        cus = [c.clone() for c in m.cu_seqlens_per_stage]
        m.eval()
        want = m(x)
        torch.cuda.synchronize()
        assert torch.equal(logits.detach(), want)                            # every block is the one launch sequence
        for (k0, c0), (k1, c1) in zip(plans, m.ats_plans):
            assert torch.equal(k0, k1) and torch.equal(c0, c1)
        assert all(torch.equal(a, b) for a, b in zip(cus, m.cu_seqlens_per_stage))
        # plans= replays in training too, and under no_grad the training-mode forward keeps nothing and gives the same bits
        m.train()
        again = m(x, plans=plans)
        assert torch.equal(again.detach(), want) and m.ats_scores == [None] * len(locs)
        with torch.no_grad():
            assert torch.equal(m(x), want)


def test_a_truly_ragged_training_batch():
    """The batch tests/test_ats_train_cpu.py shows to be ragged for the float64 reference: the GPU's counts differ too, then logits and
    gradients against the reference with the GPU's kept sets."""
    sd, images, factor, ref_counts = ragged_case()
    assert len(set(ref_counts)) > 1
    m = _ats(RAGGED["name"], sd=sd, ats_locs=RAGGED["locs"], ats_tokens=RAGGED["K"], train_sample=True)
    counts, _, _ = _train_and_compare(RAGGED["name"], m, sd, images, "exact")
    print(f"factor {factor}: reference counts {ref_counts}, GPU counts {counts[-1]}")
    assert len(set(counts[-1])) > 1, counts                                 # the batch that reached the head was ragged


def test_default_construction_still_refuses_to_train():
    from vit_models import ats
    _, images, _ = _models("micro1")
    m = _ats("micro1", ats_locs=[1], ats_tokens=8).train()
    with pytest.raises(NotImplementedError) as e:
        m(images.to(DEV))
    assert str(e.value) == ats.ATS_TRAINING_ERROR


# ---- 4. train step ----
LOCS, TOKENS = [1, 2, 3], [12, 8, 4]


def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **kw)


def _step(with_teacher, student=None, **kw):
    import vit_models
    from d2s.engine import TrainStep
    sd, _, geom = _models("micro1")
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**geom)
        teacher.load_state_dict(sd)
        teacher = teacher.to(DEV)
    student = _ats("micro1", ats_locs=LOCS, ats_tokens=TOKENS, train_sample=True) if student is None else student
    return TrainStep(student, teacher, _args(), lr=1e-3, **kw)


@pytest.mark.parametrize("with_teacher", [False, True])
def test_train_step_loss_three_steps_and_checkpoint(with_teacher):
    from tests.tome_train_ref import tome_loss
    sd, images, geom = _models("micro1")
    case = cases.MODEL_CASES["micro1"]
    x, y = images.to(DEV), torch.from_numpy(cases.make_labels(case)).to(DEV)
    ts = _step(with_teacher)
    assert ts.method.name == "ats" and ts.logits_only and ts.graph is False and (ts._teacher_stream is None) == (not with_teacher)
    info = ts(x, y)
    torch.cuda.synchronize()
    kept = _kept_sets(ts.student, images.shape[0])                           # of the forward that made the loss (the weights have moved since)
    assert info["stepped"] and [c.cpu().tolist() for c in info["tokens_per_block"]] == [[len(i) - 1 for i in s] for s in kept]
    ref_t = R.model_forward(sd, images, case["cfg"], [])[0] if with_teacher else None
    _, want, _ = T.model_grads(sd, images, case["cfg"], LOCS, kept, loss_of=lambda ls: tome_loss(ls, ref_t, y.cpu(), 1.0, 0.5))
    print(f"train step (teacher: {with_teacher}): loss {float(info['loss']):.7f}, float64 {float(want):.7f}")
    np.testing.assert_allclose(float(info["loss"]), float(want), rtol=1e-4)
    losses = [float(info["loss"])]
    losses.append(float(ts(x, y)["loss"]))
    saved = ts.state_dict()
    losses.append(float(ts(x, y)["loss"]))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses), losses
    three = ts.arena.params.clone()
    cfg = saved["config"]
    assert (cfg["ats_locs"], cfg["ats_tokens"], cfg["train_sample"], cfg["model"]) == (LOCS, TOKENS, True, "VisionTransformerATS")
    # the student rebuilt from the checkpoint's config: 2 steps, a checkpoint, 1 more step = 3 straight steps
    rebuilt = _ats("micro1", ats_locs=cfg["ats_locs"], ats_tokens=cfg["ats_tokens"], train_sample=cfg["train_sample"])
    resumed = _step(with_teacher, student=rebuilt)
    assert resumed.load_state_dict(saved) == saved["epoch"]
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three)
    from d2s import lib
    other = _step(with_teacher, student=_ats("micro1", ats_locs=LOCS, ats_tokens=[12, 8, 5], train_sample=True))
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ats_tokens"):
        other.load_state_dict(saved)
    assert "train_tome_loss" in ts.metrics and float(ts.metrics["train_cls_loss"]) > 0


def test_train_step_refusals_by_message():
    from d2s import lib
    from d2s.engine import TrainStep
    m = _ats("micro1", ats_locs=LOCS, ats_tokens=TOKENS, train_sample=True)
    with pytest.raises(ValueError, match="warmup_steps 2 with an Adaptive Token Sampling student"):
        TrainStep(m, None, _args(), warmup_steps=2)
    with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an Adaptive Token Sampling student"):
        TrainStep(m, None, _args(), graph=True)
    with pytest.raises(lib.D2SError, match="needs train_sample=True"):
        TrainStep(_ats("micro1", ats_locs=LOCS, ats_tokens=TOKENS), None, _args())
    m.drop_path_rate = 0.1
    with pytest.raises(lib.D2SError, match="Adaptive Token Sampling student and drop_path_rate > 0"):
        TrainStep(m, None, _args())


# ---- 5. command line ----
def test_cli_trains_a_checkpoint_through_the_stages(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "ats", "--ats-train", "--pruning-locs", "3", "6", "9", "--ats-tokens", "8",
                               "--epochs", "1", "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--student-checkpoint", path,
                               "--teacher-checkpoint", path, "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Start training" in out and "--ats-train: ats tokens per stage: mean [" in out and " max [" in out and "val loss:" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert (cfg["ats_locs"], cfg["ats_tokens"], cfg["train_sample"]) == ([3, 6, 9], [8, 8, 8], True)
