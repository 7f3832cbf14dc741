"""Training through token merging on the GPU: d2s_attn_keyw_bwd_f32 and d2s_tome_merge_bwd against float64
(tests/tome_train_ref.py), their bit-exact special cases and refusals, ToMeBlockFn and the train_merge model against float64 with the
GPU's own plans replayed, the train step (loss, determinism, checkpoint, accumulation + clipping) and the command line.

Tolerances are the project's: the attention backward at tests/test_kernels_gpu.py's rule for the plain one (rtol 2e-4, atol 5e-5); a
scaled row of the merge backward within 3 * 2^-24 |ref| (one rounding for the weight, one for the product: 2u + u^2 < 3u), copied rows
bit-exact; the block at tests/test_droppath_gpu.py's rule with keep = 1 (y, dx: rtol 1e-4 / atol 2e-5; a parameter gradient's relative L2
error at most 4 x that of an fp32 CPU evaluation of the same restatement, floor 2e-4); model gradients at tests/test_model_gpu.py's rule
(norms rtol 1e-3 / atol 1e-6, leading elements rtol 5e-3)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import tome_ref as R
from tests import tome_train_ref as T
from tests.test_tome_gpu import _match, _models, _qkv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _mode(ops, name):
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[name]


# ---- 1. key-weighted attention backward ----
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n", [2, 31, 32, 33, 128, 129, 197])
def test_keyw_attention_backward_against_float64(n, H):
    from d2s import ops
    B = 2
    gen = torch.Generator().manual_seed(4000 + 10 * n + H)
    qkv = torch.randn((B, n, 3, H, 64), generator=gen)
    dout = torch.randn((B * n, H * 64), generator=gen)
    w = torch.randint(1, 9, (B, n), generator=gen).float()
    w[0, n // 3], w[1, n - 1] = float(max(n // 2, 1)), float(max(n // 2, 1))          # one heavy key per image
    qd, wd, dd = qkv.reshape(B * n, 3 * H * 64).to(DEV), w.to(DEV), dout.to(DEV)
    out, lse = ops.attn_keyw_fwd(qd, wd, B, n, H, 0.125, want_lse=True)
    dqkv = ops.attn_keyw_bwd(qd, wd, out, dd, lse, B, n, H, 0.125)
    again = ops.attn_keyw_bwd(qd, wd, out, dd, lse, B, n, H, 0.125)
    torch.cuda.synchronize()
    assert torch.equal(dqkv, again)                                                    # no atomics: two runs are bit-identical
    ref = T.keyw_attention_grad(qkv, w, 0.125, dout)
    got = dqkv.cpu().reshape(B, n, 3, H, 64)
    print(f"keyw bwd n={n} H={H}: max abs err {float((got.double() - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-4, atol=5e-5)
    # every weight 1.0, the plain forward's out / lse: the plain backward, bit for bit
    ones = torch.ones((B, n), device=DEV)
    out0, lse0, _ = ops.attn_fwd(qd, B, n, H, 0.125, want_cls=False)
    assert torch.equal(ops.attn_keyw_bwd(qd, ones, out0, dd, lse0, B, n, H, 0.125), ops.attn_bwd(qd, out0, dd, lse0, B, n, H, 0.125))


# ---- 2. merge backward ----
def _scaled_rows(plan, B, n):
    """[B, n] bool: the input rows that were averaged with others (sources, and B rows with sources)"""
    _, src, dst = (t.cpu().long() for t in plan)
    m = torch.zeros((B, n), dtype=torch.bool)
    for b in range(B):
        m[b, 2 * src[b]] = True
        m[b, 2 * dst[b] + 1] = True
    return m


def _check_merge_bwd(x, size, plan, n, r, seed):
    from d2s import ops
    B, _, D = x.shape
    xd = x.to(DEV).reshape(B * n, D).contiguous()
    sd = None if size is None else size.to(DEV)
    out, size_out = ops.tome_merge(xd, sd, *plan, B, n, D, r)
    dy = torch.randn((B, n - r, D), generator=torch.Generator().manual_seed(seed))
    dyd = dy.to(DEV).reshape(B * (n - r), D)
    dx = ops.tome_merge_bwd(dyd, sd, size_out, *plan, B, n, D, r)
    again = ops.tome_merge_bwd(dyd, sd, size_out, *plan, B, n, D, r)
    torch.cuda.synchronize()
    assert torch.equal(dx, again) and dx.shape == (B * n, D)
    ref = T.merge_backward(dy, size, size_out.cpu(), tuple(t.cpu() for t in plan))
    got = dx.cpu().double().reshape(B, n, D)
    scaled = _scaled_rows(plan, B, n)
    assert int(scaled.sum()) > 0 or r == 0
    err = (got - ref).abs()
    worst = float((err / (ref.abs() + 1e-300)).max())
    print(f"merge bwd n={n} r={r} D={D} sizes={'given' if size is not None else 'ones'}: worst relative error {worst / U:.3f} u (bound 3 u), "
          f"{int(scaled.sum())} scaled rows")
    assert bool((err <= 3 * U * ref.abs()).all())
    assert torch.equal(got[~scaled], ref[~scaled])                                     # copied rows: bit for bit
    # adjoint identity <dx, x> = <dy, merge(x)>, both sides from the kernels' outputs, summed in float64
    lhs, rhs = float((got * x.double()).sum()), float((dy.double() * out.cpu().double().reshape(B, n - r, D)).sum())
    print(f"  <dx, x> = {lhs:.9e}, <dy, merge(x)> = {rhs:.9e}")
    assert lhs == pytest.approx(rhs, rel=1e-5)
    return got, ref


@pytest.mark.parametrize("B,n,H,r,D", [(2, 3, 1, 1, 128), (2, 9, 3, 2, 192), (2, 10, 3, 4, 192), (3, 65, 3, 16, 384), (3, 66, 1, 32, 128),
                                       (2, 197, 6, 13, 384), (2, 197, 3, 98, 192)])
def test_merge_backward_against_float64_on_the_kernels_own_plans(B, n, H, r, D):
    gen = torch.Generator().manual_seed(1900 + n + r)
    plan = _match(_qkv(B, n, H), r)[2:]
    x = torch.randn((B, n, D), generator=gen)
    size = torch.randint(1, 8, (B, n), generator=gen).float()
    _check_merge_bwd(x, None, plan, n, r, seed=n)
    _check_merge_bwd(x, size, plan, n, r, seed=n + 1)


def test_merge_backward_identity_at_r0_many_sources_and_a_non_plan():
    from d2s import lib, ops
    gen = torch.Generator().manual_seed(131)
    B, n, D = 2, 21, 128
    x = torch.randn((B, n, D), generator=gen)
    size = torch.randint(1, 8, (B, n), generator=gen).float()
    i32 = dict(dtype=torch.int32, device=DEV)
    # r = 0: the inverse of "A rows in order, then B rows", bit for bit
    unm0 = torch.arange(11, **i32).expand(B, -1).contiguous()
    empty = torch.empty((B, 0), **i32)
    dy = torch.randn((B, n, D), generator=gen)
    for s in (None, size.to(DEV)):
        _, so = ops.tome_merge(x.to(DEV).reshape(B * n, D), s, unm0, empty, empty, B, n, D, 0)
        dx = ops.tome_merge_bwd(dy.to(DEV).reshape(B * n, D), s, so, unm0, empty, empty, B, n, D, 0).cpu().reshape(B, n, D)
        assert torch.equal(dx[:, 0::2], dy[:, :11]) and torch.equal(dx[:, 1::2], dy[:, 11:])
    # every one of the 10 non-CLS A rows lands on B row 4 (image 0) / B row 9 (image 1)
    unm = torch.zeros((B, 1), **i32)
    src = torch.arange(1, 11, **i32).expand(B, -1).contiguous()
    dst = torch.tensor([[4] * 10, [9] * 10], **i32)
    for s in (None, size):
        got, _ = _check_merge_bwd(x, s, (unm, src, dst), n, 10, seed=7)
        if s is None:                      # eleven rows share the destination's gradient, each with weight 1/11
            dy7 = torch.randn((B, 11, D), generator=torch.Generator().manual_seed(7))          # _check_merge_bwd's dy
            want = dy7.double()[0, 1 + 4] * float(np.float32(1.0) / np.float32(11.0))
            assert torch.equal(got[0, 2], got[0, 9]) and float((got[0, 2] - want).abs().max()) <= U * float(want.abs().max())
    # not a plan: A row 4 (token 8) of image 0 is in neither list, image 1's source points outside the image, its unm_idx holds wild values.
    # The raw entry, dx followed by a guard band: zeros where nothing is owed, nothing written past the end, everything finite.
    n, r = 9, 1
    unm = torch.tensor([[0, 1, 1, 3], [0, 1, 3, 1 << 30]], **i32)
    src = torch.tensor([[2], [2]], **i32)
    dst = torch.tensor([[1], [99]], **i32)
    dy = torch.randn((B, n - r, D), generator=gen).to(DEV)
    so = torch.full((B, n - r), 2.0, device=DEV)
    buf = torch.full((B * n * D + 4096,), 7.0, device=DEV)
    rc = lib._fn("d2s_tome_merge_bwd")(lib.ptr(dy), None, lib.ptr(so), lib.ptr(unm), lib.ptr(src), lib.ptr(dst), B, n, D, r, lib.ptr(buf), lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf[B * n * D:] == 7).all())
    dx = buf[:B * n * D].cpu().reshape(B, n, D)
    assert bool(torch.isfinite(dx).all()) and bool((dx != 7).any(dim=-1).all())          # every row was written
    assert bool((dx[0, 8] == 0).all()) and bool((dx[1, 4] == 0).all()) and bool((dx[1, 8] == 0).all())
    assert torch.equal(dx[0, 4], dy.cpu().reshape(B, n - r, D)[0, 4 + 1] * 0.5)             # image 0's source: half of B row 1's gradient
    assert torch.equal(dx[0, 0], dy.cpu().reshape(B, n - r, D)[0, 0])                       # CLS is copied


# ---- 3. refusals ----
def test_backward_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, n, H, D, r = 2, 9, 2, 128, 2
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    dy, size, so, dx = f(B * 900, D), f(B, 900), f(B, 900), f(B * 900, D)
    unm, src, dst = i(B, 450), i(B, 450), i(B, 450)
    qkv, out, dout, lse, dqkv, delta = f(B * 900, 3 * H * 64), f(B * 900, H * 64), f(B * 900, H * 64), f(B, H, 900), f(B * 900, 3 * H * 64), f(B, H, 900)
    p, s = lib.ptr, lib.stream()

    def mbwd(g=dy, z=so, c=unm, d=src, e=dst, B_=B, n_=n, D_=D, r_=r, o=dx):
        return lib._fn("d2s_tome_merge_bwd")(p(g), p(size), p(z), p(c), p(d), p(e), B_, n_, D_, r_, p(o), s)

    def kbwd(q=qkv, w=size, o=out, g=dout, l=lse, dq=dqkv, ws=delta, B_=B, n_=n, H_=H):
        return lib._fn("d2s_attn_keyw_bwd_f32")(p(q), p(w), p(o), p(g), p(l), p(dq), p(ws), B_, n_, H_, ctypes.c_float(0.125), s)

    bad = [mbwd(g=None), mbwd(z=None), mbwd(c=None), mbwd(d=None), mbwd(e=None), mbwd(o=None), mbwd(r_=-1), mbwd(r_=5), mbwd(n_=1),
           mbwd(D_=130), mbwd(D_=0), mbwd(n_=897), mbwd(B_=0),
           kbwd(q=None), kbwd(w=None), kbwd(o=None), kbwd(g=None), kbwd(l=None), kbwd(dq=None), kbwd(ws=None), kbwd(n_=1), kbwd(n_=0),
           kbwd(n_=8193), kbwd(B_=0), kbwd(H_=0)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    for t in (dx, dqkv, delta):                              # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())


# ---- 4. block ----
def _block_inputs(B, n, D, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hidden, D), (hidden,), (D, hidden), (D,)]
    p = [torch.randn(s, generator=g) * (0.05 if len(s) == 2 else 0.1) for s in shapes]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    return torch.randn(B, n, D, generator=g), p, g


def _run_tome_block(x, p, size, heads, r, gy_of):
    """-> (y, size_out, plan, [dx + 12 parameter gradients]) on the GPU; gy_of(rows) makes the output gradient"""
    from d2s import functional_tome as TF
    from d2s import ops
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in p]
    y, size_out, plan = TF.tome_block_train(xd, None if size is None else size.to(DEV), pd, heads, 1e-6, 64 ** -0.5, r)
    gy = gy_of(y.shape[1])
    grads = torch.autograd.grad(y, [xd] + pd, gy.to(DEV))
    ops.join_weight_grads()
    torch.cuda.synchronize()
    return y.detach().cpu(), size_out, plan, [t.cpu() for t in grads], gy


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("sizes", [False, True])
@pytest.mark.parametrize("n,r", [(17, 3), (18, 8)])
def test_block_forward_and_all_gradients_against_float64(n, r, sizes, mode):
    from d2s import ops
    B, D, H, hid = 2, 128, 2, 512
    x, p, g = _block_inputs(B, n, D, hid, seed=n)
    size = torch.randint(1, 5, (B, n), generator=g).float() if sizes else None
    gy_of = lambda rows: torch.randn(B, rows, D, generator=torch.Generator().manual_seed(99))
    with ops.gemm_mode(_mode(ops, mode)):
        y, size_out, plan, grads, gy = _run_tome_block(x, p, size, H, r, gy_of)
    assert y.shape == (B, n - r, D) and size_out.shape == (B, n - r) and plan[1].shape == (B, r)
    plan = tuple(t.cpu() for t in plan)
    yr, dxr, dpr = T.block_with_grads(x, p, H, 1e-6, size, plan, gy)
    assert torch.equal(size_out.cpu().double(), T.merge(x.double(), size, plan)[1])
    np.testing.assert_allclose(y.numpy(), yr.float().numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(grads[0].numpy(), dxr.float().numpy(), rtol=1e-4, atol=2e-5)
    _, _, cpu = T.block_with_grads(x, p, H, 1e-6, size, plan, gy, dtype=torch.float32)      # the yardstick's own rounding error
    for name, got, want, c in zip(T.PARAM_NAMES, grads[1:], dpr, cpu):
        denom = float(want.norm())
        err = float((got.double() - want).norm()) / denom
        err_cpu = float((c.double() - want).norm()) / denom
        print(f"tome block n={n} r={r} sizes={sizes} {mode} d{name}: relative L2 error {err:.3e} (fp32 CPU {err_cpu:.3e})")
        assert err <= max(4.0 * err_cpu, 2e-4), (name, err, err_cpu)


@pytest.mark.parametrize("mode", ["exact", "split"])
def test_block_without_merging_is_the_dense_block_bit_for_bit(mode):
    from d2s import functional as DF
    from d2s import ops
    B, n, D, H, hid = 2, 17, 128, 2, 512
    x, p, _ = _block_inputs(B, n, D, hid, seed=5)
    gy_of = lambda rows: torch.randn(B, rows, D, generator=torch.Generator().manual_seed(98))
    with ops.gemm_mode(_mode(ops, mode)):
        y, size_out, plan, grads, gy = _run_tome_block(x, p, None, H, 0, gy_of)
        assert size_out is None and plan is None
        ops._BLOCK_COMPOSITE = False                    # BlockFn's per-op path
        try:
            xd = x.to(DEV).requires_grad_(True)
            pd = [t.to(DEV).requires_grad_(True) for t in p]
            yb, _ = DF.run(DF.BlockFn, xd, *pd, H, 1e-6, False, None)
            gb = torch.autograd.grad(yb, [xd] + pd, gy.to(DEV))
            ops.join_weight_grads()
            torch.cuda.synchronize()
        finally:
            ops._BLOCK_COMPOSITE = True
    assert torch.equal(y, yb.detach().cpu())
    for i, (a, b) in enumerate(zip(grads, gb)):
        assert torch.equal(a, b.cpu()), i


# ---- 5. model ----
def _tome_train(name, **kw):
    import vit_models
    _, sd, _, geom = _models(name)
    m = vit_models.VisionTransformerToMe(**geom, train_merge=True, **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.mark.parametrize("name,r,prop,counts", [("micro1", 2, True, [15, 13, 11, 9]), ("tiny32", 2, True, [3] + [2] * 11),
                                                ("micro1", [0, 3, 0, 8], False, [17, 14, 14, 8])])
def test_model_trains_through_the_merges(name, r, prop, counts):
    from d2s import ops
    _, sd, images, _ = _models(name)
    m = _tome_train(name, tome_r=r, prop_attn=prop).train()
    logits = m(images.to(DEV))
    assert m.tokens_per_block == counts and logits.requires_grad
    plans = list(m.tome_plans)
    logits.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    # the training-mode forward is the eval forward: same plans replayed, same bits, in both directions
    m.eval()
    assert torch.equal(m(images.to(DEV), plans=plans), logits.detach())
    m.train()
    assert torch.equal(m(images.to(DEV), plans=plans).detach(), logits.detach())
    cpu_plans = [None if p is None else tuple(t.cpu() for t in p) for p in plans]
    ref_logits, ref_grads = T.model_grads(sd, images, r, cpu_plans, prop_attn=prop)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits.numpy(), rtol=1e-4, atol=2e-5)
    for k, p in m.named_parameters():
        want = ref_grads[k]
        assert p.grad is not None and want is not None, k
        gf, wf = p.grad.detach().flatten().cpu(), want.flatten()
        np.testing.assert_allclose(float(gf.double().norm()), float(wf.norm()), rtol=1e-3, atol=1e-6, err_msg=k)
        h = min(8, gf.numel())
        np.testing.assert_allclose(gf[:h].numpy(), wf[:h].numpy(), rtol=5e-3, atol=5e-4 * float(wf[:h].abs().max()) + 2e-6, err_msg=k)


# ---- 6. train step ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **kw)


def _step(with_teacher, **kw):
    import vit_models
    from d2s.engine import TrainStep
    _, sd, _, geom = _models("micro1")
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**geom)
        teacher.load_state_dict(sd)
        teacher = teacher.to(DEV)
    return TrainStep(_tome_train("micro1", tome_r=2), teacher, _args(), lr=1e-3, **kw)


def _batch():
    case = cases.MODEL_CASES["micro1"]
    return torch.from_numpy(cases.make_images(case)).to(DEV), torch.from_numpy(cases.make_labels(case)).to(DEV)


@pytest.mark.parametrize("with_teacher", [False, True])
def test_train_step_loss_determinism_and_checkpoint(with_teacher):
    _, sd, images, _ = _models("micro1")
    x, y = _batch()
    ts = _step(with_teacher)
    assert ts.method.name == "tome" and ts.graph is False and (ts._teacher_stream is None) == (not with_teacher)
    info = ts(x, y)
    torch.cuda.synchronize()
    assert info["stepped"] and info["tokens_per_block"] == [15, 13, 11, 9]
    plans = [tuple(t.cpu() for t in p) for p in ts.student.tome_plans]
    # the first step's loss: the float64 restatement on the plans of that step (the weights have moved since; the plans were read first
    # from the forward that made them - a second forward of the updated student would match anew)
    ref_s = R.model_forward(sd, images, 2, plans=plans)[0]
    ref_t = R.model_forward(sd, images, 0)[0] if with_teacher else None
    want = float(T.tome_loss(ref_s, ref_t, y.cpu(), 1.0, 0.5))
    print(f"train step (teacher: {with_teacher}): loss {float(info['loss']):.7f}, float64 {want:.7f}")
    np.testing.assert_allclose(float(info["loss"]), want, rtol=1e-4)
    cfg = ts.config()
    assert cfg["tome_r"] == [2, 2, 2, 2] and cfg["prop_attn"] is True and cfg["train_merge"] is True
    ts(x, y)
    saved = ts.state_dict()
    ts(x, y)
    torch.cuda.synchronize()
    three = ts.arena.params.clone()
    again = _step(with_teacher)                          # two runs of 3 steps are bit-identical
    for _ in range(3):
        again(x, y)
    assert torch.equal(again.arena.params, three)
    resumed = _step(with_teacher)                        # 2 steps, a checkpoint, 1 more step = 3 straight steps
    resumed.load_state_dict(saved)
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three)
    assert "train_tome_loss" in ts.metrics and float(ts.metrics["train_cls_loss"]) > 0


def test_train_step_accumulates_and_clips():
    x, y = _batch()
    ts = _step(False, accum_steps=2, clip_grad=1.0)
    before = ts.arena.params.clone()
    a = ts(x, y)
    assert not a["stepped"] and torch.equal(ts.arena.params, before)
    b = ts(x, y)
    torch.cuda.synchronize()
    assert b["stepped"] and not torch.equal(ts.arena.params, before)
    assert bool(torch.isfinite(ts.last_clip).all()) and float(ts.last_clip[0]) > 0


# ---- 7. command line ----
def test_cli_trains_a_checkpoint_through_the_merges(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "tome", "--tome-train", "--tome-r", "2", "--epochs", "1", "--steps-per-epoch", "2",
                               "--val-steps", "1", "--batch-size", "4", "--dist-weight", "0", "--student-checkpoint", path])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Start training" in out and "--tome-train: tokens per block [195, 193," in out and "val loss:" in out
