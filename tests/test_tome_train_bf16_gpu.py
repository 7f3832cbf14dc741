"""Training through token merging in the bf16 arithmetic mode on the GPU (train_bf16=True / --tome-train-bf16):
d2s_attn_keyw_bwd_bf16 against float64 inside the bounds of tests/tome_train_bf16_cases.py and its bit-exact contracts,
d2s_tome_merge_bwd_bf16out against d2s_tome_merge_bwd, both entries' refusals, ToMeBlockFn with its bf16 input, the train_bf16 model, the
train step and the command line.

Where a float64 comparison has no derived bound (the block, the model, the step's loss) the bar is measured in the same test: the existing
dense path in the bf16 mode against the same float64 restatement, doubled - the roundings are the same per element and the merge adds one
bf16 rounding of the residual gradient that the dense block also has.  Every such test prints its figures before it asserts; DESIGN.md
section 22 records them.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import tome_bf16_cases as C
from tests import tome_ref as R
from tests import tome_train_bf16_cases as TC
from tests import tome_train_ref as T
from tests.test_tome_gpu import _match, _models, _qkv
from tests.test_tome_train_gpu import _block_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCALE = C.SCALE
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)
GUARD = 4096


# ---- 1. the key-weighted backward ----
@pytest.mark.parametrize("n,H", TC.SHAPES)
def test_weighted_backward_against_float64_and_its_contracts(n, H):
    """Observed worst error / bound over the 14 shapes on an MI355X: see DESIGN.md section 22 ("Training on the bf16 data path")."""
    from d2s import lib, ops
    case, B = C.keyw_case(n, H), C.KEYW_B
    qkv = case["qkv"].reshape(B * n, 3 * H * 64).contiguous().to(DEV)
    w, dout = case["w"].to(DEV), TC.dout_of(n, H).reshape(B * n, H * 64).to(DEV)
    out, lse, _ = ops.attn_keyw_fwd_bf16io(qkv, w, B, n, H, SCALE)
    # the raw entry, each output followed by a guard band
    numel = qkv.numel()
    buf, buf16 = torch.full((numel + GUARD,), 7.0, device=DEV), torch.full((numel + GUARD,), 7.0, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty((B, H, n), device=DEV)
    lib.call("d2s_attn_keyw_bwd_bf16", lib.ptr(qkv), 0, lib.ptr(w), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(buf), lib.ptr(buf16),
             lib.ptr(delta), B, n, H, SCALE)
    torch.cuda.synchronize()
    assert bool((buf[numel:] == 7).all()) and bool((buf16[numel:] == 7).all())           # nothing written past either output
    dqkv, dqkv16 = buf[:numel].view(B * n, -1), buf16[:numel].view(B * n, -1)
    fr = TC.fractions(TC.split_dqkv(dqkv.cpu(), n, H), TC.reference(n, H))
    print(f"keyw backward bf16 n {n} H {H}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert bool(torch.isfinite(dqkv).all())
    assert torch.equal(dqkv16, dqkv.bfloat16())                                           # (b)
    h16 = torch.empty_like(qkv, dtype=torch.bfloat16)
    from_bf16 = ops.attn_keyw_bwd_bf16io(qkv.bfloat16(), w, out, dout, lse, B, n, H, SCALE, dqkv16=h16)
    assert torch.equal(from_bf16, dqkv) and torch.equal(h16, dqkv16), "fp32 and bf16 qkv differ"       # (c)
    h16b = torch.empty_like(h16)
    again = ops.attn_keyw_bwd_bf16io(qkv, w, out, dout, lse, B, n, H, SCALE, dqkv16=h16b)
    assert torch.equal(again, dqkv) and torch.equal(h16b, dqkv16), "two runs differ"      # (d)
    only16 = torch.empty_like(h16)
    assert ops.attn_keyw_bwd_bf16io(qkv, w, out, dout, lse, B, n, H, SCALE, dqkv16=only16, want_f32=False) is None
    assert torch.equal(only16, dqkv16)                                                    # the bf16-only form
    assert torch.equal(ops.attn_keyw_bwd_bf16io(qkv, w, out, dout, lse, B, n, H, SCALE), dqkv)      # the fp32-only form
    for k, v in fr.items():
        assert v <= 1.0, (k, n, H, v)


@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("n", [2, 17, 33, 65, 129, 197])
def test_unit_weights_are_the_dense_bf16_backward_bit_for_bit(n, H):
    """contract (a): every weight 1.0 and the plain forward's out and lse - whichever tile form wrote them; the backward has 32-key tiles only"""
    from d2s import ops
    B = 3
    gen = torch.Generator().manual_seed(300 + n + H)
    qkv = torch.randn((B * n, 3 * H * 64), generator=gen).bfloat16().float().to(DEV)
    dout = torch.randn((B * n, H * 64), generator=gen).to(DEV)
    ones = torch.ones((B, n), device=DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        for src in (qkv, qkv.bfloat16()):
            out, lse, _, _ = ops.attn_fwd_bf16io(src, B, n, H, SCALE, want_cls=False)
            a16, b16 = torch.empty_like(qkv, dtype=torch.bfloat16), torch.empty_like(qkv, dtype=torch.bfloat16)
            want = ops.attn_bwd(src, out, dout, lse, B, n, H, SCALE, dqkv16=a16)
            got = ops.attn_keyw_bwd_bf16io(src, ones, out, dout, lse, B, n, H, SCALE, dqkv16=b16)
            torch.cuda.synchronize()
            assert torch.equal(got, want) and torch.equal(b16, a16), (n, H, src.dtype)


# ---- 2. the merge backward with its bf16 output ----
def _both_merge_bwd(dy, size, size_out, plan, B, n, D, r):
    from d2s import ops
    want = ops.tome_merge_bwd(dy, size, size_out, *plan, B, n, D, r)
    dx16 = torch.full((B * n, D), 7.0, dtype=torch.bfloat16, device=DEV)
    got = ops.tome_merge_bwd(dy, size, size_out, *plan, B, n, D, r, dx16=dx16)
    torch.cuda.synchronize()
    return got, dx16, want


@pytest.mark.parametrize("B,n,H,r,D", [(2, 3, 1, 1, 128), (2, 9, 3, 2, 192), (2, 10, 3, 4, 192), (3, 65, 3, 16, 384), (3, 66, 1, 32, 128),
                                       (2, 197, 6, 13, 384), (2, 197, 3, 98, 192)])
def test_merge_backward_bf16out_is_the_fp32_entry_and_its_rounding(B, n, H, r, D):
    """contract (e) on tests/test_tome_train_gpu.py's plan shapes, with and without sizes"""
    from d2s import ops
    gen = torch.Generator().manual_seed(2900 + n + r)
    plan = _match(_qkv(B, n, H), r)[2:]
    x = torch.randn((B * n, D), generator=gen).to(DEV)
    dy = torch.randn((B * (n - r), D), generator=gen).to(DEV)
    for size in (None, torch.randint(1, 8, (B, n), generator=gen).float().to(DEV)):
        _, size_out = ops.tome_merge(x, size, *plan, B, n, D, r)
        got, dx16, want = _both_merge_bwd(dy, size, size_out, plan, B, n, D, r)
        assert torch.equal(got, want) and torch.equal(dx16, want.bfloat16())
        again = _both_merge_bwd(dy, size, size_out, plan, B, n, D, r)
        assert torch.equal(again[0], got) and torch.equal(again[1], dx16)


def test_merge_backward_bf16out_at_r0_and_on_a_non_plan():
    from d2s import lib, ops
    gen = torch.Generator().manual_seed(231)
    B, n, D = 2, 21, 128
    i32 = dict(dtype=torch.int32, device=DEV)
    unm0 = torch.arange(11, **i32).expand(B, -1).contiguous()
    empty = torch.empty((B, 0), **i32)
    dy = torch.randn((B, n, D), generator=gen)
    x = torch.randn((B * n, D), generator=gen).to(DEV)
    for s in (None, torch.randint(1, 8, (B, n), generator=gen).float().to(DEV)):      # r = 0: the copy plus its rounding
        _, so = ops.tome_merge(x, s, unm0, empty, empty, B, n, D, 0)
        got, dx16, want = _both_merge_bwd(dy.to(DEV).reshape(B * n, D), s, so, (unm0, empty, empty), B, n, D, 0)
        dx = got.cpu().reshape(B, n, D)
        assert torch.equal(got, want) and torch.equal(dx[:, 0::2], dy[:, :11]) and torch.equal(dx[:, 1::2], dy[:, 11:])
        assert torch.equal(dx16, got.bfloat16())
    # tests/test_tome_train_gpu.py's hand-made non-plan through the raw entry, both outputs followed by a guard band: zero rows in both forms
    n, r = 9, 1
    unm = torch.tensor([[0, 1, 1, 3], [0, 1, 3, 1 << 30]], **i32)
    src = torch.tensor([[2], [2]], **i32)
    dst = torch.tensor([[1], [99]], **i32)
    dyd = torch.randn((B, n - r, D), generator=gen).to(DEV)
    so = torch.full((B, n - r), 2.0, device=DEV)
    numel = B * n * D
    buf, buf16 = torch.full((numel + GUARD,), 7.0, device=DEV), torch.full((numel + GUARD,), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib._fn("d2s_tome_merge_bwd_bf16out")(lib.ptr(dyd), None, lib.ptr(so), lib.ptr(unm), lib.ptr(src), lib.ptr(dst), B, n, D, r,
                                                lib.ptr(buf), lib.ptr(buf16), lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf[numel:] == 7).all()) and bool((buf16[numel:] == 7).all())
    want = ops.tome_merge_bwd(dyd.view(B * (n - r), D), None, so, unm, src, dst, B, n, D, r)
    dx, dx16 = buf[:numel].view(B, n, D), buf16[:numel].view(B, n, D)
    assert torch.equal(dx.view(B * n, D), want) and torch.equal(dx16, dx.bfloat16()) and bool(torch.isfinite(dx).all())
    for b, t in ((0, 8), (1, 4), (1, 8)):
        assert bool((dx[b, t] == 0).all()) and bool((dx16[b, t] == 0).all())


# ---- 3. refusals ----
def test_both_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, n, H, D, r = 2, 9, 2, 128, 2
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    h = lambda *shape: torch.full(shape, 7.0, dtype=torch.bfloat16, device=DEV)
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    dy, size, so, dx, dx16 = f(B * 900, D), f(B, 900), f(B, 900), f(B * 900, D), h(B * 900, D)
    unm, src, dst = i(B, 450), i(B, 450), i(B, 450)
    qkv, qkv16, out, dout = f(B * n, 3 * H * 64), h(B * n, 3 * H * 64), f(B * n, H * 64), f(B * n, H * 64)
    lse, dqkv, dqkv16, delta = f(B, H, n), f(B * n, 3 * H * 64), h(B * n, 3 * H * 64), f(B, H, n)
    p, s = lib.ptr, lib.stream()

    def mbwd(g=dy, z=so, c=unm, d=src, e=dst, B_=B, n_=n, D_=D, r_=r, o=dx, o16=dx16):
        return lib._fn("d2s_tome_merge_bwd_bf16out")(p(g), p(size), p(z), p(c), p(d), p(e), B_, n_, D_, r_, p(o), p(o16), s)

    def kbwd(q=qkv, is16=0, w=size, o=out, g=dout, l=lse, dq=dqkv, dq16=dqkv16, ws=delta, B_=B, n_=n, H_=H):
        return lib._fn("d2s_attn_keyw_bwd_bf16")(p(q), is16, p(w), p(o), p(g), p(l), p(dq), p(dq16), p(ws), B_, n_, H_, ctypes.c_float(SCALE), s)

    bad = [mbwd(g=None), mbwd(z=None), mbwd(c=None), mbwd(d=None), mbwd(e=None), mbwd(o=None), mbwd(o16=None), mbwd(r_=-1), mbwd(r_=5),
           mbwd(n_=1), mbwd(D_=130), mbwd(D_=0), mbwd(n_=897), mbwd(B_=0),
           kbwd(q=None), kbwd(w=None), kbwd(o=None), kbwd(g=None), kbwd(l=None), kbwd(dq=None, dq16=None), kbwd(ws=None), kbwd(n_=1),
           kbwd(n_=0), kbwd(n_=-3), kbwd(n_=8193), kbwd(B_=0), kbwd(B_=-1), kbwd(H_=0), kbwd(H_=-2), kbwd(q=qkv16, is16=1, n_=1)]
    torch.cuda.synchronize()
    assert bad == [ERR_ARG] * len(bad), bad
    for t in (dx, dx16, dqkv, dqkv16, delta):                # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    with pytest.raises(lib.D2SError):                        # lib.call serves the new table and raises on the code
        lib.call("d2s_attn_keyw_bwd_bf16", p(qkv), 0, p(size), p(out), p(dout), p(lse), None, None, p(delta), B, n, H, SCALE)
    # the limits themselves are accepted (benign values: weights, sizes and the log-sum-exp of 7, a plan of in-range indices)
    unm.fill_(0), src.fill_(1), dst.fill_(0)
    assert kbwd() == 0 and kbwd(dq=None) == 0 and kbwd(dq16=None) == 0 and kbwd(n_=2) == 0 and kbwd(q=qkv16, is16=1) == 0
    assert mbwd(r_=4) == 0 and mbwd(r_=0, d=None, e=None) == 0 and mbwd(n_=896, r_=0) == 0 and mbwd(n_=2, r_=0) == 0
    torch.cuda.synchronize()


# ---- 4. the block ----
B_, D_, H_, HID = 2, 128, 2, 512
NAMES = ("y", "dx") + tuple("d" + k for k in T.PARAM_NAMES)


def _gy_of(seed):
    return lambda rows: torch.randn(B_, rows, D_, generator=torch.Generator().manual_seed(seed))


def _run_tome(x, p, size, r, gy_of, bf16=True):
    from d2s import functional_tome as TF
    from d2s import ops
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in p]
    y, size_out, plan = TF.tome_block_train(xd, None if size is None else size.to(DEV), pd, H_, 1e-6, SCALE, r, bf16=bf16)
    gy = gy_of(y.shape[1])
    grads = torch.autograd.grad(y, [xd] + pd, gy.to(DEV))
    ops.join_weight_grads()
    torch.cuda.synchronize()
    return y.detach().cpu(), size_out, plan, [t.cpu() for t in grads], gy


def _run_dense(x, p, gy):
    from d2s import functional as DF
    from d2s import ops
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in p]
    y, _ = DF.run(DF.BlockFn, xd, *pd, H_, 1e-6, False, None)
    grads = torch.autograd.grad(y, [xd] + pd, gy.to(DEV))
    ops.join_weight_grads()
    torch.cuda.synchronize()
    return y.detach().cpu(), [t.cpu() for t in grads]


def _rel_l2(got, want):
    return [float((g.double() - w).norm()) / float(w.norm()) for g, w in zip(got, want)]


_DENSE = {}


def _dense_yardstick():
    """relative-L2 errors of the dense BlockFn in the bf16 mode against float64 at n = 17 and 18: {n: [y, dx, 12 parameters]}"""
    from d2s import ops
    if not _DENSE:
        for n in (17, 18):
            x, p, _ = _block_inputs(B_, n, D_, HID, seed=n)
            gy = _gy_of(99)(n)
            with ops.gemm_mode(ops.GEMM_BF16):
                y, grads = _run_dense(x, p, gy)
            yr, dxr, dpr = T.block_with_grads(x, p, H_, 1e-6, None, None, gy)
            _DENSE[n] = _rel_l2([y] + grads, [yr, dxr] + list(dpr))
            print(f"dense block bf16 n={n}: relative L2 error " + " ".join(f"{k} {v:.2e}" for k, v in zip(NAMES, _DENSE[n])))
    return _DENSE


@pytest.mark.parametrize("n", [17, 33])
def test_block_without_merging_is_the_dense_bf16_block_bit_for_bit(n):
    """r = 0 and no sizes: y and all 13 gradients are BlockFn's bits in the bf16 mode; 33 is where the dense forward takes 64-key tiles"""
    from d2s import ops
    x, p, _ = _block_inputs(B_, n, D_, HID, seed=5)
    with ops.gemm_mode(ops.GEMM_BF16):
        y, size_out, plan, grads, gy = _run_tome(x, p, None, 0, _gy_of(98))
        assert size_out is None and plan is None
        yb, gb = _run_dense(x, p, gy)
    assert torch.equal(y, yb)
    for i, (a, b) in enumerate(zip(grads, gb)):
        assert torch.equal(a, b), NAMES[1 + i]


@pytest.mark.parametrize("sizes", [False, True])
@pytest.mark.parametrize("n,r", [(17, 3), (18, 8)])
def test_block_forward_and_all_gradients_against_float64(n, r, sizes):
    """Observed on an MI355X: see DESIGN.md section 22 ("Training on the bf16 data path")."""
    from d2s import ops
    bar = 2.0 * max(max(v) for v in _dense_yardstick().values())
    x, p, g = _block_inputs(B_, n, D_, HID, seed=n)
    size = torch.randint(1, 5, (B_, n), generator=g).float() if sizes else None
    with ops.gemm_mode(ops.GEMM_BF16):
        y, size_out, plan, grads, gy = _run_tome(x, p, size, r, _gy_of(99))
    assert y.shape == (B_, n - r, D_) and size_out.shape == (B_, n - r) and plan[1].shape == (B_, r)
    plan = tuple(t.cpu() for t in plan)
    yr, dxr, dpr = T.block_with_grads(x, p, H_, 1e-6, size, plan, gy)
    assert torch.equal(size_out.cpu().double(), T.merge(x.double(), size, plan)[1])
    errs = _rel_l2([y] + grads, [yr, dxr] + list(dpr))
    print(f"tome block bf16 n={n} r={r} sizes={sizes}: relative L2 error " + " ".join(f"{k} {v:.2e}" for k, v in zip(NAMES, errs))
          + f" | bar {bar:.2e}")
    for name, e in zip(NAMES, errs):
        assert e <= bar, (name, e, bar)


def test_block_refuses_the_flag_outside_the_bf16_data_path_and_the_mode_without_the_flag():
    from d2s import functional_tome as TF
    from d2s import lib, ops
    x, p, _ = _block_inputs(B_, 17, D_, HID, seed=5)
    xd, pd = x.to(DEV).requires_grad_(True), [t.to(DEV) for t in p]
    with ops.gemm_mode(ops.GEMM_EXACT):
        with pytest.raises(lib.D2SError) as e:
            TF.tome_block_train(xd, None, pd, H_, 1e-6, SCALE, 3, bf16=True)
    assert str(e.value) == TF._BF16_MODE_NEEDED
    odd = [t.to(DEV) for t in _block_inputs(B_, 17, D_, 520, seed=5)[1]]             # hidden = 520: no multiple of 32
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            TF.tome_block_train(xd, None, odd, H_, 1e-6, SCALE, 3, bf16=True)
        assert str(e.value) == TF._BF16_PATH_NEEDED
        with pytest.raises(lib.D2SError) as e:
            TF.tome_block_train(xd, None, pd, H_, 1e-6, SCALE, 3)
        assert str(e.value) == TF._BF16_REFUSAL


def test_bf16_gradient_forms_are_handed_from_block_to_block():
    """two stacked merging blocks: the second block's input gradient arrives at the first with its bf16 shadow (ops.shadow_hits grows)"""
    from d2s import functional_tome as TF
    from d2s import ops
    x, p, g = _block_inputs(B_, 18, D_, HID, seed=7)
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in p]
    with ops.gemm_mode(ops.GEMM_BF16):
        y, size, _ = TF.tome_block_train(xd, None, pd, H_, 1e-6, SCALE, 3, bf16=True)
        y, size, _ = TF.tome_block_train(y, size, pd, H_, 1e-6, SCALE, 3, bf16=True)
        before = ops.shadow_hits
        y.sum().backward()
        ops.join_weight_grads()
    torch.cuda.synchronize()
    assert y.shape == (B_, 12, D_) and ops.shadow_hits > before and bool(torch.isfinite(xd.grad).all())


# ---- 5. the model ----
def _tome_train(name, **kw):
    import vit_models
    _, sd, _, geom = _models(name)
    m = vit_models.VisionTransformerToMe(**geom, train_merge=True, train_bf16=True, **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


_DENSE_MODEL = {}


def _dense_model_yardstick(name):
    """relative-L2 gradient errors of the trunk without merging (tome_r = 0) in the bf16 mode against float64, per parameter; once per case"""
    from d2s import ops
    if name not in _DENSE_MODEL:
        _, sd, images, geom = _models(name)
        with ops.gemm_mode(ops.GEMM_BF16):
            dense = _tome_train(name, tome_r=0).train()
            dense(images.to(DEV)).sum().backward()
            ops.join_weight_grads()
            torch.cuda.synchronize()
        _DENSE_MODEL[name] = _grad_errors(dense, T.model_grads(sd, images, 0, [None] * geom["depth"])[1])
    return _DENSE_MODEL[name]


def _grad_errors(m, ref_grads):
    out = {}
    for k, p in m.named_parameters():
        want = ref_grads[k]
        assert p.grad is not None and want is not None, k
        out[k] = float((p.grad.detach().cpu().double() - want).norm()) / float(want.norm())
    return out


@pytest.mark.parametrize("name,r,prop", [("micro1", 2, True), ("tiny32", 2, True), ("micro1", [0, 3, 0, 8], False)])
def test_model_trains_through_the_merges_in_bf16(name, r, prop):
    """Observed on an MI355X: see DESIGN.md section 22 ("Training on the bf16 data path")."""
    import vit_models
    from d2s import ops
    _, sd, images, geom = _models(name)
    yard = _dense_model_yardstick(name)                             # the same trunk without merging, in the bf16 mode
    with ops.gemm_mode(ops.GEMM_BF16):
        m = _tome_train(name, tome_r=r, prop_attn=prop).train()
        logits = m(images.to(DEV))
        plans = list(m.tome_plans)
        counts = list(m.tokens_per_block)
        logits.sum().backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        # the training-mode forward is the bf16 eval forward: same plans replayed, same bits
        m.eval()
        assert torch.equal(m(images.to(DEV), plans=plans), logits.detach())
        assert ops.get_gemm_mode() == ops.GEMM_BF16
    inference = vit_models.VisionTransformerToMe(**geom, tome_r=r, prop_attn=prop, bf16=True)
    inference.load_state_dict(sd)
    assert torch.equal(inference.to(DEV).eval()(images.to(DEV), plans=plans), logits.detach())      # the bf16=True route, from the exact mode
    with ops.gemm_mode(ops.GEMM_EXACT):                            # under an fp32 mode the keyword changes nothing
        fp32 = m.train()(images.to(DEV), plans=plans)
        plain = vit_models.VisionTransformerToMe(**geom, tome_r=r, prop_attn=prop, train_merge=True)
        plain.load_state_dict(sd)
        assert torch.equal(plain.to(DEV).train()(images.to(DEV), plans=plans), fp32)
    cpu_plans = [None if p is None else tuple(t.cpu() for t in p) for p in plans]
    ref_logits, ref_grads = T.model_grads(sd, images, r, cpu_plans, prop_attn=prop)
    assert R.model_forward(sd, images, r, plans=cpu_plans, prop_attn=prop)[1] == counts
    m.train()
    errs = _grad_errors(m, ref_grads)
    bar = 2.0 * max(yard.values())
    worst = max(errs, key=errs.get)
    print(f"bf16 merging model {name} r {r} prop_attn {prop}: max abs logit error {float((logits.detach().cpu().double() - ref_logits).abs().max()):.3e}; "
          f"worst relative L2 gradient error {errs[worst]:.3e} ({worst}); dense r = 0 worst {max(yard.values()):.3e} "
          f"({max(yard, key=yard.get)}), bar {bar:.3e}")
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits.float().numpy(), rtol=3e-2, atol=3e-2)      # the inference tier's rule
    for k, e in errs.items():
        assert e <= bar, (k, e, bar)


# ---- 6. the train step ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **kw)


def _step(with_teacher, r=2, train_bf16=True, **kw):
    import vit_models
    from d2s.engine import TrainStep
    _, sd, _, geom = _models("micro1")
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**geom)
        teacher.load_state_dict(sd)
        teacher = teacher.to(DEV)
    student = vit_models.VisionTransformerToMe(**geom, train_merge=True, tome_r=r, **({"train_bf16": True} if train_bf16 else {}))
    student.load_state_dict(sd)
    return TrainStep(student.to(DEV), teacher, _args(), lr=1e-3, **kw)


def _batch():
    case = cases.MODEL_CASES["micro1"]
    return torch.from_numpy(cases.make_images(case)).to(DEV), torch.from_numpy(cases.make_labels(case)).to(DEV)


@pytest.mark.parametrize("with_teacher", [False, True])
def test_train_step_loss_determinism_and_checkpoint(with_teacher):
    """Observed on an MI355X: see DESIGN.md section 22 ("Training on the bf16 data path")."""
    from d2s import lib, ops
    _, sd, images, _ = _models("micro1")
    x, y = _batch()
    ref_t = R.model_forward(sd, images, 0)[0] if with_teacher else None
    with ops.gemm_mode(ops.GEMM_BF16):
        # the yardstick: the dense (r = 0) bf16 step's first loss against float64
        dense_loss = float(_step(with_teacher, r=0)(x, y)["loss"])
        dense_dev = abs(dense_loss - float(T.tome_loss(R.model_forward(sd, images, 0)[0], ref_t, y.cpu(), 1.0, 0.5)))
        ts = _step(with_teacher)
        assert ts.method.name == "tome" and ts.graph is False
        info = ts(x, y)
        torch.cuda.synchronize()
        assert info["stepped"] and info["tokens_per_block"] == [15, 13, 11, 9]
        plans = [tuple(t.cpu() for t in p) for p in ts.student.tome_plans]
        want = float(T.tome_loss(R.model_forward(sd, images, 2, plans=plans)[0], ref_t, y.cpu(), 1.0, 0.5))
        dev = abs(float(info["loss"]) - want)
        print(f"bf16 train step (teacher: {with_teacher}): loss {float(info['loss']):.7f}, float64 {want:.7f}, deviation {dev:.3e}; "
              f"dense r = 0 step {dense_loss:.7f}, deviation {dense_dev:.3e}, tolerance {2 * dense_dev:.3e}")
        cfg = ts.config()
        assert cfg["train_bf16"] is True and cfg["train_merge"] is True and cfg["gemm_mode"] == ops.GEMM_BF16
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
        if not with_teacher:
            with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16"):      # a step without the keyword
                _step(False, train_bf16=False).load_state_dict(saved)
            old = dict(saved, config={k: v for k, v in saved["config"].items() if k != "train_bf16"})
            with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16"):      # a checkpoint without the key: off
                _step(False).load_state_dict(old)
            with pytest.raises(lib.D2SError, match="a captured merging step is not built"):
                _step(False, graph=True)
        assert dev <= 2 * dense_dev, (dev, dense_dev)


# ---- 7. the command line ----
def test_cli_trains_a_checkpoint_through_the_merges_in_bf16(tmp_path, capsys):
    import mask_predictor
    import vit_models
    from d2s import ops
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    before = ops._default_mode
    try:
        acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "tome", "--tome-train", "--tome-train-bf16", "--tome-r", "2", "--epochs", "1",
                                   "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--dist-weight", "0",
                                   "--student-checkpoint", path])
        assert ops.get_gemm_mode() == ops.GEMM_BF16          # the flag set the mode itself
    finally:
        ops.set_gemm_mode(before)
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Attention: --tome-train-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    assert "Start training" in out and "--tome-train: tokens per block [195, 193," in out and "val loss:" in out
