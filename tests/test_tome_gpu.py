"""Token merging on the GPU: d2s_tome_match, d2s_tome_merge and d2s_attn_keyw_fwd_f32 against the float64
restatement in tests/tome_ref.py, the tie rules bit for bit, the entries' refusals, the model against the restatement with the GPU's own
plans replayed, and the command line."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import tome_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MATCH_SHAPES = [(2, 3, 1, 1), (2, 9, 3, 2), (2, 9, 3, 0), (2, 10, 3, 4), (3, 65, 3, 16), (3, 66, 1, 32), (2, 197, 6, 13), (2, 197, 3, 98),
                (2, 577, 12, 100), (2, 577, 3, 288)]


def _qkv(B, n, H):
    return torch.randn((B, n, 3, H, 64), generator=torch.Generator().manual_seed(1234 + n))


def _match(qkv, r):
    from d2s import ops
    B, n, _, H, _ = qkv.shape
    out = ops.tome_match(qkv.to(DEV).reshape(B * n, 3 * H * 64).contiguous(), B, n, H, r)
    torch.cuda.synchronize()
    return out


# ---- 1. match against float64 ----
@pytest.mark.parametrize("B,n,H,r", MATCH_SHAPES)
def test_match_against_float64(B, n, H, r):
    qkv = _qkv(B, n, H)
    E = (64 + H + 4) * 2.0 ** -24          # H-term mean, normalisation, 64-term dot of unit vectors, |score| <= 1
    best_gap, rank_gap = R.gaps(qkv, r)
    print(f"n={n} H={H} r={r}: best/second gap {best_gap:.3e}, rank gap {rank_gap:.3e}, 2E {2 * E:.3e}")
    assert best_gap >= 2 * E and rank_gap >= 2 * E          # asserted on the REFERENCE: the seeds leave no row inside either gap
    node_max_r, node_idx_r, unm_r, src_r, dst_r = R.match(qkv, r)
    node_max, node_idx, unm, src, dst = _match(qkv, r)
    assert node_idx.dtype == torch.int32 and unm.shape == unm_r.shape and src.shape == (B, r) and dst.shape == (B, r)
    nm = node_max.cpu().double()
    assert bool((nm[:, 0] == -math.inf).all())
    err = float((nm[:, 1:] - node_max_r[:, 1:]).abs().max()) if nm.shape[1] > 1 else 0.0
    print(f"max |node_max - ref| = {err:.3e} (bound {E:.3e})")
    assert err <= E
    assert torch.equal(node_idx.cpu().long(), node_idx_r)
    assert torch.equal(unm.cpu().long(), unm_r) and torch.equal(src.cpu().long(), src_r) and torch.equal(dst.cpu().long(), dst_r)


# ---- 2. ties ----
def test_ties_lowest_index_wins_and_ranking_is_select_topk():
    from d2s import ops
    gen = torch.Generator().manual_seed(5)
    qkv = torch.randn((2, 10, 3, 2, 64), generator=gen)
    qkv[:, 3, 1] = qkv[:, 1, 1]                  # B rows 0 and 1 identical
    qkv[:, 2, 1] = 2.0 * qkv[:, 1, 1]            # A row 1 points exactly at them
    _, node_idx, _, _, _ = _match(qkv, 0)
    assert node_idx[:, 1].tolist() == [0, 0] and not bool((node_idx == 1).any())
    qkv = torch.randn((2, 10, 3, 2, 64), generator=gen)
    qkv[:, 4, 1] = 3.0 * qkv[:, 1, 1]            # A rows 2 and 3 identical and the best matched of all: they straddle the boundary at r = 1
    qkv[:, 6, 1] = 3.0 * qkv[:, 1, 1]
    node_max, _, unm, src, dst = _match(qkv, 1)
    assert torch.equal(node_max[:, 2], node_max[:, 3]) and src.tolist() == [[2], [2]] and dst.tolist() == [[0], [0]]
    assert unm.tolist() == [[0, 1, 3, 4]] * 2
    assert _match(qkv, 2)[3].tolist() == [[2, 3]] * 2
    # ranking consistency: d2s_select_topk on the emitted node_max picks the same sources, bit for bit
    for (B, n, H, r) in ((3, 65, 3, 16), (2, 197, 6, 13), (2, 577, 12, 100)):
        node_max, _, unm, src, _ = _match(_qkv(B, n, H), r)
        kept, dropped = ops.select_topk(node_max.contiguous(), r)
        assert torch.equal(kept.int(), src) and torch.equal(dropped.int(), unm)


# ---- 3. merge against float64 ----
def _check_merge(x, size, plan, n, r):
    from d2s import ops
    B, _, D = x.shape
    unm, src, dst = plan
    xd = x.to(DEV).reshape(B * n, D).contiguous()
    sd = None if size is None else size.to(DEV)
    out, size_out = ops.tome_merge(xd, sd, unm, src, dst, B, n, D, r)
    out2, size_out2 = ops.tome_merge(xd, sd, unm, src, dst, B, n, D, r)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(size_out, size_out2)                   # no atomics: two runs are bit-identical
    ref, size_ref, group, amax = R.merge(x, size, unm.cpu().long(), src.cpu().long(), dst.cpu().long())
    assert torch.equal(size_out.cpu().double(), size_ref)                                # sums of small integers: exact
    got = out.cpu().double().reshape(B, n - r, D)
    bound = (group.double() + 3) * 2.0 ** -24 * amax / size_ref                          # (m + 3) 2^-24 max|s x| / denominator per row
    err = (got - ref).abs().amax(dim=-1)
    print(f"merge n={n} r={r} D={D} sizes={'given' if size is not None else 'ones'}: max err/bound {float((err / bound).max()):.3f}, "
          f"largest group {int(group.max())}")
    assert bool((err <= bound).all())
    copied = group == 1
    src_rows = torch.cat([2 * unm.cpu().long(), (2 * torch.arange(n // 2) + 1).expand(B, -1)], dim=1)
    assert torch.equal(got[copied], x.double()[torch.arange(B)[:, None].expand_as(src_rows)[copied], src_rows[copied]])    # copies are exact
    return out, size_out


@pytest.mark.parametrize("B,n,H,r,D", [(2, 65, 2, 16, 128), (3, 66, 1, 32, 192), (2, 197, 3, 98, 384)])
def test_merge_against_float64_on_the_kernels_own_plans(B, n, H, r, D):
    gen = torch.Generator().manual_seed(900 + n)
    plan = _match(_qkv(B, n, H), r)[2:]
    x = torch.randn((B, n, D), generator=gen)
    size = torch.randint(1, 8, (B, n), generator=gen).float()
    _check_merge(x, None, plan, n, r)
    _check_merge(x, size, plan, n, r)


def test_merge_identity_at_r0_and_many_sources_on_one_destination():
    from d2s import ops
    gen = torch.Generator().manual_seed(31)
    B, n, D = 2, 21, 128
    x = torch.randn((B, n, D), generator=gen)
    size = torch.randint(1, 8, (B, n), generator=gen).float()
    i32 = dict(dtype=torch.int32, device=DEV)
    # r = 0: A rows in order, then B rows - the kernel's own plan is the identity permutation of the two sets
    unm0 = _match(torch.randn((B, n, 3, 1, 64), generator=gen), 0)[2]
    empty = torch.empty((B, 0), **i32)
    assert unm0.tolist() == [list(range(11))] * B
    out, so = ops.tome_merge(x.to(DEV).reshape(B * n, D), size.to(DEV), unm0, empty, empty, B, n, D, 0)
    want = torch.cat([x[:, 0::2], x[:, 1::2]], dim=1)
    assert torch.equal(out.cpu().reshape(B, n, D), want) and torch.equal(so.cpu(), torch.cat([size[:, 0::2], size[:, 1::2]], dim=1))
    out, so = ops.tome_merge(x.to(DEV).reshape(B * n, D), None, unm0, empty, empty, B, n, D, 0)
    assert torch.equal(out.cpu().reshape(B, n, D), want) and bool((so == 1).all())
    # every one of the 10 non-CLS A rows lands on B row 4 (image 0) / B row 9 (image 1)
    unm = torch.zeros((B, 1), **i32)
    src = torch.arange(1, 11, **i32).expand(B, -1).contiguous()
    dst = torch.tensor([[4] * 10, [9] * 10], **i32)
    for s in (None, size):
        out, so = _check_merge(x, s, (unm, src, dst), n, 10)
        assert so.shape == (B, 11)
        if s is None:              # CLS, then the ten B rows: the destination stands for itself and the ten sources
            assert so[0].tolist() == [1.0] * 5 + [11.0] + [1.0] * 5 and so[1].tolist() == [1.0] * 10 + [11.0]


# ---- 4. weighted attention against float64 ----
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n", [2, 31, 32, 33, 128, 129, 197])
def test_keyw_attention_against_float64(n, H):
    from d2s import ops
    B = 2
    gen = torch.Generator().manual_seed(4000 + 10 * n + H)
    qkv = torch.randn((B, n, 3, H, 64), generator=gen)
    w = torch.randint(1, n + 1, (B, n), generator=gen).float()
    qd = qkv.to(DEV).reshape(B * n, 3 * H * 64).contiguous()
    out, lse = ops.attn_keyw_fwd(qd, w.to(DEV), B, n, H, 0.125, want_lse=True)
    out_nolse, none = ops.attn_keyw_fwd(qd, w.to(DEV), B, n, H, 0.125)
    ref_out, ref_lse = R.keyw_attention(qkv, w, 0.125)
    np.testing.assert_allclose(out.cpu().numpy().reshape(B, n, H * 64), ref_out.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(lse.cpu().numpy(), ref_lse.numpy(), rtol=1e-5, atol=1e-5)
    assert none is None and torch.equal(out, out_nolse)
    # all weights 1.0: bit for bit the plain forward
    ones = torch.ones((B, n), dtype=torch.float32, device=DEV)
    out1, lse1 = ops.attn_keyw_fwd(qd, ones, B, n, H, 0.125, want_lse=True)
    outp, lsep, _ = ops.attn_fwd(qd, B, n, H, 0.125, want_cls=False)
    assert torch.equal(out1, outp) and torch.equal(lse1, lsep)


# ---- 5. refusals ----
def test_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, n, H, D, r = 2, 9, 2, 128, 2
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    qkv, x, size = f(B * 900, 3 * H * 64), f(B * 900, D), f(B, 900)
    nm, ni, unm, src, dst = f(B, 450), i(B, 450), i(B, 450), i(B, 450), i(B, 450)
    xo, so, out, lse = f(B * 900, D), f(B, 900), f(B * 900, H * 64), f(B, H, 900)
    outputs = (nm, ni, unm, src, dst, xo, so, out, lse)
    p, s = lib.ptr, lib.stream()

    def match(q=qkv, B_=B, n_=n, H_=H, r_=r, a=nm, b=ni, c=unm, d=src, e=dst):
        return lib._fn("d2s_tome_match")(p(q), B_, n_, H_, r_, p(a), p(b), p(c), p(d), p(e), s)

    def merge(x_=x, c=unm, d=src, e=dst, B_=B, n_=n, D_=D, r_=r, o=xo, z=so):
        return lib._fn("d2s_tome_merge")(p(x_), p(size), p(c), p(d), p(e), B_, n_, D_, r_, p(o), p(z), s)

    def keyw(q=qkv, w=size, o=out, n_=n, B_=B, H_=H):
        return lib._fn("d2s_attn_keyw_fwd_f32")(p(q), p(w), p(o), p(lse), B_, n_, H_, ctypes.c_float(0.125), s)

    bad = [match(q=None), match(a=None), match(b=None), match(c=None), match(d=None), match(e=None), match(r_=-1), match(r_=5), match(n_=1),
           match(n_=897, r_=0), match(n_=4096, r_=0), match(H_=0), match(B_=0),
           merge(x_=None), merge(c=None), merge(d=None), merge(e=None), merge(o=None), merge(z=None), merge(r_=-1), merge(r_=5), merge(n_=1),
           merge(D_=130), merge(D_=0), merge(n_=897), merge(B_=0),
           keyw(q=None), keyw(w=None), keyw(o=None), keyw(n_=1), keyw(n_=0), keyw(n_=8193), keyw(B_=0), keyw(H_=0)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    for t in outputs:                                     # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    assert match(r_=4) == 0 and match(n_=896, r_=0) == 0  # the limits themselves are accepted
    torch.cuda.synchronize()


# ---- 6. model ----
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


def _tome(name, **kw):
    import vit_models
    _, sd, _, geom = _models(name)
    m = vit_models.VisionTransformerToMe(**geom, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", ["micro1", "tiny32"])
def test_model_r0_is_the_teacher_bit_for_bit(name):
    teacher, _, images, geom = _models(name)
    m = _tome(name, tome_r=0)
    with torch.no_grad():
        want = teacher(images.to(DEV))[0]
    got = m(images.to(DEV))
    assert torch.equal(got, want)
    n = (geom["img_size"] // geom["patch_size"]) ** 2 + 1
    assert m.tokens_per_block == [n] * geom["depth"] and m.tome_plans == [None] * geom["depth"]


@pytest.mark.parametrize("name,r,prop,mode,counts", [
    ("micro1", 2, True, "exact", [15, 13, 11, 9]),
    ("micro1", 8, True, "exact", [9, 5, 3, 2]),
    ("micro1", 8, False, "exact", [9, 5, 3, 2]),
    ("micro1", [0, 3, 0, 8], True, "exact", [17, 14, 14, 8]),
    ("micro1", 2, True, "split", [15, 13, 11, 9]),
    ("tiny32", 2, True, "exact", [3] + [2] * 11),
])
def test_model_against_float64_with_the_gpu_plans_replayed(name, r, prop, mode, counts):
    from d2s import ops
    _, sd, images, _ = _models(name)
    m = _tome(name, tome_r=r, prop_attn=prop)
    with ops.gemm_mode(ops.GEMM_SPLIT if mode == "split" else ops.GEMM_EXACT):
        logits = m(images.to(DEV))
        assert m.tokens_per_block == counts
        plans = [None if p is None else tuple(t.cpu() for t in p) for p in m.tome_plans]
        again = m(images.to(DEV), plans=[None if p is None else tuple(t.to(DEV) for t in p) for p in plans])
    assert torch.equal(again, logits)                                          # replaying the model's own plans changes nothing
    ref, ref_counts = R.model_forward(sd, images, r, plans=plans, prop_attn=prop)
    assert ref_counts == counts
    np.testing.assert_allclose(logits.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-5)
    if prop and name == "micro1" and r == 8:                                   # the sizes matter: without them the logits move
        other = R.model_forward(sd, images, r, plans=plans, prop_attn=False)[0]
        assert float((other - ref).abs().max()) > 1e-4


def test_model_refuses_training_and_the_bf16_mode():
    from d2s import lib, ops
    from vit_models import tome
    _, _, images, _ = _models("micro1")
    m = _tome("micro1", tome_r=2)
    m.train()
    with pytest.raises(NotImplementedError) as e:
        m(images.to(DEV))
    assert str(e.value) == tome.TOME_TRAINING_ERROR
    m.eval()
    with ops.gemm_mode(ops.GEMM_BF16), pytest.raises(lib.D2SError):
        m(images.to(DEV))
    dense = _tome("micro1", tome_r=0).train()                                 # r = 0 in training mode: the dense, differentiable trunk
    out = dense(images.to(DEV))
    out.sum().backward()
    assert dense.head.weight.grad is not None and out.shape == (images.shape[0], 10)


# ---- 7. command line ----
def test_cli_evaluates_a_checkpoint_with_predictor_keys(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    sd = vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()
    sd["score_predictor.0.in_conv.0.weight"] = torch.ones(192)               # a dense-to-sparse student's file carries predictors
    path = os.path.join(tmp_path, "student.pt")
    torch.save({"model": sd}, path)
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "tome", "--tome-r", "2", "--eval-only", "--student-checkpoint", path,
                               "--batch-size", "4", "--val-steps", "1"])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "ignored 1 predictor tensors" in out and "val loss:" in out and "tokens per block [195, 193," in out
    assert "Start training" not in out
