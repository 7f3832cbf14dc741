"""Token merging on the bf16 data path (--tome-bf16) on the GPU: d2s_attn_keyw_fwd_bf16 anchored to the dense bf16
kernel and against float64, d2s_tome_match_bf16 against d2s_tome_match bit for bit, both entries' refusals, the block, the entries a
model issues, the model against the float64 restatement with the GPU's plans replayed, and the command line.

The bounds of the float64 comparison are derived in tests/tome_bf16_cases.py (its docstring); tests/test_tome_bf16_cpu.py checks there
that an emulation of the kernel's roundings stays inside them.  Every float64 test prints its observed figures before it asserts;
DESIGN.md section 22 records them.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases
from tests import test_tome_gpu as T
from tests import tome_bf16_cases as C
from tests import tome_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCALE = C.SCALE
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _dense_runs_32_key_tiles(n):
    """the rule of the dense entry (attention_bf16.hip, attn_t64, default setting): 64-key tiles from n = 384 on and wherever they pad no
    more than 32-key tiles"""
    return not (n >= 384 or (n + 63) // 64 * 64 == (n + 31) // 32 * 32)


# ---- 1. anchor: unit weights are the dense bf16 kernel, bit for bit ----
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("n", [17, 65, 129, 197])
def test_unit_weights_are_the_dense_bf16_kernel_bit_for_bit(n, H):
    from d2s import ops
    assert _dense_runs_32_key_tiles(n)
    assert not any(_dense_runs_32_key_tiles(m) for m in (33, 99, 128))          # those take 64-key tiles: no anchors
    B = 3
    qkv = torch.randn((B * n, 3 * H * 64), generator=torch.Generator().manual_seed(100 + n + H)).bfloat16().float().to(DEV)
    ones = torch.ones((B, n), dtype=torch.float32, device=DEV)
    for src in (qkv, qkv.bfloat16()):
        out, lse, _, out16 = ops.attn_fwd_bf16io(src, B, n, H, SCALE, want_cls=False)
        kout, klse, kout16 = ops.attn_keyw_fwd_bf16io(src, ones, B, n, H, SCALE)
        assert torch.equal(kout, out) and torch.equal(kout16, out16) and torch.equal(klse, lse), (n, H, src.dtype)
        only16 = ops.attn_keyw_fwd_bf16io(src, ones, B, n, H, SCALE, want_f32=False)                      # out == NULL
        assert only16[0] is None and torch.equal(only16[1], lse) and torch.equal(only16[2], out16)


# ---- 2. weighted attention against float64 ----
@pytest.mark.parametrize("n,H", C.KEYW_SHAPES)
def test_weighted_attention_against_float64(n, H):
    """Observed worst error / bound over all 14 shapes on an MI355X: see DESIGN.md section 22 ("Inference on the bf16 data path")."""
    from d2s import ops
    case = C.keyw_case(n, H)
    B = C.KEYW_B
    qkv = case["qkv"].reshape(B * n, 3 * H * 64).contiguous().to(DEV)
    w = case["w"].to(DEV)
    out, lse, out16 = ops.attn_keyw_fwd_bf16io(qkv, w, B, n, H, SCALE)
    out_b, lse_b, out16_b = ops.attn_keyw_fwd_bf16io(qkv.bfloat16(), w, B, n, H, SCALE)
    out_2, lse_2, out16_2 = ops.attn_keyw_fwd_bf16io(qkv, w, B, n, H, SCALE)
    torch.cuda.synchronize()
    fr = C.fractions(case, out.cpu(), out16.cpu(), lse.cpu())
    print(f"keyw attention bf16 n {n} H {H}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert torch.equal(out, out_b) and torch.equal(lse, lse_b) and torch.equal(out16, out16_b), "fp32 and bf16 qkv differ"
    assert torch.equal(out16, out.bfloat16())
    assert torch.equal(out, out_2) and torch.equal(lse, lse_2) and torch.equal(out16, out16_2), "two runs differ"
    for k, v in fr.items():
        assert v <= 1.0, (k, n, H, v)


# ---- 3. argument checks ----
def test_both_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, n, H, r = 2, 9, 2, 2
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    h = lambda *shape: torch.full(shape, 7.0, dtype=torch.bfloat16, device=DEV)
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    qkv32, qkv16, w = f(B * n, 3 * H * 64), h(B * 896, 3 * H * 64), f(B, n)
    out, out16, lse = f(B * n, H * 64), h(B * n, H * 64), f(B, H, n)
    nm, ni, unm, src, dst = f(B, 448), i(B, 448), i(B, 448), i(B, 448), i(B, 448)
    outputs = (out, out16, lse, nm, ni, unm, src, dst)
    p, s = lib.ptr, lib.stream()

    def keyw(q=qkv32, is16=0, w_=w, o=out, o16=out16, l=lse, B_=B, n_=n, H_=H):
        return lib._fn("d2s_attn_keyw_fwd_bf16")(p(q), is16, p(w_), p(o), p(o16), p(l), B_, n_, H_, ctypes.c_float(SCALE), s)

    def match(q=qkv16, B_=B, n_=n, H_=H, r_=r, a=nm, b=ni, c=unm, d=src, e=dst):
        return lib._fn("d2s_tome_match_bf16")(p(q), B_, n_, H_, r_, p(a), p(b), p(c), p(d), p(e), s)

    bad = [keyw(q=None), keyw(w_=None), keyw(l=None), keyw(o=None, o16=None), keyw(B_=0), keyw(B_=-1), keyw(H_=0), keyw(H_=-2), keyw(n_=1),
           keyw(n_=0), keyw(n_=-5), keyw(n_=8193), keyw(q=qkv16, is16=1, n_=1),
           match(q=None), match(a=None), match(b=None), match(c=None), match(d=None), match(e=None), match(r_=-1), match(r_=5), match(n_=1),
           match(n_=897, r_=0), match(n_=4096, r_=0), match(H_=0), match(B_=0)]
    torch.cuda.synchronize()
    assert bad == [ERR_ARG] * len(bad), bad
    for t in outputs:                                     # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    with pytest.raises(lib.D2SError):                     # lib.call serves the extension table and raises on the code
        lib.call("d2s_attn_keyw_fwd_bf16", p(qkv32), 0, p(w), None, None, p(lse), B, n, H, SCALE)
    assert keyw() == 0 and keyw(o=None) == 0 and keyw(o16=None) == 0 and keyw(n_=2) == 0
    assert match(r_=4) == 0 and match(r_=0, d=None, e=None) == 0 and match(n_=896, r_=0) == 0      # the limits themselves are accepted
    torch.cuda.synchronize()


# ---- 4. the match on a bf16 qkv ----
def _both_matches(q16, r):
    from d2s import ops
    B, n, _, H, _ = q16.shape
    flat = q16.to(DEV).reshape(B * n, 3 * H * 64).contiguous()
    got = ops.tome_match_bf16(flat, B, n, H, r)
    want = ops.tome_match(flat.float(), B, n, H, r)
    torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize("B,n,H,r", T.MATCH_SHAPES)
def test_match_on_bf16_qkv_is_the_fp32_match_bit_for_bit(B, n, H, r):
    got, want = _both_matches(T._qkv(B, n, H).bfloat16(), r)
    for g, w, name in zip(got, want, ("node_max", "node_idx", "unm_idx", "src_idx", "dst_idx")):
        assert g.dtype == w.dtype and torch.equal(g, w), (name, B, n, H, r)
    again = _both_matches(T._qkv(B, n, H).bfloat16(), r)[0]
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_match_ties_on_rows_made_after_the_rounding():
    gen = torch.Generator().manual_seed(5)
    q16 = torch.randn((2, 10, 3, 2, 64), generator=gen).bfloat16()
    q16[:, 3, 1] = q16[:, 1, 1]                  # B rows 0 and 1 identical
    q16[:, 2, 1] = 2.0 * q16[:, 1, 1]            # A row 1 points exactly at them (a power of two: exact in bf16)
    got, want = _both_matches(q16, 0)
    assert got[1][:, 1].tolist() == [0, 0] and not bool((got[1] == 1).any())
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    q16 = torch.randn((2, 10, 3, 2, 64), generator=gen).bfloat16()
    q16[:, 4, 1] = 4.0 * q16[:, 1, 1]            # A rows 2 and 3 identical and the best matched of all: they straddle the boundary at r = 1
    q16[:, 6, 1] = 4.0 * q16[:, 1, 1]
    got, want = _both_matches(q16, 1)
    node_max, _, unm, src, dst = got
    assert torch.equal(node_max[:, 2], node_max[:, 3]) and src.tolist() == [[2], [2]] and dst.tolist() == [[0], [0]]
    assert unm.tolist() == [[0, 1, 3, 4]] * 2
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    got, want = _both_matches(q16, 2)
    assert got[3].tolist() == [[2, 3]] * 2 and all(torch.equal(g, w) for g, w in zip(got, want))


# ---- 5. the block ----
_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _block_params(D, hid):
    from d2s import synth
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hid, D), (hid,), (D, hid), (D,)]
    p = [_t(synth.normal(f"tome16/block/p{i}", s, std=0.05 if len(s) == 2 else 0.1, seed=11)) for i, s in enumerate(shapes)]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    return p


def test_block_without_merging_is_the_bf16_forward_only_block_bit_for_bit():
    from d2s import lib, ops, synth
    from d2s import functional as DF
    from d2s import functional_tome as TF
    B, n, D, H, hid = 4, 65, 128, 2, 512
    p = [t.to(DEV) for t in _block_params(D, hid)]
    x = _t(synth.normal("tome16/block/x", (B, n, D), seed=12)).to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        want, _ = DF.run(DF.BlockFn, x, *p, H, 1e-6, False, None)
        y, size, plan = TF.tome_block_forward_bf16(x.view(B * n, D), None, p, B, n, H, 1e-6, SCALE, 0)
    torch.cuda.synchronize()
    assert size is None and plan is None and torch.equal(y, want.view(B * n, D))
    with pytest.raises(lib.D2SError) as e, torch.no_grad():                               # outside the bf16 data path: refused, by name
        TF.tome_block_forward_bf16(x.view(B * n, D), None, p, B, n, H, 1e-6, SCALE, 0)
    assert "bf16 arithmetic mode" in str(e.value) and "D2S_BF16_IO" in str(e.value) and "multiples of 32" in str(e.value)


def _block_ref(p, x, size, plan, H):
    """float64 restatement of the merging block: tests/tome_ref.py's pieces around the given plan"""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = [t.double() for t in p]
    B, n, D = x.shape
    x = x.double()
    qkv = F.linear(F.layer_norm(x, (D,), n1w, n1b, 1e-6), qkvw, qkvb).reshape(B, n, 3, H, 64)
    ao, _ = R.keyw_attention(qkv, size.double(), SCALE)
    x1 = x + F.linear(ao, projw, projb)
    x1, size_out = R.merge(x1, size, *[t.long() for t in plan])[:2]
    y = x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, (D,), n2w, n2b, 1e-6), fc1w, fc1b)), fc2w, fc2b)
    return y, size_out


@pytest.mark.parametrize("B,n,D,H,hid,r", [(3, 33, 128, 2, 512, 5), (2, 66, 128, 2, 512, 16)])
def test_merging_block_against_float64_with_the_gpu_plan_replayed(B, n, D, H, hid, r):
    from d2s import ops, synth
    from d2s import functional_tome as TF
    p = _block_params(D, hid)
    x = _t(synth.normal(f"tome16/block/xm{n}", (B, n, D), seed=13))
    size = torch.randint(1, 5, (B, n), generator=torch.Generator().manual_seed(n)).float()
    pd = [t.to(DEV) for t in p]
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        y, size_out, plan = TF.tome_block_forward_bf16(x.to(DEV).view(B * n, D), size.to(DEV), pd, B, n, H, 1e-6, SCALE, r)
        y2, size_out2, plan2 = TF.tome_block_forward_bf16(x.to(DEV).view(B * n, D), size.to(DEV), pd, B, n, H, 1e-6, SCALE, r, plan=plan)
    torch.cuda.synchronize()
    assert y.shape == (B * (n - r), D) and size_out.shape == (B, n - r) and [t.shape[1] for t in plan] == [(n + 1) // 2 - r, r, r]
    assert torch.equal(y2, y) and torch.equal(size_out2, size_out) and plan2 is plan
    want, want_size = _block_ref(p, x, size, [t.cpu() for t in plan], H)
    assert torch.equal(size_out.cpu().double(), want_size)
    err = float((y.cpu().double().view(B, n - r, D) - want).abs().max())
    print(f"merging block bf16 n {n} r {r}: max abs error against float64 {err:.3e}")
    np.testing.assert_allclose(y.cpu().numpy().reshape(B, n - r, D), want.float().numpy(), rtol=3e-2, atol=3e-2)


# ---- 6. the route ----
def _spy_calls(monkeypatch):
    from d2s import lib
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return names


def _route(embed, ln, gemm, attn0, attn, match, head, depth):
    block = lambda a: [ln, gemm, a, gemm, match, "d2s_tome_merge", ln, gemm, gemm]
    return embed + block(attn0) + block(attn) * (depth - 1) + head


_EMBED = ["d2s_im2col_patch", "d2s_gemm_f32", "d2s_fill_cls"]
_HEAD = ["d2s_layernorm_fwd", "d2s_gemm_f32"]
# what the default (fp32) model issues in exact mode, micro1 with r = 2: the parent's list
FP32_ROUTE = _route(_EMBED, "d2s_layernorm_fwd", "d2s_gemm_f32", "d2s_attn_fwd_f32", "d2s_attn_keyw_fwd_f32", "d2s_tome_match", _HEAD, 4)
BF16_ROUTE = _route(_EMBED, "d2s_layernorm_fwd_bf16out", "d2s_gemm_f32_bf16io", "d2s_attn_fwd_bf16_bf16out", "d2s_attn_keyw_fwd_bf16",
                    "d2s_tome_match_bf16", _HEAD, 4)


def test_only_the_bf16_model_takes_the_bf16_route(monkeypatch):
    from d2s import ops
    _, _, images, _ = T._models("micro1")
    fp32, bf16 = T._tome("micro1", tome_r=2), T._tome("micro1", tome_r=2, bf16=True)
    names = _spy_calls(monkeypatch)
    with ops.gemm_mode(ops.GEMM_EXACT):
        bf16(images.to(DEV))
        got16 = [s for s in names if s != "d2s_convert_bf16"]      # a frozen weight's bf16 form is made once, on its first use
        del names[:]
        fp32(images.to(DEV))
        got32 = list(names)
    torch.cuda.synchronize()
    assert got16 == BF16_ROUTE, got16
    assert got32 == FP32_ROUTE, got32
    assert "d2s_attn_keyw_fwd_f32" not in got16 and "d2s_tome_match" not in got16
    assert got16.count("d2s_attn_fwd_bf16_bf16out") == 1 and got16.index("d2s_attn_fwd_bf16_bf16out") < got16.index("d2s_attn_keyw_fwd_bf16")
    assert bf16.tokens_per_block == fp32.tokens_per_block == [15, 13, 11, 9]


# ---- 7. the model ----
@pytest.mark.parametrize("name", ["micro1", "tiny32"])
def test_bf16_model_r0_is_the_teacher_in_bf16_mode_bit_for_bit(name):
    from d2s import ops
    teacher, _, images, geom = T._models(name)
    m = T._tome(name, tome_r=0, bf16=True)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        want = teacher(images.to(DEV))[0]
    got = m(images.to(DEV))                               # from the ambient (exact) mode: the model enters the bf16 mode itself
    assert torch.equal(got, want)
    n = (geom["img_size"] // geom["patch_size"]) ** 2 + 1
    assert m.tokens_per_block == [n] * geom["depth"] and m.tome_plans == [None] * geom["depth"]


@pytest.mark.parametrize("name,r,prop,ambient", [
    ("micro1", 2, True, "exact"),
    ("micro1", 8, True, "split"),
    ("micro1", 8, False, "exact"),
    ("micro1", [0, 3, 0, 8], True, "exact"),
    ("tiny32", 2, True, "exact"),
])
def test_bf16_model_against_float64_with_the_gpu_plans_replayed(name, r, prop, ambient):
    from d2s import ops
    _, sd, images, _ = T._models(name)
    m = T._tome(name, tome_r=r, prop_attn=prop, bf16=True)
    fp32 = T._tome(name, tome_r=r, prop_attn=prop)
    mode = ops.GEMM_SPLIT if ambient == "split" else ops.GEMM_EXACT
    with ops.gemm_mode(mode):
        logits = m(images.to(DEV))
        assert ops.get_gemm_mode() == mode                                     # the ambient mode is back
        plans = [None if p is None else tuple(t.cpu() for t in p) for p in m.tome_plans]
        again = m(images.to(DEV), plans=[None if p is None else tuple(t.to(DEV) for t in p) for p in plans])
        assert ops.get_gemm_mode() == mode
        fp32(images.to(DEV))
    assert torch.equal(again, logits)                                          # replaying the model's own plans changes nothing
    assert m.tokens_per_block == fp32.tokens_per_block
    ref, ref_counts = R.model_forward(sd, images, r, plans=plans, prop_attn=prop)
    assert ref_counts == m.tokens_per_block
    err = float((logits.cpu().double() - ref).abs().max())
    print(f"bf16 merging model {name} r {r} prop_attn {prop}: max abs logit error against float64 {err:.3e}")
    np.testing.assert_allclose(logits.cpu().numpy(), ref.float().numpy(), rtol=3e-2, atol=3e-2)


def test_bf16_model_restores_the_mode_on_an_exception_and_refuses_training():
    from d2s import ops
    from vit_models import tome
    _, _, images, _ = T._models("micro1")
    m = T._tome("micro1", tome_r=2, bf16=True)
    for mode in (ops.GEMM_EXACT, ops.GEMM_SPLIT):
        with ops.gemm_mode(mode):
            with pytest.raises(Exception):
                m(images.to(DEV), plans=[None])                                # too short a plan list: raised inside the bf16 mode
            assert ops.get_gemm_mode() == mode
    m.train()
    with pytest.raises(NotImplementedError) as e:
        m(images.to(DEV))
    assert str(e.value) == tome.TOME_TRAINING_ERROR


# ---- 8. command line ----
def test_cli_evaluates_on_the_bf16_data_path(tmp_path, capsys):
    import mask_predictor
    import vit_models
    from d2s import ops
    torch.manual_seed(0)
    sd = vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()
    sd["score_predictor.0.in_conv.0.weight"] = torch.ones(192)               # a dense-to-sparse student's file carries predictors
    path = os.path.join(tmp_path, "student.pt")
    torch.save({"model": sd}, path)
    before = ops._default_mode
    try:
        acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "tome", "--tome-r", "2", "--eval-only", "--tome-bf16",
                                   "--student-checkpoint", path, "--batch-size", "4", "--val-steps", "1"])
    finally:
        ops.set_gemm_mode(before)
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "ignored 1 predictor tensors" in out and "val loss:" in out and "tokens per block [195, 193," in out
    assert "(bf16 data path)" in out and "Start training" not in out
