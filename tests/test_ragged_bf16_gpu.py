"""Ragged (varlen) attention on the bf16 matrix cores (d2s_attn_varlen_fwd_bf16) and the route that reaches it: the anchor to the dense
bf16 kernel, a genuinely ragged batch against float64, the entry's argument checks, a block on equal and on ragged lengths, the entries
each arithmetic mode issues, and the dynamic-keep-ratio student in eval mode (bf16 arithmetic mode).

Bounds of the float64 comparison (section 2) are the ones tests/test_policy_attention_bf16_gpu.py derives for its mask-free anchor
(all-ones policy, eps = 0), with that file's counts and formulas, per element and per image of length n:
    out_i[d]   = sum_j P_ij v_jd   c = 1 (P is rounded to bf16), L = n:   (2 c 2^-9 + 2 (L + 2) 2^-24) sum_j P_ij |v_jd|
    cls_row_j  = P_0j              c = 0:                                  2 (64 + n + 2) 2^-24 P_0j (1 + T_0j + max_j' T_0j'),
                                                                           T_0j = scale sum_d |q_0d k_jd|
    bf16 copy of out: one more rounding of the fp32 result, at most 2^-8 = 2 * 2^-9 of its magnitude (bf16 keeps 8 significant bits):
                                                                           out bound + 2^-8 (|reference| + out bound)
The reference is evaluated on the bf16-rounded q, k, v, so those carry no error.

Every float64 test prints its observed figures (error / bound per image and quantity, the block's maximum absolute error) before it
asserts; DESIGN.md section 19 is where they are recorded.
"""
import numpy as np
import pytest
import torch

from tests import cases
from tests import dynamicvit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, U16 = 2.0 ** -24, 2.0 ** -9
DH = 64
SCALE = DH ** -0.5
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)
RAGGED = (1, 2, 17, 32, 33, 64, 65, 128, 129, 197)
RAGGED_H = 2


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _dense_runs_32_key_tiles(n):
    """the rule of the dense entry (attention_bf16.hip, attn_t64, default setting): 64-key tiles from n = 384 on and wherever they pad no
    more than 32-key tiles"""
    return not (n >= 384 or (n + 63) // 64 * 64 == (n + 31) // 32 * 32)


def _qkv(tag, total, H):
    """bf16-rounded qkv [total, 3*H*64] (fp32 holding bf16 values) from d2s.synth"""
    from d2s import synth
    return _t(synth.normal(f"rg16/{tag}/{total}/{H}", (total, 3 * H * DH), std=0.7, seed=3)).bfloat16().float()


def _cu(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)


def _varlen(ops, src, cu, B, total, max_n, H):
    out, cls_row, out16 = ops.attn_varlen_fwd_bf16io(src, cu, B, total, max_n, H, SCALE, want_cls=True)
    return out, cls_row, out16


# ---- 1. anchor: equal lengths, bit for bit ----
@pytest.mark.parametrize("n,H", [(17, 2), (65, 2), (197, 2), (65, 3)])
def test_equal_lengths_are_the_dense_bf16_kernel_bit_for_bit(n, H):
    """17, 65 and 197 are lengths at which d2s_attn_fwd_bf16_bf16out runs the 32-key-tile kernel the ragged form is built from"""
    from d2s import ops
    assert _dense_runs_32_key_tiles(n)
    B = 3
    qkv = _qkv("anchor", B * n, H).to(DEV)
    cu = _cu([n] * B).to(DEV)
    for src in (qkv, qkv.bfloat16()):
        out, _, cls_row, out16 = ops.attn_fwd_bf16io(src, B, n, H, SCALE, want_cls=True)
        cls_packed = cls_row.permute(1, 0, 2).reshape(H, B * n)                    # [B, H, n] -> [H, total]
        for max_n in (n, 256):
            vout, vcls, vout16 = _varlen(ops, src, cu, B, B * n, max_n, H)
            assert torch.equal(vout, out), (n, H, max_n, src.dtype)
            assert torch.equal(vout16, out16), (n, H, max_n, src.dtype)
            assert torch.equal(vcls, cls_packed), (n, H, max_n, src.dtype)
            only16 = ops.attn_varlen_fwd_bf16io(src, cu, B, B * n, max_n, H, SCALE, want_cls=False, want_f32=False)      # out == NULL
            assert only16[0] is None and only16[1] is None and torch.equal(only16[2], out16)


# ---- 2. a genuinely ragged batch against float64 ----
_REF = {}


def _ragged_reference():
    """per image: float64 softmax(Q K^T scale) V on the bf16-rounded inputs, the CLS row, and the bounds of the module docstring; once"""
    if _REF:
        return _REF
    H, total = RAGGED_H, sum(RAGGED)
    qkv = _qkv("ragged", total, H)
    cu = _cu(RAGGED).numpy()
    out, out_bound, cls, cls_bound = [], [], [], []
    for b, n in enumerate(RAGGED):
        q, k, v = qkv[cu[b]:cu[b + 1]].double().reshape(n, 3, H, DH).permute(1, 2, 0, 3)          # [H, n, 64]
        P = ((q @ k.transpose(-2, -1)) * SCALE).softmax(dim=-1)
        m_out = P @ v.abs()
        T0 = SCALE * (q[:, :1].abs() @ k.abs().transpose(-2, -1))[:, 0]                           # [H, n]
        out.append((P @ v).transpose(0, 1).reshape(n, H * DH))
        out_bound.append(((2 * 1 * U16 + 2 * (n + 2) * U) * m_out).transpose(0, 1).reshape(n, H * DH))
        cls.append(P[:, 0])
        cls_bound.append(2 * (64 + n + 2) * U * P[:, 0] * (1.0 + T0 + T0.max(dim=-1, keepdim=True)[0]))
    _REF.update(qkv=qkv, cu=cu, out=torch.cat(out), out_bound=torch.cat(out_bound), cls=torch.cat(cls, dim=1),
                cls_bound=torch.cat(cls_bound, dim=1))
    return _REF


@pytest.mark.parametrize("max_n", [197, 200])
def test_ragged_batch_against_float64_and_the_dense_kernel(max_n):
    from d2s import ops
    ref = _ragged_reference()
    H, B, total, cu = RAGGED_H, len(RAGGED), sum(RAGGED), ref["cu"]
    qkv = ref["qkv"].to(DEV)
    out, cls_row, out16 = _varlen(ops, qkv, _cu(RAGGED).to(DEV), B, total, max_n, H)
    out_b, cls_b, out16_b = _varlen(ops, qkv.bfloat16(), _cu(RAGGED).to(DEV), B, total, max_n, H)
    torch.cuda.synchronize()
    assert torch.equal(out, out_b) and torch.equal(cls_row, cls_b) and torch.equal(out16, out16_b), "fp32 and bf16 qkv differ"
    assert torch.equal(out16, out.bfloat16())
    got, got16, gcls = out.cpu().double(), out16.cpu().double(), cls_row.cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(got16).all() and torch.isfinite(gcls).all()
    bound16 = ref["out_bound"] + 2 * U16 * (ref["out"].abs() + ref["out_bound"])
    worst = dict(out=0.0, out_bf16=0.0, cls_row=0.0)
    for b, n in enumerate(RAGGED):
        rows = slice(cu[b], cu[b + 1])
        fr = dict(out=float(((got[rows] - ref["out"][rows]).abs() / ref["out_bound"][rows].clamp_min(1e-300)).max()),
                  out_bf16=float(((got16[rows] - ref["out"][rows]).abs() / bound16[rows].clamp_min(1e-300)).max()),
                  cls_row=float(((gcls[:, rows] - ref["cls"][:, rows]).abs() / ref["cls_bound"][:, rows].clamp_min(1e-300)).max()))
        print(f"varlen attention bf16 max_n {max_n} image {b} n {n}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))
        for k, v in fr.items():
            worst[k] = max(worst[k], v)
            assert v <= 1.0, (k, n, v)
        np.testing.assert_allclose(gcls[:, rows].sum(dim=1).numpy(), 1.0, rtol=1e-5)
        if _dense_runs_32_key_tiles(n):      # the image alone through the dense entry: the same kernel, the same bits
            dout, _, dcls, dout16 = ops.attn_fwd_bf16io(qkv[rows].contiguous(), 1, n, H, SCALE, want_cls=True)
            assert torch.equal(out[rows], dout) and torch.equal(out16[rows], dout16) and torch.equal(cls_row[:, rows], dcls[0]), n
    print(f"varlen attention bf16 max_n {max_n}: worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- 3. argument checks ----
def test_argument_checks():
    """every D2S_ERR_ARG case, through the bound function itself: a refused call launches nothing"""
    from d2s import lib
    B, H, n = 2, 2, 17
    total = B * n
    qkv = torch.zeros(total, 3 * H * DH, device=DEV)
    out = torch.zeros(total, H * DH, device=DEV)
    out16 = torch.zeros(total, H * DH, device=DEV, dtype=torch.bfloat16)
    cu = _cu([n] * B).to(DEV)
    fn = lib._fn("d2s_attn_varlen_fwd_bf16")
    P = lambda t: None if t is None else t.data_ptr()

    def rc(qkv_=qkv, cu_=cu, out_=out, out16_=out16, B_=B, total_=total, max_n_=n, H_=H):
        return fn(P(qkv_), 0, P(cu_), P(out_), P(out16_), None, B_, total_, max_n_, H_, SCALE, lib.stream())
    for bad in (dict(qkv_=None), dict(cu_=None), dict(out_=None, out16_=None), dict(B_=0), dict(B_=-1), dict(total_=0), dict(total_=-3),
                dict(max_n_=0), dict(max_n_=-1), dict(max_n_=8193), dict(H_=0), dict(H_=-2)):
        assert rc(**bad) == ERR_ARG, bad
    with pytest.raises(lib.D2SError):
        lib.call("d2s_attn_varlen_fwd_bf16", P(qkv), 0, P(cu), None, None, None, B, total, n, H, SCALE)
    assert rc() == 0 and rc(out_=None) == 0 and rc(out16_=None) == 0 and rc(max_n_=8192) == 0
    torch.cuda.synchronize()


# ---- 4. - 6. a block ----
_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
BLOCK_D, BLOCK_H, BLOCK_HID = 128, 2, 512


def _block_params():
    from d2s import synth
    D, hid = BLOCK_D, BLOCK_HID
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hid, D), (hid,), (D, hid), (D,)]
    p = [_t(synth.normal(f"rg16/block/p{i}", s, std=0.05 if len(s) == 2 else 0.1, seed=11)) for i, s in enumerate(shapes)]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    return p


def _spy_calls(monkeypatch):
    from d2s import lib
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return names


def test_block_on_equal_lengths_is_the_dense_forward_only_block_bit_for_bit():
    from d2s import ops, synth
    from d2s import functional as DF
    B, n, D, H = 4, 65, BLOCK_D, BLOCK_H
    p = [t.to(DEV) for t in _block_params()]
    x = _t(synth.normal("rg16/block/x", (B, n, D), seed=12)).to(DEV)
    cu = _cu([n] * B).to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        y, cls_row = DF.run(DF.BlockFn, x, *p, H, 1e-6, True, None)
        yr, cls_r = DF.ragged_block_forward(x.view(B * n, D), cu, B, n, p, H, 1e-6, SCALE, want_cls=True)
        y0, _ = DF.run(DF.BlockFn, x, *p, H, 1e-6, False, None)
        yr0, none = DF.ragged_block_forward(x.view(B * n, D), cu, B, n, p, H, 1e-6, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(yr, y.view(B * n, D)) and torch.equal(cls_r, cls_row.permute(1, 0, 2).reshape(H, B * n))
    assert none is None and torch.equal(yr0, y0.view(B * n, D)) and torch.equal(yr0, yr)


BLOCK_LENGTHS = (5, 33, 65, 99)


def _ragged_block_case():
    from d2s import synth
    total = sum(BLOCK_LENGTHS)
    return _block_params(), _t(synth.normal("rg16/block/xr", (total, BLOCK_D), seed=15)), _cu(BLOCK_LENGTHS)


def test_ragged_block_in_bf16_mode_against_float64():
    from d2s import ops
    from d2s import functional as DF
    p, x, cu = _ragged_block_case()
    sd = {"b." + k: t.double() for k, t in zip(_NAMES, p)}
    B, H = len(BLOCK_LENGTHS), BLOCK_H
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        y, cls_rows = DF.ragged_block_forward(x.to(DEV), cu.to(DEV), B, max(BLOCK_LENGTHS), [t.to(DEV) for t in p], H, 1e-6, SCALE,
                                              want_cls=True)
    torch.cuda.synchronize()
    y, cls_rows = y.cpu(), cls_rows.cpu()
    assert torch.isfinite(y).all()
    worst = 0.0
    for b in range(B):
        rows = slice(int(cu[b]), int(cu[b + 1]))
        want = R.block(sd, "b.", x[rows].double()[None], None, H)[0]
        worst = max(worst, float((y[rows].double() - want).abs().max()))
        np.testing.assert_allclose(y[rows].numpy(), want.float().numpy(), rtol=3e-2, atol=3e-2)
        np.testing.assert_allclose(cls_rows[:, rows].sum(dim=1).numpy(), 1.0, rtol=1e-5)
    print(f"ragged block bf16: max abs error against float64 {worst:.3e}")


# what ragged_block_forward issues outside the bf16 data path (exact mode, split mode, bf16 mode with the data path off): unchanged
FP32_ROUTE = ["d2s_layernorm_fwd", "d2s_gemm_f32", "d2s_attn_varlen_fwd_f32", "d2s_gemm_f32", "d2s_layernorm_fwd", "d2s_gemm_f32",
              "d2s_gemm_f32"]
BF16_ROUTE = ["d2s_layernorm_fwd_bf16out", "d2s_gemm_f32_bf16io", "d2s_attn_varlen_fwd_bf16", "d2s_gemm_f32_bf16io",
              "d2s_layernorm_fwd_bf16out", "d2s_gemm_f32_bf16io", "d2s_gemm_f32_bf16io"]


def test_only_the_bf16_data_path_takes_the_bf16_route(monkeypatch):
    from d2s import ops
    from d2s import functional as DF
    p, x, cu = _ragged_block_case()
    p, x, cu = [t.to(DEV) for t in p], x.to(DEV), cu.to(DEV)
    B, H = len(BLOCK_LENGTHS), BLOCK_H
    names = _spy_calls(monkeypatch)

    def route(mode, io=True):
        saved = ops._BF16_IO
        ops._BF16_IO = io
        del names[:]
        try:
            with ops.gemm_mode(mode), torch.no_grad():
                y, _ = DF.ragged_block_forward(x, cu, B, max(BLOCK_LENGTHS), p, H, 1e-6, SCALE, want_cls=True)
            torch.cuda.synchronize()
        finally:
            ops._BF16_IO = saved
        return [s for s in names if s != "d2s_convert_bf16"], y      # a frozen weight's bf16 form is made once, on its first use
    bf16, y16 = route(ops.GEMM_BF16)
    exact, y = route(ops.GEMM_EXACT)
    split, _ = route(ops.GEMM_SPLIT)
    off, _ = route(ops.GEMM_BF16, io=False)
    assert bf16 == BF16_ROUTE, bf16
    for got in (exact, split, off):
        assert got == FP32_ROUTE, got
    np.testing.assert_allclose(y16.cpu().numpy(), y.cpu().numpy(), rtol=3e-2, atol=3e-2)


# ---- 7. the model ----
def test_ragged_inference_in_bf16_mode_matches_the_dense_blocks_per_image(monkeypatch):
    """micro_thr1 of tests/test_threshold_gpu.py::test_ragged_inference_matches_oracle, eval mode, bf16 arithmetic mode: the keep masks are
    read back, then every image's packed features and logits are compared with the same blocks run densely (bf16 mode, forward only) on that
    image's kept tokens alone"""
    import vit_models
    from d2s import ops
    case = cases.THRESHOLD_CASES["micro_thr1"]
    cfg = case["cfg"]
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    student = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
                                                      topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                      patch_score_threshold=case["threshold"], **common)
    sd_s, _ = cases.make_weights(case)
    student.load_state_dict({k: _t(v) for k, v in sd_s.items()}, strict=True)
    student = student.to(DEV).eval()
    x = _t(cases.make_images(case)).to(DEV)
    B, loc, D = x.shape[0], cfg["pruning_loc"][0], cfg["dim"]
    names = _spy_calls(monkeypatch)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        logits, cls_attns, _, masks = student(x)
        ragged_names = list(names)
        cu = student.cu_seqlens.cpu().numpy()
        feats = student.ragged_features.clone()
        mask = masks[0].cpu()
        counts = mask.sum(dim=1).int().numpy() + 1
        np.testing.assert_array_equal(cu, np.concatenate([[0], np.cumsum(counts)]))
        assert len(set(counts.tolist())) >= 2, f"the batch should be genuinely ragged: {counts.tolist()}"
        assert ragged_names.count("d2s_attn_varlen_fwd_bf16") == cfg["depth"] - loc and "d2s_attn_varlen_fwd_f32" not in ragged_names
        x0 = student._embed(x)                            # the dense part of the forward
        for blk in student.blocks[:loc]:
            x0 = blk(x0)
        for b in range(B):
            idx = torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.nonzero(mask[b] > 0).flatten()]).to(DEV)
            nb = int(idx.numel())
            assert nb == counts[b]
            xb = x0[b].index_select(0, idx).view(1, nb, D).contiguous()
            for blk in student.blocks[loc:]:
                xb = blk(xb)
            want_logits, _ = student._head(xb)
            want_feats, _, _ = ops.layernorm_fwd(xb.view(nb, D), ops.contiguous_map(nb, D), student.norm.weight, student.norm.bias, nb, D,
                                                 student.norm.eps, stats=False)
            err = float((feats[cu[b]:cu[b + 1]] - want_feats).abs().max())
            print(f"ragged inference bf16 image {b} ({nb} tokens): max abs feature difference {err:.3e}")
            np.testing.assert_allclose(feats[cu[b]:cu[b + 1]].cpu().numpy(), want_feats.cpu().numpy(), rtol=3e-2, atol=3e-2)
            np.testing.assert_allclose(logits[b].cpu().numpy(), want_logits[0].cpu().numpy(), rtol=3e-2, atol=3e-2)
    assert tuple(cls_attns[-1].shape) == (cfg["heads"], int(cu[-1]))
    for b in range(B):
        np.testing.assert_allclose(cls_attns[-1][:, cu[b]:cu[b + 1]].sum(dim=1).cpu().numpy(), 1.0, rtol=1e-5)
