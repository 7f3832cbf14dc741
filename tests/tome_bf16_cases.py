"""Inputs, float64 reference and bounds of the key-weighted attention on the bf16 matrix cores (d2s_attn_keyw_fwd_bf16),
shared by tests/test_tome_bf16_gpu.py (the kernel against float64) and tests/test_tome_bf16_cpu.py (a CPU emulation of the kernel's
roundings against the same bounds, so that the bounds are not fixed blind).  Plain torch on the CPU.

Bounds, per element, reference evaluated on the bf16-rounded q, k, v (those carry no error); U = 2^-24, U16 = 2^-9:
    out_i[d] = sum_j Pw_ij v_jd, Pw = softmax(S + log w):  (2 U16 + 2 (n + 3) U) sum_j Pw_ij |v_jd|
        section 19's bound of `out` (P rounded to bf16 once: c = 1; n-term fp32 sums, the division) with one more fp32 rounding for e * w
    bf16 copy of out: one more rounding of the fp32 result:  out bound + 2 U16 (|reference| + out bound)
    lse_i = log sum_j w_j exp(S_ij):  2 (64 + n + 3) U (1 + |reference| + T_i),  T_i = scale max_j sum_d |q_id| |k_jd|
        the 64-term fp32 accumulation of exact products, the fma and exp2 arguments, the n-term sum and the log
"""
import torch

U, U16 = 2.0 ** -24, 2.0 ** -9
DH = 64
SCALE = DH ** -0.5
KEYW_B = 2
KEYW_SHAPES = [(n, H) for n in (2, 31, 32, 33, 128, 129, 197) for H in (1, 3)]
_CACHE = {}


def keyw_case(n, H):
    """-> dict(qkv [B,n,3,H,64] fp32 holding bf16 values, w [B,n] fp32: integers in [1, 8] and one key of weight n // 2 per image (at
    least 1), out [B,n,H*64] / lse [B,H,n] float64, their bounds); built once per shape and left unchanged"""
    key = (n, H)
    if key in _CACHE:
        return _CACHE[key]
    B = KEYW_B
    gen = torch.Generator().manual_seed(7000 + 10 * n + H)
    qkv = torch.randn((B, n, 3, H, DH), generator=gen).bfloat16().float()
    w = torch.randint(1, 9, (B, n), generator=gen).float()
    heavy = torch.randint(0, n, (B,), generator=gen)
    w[torch.arange(B), heavy] = float(max(n // 2, 1))
    q, k, v = (qkv[:, :, i].double().transpose(1, 2) for i in range(3))                   # [B,H,n,64]
    S = (q @ k.transpose(-1, -2)) * SCALE + torch.log(w.double())[:, None, None, :]
    lse = torch.logsumexp(S, dim=-1)                                                       # [B,H,n]
    Pw = torch.exp(S - lse[..., None])
    out = (Pw @ v).transpose(1, 2).reshape(B, n, H * DH)
    out_bound = ((2 * U16 + 2 * (n + 3) * U) * (Pw @ v.abs())).transpose(1, 2).reshape(B, n, H * DH)
    T = SCALE * (q.abs() @ k.abs().transpose(-1, -2)).max(dim=-1).values                   # [B,H,n]
    case = dict(qkv=qkv, w=w, out=out, lse=lse, out_bound=out_bound,
                out16_bound=out_bound + 2 * U16 * (out.abs() + out_bound),
                lse_bound=2 * (64 + n + 3) * U * (1.0 + lse.abs() + T))
    _CACHE[key] = case
    return case


def fractions(case, out, out16, lse):
    """worst error / bound of the three outputs (tensors on the CPU, any float dtype)"""
    B, n = case["w"].shape
    fr = {}
    if out is not None:
        fr["out"] = float(((out.double().reshape(B, n, -1) - case["out"]).abs() / case["out_bound"].clamp_min(1e-300)).max())
    fr["out_bf16"] = float(((out16.double().reshape(B, n, -1) - case["out"]).abs() / case["out16_bound"].clamp_min(1e-300)).max())
    fr["lse"] = float(((lse.double() - case["lse"]).abs() / case["lse_bound"]).max())
    return fr


def emulate_kernel(case):
    """The kernel's roundings on the CPU: inputs are bf16 values already; scores by an fp32 product of q * scale (exact: scale = 2^-3) and
    k; fp32 e = exp(S - max) with the maximum over the raw scores; p = fl32(e * w); p rounded to bf16 for the numerator, which is then
    accumulated in float64 from the rounded p and the bf16 v (the matrix core's fp32 accumulation is inside the n-term allowance); the
    denominator is the fp32 sum of the UNROUNDED p; lse = max + log(denominator) in fp32.  -> (out fp32, out16 bf16, lse fp32)"""
    qkv, w = case["qkv"], case["w"]
    B, n, _, H, _ = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))                            # fp32 [B,H,n,64]
    S = (q * SCALE) @ k.transpose(-1, -2)
    mx = S.max(dim=-1, keepdim=True).values
    p = torch.exp(S - mx) * w[:, None, None, :]                                            # fp32, one rounding for the product
    den = p.sum(dim=-1, keepdim=True)                                                      # fp32
    num = p.bfloat16().double() @ v.double()
    out = (num / den.double()).float().transpose(1, 2).reshape(B, n, H * DH)
    lse = (mx + torch.log(den)).squeeze(-1)
    return out, out.bfloat16(), lse
