"""Inputs, float64 reference, bounds and emulation of the key-weighted attention backward on the bf16 matrix cores (d2s_attn_keyw_bwd_bf16,
DESIGN.md section 22), shared by tests/test_tome_train_bf16_gpu.py (the kernels against float64) and tests/test_tome_train_bf16_cpu.py (the
emulation of the kernels' roundings against the same bounds, so that the bounds are not fixed blind).  Plain torch on the CPU.

Inputs: tome_bf16_cases.keyw_case(n, H) - B = 2, bf16-valued qkv, integer weights in [1, 8] and one key of weight n // 2 - and a seeded
randn dout [B, n, H*64].

Reference: Pw = softmax(S + log w), out = Pw v, dqkv = autograd of sum(out * dout) in float64 with the weights constant.

Bounds, per element: those of attention_bf16_ref.reference with P replaced by Pw and every fp32 chain one operation longer for the weight
product (U = 2^-24, U16 = 2^-9):
    dV   (4 U16 + 2 (n + 3) U)  sum_i Pw_ij |dO_id|           + sum_i r_ij Pw_ij |dO_id|
    dQ   scale ((6 U16 + 2 (n + 67) U) sum_j W_ij |k_jd|      + sum_j W'_ij |k_jd|)
    dK   scale ((6 U16 + 2 (n + 67) U) sum_i W_ij |q_id|      + sum_i W'_ij |q_id|)
with that module's r_ij = 2 (64 + 2) U (T_ij + max_j' T_ij'), W_ij = Pw_ij (A_ij + D_i) and W'_ij = r_ij W_ij + Pw_ij D'_i.

Emulation (the kernels' roundings, float64 otherwise; rb = round to bf16): out and lse from tome_bf16_cases.emulate_kernel (the forward's
own), delta = dO . out with the unrounded dO, P~ = fl32(exp(S - lse) w), dS = rb(P~ (rb(dO) v^T - delta)), dV = rb(P~)^T rb(dO),
dQ = scale dS k, dK = scale dS^T q.  weighted=False leaves the weight product out of P~ (what a backward that forgot the weights would
compute from the weighted forward's lse): the test of the test.
"""
import torch

from tests import tome_bf16_cases as C
from tests.attention_bf16_ref import rb

U, U16, DH, SCALE = C.U, C.U16, C.DH, C.SCALE
SHAPES = C.KEYW_SHAPES
_REF, _EMU = {}, {}


def dout_of(n, H):
    return torch.randn((C.KEYW_B, n, H * DH), generator=torch.Generator().manual_seed(7100 + 10 * n + H))


def _heads(t, B, n, H):
    """[B, n, H*64] -> [B, H, n, 64]"""
    return t.reshape(B, n, H, DH).permute(0, 2, 1, 3)


def reference(n, H):
    """-> dict(dq, dk, dv and their bounds, each [B, H, n, 64] float64); built once per shape and left unchanged"""
    key = (n, H)
    if key in _REF:
        return _REF[key]
    case = C.keyw_case(n, H)
    B = C.KEYW_B
    x = case["qkv"].double().requires_grad_(True)                                          # [B,n,3,H,64]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                               # [B,H,n,64]
    dO = _heads(dout_of(n, H).double(), B, n, H)
    logw = torch.log(case["w"].double())[:, None, None, :]
    Pw = torch.softmax((q @ k.transpose(-1, -2)) * SCALE + logw, dim=-1)
    dqkv, = torch.autograd.grad(((Pw @ v) * dO).sum(), [x])
    with torch.no_grad():
        q, k, v, Pw = q.detach(), k.detach(), v.detach(), Pw.detach()
        dq, dk, dv = (dqkv[:, :, i].transpose(1, 2).contiguous() for i in range(3))
        T = SCALE * (q.abs() @ k.abs().transpose(-2, -1))
        r = 2 * (64 + 2) * U * (T + T.max(dim=-1, keepdim=True)[0])
        m_out = Pw @ v.abs()
        A = dO.abs() @ v.abs().transpose(-2, -1)
        D = (dO.abs() * m_out).sum(-1, keepdim=True)
        W = Pw * (A + D)
        Pr = Pw * r
        D1 = (dO.abs() * (Pr @ v.abs())).sum(-1, keepdim=True)
        W1 = r * W + Pw * D1
        c_v, c_qk = 4 * U16 + 2 * (n + 3) * U, 6 * U16 + 2 * (n + 67) * U
        ref = dict(dq=dq, dk=dk, dv=dv,
                   dq_bound=SCALE * (c_qk * (W @ k.abs()) + W1 @ k.abs()),
                   dk_bound=SCALE * (c_qk * (W.transpose(-2, -1) @ q.abs()) + W1.transpose(-2, -1) @ q.abs()),
                   dv_bound=c_v * (Pw.transpose(-2, -1) @ dO.abs()) + Pr.transpose(-2, -1) @ dO.abs())
    _REF[key] = ref
    return ref


def emulate(n, H, weighted=True):
    key = (n, H, weighted)
    if key in _EMU:
        return _EMU[key]
    case = C.keyw_case(n, H)
    B = C.KEYW_B
    out32, _, lse32 = C.emulate_kernel(case)
    q, k, v = (case["qkv"][:, :, i].double().transpose(1, 2) for i in range(3))
    dO = _heads(dout_of(n, H).double(), B, n, H)
    out = _heads(out32.double(), B, n, H)
    delta = (dO * out).sum(-1, keepdim=True)
    S = (q @ k.transpose(-1, -2)) * SCALE
    Pt = torch.exp(S - lse32.double()[..., None]).float()
    if weighted:
        Pt = Pt * case["w"][:, None, None, :]                                             # fp32 product: one rounding
    Pt = Pt.double()
    dO16 = rb(dO)
    dS = rb(Pt * (dO16 @ v.transpose(-1, -2) - delta))
    emu = dict(dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-1, -2) @ q), dv=rb(Pt).transpose(-1, -2) @ dO16)
    _EMU[key] = emu
    return emu


def fractions(got, ref):
    """{dq, dk, dv: max |got - ref| / bound}; got [B, H, n, 64]"""
    return {k: float(((got[k].double() - ref[k]).abs() / ref[k + "_bound"].clamp_min(1e-300)).max()) for k in ("dq", "dk", "dv")}


def split_dqkv(dqkv, n, H):
    """a kernel's dqkv [B * n, 3 * H * 64] (any float dtype, on the CPU) -> dict(dq, dk, dv [B, H, n, 64])"""
    t = dqkv.reshape(C.KEYW_B, n, 3, H, DH)
    return {name: t[:, :, i].transpose(1, 2) for i, name in enumerate(("dq", "dk", "dv"))}
