"""Dense bf16 attention (d2s_attn_fwd_bf16 / d2s_attn_bwd_bf16 and their _bf16out forms): inputs, a float64 reference, derived per-element
bounds and a float64 emulation of the kernels' bf16 roundings.  Plain torch and numpy on the CPU; scale = 2^-3 throughout.

The kernels round q * scale, k and v to bf16.  The scale is a power of two, so that is the rounding of q itself: the inputs here hold
bf16 values, the reference is evaluated on them and they carry no error.

Inputs (inputs(B, H, n, kind)): qkv [B*n, 3*H*64] fp32 holding bf16 values, std 0.7, and dout [B*n, H*64], std 1.0, from d2s.synth.
    normal  as drawn: the running maximum of the online softmax moves in most key tiles for some query of every wave.
    sink    key 0 dominates every row - the attention sink of a ViT's CLS token: with one unit direction u per image and head, every q gets
            + 4 u and key 0 gets + 16 u (scale * 4 * 16 = 8 more on column 0 of the scores), rounded to bf16 afterwards.  The maximum is
            final after the first tile, so the 64-key kernel's "no lane changed its maximum" branch is taken in every later tile; random
            inputs take it with probability (t / (t + 1))^32 per wave, i.e. almost never.
    last    the same with key n - 1: the maximum changes in the last, partial tile and the dominant probability sits on the tail key.
reference() asserts argmax_j S_ij = 0 (sink) / n - 1 (last) for every row and max |S| < 30, on the float64 scores.

Reference: S = scale q k^T, P = softmax(S), out = P v, lse = logsumexp(S), the CLS row P[:, :, 0, :], and dqkv = autograd of
sum(out * dout), all float64.

Bounds, per element: the model of tests/test_policy_attention_bf16_gpu.py with mk = 1, eps = 0, cinv = 0.  U = 2^-24, U16 = 2^-9.  Every
output element is a sum of leaf products; c counts the bf16-rounded factors of a leaf and is doubled once (bf16 keeps 8 significant bits: one
rounding is off by at most 2^-8 = 2 U16 relative), and a chain of L fp32 operations adds 2 (L + 2) U, both times the sum of |leaves|:
    out_i[d]  = sum_j P_ij v_jd               c = 1 (e, the unnormalised P, is rounded)    L = n       M = M_out = sum_j P_ij |v_jd|
    dV_j[d]   = sum_i P_ij dO_id              c = 2 (P~ = exp(S - lse) and dO are rounded) L = n       M = sum_i P_ij |dO_id|
    dS_ij     = P_ij (dP_ij - delta_i),  dP_ij = sum_d dO_id v_jd,  delta_i = sum_d dO_id out_id
                |dS_ij| <= W_ij = P_ij (A_ij + D_i),  A_ij = sum_d |dO_id| |v_jd|,  D_i = sum_d |dO_id| M_out_id  (out is the forward's own:
                its error is relative to M_out, not to |out|)
    dQ_i[d]   = scale sum_j dS_ij k_jd        c = 3 (dS is rounded; inside it dO is rounded in dP, and delta reads the forward's out, which
                                              carries e's rounding)                         L = n + 64  M = scale sum_j W_ij |k_jd|
    dK_j[d]   = scale sum_i dS_ij q_id        c = 3 (the same three)                        L = n + 64  M = scale sum_i W_ij |q_id|
    cls_row_j = P_0j                          c = 0.  The exponent's argument is a 64-term fp32 dot product, absolute error (64 + 2) U T_0j
                with T_ij = scale sum_d |q_id k_jd|; that is the relative error of e_0j, and l_0 is an n-term sum of such values:
                |err| <= 2 (64 + n + 2) U P_0j (1 + T_0j + max_j' T_0j')
    lse_i     = m_i + log(l_i)                c = 0: l sums the unrounded exponentials.  The fp32 error of the 64-term score under the
                maximum, the n-term sum (an error relative to l is an absolute error of log l), logf and the final add, which is relative to
                |lse_i|:  |err| <= 2 (64 + n + 2) U (1 + max_j T_ij + |lse_i|)
The fp32 error of the score under the exponential is not a bf16 rounding and does not shrink with n, so it is a term of its own rather than
slack: S_ij is off by (64 + 2) U T_ij and lse_i by at most the largest of those, hence P_ij is off by the relative error
    r_ij = 2 (64 + 2) U (T_ij + max_j' T_ij')
and that goes through the same absolute-value sums: out + sum_j r_ij P_ij |v_jd|,  dV + sum_i r_ij P_ij |dO_id|, and |dS_ij| moves by
r_ij W_ij (its factor P_ij) plus P_ij D'_i (delta_i through out), D'_i = sum_d |dO_id| sum_j r_ij P_ij |v_jd|, so with W'_ij = r_ij W_ij +
P_ij D'_i:  dQ + scale sum_j W'_ij |k_jd|,  dK + scale sum_i W'_ij |q_id|.  With sink and last inputs it is about 5 % of one bf16 rounding.

Emulation (emulate()): the same computation in float64 with exactly the bf16 roundings of csrc/attention_bf16.hip - the yardstick of the
relative-L2 test, and the evidence that the reference alone meets the bounds.  rb() below is a round-to-nearest-even to bf16:
    forward   e = exp(S - m) against the row maximum; l = sum_j e_ij unrounded; out = (rb(e) v) / l; lse = m + log l   (pf = (__bf16)s)
    delta     delta_i = sum_d dO_id out_id with the unrounded dO and the emulated out                                  (d2s_attn_delta)
    dP        rb(dO) v^T                                                                                               (dof / Ds)
    dS        P~ (dP - delta), P~ = exp(S - lse) with the emulated lse; rb(dS) multiplies K (dQ) and Q (dK)            (pack2(s) / pack2(dp))
    dV        rb(P~)^T rb(dO)                                                                                          (pack2(s), Dt)
    q, k, v are bf16 already; the two scale multiplies (2^-3) are exact.
What it does not emulate: the running maximum (the kernel rounds e against the maximum so far and rescales the accumulator, so its e sit at
other positions of their binades - the same error distribution, other individual values) and the fp32 chains.
"""
import numpy as np
import torch

U, U16 = 2.0 ** -24, 2.0 ** -9
DH = 64
SCALE = 0.125
KINDS = ("normal", "sink", "last")
# the edges of 32-key tiles, 64-key tiles and 128-query workgroups
SHAPES = [(2, 2, 1), (2, 2, 2), (2, 2, 17), (2, 2, 31), (2, 2, 32), (2, 2, 33), (2, 2, 63), (2, 2, 64), (2, 2, 65), (2, 3, 96), (2, 3, 97),
          (2, 2, 127), (2, 2, 128), (2, 2, 129), (1, 6, 197), (1, 2, 257), (1, 2, 384), (1, 2, 577)]
CASES = [(B, H, n, kind) for (B, H, n) in SHAPES for kind in KINDS]
OUTPUTS = ("out", "lse", "cls_row", "dq", "dk", "dv")
L2_OUTPUTS = ("out", "dq", "dk", "dv")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rb(x):
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    return x.float().bfloat16().double()


def inputs(B, H, n, kind):
    """bf16-valued qkv [B*n, 3*H*64] fp32 and dout [B*n, H*64] fp32 of one case"""
    from d2s import synth
    assert kind in KINDS
    tag = f"da16/{B}/{H}/{n}"
    qkv = _t(synth.normal(tag + "/qkv", (B * n, 3 * H * DH), std=0.7, seed=3)).double().view(B, n, 3, H, DH).clone()
    dout = _t(synth.normal(tag + "/go", (B * n, H * DH), std=1.0, seed=5))
    if kind != "normal":
        u = _t(synth.normal(tag + "/u", (B, H, DH), seed=6)).double()
        u = u / u.norm(dim=-1, keepdim=True)
        qkv[:, :, 0] += 4.0 * u.view(B, 1, H, DH)
        qkv[:, 0 if kind == "sink" else n - 1, 1] += 16.0 * u
    return qkv.view(B * n, 3 * H * DH).float().bfloat16().float().contiguous(), dout


def split(t, B, H, n):
    """[B*n, 3*H*64] -> q, k, v, each [B, H, n, 64]"""
    return t.reshape(B, n, 3, H, DH).permute(2, 0, 3, 1, 4)


def heads(t, B, H, n):
    """[B*n, H*64] -> [B, H, n, 64]"""
    return t.reshape(B, n, H, DH).permute(0, 2, 1, 3)


def rows(t, B, H, n):
    """[B, H, n, 64] -> [B*n, H*64]"""
    return t.permute(0, 2, 1, 3).reshape(B * n, H * DH)


_REF = {}


def reference(B, H, n, kind):
    """float64 attention on the bf16-valued inputs, its autograd, and the bounds of the module docstring; computed once per case, shared
    and never modified.  out / dq / dk / dv and their bounds are [B, H, n, 64]; lse, cls_row [B, H, n]"""
    key = (B, H, n, kind)
    if key in _REF:
        return _REF[key]
    qkv, dout = inputs(B, H, n, kind)
    x = qkv.double().requires_grad_(True)
    q, k, v = split(x, B, H, n)
    dO = heads(dout.double(), B, H, n)
    S = (q @ k.transpose(-2, -1)) * SCALE
    P = torch.softmax(S, dim=-1)
    out = P @ v
    dqkv, = torch.autograd.grad((out * dO).sum(), [x])
    with torch.no_grad():
        q, k, v, S, P, out = q.detach(), k.detach(), v.detach(), S.detach(), P.detach(), out.detach()
        arg = S.argmax(dim=-1)
        if kind == "sink":
            assert bool((arg == 0).all()), "sink: key 0 must hold every row's maximum"
        if kind == "last":
            assert bool((arg == n - 1).all()), "last: key n - 1 must hold every row's maximum"
        smax = float(S.abs().max())
        assert smax < 30.0, smax
        lse = torch.logsumexp(S, dim=-1)
        dq, dk, dv = split(dqkv, B, H, n)
        T = SCALE * (q.abs() @ k.abs().transpose(-2, -1))                     # [B, H, n(i), n(j)]
        Tmax = T.max(dim=-1, keepdim=True)[0]
        r = 2 * (64 + 2) * U * (T + Tmax)                                     # relative error of P_ij from the fp32 score
        m_out = P @ v.abs()
        A = dO.abs() @ v.abs().transpose(-2, -1)
        D = (dO.abs() * m_out).sum(-1, keepdim=True)
        W = P * (A + D)
        Pr = P * r
        D1 = (dO.abs() * (Pr @ v.abs())).sum(-1, keepdim=True)
        W1 = r * W + P * D1
        c_o, c_v, c_qk = 2 * 1 * U16 + 2 * (n + 2) * U, 2 * 2 * U16 + 2 * (n + 2) * U, 2 * 3 * U16 + 2 * (n + 64 + 2) * U
        ref = dict(
            S=S, P=P, smax=smax,
            out=out, out_bound=c_o * m_out + Pr @ v.abs(),
            lse=lse, lse_bound=2 * (64 + n + 2) * U * (1.0 + Tmax[..., 0] + lse.abs()),
            cls_row=P[:, :, 0], cls_row_bound=2 * (64 + n + 2) * U * P[:, :, 0] * (1.0 + T[:, :, 0] + Tmax[:, :, 0]),
            dq=dq.contiguous(), dq_bound=SCALE * (c_qk * (W @ k.abs()) + W1 @ k.abs()),
            dk=dk.contiguous(), dk_bound=SCALE * (c_qk * (W.transpose(-2, -1) @ q.abs()) + W1.transpose(-2, -1) @ q.abs()),
            dv=dv.contiguous(), dv_bound=c_v * (P.transpose(-2, -1) @ dO.abs()) + Pr.transpose(-2, -1) @ dO.abs())
    _REF[key] = ref
    return ref


def closed_form(B, H, n, kind):
    """dq, dk, dv [B, H, n, 64] from dS = P (dP - delta) in float64: what the kernels evaluate, without any rounding"""
    ref = reference(B, H, n, kind)
    qkv, dout = inputs(B, H, n, kind)
    q, k, v = split(qkv.double(), B, H, n)
    dO = heads(dout.double(), B, H, n)
    P = ref["P"]
    dS = P * (dO @ v.transpose(-2, -1) - (dO * ref["out"]).sum(-1, keepdim=True))
    return dict(dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-2, -1) @ q), dv=P.transpose(-2, -1) @ dO)


_EMU = {}


def emulate(B, H, n, kind):
    """the kernels' computation in float64 with their bf16 roundings (module docstring); same layout as reference()"""
    key = (B, H, n, kind)
    if key in _EMU:
        return _EMU[key]
    qkv, dout = inputs(B, H, n, kind)
    q, k, v = split(qkv.double(), B, H, n)
    dO = heads(dout.double(), B, H, n)
    S = (q @ k.transpose(-2, -1)) * SCALE
    m = S.max(dim=-1, keepdim=True)[0]
    e = (S - m).exp()
    l = e.sum(dim=-1, keepdim=True)
    out = (rb(e) @ v) / l
    lse = m + l.log()
    delta = (dO * out).sum(-1, keepdim=True)
    Pt = (S - lse).exp()
    dO16 = rb(dO)
    dS = rb(Pt * (dO16 @ v.transpose(-2, -1) - delta))
    emu = dict(out=out, lse=lse[..., 0], cls_row=(e / l)[:, :, 0], dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-2, -1) @ q),
               dv=rb(Pt).transpose(-2, -1) @ dO16)
    _EMU[key] = emu
    return emu


def bound_fractions(got, ref):
    """{output: max |got - ref| / bound}"""
    return {name: float(((got[name].double() - ref[name]).abs() / ref[name + "_bound"]).max()) for name in OUTPUTS}


def l2_errors(got, ref, name):
    """per (b, h) slice: (|got - ref|_2, |ref|_2), each [B, H]"""
    d = (got[name].double() - ref[name]).flatten(2).norm(dim=-1)
    return d, ref[name].flatten(2).norm(dim=-1)


def l2_floor(n):
    """the fp32 chains, relative to the slice's norm"""
    return 2 * (n + 64 + 2) * U
