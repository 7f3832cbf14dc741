"""Policy attention on the bf16 matrix cores (d2s_attn_policy_fwd_bf16 / d2s_attn_policy_bwd_bf16) and the routes that reach it: the
anchor to the plain bf16 kernels, a float64 restatement with derived per-element bounds, the bit-level consistency of the entry's forms,
its argument checks, a policy block and the two policy training paths in the bf16 arithmetic mode.

Bounds of the float64 comparison (section 2), per element: c 2^-9 sum |leaves| with c doubled once, plus the fp32 chain term
2 (L + 2) 2^-24 sum |leaves| of tests/test_dynamicvit_gpu.py.  The reference is evaluated on the bf16-rounded q, k, v, so those carry no
error.  Every output element is a sum of leaf products and c counts the bf16-rounded factors of a leaf.  bf16 keeps 8 significant bits,
so one rounding is off by at most 2^-8 = 2 * 2^-9 relative: the doubled count is the worst case of the c roundings themselves.  What is
not a bf16 rounding - v_exp_f32, the log2-domain FMA, the fp32 error of the 64-term score under the exponential, each a few 1e-5 relative
at these magnitudes - has to fit into the chain term and into the distance of the actual roundings from their worst case (a CPU emulation
of the kernel's roundings with exact exponentials reaches 0.96 of the out bound and 0.93 of the dV bound on the CLS-only image, whose rows
have two live keys; the sums over many keys stay below 0.6).
    out_i[d]    = sum_j P_ij v_jd                       c = 1 (P, the masked e, is rounded),          L = n,      M = sum_j P_ij |v_jd|
    dV_j[d]     = sum_i (P~_ij mk_ij + cinv_i) dO_id    c = 2 (that sum is rounded, and dO),          L = n,      M = sum_i P_ij |dO_id|
    dS_ij       = P~_ij mk_ij (dP_ij - delta_i), dP_ij = sum_d dO_id v_jd, delta_i = sum_d dO_id out_id
                  |dS_ij| <= W_ij = P~_ij mk_ij (A_ij + D_i),  A_ij = sum_d |dO_id| |v_jd|,  D_i = sum_d |dO_id| M_out_id
                  (out is the forward's: its error is u16-relative to M_out, not to |out|)
    dQ_i[d]     = scale sum_j dS_ij k_jd                c = 3 (dS is rounded; inside it dO is rounded in dP, and delta reads the forward's
                                                        out, which carries P's rounding),            L = n + 64, M = scale sum_j W_ij |k_jd|
    dK_j[d]     = scale sum_i dS_ij q_id                c = 3 (the same three),                       L = n + 64, M = scale sum_i W_ij |q_id|
    dpolicy_bj  = sum_h sum_{i != j} P~_ij (dP_ij - delta_i)   c = 1 (nothing is rounded but dO in dP / P inside out: one per leaf),
                                                        L = H (n - 1) + 64,                           M = sum_h sum_{i != j} P~_ij (A_ij + D_i)
    cls_row_j   = (e_0j mk_0j + eps/n) / (l_0 + eps)    c = 0: no bf16 rounding at all.  The exponent's argument is a 64-term fp32 dot
                  product (absolute error (64 + 2) u T_0j, T_0j = scale sum_d |q_0d k_jd|, which is the relative error of e_0j), l_0 is an
                  n-term sum of such values: to first order |err| <= 2 (64 + n + 2) u P_0j (1 + T_0j + max_j' T_0j').
"""
import numpy as np
import pytest
import torch

from tests import cases
from tests import dynamicvit_cases as DC
from tests import dynamicvit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, U16 = 2.0 ** -24, 2.0 ** -9
DH = 64
SCALE = DH ** -0.5
SHAPES = [(2, 2, 17), (2, 2, 33), (3, 2, 64), (2, 3, 99), (1, 6, 197), (1, 2, 577)]
KINDS = ["uniform", "binary", "ones", "single"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(B, H, n, kind):
    """bf16-rounded qkv [B*n, 3*H*64] (fp32 holding bf16 values), dout [B*n, H*64], policy [B, n] - all from d2s.synth"""
    from d2s import synth
    tag = f"pa16/{B}/{H}/{n}"
    qkv = _t(synth.normal(tag + "/qkv", (B * n, 3 * H * DH), std=0.7, seed=3)).bfloat16().float()
    dout = _t(synth.normal(tag + "/go", (B * n, H * DH), std=1.0, seed=5))
    r = _t(synth.normal(tag + "/pol/" + kind, (B, n), seed=4))
    if kind == "uniform":
        pol = (0.5 * (1.0 + torch.erf(r / 2 ** 0.5))).clamp(1e-3, 1 - 1e-3)          # real values in (0, 1)
    elif kind == "ones":
        pol = torch.ones(B, n)
    else:
        pol = (r > 0.3).float()
        if kind == "single":                                                          # one image keeps only CLS
            pol[0] = 0.0
    pol[:, 0] = 1.0
    return qkv, dout, pol.float().contiguous()


_REF = {}


def _reference(B, H, n, kind, eps=1e-6):
    """float64 restatement (max detached) on the bf16-rounded q, k, v, its autograd, and the magnitude sums of the module docstring;
    computed once per case and shared"""
    key = (B, H, n, kind)
    if key in _REF:
        return _REF[key]
    qkv, dout, pol = _inputs(B, H, n, kind)
    x = qkv.double().view(B, n, 3 * H * DH).requires_grad_(True)
    p = pol.double().requires_grad_(True)
    q, k, v = x.reshape(B, n, 3, H, DH).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    eye = torch.eye(n, dtype=torch.float64).view(1, 1, n, n)
    mk = p.reshape(B, 1, 1, n)
    mk = mk + (1.0 - mk) * eye
    eu = (s - s.max(dim=-1, keepdim=True)[0].detach()).exp()
    e = eu * mk
    l = e.sum(dim=-1, keepdim=True)
    P = (e + eps / n) / (l + eps)
    out = (P @ v).transpose(1, 2).reshape(B, n, H * DH)
    np.testing.assert_allclose(out.detach().numpy(), R.policy_attention(x.detach(), p.detach(), H, SCALE, eps).numpy(), rtol=1e-12, atol=1e-14)
    dO = dout.double().view(B, n, H, DH).permute(0, 2, 1, 3)
    dqkv, dpol = torch.autograd.grad((out * dout.double().view(B, n, H * DH)).sum(), [x, p])
    with torch.no_grad():
        q, k, v, P, Pm, Pu = q.detach(), k.detach(), v.detach(), P.detach(), (e / (l + eps)).detach(), (eu / (l + eps)).detach()
        m_out = P @ v.abs()                                                   # [B, H, n, 64]
        A = dO.abs() @ v.abs().transpose(-2, -1)                              # [B, H, n(i), n(j)]
        D = (dO.abs() * m_out).sum(-1, keepdim=True)                          # [B, H, n, 1]
        W = Pm * (A + D)
        m_dq, m_dk, m_dv = SCALE * (W @ k.abs()), SCALE * (W.transpose(-2, -1) @ q.abs()), P.transpose(-2, -1) @ dO.abs()
        m_dpol = (Pu * (A + D) * (1.0 - eye)).sum(dim=(1, 2))                 # [B, n]
        T0 = SCALE * (q[:, :, :1].abs() @ k.abs().transpose(-2, -1))[:, :, 0]          # [B, H, n]
        lay = lambda a, b_, c: torch.stack([a, b_, c]).permute(1, 3, 0, 2, 4).reshape(B * n, 3 * H * DH)
        c_qk = 2 * 3 * U16 + 2 * (n + 64 + 2) * U
        ref = dict(
            out=out.detach().reshape(B * n, H * DH),
            out_bound=((2 * 1 * U16 + 2 * (n + 2) * U) * m_out).transpose(1, 2).reshape(B * n, H * DH),
            cls=P[:, :, 0], cls_bound=2 * (64 + n + 2) * U * P[:, :, 0] * (1.0 + T0 + T0.max(dim=-1, keepdim=True)[0]),
            dqkv=dqkv.reshape(B * n, 3 * H * DH),
            dqkv_bound=lay(c_qk * m_dq, c_qk * m_dk, (2 * 2 * U16 + 2 * (n + 2) * U) * m_dv),
            dpol=dpol, dpol_bound=(2 * 1 * U16 + 2 * (H * (n - 1) + 64 + 2) * U) * m_dpol)
    _REF[key] = ref
    return ref


def _fwd_bwd(ops, qkv, pol, dout, B, H, n, eps=1e-6, want_dpolicy=True, dqkv16=None, want_f32=True):
    out, lse, cinv, cls_row, out16 = ops.attn_policy_fwd_bf16io(qkv, pol, B, n, H, SCALE, eps=eps, want_cls=True)
    dqkv, dpol = ops.attn_policy_bwd_bf16io(qkv, pol, out, dout, lse, cinv, B, n, H, SCALE, dqkv16=dqkv16, want_f32=want_f32,
                                            want_dpolicy=want_dpolicy)
    return dict(out=out, lse=lse, cinv=cinv, cls=cls_row, out16=out16, dqkv=dqkv, dpol=dpol, dqkv16=dqkv16)


# ---- 1. anchor ----
@pytest.mark.parametrize("B,H,n", [(2, 2, 17), (1, 6, 197)])
def test_all_ones_policy_and_eps_zero_is_the_plain_bf16_kernel_bit_for_bit(B, H, n):
    """n = 17 and 197 are sizes at which d2s_attn_fwd_bf16_bf16out takes the 32-key-tile kernel the policy form is built from"""
    from d2s import ops
    qkv, dout, pol = _inputs(B, H, n, "ones")
    qkv, dout, pol = qkv.to(DEV), dout.to(DEV), pol.to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        for src in (qkv, qkv.bfloat16()):
            out, lse, cls_row, out16 = ops.attn_fwd_bf16io(src, B, n, H, SCALE, want_cls=True)
            pout, plse, pcinv, pcls, pout16 = ops.attn_policy_fwd_bf16io(src, pol, B, n, H, SCALE, eps=0.0, want_cls=True)
            assert torch.equal(pout, out) and torch.equal(pout16, out16) and torch.equal(plse, lse) and torch.equal(pcls, cls_row)
            assert float(pcinv.abs().max()) == 0.0
            d16, p16 = torch.empty_like(src, dtype=torch.bfloat16), torch.empty_like(src, dtype=torch.bfloat16)
            dqkv = ops.attn_bwd(src, out, dout, lse, B, n, H, SCALE, dqkv16=d16)
            pdqkv, _ = ops.attn_policy_bwd_bf16io(src, pol, out, dout, lse, torch.zeros_like(lse), B, n, H, SCALE, dqkv16=p16)
            assert torch.equal(pdqkv, dqkv) and torch.equal(p16, d16)


# ---- 2. float64 ----
@pytest.mark.parametrize("B,H,n", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_backward_against_float64(B, H, n, kind):
    from d2s import ops
    ref = _reference(B, H, n, kind)
    qkv, dout, pol = _inputs(B, H, n, kind)
    got = _fwd_bwd(ops, qkv.to(DEV), pol.to(DEV), dout.to(DEV), B, H, n)
    torch.cuda.synchronize()
    fracs = {}
    for name, g, want, bound in (("out", got["out"], ref["out"], ref["out_bound"]), ("cls_row", got["cls"], ref["cls"], ref["cls_bound"]),
                                 ("dqkv", got["dqkv"], ref["dqkv"], ref["dqkv_bound"])):
        g = g.cpu().double()
        assert torch.isfinite(g).all(), name
        fracs[name] = float(((g - want).abs() / bound).max())
    dq = got["dqkv"].cpu().double().view(B * n, 3, H * DH)
    for i, part in enumerate(("dq", "dk", "dv")):
        fracs[part] = float(((dq[:, i] - ref["dqkv"].view(B * n, 3, -1)[:, i]).abs() / ref["dqkv_bound"].view(B * n, 3, -1)[:, i]).max())
    gp = got["dpol"].cpu().double()
    assert torch.all(gp[:, 0] == 0) and torch.isfinite(gp).all()
    fracs["dpolicy"] = float(((gp - ref["dpol"])[:, 1:].abs() / ref["dpol_bound"][:, 1:]).max())
    print(f"policy attention bf16 B{B} H{H} n{n} {kind}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
    for k, v in fracs.items():
        assert v <= 1.0, (k, v)
    if kind in ("binary", "single"):      # a masked key keeps its gradient: the straight-through signal
        masked = pol[:, 1:] == 0
        assert masked.any() and float(gp[:, 1:][masked].abs().max()) > 0


# ---- 3. consistency ----
@pytest.mark.parametrize("B,H,n", SHAPES)
def test_forms_of_the_entry_agree_bit_for_bit(B, H, n):
    from d2s import ops
    kind = "binary" if n % 2 else "uniform"
    qkv, dout, pol = _inputs(B, H, n, kind)
    qkv, dout, pol = qkv.to(DEV), dout.to(DEV), pol.to(DEV)
    h = lambda: torch.empty_like(qkv, dtype=torch.bfloat16)
    a = _fwd_bwd(ops, qkv, pol, dout, B, H, n, dqkv16=h())
    b = _fwd_bwd(ops, qkv.bfloat16(), pol, dout, B, H, n, dqkv16=h())                 # qkv in bf16
    again = _fwd_bwd(ops, qkv, pol, dout, B, H, n, dqkv16=h())                         # a second launch
    nodp = _fwd_bwd(ops, qkv, pol, dout, B, H, n, want_dpolicy=False, dqkv16=h())      # without dpolicy
    only16 = _fwd_bwd(ops, qkv, pol, dout, B, H, n, dqkv16=h(), want_f32=False)        # dqkv == NULL
    fwd16 = ops.attn_policy_fwd_bf16io(qkv, pol, B, n, H, SCALE, want_cls=True, want_f32=False)      # out == NULL
    torch.cuda.synchronize()
    for k in ("out", "lse", "cinv", "cls", "out16", "dqkv", "dpol", "dqkv16"):
        assert torch.equal(a[k], b[k]), f"fp32 and bf16 qkv differ in {k}"
        assert torch.equal(a[k], again[k]), f"two launches differ in {k}"
    assert torch.equal(a["out16"], a["out"].bfloat16()) and torch.equal(a["dqkv16"], a["dqkv"].bfloat16())
    assert fwd16[0] is None and torch.equal(fwd16[4], a["out16"]) and torch.equal(fwd16[1], a["lse"]) and torch.equal(fwd16[3], a["cls"])
    assert only16["dqkv"] is None and torch.equal(only16["dqkv16"], a["dqkv16"]) and torch.equal(only16["dpol"], a["dpol"])
    assert nodp["dpol"] is None and torch.equal(nodp["dqkv"], a["dqkv"]) and torch.equal(nodp["dqkv16"], a["dqkv16"])
    assert torch.all(a["dpol"][:, 0] == 0)


# ---- 4. argument checks ----
def test_argument_checks():
    from d2s import lib
    B, H, n = 2, 2, 17
    f = lambda *s: torch.zeros(*s, device=DEV)
    qkv, pol, out, dout = f(B * n, 3 * H * DH), torch.ones(B, n, device=DEV), f(B * n, H * DH), f(B * n, H * DH)
    lse, cinv, delta, dqkv, dpol, ws = f(B, H, n), f(B, H, n), f(B, H, n), f(B * n, 3 * H * DH), f(B, n), f(B, H, n)
    P = lambda t: None if t is None else t.data_ptr()

    def fwd(policy=pol, out_=out, lse_=lse, cinv_=cinv, n_=n):
        lib.call("d2s_attn_policy_fwd_bf16", P(qkv), 0, P(policy), P(out_), None, P(lse_), P(cinv_), None, B, n_, H, SCALE, 1e-6)

    def bwd(policy=pol, lse_=lse, cinv_=cinv, dpol_=None, ws_=None, n_=n, dqkv_=dqkv):
        lib.call("d2s_attn_policy_bwd_bf16", P(qkv), 0, P(policy), P(out), P(dout), P(lse_), P(cinv_), P(dqkv_), None, P(delta), P(dpol_),
                 P(ws_), B, n_, H, SCALE)
    fwd()
    bwd()
    bwd(dpol_=dpol, ws_=ws)
    for bad in (dict(policy=None), dict(lse_=None), dict(cinv_=None), dict(n_=0), dict(out_=None)):
        with pytest.raises(lib.D2SError):
            fwd(**bad)
    for bad in (dict(policy=None), dict(lse_=None), dict(cinv_=None), dict(n_=0), dict(dpol_=dpol, ws_=None), dict(dqkv_=None)):
        with pytest.raises(lib.D2SError):
            bwd(**bad)
    torch.cuda.synchronize()


# ---- 5. a block ----
_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _block_case():
    from d2s import synth
    B, n, D, H, hid = 4, 99, 128, 2, 512
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hid, D), (hid,), (D, hid), (D,)]
    p = [_t(synth.normal(f"pa16/block/p{i}", s, std=0.05 if len(s) == 2 else 0.1, seed=11)) for i, s in enumerate(shapes)]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    x = _t(synth.normal("pa16/block/x", (B, n, D), seed=12))
    gy = _t(synth.normal("pa16/block/gy", (B, n, D), seed=13))
    pol = (_t(synth.normal("pa16/block/pol", (B, n), seed=14)) > 0.3).float()
    pol[0] = 0.0                                                                      # the CLS-only image
    pol[:, 0] = 1.0
    return B, n, D, H, hid, x, p, gy, pol.contiguous()


def _spy_calls(monkeypatch):
    from d2s import lib
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return names


def _run_policy_block(ops, x, p, gy, pol, H, pol_grad):
    from d2s import functional as DF
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in p]
    pold = None if pol is None else pol.to(DEV).requires_grad_(pol_grad)
    y, _ = DF.run(DF.BlockFn, xd, *pd, H, 1e-6, False, None, pold)
    grads = torch.autograd.grad(y, [xd] + pd + ([pold] if pol_grad else []), gy.to(DEV))
    ops.join_weight_grads()
    torch.cuda.synchronize()
    return y.detach().cpu(), [g.cpu() for g in grads]


def test_policy_block_in_bf16_mode_against_float64_and_takes_the_bf16_route(monkeypatch):
    from d2s import ops
    B, n, D, H, hid, x, p, gy, pol = _block_case()
    x64 = x.double().requires_grad_(True)
    sd = {"b." + k: t.double().requires_grad_(True) for k, t in zip(_NAMES, p)}
    pol64 = pol.double().requires_grad_(True)
    y64 = R.block(sd, "b.", x64, pol64, H)
    want = torch.autograd.grad(y64, [x64] + [sd["b." + k] for k in _NAMES] + [pol64], gy.double())
    names = _spy_calls(monkeypatch)
    with ops.gemm_mode(ops.GEMM_BF16):
        y, grads = _run_policy_block(ops, x, p, gy, pol, H, pol_grad=True)
        bf16_names = list(names)
        del names[:]
        y0, grads0 = _run_policy_block(ops, x, p, gy, pol, H, pol_grad=False)         # a constant mask: no dpolicy, the same dqkv
        const_names = list(names)
        del names[:]
        with torch.no_grad():
            from d2s import functional as DF
            y_ng, _ = DF.run(DF.BlockFn, x.to(DEV), *[t.to(DEV) for t in p], H, 1e-6, False, None, pol.to(DEV))
        fwd_only_names = list(names)
        del names[:]
        _run_policy_block(ops, x, p, gy, None, H, pol_grad=False)
        plain_names = list(names)
    del names[:]
    _run_policy_block(ops, x, p, gy, pol, H, pol_grad=True)
    exact_names = list(names)
    is_f32_policy = lambda s: "_policy_" in s and s.endswith("_f32")
    for got_names in (bf16_names, const_names):
        assert "d2s_attn_policy_fwd_bf16" in got_names and "d2s_attn_policy_bwd_bf16" in got_names
        assert not any(is_f32_policy(s) for s in got_names), got_names
    assert "d2s_attn_policy_fwd_bf16" in fwd_only_names and not any(is_f32_policy(s) for s in fwd_only_names)
    assert not any("_policy_" in s for s in plain_names) and "d2s_attn_fwd_bf16_bf16out" in plain_names
    assert "d2s_attn_policy_fwd_f32" in exact_names and "d2s_attn_policy_bwd_dpol_f32" in exact_names
    assert not any(s.startswith("d2s_attn_policy_") and s.endswith("_bf16") for s in exact_names)
    np.testing.assert_allclose(y.numpy(), y64.detach().float().numpy(), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(y_ng.cpu().numpy(), y64.detach().float().numpy(), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(grads[0].numpy(), want[0].float().numpy(), rtol=3e-2, atol=3e-2)
    assert torch.equal(y, y0) and all(torch.equal(a, b) for a, b in zip(grads[:13], grads0))
    for name, g, w in zip(_NAMES + ("policy",), grads[1:], want[1:]):
        assert torch.isfinite(g).all(), name
        w_ = w[:, 1:] if name == "policy" else w
        g_ = g[:, 1:] if name == "policy" else g
        err = float((g_.double() - w_).norm() / w_.norm())
        print(f"policy block bf16 d{name}: relative L2 error {err:.3e}")
        assert err <= 3e-2, (name, err)
    assert float(grads[-1][:, 0].abs().max()) == 0.0


# ---- 6. the two training paths ----
def _close(a, b, what):
    a, b = float(a), float(b)
    assert abs(a - b) <= max(3e-2 * abs(b), 2e-3), (what, a, b)


def test_dynamicvit_train_step_in_bf16_mode_tracks_the_exact_step(monkeypatch):
    from d2s import ops, synth
    from tests.test_dynamicvit_gpu import _build, _train_step
    case = DC.CASES["stage2"]
    cfg = case["cfg"]
    B, N, S = case["batch"], cfg["init_n"], len(cfg["pruning_loc"])
    x = _t(DC.make_images(case)).to(DEV)
    y = _t(synth.labels(B, cfg["num_classes"], seed=case["seed"])).to(DEV)
    noise = []
    for i in range(S):      # g0 - g1 = +-6, the sign from a synth draw: the decision is the noise's unless |logp0 - logp1| >= 6
        sign = torch.where(_t(synth.normal(f"pa16/noise{i}", (B, N), seed=case["seed"])) > 0, 3.0, -3.0)
        noise.append(torch.stack([sign, -sign], dim=-1).float())
    # precondition, in exact mode: |logp0 - logp1| < 1 on every token, so the margin of every decision is >= 5
    logps, real = [], ops.gumbel_keep_fwd

    def spy(z, g, prev):
        res = real(z, g, prev)
        logps.append(res[0].detach().clone())
        return res
    monkeypatch.setattr(ops, "gumbel_keep_fwd", spy)
    decs = {}
    for mode in (ops.GEMM_EXACT, ops.GEMM_BF16):
        m = _build(case).train()
        m.gumbel_noise = noise
        with ops.gemm_mode(mode):
            decs[mode] = [d.detach().clone() for d in m(x)[3]]
        if mode == ops.GEMM_EXACT:
            assert len(logps) == S
            for lp in logps:
                lp = lp.view(-1, 2)
                assert float((lp[:, 0] - lp[:, 1]).abs().max()) < 1.0
    monkeypatch.setattr(ops, "gumbel_keep_fwd", real)
    assert all(torch.equal(a, b) for a, b in zip(decs[ops.GEMM_EXACT], decs[ops.GEMM_BF16])), "the two modes must take the same decisions"
    assert all(0 < float(d.sum()) < d.numel() for d in decs[ops.GEMM_EXACT])

    def one_step(mode):
        ops.set_gemm_mode(mode)
        try:
            step = _train_step()
            step_case = DC.CASES["stage1"]                          # _train_step builds the stage1 student
            step.student.gumbel_noise = noise[:len(step_case["cfg"]["pruning_loc"])]
            before = {k: v.detach().clone() for k, v in step.student.named_parameters()}
            info = step(x, y)
            torch.cuda.synchronize()
            moved = {k: not torch.equal(v, before[k]) for k, v in step.student.named_parameters()}
            return ([t.detach().clone() for t in step.dynamicvit_loss_fn.last], info["loss"].detach().clone(), step.arena.params.clone(),
                    step.arena.grads.clone(), moved)
        finally:
            ops.set_gemm_mode(ops.GEMM_EXACT)
    exact, a, b = one_step(ops.GEMM_EXACT), one_step(ops.GEMM_BF16), one_step(ops.GEMM_BF16)
    assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.isfinite(a[3]).all() and float(a[3].abs().max()) > 0
    assert all(a[4][k] for k in a[4] if "score_predictor" in k), "every predictor parameter must move"
    for name, u, v in zip(("total", "cls", "ratio", "kl", "token"), a[0], exact[0]):
        print(f"dynamicvit step loss {name}: bf16 {float(u):.6f} exact {float(v):.6f}")
        _close(u, v, name)


def test_threshold_training_forward_backward_in_bf16_mode_tracks_the_exact_one():
    """the dynamic-keep-ratio path (every block after the first stage attends through the keep mask) with the fixture's masks injected"""
    from d2s import ops
    from d2s.engine import TrainStep
    from tests.test_droppath_gpu import _fixture_student
    from tests.test_model_gpu import make_args
    from tests.test_threshold_gpu import build_threshold_models
    g = cases.load_golden("droppath_micro")
    case = cases.THRESHOLD_CASES["micro_thr1"]
    y = _t(cases.make_labels(case)).to(DEV)

    def one(mode):
        ops.set_gemm_mode(mode)
        try:
            student, x, _, _ = _fixture_student(g, "thr_")
            _, teacher, _, _ = build_threshold_models(case, torch.device(DEV))
            args = make_args(case["cfg"])
            args.patch_score_threshold = case["threshold"]
            ts = TrainStep(student, teacher, args, warmup_steps=0, graph=False)
            loss, info = ts._forward_backward(x, y, accumulate=False)
            ops.join_weight_grads()
            torch.cuda.synchronize()
            return (loss.detach().clone(), info["mask_loss"].detach().clone(), info["backbone_loss"].detach().clone(), ts.arena.grads.clone(),
                    [k.detach().clone() for k in info["kept"]])
        finally:
            ops.set_gemm_mode(ops.GEMM_EXACT)
    exact, a, b = one(ops.GEMM_EXACT), one(ops.GEMM_BF16), one(ops.GEMM_BF16)
    assert all(torch.equal(u, v) for u, v in zip(a[:4], b[:4]))
    assert torch.isfinite(a[3]).all() and float(a[3].abs().max()) > 0
    for name, u, v in zip(("total", "mask", "backbone"), a[:3], exact[:3]):
        print(f"threshold step loss {name}: bf16 {float(u):.6f} exact {float(v):.6f}")
        _close(u, v, name)
