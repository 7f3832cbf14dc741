"""GPU tier: the performer attention of the T2T module (csrc/t2t.hip: d2s_performer_attn_fwd / d2s_performer_attn_bwd, six kernels each
way) against tests/losspath_ref.py performer / performer_backward in float64, at token counts that leave a ragged group of four tokens
(one wave per token, four per workgroup), sit on both sides of the two chunk thresholds of the token-sum (256 and 2048) and leave a
ragged last chunk.  Every output may be 4 times as far from float64 as the fp32 restatement on the CPU by the relative 2-norm, or 3e-7."""
import math

import pytest
import torch

from tests import losspath_ref as R

pytestmark = pytest.mark.gpu

EPS = 1e-8
SHAPES = [(1, 1), (2, 5), (1, 33), (2, 255), (1, 256), (2, 257), (1, 2047), (1, 2048), (1, 2050)]
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _inputs(B, T, std):
    """kqv with the given std; w = 32 rows of a random orthogonal 64 x 64 matrix times sqrt(32) (Token_performer's initialisation).  At
    std 0.5 the normaliser D is far above eps; at std 1.0 it is far below and y is num / eps."""
    g = torch.Generator().manual_seed(1000 * B + T + int(std * 100000))
    kqv = (torch.randn(B * T, 192, generator=g) * std).float()
    q, _ = torch.linalg.qr(torch.randn(64, 64, generator=g, dtype=torch.float64))
    w = (q[:32] * math.sqrt(32.0)).float().contiguous()
    gy = torch.randn(B * T, 64, generator=g).float()
    skip = torch.randn(B * T, 64, generator=g).float()
    return kqv, w, gy, skip


def _case(B, T, std):
    """inputs, float64 reference and fp32 yardstick of one shape, computed once and shared by the forward and the backward test"""
    key = (B, T, std)
    if key not in _CACHE:
        kqv, w, gy, skip = _inputs(B, T, std)
        c = {"in": (kqv, w, gy, skip)}
        for name, dt in (("ref64", torch.float64), ("ref32", torch.float32)):
            k_, w_, gy_, skip_ = (x.to(dt) for x in (kqv, w, gy, skip))
            c[name] = dict(R.performer(k_, w_, B, T, EPS))
            c[name]["dkqv_skip"] = R.performer_backward(k_, w_, B, T, EPS, gy_, skip_)
            c[name]["dkqv"] = R.performer_backward(k_, w_, B, T, EPS, gy_, None)
        _CACHE[key] = c
    return _CACHE[key]


def _check_normaliser(what, got, c):
    """D_t = sum_m qp[t, m] ksum[m] is one number per token, and with B T = 1 the whole tensor is one number: the ratio of two single
    rounding errors exceeds 4 one time in six whatever the kernel does (measured at (1, 1): err_hip 5.2e-7, err_cpu32 7.1e-8, ratio 7.3,
    with every other shape between 0.7 and 2.3).  So for D the factor gives way, where it is exceeded, to a bound from the operation
    count.  All terms are positive, hence relative errors add: the largest relative error of the qp row, that of the ksum row (both as the
    kernels produced them, each held to the fp32 yardstick above), and the 32 fused multiply-adds of the dot product on one serial path,
    (32 + 1) u: 4.8e-6 to 1.3e-5 on these inputs, against measured errors of D of 4e-7 to 2.6e-6 on both sides.  A D kernel that reads
    the wrong ksum row, drops a feature or guards a token wrongly is off by far more than that."""
    B = c["ref64"]["ksum"].shape[0]
    T = c["ref64"]["D"].numel() // B
    rel = lambda k: ((got[k].cpu().double() - c["ref64"][k].reshape(got[k].shape)).abs() / c["ref64"][k].reshape(got[k].shape)).reshape(B, -1).max(dim=1)[0]
    derived = float((rel("qp") + rel("ksum")).max()) + 33 * R.F32_EPS * (1 + 1e-3)
    e_hip, e_cpu = R.rel_err(got["D"].cpu(), c["ref64"]["D"]), R.rel_err(c["ref32"]["D"], c["ref64"]["D"])
    print(f"[parity] {what} D: err_hip {e_hip:.3e}  err_cpu32 {e_cpu:.3e}  ratio {e_hip / e_cpu:.2f}  derived bound {derived:.3e}")
    assert T * B == got["D"].numel() and e_hip <= max(R.ERR_FACTOR * e_cpu, R.ERR_FLOOR, derived), (what, e_hip, e_cpu, derived)


def _forward_and_backward(B, T, std):
    from d2s import ops
    dev = _dev()
    c = _case(B, T, std)
    kqv, w, gy, skip = (x.to(dev) for x in c["in"])
    assert kqv.shape == (B * T, 192) and w.shape == (32, 64) and gy.shape == (B * T, 64)
    y, kp, qp, A, ksum, D = ops.performer_attn_fwd(kqv, w, B, T, EPS)
    got = {"y": y, "kp": kp, "qp": qp, "A": A, "ksum": ksum, "D": D}
    what = f"performer B {B} T {T} std {std}"
    ratios = {}
    for k, v in got.items():
        assert v.shape == c["ref64"][k].shape, k
        if k != "D":
            ratios[k] = R.assert_close_as_fp32(f"{what} {k}", v.cpu(), c["ref64"][k], c["ref32"][k])
    _check_normaliser(what, got, c)
    # the backward from the tensors the forward saved
    d1 = ops.performer_attn_bwd(kqv, w, y, kp, qp, A, ksum, D, gy, skip, B, T, EPS)
    d0 = ops.performer_attn_bwd(kqv, w, y, kp, qp, A, ksum, D, gy, None, B, T, EPS)
    for name, d in (("dkqv_skip", d1), ("dkqv", d0)):
        assert d.shape == (B * T, 192)
        ratios[name] = R.assert_close_as_fp32(f"{what} {name}", d.cpu(), c["ref64"][name], c["ref32"][name])
    assert torch.equal(d1[:, :128], d0[:, :128])                        # the skip gradient reaches v only
    return ratios


@pytest.mark.parametrize("B,T", SHAPES)
def test_performer_forward_and_backward(B, T):
    """y, kp, qp, A, ksum, D and dkqv (with and without the skip gradient) at kqv std 0.5, where D is 2.6e-5 at the least: thousands of times eps.
    Measured err_hip / err_cpu32 on the MI355X, largest over the shapes: y 1.5, kp 2.6, qp 2.0, A 2.6, ksum 2.8, dkqv 1.9 (with and
    without skip); from T = 33 on every ratio is between 0.6 and 1.3, errors 3e-7 to 2.6e-6 on both sides.  D: see _check_normaliser."""
    c = _case(B, T, 0.5)
    assert float(c["ref64"]["D"].min()) > 1e3 * EPS                     # the normaliser, not eps, sets the output
    _forward_and_backward(B, T, 0.5)


def test_performer_eps_dominated():
    """kqv std 1.0: D is far below eps = 1e-8, the output is num / eps and the gradient through D is dead weight: pinned separately.
    Measured err_hip / err_cpu32: 0.45 to 0.98 forward, 0.85 (dkqv) and 1.35 (dkqv with skip, 4e-8 against 3e-8)."""
    c = _case(2, 257, 1.0)
    assert float(c["ref64"]["D"].max()) < 0.1 * EPS
    _forward_and_backward(2, 257, 1.0)


def test_performer_workspace_one_byte_short():
    from d2s import lib
    dev = _dev()
    B, T = 2, 257
    kqv, w, gy, skip = (x.to(dev) for x in _inputs(B, T, 0.5))
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    M = B * T
    y, kp, qp, A, ksum, D = f(M, 64), f(M, 32), f(M, 32), f(B, 64, 32), f(B, 32), f(M)
    need = lib.query("d2s_performer_workspace_bytes", B, T)
    assert need == B * math.ceil(T / 64) * (64 * 32 + 32) * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    fwd = (lib.ptr(kqv), lib.ptr(w), lib.ptr(y), lib.ptr(kp), lib.ptr(qp), lib.ptr(A), lib.ptr(ksum), lib.ptr(D), B, T, EPS, lib.ptr(ws))
    with pytest.raises(lib.D2SError):
        lib.call("d2s_performer_attn_fwd", *fwd, need - 1)
    dkqv, dnum, dD, dqp, dkp, dA, dksum = f(M, 192), f(M, 64), f(M), f(M, 32), f(M, 32), f(B, 64, 32), f(B, 32)
    bwd = (lib.ptr(kqv), lib.ptr(w), lib.ptr(y), lib.ptr(kp), lib.ptr(qp), lib.ptr(A), lib.ptr(ksum), lib.ptr(D), lib.ptr(gy), lib.ptr(skip),
           lib.ptr(dkqv), lib.ptr(dnum), lib.ptr(dD), lib.ptr(dqp), lib.ptr(dkp), lib.ptr(dA), lib.ptr(dksum), B, T, EPS, lib.ptr(ws))
    with pytest.raises(lib.D2SError):
        lib.call("d2s_performer_attn_bwd", *bwd, need - 1)
    torch.cuda.synchronize()
    assert bool((y == 0).all()) and bool((dkqv == 0).all())             # refused before any launch
    lib.call("d2s_performer_attn_fwd", *fwd, need)                      # the exact size is accepted
    torch.cuda.synchronize()
    assert bool((D > 0).all())
