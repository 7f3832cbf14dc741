"""Plain torch restatements of the loss path, the weight update, the performer attention and the mask helpers (csrc/loss.hip,
csrc/threshold.hip, csrc/t2t.hip), written from the formulas and not from the kernels.  Nothing here imports the package under test.

Every function works in the dtype of its tensor arguments: with float64 inputs it is the reference of the kernel tests, with the same
inputs in float32 it is their yardstick (what plain fp32 arithmetic on the CPU makes of the same operation).  Scalars are Python floats;
a test hands in the values the C ABI receives, i.e. already rounded to fp32, so reference and kernel start from the same numbers."""
import math

import torch

F32_EPS = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
ERR_FACTOR = 4.0              # a kernel may be this many times as far from float64 as the fp32 restatement (tests/test_kernels_gpu.py, test_gemm_split_modes)
ERR_FLOOR = 3e-7              # ... or within about 2 ulp, whichever is larger

KL_LOGIT_TARGET, KL_PROB_TARGET, CE_LABEL, MSE_TARGET, SOFT_CE = 0, 1, 2, 3, 4      # == d2s.ops.* (checked by the CPU test)


# ---------------------------------------------------------------------------------------------------------------- error measures
def rel_err(got, ref64):
    """relative 2-norm error of a whole tensor against float64; a reference that is all zeros admits only zeros"""
    got, ref64 = got.double().reshape(-1), ref64.double().reshape(-1)
    assert bool(torch.isfinite(ref64).all()), "NaN / Inf in the reference: a broken input"
    den = float(ref64.norm())
    num = float((got - ref64).norm())
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / den


def sum_bound(depth, abs_sum, extra_roundings=0):
    """a-priori bound of an fp32 summation tree with `depth` additions on its longest path over terms whose magnitudes sum to abs_sum,
    plus `extra_roundings` further roundings of the result (a scale, a division): (depth + 1 + extra) * 2^-24 * sum|terms|"""
    return (depth + 1 + extra_roundings) * F32_EPS * float(abs_sum) * (1 + 1e-3)


# ---------------------------------------------------------------------------------------------------------------- mask loss targets
def teacher_target(cls_attn):
    """cls_attn [B, L, H, n] -> [B, n - 1]: mean over layers, max over heads, drop the CLS column, renormalise"""
    w = cls_attn.mean(dim=1).max(dim=1)[0][:, 1:]
    return w / w.sum(dim=-1, keepdim=True)


def gather_renorm(target, ids, normalize):
    g = torch.gather(target, 1, ids)
    return g / g.sum(dim=1, keepdim=True) if normalize else g


# ---------------------------------------------------------------------------------------------------------------- row losses
def row_loss_value(mode, s, t=None, labels=None):
    """per-row loss [rows] of s [rows, C]; t [rows, C] (logits in mode 0, probabilities / targets otherwise), labels [rows] int64"""
    if mode == MSE_TARGET:
        return ((s - t) ** 2).sum(dim=-1)
    ls = torch.log_softmax(s, dim=-1)
    if mode == KL_LOGIT_TARGET:                               # KL(softmax(t) || softmax(s))
        lt = torch.log_softmax(t, dim=-1)
        return (lt.exp() * (lt - ls)).sum(dim=-1)
    if mode == KL_PROB_TARGET:                                # KL(t || softmax(s)), t > 0
        return (t * (t.log() - ls)).sum(dim=-1)
    if mode == CE_LABEL:
        return -ls.gather(1, labels[:, None])[:, 0]
    if mode == SOFT_CE:                                       # -sum_c t_c log softmax(s)_c; a zero target contributes nothing
        return -(t * ls).sum(dim=-1)
    raise ValueError(mode)


def row_loss(mode, s, t=None, labels=None, row_weight=None):
    """-> (loss_row [rows], d loss_row / d s [rows, C]), both times row_weight when given; the gradient is autograd in the dtype of s"""
    s = s.detach().clone().requires_grad_(True)
    loss = row_loss_value(mode, s, t, labels)
    if row_weight is not None:
        loss = loss * row_weight
    (grad,) = torch.autograd.grad(loss.sum(), s)
    return loss.detach(), grad


# ---------------------------------------------------------------------------------------------------------------- masks
def mask_agreement(ids_a, ids_b, T):
    """number of the T token positions on which the two masks given as id lists [B, k] (unique ids per list) coincide"""
    B = ids_a.shape[0]
    ma, mb = torch.zeros((B, T), dtype=torch.bool), torch.zeros((B, T), dtype=torch.bool)
    if ids_a.shape[1]:
        ma.scatter_(1, ids_a, True)
        mb.scatter_(1, ids_b, True)
    return (ma == mb).sum(dim=1)


def dense_mask_agreement(a, b):
    return (a == b).sum(dim=1)


def mask_row_weights(mask):
    """mask / sum(mask); all zeros when the sum is 0"""
    m = mask.reshape(-1)
    tot = m.sum()
    return m / tot if float(tot) > 0 else torch.zeros_like(m)


# ---------------------------------------------------------------------------------------------------------------- activations
def act_grad(g, z, kind):
    """gelu: g * (Phi(z) + z phi(z)) with z the pre-activation; relu: g * [z > 0]"""
    if kind == "relu":
        return g * (z > 0).to(g.dtype)
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return g * (cdf + z * pdf)


# ---------------------------------------------------------------------------------------------------------------- AdamW, EMA
def adamw_step(p, g, m, v, lr, wd, b1, b2, eps, t, grad_scale=1.0):
    """One decoupled-weight-decay Adam step (Loshchilov & Hutter; torch.optim.AdamW): -> (p, m, v) after the step.
    lr, wd, t: floats or tensors broadcastable to p; t >= 1 is the number of this update of the tensor an element belongs to (the
    per-tensor step counter), the bias corrections 1 - b^t are formed in float64 whatever the dtype of p."""
    dt = p.dtype
    t = torch.as_tensor(t, dtype=torch.float64)
    bc1 = (1.0 - torch.as_tensor(b1, dtype=torch.float64) ** t).to(dt)
    bc2 = (1.0 - torch.as_tensor(b2, dtype=torch.float64) ** t).to(dt)
    lr, wd = torch.as_tensor(lr, dtype=torch.float64).to(dt), torch.as_tensor(wd, dtype=torch.float64).to(dt)
    g = g * grad_scale
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / bc1) * m / (v.sqrt() / bc2.sqrt() + eps)
    return p, m, v


def ema_step(ema, p_new, decay):
    """timm ModelEmaV2: decay * ema + (1 - decay) * p_new"""
    return decay * ema + (1.0 - decay) * p_new


# ---------------------------------------------------------------------------------------------------------------- performer
def prm_exp(x, w):
    """positive random features of x [B, T, e] under w [m, e]: exp(w x - |x|^2 / 2) / sqrt(m)"""
    m = w.shape[0]
    return torch.exp(x @ w.t() - 0.5 * (x * x).sum(dim=-1, keepdim=True)) / math.sqrt(m)


def performer(kqv, w, B, T, eps):
    """kqv [B*T, 192] = [k | q | v] rows, w [32, 64] -> dict of y [B*T, 64] and the tensors the backward keeps: kp, qp [B*T, 32],
    A [B, 64, 32] = sum_t v_t kp_t^T, ksum [B, 32] = sum_t kp_t, D [B*T] = qp_t . ksum.  y_t = A qp_t / (D_t + eps)."""
    k, q, v = (kqv.view(B, T, 192)[:, :, i * 64:(i + 1) * 64] for i in range(3))
    kp, qp = prm_exp(k, w), prm_exp(q, w)
    ksum = kp.sum(dim=1)
    D = torch.einsum("btm,bm->bt", qp, ksum)
    A = torch.einsum("btn,btm->bnm", v, kp)
    y = torch.einsum("btm,bnm->btn", qp, A) / (D[:, :, None] + eps)
    return {"y": y.reshape(B * T, 64), "kp": kp.reshape(B * T, 32), "qp": qp.reshape(B * T, 32), "A": A, "ksum": ksum,
            "D": D.reshape(B * T)}


def performer_backward(kqv, w, B, T, eps, gy, skip=None):
    """d/d kqv of <y, gy> (+ <v, skip>: the gradient that reaches v through the skip connection), autograd in the dtype of kqv"""
    kqv = kqv.detach().clone().requires_grad_(True)
    obj = (performer(kqv, w, B, T, eps)["y"] * gy).sum()
    if skip is not None:
        obj = obj + (kqv[:, 128:192] * skip).sum()
    (dkqv,) = torch.autograd.grad(obj, kqv)
    return dkqv


def assert_close_as_fp32(what, got, ref64, ref32, derived=0.0):
    """The kernel's output may be ERR_FACTOR times as far from float64 as the fp32 restatement is, or ERR_FLOOR, or - for a kernel whose
    operation count is known to cost more than that - within `derived`, a bound worked out from that count; -> err_hip / err_cpu32"""
    e_hip, e_cpu = rel_err(got, ref64), rel_err(ref32, ref64)
    ratio = e_hip / e_cpu if e_cpu > 0 else (0.0 if e_hip == 0 else math.inf)
    print(f"[parity] {what}: err_hip {e_hip:.3e}  err_cpu32 {e_cpu:.3e}  ratio {ratio:.2f}" + (f"  derived bound {derived:.3e}" if derived else ""))
    assert e_hip <= max(ERR_FACTOR * e_cpu, ERR_FLOOR, derived), (what, e_hip, e_cpu, derived)
    return ratio


def kl_rows_error_bound(mode, s, t=None, labels=None, row_weight=None):
    """A-priori rounding-error bound of csrc/loss.hip kl_rows_kernel from its operation count, as relative 2-norm errors
    (loss_row, grad); float64 inputs.  u = 2^-24, C columns, NE = ceil(C / 64) columns per lane, `depth` = NE + 6 additions on the
    longest path of a row sum (NE in the lane, 6 wave steps).  Per row, with M the row maximum:
      d_c = fl(s_c - M)                        exact up to u |d_c|
      es  = sum_c expf(d_c), logf(es) = L      es relative (depth + 2) u, so L absolute (depth + 3) u + u |L|
      lse = fl(M + L)                          one rounding AT THE SIZE OF lse: u |lse| - the term an fp32 log_softmax that subtracts
                                               the maximum first does not have; it is what a row offset by 30 costs
      ls_c = fl(s_c - lse)                     u |ls_c|
    hence |err ls_c| <= delta_c = u (|lse| + |ls_c| + |L| + depth + 4), and p_c = expf(ls_c) is off by at most p_c (delta_c + 2 u).
    The loss terms and gradients are products and differences of these (one more u each) and a row sum of `depth` additions,
    (depth + 1) u sum |terms|; a row weight adds one rounding.  Mode 3 has no transcendental: no bound is needed and (0, 0) is returned."""
    u = F32_EPS
    rows, C = s.shape
    depth = (C + 63) // 64 + 6
    if mode == MSE_TARGET:
        return 0.0, 0.0

    def log_softmax_with_bound(x):
        M = x.max(dim=-1, keepdim=True)[0]
        L = torch.log(torch.exp(x - M).sum(dim=-1, keepdim=True))
        lse = M + L
        ls = x - lse
        return ls, u * (lse.abs() + ls.abs() + L.abs() + depth + 4)

    ls, d = log_softmax_with_bound(s)
    p = ls.exp()
    ep = p * (d + 2 * u)
    if mode == KL_LOGIT_TARGET:
        lt, dt = log_softmax_with_bound(t)
        pt = lt.exp()
        ept = pt * (dt + 2 * u)
        g, eg = p - pt, ep + ept
        terms = pt * (lt - ls)
        eterm = ept * (lt - ls).abs() + pt * (dt + d + u * (lt - ls).abs())
    elif mode in (KL_PROB_TARGET, SOFT_CE):
        tsum = t.sum(dim=-1, keepdim=True)
        g, eg = p * tsum - t, ep * tsum + p * tsum * (depth + 2) * u
        if mode == KL_PROB_TARGET:
            logt = t.log()
            terms = t * (logt - ls)
            eterm = t * (2 * u * logt.abs() + d + u * (logt - ls).abs())
        else:
            terms = -t * ls
            eterm = t * d
    elif mode == CE_LABEL:
        onehot = torch.zeros_like(s).scatter_(1, labels[:, None], 1.0)
        g, eg = p - onehot, ep
        terms = -onehot * ls
        eterm = onehot * d
    else:
        raise ValueError(mode)
    eg = eg + u * g.abs()
    loss = terms.sum(dim=-1)
    eloss = (eterm + u * terms.abs()).sum(dim=-1) + (depth + 1) * u * terms.abs().sum(dim=-1)
    if row_weight is not None:
        w = row_weight.abs()
        eloss, loss = w * (eloss + u * loss.abs()), w * loss
        eg, g = w[:, None] * (eg + u * g.abs()), w[:, None] * g
    rel = lambda e, r: 0.0 if float(r.norm()) == 0.0 else float(e.norm() / r.norm()) * (1 + 1e-3)
    return rel(eloss, loss), rel(eg, g)
