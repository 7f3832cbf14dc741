"""Plain torch restatement of the fp32 GEMM entries (d2s_gemm_f32, d2s_gemm_f32_rowscale, d2s_linear_wgrad_f32, d2s_colsum_f32), written
from the formulas of include/d2s_hip.h and not from the kernels.  Nothing here imports the package under test.

Operands are 2-D views, strided as the call will see them (a leading dimension larger than the row length is a view into a wider
buffer), so the leading dimensions are part of the reference.  Every function works in the dtype of its operands: float64 inputs give
the reference of the kernel tests, the same inputs in float32 their yardstick (what plain fp32 arithmetic on the CPU makes of it).

    layout 0 (NT)  A [M, K], B [N, K]    acc = A B^T        forward y = x W^T
    layout 1 (NN)  A [M, K], B [K, N]    acc = A B          input gradient dx = dy W
    layout 2 (TN)  A [K, M], B [K, N]    acc = A^T B        weight gradient dW = dy^T x, with db = column sums of A

Acceptance of a kernel result, two rules that both apply (check):
  (a) whole tensor: tests.losspath_ref.assert_close_as_fp32 - the kernel may be ERR_FACTOR times as far from float64, in the relative
      2-norm, as the same formula evaluated in fp32 on the CPU, or within ERR_FLOOR;
  (b) per element: |got - ref64| <= (K + slices + 4) 2^-24 S_mn, S_mn = sum_k |a_mk| |b_nk| + |bias_n| + |aux_mn| + |C_old,mn| with the
      terms the epilogue uses.  First order in 2^-24 and independent of the summation order: K roundings for the products' chain (any
      order: a term passes through at most K - 1 additions, plus its own product rounding when no fma is used), one per slab added by the
      ordered combine, and 4 for the epilogue's additions, its scale and the store.  It is loose by design: the whole-tensor norm of (a)
      dilutes a localized fault - a dropped or doubled product, a wrong row - and this does not.
      GELU outputs and the GELU-gradient mask: the bound is multiplied by 1.13 >= max |gelu'| (and the gradient mask's factor has the same
      maximum), and ERR_FACTOR times the largest absolute error of torch's fp32 gelu (its fp32 derivative times |acc|) against float64
      on the same pre-activations is added; that figure comes from the CPU, never from the kernel, and is printed.
      Row scale (epilogue 11): the product and bias terms of S are multiplied by |scale|, since their error is."""
import math

import torch
import torch.nn.functional as F

from tests.losspath_ref import ERR_FACTOR, F32_EPS, assert_close_as_fp32

NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_BIAS_RESID = 0, 1, 2, 3, 4
EPI_MUL_GELU_GRAD, EPI_MUL_RELU_MASK, EPI_BIAS_ROWADD, EPI_ACCUM = 5, 6, 7, 8
EPI_BIAS_RESID_ROWSCALE = 11
EPILOGUES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 11)
HAS_BIAS = (EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_ROWADD, EPI_BIAS_RESID_ROWSCALE)
GELU_SLOPE = 1.13             # max |gelu'(z)| = 1.1289 at z = sqrt(2)


def product(layout, A, B):
    """acc [M, N] of the layout's product, in the dtype of A and B"""
    if layout == NT:
        return A @ B.t()
    if layout == NN:
        return A @ B
    if layout == TN:
        return A.t() @ B
    raise ValueError(layout)


def gelu_grad(z):
    """d/dz of z Phi(z): Phi(z) + z phi(z)"""
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def rowadd_index(M, aux_rows):
    """row of aux that epilogue 7 adds to output row m: m mod aux_rows"""
    return torch.arange(M) % aux_rows


def remap_index(M, rows_per_img, skip):
    """buffer row that result row m is stored to: m + (m // rows_per_img + 1) * skip; rows_per_img 0: no remap"""
    m = torch.arange(M)
    return m if rows_per_img <= 0 else m + (m // rows_per_img + 1) * skip


def group_scale(rowscale, M, rows_per_group):
    """[M, 1]: the scale of row m is rowscale[m // rows_per_group]"""
    return rowscale[torch.arange(M) // rows_per_group][:, None]


def epilogue(acc, epi, bias=None, aux=None, aux_rows=0, c_old=None, rowscale=None, rows_per_group=0):
    """-> (C [M, N], pre): what the store writes for result rows 0 .. M-1 (before any row remap) and, for epilogue 3, the pre-activation
    copy (else None).  aux is [M, N] (epilogues 4, 5, 6, 11) or [aux_rows, N] (7); c_old the previous content of C (8)."""
    M = acc.shape[0]
    v = acc + bias if (epi in HAS_BIAS and bias is not None) else acc
    if epi in (EPI_NONE, EPI_BIAS):
        return v, None
    if epi == EPI_BIAS_RELU:
        return torch.relu(v), None
    if epi == EPI_BIAS_GELU:
        return F.gelu(v), v
    if epi == EPI_BIAS_RESID:
        return v + aux, None
    if epi == EPI_MUL_GELU_GRAD:
        return v * gelu_grad(aux), None
    if epi == EPI_MUL_RELU_MASK:
        return torch.where(aux > 0, v, torch.zeros_like(v)), None
    if epi == EPI_BIAS_ROWADD:
        return v + aux[rowadd_index(M, aux_rows)], None
    if epi == EPI_ACCUM:
        return c_old + v, None
    if epi == EPI_BIAS_RESID_ROWSCALE:
        s = group_scale(rowscale, M, rows_per_group)
        return torch.where(s == 0, aux, s * v + aux), None      # a zero scale: the row is aux itself, whatever the branch holds
    raise ValueError(epi)


def gemm_ref(layout, A, B, epi=EPI_NONE, **kw):
    return epilogue(product(layout, A, B), epi, **kw)


def colsum(X):
    """bias gradient: the column sums of X [rows, N]; for layout 2 X is the A operand (dy)"""
    return X.sum(dim=0)


def magnitude(layout, A, B):
    """sum_k |a_mk| |b_nk|, float64"""
    return product(layout, A.double().abs(), B.double().abs())


def elem_bound(K, slices, absprod, epi=EPI_NONE, bias=None, aux=None, aux_rows=0, c_old=None, rowscale=None, rows_per_group=0, acc64=None,
               what=""):
    """rule (b): -> (bound of C [M, N], bound of the pre-activation copy or None); float64 operands, absprod = magnitude(...)"""
    M = absprod.shape[0]
    S = absprod.clone()
    if epi in HAS_BIAS and bias is not None:
        S = S + bias.double().abs()
    if epi == EPI_BIAS_RESID_ROWSCALE:
        S = S * group_scale(rowscale.double(), M, rows_per_group).abs()
    if epi in (EPI_BIAS_RESID, EPI_BIAS_RESID_ROWSCALE):
        S = S + aux.double().abs()
    if epi == EPI_BIAS_ROWADD:
        S = S + aux.double().abs()[rowadd_index(M, aux_rows)]
    if epi == EPI_ACCUM:
        S = S + c_old.double().abs()
    b = (K + slices + 4) * F32_EPS * S
    if epi == EPI_MUL_RELU_MASK:
        return b * (aux > 0), None
    if epi == EPI_BIAS_GELU:
        pre64 = acc64 + (bias.double() if bias is not None else 0.0)
        gerr = float((F.gelu(pre64.float()).double() - F.gelu(pre64)).abs().max())
        print(f"[gelu] {what}: largest error of the fp32 CPU gelu on these pre-activations {gerr:.3e}")
        return GELU_SLOPE * b + ERR_FACTOR * gerr, b
    if epi == EPI_MUL_GELU_GRAD:
        gerr = float(((gelu_grad(aux.float()).double() - gelu_grad(aux.double())).abs() * acc64.abs()).max())
        print(f"[gelu] {what}: largest error of the fp32 CPU gelu' times |acc| {gerr:.3e}")
        return GELU_SLOPE * b + ERR_FACTOR * gerr, None
    return b, None


def check_elements(what, got, ref64, bound):
    """rule (b); -> the largest |got - ref64| / bound"""
    assert bool(torch.isfinite(got).all()), f"{what}: NaN / Inf in the result"
    err = (got.double() - ref64).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    over = err > bound
    used = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if bool(over.any()):
        idx = tuple(int(i) for i in over.nonzero()[0])
        raise AssertionError(f"{what}: {int(over.sum())} elements outside the per-element bound, first at {list(idx)}: got {float(got[idx])!r}, "
                             f"ref {float(ref64[idx])!r}, bound {float(bound[idx]):.3e}")
    print(f"[bound] {what}: largest per-element error uses {100 * used:.1f} % of its bound")
    return used


def check(what, got, ref64, ref32, bound):
    """rules (a) and (b); -> (err_hip / err_cpu32 of (a), largest |got - ref64| / bound of (b))"""
    used = check_elements(what, got, ref64, bound)
    return assert_close_as_fp32(what, got, ref64, ref32), used
