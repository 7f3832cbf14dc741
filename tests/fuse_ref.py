"""Token fusion at a pruning stage (fuse_dropped), restated in plain torch.  This is the definition, the build's
own: the reference has no counterpart.

A stage receives x [B, n, D] - row 0 CLS, then T = n - 1 - t scored tokens, then the t package tokens of earlier stages -, the stage's
keep probabilities p [B, T] and the ascending stage-relative id lists kept [B, k] / dropped [B, T - k] of the hard top-k.  It returns
y [B, k + t + 2, D]:

    y[:, 0]         = x[:, 0]
    y[:, 1 + i]     = x[:, 1 + kept[:, i]]
    y[:, 1 + k + s] = x[:, 1 + T + s]                        s < t, copied
    y[:, -1]        = f = sum_{j in dropped} w_j x[:, 1 + j],   w_j = p_j / S,  S = sum_{j in dropped} p_j

With an empty dropped set, or one whose probabilities sum to zero, f is a row of zeros and nothing flows through it.  The ids get no
gradient.  `fuse_forward` is dtype-generic: float64 for the kernel tests, fp32 on device tensors for the model-level test."""
import torch


def fuse_forward(x, p, kept, dropped, t):
    B, n, D = x.shape
    T = n - 1 - int(t)
    tokens = x[:, 1:1 + T]
    rows = lambda ids: torch.gather(tokens, 1, ids[:, :, None].expand(B, ids.shape[1], D))
    pd = torch.gather(p, 1, dropped)                                          # [B, m]
    S = pd.sum(dim=1, keepdim=True)
    ok = S > 0
    w = torch.where(ok, pd / torch.where(ok, S, torch.ones_like(S)), torch.zeros_like(pd))
    f = (w[:, :, None] * rows(dropped)).sum(dim=1, keepdim=True)
    return torch.cat([x[:, :1], rows(kept), x[:, 1 + T:], f], dim=1)


def fuse_forward_f64(x, p, kept, dropped, t):
    return fuse_forward(x.double(), p.double(), kept, dropped, t)


def fuse_autograd(x, p, kept, dropped, t, g):
    """-> (y, dx, dp) by autograd in the dtype of x"""
    x, p = x.detach().clone().requires_grad_(True), p.detach().clone().requires_grad_(True)
    y = fuse_forward(x, p, kept, dropped, t)
    dx, dp = torch.autograd.grad(y, (x, p), g.to(y.dtype))
    return y.detach(), dx, dp


def fuse_closed_form_backward(x, p, kept, dropped, t, g):
    """The backward as the kernel computes it: CLS, kept and carried rows of dx are rows of g, a dropped row j is w_j g_f, and
    dp_j = (<x_j, g_f> - <f, g_f>) / S for dropped j, 0 for kept j (g_f: the last row of g)."""
    B, n, D = x.shape
    T, k = n - 1 - int(t), kept.shape[1]
    y = fuse_forward(x, p, kept, dropped, t)
    f, gf = y[:, -1], g[:, -1]
    pd = torch.gather(p, 1, dropped)
    S = pd.sum(dim=1, keepdim=True)
    ok = S > 0
    Ss = torch.where(ok, S, torch.ones_like(S))
    w = torch.where(ok, pd / Ss, torch.zeros_like(pd))
    dx = torch.zeros_like(x)
    dx[:, 0] = g[:, 0]
    dx[:, 1 + T:] = g[:, 1 + k:1 + k + int(t)]
    tok = dx[:, 1:1 + T]
    tok.scatter_(1, kept[:, :, None].expand(B, k, D), g[:, 1:1 + k])
    tok.scatter_(1, dropped[:, :, None].expand(B, dropped.shape[1], D), w[:, :, None] * gf[:, None, :])
    xd = torch.gather(x[:, 1:1 + T], 1, dropped[:, :, None].expand(B, dropped.shape[1], D))
    dpd = torch.where(ok, ((xd * gf[:, None, :]).sum(-1) - (f * gf).sum(-1, keepdim=True)) / Ss, torch.zeros_like(pd))
    dp = torch.zeros_like(p).scatter_(1, dropped, dpd)
    return dx, dp


class TorchGatherFuse:
    """Stands in for d2s.functional.GatherFuseFn (same call: .apply(x, p, kept, dropped, t)) with torch ops and autograd."""
    apply = staticmethod(fuse_forward)


def topk_ids(p, k):
    """(kept, dropped) as d2s_select_topk orders them: value descending, ties lowest index first, each list ascending"""
    order = torch.argsort(p, dim=1, descending=True, stable=True)
    return torch.sort(order[:, :k], dim=1)[0].contiguous(), torch.sort(order[:, k:], dim=1)[0].contiguous()


def stage_lengths(init_n, ratios, fuse):
    """Rows of the sequence after each pruning stage: 1 + k_s, plus s + 1 package rows with fusion"""
    return [1 + int(init_n * r) + (s + 1 if fuse else 0) for s, r in enumerate(ratios)]
