"""Float64 helpers for training through token merging: the merge's backward in closed form, a restatement of the
merging block in the dtype of its input (float64 for the reference, float32 for the yardstick's own rounding error) with its gradients by
torch autograd, gradients of tests/tome_ref.py's key-weighted attention and whole-model forward (plans replayed: both are differentiable
as written), and the objective of a merging student.  Plain torch on the CPU."""
import torch
import torch.nn.functional as F

from tests import tome_ref as R

PARAM_NAMES = ("n1w", "n1b", "qkvw", "qkvb", "projw", "projb", "n2w", "n2b", "fc1w", "fc1b", "fc2w", "fc2b")


def merge_backward(dy, size, size_out, plan):
    """dy [B,n-r,D], size [B,n] or None, size_out [B,n-r], plan (unm, src, dst) -> dx [B,n,D] float64: every input row takes the gradient of
    the output row it went into, times size_t / size_out_row where that row is an average of several (copied rows: times exactly 1)"""
    unm, src, dst = (t.long() for t in plan)
    B, no, D = dy.shape
    r = src.shape[1]
    n = no + r
    na = unm.shape[1]
    dy, size_out = dy.double(), size_out.double()
    size = torch.ones((B, n), dtype=torch.float64) if size is None else size.double()
    dx = torch.zeros((B, n, D), dtype=torch.float64)
    for b in range(B):
        for o, u in enumerate(unm[b].tolist()):
            dx[b, 2 * u] = dy[b, o]
        merged = set(dst[b].tolist())
        for j in range(n // 2):
            t, o = 2 * j + 1, na + j
            dx[b, t] = dy[b, o] * (size[b, t] / size_out[b, o]) if j in merged else dy[b, o]
        for p in range(r):
            t, o = 2 * int(src[b, p]), na + int(dst[b, p])
            dx[b, t] = dy[b, o] * (size[b, t] / size_out[b, o])
    return dx


def merge(x, size, plan):
    """tome_ref.merge's (x_out, size_out) in the dtype of x, vectorised (differentiable in x)"""
    unm, src, dst = (t.long() for t in plan)
    B, n, D = x.shape
    s = torch.ones((B, n), dtype=x.dtype) if size is None else size.to(x.dtype)
    a, b, sa, sb = x[:, 0::2], x[:, 1::2], s[:, 0::2], s[:, 1::2]
    ex = lambda idx: idx[..., None].expand(-1, -1, D)
    keep, keep_s = a.gather(1, ex(unm)), sa.gather(1, unm)
    if src.shape[1] == 0:
        return torch.cat([keep, b], dim=1), torch.cat([keep_s, sb], dim=1)
    num = (b * sb[..., None]).scatter_add(1, ex(dst), a.gather(1, ex(src)) * sa.gather(1, src)[..., None])
    den = sb.scatter_add(1, dst, sa.gather(1, src))
    hit = torch.zeros(sb.shape, dtype=torch.bool).scatter(1, dst, torch.ones(dst.shape, dtype=torch.bool))
    return torch.cat([keep, torch.where(hit[..., None], num / den[..., None], b)], dim=1), torch.cat([keep_s, den], dim=1)


def keyw_attention(qkv, key_w, scale):
    """tome_ref.keyw_attention's output in the dtype of qkv [B,n,3,H,64]"""
    B, n, _, H, dh = qkv.shape
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    S = (q @ k.transpose(-1, -2)) * scale + torch.log(key_w.to(qkv.dtype))[:, None, None, :]
    return (torch.softmax(S, dim=-1) @ v).transpose(1, 2).reshape(B, n, H * dh)


def block(x, p, H, eps, size, plan, prop_attn=True):
    """One merging block (tome_ref.model_forward's loop body) in the dtype of x [B,n,D]; plan None: r = 0.  -> (y [B,n-r,D], size_out)"""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = p
    B, n, D = x.shape
    qkv = F.linear(F.layer_norm(x, (D,), n1w, n1b, eps), qkvw, qkvb).reshape(B, n, 3, H, 64)
    kw = size.to(x.dtype) if (size is not None and prop_attn) else torch.ones((B, n), dtype=x.dtype)
    x1 = x + F.linear(keyw_attention(qkv, kw, 64 ** -0.5), projw, projb)
    if plan is not None:
        x1, size = merge(x1, size, plan)
    return x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, (D,), n2w, n2b, eps), fc1w, fc1b)), fc2w, fc2b), size


def block_with_grads(x, p, H, eps, size, plan, gy, prop_attn=True, dtype=torch.float64):
    """-> (y, dx, [12 parameter gradients]) of block() evaluated in `dtype`"""
    xd = x.to(dtype).requires_grad_(True)
    pd = [t.to(dtype).requires_grad_(True) for t in p]
    y, _ = block(xd, pd, H, eps, size, plan, prop_attn)
    grads = torch.autograd.grad(y, [xd] + pd, gy.to(dtype))
    return y.detach(), grads[0], list(grads[1:])


def keyw_attention_grad(qkv, key_w, scale, dout):
    """d/dqkv of sum(tome_ref.keyw_attention(qkv, key_w, scale)[0] * dout) in float64"""
    q = qkv.double().requires_grad_(True)
    out, _ = R.keyw_attention(q, key_w, scale)
    out.backward(dout.double().reshape(out.shape))
    return q.grad


def model_grads(state_dict, images, r, plans, prop_attn=True):
    """tome_ref.model_forward with the plans replayed -> (logits, {name: d logits.sum() / d parameter}) in float64"""
    sd = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in state_dict.items()}
    logits, _ = R.model_forward(sd, images, r, plans=plans, prop_attn=prop_attn)
    names = list(sd)
    grads = torch.autograd.grad(logits.sum(), [sd[k] for k in names], allow_unused=True)
    return logits.detach(), dict(zip(names, grads))


def tome_loss(logits_s, logits_t, labels, cls_weight=1.0, dist_weight=0.5):
    """cls_weight * CE + dist_weight * KL(log_softmax(s) || log_softmax(t)) (batchmean), float64.  labels: [B] class ids or [B,C] soft
    targets; logits_t None or dist_weight 0: no teacher term."""
    ls = torch.log_softmax(logits_s.double(), dim=-1)
    if labels.dim() == 1:
        ce = -ls.gather(1, labels.long()[:, None]).mean()
    else:
        ce = -(labels.double() * ls).sum(dim=-1).mean()
    loss = cls_weight * ce
    if logits_t is not None and dist_weight != 0.0:
        lt = torch.log_softmax(logits_t.double(), dim=-1)
        loss = loss + dist_weight * (lt.exp() * (lt - ls)).sum(dim=-1).mean()
    return loss
