"""The yardstick of the loss-path kernel tests, tested: every restatement in tests/losspath_ref.py against independent ground truth
(torch.nn.functional, torch.optim.AdamW, the CPU oracle, element-by-element loops).  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O
from tests import losspath_ref as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_mode_numbers_are_the_ops_constants():
    from d2s import ops
    assert (R.KL_LOGIT_TARGET, R.KL_PROB_TARGET, R.CE_LABEL, R.MSE_TARGET, R.SOFT_CE) == \
           (ops.KL_LOGIT_TARGET, ops.KL_PROB_TARGET, ops.CE_LABEL, ops.MSE_TARGET, ops.SOFT_CE)


@pytest.mark.parametrize("rows,C", [(1, 1), (7, 65), (5, 1000)])
def test_row_loss_against_torch_functional(rows, C):
    g = _gen(rows * 1000 + C)
    s = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 3 + 30 * torch.sign(torch.randn(rows, 1, generator=g, dtype=torch.float64)))
    tl = torch.randn(rows, C, generator=g, dtype=torch.float64) * 3
    tp = torch.softmax(torch.randn(rows, C, generator=g, dtype=torch.float64) * 2, dim=-1)
    labels = torch.randint(0, C, (rows,), generator=g)
    w = torch.rand(rows, generator=g, dtype=torch.float64) * 2
    w[0] = 0.0

    def truth(fn):
        sg = s.clone().requires_grad_(True)
        loss = fn(sg)
        (grad,) = torch.autograd.grad((loss * w).sum(), sg)
        return (loss * w).detach(), grad

    soft = tp.clone()
    soft[:, ::2] = 0.0                                         # a mixup target: exact zeros
    want = {
        R.KL_LOGIT_TARGET: lambda x: F.kl_div(F.log_softmax(x, -1), F.log_softmax(tl, -1), log_target=True, reduction="none").sum(-1),
        R.KL_PROB_TARGET: lambda x: F.kl_div(F.log_softmax(x, -1), tp, reduction="none").sum(-1),
        R.CE_LABEL: lambda x: F.cross_entropy(x, labels, reduction="none"),
        R.MSE_TARGET: lambda x: F.mse_loss(x, tp, reduction="none").sum(-1),
        R.SOFT_CE: lambda x: torch.sum(-soft * F.log_softmax(x, dim=-1), dim=-1),         # timm SoftTargetCrossEntropy, per row
    }
    args = {R.KL_LOGIT_TARGET: dict(t=tl), R.KL_PROB_TARGET: dict(t=tp), R.CE_LABEL: dict(labels=labels), R.MSE_TARGET: dict(t=tp),
            R.SOFT_CE: dict(t=soft)}
    for mode, fn in want.items():
        loss, grad = R.row_loss(mode, s, row_weight=w, **args[mode])
        wl, wg = truth(fn)
        torch.testing.assert_close(loss, wl, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(grad, wg, rtol=1e-12, atol=1e-13)
        assert bool((grad[0] == 0).all()) and float(loss[0]) == 0.0               # the zero row weight
        loss1, grad1 = R.row_loss(mode, s, **args[mode])                          # no weights == unit weights
        wl1, wg1 = R.row_loss(mode, s, row_weight=torch.ones(rows, dtype=torch.float64), **args[mode])
        assert torch.equal(loss1, wl1) and torch.equal(grad1, wg1)


def test_adamw_step_against_torch_optim():
    """5 steps, two parameter groups; one tensor has no gradient in the first two steps, so its own step counter lags (the
    per-tensor t of adamw_step)."""
    g = _gen(3)
    b1, b2, eps = 0.9, 0.999, 1e-8
    shapes = [(7, 5), (11,), (3, 4)]
    hyper = [(1e-3, 0.05), (5e-4, 0.0), (1e-3, 0.05)]
    params = [torch.nn.Parameter(torch.randn(sh, generator=g, dtype=torch.float64)) for sh in shapes]
    opt = torch.optim.AdamW([{"params": [params[0], params[2]], "lr": 1e-3, "weight_decay": 0.05},
                             {"params": [params[1]], "lr": 5e-4, "weight_decay": 0.0}], betas=(b1, b2), eps=eps)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), 0) for p in params]
    for step in range(5):
        grads = [torch.randn(sh, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 3, (1,), generator=g)) for sh in shapes]
        for i, p in enumerate(params):
            p.grad = None if (i == 2 and step < 2) else grads[i].clone()
        opt.step()
        for i, (p, m, v, t) in enumerate(mine):
            if i == 2 and step < 2:
                continue
            lr, wd = hyper[i]
            p, m, v = R.adamw_step(p, grads[i], m, v, lr, wd, b1, b2, eps, t + 1)
            mine[i] = (p, m, v, t + 1)
        for i, p in enumerate(params):
            torch.testing.assert_close(mine[i][0], p.detach(), rtol=1e-12, atol=1e-15)
            if opt.state[p]:
                torch.testing.assert_close(mine[i][1], opt.state[p]["exp_avg"], rtol=1e-12, atol=0)
                torch.testing.assert_close(mine[i][2], opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=0)
                assert int(opt.state[p]["step"]) == mine[i][3]
    assert [t for (_, _, _, t) in mine] == [5, 5, 3]


def test_adamw_step_per_element_hyper_parameters_and_grad_scale():
    """tensors of lr / wd / t broadcast element by element; grad_scale multiplies the gradient first"""
    g = _gen(4)
    p, gr, m = (torch.randn(6, generator=g, dtype=torch.float64) for _ in range(3))
    v = torch.rand(6, generator=g, dtype=torch.float64)
    lr, wd, t = torch.tensor([1e-3, 0.0, 1e-3, 5e-4, 1e-3, 1e-3]), torch.tensor([0.05, 0.05, 0.0, 0.05, 0.05, 0.05]), [1, 2, 3, 1000, 1, 8]
    got = R.adamw_step(p, gr, m, v, lr.double(), wd.double(), 0.9, 0.999, 1e-8, t, grad_scale=1.0 / 3.0)
    for i in range(6):
        one = R.adamw_step(p[i:i + 1], gr[i:i + 1] / 3.0, m[i:i + 1], v[i:i + 1], float(lr[i]), float(wd[i]), 0.9, 0.999, 1e-8, t[i])
        for a, b in zip(got, one):
            torch.testing.assert_close(a[i:i + 1], b, rtol=1e-14, atol=0)
    assert float(got[0][1]) == float(p[1])                     # lr = 0: the parameter does not move, the moments do
    assert float(got[1][1]) != float(m[1])


def test_ema_step():
    e, p = torch.tensor([1.0, -2.0], dtype=torch.float64), torch.tensor([3.0, 5.0], dtype=torch.float64)
    torch.testing.assert_close(R.ema_step(e, p, 0.75), torch.tensor([1.5, -0.25], dtype=torch.float64), rtol=0, atol=0)
    assert torch.equal(R.ema_step(e, p, 0.0), p)


@pytest.mark.parametrize("B,T", [(1, 1), (2, 5), (2, 33)])
def test_performer_against_the_oracle_pieces(B, T):
    g = _gen(B * 100 + T)
    kqv = torch.randn(B * T, 192, generator=g, dtype=torch.float64) * 0.5
    w = torch.randn(32, 64, generator=g, dtype=torch.float64)
    out = R.performer(kqv, w, B, T, 1e-8)
    k, q, v = torch.split(kqv.view(B, T, 192), 64, dim=-1)
    kp, qp = O.prm_exp(k, w), O.prm_exp(q, w)                                    # the oracle's lines of Token_performer.single_attn
    D = torch.einsum("bti,bi->bt", qp, kp.sum(dim=1)).unsqueeze(dim=2)
    kptv = torch.einsum("bin,bim->bnm", v, kp)
    y = torch.einsum("bti,bni->btn", qp, kptv) / (D.repeat(1, 1, 64) + 1e-8)
    torch.testing.assert_close(out["kp"].view(B, T, 32), kp, rtol=1e-13, atol=0)
    torch.testing.assert_close(out["qp"].view(B, T, 32), qp, rtol=1e-13, atol=0)
    torch.testing.assert_close(out["A"], kptv, rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(out["ksum"], kp.sum(dim=1), rtol=1e-13, atol=0)
    torch.testing.assert_close(out["D"].view(B, T, 1), D, rtol=1e-12, atol=0)
    torch.testing.assert_close(out["y"].view(B, T, 64), y, rtol=1e-11, atol=1e-14)
    # the backward is autograd through it: check it against central differences of the scalar it differentiates
    gy = torch.randn(B * T, 64, generator=g, dtype=torch.float64)
    skip = torch.randn(B * T, 64, generator=g, dtype=torch.float64)
    dk = R.performer_backward(kqv, w, B, T, 1e-8, gy, skip)
    dk0 = R.performer_backward(kqv, w, B, T, 1e-8, gy, None)
    assert torch.equal(dk[:, :128], dk0[:, :128])
    torch.testing.assert_close(dk[:, 128:] - dk0[:, 128:], skip, rtol=1e-10, atol=1e-12)
    f = lambda x: float((R.performer(x, w, B, T, 1e-8)["y"] * gy).sum() + (x[:, 128:] * skip).sum())
    for (r, c) in ((0, 3), (B * T - 1, 70), (B * T // 2, 130)):
        h = 1e-6
        e = torch.zeros_like(kqv)
        e[r, c] = h
        fd = (f(kqv + e) - f(kqv - e)) / (2 * h)
        assert abs(fd - float(dk[r, c])) <= 1e-6 * max(1.0, abs(fd)), (r, c, fd, float(dk[r, c]))


def test_teacher_target_and_gather_renorm():
    g = _gen(5)
    B, L, H, n = 3, 4, 2, 11
    a = torch.softmax(torch.randn(B, L, H, n, generator=g, dtype=torch.float64), dim=-1)
    got = R.teacher_target(a)
    torch.testing.assert_close(got, O.teacher_target(a), rtol=1e-14, atol=0)
    for b in range(B):                                                            # and element by element
        w = [max(sum(float(a[b, l, h, t]) for l in range(L)) / L for h in range(H)) for t in range(1, n)]
        np.testing.assert_allclose(got[b].numpy(), np.array(w) / sum(w), rtol=1e-13)
    np.testing.assert_allclose(got.sum(-1).numpy(), 1.0, rtol=1e-14)
    ids = torch.stack([torch.sort(torch.randperm(n - 1, generator=g)[:6])[0] for _ in range(B)])
    raw, ren = R.gather_renorm(got, ids, False), R.gather_renorm(got, ids, True)
    for b in range(B):
        vals = [float(got[b, int(j)]) for j in ids[b]]
        assert raw[b].tolist() == vals
        np.testing.assert_allclose(ren[b].numpy(), np.array(vals) / sum(vals), rtol=1e-14)


def test_mask_helpers():
    T = 9
    a, b = torch.tensor([[0, 2, 4, 6], [1, 3, 5, 7]]), torch.tensor([[0, 2, 5, 7], [0, 2, 4, 6]])
    assert R.mask_agreement(a, b, T).tolist() == [T - 4, T - 8]                # T - 2 (k - |intersection|)
    assert R.mask_agreement(a[:, :0], b[:, :0], T).tolist() == [T, T]
    assert R.mask_agreement(a, a, T).tolist() == [T, T]
    ma, mb = torch.tensor([[1., 0., 1., 1.], [0., 0., 0., 0.]]), torch.tensor([[1., 1., 1., 0.], [0., 0., 0., 0.]])
    assert R.dense_mask_agreement(ma, mb).tolist() == [2, 4]
    assert R.mask_row_weights(ma.double()).tolist() == [1 / 3, 0, 1 / 3, 1 / 3, 0, 0, 0, 0]
    assert R.mask_row_weights(torch.zeros(2, 3)).tolist() == [0.0] * 6


def test_act_grad_against_autograd():
    z = torch.tensor([0.0, -0.0, 8.0, -8.0, 1e-4, -1e-4, 0.7, -1.3], dtype=torch.float64, requires_grad=True)
    g = torch.linspace(-2, 2, 8, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.gelu(z), z, g)
    torch.testing.assert_close(R.act_grad(g, z.detach(), "gelu"), want, rtol=1e-13, atol=1e-16)
    (want,) = torch.autograd.grad(F.relu(z), z, g)
    assert torch.equal(R.act_grad(g, z.detach(), "relu"), want)


def test_error_measures():
    ref = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert R.rel_err(torch.tensor([3.0, 4.5]), ref) == pytest.approx(0.1)
    assert R.rel_err(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) == 0.0
    assert R.rel_err(torch.tensor([0.0, 1e-30]), torch.zeros(2, dtype=torch.float64)) == math.inf
    with pytest.raises(AssertionError):
        R.rel_err(torch.zeros(1), torch.tensor([float("nan")], dtype=torch.float64))
    assert R.sum_bound(9, 2.0, 1) == pytest.approx(11 * 2.0 ** -24 * 2.0, rel=2e-3)


@pytest.mark.parametrize("C", [63, 257, 1000])
def test_kl_rows_error_bound_covers_fp32_in_the_kernels_order(C):
    """The derived bound against plain fp32 arithmetic in the order it is derived for, s - (max + log sum), on rows offset by +-30
    (cross entropy: the loss is -ls_y, the gradient softmax - onehot); it carries the |lse| term, so it grows with the offset."""
    g = _gen(C)
    rows = 7
    base = (torch.randn(rows, C, generator=g) * 3.0).float()
    labels = torch.randint(0, C, (rows,), generator=g)
    bounds = []
    for off in (0.0, 30.0, -30.0):
        s = (base + off).float()
        M = s.max(dim=-1, keepdim=True)[0]
        ls = s - (M + torch.log(torch.exp(s - M).sum(dim=-1, keepdim=True)))             # fp32, the maximum put back before the subtraction
        loss32 = -ls.gather(1, labels[:, None])[:, 0]
        grad32 = ls.exp() - torch.zeros_like(s).scatter_(1, labels[:, None], 1.0)
        ref_l, ref_g = R.row_loss(R.CE_LABEL, s.double(), labels=labels)
        bl, bg = R.kl_rows_error_bound(R.CE_LABEL, s.double(), labels=labels)
        assert 0 < R.rel_err(loss32, ref_l) <= bl and 0 < R.rel_err(grad32, ref_g) <= bg
        bounds.append(bg)
    assert bounds[1] > bounds[0] and bounds[2] > bounds[0]
    assert R.kl_rows_error_bound(R.MSE_TARGET, base.double(), base.double()) == (0.0, 0.0)
