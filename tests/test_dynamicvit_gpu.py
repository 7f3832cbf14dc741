"""GPU tier of the DynamicViT baseline: the policy gradient of the attention backward, the Gumbel keep / pooling / noise kernels, and the
student with injected noise against the reference's fixture and the float64 restatement."""
import math

import numpy as np
import pytest
import torch

from tests import dynamicvit_cases as DC
from tests import dynamicvit_ref as R

import vit_models.default_dynamic_vit as DV
from d2s import ops
from d2s.functional_dynamicvit import DynPredictorFn, GumbelKeepFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _policies(kind, B, n, gen):
    if kind == "uniform":
        p = torch.rand(B, n, generator=gen)
    elif kind == "binary":
        p = (torch.rand(B, n, generator=gen) > 0.5).float()
    elif kind == "ones":
        p = torch.ones(B, n)
    else:                       # one image keeps a single patch token
        p = (torch.rand(B, n, generator=gen) > 0.5).float()
        p[0] = 0.0
        p[0, min(3, n - 1)] = 1.0
    p[:, 0] = 1.0
    return p


@pytest.mark.parametrize("B,H,n", [(2, 2, 17), (2, 2, 33), (3, 2, 64), (2, 3, 99), (1, 6, 197)])
@pytest.mark.parametrize("kind", ["uniform", "binary", "ones", "single"])
def test_dpolicy_against_float64_autograd(B, H, n, kind):
    """dpolicy[b, j] = sum_h sum_{i != j} w_hij.  Bound (the form of DESIGN section 14): each of the L = H (n - 1) summands carries a few
    roundings of its own and the sum L - 1 more: |err| <= 2 (L + 2) 2^-24 sum |w_hij|, the summands taken from the float64 reference.
    dqkv must be the plain policy backward's bits and two launches the same bits."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * H + B)
    qkv = torch.randn(B, n, 3 * H * 64, generator=gen)
    dout = torch.randn(B, n, H * 64, generator=gen)
    pol = _policies(kind, B, n, gen)
    scale = 64 ** -0.5
    q64 = qkv.double()
    # float64: gradient w.r.t. the full mask m [B, H, n, n] gives the summands; autograd w.r.t. the policy gives the sum
    p64 = pol.double().requires_grad_(True)
    o64 = R.policy_attention(q64, p64, H, scale)
    (want,) = torch.autograd.grad((o64 * dout.double()).sum(), p64)
    qh, kh, vh = q64.reshape(B, n, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (qh @ kh.transpose(-2, -1)) * scale
    m = pol.double().reshape(B, 1, 1, n)
    eye = torch.eye(n, dtype=torch.float64).view(1, 1, n, n)
    mfull = (m + (1 - m) * eye).expand(B, H, n, n).clone().requires_grad_(True)
    e = (s - s.max(-1, keepdim=True)[0]).exp() * mfull
    a = (e + 1e-6 / n) / (e.sum(-1, keepdim=True) + 1e-6)
    (w,) = torch.autograd.grad(((a @ vh).transpose(1, 2).reshape(B, n, H * 64) * dout.double()).sum(), mfull)
    w = w * (1 - eye)
    np.testing.assert_allclose(w.sum(dim=(1, 2))[:, 1:].numpy(), want[:, 1:].numpy(), rtol=1e-9, atol=1e-12)      # the formula itself
    bound = 2 * (H * (n - 1) + 2) * U * w.abs().sum(dim=(1, 2))

    qd, pd, dd = qkv.view(B * n, -1).to(DEV), pol.to(DEV), dout.view(B * n, -1).to(DEV)
    out, lse, cinv, _ = ops.attn_policy_fwd(qd, pd, B, n, H, scale)
    dqkv_ref = ops.attn_policy_bwd(qd, pd, out, dd, lse, cinv, B, n, H, scale)
    dqkv, dpol = ops.attn_policy_bwd_dpol(qd, pd, out, dd, lse, cinv, B, n, H, scale)
    dqkv2, dpol2 = ops.attn_policy_bwd_dpol(qd, pd, out, dd, lse, cinv, B, n, H, scale)
    torch.cuda.synchronize()
    assert torch.equal(dqkv, dqkv_ref), "dqkv differs from d2s_attn_policy_bwd_f32"
    assert torch.equal(dqkv, dqkv2) and torch.equal(dpol, dpol2), "two launches differ"
    got = dpol.cpu().double()
    assert torch.all(got[:, 0] == 0)
    err = (got - want)[:, 1:].abs()
    frac = float((err / bound[:, 1:]).max())
    print(f"dpolicy B{B} H{H} n{n} {kind}: max err / bound = {frac:.3f}")
    assert frac <= 1.0
    if kind in ("binary", "single"):      # a masked key still has a gradient: the straight-through signal
        masked = (pol[:, 1:] == 0)
        assert masked.any() and float(got[:, 1:][masked].abs().max()) > 0


def test_autograd_returns_policy_gradient_only_when_asked():
    from d2s import functional as DF
    B, H, n = 2, 2, 33
    gen = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * n, 3 * H * 64, generator=gen).to(DEV).requires_grad_(True)
    pol = _policies("uniform", B, n, gen).to(DEV)
    w = torch.randn(B * n, H * 64, generator=gen).to(DEV)
    o, _ = DF.AttnCoreFn.apply(qkv, B, n, H, 64 ** -0.5, False, pol)
    (g0,) = torch.autograd.grad((o * w).sum(), [qkv])
    polg = pol.clone().requires_grad_(True)
    o, _ = DF.AttnCoreFn.apply(qkv, B, n, H, 64 ** -0.5, False, polg)
    g1, gp = torch.autograd.grad((o * w).sum(), [qkv, polg])
    assert torch.equal(g0, g1) and gp.shape == pol.shape and float(gp.abs().max()) > 0


@pytest.mark.parametrize("N", [16, 33, 196])
def test_gumbel_keep_and_pool_against_float64(N):
    B, D = 3, 128
    gen = torch.Generator().manual_seed(N)
    z = torch.randn(B * N, 2, generator=gen)
    g = -torch.log(-torch.log(torch.rand(B, N, 2, generator=gen).clamp(1e-6, 1 - 1e-6)))
    prev = (torch.rand(B, N, generator=gen) > 0.3).float()
    assert (prev == 0).any()
    wd = torch.randn(B, N, generator=gen)
    z64 = z.double().requires_grad_(True)
    p64 = prev.double().requires_grad_(True)
    logp64 = torch.log_softmax(z64, -1).view(B, N, 2)
    a = logp64 + g.double()
    assert float((a[..., 0] - a[..., 1]).detach().abs().min()) >= 2e-5      # the margin: `hard` is then exact
    dec64, hard64, _ = R.gumbel_keep(logp64, g.double(), p64)
    gz64, gp64 = torch.autograd.grad((dec64 * wd.double()).sum(), [z64, p64])
    zd, pd = z.to(DEV).requires_grad_(True), prev.to(DEV).requires_grad_(True)
    dec, logp = GumbelKeepFn.apply(zd, g.to(DEV), pd)
    gz, gp = torch.autograd.grad((dec * wd.to(DEV)).sum(), [zd, pd])
    assert torch.equal(dec.detach().cpu().double(), dec64.detach())
    np.testing.assert_allclose(logp.cpu().numpy(), logp64.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gz.cpu().numpy(), gz64.numpy(), rtol=2e-5, atol=1e-7)
    assert torch.equal(gp.cpu().double(), gp64)
    # pooling: real-valued policy with zeros
    C = D
    x = torch.randn(B, N, C, generator=gen)
    p = torch.rand(B, N, generator=gen) * prev
    go = torch.randn(B, N, C, generator=gen)
    x64, pp64 = x.double().requires_grad_(True), p.double().requires_grad_(True)
    o64 = R.policy_pool(x64, pp64)
    gx64, gpp64 = torch.autograd.grad((o64 * go.double()).sum(), [x64, pp64])
    xd, pdv = x.view(B * N, C).to(DEV), p.to(DEV)
    o, psum, glob = ops.policy_pool_fwd(xd, pdv, B, N, C)
    dx, dp = ops.policy_pool_bwd(go.view(B * N, C).to(DEV), xd, pdv, psum, glob, B, N, C)
    # fp32 sums of N terms (forward, G) and of C/2 terms (the two dot products): (len + 2) 2^-24 times the sum of the magnitudes summed
    pmin = float(p.double().sum(1).min())
    xmax, gabs = float(x.abs().max()), go.double().abs().sum(1)[:, C // 2:]                 # gabs [B, C/2] bounds |G_c|
    np.testing.assert_allclose(o.cpu().view(B, N, C).numpy(), o64.detach().numpy(), rtol=0, atol=(N + 2) * U * xmax * float(p.sum(1).max()) / pmin)
    np.testing.assert_allclose(dx.cpu().view(B, N, C).numpy(), gx64.numpy(), rtol=0, atol=(N + 2) * U * float(gabs.max()) / pmin)
    np.testing.assert_allclose(dp.cpu().numpy(), gpp64.numpy(), rtol=0, atol=2 * (C // 2 + N + 4) * U * float(gabs.sum(-1).max()) * xmax / pmin)


def test_gumbel_noise():
    n = 100000
    a = ops.gumbel_noise((n,), 1234, DEV)
    b = ops.gumbel_noise((n,), 1234, DEV)
    c = ops.gumbel_noise((n,), 1235, DEV)
    assert torch.equal(a, b) and not torch.equal(a, c)
    x = a.double().cpu()
    var = math.pi ** 2 / 6
    assert abs(float(x.mean()) - 0.5772156649) <= 5 * math.sqrt(var / n)
    # Var of the sample variance ~ (mu4 - var^2) / n with mu4 = (12/5 + 3) var^2 for Gumbel (excess kurtosis 12/5)
    assert abs(float(x.var()) - var) <= 5 * math.sqrt((4.4 * var * var) / n)
    assert torch.isfinite(a).all()


def _build(case):
    cfg = case["cfg"]
    m = DV.DefaultVisionTransformerDiffPruning(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                                               num_heads=cfg["heads"], num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
                                               token_ratio=list(cfg["token_ratio"]), distill=True, init_n=cfg["init_n"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DC.make_weights(case).items()})
    return m.to(DEV)


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_student_against_fixture_and_float64(name):
    golden = np.load(DC.GOLDEN, allow_pickle=False)
    case = DC.CASES[name]
    cfg = case["cfg"]
    S = len(cfg["pruning_loc"])
    x = torch.from_numpy(DC.make_images(case))
    noise = [torch.from_numpy(golden[f"{name}/noise{i}"]) for i in range(S)]
    m = _build(case)
    m.train()
    m.gumbel_noise = noise
    logits, feats, final, decs = m(x.to(DEV))
    for i, d in enumerate(decs):
        assert np.array_equal(d.detach().cpu().numpy().astype(np.uint8), golden[f"{name}/decision{i}"]), f"stage {i} decisions"
    assert np.array_equal(final.cpu().numpy(), golden[f"{name}/final_decision"]) and not final.requires_grad
    np.testing.assert_allclose(logits.detach().cpu().numpy(), golden[f"{name}/logits"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(feats.detach().cpu().numpy(), golden[f"{name}/features"], rtol=1e-4, atol=3e-5)
    R.probe(dict(logits=logits, features=feats, decisions=list(decs)), cfg).backward()
    sd64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in DC.make_weights(case).items()}
    R.probe(R.forward(sd64, cfg, x, noise=noise), cfg).backward()
    worst = 0.0
    for k, p in m.named_parameters():
        want = sd64[k].grad
        assert p.grad is not None, k
        rel = float((p.grad.cpu().double() - want).norm() / want.norm())
        worst = max(worst, rel)
        assert rel <= 1e-3, f"{k}: relative L2 {rel:.2e}"
        if "score_predictor" in k:
            assert float(want.norm()) > 0
    print(f"{name}: worst relative L2 of a parameter gradient {worst:.2e}")
    # without injected noise: the same seed gives the same decisions
    m.gumbel_noise = None
    torch.manual_seed(7)
    d1 = m(x.to(DEV))[3]
    torch.manual_seed(7)
    d2 = m(x.to(DEV))[3]
    assert all(torch.equal(a, b) for a, b in zip(d1, d2))
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV))
    np.testing.assert_allclose(ev.cpu().numpy(), golden[f"{name}/eval_logits"], rtol=1e-4, atol=2e-5)


# ---- the objective and the fused step ----
def _loss_args(ratios, mixup=0.0):
    import types
    return types.SimpleNamespace(keep_ratios=list(ratios), mask_loss_type="kl_div", mixup=mixup, patch_score_threshold=None, step=0,
                                 warmup_steps=0, cls_weight=1.0, ratio_weight=2.0, dist_weight=0.5)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("B,N,D", [(4, 16, 128), (3, 33, 192), (5, 196, 384)])
def test_loss_against_float64_restatement(soft, B, N, D):
    """losses.DynamicViTLoss (row-loss, ratio and row-weight kernels) against tests/dynamicvit_ref.loss in float64: every term and every
    gradient.  Each term is an fp32 sum of at most max(D, N, B) <= 384 terms of one sign or of a log-softmax row, and a gradient element
    is a few roundings of its own: rtol 386 * 2^-24 = 2.3e-5 on the values, 2e-5 / 2e-7 on the gradients (expf within 2 ulp of a
    probability <= 1 scaled by 1 / B)."""
    import losses
    K = 10
    gen = torch.Generator().manual_seed(31 * N + B)
    r = lambda *s: torch.randn(*s, generator=gen)
    mask = (torch.rand(B, N, generator=gen) > 0.4).float()
    mask[0] = 0.0
    mask[0, N // 2] = 1.0
    ratios = [0.5, 0.25]
    t = dict(logits_s=r(B, K), feat_s=r(B, N, D), d0=(torch.rand(B, N, generator=gen) > 0.3).float(), d1=mask.clone(),
             logits_t=r(B, K), feat_t=r(B, N, D))
    labels = torch.softmax(r(B, K), -1) if soft else torch.randint(0, K, (B,), generator=gen)
    leaves64 = {k: t[k].double().requires_grad_(True) for k in ("logits_s", "feat_s", "d0", "d1")}
    want = R.loss(leaves64["logits_s"], leaves64["feat_s"], mask.double(), [leaves64["d0"], leaves64["d1"]], t["logits_t"].double(),
                  t["feat_t"].double(), labels.double() if soft else labels, ratios)
    gwant = torch.autograd.grad(want["total"], list(leaves64.values()))
    leaves = {k: t[k].to(DEV).requires_grad_(True) for k in leaves64}
    fn = losses.DynamicViTLoss(_loss_args(ratios, mixup=0.8 if soft else 0.0))
    metrics = {}
    got = fn(leaves["logits_s"], leaves["feat_s"], mask.to(DEV), [leaves["d0"], leaves["d1"]], t["logits_t"].to(DEV), t["feat_t"].to(DEV),
             labels.to(DEV), metrics)
    ggot = torch.autograd.grad(got, list(leaves.values()))
    tol = (max(D, N, B) + 2) * U
    for name, v in zip(("total", "cls", "ratio", "kl", "token"), fn.last):
        print(f"loss {name}: {float(v):.8f} want {float(want[name]):.8f}")
        assert float(v) == pytest.approx(float(want[name]), rel=tol, abs=1e-7), name
    assert float(metrics["train_dynamicvit_loss"]) == float(fn.last[0]) and all(torch.is_tensor(v) and v.is_cuda for v in metrics.values())
    for k, a, b in zip(leaves, ggot, gwant):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=2e-5, atol=2e-7, err_msg=k)
        assert float(b.abs().max()) > 0, k


def _train_step(**kw):
    from d2s.engine import TrainStep
    case = DC.CASES["stage1"]
    cfg = case["cfg"]
    student = _build(case)
    torch.manual_seed(3)
    teacher = DV.DefaultVisionTransformerTeacher(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                                                 num_heads=cfg["heads"], num_classes=cfg["num_classes"]).to(DEV)
    kw.setdefault("graph", False)
    return TrainStep(student, teacher, _loss_args(cfg["token_ratio"]), lr=1e-3, epochs=4, warmup_steps=0, **kw)


def _batch(i):
    gen = torch.Generator().manual_seed(100 + i)
    return torch.randn(4, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 10, (4,), generator=gen).to(DEV)


def test_train_step_two_runs_bit_identical_and_predictor_learns():
    runs = []
    for _ in range(2):
        step = _train_step()
        before = {k: v.detach().clone() for k, v in step.student.named_parameters()}
        torch.manual_seed(5)
        losses_ = [step(*_batch(i))["loss"].clone() for i in range(2)]
        runs.append((torch.stack(losses_), step.arena.params.clone()))
        assert torch.isfinite(runs[-1][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    moved = {k: not torch.equal(v, before[k]) for k, v in step.student.named_parameters()}
    assert all(moved[k] for k in moved if "score_predictor" in k), "every predictor parameter must move (policy gradient + pooling)"
    assert step.config()["model"] == "DefaultVisionTransformerDiffPruning"
    for k in ("train_dynamicvit_loss", "train_cls_loss", "train_ratio_loss", "train_cls_kl_loss", "train_token_mse_loss"):
        assert k in step.metrics


def test_train_step_resume_continues_bit_for_bit():
    from d2s import lib
    a = _train_step()
    torch.manual_seed(5)
    a(*_batch(0))
    sd = a.state_dict()
    a(*_batch(1))
    b = _train_step()
    with torch.no_grad():
        b.arena.params.add_(0.25)              # a run that starts elsewhere
    torch.manual_seed(99)
    b.load_state_dict(sd)
    b(*_batch(1))
    assert torch.equal(a.arena.params, b.arena.params)
    other = dict(sd, config=dict(sd["config"], model="VisionTransformerDiffPruning"))      # a d2s student's checkpoint is refused
    with pytest.raises(lib.D2SError, match="model"):
        b.load_state_dict(other)


def test_train_step_accumulation_and_clipping_run():
    step = _train_step(accum_steps=2, clip_grad=1.0)
    torch.manual_seed(5)
    before = step.arena.params.clone()
    i0 = step(*_batch(0))
    assert i0["stepped"] is False and torch.equal(before, step.arena.params)
    i1 = step(*_batch(1))
    assert i1["stepped"] is True and not torch.equal(before, step.arena.params)
    assert math.isfinite(float(i1["grad_norm"])) and float(i1["grad_norm"]) > 0
    assert torch.isfinite(step.arena.params).all()


def test_train_step_refuses_graph_capture():
    from d2s import lib
    with pytest.raises(lib.D2SError, match="DynamicViT baseline"):
        _train_step(graph=True)


def test_gumbel_conversion_is_finite_at_the_extreme_draws():
    """The bits -> Gumbel conversion of d2s_gumbel_noise at the ends of its range and around them: u must stay strictly inside (0, 1)
    (an all-ones draw must not round to u = 1, which gives +inf and NaN predictor gradients).  Expected values in float64 from
    u = (k + 0.5) 2^-23, k = bits >> 9, which is exact in fp32.  With E = -log u accurate to a few ulp, g = -log E moves by
    |dE| / E plus a few ulp of its own, about 1e-6 absolute at these magnitudes (|g| <= 17): rtol 1e-5 with atol 1e-5 near g = 0."""
    raw = [0x00000000, 0x000001FF, 0x00000200, 0x7FFFFFFF, 0x80000000, 0xFFFFFDFF, 0xFFFFFE00, 0xFFFFFF00, 0xFFFFFFFF]
    bits = torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in raw], dtype=torch.int32, device=DEV)
    g = ops.gumbel_from_bits(bits).cpu().double()
    assert torch.isfinite(g).all(), g
    u = (torch.tensor([v >> 9 for v in raw], dtype=torch.float64) + 0.5) * 2.0 ** -23
    assert float(u.min()) == 2.0 ** -24 and float(u.max()) == 1 - 2.0 ** -24
    want = -torch.log(-torch.log(u))
    np.testing.assert_allclose(g.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert float(g.max()) < 16.7 and float(g.min()) > -2.9
    # such noise goes through the keep decision and its backward without a NaN
    pairs = torch.tensor([[-1, 0], [0, -1], [-1, -1], [0, 0]], dtype=torch.int32, device=DEV)      # all-ones / zero draws in either slot
    z = torch.zeros(pairs.shape[0], 2, device=DEV)
    gg = ops.gumbel_from_bits(pairs.view(-1).contiguous()).view(-1, 2)
    logp, y0, hard, dec = ops.gumbel_keep_fwd(z, gg.contiguous(), torch.ones(z.shape[0], device=DEV))
    dz, dprev = ops.gumbel_keep_bwd(torch.ones(z.shape[0], device=DEV), torch.ones(z.shape[0], device=DEV), y0, hard)
    assert all(torch.isfinite(t).all() for t in (logp, y0, dec, dz, dprev))


def test_noise_streams_differ_by_rank_and_stage(monkeypatch):
    """One training forward draws one seed (torch's CPU generator mixed with the data-parallel rank) and offsets it per stage: the same
    torch seed gives the same streams again, another rank gives other streams, and the two stages of one forward differ."""
    import torch.distributed as dist
    case = DC.CASES["stage2"]
    m = _build(case)
    m.train()
    x = torch.from_numpy(DC.make_images(case)).to(DEV)
    seen = []
    real = ops.gumbel_noise

    def spy(shape, seed, device):
        out = real(shape, seed, device)
        seen.append((int(seed), out.clone()))
        return out
    monkeypatch.setattr(ops, "gumbel_noise", spy)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    for rank in (0, 1, 0):
        monkeypatch.setattr(dist, "get_rank", lambda group=None, r=rank: r)
        torch.manual_seed(7)
        m(x)
    assert len(seen) == 6                                          # two stages per forward
    (s00, g00), (s01, g01), (s10, g10), (s11, g11), (r00, h00), (r01, h01) = seen
    assert len({s00, s01, s10, s11}) == 4
    assert not torch.equal(g00, g01) and not torch.equal(g00, g10) and not torch.equal(g01, g11) and not torch.equal(g10, g11)
    assert (r00, r01) == (s00, s01) and torch.equal(g00, h00) and torch.equal(g01, h01)
