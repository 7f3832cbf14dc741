"""Differentiable token selection on the GPU: the three soft-gather products (csrc/softgather.hip) against float64 with derived bounds,
their one-hot and determinism properties, the student with the reference's noise injected against tests/golden/difftopk_micro.npz and the
float64 restatement (tests/difftopk_ref.py), the capability itself (the predictor gets a gradient from the backbone outputs), the hard
limit sigma -> 0, TrainStep reproducibility / resume / refusals, and one full-size step.  Every step runs once."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import difftopk_ref as R
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

SHAPES = [(3, 196, 98, 384), (2, 137, 98, 384), (2, 98, 58, 384), (2, 576, 172, 768), (4, 16, 8, 128), (1, 33, 1, 64)]


def _ops():
    from d2s import ops
    return ops


def _inputs(B, N, k, D, seed=0):
    gen = torch.Generator().manual_seed(seed + 1000 * N + k)
    x = torch.randn((B, N + 1, D), generator=gen)
    ind = torch.rand((B, k, N), generator=gen)
    ind = ind / ind.sum(dim=-1, keepdim=True)           # dense rows that sum to 1, like early-training indicators
    g = torch.randn((B, k + 1, D), generator=gen)
    return x, ind, g


# ---- 1. kernels against float64 ----
@pytest.mark.parametrize("B,N,k,D", SHAPES)
def test_products_against_float64_within_the_derived_bounds(B, N, k, D):
    """A length-L fp32 dot product accumulated in any order errs by at most (L - 1 + 1) u sum|a_i b_i| to first order (u = 2^-24: one
    rounding per product - the MFMA's fused multiply-adds have none, it is counted anyway - and L - 1 per addition chain); the bound
    used is (L + 2) u sum|a b|, times 2 for the accumulation-order constant (second-order terms, the zero-padded K tail and the split of
    the chain over the two half-waves' k ranges).  L = N for y, k for dx, D for dind.  The CLS rows are copies: exact."""
    ops = _ops()
    x, ind, g = _inputs(B, N, k, D)
    xd, indd, gd = x.to(DEV), ind.to(DEV), g.to(DEV)
    y = ops.soft_gather_fwd(xd, indd).cpu()
    dx = ops.soft_gather_bwd_x(gd, indd, N + 1).cpu()
    dind = ops.soft_gather_bwd_ind(gd, xd).cpu()
    torch.cuda.synchronize()
    x64, i64, g64 = x.double(), ind.double(), g.double()
    assert y.shape == (B, k + 1, D) and dx.shape == (B, N + 1, D) and dind.shape == (B, k, N)
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(dx[:, 0], g[:, 0])
    checks = [("y", y[:, 1:], i64 @ x64[:, 1:], i64.abs() @ x64[:, 1:].abs(), N),
              ("dx", dx[:, 1:], i64.transpose(1, 2) @ g64[:, 1:], i64.abs().transpose(1, 2) @ g64[:, 1:].abs(), k),
              ("dind", dind, g64[:, 1:] @ x64[:, 1:].transpose(1, 2), g64[:, 1:].abs() @ x64[:, 1:].abs().transpose(1, 2), D)]
    for name, got, want, mag, L in checks:
        bound = 2.0 * (L + 2) * EPS * mag
        err = (got.double() - want).abs()
        frac = float((err / bound).max())
        print(f"[softgather {B}x{N}x{k}x{D}] {name}: largest fraction of the bound {frac:.3f}, max abs err {float(err.max()):.3e}")
        assert bool((err <= bound).all()), (name, frac)


# ---- 2. one-hot indicators: the hard gather / scatter bit for bit ----
@pytest.mark.parametrize("B,N,k,D", SHAPES)
def test_one_hot_indicators_give_the_hard_gather_and_scatter_bits(B, N, k, D):
    """1.0 * x plus exact zeros (finite inputs): no rounding anywhere"""
    ops = _ops()
    x, _, g = _inputs(B, N, k, D, seed=1)
    gen = torch.Generator().manual_seed(7)
    ids = torch.stack([torch.sort(torch.randperm(N, generator=gen)[:k])[0] for _ in range(B)]).to(torch.int64)
    ind = torch.nn.functional.one_hot(ids, N).float()
    xd, indd, gd, idsd = x.to(DEV), ind.to(DEV), g.to(DEV), ids.to(DEV)
    assert torch.equal(ops.soft_gather_fwd(xd, indd), ops.gather_pack(xd, idsd))
    assert torch.equal(ops.soft_gather_bwd_x(gd, indd, N + 1), ops.scatter_unpack(gd, idsd, N + 1))


# ---- 3. determinism ----
@pytest.mark.parametrize("B,N,k,D", SHAPES)
def test_two_runs_are_bit_identical(B, N, k, D):
    ops = _ops()
    x, ind, g = (t.to(DEV) for t in _inputs(B, N, k, D, seed=2))
    run = lambda: (ops.soft_gather_fwd(x, ind), ops.soft_gather_bwd_x(g, ind, N + 1), ops.soft_gather_bwd_ind(g, x))
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_softmax_rows_backward_against_float64():
    ops = _ops()
    gen = torch.Generator().manual_seed(3)
    s, g = torch.randn((37, 196), generator=gen), torch.randn((37, 196), generator=gen)
    p = ops.softmax_rows(s.to(DEV))
    dz = ops.softmax_rows_bwd(p, g.to(DEV)).cpu()
    s64 = s.double().requires_grad_(True)
    torch.softmax(s64, dim=-1).backward(g.double())
    np.testing.assert_allclose(dz.numpy(), s64.grad.numpy(), rtol=1e-4, atol=1e-7)


# ---- 4. the model with the fixture's noise ----
def _student(case, diff_topk, nS=16, **kw):
    import vit_models
    cfg = case["cfg"]
    student, teacher, _, _ = build_models(case, torch.device(DEV))
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    m = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
                                                topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                small_predictor=cfg["small_predictor"], init_n=cfg["init_n"], diff_topk=diff_topk,
                                                topk_num_samples=nS, **common, **kw)
    m.load_state_dict(student.state_dict(), strict=True)
    m.keep_topk_indicators = True
    return m.to(DEV), teacher


@pytest.mark.parametrize("tag", ["m1", "m2"])
def test_student_with_the_fixture_noise_matches_the_reference_composition(tag):
    """First the condition that makes exact indicator equality meaningful: twice the largest difference between the GPU's keep
    probabilities and the fixture's stays below the stored margin (a hard assert).  Then indicators and kept ids exactly; logits, features,
    predictor logits and the probe's predictor gradients at the tolerances tests/test_model_gpu.py applies to these quantities (1e-4 /
    2e-5, features atol 3e-5, gradient norms 1e-3, leading elements 5e-3, full tensors 3e-3 relative L2 against float64)."""
    from d2s import synth
    ops = _ops()
    g = cases.load_golden("difftopk_micro")
    case, noises, sigma = R.fixture_case(g, tag)
    cfg = case["cfg"]
    student, _ = _student(case, True, nS=int(g[f"{tag}_num_samples"]))
    student.train()
    student.current_sigma = sigma
    student.topk_noise = noises
    x = _t(synth.images(case["batch"], 3, cfg["img_size"], seed=case["seed"])).to(DEV)
    logits, features, pred_logits, kept = student(x)
    margin = float(g[f"{tag}_margin"])
    for i in range(len(kept)):
        p_gpu = ops.softmax_rows(pred_logits[i].detach().contiguous()).cpu().numpy()
        dp = float(np.abs(p_gpu - g[f"{tag}_probs_{i}"]).max())
        print(f"[difftopk {tag}] stage {i}: max |p_gpu - p_fixture| = {dp:.3e}, margin {margin:.3e}")
        assert 2.0 * dp < margin, (i, dp, margin)
    for i in range(len(kept)):
        np.testing.assert_array_equal(student.topk_indicators[i].cpu().numpy(), g[f"{tag}_ind_{i}"])
        np.testing.assert_array_equal(kept[i].cpu().numpy(), g[f"{tag}_kept_{i}"])
        np.testing.assert_allclose(pred_logits[i].detach().cpu().numpy(), g[f"{tag}_pred_logits_{i}"], rtol=1e-4, atol=2e-5)
    ref64 = R.run_fixture_case(g, tag, torch.float64)
    for want in (g[f"{tag}_logits"], ref64["logits"].float().numpy()):
        np.testing.assert_allclose(logits.detach().cpu().numpy(), want, rtol=1e-4, atol=2e-5)
    for want in (g[f"{tag}_features"], ref64["features"].float().numpy()):
        np.testing.assert_allclose(features.detach().cpu().numpy(), want, rtol=1e-4, atol=3e-5)
    loss = R.probe_loss(tag, case["seed"], logits, features)
    np.testing.assert_allclose(float(loss.detach()), float(g[f"{tag}_probe_loss"]), rtol=1e-4, atol=2e-5)
    loss.backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    params = dict(student.named_parameters())
    worst = 0.0
    for n, ref_norm, ref_head in zip([str(v) for v in g[f"{tag}_grad_names"]], g[f"{tag}_grad_norms"], g[f"{tag}_grad_heads"]):
        assert params[n].grad is not None, n
        gf = params[n].grad.detach().flatten().cpu()
        np.testing.assert_allclose(float(gf.double().norm()), ref_norm, rtol=1e-3, atol=1e-6, err_msg=n)
        m = min(8, gf.numel())
        np.testing.assert_allclose(gf[:m].numpy(), ref_head[:m], rtol=5e-3, atol=5e-4 * float(np.abs(ref_head[:m]).max()) + 2e-6, err_msg=n)
        g64 = ref64["grads"][n].flatten()
        if float(g64.norm()) > 1e-6:
            err = float((gf.double() - g64).norm()) / float(g64.norm())
            worst = max(worst, err)
            assert err < 3e-3, (n, err)
    print(f"[difftopk {tag}] worst relative predictor-gradient error vs the float64 restatement: {worst:.2e}")
    # the layers in front of the first stage receive their whole gradient through soft_gather_bwd_x (dx = ind^T g) plus the predictor's
    # input gradient: every parameter of the student against the float64 restatement, full tensors, 3e-3 relative L2 as above
    worst_all, upstream = 0.0, 0
    for n, p_ in params.items():
        g64 = ref64["grads"][n]
        if g64 is None or float(g64.norm()) <= 1e-6:
            continue
        assert p_.grad is not None, n
        err = float((p_.grad.detach().cpu().double().flatten() - g64.flatten()).norm()) / float(g64.norm())
        worst_all = max(worst_all, err)
        assert err < 3e-3, (n, err)
        upstream += n.startswith(("patch_embed.", "blocks.0.", "cls_token", "pos_embed"))
    assert upstream >= 14
    print(f"[difftopk {tag}] worst relative gradient error over all parameters vs the float64 restatement: {worst_all:.2e}")


@pytest.mark.parametrize("small", [False, True])
def test_recomputed_keep_probabilities_are_the_predictors_own_bits(small):
    """`kept` comes from the predictor's keep_probs, `ind` from KeepProbsFn(scores): they agree only if the two are the same bits"""
    import vit_models
    from d2s import functional as DF
    torch.manual_seed(6)
    pred = vit_models.PredictorLG(128, topk_selection=True, k=9, small_predictor=small, loss_type="kl_div").to(DEV).train()
    x = torch.randn(5, 17, 128, device=DEV, requires_grad=True)
    scores, probs = pred.forward_tokens(x)
    again = DF.KeepProbsFn.apply(scores)
    assert torch.equal(again.detach(), probs.detach()) and again.requires_grad and not probs.requires_grad


# ---- 5. the capability ----
def test_backbone_outputs_give_the_predictor_a_gradient_only_with_diff_topk():
    """with the hard gather the predictor gets no gradient from the logits; with the soft gather every tensor does"""
    ops = _ops()
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    for on in (True, False):
        student, _ = _student(case, on)
        student.train()
        torch.manual_seed(3)
        student(x)[0].sum().backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        grads = {n: p.grad for n, p in student.named_parameters() if n.startswith("score_predictor.")}
        assert len(grads) == 48
        for n, gr in grads.items():
            if on:
                assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0.0, n
            else:
                assert gr is None, n


# ---- 6. the hard limit ----
def test_tiny_sigma_is_the_hard_path_and_eval_ignores_the_mode():
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    soft, _ = _student(case, True)
    hard, _ = _student(case, False)
    soft.train(), hard.train()
    soft.current_sigma = 1e-12          # p + sigma * noise rounds to p in fp32: one-hot indicators
    torch.manual_seed(4)
    ls, fs, _, ks = soft(x)
    lh, fh, _, kh = hard(x)
    for ind, kept in zip(soft.topk_indicators, ks):
        assert torch.equal(ind, torch.nn.functional.one_hot(kept, ind.shape[-1]).float())
    assert torch.equal(ls, lh) and torch.equal(fs, fh)
    assert all(torch.equal(a, b) for a, b in zip(ks, kh))
    soft.current_sigma = 0.0            # sigma <= 0: the hard gather itself
    l0 = soft(x)[0]
    assert torch.equal(l0, lh) and soft.topk_indicators == []
    soft.eval(), hard.eval()
    for sigma in (0.05, 1.0):
        soft.current_sigma = sigma
        with torch.no_grad():
            a, b = soft(x), hard(x)
        assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
    soft.train(), hard.train()
    with torch.no_grad():
        assert torch.equal(soft(x)[0], hard(x)[0]), "forward-only paths keep the hard gather"


def test_noise_follows_torch_manual_seed():
    case = cases.MODEL_CASES["micro1"]
    x = _t(cases.make_images(case)).to(DEV)
    m, _ = _student(case, True)
    m.train()

    def run(seed):
        torch.manual_seed(seed)
        out = m(x)[0].detach().clone()
        return out, m.topk_indicators[0].clone()
    (a, ia), (b, ib), (c, ic) = run(1), run(1), run(2)
    assert torch.equal(a, b) and torch.equal(ia, ib) and not torch.equal(ia, ic)
    np.testing.assert_allclose(ia.sum(dim=-1).cpu().numpy(), 1.0, rtol=0, atol=16 * EPS)


# ---- 7. TrainStep ----
def _steps(case, on, n, seed=5, resume_after=None):
    from d2s.engine import TrainStep
    student, teacher = _student(case, on)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=False)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(seed)
    rec, sd = [], None
    for i in range(n):
        info = ts(x, y)
        torch.cuda.synchronize()
        rec.append((info["loss"].detach().clone(), ts.arena.params.clone()))
        if resume_after is not None and i + 1 == resume_after:
            sd = ts.state_dict(epoch=0)
    return rec, sd


@pytest.mark.parametrize("name", ["micro1", "micro2"])
def test_train_step_is_reproducible_differs_from_the_hard_path_and_resumes_bit_identically(name):
    from d2s.engine import TrainStep
    from d2s import lib
    case = cases.MODEL_CASES[name]
    a, sd = _steps(case, True, 4, resume_after=2)
    b, _ = _steps(case, True, 4)
    z, _ = _steps(case, False, 4)
    for i in range(4):
        assert torch.equal(a[i][0], b[i][0]) and torch.equal(a[i][1], b[i][1]), i
    assert not torch.equal(a[3][1], z[3][1])
    assert sd["config"]["diff_topk"] is True and sd["config"]["topk_num_samples"] == 16
    student, teacher = _student(case, True)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=False)
    torch.manual_seed(999)                       # the checkpoint's generator state must win
    ts.load_state_dict(sd)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    for i in (2, 3):
        info = ts(x, y)
        torch.cuda.synchronize()
        assert torch.equal(info["loss"].detach(), a[i][0]) and torch.equal(ts.arena.params, a[i][1]), i
    student0, teacher0 = _student(case, False)
    ts0 = TrainStep(student0, teacher0, make_args(case["cfg"]), warmup_steps=0, graph=False)
    with pytest.raises(lib.D2SError, match="diff_topk"):
        ts0.load_state_dict(sd)
    old = dict(sd, config={k: v for k, v in sd["config"].items() if k not in ("diff_topk", "topk_num_samples")})
    with pytest.raises(lib.D2SError, match="diff_topk"):
        ts.load_state_dict(old)                 # a checkpoint without the keys counts as off


def _warmup_steps(case, on, seed=5):
    """epoch 0 with warmup_steps=1 (backbone frozen: the stage input needs no gradient, SoftGatherFn returns dind only), then epoch 1"""
    from d2s.engine import TrainStep
    student, teacher = _student(case, on)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=1, graph=False)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(seed)
    names = [n for n, _ in student.named_parameters()]
    rec = [{n: p.detach().clone() for n, p in student.named_parameters()}]
    for epoch in (0, 1):
        ts.set_epoch(epoch)
        info = ts(x, y)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(info["loss"]))
        rec.append({n: p.detach().clone() for n, p in student.named_parameters()})
    return names, rec


@pytest.mark.parametrize("name", ["micro1", "micro2"])
def test_train_step_in_the_warm_up_epoch(name):
    """The frozen-backbone epoch: only the predictors move, bit-reproducibly.  Its loss is the mask loss alone (train.py:50-53), which
    reaches a stage's predictor directly and, through the soft-gathered tokens, the predictors of the stages before it: with one stage
    (micro1) the update is the hard path's bit for bit, with two (micro2) both predictors move differently - stage 0 through
    SoftGatherFn's indicator gradient alone, its token input needing none.  The first full epoch then moves everything."""
    case = cases.MODEL_CASES[name]
    names, a = _warmup_steps(case, True)
    _, b = _warmup_steps(case, True)
    _, z = _warmup_steps(case, False)
    for n in names:
        assert torch.equal(a[1][n], b[1][n]) and torch.equal(a[2][n], b[2][n]), n
        if n.startswith("score_predictor."):
            assert not torch.equal(a[1][n], a[0][n]), n
        else:
            assert torch.equal(a[1][n], a[0][n]), n
    for stage in range(len(case["cfg"]["pruning_loc"])):
        mine = [n for n in names if n.startswith(f"score_predictor.{stage}.")]
        if name == "micro1":
            assert all(torch.equal(a[1][n], z[1][n]) for n in mine)
        else:
            assert any(not torch.equal(a[1][n], z[1][n]) for n in mine), stage
    assert any(not torch.equal(a[2][n], z[2][n]) for n in names if n.startswith("score_predictor."))
    assert all(not torch.equal(a[2][n], a[1][n]) for n in ("blocks.0.attn.qkv.weight", "patch_embed.proj.weight", "head.weight"))


@pytest.mark.parametrize("collective,port", [("allreduce", 29561), ("rs_ag", 29563)])
def test_two_ranks_match_single_process_with_diff_topk(collective, port):
    """tools/ddp_check.py with the mode on (D2S_DDP_DIFF_TOPK=1): two ranks sharing the GPU, each injecting its slice of one shared noise
    tensor, against one process with the concatenated batch - epoch 0 (backbone frozen, hooks fire from the stage outputs against the
    predictor-only live set) and epoch 1.  Exit code 3 would mean the noise seed violates the margin condition, not a mismatch."""
    import os
    import subprocess
    import sys
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(cases.REPO, "tools", "ddp_check.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", D2S_DDP_COLLECTIVE=collective, D2S_DDP_DIFF_TOPK="1")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.count("[ddp_check] diff_topk epoch") == 2


def test_graph_mode_with_diff_topk_is_refused_at_construction():
    from d2s.engine import TrainStep
    from d2s import lib
    case = cases.MODEL_CASES["micro2"]
    student, teacher = _student(case, True)
    with pytest.raises(lib.D2SError, match="diff_topk"):
        TrainStep(student, teacher, make_args(case["cfg"]), graph=True)


def test_kept_token_override_in_training_is_refused():
    case = cases.MODEL_CASES["micro1"]
    x = _t(cases.make_images(case)).to(DEV)
    m, _ = _student(case, True)
    m.train()
    m.kept_token_override = [torch.arange(9).repeat(x.shape[0], 1)]
    with pytest.raises(RuntimeError, match="kept_token_override"):
        m(x)


# ---- 8. full size ----
def test_full_size_step_is_bit_reproducible_and_indicators_are_distributions():
    """B 128, DeiT-S, one stage at keep 0.5 (N 196 -> k 98), nS 500.  The integer sample counters and the ordered reductions of every
    kernel make two steps from the same seed bit-identical; a row of indicators is counts / nS over one sample's k-th id: it sums to 1
    (N roundings of 2^-24 at most), a column to at most 1."""
    import types
    import vit_models
    from d2s.engine import TrainStep
    B, N = 128, 196

    def run():
        torch.manual_seed(11)
        student = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                                   diff_topk=True).to(DEV)
        student.keep_topk_indicators = True
        teacher = vit_models.dynamic_vit_small_patch16_224_teacher().to(DEV)
        args = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", mixup=0.0, patch_score_threshold=None, step=0)
        ts = TrainStep(student, teacher, args, warmup_steps=0, graph=False)
        gen = torch.Generator().manual_seed(12)
        x = torch.randn((B, 3, 224, 224), generator=gen).to(DEV)
        y = torch.randint(0, 1000, (B,), generator=gen).to(DEV)
        info = ts(x, y)
        torch.cuda.synchronize()
        return info["loss"].detach().clone(), ts.arena.params.clone(), student.topk_indicators[0].clone()

    la, pa, ia = run()
    assert ia.shape == (B, 98, N) and bool(torch.isfinite(la))
    tol = N * EPS
    rows, cols = ia.double().sum(dim=-1), ia.double().sum(dim=1)
    print(f"[difftopk full] loss {float(la):.6f}; indicator rows sum within {float((rows - 1).abs().max()):.2e} of 1, "
          f"largest column sum {float(cols.max()):.6f}, non-zero fraction {float((ia > 0).float().mean()):.3f}")
    assert float((rows - 1).abs().max()) <= tol
    assert float(cols.max()) <= 1.0 + tol
    lb, pb, ib = run()
    assert torch.equal(ia, ib) and torch.equal(la, lb) and torch.equal(pa, pb)
