"""CPU tier of the DynamicViT baseline: the torch restatement (tests/dynamicvit_ref.py) reproduces the reference's fixture, the public
surface exists, and the library exports the new entries."""
import os

import numpy as np
import pytest
import torch

from tests import dynamicvit_cases as DC
from tests import dynamicvit_ref as R

import vit_models
import vit_models.default_dynamic_vit as DV
from d2s import lib

MARGIN = 2e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(DC.GOLDEN, allow_pickle=False)


def _sd(case, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in DC.make_weights(case).items()}


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_restatement_reproduces_fixture(golden, name):
    case = DC.CASES[name]
    cfg = case["cfg"]
    x = torch.from_numpy(DC.make_images(case))
    noise = [torch.from_numpy(golden[f"{name}/noise{i}"]) for i in range(len(cfg["pruning_loc"]))]
    sd = {k: v.requires_grad_(True) for k, v in _sd(case, torch.float32).items()}
    out = R.forward(sd, cfg, x, noise=noise)
    for i, d in enumerate(out["decisions"]):
        assert np.array_equal(d.detach().numpy().astype(np.uint8), golden[f"{name}/decision{i}"]), f"stage {i} decisions"
    assert np.array_equal(out["decisions"][-1].detach().numpy(), golden[f"{name}/final_decision"])
    np.testing.assert_allclose(out["logits"].detach().numpy(), golden[f"{name}/logits"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["features"].detach().numpy(), golden[f"{name}/features"], rtol=1e-5, atol=1e-6)
    ev = R.forward(_sd(case, torch.float32), cfg, x, training=False)
    np.testing.assert_allclose(ev["logits"].numpy(), golden[f"{name}/eval_logits"], rtol=1e-5, atol=1e-6)
    # the fixture's condition: no decision and no eval top-k boundary within the margin of a flip
    assert float(golden[f"{name}/gap"]) >= MARGIN and float(golden[f"{name}/eval_gap"]) >= MARGIN
    assert int(golden[f"{name}/seeds_qualified"]) * 2 >= int(golden[f"{name}/seeds_tried"])
    # probe gradients: float64 restatement against the reference's fp32 autograd, by norm and by strided samples
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    R.probe(R.forward(sd64, cfg, x, noise=noise), cfg).backward()
    names = sorted(sd64)
    norms, samples = golden[f"{name}/grad_norm"], golden[f"{name}/grad_sample"]
    for j, k in enumerate(names):
        g = sd64[k].grad
        np.testing.assert_allclose(float(g.norm()), norms[j], rtol=1e-4, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(DC.grad_sample(g).numpy(), samples[j], rtol=1e-3, atol=1e-5 * norms[j] + 1e-7, err_msg=k)
        if "score_predictor" in k:
            assert norms[j] > 0, f"{k}: the predictor must receive a gradient (through the policy of the masked softmax)"


def test_gumbel_keep_restatement_is_torch_gumbel_softmax():
    """gumbel_keep with the noise given == F.gumbel_softmax with the same draw (forward and straight-through backward), float64"""
    torch.manual_seed(3)
    logp = torch.log_softmax(torch.randn(5, 7, 2, dtype=torch.float64), -1).requires_grad_(True)
    prev = (torch.rand(5, 7, dtype=torch.float64) > 0.3).double().requires_grad_(True)
    torch.manual_seed(9)
    want = torch.nn.functional.gumbel_softmax(logp, hard=True)[..., 0] * prev
    torch.manual_seed(9)
    g = -torch.empty_like(logp).exponential_().log()
    got, _, _ = R.gumbel_keep(logp, g, prev)
    assert torch.equal(got, want)
    w = torch.randn(5, 7, dtype=torch.float64)
    ga = torch.autograd.grad((got * w).sum(), [logp, prev])
    gb = torch.autograd.grad((want * w).sum(), [logp, prev])
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_public_surface():
    for n in ("DefaultVisionTransformerDiffPruning", "DefaultVisionTransformerTeacher", "default_dynamic_vit_tiny_patch16_224_student",
              "default_dynamic_vit_small_patch16_224_student", "default_dynamic_vit_base_patch16_224_student",
              "default_dynamic_vit_tiny_patch16_224_teacher", "default_dynamic_vit_small_patch16_224_teacher",
              "default_dynamic_vit_base_patch16_224_teacher"):
        assert hasattr(vit_models, n) and hasattr(DV, n), n
    assert hasattr(DV, "PredictorLG")
    case = DC.CASES["stage2"]
    cfg = case["cfg"]
    m = DV.DefaultVisionTransformerDiffPruning(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
                                               num_heads=cfg["heads"], num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
                                               token_ratio=list(cfg["token_ratio"]), distill=True, init_n=cfg["init_n"])
    want = DC.param_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want       # the reference's state-dict keys (the fixture loaded them)
    with pytest.raises(AssertionError):
        DV.DefaultVisionTransformerDiffPruning(embed_dim=128, num_heads=2, depth=1, pruning_loc=[], token_ratio=[], drop_rate=0.1)


def test_library_exports():
    header = open(os.path.join(DC.REPO, "include", "d2s_hip.h")).read()
    for name in ("d2s_attn_policy_bwd_dpol_f32", "d2s_gumbel_noise", "d2s_gumbel_keep_fwd", "d2s_gumbel_keep_bwd", "d2s_policy_pool_fwd",
                 "d2s_policy_pool_bwd"):
        assert name in lib.symbols("d2s_hip.h") and name in header
        assert hasattr(lib.load(), name)


def _loss_inputs(dtype, seed=4, B=4, N=16, D=32, K=10):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    mask = (torch.rand(B, N, generator=gen) > 0.4).to(dtype)
    decisions = [(torch.rand(B, N, generator=gen) > 0.3).to(dtype).requires_grad_(True), mask.clone().requires_grad_(True)]
    return dict(logits_s=r(B, K).requires_grad_(True), feat_s=r(B, N, D).requires_grad_(True), mask=mask, decisions=decisions,
                logits_t=r(B, K), feat_t=r(B, N, D), labels=torch.randint(0, K, (B,), generator=gen),
                soft=torch.softmax(r(B, K), -1), ratios=[0.5, 0.25])


@pytest.mark.parametrize("soft", [False, True])
def test_loss_restatement_against_float64_autograd(soft):
    """The term-by-term restatement equals the objective composed from torch's own losses (cross_entropy, kl_div with batchmean and
    log_target, mse_loss), value and every gradient, in float64."""
    import torch.nn.functional as F
    t = _loss_inputs(torch.float64)
    labels = t["soft"] if soft else t["labels"]
    got = R.loss(t["logits_s"], t["feat_s"], t["mask"], t["decisions"], t["logits_t"], t["feat_t"], labels, t["ratios"])
    ls = F.log_softmax(t["logits_s"], -1)
    cls = F.cross_entropy(t["logits_s"], labels)      # probabilities as the target: the soft-target cross entropy
    ratio = sum(F.mse_loss(d.mean(1), torch.full((d.shape[0],), r, dtype=d.dtype)) for d, r in zip(t["decisions"], t["ratios"])) / 2
    kl = F.kl_div(ls, F.log_softmax(t["logits_t"], -1), reduction="batchmean", log_target=True)
    per_token = F.mse_loss(t["feat_s"], t["feat_t"], reduction="none").mean(-1)
    token = (per_token * t["mask"]).sum() / t["mask"].sum()
    want = 1.0 * cls + 2.0 * ratio + 0.5 * kl + 0.5 * token
    for k, v in (("cls", cls), ("ratio", ratio), ("kl", kl), ("token", token), ("total", want)):
        assert float(got[k]) == pytest.approx(float(v), rel=1e-12, abs=1e-14), k
    leaves = [t["logits_s"], t["feat_s"]] + t["decisions"]
    for a, b in zip(torch.autograd.grad(got["total"], leaves), torch.autograd.grad(want, leaves)):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-11, atol=1e-15)
        assert float(b.abs().max()) > 0


@pytest.mark.parametrize("extra,flag", [(["--topk-selection"], "--topk-selection"), (["--topk-selection", "--diff-topk"], "--diff-topk"),
                                        (["--patch-score-threshold", "0.3"], "--patch-score-threshold"),
                                        (["--small-predictor"], "--small-predictor"), (["--predictor-bn"], "--predictor-bn")])
def test_cli_rejects_d2s_selection_flags_with_dynamicvit(extra, flag):
    import mask_predictor
    import utils
    with pytest.raises(SystemExit) as e:
        mask_predictor.check_supported(utils.parse_args(["--method", "dynamicvit"] + extra))
    assert f"--method dynamicvit with {flag}" in str(e.value)


def test_cli_method_flag():
    import mask_predictor
    import utils
    assert utils.parse_args([]).method == "d2s"
    a = utils.parse_args(["--method", "dynamicvit", "--pruning-locs", "3", "6", "--keep-ratios", "0.7", "0.49", "--drop-path", "0.1"])
    assert a.method == "dynamicvit"
    mask_predictor.check_supported(a)
    mask_predictor.check_supported(utils.parse_args(["--topk-selection"]))      # unchanged for the default method
    with pytest.raises(SystemExit):
        utils.parse_args(["--method", "other"])


def test_loss_class_and_entries_exist():
    import losses
    from d2s.functional_dynamicvit import RatioLossFn  # noqa: F401
    assert hasattr(losses, "DynamicViTLoss")
    header = open(os.path.join(DC.REPO, "include", "d2s_hip.h")).read()
    for name in ("d2s_ratio_rows_fwd", "d2s_ratio_rows_bwd", "d2s_gumbel_from_bits"):
        assert name in lib.symbols("d2s_hip.h") and name in header
