"""The A-ViT baseline (--method avit), the parts that need no GPU: the dense masked restatement of
tests/avit_ref.py against itself (weights, ponder cost, physical deletion, the prior against torch's kl_div, the closed-form gradient of
a halting score against float64 autograd), the condition on the inputs the GPU tests run on, the seventh header and binding table, the
command line, build_models, the constructor, TrainStep's refusals and the checkpoint config."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import avit_ref as R
from oracle import d2s_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_avit_halt", "d2s_avit_halt_bwd", "d2s_avit_penalty_bwd", "d2s_avit_penalty_fwd"]
EPS = 0.01

# The model cases of the GPU tests: the micro geometry (D 128, H 2, depth 4, N 17) with B = 4, gate constants picked on the CPU with the
# restatement so that halting spreads (with the default centre of 30 nothing halts on random weights).
CFG = O.make_cfg(img_size=64, dim=128, depth=4, heads=2, num_classes=10, pruning_loc=(1,), token_ratio=(0.05,))
AVIT_CASES = {
    "avit1": dict(case=dict(cfg=CFG, batch=4, seed=71), gamma=4.0, beta=-0.5),
    "avit2": dict(case=dict(cfg=CFG, batch=4, seed=72), gamma=10.0, beta=0.0),
}
_BUILT = {}


def built(name):
    """(state dict, images, labels, float64 restatement without gradients) of a model case, once"""
    if name not in _BUILT:
        c = AVIT_CASES[name]
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cases.make_weights(c["case"])[1].items()}
        images = torch.from_numpy(cases.make_images(c["case"]))
        labels = torch.from_numpy(cases.make_labels(c["case"])).long()
        with torch.no_grad():
            out = R.forward({k: v.double() for k, v in sd.items()}, images, CFG, c["gamma"], c["beta"], EPS)
        _BUILT[name] = (sd, images, labels, out)
    return _BUILT[name]


def check_condition(out, L):
    """The condition on the inputs (a condition, not a measurement): every live token at every layer is at least 1e-4 away from the
    threshold, the halting layers take at least three values, a CLS token halts before L, an image keeps tokens to L."""
    n = out["n"]
    assert out["margin"] >= 1e-4, out["margin"]
    assert len(torch.unique(n)) >= 3, torch.unique(n)
    assert bool((n[:, 0] < L).any()) and bool((n[:, 0] == L).any()), n[:, 0]


@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_the_model_cases_qualify_and_fp32_agrees_on_the_halting_layers(name):
    sd, images, _, out = built(name)
    c = AVIT_CASES[name]
    check_condition(out, CFG["depth"])
    with torch.no_grad():
        out32 = R.forward(sd, images, CFG, c["gamma"], c["beta"], EPS, dtype=torch.float32)
    assert torch.equal(out32["n"], out["n"])
    print(name, "halting layers of CLS", out["n"][:, 0].tolist(), "margin", out["margin"])


@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_weights_sum_to_one_and_rho_is_n_plus_r(name):
    _, _, _, out = built(name)
    n, Rm = out["n"], out["R"]
    B, N = n.shape
    wsum = torch.zeros((B, N), dtype=torch.float64)
    for l, (h, live) in enumerate(zip(out["h"], out["live"]), start=1):
        wsum += torch.where(n > l, h, torch.zeros_like(h)) * live
    wsum += Rm
    assert torch.allclose(wsum, torch.ones_like(wsum), atol=1e-12)
    assert bool((Rm > 0).all()) and bool((n >= 1).all())
    assert torch.allclose(R.ponder(out), (n.double() + Rm).mean())
    # the CLS token takes its image's live tokens with it: nothing outlives it
    assert bool((n <= n[:, :1]).all())


@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_an_image_alone_with_its_halted_tokens_deleted_gives_the_masked_logits(name):
    sd, images, _, out = built(name)
    c = AVIT_CASES[name]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        for b in range(images.shape[0]):
            logits, n = R.forward_deleted(sd64, images[b:b + 1], CFG, c["gamma"], c["beta"], EPS)
            assert torch.equal(n, out["n"][b])
            assert torch.allclose(logits[0], out["logits"][b], rtol=1e-10, atol=1e-12)


def test_prior_against_torch_kl_div():
    g = torch.Generator().manual_seed(5)
    for L in (4, 12):
        hb = torch.rand(L, generator=g, dtype=torch.float64)
        hb[0] = 1e-4                                    # below the clamp
        tgt = R.target(L, 7.0 if L == 12 else 2.0)
        p = torch.clamp(hb / hb.sum(), 0.01, 0.99)
        want = F.kl_div(p.log(), tgt, reduction="batchmean")
        assert torch.allclose(R.prior(hb, tgt), want, rtol=1e-12)
        hbg = hb.clone().requires_grad_(True)
        (grad,) = torch.autograd.grad(R.prior(hbg, tgt), hbg)
        assert torch.allclose(R.prior_grad_closed_form(hb, tgt), grad, rtol=1e-10, atol=1e-14)
    assert abs(float(R.target(12, 7.0).sum()) - 1.0) < 1e-12


@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_closed_form_gradient_of_the_halting_scores_against_autograd(name):
    sd, images, labels, _ = built(name)
    c = AVIT_CASES[name]
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    out = R.forward(sd64, images, CFG, c["gamma"], c["beta"], EPS)
    ps, pa, td = 5e-2, 0.3, 2.0                         # larger than the defaults so that every term is visible
    loss, _ = R.objective(out, labels, ponder_scale=ps, prior_alpha=pa, target_depth=td)
    grads = torch.autograd.grad(loss, [out["acc"]] + out["h"])
    dacc, gh = grads[0], grads[1:]
    closed = R.gh_closed_form(out, dacc, ps, pa, td)
    for l, (a, b, live) in enumerate(zip(gh, closed, out["live"]), start=1):
        assert torch.allclose(a * live, b, rtol=1e-9, atol=1e-14), l
        assert float((a * ~live).abs().max()) == 0.0 or not bool((~live).any())


# ---- header and binding ----
def test_avit_header_and_binding_tables():
    from d2s import lib, ops, functional_avit
    text = open(os.path.join(REPO, "include", "d2s_hip_avit.h")).read()
    assert NEW == lib.symbols("d2s_hip_avit.h") and "D2S_ERR_ARG" in text
    assert all(lib.signature(name)[0] is lib.I and lib.signature(name)[1] for name in NEW)
    for fn in ("avit_state", "avit_halt", "avit_halt_bwd", "avit_penalty_fwd", "avit_penalty_bwd"):
        assert callable(getattr(ops, fn))
    assert callable(functional_avit.AViTHaltFn.apply) and callable(functional_avit.AViTPenaltyFn.apply)
    t = functional_avit.target_distribution(12, 7.0)
    assert torch.allclose(t.double(), R.target(12, 7.0), atol=1e-8)


# ---- command line ----
AVIT = ["--method", "avit"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_avit_and_fills_the_defaults():
    import utils
    assert utils.parse_args([]).avit_gate_scale is None
    for mode in ("exact", "split"):
        a = _check(AVIT + ["--student-checkpoint", "w.pt", "--gemm-mode", mode])
        assert a.method == "avit" and a.warmup_steps == 0
        assert (a.avit_gate_scale, a.avit_gate_center, a.avit_ponder_scale, a.avit_prior_alpha, a.avit_target_depth) == (10.0, 30.0, 5e-4, 0.01, 7.0)
    a = _check(AVIT + ["--avit-gate-scale", "4", "--avit-gate-center", "-0.5", "--avit-ponder-scale", "0.001", "--avit-prior-alpha", "0.1",
                       "--avit-target-depth", "5", "--dist-weight", "0", "--warmup-steps", "0"])
    assert (a.avit_gate_scale, a.avit_gate_center, a.avit_ponder_scale, a.avit_prior_alpha, a.avit_target_depth) == (4.0, -0.5, 0.001, 0.1, 5.0)
    for mode in ("exact", "split", "bf16"):                                          # inference runs in all three modes
        assert _check(AVIT + ["--eval-only", "--student-checkpoint", "w.pt", "--gemm-mode", mode]).eval_only
    assert _check(["--warmup-steps", "5"]).warmup_steps == 5                         # the other methods keep their warm-up
    d = _check([])
    assert d.avit_gate_scale is None and d.avit_target_depth is None                 # ... and are not handed the defaults


@pytest.mark.parametrize("argv,fragment", [
    (AVIT + ["--topk-selection"], "--method avit with --topk-selection"),
    (AVIT + ["--topk-selection", "--attn-selection"], "--method avit with --attn-selection"),
    (AVIT + ["--topk-selection", "--fuse-dropped"], "--method avit with --fuse-dropped"),
    (AVIT + ["--topk-selection", "--squeeze-dropped"], "--method avit with --squeeze-dropped"),
    (AVIT + ["--topk-selection", "--diff-topk"], "--method avit with --diff-topk"),
    (AVIT + ["--patch-score-threshold", "0.4"], "--method avit with --patch-score-threshold"),
    (AVIT + ["--gemm-mode", "bf16"], "--method avit with --gemm-mode bf16"),
    (AVIT + ["--drop-path", "0.1"], "--method avit with --drop-path 0.1"),
    (AVIT + ["--torch-optim"], "--method avit with --torch-optim"),
    (AVIT + ["--warmup-steps", "3"], "--method avit with --warmup-steps 3"),
    (["--avit-gate-scale", "4"], "--avit-gate-scale with --method d2s"),
    (["--avit-gate-center", "1"], "--avit-gate-center with --method d2s"),
    (["--method", "dynamicvit", "--avit-ponder-scale", "0.1"], "--avit-ponder-scale with --method dynamicvit"),
    (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--avit-prior-alpha", "0.1"], "--avit-prior-alpha with --method tome"),
    (["--method", "ats", "--eval-only", "--student-checkpoint", "w.pt", "--avit-target-depth", "5"], "--avit-target-depth with --method ats"),
    # the older flags' generic refusals cover the new method
    (AVIT + ["--tome-r", "2"], "--tome-r 2 with --method avit"),
    (AVIT + ["--ats-tokens", "8"], "--ats-tokens with --method avit"),
    (AVIT + ["--ragged-train", "--patch-score-threshold", "0.4"], "--ragged-train with --method avit"),
    (AVIT + ["--tome-train"], "--tome-train with --method avit"),
    (AVIT + ["--ats-train"], "--ats-train with --method avit"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_the_method_was_refused_by_argparse_before_and_the_others_stay():
    import utils
    for m in ("d2s", "dynamicvit", "tome", "ats", "avit"):
        assert utils.parse_args(["--method", m]).method == m
    with pytest.raises(SystemExit):
        utils.parse_args(["--method", "nosuch"])


def test_build_models_builds_the_teacher_unless_dist_weight_is_zero(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(checkpoint_path=None, **kw):
        seen["kw"] = kw
        return vit_models.VisionTransformerAViT(**MICRO, **kw)

    def teacher_factory(checkpoint_path=None):
        seen["teacher_checkpoint"] = checkpoint_path
        return vit_models.VisionTransformerTeacher(**MICRO)
    monkeypatch.setattr(vit_models, "avit_deit_tiny_patch16_224", factory)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_teacher", teacher_factory)
    base = dict(arch="deit_tiny", method="avit", student_checkpoint=None, resume=None, teacher_checkpoint=None, device=torch.device("cpu"))
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.5, avit_gate_scale=4.0, avit_gate_center=-0.5,
                                                                         avit_target_depth=5.0))
    assert isinstance(student, vit_models.VisionTransformerAViT) and isinstance(teacher, vit_models.VisionTransformerTeacher)
    assert seen["kw"] == dict(gate_scale=4.0, gate_center=-0.5, target_depth=5.0)
    assert (student.gate_scale, student.gate_center, student.eps_halt, student.target_depth) == (4.0, -0.5, 0.01, 5.0)
    seen.pop("teacher_checkpoint")
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.0))
    assert teacher is None and "teacher_checkpoint" not in seen                      # --dist-weight 0: no teacher is built
    assert (student.gate_scale, student.gate_center, student.target_depth) == (10.0, 30.0, 7.0)
    assert "the trunk starts from its random initialisation" in capsys.readouterr().out


# ---- constructor, TrainStep ----
def test_constructor_and_state_dict_keys():
    import vit_models
    m = vit_models.VisionTransformerAViT(**MICRO)
    assert (m.gate_scale, m.gate_center, m.eps_halt, m.target_depth) == (10.0, 30.0, 0.01, 7.0) and m.grad_ready_hook is None
    assert list(m.state_dict()) == list(vit_models.VisionTransformerTeacher(**MICRO).state_dict())      # no new parameter, no buffer
    m = vit_models.VisionTransformerAViT(**MICRO, gate_scale=4, gate_center=-0.5, eps_halt=0.05)
    assert (m.gate_scale, m.gate_center, m.eps_halt) == (4.0, -0.5, 0.05)
    assert vit_models.avit_deit_tiny_patch16_224(gate_center=3.0).gate_center == 3.0
    assert len(vit_models.avit_deit_small_patch16_224().blocks) == 12 and vit_models.avit_deit_small_patch16_224().embed_dim == 384
    with pytest.raises(ValueError, match="drop_path_rate"):
        vit_models.VisionTransformerAViT(**MICRO, drop_path_rate=0.1)
    with pytest.raises(ValueError, match="eps_halt"):
        vit_models.VisionTransformerAViT(**MICRO, eps_halt=1.5)


def test_train_step_refusals_come_before_the_device():
    import vit_models
    from d2s import lib
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    m = vit_models.VisionTransformerAViT(**MICRO)
    with pytest.raises(lib.D2SError, match="graph=True.*A-ViT"):
        TrainStep(m, None, args, graph=True)
    with pytest.raises(ValueError, match="warmup_steps 1 with an A-ViT student"):
        TrainStep(m, None, args, warmup_steps=1)
    dp = vit_models.VisionTransformerAViT(**MICRO)
    dp.drop_path_rate = 0.1                                                       # the constructor refuses it; a model altered afterwards
    with pytest.raises(lib.D2SError, match="A-ViT student and drop_path_rate > 0"):
        TrainStep(dp, None, args)
    with pytest.raises(lib.D2SError) as e:                                        # the message the other students reach is what it was
        TrainStep(vit_models.VisionTransformerTeacher(**MICRO), None, args)
    assert str(e.value) == "TrainStep without a teacher: only a Token Merging student trains without one"


def test_loss_defaults_and_metric_keys():
    from losses import AViTLoss
    fn = AViTLoss(types.SimpleNamespace(mixup=0.0))
    assert (fn.ponder_scale, fn.prior_alpha, fn.cls_weight, fn.dist_weight) == (5e-4, 0.01, 1.0, 0.5)
    fn = AViTLoss(types.SimpleNamespace(mixup=0.0, avit_ponder_scale=0.1, avit_prior_alpha=0.2, dist_weight=0.0))
    assert (fn.ponder_scale, fn.prior_alpha, fn.dist_weight) == (0.1, 0.2, 0.0)
    metrics = {}
    one = torch.ones(())
    fn.accumulate(metrics, (one, one, one), (2 * one, 3 * one, 4 * one))
    assert sorted(metrics) == ["train_avg_depth", "train_avit_loss", "train_cls_kl_loss", "train_cls_loss", "train_ponder_loss", "train_prior_loss"]
    assert (float(metrics["train_ponder_loss"]), float(metrics["train_prior_loss"]), float(metrics["train_avg_depth"])) == (2.0, 3.0, 4.0)


# ---- checkpoints ----
def test_checkpoint_config_records_the_class_and_the_gate():
    import vit_models
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    a = cfg(vit_models.VisionTransformerAViT(**MICRO, gate_scale=4.0, gate_center=-0.5))
    b = cfg(vit_models.VisionTransformerAViT(**MICRO))
    c = cfg(vit_models.VisionTransformerTeacher(**MICRO))
    assert a["model"] == "VisionTransformerAViT" and (a["avit_gate_scale"], a["avit_gate_center"], a["avit_eps_halt"]) == (4.0, -0.5, 0.01)
    assert {k for k in a if a[k] != b[k]} == {"avit_gate_scale", "avit_gate_center"}
    assert (c["avit_gate_scale"], c["avit_gate_center"], c["avit_eps_halt"]) == (None, None, None)
    assert {k for k in a if a[k] != c[k]} == {"model", "avit_gate_scale", "avit_gate_center", "avit_eps_halt"}
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in c.items() if not k.startswith("avit_")}
    filled = engine.checkpoint_config(old)
    assert filled == c and "avit_gate_scale" not in old                           # a checkpoint written before: no such student
    assert engine.checkpoint_config(a) == a
