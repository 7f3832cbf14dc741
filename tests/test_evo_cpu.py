"""The Evo-ViT baseline (--method evo), the parts that need no GPU: the closed-form backwards of the float64
restatement in tests/evo_ref.py against autograd, the condition on the inputs the GPU tests run on, the eighth header and binding table,
the command line, build_models, the constructor, TrainStep's refusals and the checkpoint config."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import evo_ref as R
from oracle import d2s_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_evo_gather_bwd", "d2s_evo_scatter_bwd", "d2s_evo_scatter_fwd", "d2s_evo_select"]

# The model cases of the GPU tests: the micro geometry of tests/test_avit_gpu.py (D 128, H 2, depth 4, T 16) with B = 4; one case on an 80
# pixel image (T 25) with keep 0.3 and every block slow-fast but the first, one with evo_start = depth (the dense trunk).  The seeds were
# picked on the CPU with the restatement alone so that check_condition holds.  On random weights the attention is close to uniform, so a
# kept token's score rises from about 1 / (T + 1) to about 1 / (k + 2) and the lists stay as they are; evo2 keeps all tokens but one,
# where the two are equal and the dropped token does change from block to block.
CFG = O.make_cfg(img_size=64, dim=128, depth=4, heads=2, num_classes=10, pruning_loc=(1,), token_ratio=(0.05,))
CFG80 = O.make_cfg(img_size=80, dim=128, depth=4, heads=2, num_classes=10, pruning_loc=(1,), token_ratio=(0.05,))
EVO_CASES = {
    "evo1": dict(case=dict(cfg=CFG, batch=4, seed=90), start=2, keep=0.5, tau=0.5),
    "evo2": dict(case=dict(cfg=CFG, batch=4, seed=94), start=1, keep=0.95, tau=0.9),      # k = T - 1: the one dropped token changes
    "evo80": dict(case=dict(cfg=CFG80, batch=4, seed=83), start=1, keep=0.3, tau=0.5),
    "evodense": dict(case=dict(cfg=CFG, batch=4, seed=85), start=4, keep=0.5, tau=0.5),
}
_BUILT = {}


def built(name):
    """(state dict, images, labels, float64 restatement without gradients) of a model case, once"""
    if name not in _BUILT:
        c = EVO_CASES[name]
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cases.make_weights(c["case"])[1].items()}
        images = torch.from_numpy(cases.make_images(c["case"]))
        labels = torch.from_numpy(cases.make_labels(c["case"])).long()
        with torch.no_grad():
            out = R.forward({k: v.double() for k, v in sd.items()}, images, c["case"]["cfg"], c["start"], c["keep"], c["tau"])
        _BUILT[name] = (sd, images, labels, out)
    return _BUILT[name]


def check_condition(out):
    """The condition on the inputs (a condition, not a measurement): at every selection the k-th and the (k+1)-th value of g are more than
    1e-4 apart in every image, so 'the same selection as float64' is a fair demand of the fp32 arithmetic modes."""
    assert out["gaps"] and min(out["gaps"]) > 1e-4, out["gaps"]


@pytest.mark.parametrize("name", sorted(EVO_CASES))
def test_the_model_cases_qualify_and_fp32_agrees_on_the_selection(name):
    sd, images, _, out = built(name)
    c = EVO_CASES[name]
    check_condition(out)
    L = c["case"]["cfg"]["depth"]
    assert len(out["kept"]) == L - c["start"] and len(out["gaps"]) == max(1, L - c["start"])
    with torch.no_grad():
        out32 = R.forward(sd, images, c["case"]["cfg"], c["start"], c["keep"], c["tau"], dtype=torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(out32["kept"], out["kept"]))
    if name == "evo2":                              # the re-selection moves: a token that was dropped comes back
        assert any(not torch.equal(a, b) for a, b in zip(out["kept"], out["kept"][1:]))
    print(name, "gaps", [f"{v:.2e}" for v in out["gaps"]])


def test_selection_rule_ties_and_order():
    g = torch.tensor([[0.5, 0.2, 0.5, 0.1, 0.5, 0.2], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    kept, dropped = R.topk_rule(g, 2)
    assert kept.tolist() == [[0, 2], [0, 1]] and dropped.tolist() == [[1, 3, 4, 5], [2, 3, 4, 5]]
    kept, dropped = R.topk_rule(g, 4)
    assert kept.tolist() == [[0, 1, 2, 4], [0, 1, 2, 3]] and dropped.tolist() == [[3, 5], [4, 5]]
    a = torch.rand(2, 3, 4, dtype=torch.float64)             # the evolution touches the kept entries only
    g2, _, _ = R.select(g, torch.tensor([[0, 2], [0, 1]]), a, 0.25, 2)
    assert torch.equal(g2[:, 3:], g[:, 3:]) and float(g2[0, 1]) == 0.2
    assert torch.allclose(g2[0, 2], 0.75 * g[0, 2] + 0.25 * a[0, :, 2].mean())


@pytest.mark.parametrize("B,T,k,D", [(2, 9, 4, 8), (1, 2, 1, 4), (3, 7, 6, 12)])
def test_closed_form_backwards_against_autograd(B, T, k, D):
    """One slow-fast block composed from the differentiable restatement with a smooth stand-in for the block; the gradient of X by autograd
    against scatter_bwd -> the stand-in's backward -> gather_bwd."""
    gen = torch.Generator().manual_seed(100 * T + k)
    X = torch.randn(B, 1 + T, D, generator=gen, dtype=torch.float64, requires_grad=True)
    W = torch.randn(D, D, generator=gen, dtype=torch.float64) / D ** 0.5
    g = torch.rand(B, T, generator=gen, dtype=torch.float64)
    up = torch.randn(B, 1 + T, D, generator=gen, dtype=torch.float64)
    kept, dropped = R.topk_rule(g, k)
    xc = R.gather(X, g, kept, dropped)
    yc = torch.tanh(xc @ W) + xc.mean(dim=1, keepdim=True)          # rows mix, as in attention
    Xn = R.scatter_fwd(X, yc, xc, kept, dropped)
    (auto,) = torch.autograd.grad((Xn * up).sum(), X, retain_graph=True)
    dyc = R.scatter_bwd(up, kept, dropped)
    (dyc_auto,) = torch.autograd.grad((R.scatter_fwd(X.detach(), yc, xc.detach(), kept, dropped) * up).sum(), yc, retain_graph=True)
    assert torch.allclose(dyc, dyc_auto, rtol=1e-9, atol=1e-13)
    (dxc,) = torch.autograd.grad(yc, xc, dyc, retain_graph=True)    # the block's own backward: without the direct -delta term on r
    _, S = R.weights(g, dropped)
    closed = R.gather_bwd(up, dxc, dyc[:, k + 1], g, S, kept, dropped)
    assert torch.allclose(closed, auto, rtol=1e-9, atol=1e-13)
    bound = R.gather_bwd_bound(up, dxc, dyc[:, k + 1], g, S, dropped)
    assert bound.shape == (B, T - k, D) and bool((bound > 0).all())


# ---- header and binding ----
def test_evo_header_and_binding_tables():
    from d2s import lib, ops, functional_evo
    text = open(os.path.join(REPO, "include", "d2s_hip_evo.h")).read()
    assert NEW == lib.symbols("d2s_hip_evo.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert all(lib.signature(name)[0] is lib.I and lib.signature(name)[1] for name in NEW)
    for fn in ("evo_select", "evo_scatter_fwd", "evo_scatter_bwd", "evo_gather_bwd"):
        assert callable(getattr(ops, fn))
    assert callable(functional_evo.EvoGatherFn.apply) and callable(functional_evo.EvoScatterFn.apply)
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "evo.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "hipMemset" not in src
    assert "evo (26)" in open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "Makefile")).read()


# ---- command line ----
EVO = ["--method", "evo"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_evo_and_fills_the_defaults():
    import utils
    p = utils.parse_args([])
    assert p.evo_start is None and p.evo_keep is None and p.evo_tradeoff is None
    for mode in ("exact", "split", "bf16"):                                          # training runs in all three modes
        a = _check(EVO + ["--student-checkpoint", "w.pt", "--gemm-mode", mode])
        assert a.method == "evo" and a.warmup_steps == 0
        assert (a.evo_start, a.evo_keep, a.evo_tradeoff) == (4, 0.5, 0.5)
    a = _check(EVO + ["--evo-start", "12", "--evo-keep", "0.25", "--evo-tradeoff", "0.9", "--dist-weight", "0", "--warmup-steps", "0"])
    assert (a.evo_start, a.evo_keep, a.evo_tradeoff) == (12, 0.25, 0.9)
    assert _check(EVO + ["--eval-only", "--student-checkpoint", "w.pt"]).eval_only
    assert _check(["--warmup-steps", "5"]).warmup_steps == 5                         # the other methods keep their warm-up
    d = _check([])
    assert d.evo_start is None and d.evo_keep is None and d.evo_tradeoff is None     # ... and are not handed the defaults


@pytest.mark.parametrize("argv,fragment", [
    (EVO + ["--topk-selection"], "--method evo with --topk-selection"),
    (EVO + ["--topk-selection", "--attn-selection"], "--method evo with --attn-selection"),
    (EVO + ["--topk-selection", "--fuse-dropped"], "--method evo with --fuse-dropped"),
    (EVO + ["--topk-selection", "--squeeze-dropped"], "--method evo with --squeeze-dropped"),
    (EVO + ["--topk-selection", "--diff-topk"], "--method evo with --diff-topk"),
    (EVO + ["--patch-score-threshold", "0.4"], "--method evo with --patch-score-threshold"),
    (EVO + ["--drop-path", "0.1"], "--method evo with --drop-path 0.1"),
    (EVO + ["--torch-optim"], "--method evo with --torch-optim"),
    (EVO + ["--warmup-steps", "3"], "--method evo with --warmup-steps 3"),
    (EVO + ["--evo-start", "0"], "--evo-start 0 (a block in 1..12"),
    (EVO + ["--evo-start", "13"], "--evo-start 13 (a block in 1..12"),
    (EVO + ["--evo-keep", "0.001"], "--evo-keep 0.001 (k = int(196 * keep) must lie in 1..195)"),
    (EVO + ["--evo-keep", "1.0"], "--evo-keep 1.0 (k = int(196 * keep) must lie in 1..195)"),
    (["--evo-start", "4"], "--evo-start with --method d2s"),
    (["--method", "dynamicvit", "--evo-keep", "0.5"], "--evo-keep with --method dynamicvit"),
    (["--method", "avit", "--evo-tradeoff", "0.5"], "--evo-tradeoff with --method avit"),
    (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--evo-keep", "0.5"], "--evo-keep with --method tome"),
    # the older flags' generic refusals cover the new method
    (EVO + ["--tome-r", "2"], "--tome-r 2 with --method evo"),
    (EVO + ["--ats-tokens", "8"], "--ats-tokens with --method evo"),
    (EVO + ["--avit-gate-scale", "4"], "--avit-gate-scale with --method evo"),
    (EVO + ["--ragged-train", "--patch-score-threshold", "0.4"], "--ragged-train with --method evo"),
    (EVO + ["--tome-train"], "--tome-train with --method evo"),
    (EVO + ["--ats-train"], "--ats-train with --method evo"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_the_method_parses_and_an_unknown_one_does_not():
    import utils
    for m in ("d2s", "dynamicvit", "tome", "ats", "avit", "evo"):
        assert utils.parse_args(["--method", m]).method == m
    with pytest.raises(SystemExit):
        utils.parse_args(["--method", "nosuch"])


def test_build_models_builds_the_teacher_unless_dist_weight_is_zero(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(checkpoint_path=None, **kw):
        seen["kw"] = kw
        return vit_models.VisionTransformerEvo(**MICRO, **kw)

    def teacher_factory(checkpoint_path=None):
        seen["teacher_checkpoint"] = checkpoint_path
        return vit_models.VisionTransformerTeacher(**MICRO)
    monkeypatch.setattr(vit_models, "evo_deit_tiny_patch16_224", factory)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_teacher", teacher_factory)
    base = dict(arch="deit_tiny", method="evo", student_checkpoint=None, resume=None, teacher_checkpoint=None, device=torch.device("cpu"))
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.5, evo_start=2, evo_keep=0.25, evo_tradeoff=0.9))
    assert isinstance(student, vit_models.VisionTransformerEvo) and isinstance(teacher, vit_models.VisionTransformerTeacher)
    assert seen["kw"] == dict(evo_start=2, evo_keep=0.25, evo_tradeoff=0.9)
    assert (student.evo_start, student.evo_keep, student.evo_tradeoff, student.evo_k) == (2, 0.25, 0.9, 4)
    seen.pop("teacher_checkpoint")
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.0))
    assert teacher is None and "teacher_checkpoint" not in seen                      # --dist-weight 0: no teacher is built
    assert (student.evo_start, student.evo_keep, student.evo_tradeoff) == (4, 0.5, 0.5)
    assert "the trunk starts from its random initialisation" in capsys.readouterr().out


# ---- constructor, TrainStep ----
def test_constructor_and_state_dict_keys():
    import vit_models
    m = vit_models.VisionTransformerEvo(**MICRO)
    assert (m.evo_start, m.evo_keep, m.evo_tradeoff, m.evo_k) == (4, 0.5, 0.5, 8) and m.grad_ready_hook is None
    assert list(m.state_dict()) == list(vit_models.VisionTransformerTeacher(**MICRO).state_dict())      # no new parameter, no buffer
    m.load_state_dict(vit_models.VisionTransformerTeacher(**MICRO).state_dict(), strict=True)
    assert vit_models.evo_deit_tiny_patch16_224(evo_keep=0.7).evo_k == 137
    small = vit_models.evo_deit_small_patch16_224()
    assert len(small.blocks) == 12 and small.embed_dim == 384 and (small.evo_start, small.evo_k) == (4, 98)
    assert vit_models.evo_deit_base_patch16_224(evo_start=12).embed_dim == 768
    with pytest.raises(ValueError, match="drop_path_rate"):
        vit_models.VisionTransformerEvo(**MICRO, drop_path_rate=0.1)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="evo_start"):
            vit_models.VisionTransformerEvo(**MICRO, evo_start=bad)
    for bad in (0.01, 1.0):                                                       # k = 0 and k = T
        with pytest.raises(ValueError, match="evo_keep"):
            vit_models.VisionTransformerEvo(**MICRO, evo_keep=bad)
    assert vit_models.VisionTransformerEvo(**MICRO, evo_keep=0.99).evo_k == 15     # k = T - 1 is the last legal one


def test_train_step_refusals_come_before_the_device():
    import vit_models
    from d2s import lib
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    m = vit_models.VisionTransformerEvo(**MICRO)
    with pytest.raises(ValueError, match="warmup_steps 1 with an Evo-ViT student"):
        TrainStep(m, None, args, warmup_steps=1)
    dp = vit_models.VisionTransformerEvo(**MICRO)
    dp.drop_path_rate = 0.1                                                       # the constructor refuses it; a model altered afterwards
    with pytest.raises(lib.D2SError, match="Evo-ViT student and drop_path_rate > 0"):
        TrainStep(dp, None, args)


# ---- checkpoints ----
def test_checkpoint_config_round_trip_with_the_new_keys():
    import vit_models
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    a = cfg(vit_models.VisionTransformerEvo(**MICRO, evo_start=2, evo_keep=0.25, evo_tradeoff=0.9))
    b = cfg(vit_models.VisionTransformerEvo(**MICRO))
    c = cfg(vit_models.VisionTransformerTeacher(**MICRO))
    assert a["model"] == "VisionTransformerEvo" and (a["evo_start"], a["evo_keep"], a["evo_tradeoff"]) == (2, 0.25, 0.9)
    assert {k for k in a if a[k] != b[k]} == {"evo_start", "evo_keep", "evo_tradeoff"}
    assert (c["evo_start"], c["evo_keep"], c["evo_tradeoff"]) == (None, None, None)
    assert {k for k in a if a[k] != c[k]} == {"model", "evo_start", "evo_keep", "evo_tradeoff"}
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in c.items() if not k.startswith("evo_")}
    filled = engine.checkpoint_config(old)
    assert filled == c and "evo_start" not in old                                 # a checkpoint written before: no such student
    assert engine.checkpoint_config(a) == a
