"""Training the dynamic keep ratio on the ragged packed batch (--patch-score-threshold --ragged-train), the parts
that need no GPU: the float64 restatement (tests/ragged_train_ref.py) against the inference cascade's restatement, its two loss terms
against torch.nn.functional, its one-stage loss against the policy-mode oracle, the selection gaps of the cases the GPU tier trains on,
the sixth header and binding table, the command line, build_models, the constructor and TrainStep's refusals, the checkpoint config."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import ragged_cascade_ref as C
from tests import ragged_train_ref as R
from oracle import d2s_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_half_mean_concat_varlen_bwd", "d2s_ragged_mask_loss_bwd", "d2s_ragged_mask_loss_fwd", "d2s_ragged_teacher_rows"]
# smallest |running sum - threshold| of the fp32 restatement per stage, recorded from test_selection_gaps_of_the_cases' printout
RECORDED_GAPS = {
    "micro_thr1": [1.693e-02],
    "micro_thr2": [2.030e-03, 1.745e-02],
    "micro_thr3s": [4.661e-03, 2.568e-03, 1.291e-02],
}


# ---- the restatement ----
@pytest.mark.parametrize("name", ["micro_thr2", "micro_thr3s"])
def test_reference_forward_is_the_inference_cascade(name):
    """the training definition IS the inference cascade: same logits, same normed rows, same masks, same scores (fp32 against fp32)"""
    case, sd, _, x, _ = R.case_tensors(name)
    cfg = case["cfg"]
    with torch.no_grad():
        out = R.train_forward(sd, x, cfg, case["threshold"], dtype=torch.float32)
    logits, feats, stages = C.reference(name)
    torch.testing.assert_close(out["logits"], logits, rtol=1e-6, atol=1e-6)
    for a, b in zip(out["feats"], feats):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    for got, want in zip(out["masks"], C.dense_masks(stages, cfg["n_patches"])):
        assert torch.equal(got, want)
    for s in range(1, len(stages)):
        for b, (T, ids, sc) in enumerate(stages[s]):
            assert out["ids_in"][s][b].numel() == T and torch.equal(out["ids"][s][b], ids)
            torch.testing.assert_close(out["pred_logits"][s][b], sc, rtol=1e-6, atol=1e-6)
    # replaying its own masks changes nothing; float64 selects the same tokens
    with torch.no_grad():
        again = R.train_forward(sd, x, cfg, case["threshold"], masks=out["masks"], dtype=torch.float32)
        f64 = R.train_forward(sd, x, cfg, case["threshold"])
    assert torch.equal(again["logits"], out["logits"])
    assert all(torch.equal(a, b) for a, b in zip(f64["masks"], out["masks"]))


@pytest.mark.parametrize("name", sorted(RECORDED_GAPS))
def test_selection_gaps_of_the_cases(name):
    """The GPU tier asserts mask equality with the fp32 restatement only where no running sum comes closer to the threshold than section
    14's margin, 2e-5; these are the gaps of the cases it uses."""
    case, sd, _, x, _ = R.case_tensors(name)
    with torch.no_grad():
        out = R.train_forward(sd, x, case["cfg"], case["threshold"], dtype=torch.float32)
    print(f"{name}: threshold {case['threshold']}, gaps per stage {['%.3e' % g for g in out['gaps']]}, "
          f"kept per stage {[[int(i.numel()) for i in per] for per in out['ids']]}")
    assert all(g >= R.SELECTION_MARGIN for g in out["gaps"]), out["gaps"]
    for g, rec in zip(out["gaps"], RECORDED_GAPS[name]):
        assert rec is not None and abs(g - rec) <= 0.05 * rec, (g, rec)
    counts = [int(i.numel()) for i in out["ids"][-1]]
    if name != "micro_thr1":
        assert len(set(counts)) > 1 or any(len(set(int(i.numel()) for i in per)) > 1 for per in out["ids"]), "the case should be ragged"


@pytest.mark.parametrize("kind", ["kl_div", "mse"])
def test_packed_mask_term_against_torch_functional(kind):
    g = torch.Generator().manual_seed(3)
    B, N = 4, 12
    target = torch.rand((B, N), generator=g, dtype=torch.float64)
    target[1, 3] = 0.0                                                        # a zero target entry among the survivors
    target = target / target.sum(dim=1, keepdim=True)
    ids_in = [torch.tensor([0, 2, 5, 7, 11]), torch.tensor([3, 4, 9]), torch.zeros(0, dtype=torch.long), torch.tensor([6])]
    scores = [torch.randn(i.numel(), generator=g, dtype=torch.float64) for i in ids_in]
    got = R.packed_mask_term(scores, ids_in, target, kind)
    want, rows = 0.0, 0
    for b in range(B):
        if ids_in[b].numel() == 0:
            continue
        q = target[b, ids_in[b]] / target[b, ids_in[b]].sum()
        if kind == "mse":
            want = want + F.mse_loss(scores[b], q, reduction="sum")
            rows += ids_in[b].numel()
        else:
            want = want + F.kl_div(F.log_softmax(scores[b], dim=-1), q, reduction="sum")      # zero targets contribute nothing
    want = 100.0 * want / rows if kind == "mse" else want / B
    assert float(got) == pytest.approx(float(want), rel=1e-12)
    # one row: softmax of one score is 1 and q is 1 - the KL is 0; an empty image contributes nothing
    if kind == "kl_div":
        assert float(R.packed_mask_term([scores[3]], [ids_in[3]], target[3:4], kind)) == pytest.approx(0.0, abs=1e-15)
    assert float(R.packed_mask_term([scores[2]], [ids_in[2]], target[2:3], kind)) == 0.0


def test_token_distill_term_against_torch_functional():
    g = torch.Generator().manual_seed(4)
    D, N = 8, 6
    token_t = torch.randn((2, N, D), generator=g, dtype=torch.float64)
    ids = [torch.tensor([1, 4, 5]), torch.tensor([0])]
    feats = [torch.randn((i.numel() + 1, D), generator=g, dtype=torch.float64) for i in ids]
    got = R.token_distill_term(feats, ids, token_t)
    s = torch.cat([f[1:] for f in feats])
    t = torch.cat([token_t[b, i] for b, i in enumerate(ids)])
    want = F.kl_div(F.log_softmax(s, dim=-1), F.log_softmax(t, dim=-1), reduction="batchmean", log_target=True)
    assert float(got) == pytest.approx(float(want), rel=1e-12)


def test_one_stage_loss_is_the_policy_mode_loss_up_to_the_eps_terms():
    """One stage: the ragged definition and the policy-mode training forward keep the same tokens; policy attention adds eps / n to every
    numerator and eps to every denominator (softmax_with_policy, eps = 1e-6), so a dropped key keeps a weight of order eps and every
    kept row moves by O(eps) per block.  Bound: 100 eps = 1e-4 relative on logits and losses (a handful of blocks, O(1) gains each)."""
    case, sd, sd_t, x, y = R.case_tensors("micro_thr1")
    cfg, thr = case["cfg"], case["threshold"]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        out = R.train_forward(sd64, x, cfg, thr)
        teacher_out = O.teacher_forward({k: v.double() for k, v in sd_t.items()}, x.double(), cfg)
        mask_loss, backbone_loss, terms = R.losses(out, teacher_out, y, cfg)
        logits, feats, pred_logits, masks = O.student_forward_threshold_train(sd64, x.double(), cfg, thr)
        want_mask, _ = O.mask_loss_threshold(pred_logits, teacher_out[2], masks, thr)
        want_bb, *want_terms = O.backbone_loss_threshold(logits, feats, teacher_out[0], teacher_out[1], masks, y)
    assert torch.equal(masks[0].float(), out["masks"][0])
    # the blocks before the stage are plain dense blocks here and all-ones-policy blocks there: the scores already differ by O(eps)
    torch.testing.assert_close(out["pred_logits"][0], pred_logits[0], rtol=1e-4, atol=1e-4 * float(pred_logits[0].abs().max()))
    diff = float((out["logits"] - logits).abs().max() / logits.abs().max())
    print(f"one stage, ragged vs policy mode: logits rel {diff:.3e}, mask loss {float(mask_loss):.9f} vs {float(want_mask):.9f}, "
          f"backbone {float(backbone_loss):.9f} vs {float(want_bb):.9f}, token kl {float(terms[2]):.9f} vs {float(want_terms[2]):.9f}")
    assert diff <= 1e-4
    assert float(mask_loss) == pytest.approx(float(want_mask), rel=1e-4)
    assert float(backbone_loss) == pytest.approx(float(want_bb), rel=1e-4)
    assert float(terms[2]) == pytest.approx(float(want_terms[2]), rel=1e-4)


def test_warmup_mask_loss_reaches_every_predictor_of_the_reference():
    _, _, grads, _ = R.model_grads("micro_thr3s", warmup=True)
    for k, g in grads.items():
        if "score_predictor" in k:
            assert g is not None and float(g.abs().max()) > 0, k


# ---- header and binding ----
def test_ragged_threshold_header_and_binding_tables():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ragged_threshold.h")).read()
    assert NEW == lib.symbols("d2s_hip_ragged_threshold.h") and "D2S_ERR_ARG" in text
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "ragged_threshold.hip")).read()
    for name in NEW:
        assert len(re.findall(rf"^int {name}\(", src, flags=re.M)) == 1, name
    assert "atomic" not in src.lower().replace("no atomics", "")
    for fn in ("half_mean_concat_varlen_bwd", "ragged_mask_loss_fwd", "ragged_mask_loss_bwd", "ragged_teacher_rows"):
        assert callable(getattr(ops, fn))
    from d2s import functional_ragged as RF
    for fn in ("RaggedPackFn", "RaggedRepackFn", "RaggedPredictorFn", "RaggedMaskLossFn"):
        assert callable(getattr(RF, fn).apply)
    assert callable(RF.ragged_head) and callable(RF.ragged_predictor_forward)
    # one pattern target prints every file's resource report; ragged_threshold.hip is a source it serves
    assert re.search(r"^resources-%: %\.hip$", open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "Makefile")).read(), flags=re.M)
    assert os.path.exists(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "ragged_threshold.hip"))


def test_library_resolves_the_new_entries():
    from d2s import lib
    loaded = lib.load()
    for name in NEW:
        assert hasattr(loaded, name) and callable(lib._fn(name))


# ---- command line ----
THR = ["--topk-selection", "--patch-score-threshold", "0.4"]
TRAIN = THR + ["--ragged-train"]
THREE = ["--pruning-locs", "3", "6", "9", "--keep-ratios", "0.7", "0.5", "0.3"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_ragged_train(capsys):
    import utils
    assert utils.parse_args([]).ragged_train is False
    for mode in ("exact", "split"):
        a = _check(TRAIN + ["--gemm-mode", mode])
        assert a.ragged_train and a.patch_score_threshold == 0.4 and a.method == "d2s"
    out = capsys.readouterr().out
    assert "Attention: --ragged-train: training follows the cascade definition" in out
    a = _check(TRAIN + THREE + ["--ragged-cascade", "--warmup-steps", "2", "--small-predictor"])
    assert a.ragged_train and a.ragged_cascade and a.warmup_steps == 2
    assert "Attention: --ragged-train" in capsys.readouterr().out
    _check(THR)
    assert "--ragged-train" not in capsys.readouterr().out                    # without the flag: the lines that were there


@pytest.mark.parametrize("argv,fragment", [
    (["--topk-selection", "--ragged-train"], "--ragged-train without --patch-score-threshold"),
    (["--method", "dynamicvit", "--ragged-train"], "--ragged-train with --method dynamicvit"),
    (["--method", "ats", "--ats-train", "--ragged-train"], "--ragged-train with --method ats"),
    (TRAIN + ["--gemm-mode", "bf16"], "--ragged-train with --gemm-mode bf16"),
    (TRAIN + ["--drop-path", "0.1"], "--ragged-train with --drop-path 0.1"),
    (TRAIN + ["--torch-optim"], "--ragged-train with --torch-optim"),
    (TRAIN + ["--eval-only", "--student-checkpoint", "w.pt"], "--ragged-train with --eval-only"),
    (TRAIN + THREE, "--patch-score-threshold with more than one pruning stage"),                     # several stages still need --ragged-cascade
    (TRAIN + THREE + ["--ragged-cascade", "--predictor-bn"], "--ragged-cascade with --predictor-bn"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_build_models_passes_the_keyword_only_under_the_flag(monkeypatch):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(pruning_locs, keep_ratios, **kw):
        seen["kw"] = kw
        kw = {k: v for k, v in kw.items() if k != "checkpoint_path"}
        return vit_models.VisionTransformerDiffPruning(pruning_loc=pruning_locs, token_ratio=keep_ratios, distill=True, **MICRO, **kw)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_student", factory)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_teacher", lambda checkpoint_path=None: vit_models.VisionTransformerTeacher(**MICRO))
    base = dict(arch="deit_tiny", method="d2s", pruning_locs=[1, 2], keep_ratios=[0.5, 0.3], topk_selection=True, early_exit=False,
                mean_heads=False, random_drop=False, small_predictor=False, mask_loss_type="kl_div", predictor_bn=False,
                patch_score_threshold=0.4, student_checkpoint=None, teacher_checkpoint=None, device=torch.device("cpu"))
    student, _ = mask_predictor.build_models(types.SimpleNamespace(**base))
    assert "ragged_train" not in seen["kw"] and student.ragged_train is False
    student, _ = mask_predictor.build_models(types.SimpleNamespace(**base, ragged_train=False))
    assert "ragged_train" not in seen["kw"] and student.ragged_train is False
    student, _ = mask_predictor.build_models(types.SimpleNamespace(**base, ragged_train=True))
    assert seen["kw"]["ragged_train"] is True and student.ragged_train is True


# ---- constructor, TrainStep ----
def _student(**kw):
    import vit_models
    args = dict(pruning_loc=[1, 2], token_ratio=[0.5, 0.3], distill=True, topk_selection=True, predictor_loss_type="kl_div")
    args.update(kw)
    return vit_models.VisionTransformerDiffPruning(**MICRO, **args)


def test_constructor_keyword_and_its_refusals():
    import inspect
    import vit_models
    from vit_models import dynamic_vit
    from d2s import lib, ops
    sig = inspect.signature(vit_models.VisionTransformerDiffPruning.__init__).parameters
    assert sig["ragged_train"].default is False and list(sig)[-3:] == ["init_n", "diff_topk", "topk_num_samples"]
    off, on = _student(patch_score_threshold=0.4), _student(patch_score_threshold=0.4, ragged_train=True)
    assert off.ragged_train is False and on.ragged_train is True
    assert list(off.state_dict()) == list(on.state_dict())                    # no parameters are added
    assert vit_models.dynamic_vit_tiny_patch16_224_student([3], [0.5], patch_score_threshold=0.4, ragged_train=True).ragged_train
    with pytest.raises(ValueError) as e:
        _student(ragged_train=True)
    assert str(e.value) == dynamic_vit.RAGGED_TRAIN_THRESHOLD_ERROR
    with pytest.raises(ValueError) as e:
        _student(patch_score_threshold=0.4, ragged_train=True, drop_path_rate=0.1)
    assert str(e.value) == dynamic_vit.RAGGED_TRAIN_DROP_PATH_ERROR
    # the training forward without a device: the library's loud refusal, not a fall-back to the policy-mode forward
    with pytest.raises(lib.D2SError):
        on.train()(torch.zeros(1, 3, 64, 64))


def test_train_step_refusals_come_before_the_device():
    from d2s import lib
    from d2s.engine import TrainStep
    import vit_models
    teacher = vit_models.VisionTransformerTeacher(**MICRO)
    args = types.SimpleNamespace(mixup=0.0, keep_ratios=[0.5, 0.3], mask_loss_type="kl_div", patch_score_threshold=0.4, ragged_train=True)
    m = _student(patch_score_threshold=0.4, ragged_train=True)
    with pytest.raises(lib.D2SError, match=r"graph=True\) with ragged_train.*one host read per stage"):
        TrainStep(m, teacher, args, graph=True)
    with pytest.raises(lib.D2SError, match="both must agree"):
        TrainStep(m, teacher, types.SimpleNamespace(**{**vars(args), "ragged_train": False}))
    with pytest.raises(lib.D2SError, match="both must agree"):
        TrainStep(_student(patch_score_threshold=0.4), teacher, args)
    m.drop_path_rate = 0.1                                                    # the constructor refuses it; a model altered afterwards
    with pytest.raises(lib.D2SError, match="ragged_train and drop_path_rate > 0"):
        TrainStep(m, teacher, args)


def test_train_one_epoch_needs_the_fused_step():
    import train
    m = _student(patch_score_threshold=0.4, ragged_train=True)
    args = types.SimpleNamespace(mixup=0.0, keep_ratios=[0.5, 0.3], mask_loss_type="kl_div", patch_score_threshold=0.4, ragged_train=True)
    with pytest.raises(ValueError, match="trains through d2s.engine.TrainStep only"):
        train.train_one_epoch(args, m, None, [], torch.optim.SGD(m.parameters(), lr=0.1))


# ---- checkpoints ----
def test_checkpoint_config_records_the_flag():
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    a = cfg(_student(patch_score_threshold=0.4, ragged_train=True))
    b = cfg(_student(patch_score_threshold=0.4))
    assert a["ragged_train"] is True and b["ragged_train"] is False and a["patch_score_threshold"] == 0.4
    assert {k: v for k, v in a.items() if k != "ragged_train"} == {k: v for k, v in b.items() if k != "ragged_train"}
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in b.items() if k != "ragged_train"}
    assert engine.checkpoint_config(old)["ragged_train"] is False and "ragged_train" not in old       # a checkpoint without the key: off
    assert engine.checkpoint_config(a) == a


def test_losses_keep_their_values_without_the_flag():
    """the new keyword of the two loss classes defaults to None and is ignored unless args.ragged_train is set"""
    import inspect
    import losses
    for cls in (losses.MaskLoss, losses.BackboneLoss):
        assert inspect.signature(cls.forward).parameters["ragged"].default is None
    a = types.SimpleNamespace(keep_ratios=[0.5], mask_loss_type="kl_div", patch_score_threshold=0.4)
    assert losses.MaskLoss(a, "train").ragged_train is False and losses.BackboneLoss(a).ragged_train is False
    a.ragged_train = True
    assert losses.MaskLoss(a, "train").ragged_train is True and losses.BackboneLoss(a).ragged_train is True
