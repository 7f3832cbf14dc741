"""Adaptive token sampling, the parts that need no GPU: the properties of the selection rule as tests/ats_ref.py
states it, and the host side - header and binding tables, command line, build_models, constructor, state-dict keys."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import ats_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_ats_select"]


# ---- the selection rule ----
@pytest.mark.parametrize("T,K", [(1, 1), (1, 7), (4, 4), (16, 3), (16, 40), (196, 196), (196, 64), (300, 98), (576, 576), (576, 1)])
def test_select_keeps_between_one_and_min_K_T_and_every_heavy_token(T, K):
    rng = np.random.default_rng(100 * T + K)
    for alpha in (0.05, 0.3, 1.0, 20.0):
        s = rng.dirichlet(np.full(T, alpha)).astype(np.float32)
        keep = R.select(s, K)
        assert keep.dtype == bool and keep.shape == (T,)
        assert 1 <= int(keep.sum()) <= min(K, T)
        heavy = s >= np.float32(1.01) / np.float32(K)
        assert bool(keep[heavy].all()), (T, K, alpha, np.nonzero(heavy & ~keep)[0])


def test_select_scores_with_zeros_and_ties():
    s = np.array([0.0, 0.5, 0.0, 0.5, 0.0], dtype=np.float32)
    assert R.select(s, 2).tolist() == [False, True, False, True, False]      # thresholds 0.25 and 0.75: the two heavy tokens, in index order
    assert R.select(s, 1).tolist() == [False, True, False, False, False]     # 0.5: reached by the first of the two equal tokens
    assert R.select(np.zeros(0, dtype=np.float32), 3).shape == (0,)


@pytest.mark.parametrize("T", [1, 4, 16, 196, 576])
def test_uniform_scores_with_K_equal_T_keep_everything(T):
    s = np.full(T, np.float32(1.0) / np.float32(T), dtype=np.float32)
    assert bool(R.select(s, T).all())
    assert 1 <= int(R.select(s, T + 5).sum()) <= T      # K > T works: with more thresholds than tokens some positions are picked twice


def test_uniform_scores_with_half_the_tokens_keep_every_second_one_from_token_0():
    s = np.full(16, np.float32(1.0 / 16), dtype=np.float32)
    assert np.nonzero(R.select(s, 8))[0].tolist() == list(range(0, 16, 2))       # the tie rule: equal values lowest index first


def test_scores_reference_normalises_per_image_and_falls_back_to_uniform():
    rng = np.random.default_rng(3)
    cu = [0, 5, 6, 9]
    cls_row, v = rng.random((2, 9)), rng.standard_normal((9, 128))
    s = R.scores(cls_row, v, cu)
    assert s[0] == s[5] == s[6] == 0 and s[1:5].sum() == pytest.approx(1.0) and s[7:9].sum() == pytest.approx(1.0)
    want = cls_row.sum(0)[1:5] * np.linalg.norm(v[1:5], axis=1)
    np.testing.assert_allclose(s[1:5], want / want.sum(), rtol=1e-12)
    assert R.scores(np.zeros((2, 9)), v, cu)[1:5].tolist() == [0.25] * 4
    assert R.scores(np.full((2, 9), np.inf), v, cu)[7:9].tolist() == [0.5] * 2


# ---- header and binding ----
def test_ats_header_and_binding_tables():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ats.h")).read()
    assert NEW == lib.symbols("d2s_hip_ats.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) >= 1 + len(NEW)               # the file's own comment and one per entry
    assert callable(ops.ats_select)
    from d2s import functional_ats
    assert callable(functional_ats.ats_block_forward)


# ---- command line ----
ATS = ["--method", "ats", "--eval-only", "--student-checkpoint", "w.pt"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_the_method_and_its_token_counts():
    a = _check(ATS + ["--pruning-locs", "3", "6", "9", "--ats-tokens", "64"])
    assert a.method == "ats" and a.ats_tokens == [64] and a.pruning_locs == [3, 6, 9]
    assert _check(ATS + ["--pruning-locs", "3", "6", "9", "--ats-tokens", "128", "64", "32"]).ats_tokens == [128, 64, 32]
    assert _check(ATS + ["--pruning-locs", "3", "6"]).ats_tokens is None
    for mode in ("exact", "split", "bf16"):
        assert _check(ATS + ["--gemm-mode", mode]).gemm_mode == mode
    assert _check([]).ats_tokens is None and _check([]).method == "d2s"
    import utils
    with pytest.raises(SystemExit):
        utils.parse_args(["--method", "other"])


@pytest.mark.parametrize("argv,fragment", [
    (["--method", "ats", "--student-checkpoint", "w.pt"], "--method ats without --eval-only"),
    (ATS + ["--tome-r", "2"], "--tome-r 2 with --method ats"),
    (ATS + ["--tome-train"], "--tome-train with --method ats"),
    (ATS + ["--tome-bf16"], "--tome-bf16 with --method ats"),
    (ATS + ["--topk-selection"], "--method ats with --topk-selection"),
    (ATS + ["--topk-selection", "--attn-selection"], "--method ats with --attn-selection"),
    (ATS + ["--topk-selection", "--fuse-dropped"], "--method ats with --fuse-dropped"),
    (ATS + ["--topk-selection", "--squeeze-dropped"], "--method ats with --squeeze-dropped"),
    (ATS + ["--topk-selection", "--diff-topk"], "--method ats with --diff-topk"),
    (ATS + ["--patch-score-threshold", "0.4"], "--method ats with --patch-score-threshold"),
    (ATS + ["--pruning-locs", "3", "6", "9", "--ats-tokens", "64", "32"], "--ats-tokens with 2 values for 3 stages"),
    (ATS + ["--ats-tokens", "0"], "--ats-tokens 0 (at least 1"),
    (["--ats-tokens", "64"], "--ats-tokens with --method d2s"),
    (["--method", "tome", "--tome-r", "2", "--eval-only", "--student-checkpoint", "w.pt", "--ats-tokens", "64"], "--ats-tokens with --method tome"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert "not on the accelerated path" in str(e.value) and fragment in str(e.value), str(e.value)


def test_build_models_passes_the_stages_on(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(ats_locs=(), ats_tokens=None, checkpoint_path=None, **kw):
        seen.update(ats_locs=ats_locs, ats_tokens=ats_tokens, checkpoint_path=checkpoint_path, kw=kw)
        return vit_models.VisionTransformerATS(ats_locs=ats_locs, ats_tokens=ats_tokens, **MICRO)
    monkeypatch.setattr(vit_models, "ats_deit_tiny_patch16_224", factory)
    args = types.SimpleNamespace(arch="deit_tiny", method="ats", pruning_locs=[1, 3], ats_tokens=[8, 4], student_checkpoint=None, resume=None,
                                 device=torch.device("cpu"))
    student, teacher = mask_predictor.build_models(args)
    assert teacher is None and isinstance(student, vit_models.VisionTransformerATS)
    assert seen["ats_locs"] == [1, 3] and seen["ats_tokens"] == [8, 4] and seen["checkpoint_path"] is None and seen["kw"] == {}
    assert student.ats_locs == [1, 3] and student.ats_tokens == [8, 4]
    assert "starts from its random initialisation" in capsys.readouterr().out
    args.ats_tokens = [6]
    assert mask_predictor.build_models(args)[0].ats_tokens == [6, 6] and seen["ats_tokens"] == 6
    args.ats_tokens = None
    assert mask_predictor.build_models(args)[0].ats_tokens == [16, 16] and seen["ats_tokens"] is None


def test_build_models_ignores_predictor_tensors_of_the_checkpoint(monkeypatch, tmp_path, capsys):
    import mask_predictor
    import vit_models
    monkeypatch.setattr(vit_models, "ats_deit_tiny_patch16_224",
                        lambda ats_locs=(), ats_tokens=None, **kw: vit_models.VisionTransformerATS(ats_locs=ats_locs, ats_tokens=ats_tokens, **MICRO))
    sd = vit_models.VisionTransformerTeacher(**MICRO).state_dict()
    sd["score_predictor.0.in_conv.0.weight"] = torch.ones(128)
    path = os.path.join(tmp_path, "student.pt")
    torch.save({"model": sd}, path)
    args = types.SimpleNamespace(arch="deit_tiny", method="ats", pruning_locs=[1], ats_tokens=None, student_checkpoint=path, resume=None,
                                 device=torch.device("cpu"))
    student, _ = mask_predictor.build_models(args)
    out = capsys.readouterr().out
    assert "--method ats: trunk weights from" in out and "ignored 1 predictor tensors (adaptive token sampling has no predictor)" in out
    assert torch.equal(student.head.weight, sd["head.weight"])
    del sd["head.weight"]
    torch.save({"model": sd}, path)
    with pytest.raises(SystemExit, match="no weights for 1 tensors"):
        mask_predictor.build_models(args)


# ---- model ----
def test_constructor_validates_its_arguments():
    import vit_models
    m = vit_models.VisionTransformerATS(ats_locs=[1, 2, 3], ats_tokens=[12, 8, 4], **MICRO)
    assert m.ats_locs == [1, 2, 3] and m.ats_tokens == [12, 8, 4]
    assert vit_models.VisionTransformerATS(ats_locs=(0, 2), ats_tokens=5, **MICRO).ats_tokens == [5, 5]
    assert vit_models.VisionTransformerATS(ats_locs=(0, 2), **MICRO).ats_tokens == [16, 16]
    plain = vit_models.VisionTransformerATS(**MICRO)
    assert plain.ats_locs == [] and plain.ats_tokens == [] and plain.tokens_per_stage == [] and plain.ats_plans == []
    for kw in (dict(ats_locs=[4]), dict(ats_locs=[-1]), dict(ats_locs=[2, 1]), dict(ats_locs=[1, 1]), dict(ats_locs=[1], ats_tokens=[3, 4]),
               dict(ats_locs=[1, 2], ats_tokens=[3]), dict(ats_locs=[1], ats_tokens=0), dict(ats_locs=[1], ats_tokens=[-2])):
        with pytest.raises(ValueError):
            vit_models.VisionTransformerATS(**MICRO, **kw)


def test_state_dict_keys_are_the_teachers_and_the_factories_exist():
    import vit_models
    from vit_models import ats
    teacher = vit_models.VisionTransformerTeacher(**MICRO)
    m = vit_models.VisionTransformerATS(ats_locs=[1, 2], ats_tokens=4, **MICRO)
    assert list(m.state_dict()) == list(teacher.state_dict())
    m.load_state_dict(teacher.state_dict(), strict=True)
    for size in ("tiny", "small", "base"):
        assert callable(getattr(vit_models, f"ats_deit_{size}_patch16_224"))
    assert isinstance(ats.ATS_TRAINING_ERROR, str) and "inference only" in ats.ATS_TRAINING_ERROR
    tiny = vit_models.ats_deit_tiny_patch16_224(ats_locs=(3, 6, 9), ats_tokens=64)
    assert tiny.ats_locs == [3, 6, 9] and tiny.ats_tokens == [64] * 3 and len(tiny.blocks) == 12
    assert list(tiny.state_dict()) == list(vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict())


def test_training_mode_with_a_stage_is_refused_before_anything_runs():
    import vit_models
    from vit_models import ats
    m = vit_models.VisionTransformerATS(ats_locs=[1], **MICRO).train()
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(1, 3, 64, 64))
    assert str(e.value) == ats.ATS_TRAINING_ERROR


def test_evaluate_treats_the_model_as_a_baseline():
    """evaluate_performance asks methods.eval_returns_logits_alone: with and without stages the model's eval() returns logits alone."""
    import methods
    import vit_models
    for kw in (dict(ats_locs=[1], ats_tokens=4), dict()):
        m = vit_models.VisionTransformerATS(**MICRO, **kw)
        assert methods.eval_returns_logits_alone(m) is True
        assert methods.of(m).eval_extras == ()
    assert methods.of(vit_models.VisionTransformerATS(**MICRO, ats_locs=[1])).name == "ats"
    assert methods.of(vit_models.VisionTransformerATS(**MICRO)).name == "d2s"          # no stage: the dense trunk, where it was
    import evaluate
    assert evaluate.methods is methods
