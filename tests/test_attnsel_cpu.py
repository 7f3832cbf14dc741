"""Attention selection (attn_selection), the parts that need no GPU: the float64 restatement in tests/attnsel_ref.py on hand-computed
rows (exact ties included), the command line's refusals and its forced warm-up of 0, the constructor's refusals, the checkpoint config
keys and their default for a checkpoint written before the feature, and the library binding."""
import json
import os
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import attnsel_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


# ---- 1. the reference on rows computed by hand ----
def test_ref_max_and_mean_over_heads_on_a_hand_computed_row():
    # one image, two heads, n = 5: column 0 is CLS (lead = 1), four scored tokens
    row = torch.tensor([[[9.0, 1.0, 4.0, 2.0, 1.0],
                         [9.0, 3.0, 2.0, 2.0, 1.0]]])
    w = R.reduce_heads(row, 1, 4)
    assert w.dtype == torch.float64 and w.tolist() == [[3.0, 4.0, 2.0, 1.0]]
    probs, kept, dropped = R.select(row, 1, 4, 2)
    assert probs.tolist() == [[0.3, 0.4, 0.2, 0.1]]
    assert kept.tolist() == [[0, 1]] and dropped.tolist() == [[2, 3]]
    wm = R.reduce_heads(row, 1, 4, mean_heads=True)
    assert wm.tolist() == [[2.0, 3.0, 2.0, 1.0]]
    probs, kept, dropped = R.select(row, 1, 4, 1, mean_heads=True)
    assert probs.tolist() == [[0.25, 0.375, 0.25, 0.125]] and kept.tolist() == [[1]] and dropped.tolist() == [[0, 2, 3]]
    # trailing carried columns are not scored: T = 3 leaves the last column out of the sum too
    probs, kept, dropped = R.select(row, 1, 3, 3)
    assert probs.tolist() == [[3.0 / 9.0, 4.0 / 9.0, 2.0 / 9.0]] and kept.tolist() == [[0, 1, 2]] and dropped.shape == (1, 0)
    assert R.select(row, 1, 4, 0)[1].shape == (1, 0)


def test_ref_exact_ties_take_the_lowest_index_first():
    p = torch.tensor([[0.1, 0.3, 0.3, 0.1, 0.3, 0.1],
                      [0.2, 0.2, 0.2, 0.2, 0.2, 0.2]], dtype=torch.float64)
    for k, kept0, kept1 in ((1, [1], [0]), (2, [1, 2], [0, 1]), (3, [1, 2, 4], [0, 1, 2]), (4, [0, 1, 2, 4], [0, 1, 2, 3])):
        kept, dropped = R.stable_topk(p, k)
        assert kept.tolist() == [kept0, kept1]
        for b in range(2):
            assert sorted(kept[b].tolist() + dropped[b].tolist()) == list(range(6))
            assert dropped[b].tolist() == sorted(dropped[b].tolist())
    # the same through select(): duplicate columns, identical in every head
    row = torch.tensor([[[7.0, 1.0, 5.0, 5.0, 2.0], [7.0, 0.5, 4.0, 4.0, 1.0]]])
    assert R.select(row, 1, 4, 1)[1].tolist() == [[1]] and R.select(row, 1, 4, 1, mean_heads=True)[1].tolist() == [[1]]


def test_ref_stage_loop_and_agreement():
    gen = torch.Generator().manual_seed(3)
    rows = [torch.softmax(torch.randn((2, 2, 16), generator=gen), -1), torch.softmax(torch.randn((2, 2, 9), generator=gen), -1),
            torch.softmax(torch.randn((2, 2, 6), generator=gen), -1)]
    out = R.stage_loop(rows, [1, 2], [8, 4], carried=[0, 1])
    assert out[0][0].shape == (2, 16) and out[0][1].shape == (2, 8) and out[0][2].shape == (2, 8)
    assert out[1][0].shape == (2, 8) and out[1][1].shape == (2, 4)                    # 9 columns, the last one carried
    torch.testing.assert_close(out[1][0].sum(dim=1), torch.ones(2, dtype=torch.float64))
    a = torch.tensor([[0, 1, 2]]); b = torch.tensor([[1, 2, 3]])
    assert R.mask_agreement(a, a, 6) == 1.0 and R.mask_agreement(a, b, 6) == pytest.approx(4.0 / 6.0)
    t = R.teacher_target(torch.softmax(torch.randn((2, 3, 2, 7), generator=gen), -1))
    assert t.shape == (2, 6) and torch.allclose(t.sum(dim=1), torch.ones(2, dtype=torch.float64))


def test_gapped_rows_have_the_gap_they_promise():
    for (B, H, n, lead, T) in ((1, 1, 6, 1, 5), (2, 6, 199, 1, 196), (1, 12, 577, 1, 576)):
        for mean in (False, True):
            rows = R.gapped_rows(B, H, n, lead, T, mean, seed=1)
            assert rows.dtype == torch.float32 and bool((rows > 0).all())
            rel, of_sum = R.rank_gaps(R.reduce_heads(rows, lead, T, mean))
            assert rel >= 1e-3
            if T * (T - 1) // 2 <= 1000:
                assert of_sum >= 1e-3


# ---- 2. command line ----
def test_check_supported_refusals_and_the_forced_warmup(capsys):
    import mask_predictor
    import utils
    assert utils.parse_args([]).attn_selection is False and utils.parse_args([]).mean_heads is False
    refusals = ((["--attn-selection"], "--attn-selection without --topk-selection"),
                (["--attn-selection", "--topk-selection", "--patch-score-threshold", "0.5"], "--attn-selection with --patch-score-threshold"),
                (["--attn-selection", "--topk-selection", "--diff-topk"], "--attn-selection with --diff-topk"),
                (["--attn-selection", "--method", "dynamicvit"], "--method dynamicvit with --attn-selection"),
                (["--attn-selection", "--topk-selection", "--pruning-locs", "0", "--keep-ratios", "0.5"], "pruning location of 0"),
                (["--attn-selection", "--topk-selection", "--pruning-locs", "3", "0", "--keep-ratios", "0.5", "0.3"], "pruning location of 0"))
    for extra, needle in refusals:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert needle in str(e.value), (extra, str(e.value))
    capsys.readouterr()
    a = utils.parse_args(["--attn-selection", "--topk-selection", "--warmup-steps", "5"])
    assert a.warmup_steps == 5
    mask_predictor.check_supported(a)
    out = capsys.readouterr().out
    assert a.warmup_steps == 0
    assert any(line.startswith("Attention:") and "mask_predictor.py:300" in line and "--attn-selection" in line for line in out.splitlines())
    a = utils.parse_args(["--attn-selection", "--topk-selection", "--fuse-dropped", "--mean-heads"])     # EViT: allowed
    mask_predictor.check_supported(a)
    assert a.warmup_steps == 0 and a.fuse_dropped and a.mean_heads
    capsys.readouterr()
    a = utils.parse_args(["--topk-selection", "--mean-heads", "--warmup-steps", "2"])
    mask_predictor.check_supported(a)
    out = capsys.readouterr().out
    assert a.warmup_steps == 2                                              # untouched without the flag
    assert any(line.startswith("Attention:") and "--mean-heads has no effect" in line for line in out.splitlines())
    capsys.readouterr()
    mask_predictor.check_supported(utils.parse_args(["--topk-selection"]))
    out = capsys.readouterr().out
    assert "attn-selection" not in out and "mean-heads" not in out


def test_build_models_passes_the_flag(monkeypatch):
    import mask_predictor
    import utils
    import vit_models
    seen = {}

    def fake_student(locs, ratios, **kw):
        seen.update(kw)
        return torch.nn.Identity()
    monkeypatch.setattr(vit_models, "dynamic_vit_small_patch16_224_student", fake_student)
    monkeypatch.setattr(vit_models, "dynamic_vit_small_patch16_224_teacher", lambda **kw: torch.nn.Identity())
    for flags, want in ((["--topk-selection", "--attn-selection", "--mean-heads"], (True, True)), (["--topk-selection"], (False, False))):
        a = utils.parse_args(["--arch", "deit_small"] + flags)
        a.device = "cpu"
        mask_predictor.build_models(a)
        assert (seen["attn_selection"], seen["mean_heads"]) == want


# ---- 3. constructor ----
def _student(**kw):
    import vit_models
    kw.setdefault("topk_selection", True)
    kw.setdefault("pruning_loc", [1])
    kw.setdefault("token_ratio", [0.05] * len(kw["pruning_loc"]))
    return vit_models.VisionTransformerDiffPruning(distill=True, predictor_loss_type="kl_div", **MICRO, **kw)


def test_constructor_default_and_refusals():
    from vit_models import dynamic_vit
    off, on = _student(), _student(attn_selection=True, mean_heads=True)
    assert not off.attn_selection and on.attn_selection and on.mean_heads
    assert list(off.state_dict()) == list(on.state_dict())                    # the predictors are still constructed: same keys
    assert len(on.score_predictor) == 1 and on.attn_selection_threshold == 0.0
    for kw, msg in ((dict(topk_selection=False), dynamic_vit.ATTN_SELECTION_TOPK_SELECTION_ERROR),
                    (dict(patch_score_threshold=0.5), dynamic_vit.ATTN_SELECTION_THRESHOLD_ERROR),
                    (dict(diff_topk=True), dynamic_vit.ATTN_SELECTION_DIFF_TOPK_ERROR),
                    (dict(pruning_loc=[0]), dynamic_vit.ATTN_SELECTION_BLOCK0_ERROR),
                    (dict(pruning_loc=[0, 2]), dynamic_vit.ATTN_SELECTION_BLOCK0_ERROR)):
        with pytest.raises(ValueError) as e:
            _student(attn_selection=True, **kw)
        assert str(e.value) == msg
    _student(pruning_loc=[0])                                                 # block 0 stays legal for the predictor
    _student(attn_selection=True, fuse_dropped=True)                          # EViT
    import vit_models
    small = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, attn_selection=True)
    assert small.attn_selection                                               # the factories forward **kwargs
    assert "attn_selection" in vit_models.VisionTransformerDiffPruning.__doc__ and "pred_logits" in vit_models.VisionTransformerDiffPruning.__doc__


# ---- 4. checkpoint config ----
def test_checkpoint_config_records_the_flags_and_old_checkpoints_count_as_off():
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    students = (_student(), _student(attn_selection=True), _student(attn_selection=True, mean_heads=True), _student(mean_heads=True))
    cfgs = [engine.TrainStep.config(types.SimpleNamespace(student=s, args=args)) for s in students]
    assert [(c["attn_selection"], c["mean_heads"]) for c in cfgs] == [(False, False), (True, False), (True, True), (False, False)]
    for c in cfgs:
        assert json.loads(json.dumps(c)) == c
    assert {k for k in cfgs[0] if cfgs[0][k] != cfgs[2][k]} == {"attn_selection", "mean_heads"}
    assert cfgs[0] == cfgs[3]                                                 # mean_heads alone changes nothing, so it is not recorded
    old = {k: v for k, v in cfgs[0].items() if k not in ("attn_selection", "mean_heads")}
    filled = engine.checkpoint_config(old)
    assert filled["attn_selection"] is False and filled["mean_heads"] is False and filled == cfgs[0]
    assert "attn_selection" not in old                                        # the checkpoint's own dict is left alone
    assert engine.checkpoint_config(cfgs[2]) == cfgs[2]


def test_train_step_refuses_a_warmup_with_an_attention_selecting_student():
    """the refusal comes before anything touches the device"""
    from d2s.engine import TrainStep
    with pytest.raises(ValueError, match="warmup_steps"):
        TrainStep(_student(attn_selection=True), torch.nn.Identity(), types.SimpleNamespace(), warmup_steps=1)


# ---- 5. binding ----
def test_library_binding_declares_the_entry():
    from d2s import lib
    header = open(os.path.join(REPO, "include", "d2s_hip.h")).read()
    assert "d2s_select_cls_attn" in lib.symbols("d2s_hip.h") and "int d2s_select_cls_attn(" in header
    from d2s import ops
    assert callable(ops.select_cls_attn)
