"""CPU tier of training on the ragged packed batch in the bf16 arithmetic mode (ragged_bf16=True / --ragged-bf16): the
closed header and its binding table, the command line, the constructor keyword, the checkpoint key, and the evidence that the float64
reference of tests/attention_bf16_ref.py carries the GPU tier's lengths - the emulation of the kernels' roundings alone stays inside
the derived bounds at every length of tests/test_ragged_bf16_train_gpu.py, n = 1 included."""
import json
import os
import re
import types

import pytest
import torch

from tests import attention_bf16_ref as AR
from tests import cases  # noqa: F401  (puts the package on sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_attn_varlen_bwd_bf16", "d2s_attn_varlen_fwd_lse_bf16"]
# the packed batches of the GPU tier: (lengths, H, the two bounds max_n)
SETS = {"a": ((1, 2, 17, 32, 33), 2, (33, 64)), "b": ((128, 129, 1, 97), 3, (129, 256)), "c": ((197, 70), 2, (197,))}


# ---- the header and the binding tables ----
def test_header_declares_the_two_entries_and_the_older_tables_are_what_they_were():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ragged_bf16.h")).read()
    assert NEW == lib.symbols("d2s_hip_ragged_bf16.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    # the signatures: the inference entry's with lse behind the outputs; the dense bf16out backward's with cu_seqlens and total, max_n for n
    fwd, bwd = lib.signature("d2s_attn_varlen_fwd_lse_bf16"), lib.signature("d2s_attn_varlen_bwd_bf16")
    inf = lib.signature("d2s_attn_varlen_fwd_bf16")[1]
    assert fwd[0] is lib.I and fwd[1] == inf[:5] + [lib.P] + inf[5:]
    dense = lib.signature("d2s_attn_bwd_bf16_bf16out")[1]
    assert bwd[0] is lib.I and bwd[1] == dense[:2] + [lib.P] + dense[2:8] + [lib.I, lib.I, lib.I, lib.I, lib.F]
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "attention_bf16.hip")).read()
    for name in NEW:
        assert len(re.findall(rf"^int {name}\(", src, flags=re.M)) == 1, name
    assert "atomic" not in src.lower().replace("no atomics", "")
    assert callable(ops.attn_varlen_fwd_lse_bf16io) and callable(ops.attn_varlen_bwd_bf16io)


# ---- command line ----
THR = ["--topk-selection", "--patch-score-threshold", "0.4"]
TRAIN = THR + ["--ragged-train"]
PINNED = "--ragged-train with --gemm-mode bf16 (training through a ragged block is built on the fp32 data path; exact and split run)"


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_the_flag_and_reports_the_bf16_mode(capsys):
    import utils
    assert utils.parse_args([]).ragged_bf16 is False
    a = _check(TRAIN + ["--ragged-bf16"])
    assert a.ragged_train and a.ragged_bf16 and a.gemm_mode == "exact"           # the flag, not --gemm-mode, selects the path
    out = capsys.readouterr().out
    assert "Attention: --ragged-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    assert "Attention: --ragged-train: training follows the cascade definition" in out
    _check(TRAIN + ["--ragged-bf16", "--gemm-mode", "exact"])
    capsys.readouterr()
    _check(TRAIN)
    assert "--ragged-bf16" not in capsys.readouterr().out                       # without the flag: the lines that were there


@pytest.mark.parametrize("argv,fragment", [
    (THR + ["--ragged-bf16"], "--ragged-bf16 without --ragged-train"),
    (["--ragged-bf16"], "--ragged-bf16 without --ragged-train"),
    (TRAIN + ["--ragged-bf16", "--gemm-mode", "split"], "--ragged-bf16 with --gemm-mode split"),
    (TRAIN + ["--gemm-mode", "bf16"], PINNED),
    (TRAIN + ["--ragged-bf16", "--gemm-mode", "bf16"], PINNED),
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
                patch_score_threshold=0.4, student_checkpoint=None, teacher_checkpoint=None, device=torch.device("cpu"), ragged_train=True)
    student, _ = mask_predictor.build_models(types.SimpleNamespace(**base))
    assert "ragged_bf16" not in seen["kw"] and student.ragged_bf16 is False
    student, _ = mask_predictor.build_models(types.SimpleNamespace(**base, ragged_bf16=True))
    assert seen["kw"]["ragged_bf16"] is True and student.ragged_bf16 is True and student.ragged_train is True


# ---- constructor, TrainStep, checkpoints ----
def _student(**kw):
    import vit_models
    args = dict(pruning_loc=[1, 2], token_ratio=[0.5, 0.3], distill=True, topk_selection=True, predictor_loss_type="kl_div")
    args.update(kw)
    return vit_models.VisionTransformerDiffPruning(**MICRO, **args)


def test_constructor_keyword_and_its_refusal():
    import inspect
    import vit_models
    from vit_models import dynamic_vit
    names = list(inspect.signature(vit_models.VisionTransformerDiffPruning.__init__).parameters)
    assert names.index("ragged_bf16") == names.index("ragged_train") + 1 and names[-3:] == ["init_n", "diff_topk", "topk_num_samples"]
    assert inspect.signature(vit_models.VisionTransformerDiffPruning.__init__).parameters["ragged_bf16"].default is False
    off, on = _student(patch_score_threshold=0.4, ragged_train=True), _student(patch_score_threshold=0.4, ragged_train=True, ragged_bf16=True)
    assert off.ragged_bf16 is False and on.ragged_bf16 is True and on.ragged_train is True
    assert list(off.state_dict()) == list(on.state_dict())                    # no parameters are added
    for factory in (vit_models.dynamic_vit_tiny_patch16_224_student, vit_models.dynamic_vit_small_patch16_224_student,
                    vit_models.dynamic_vit_base_patch16_224_student):
        with pytest.raises(ValueError) as e:                                  # the three factories hand the keyword through
            factory([3], [0.5], patch_score_threshold=0.4, ragged_bf16=True)
        assert str(e.value) == dynamic_vit.RAGGED_BF16_ERROR
    assert vit_models.dynamic_vit_tiny_patch16_224_student([3], [0.5], patch_score_threshold=0.4, ragged_train=True, ragged_bf16=True).ragged_bf16
    with pytest.raises(ValueError) as e:
        _student(patch_score_threshold=0.4, ragged_bf16=True)
    assert str(e.value) == dynamic_vit.RAGGED_BF16_ERROR


def test_refusal_texts_and_the_ragged_description():
    from d2s import functional_ats as AF
    assert AF._BF16_REFUSAL == ("training through a ragged block runs in the fp32 arithmetic modes (exact, split): the varlen attention "
                                "backward is an fp32 kernel")
    assert AF._BF16_STAGE_REFUSAL.startswith(AF._BF16_REFUSAL) and "sample_bwd" in AF._BF16_STAGE_REFUSAL
    cu = torch.tensor([0, 3], dtype=torch.int32)
    assert AF._Ragged(cu, 1, 3, 2, 0.125).bf16 is False and AF._Ragged(cu, 1, 3, 2, 0.125, bf16=True).bf16 is True
    assert AF._Ragged(cu, 1, 3, 2, 0.125, None, 2, 4, None).K == 2                # the positional layout of the existing callers


def test_train_step_graph_refusal_and_checkpoint_config():
    from d2s import engine, lib
    import vit_models
    teacher = vit_models.VisionTransformerTeacher(**MICRO)
    args = types.SimpleNamespace(mixup=0.0, keep_ratios=[0.5, 0.3], mask_loss_type="kl_div", patch_score_threshold=0.4, ragged_train=True)
    on = _student(patch_score_threshold=0.4, ragged_train=True, ragged_bf16=True)
    with pytest.raises(lib.D2SError, match=r"graph=True\) with ragged_train.*one host read per stage"):
        engine.TrainStep(on, teacher, args, graph=True)
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=types.SimpleNamespace(mask_loss_type="kl_div")))
    a, b = cfg(on), cfg(_student(patch_score_threshold=0.4, ragged_train=True))
    assert a["ragged_bf16"] is True and b["ragged_bf16"] is False and a["ragged_train"] is b["ragged_train"] is True
    assert {k: v for k, v in a.items() if k != "ragged_bf16"} == {k: v for k, v in b.items() if k != "ragged_bf16"}
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in a.items() if k != "ragged_bf16"}
    assert engine.checkpoint_config(old)["ragged_bf16"] is False and "ragged_bf16" not in old       # a checkpoint without the key: off
    assert engine.checkpoint_config(a) == a


# ---- the float64 reference at the GPU tier's lengths ----
@pytest.mark.parametrize("kind", AR.KINDS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_emulation_stays_inside_the_bounds_at_the_lengths_of_the_gpu_tier(name, kind):
    """the emulation of the kernels' bf16 roundings (float64 otherwise) against the float64 reference, one image at a time as the GPU
    tier builds its packed batches: |emu - ref| / bound <= 1 for all six outputs, so the bounds have room for the fp32 chains"""
    lengths, H, _ = SETS[name]
    worst = {}
    for n in sorted(set(lengths)):
        fr = AR.bound_fractions(AR.emulate(1, H, n, kind), AR.reference(1, H, n, kind))
        for k, v in fr.items():
            assert v <= 1.0, (n, H, kind, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"set {name} H {H} {kind}: emulation max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
