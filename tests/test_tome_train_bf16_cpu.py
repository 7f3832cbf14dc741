"""CPU tier of training through token merging in the bf16 arithmetic mode (train_bf16=True / --tome-train-bf16): the
closed header and its binding table, the command line, the constructor keyword, the checkpoint key, the hook convention of
block_backward_sequence, and the evidence that the bounds of tests/tome_train_bf16_cases.py are not fixed blind - the emulation of the
kernels' roundings stays inside them on every input of tests/test_tome_train_bf16_gpu.py, and the same emulation without the weights
does not."""
import inspect
import json
import os
import re
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import tome_bf16_cases as C
from tests import tome_train_bf16_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_attn_keyw_bwd_bf16", "d2s_tome_merge_bwd_bf16out"]


# ---- the header and the binding tables ----
def test_header_declares_the_two_entries_and_the_older_tables_are_what_they_were():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_tome_train_bf16.h")).read()
    assert NEW == lib.symbols("d2s_hip_tome_train_bf16.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    # the signatures: the dense bf16out backward's with key_w behind qkv; the fp32 merge backward's with the bf16 output last
    kb, mb = lib.signature("d2s_attn_keyw_bwd_bf16"), lib.signature("d2s_tome_merge_bwd_bf16out")
    dense = lib.signature("d2s_attn_bwd_bf16_bf16out")[1]
    assert kb[0] is lib.I and kb[1] == dense[:2] + [lib.P] + dense[2:]
    assert mb[0] is lib.I and mb[1] == lib.signature("d2s_tome_merge_bwd")[1] + [lib.P]
    for name, f in zip(NEW, ("attention_bf16.hip", "tome.hip")):
        src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", f)).read()
        assert len(re.findall(rf"^int {name}\(", src, flags=re.M)) == 1, name
        assert "atomic" not in src.lower().replace("no atomics", "")
    assert callable(ops.attn_keyw_bwd_bf16io) and "dx16" in inspect.signature(ops.tome_merge_bwd).parameters


# ---- command line ----
TRAIN = ["--method", "tome", "--tome-train", "--tome-r", "2"]
PINNED_MODE = "--method tome with --gemm-mode bf16 (the key-weighted attention is an fp32 kernel; exact and split run)"
PINNED_BF16 = "--tome-bf16 with --tome-train (training through the merges is built in fp32 only)"


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_the_flag_and_reports_the_bf16_mode(capsys):
    import utils
    assert getattr(utils.parse_args([]), "tome_train_bf16", False) is False
    assert "tome_train_bf16" not in vars(utils.parse_args([]))                    # the namespace of every other command line is what it was
    a = _check(TRAIN + ["--tome-train-bf16"])
    assert a.tome_train and a.tome_train_bf16 is True and a.gemm_mode == "exact"   # the flag, not --gemm-mode, selects the path
    out = capsys.readouterr().out
    assert "Attention: --tome-train-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    _check(TRAIN + ["--tome-train-bf16", "--gemm-mode", "exact"])
    capsys.readouterr()
    _check(TRAIN)
    assert "--tome-train-bf16" not in capsys.readouterr().out                    # without the flag: the lines that were there


@pytest.mark.parametrize("argv,fragment", [
    (["--method", "tome", "--tome-train-bf16", "--eval-only", "--student-checkpoint", "w.pt"], "--tome-train-bf16 without --tome-train"),
    (["--tome-train-bf16"], "--tome-train-bf16 without --tome-train"),
    (TRAIN + ["--tome-train-bf16", "--tome-bf16"], "--tome-train-bf16 with --tome-bf16"),
    (TRAIN + ["--tome-train-bf16", "--gemm-mode", "split"], "--tome-train-bf16 with --gemm-mode split"),
    (TRAIN + ["--gemm-mode", "bf16"], PINNED_MODE),
    (TRAIN + ["--tome-train-bf16", "--gemm-mode", "bf16"], PINNED_MODE),
    (TRAIN + ["--tome-bf16"], PINNED_BF16),
    (TRAIN + ["--tome-train-bf16", "--tome-bf16"], PINNED_BF16),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_build_tome_passes_the_keyword_only_under_the_flag(monkeypatch):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(tome_r, **kw):
        seen["kw"] = kw
        return vit_models.VisionTransformerToMe(**MICRO, tome_r=tome_r, **kw)
    monkeypatch.setattr(vit_models, "tome_deit_tiny_patch16_224", factory)
    base = dict(arch="deit_tiny", method="tome", tome_r=2, tome_train=True, student_checkpoint=None, resume=None, device=torch.device("cpu"))
    m = mask_predictor.build_tome(types.SimpleNamespace(**base))
    assert "train_bf16" not in seen["kw"] and m.train_bf16 is False and m.train_merge is True
    m = mask_predictor.build_tome(types.SimpleNamespace(**base, tome_train_bf16=True))
    assert seen["kw"]["train_bf16"] is True and m.train_bf16 is True and m.train_merge is True and m.bf16 is False


# ---- constructor, TrainStep, checkpoints ----
def test_constructor_keyword_and_its_refusals():
    import vit_models
    from vit_models import tome
    params = inspect.signature(tome.VisionTransformerToMe.__init__).parameters
    assert params["train_bf16"].default is False and list(params).index("train_bf16") == list(params).index("bf16") + 1
    on = vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_merge=True, train_bf16=True)
    off = vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_merge=True)
    assert on.train_bf16 is True and off.train_bf16 is False and on.bf16 is False
    assert list(on.state_dict()) == list(off.state_dict())                        # no parameters are added
    with pytest.raises(ValueError, match="train_bf16 without train_merge"):
        vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_bf16=True)
    with pytest.raises(ValueError, match="bf16 with train_merge: training through a merge is built in fp32 only"):      # the pinned one first
        vit_models.VisionTransformerToMe(**MICRO, tome_r=3, bf16=True, train_merge=True, train_bf16=True)
    for factory in (vit_models.tome_deit_tiny_patch16_224, vit_models.tome_deit_small_patch16_224, vit_models.tome_deit_base_patch16_224):
        with pytest.raises(ValueError, match="train_bf16 without train_merge"):   # the three factories hand the keyword through
            factory(2, train_bf16=True)
    assert vit_models.tome_deit_tiny_patch16_224(2, train_merge=True, train_bf16=True).train_bf16 is True


def test_train_step_config_graph_refusal_and_checkpoint_key():
    from d2s import engine, lib
    import vit_models
    make = lambda **kw: vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_merge=True, **kw)
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=types.SimpleNamespace(mask_loss_type="kl_div")))
    a, b = cfg(make(train_bf16=True)), cfg(make())
    # the key is recorded where it is on; without it - the default, every other family, every older checkpoint - it counts as off
    assert a["train_bf16"] is True and b.get("train_bf16", False) is False and "train_bf16" not in b
    assert {k: v for k, v in a.items() if k != "train_bf16"} == b and list(a)[:-1] == list(b)
    assert json.loads(json.dumps(a)) == a
    assert engine.checkpoint_config(b).get("train_bf16", False) is False and engine.checkpoint_config(a)["train_bf16"] is True
    with pytest.raises(lib.D2SError, match=r"graph=True\).*a captured merging step is not built"):
        engine.TrainStep(make(train_bf16=True), None, types.SimpleNamespace(mixup=0.0), graph=True)


def test_refusal_texts_and_the_hook_convention():
    from d2s import functional as DF
    from d2s import functional_tome as TF
    assert TF._BF16_REFUSAL == "token merging runs in the fp32 arithmetic modes (exact, split): the key-weighted attention has no bf16 kernel"
    assert "bf16 arithmetic mode" in TF._BF16_MODE_NEEDED and "data path" in TF._BF16_PATH_NEEDED
    p = inspect.signature(DF.block_backward_sequence).parameters
    assert list(p)[-2:] == ["mid_bwd", "mid_bwd_bf16"] and p["mid_bwd_bf16"].default is False and p["mid_bwd"].default is None
    assert inspect.signature(TF.tome_block_train).parameters["bf16"].default is False
    assert list(inspect.signature(TF.tome_block_train).parameters)[:9] == ["x", "size", "params", "heads", "eps", "scale", "r", "prop_attn", "plan"]
    m = TF._Merging(None, 2, 9, 128, 2, 0.125, 0, True, None)
    g, gh = torch.zeros(18, 128), torch.zeros(18, 128, dtype=torch.bfloat16)
    assert m.merge_bwd(g) is g and m.merge_bwd_bf16(g, gh) == (g, gh)             # r = 0: both forms pass through


# ---- the float64 reference on the GPU tier's inputs ----
@pytest.mark.parametrize("n,H", TC.SHAPES)
def test_emulation_stays_inside_the_bounds_and_fails_them_without_the_weights(n, H):
    """the emulation of the kernels' roundings (float64 otherwise) against the float64 reference: |emu - ref| / bound <= 1 for dq, dk and
    dv, so the bounds have room for the fp32 chains; the same emulation with the weights left out of P~ exceeds them"""
    case = C.keyw_case(n, H)
    assert torch.equal(case["qkv"], case["qkv"].bfloat16().float()) and bool((case["w"] >= 1).all())
    ref = TC.reference(n, H)
    fr = TC.fractions(TC.emulate(n, H), ref)
    bad = TC.fractions(TC.emulate(n, H, weighted=False), ref)
    print(f"emulated keyw backward n {n} H {H}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items())
          + " | without the weights " + " ".join(f"{k} {v:.1f}" for k, v in bad.items()))
    for k, v in fr.items():
        assert v <= 1.0, (k, n, H, v)
    for k, v in bad.items():
        assert v > 1.0, (k, n, H, v)


def test_the_package_still_imports_neither_the_oracle_nor_the_tests():
    pkg = os.path.join(REPO, "dense2sparse-vit_amd")
    pat = re.compile(r"^\s*(?:from|import)\s+(?:oracle|tests)\b", flags=re.M)
    seen = 0
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                assert not pat.search(open(os.path.join(root, f)).read()), os.path.join(root, f)
    assert seen > 10
