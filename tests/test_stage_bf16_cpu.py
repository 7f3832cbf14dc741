"""CPU tier of training ATS and A-ViT in the bf16 arithmetic mode (train_bf16=True / --ats-train-bf16, --avit-bf16; DESIGN.md sections 24
and 25): the closed header and its binding table, the command line, the constructor keywords, the _Ragged and AViTRun keywords, the
checkpoint key, and the texts that stay what they were."""
import inspect
import json
import os
import re
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_avit_halt_repack_bwd_bf16out", "d2s_ragged_repack_bwd_bf16out"]


# ---- the header and the binding (tests/test_abi_cpu.py compares the two entry by entry) ----
def test_header_declares_the_two_entries_and_the_older_tables_are_what_they_were():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ragged_stage_bf16.h")).read()
    assert NEW == lib.symbols("d2s_hip_ragged_stage_bf16.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    # the signatures: the fp32 row move's with the bf16 output behind g_old; the halting backward's with (g_new, keep, cu_new) in place
    # of g, the two outputs behind gsc and without `fresh`
    rp, hb = lib.signature("d2s_ragged_repack_bwd_bf16out"), lib.signature("d2s_avit_halt_repack_bwd_bf16out")
    plain = lib.signature("d2s_ragged_repack_bwd")[1]
    assert rp[0] is lib.I and rp[1] == plain[:5] + [lib.P] + plain[5:]
    halt = lib.signature("d2s_avit_halt_bwd")[1]
    assert hb[0] is lib.I and hb[1] == [lib.P] * 3 + halt[1:10] + [lib.P, lib.P] + halt[10:16] + halt[17:]
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "ragged_stage_bf16.hip")).read()
    for name in NEW:
        assert len(re.findall(rf"^int {name}\(", src, flags=re.M)) == 1, name
    assert "atomic" not in src.lower().replace("no atomics", "") and "memset" not in src.lower().replace("no memset", "")
    assert callable(ops.avit_halt_repack_bwd_bf16io) and inspect.signature(ops.ragged_repack_bwd).parameters["g16"].default is None
    assert list(inspect.signature(ops.ragged_repack_bwd).parameters)[:6] == ["g_new", "keep", "cu_old", "cu_new", "total_old", "B"]


# ---- command line ----
ATS = ["--method", "ats", "--pruning-locs", "3", "6", "--ats-train"]
AVIT = ["--method", "avit"]
PINNED_ATS = "--ats-train with --gemm-mode bf16 (training through a sampling stage is built on the fp32 data path; exact and split run)"
PINNED_AVIT = ("--method avit with --gemm-mode bf16 (training through a ragged block is built on the fp32 data path; exact and split run, "
               "--eval-only runs in all three)")


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_the_flags_and_reports_the_bf16_mode(capsys):
    import utils
    empty = vars(utils.parse_args([]))
    assert "ats_train_bf16" not in empty and "avit_bf16" not in empty            # the namespace of every other command line is what it was
    a = _check(ATS + ["--ats-train-bf16"])
    assert a.ats_train and a.ats_train_bf16 is True and a.gemm_mode == "exact"    # the flag, not --gemm-mode, selects the path
    out = capsys.readouterr().out
    assert "Attention: --ats-train-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    a = _check(AVIT + ["--avit-bf16"])
    assert a.avit_bf16 is True and a.gemm_mode == "exact"
    out = capsys.readouterr().out
    assert "Attention: --avit-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    _check(ATS + ["--ats-train-bf16", "--gemm-mode", "exact"])
    _check(AVIT + ["--avit-bf16", "--gemm-mode", "exact"])
    capsys.readouterr()
    _check(ATS)
    _check(AVIT)
    out = capsys.readouterr().out
    assert "--ats-train-bf16" not in out and "--avit-bf16" not in out             # without the flags: the lines that were there
    _check(AVIT + ["--gemm-mode", "bf16", "--eval-only", "--student-checkpoint", "w.pt"])      # evaluation in the bf16 mode runs as before


@pytest.mark.parametrize("argv,fragment", [
    (["--method", "ats", "--pruning-locs", "3", "--ats-train-bf16", "--eval-only", "--student-checkpoint", "w.pt"],
     "--ats-train-bf16 without --ats-train"),
    (["--ats-train-bf16"], "--ats-train-bf16 without --ats-train"),
    (ATS + ["--ats-train-bf16", "--gemm-mode", "split"], "--ats-train-bf16 with --gemm-mode split"),
    (ATS + ["--gemm-mode", "bf16"], PINNED_ATS),
    (ATS + ["--ats-train-bf16", "--gemm-mode", "bf16"], PINNED_ATS),
    (["--avit-bf16"], "--avit-bf16 with --method d2s"),
    (ATS + ["--avit-bf16"], "--avit-bf16 with --method ats"),
    (AVIT + ["--avit-bf16", "--eval-only", "--student-checkpoint", "w.pt"], "--avit-bf16 with --eval-only"),
    (AVIT + ["--avit-bf16", "--gemm-mode", "split"], "--avit-bf16 with --gemm-mode split"),
    (AVIT + ["--gemm-mode", "bf16"], PINNED_AVIT),
    (AVIT + ["--avit-bf16", "--gemm-mode", "bf16"], PINNED_AVIT),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_build_models_passes_the_keyword_only_under_the_flags(monkeypatch):
    import mask_predictor
    import vit_models
    seen = {}

    def ats_factory(**kw):
        seen["ats"] = kw
        return vit_models.VisionTransformerATS(**MICRO, **kw)

    def avit_factory(**kw):
        seen["avit"] = kw
        return vit_models.VisionTransformerAViT(**MICRO, **kw)
    monkeypatch.setattr(vit_models, "ats_deit_tiny_patch16_224", ats_factory)
    monkeypatch.setattr(vit_models, "avit_deit_tiny_patch16_224", avit_factory)
    base = dict(arch="deit_tiny", student_checkpoint=None, resume=None, teacher_checkpoint=None, dist_weight=0, device=torch.device("cpu"))
    ats = dict(base, method="ats", ats_train=True, pruning_locs=[1, 2], ats_tokens=[8])
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**ats))
    assert "train_bf16" not in seen["ats"] and m.train_bf16 is False and m.train_sample is True
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**ats, ats_train_bf16=True))
    assert seen["ats"]["train_bf16"] is True and m.train_bf16 is True and m.train_sample is True
    avit = dict(base, method="avit")
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**avit))
    assert "train_bf16" not in seen["avit"] and m.train_bf16 is False
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**avit, avit_bf16=True))
    assert seen["avit"]["train_bf16"] is True and m.train_bf16 is True


# ---- constructors, TrainStep, checkpoints ----
def test_constructor_keywords_and_their_refusals():
    import vit_models
    from vit_models import ats, avit
    p = inspect.signature(ats.VisionTransformerATS.__init__).parameters
    assert p["train_bf16"].default is False and list(p).index("train_bf16") == list(p).index("train_sample") + 1
    p = inspect.signature(avit.VisionTransformerAViT.__init__).parameters
    assert p["train_bf16"].default is False and list(p).index("train_bf16") == list(p).index("target_depth") + 1
    on = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], ats_tokens=4, train_sample=True, train_bf16=True)
    off = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], ats_tokens=4, train_sample=True)
    assert on.train_bf16 is True and off.train_bf16 is False and list(on.state_dict()) == list(off.state_dict())
    von, voff = vit_models.VisionTransformerAViT(**MICRO, train_bf16=True), vit_models.VisionTransformerAViT(**MICRO)
    assert von.train_bf16 is True and voff.train_bf16 is False and list(von.state_dict()) == list(voff.state_dict())
    with pytest.raises(ValueError, match="train_bf16 without train_sample"):
        vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], ats_tokens=4, train_bf16=True)
    for factory in (vit_models.ats_deit_tiny_patch16_224, vit_models.ats_deit_small_patch16_224, vit_models.ats_deit_base_patch16_224):
        with pytest.raises(ValueError, match="train_bf16 without train_sample"):   # the three factories hand the keyword through
            factory([3], 8, train_bf16=True)
    assert vit_models.ats_deit_tiny_patch16_224([3], 8, train_sample=True, train_bf16=True).train_bf16 is True
    for factory in (vit_models.avit_deit_tiny_patch16_224, vit_models.avit_deit_small_patch16_224, vit_models.avit_deit_base_patch16_224):
        with pytest.raises(ValueError, match="eps_halt"):                          # ... and so do A-ViT's, in front of the older check
            factory(train_bf16=True, eps_halt=2.0)
    assert vit_models.avit_deit_tiny_patch16_224(train_bf16=True).train_bf16 is True


def _students():
    import vit_models
    ats = lambda **kw: vit_models.VisionTransformerATS(**MICRO, ats_locs=[1, 2], ats_tokens=[8, 4], train_sample=True, **kw)
    avit = lambda **kw: vit_models.VisionTransformerAViT(**MICRO, **kw)
    return (("an Adaptive Token Sampling student", ats), ("an A-ViT student", avit))


def test_train_step_config_key_and_the_refusals_that_stay():
    from d2s import engine, lib
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=types.SimpleNamespace(mask_loss_type="kl_div")))
    for title, make in _students():
        a, b = cfg(make(train_bf16=True)), cfg(make())
        # the key is recorded where it is on; without it - the default, every older checkpoint - it counts as off
        assert a["train_bf16"] is True and "train_bf16" not in b and b.get("train_bf16", False) is False
        assert {k: v for k, v in a.items() if k != "train_bf16"} == b and list(a)[:-1] == list(b)
        assert json.loads(json.dumps(a)) == a
        assert engine.checkpoint_config(b).get("train_bf16", False) is False and engine.checkpoint_config(a)["train_bf16"] is True
        args = types.SimpleNamespace(mixup=0.0)
        with pytest.raises(lib.D2SError, match=rf"TrainStep\(graph=True\) with {title}"):
            engine.TrainStep(make(train_bf16=True), None, args, graph=True)
        with pytest.raises(ValueError, match=f"warmup_steps 2 with {title}"):
            engine.TrainStep(make(train_bf16=True), None, args, warmup_steps=2)
        m = make(train_bf16=True)
        m.drop_path_rate = 0.1
        with pytest.raises(lib.D2SError, match="drop_path_rate > 0"):
            engine.TrainStep(m, None, args)


def test_pinned_texts_are_the_parents():
    import methods
    from d2s import functional_ats as AF
    assert AF._BF16_REFUSAL == ("training through a ragged block runs in the fp32 arithmetic modes (exact, split): the varlen attention "
                                "backward is an fp32 kernel")
    assert AF._BF16_STAGE_REFUSAL == (AF._BF16_REFUSAL + ".  A block with a sampling stage stays there with bf16=True too: behind the hook "
                                      "between the halves (sample_bwd) the bf16 shadow of the gradient would have to be made again")
    assert AF._BF16_MODE_REFUSAL == "a ragged block with bf16=True runs in the bf16 arithmetic mode only (ops.gemm_mode(GEMM_BF16))"
    assert methods.by_name("ats").cli_bf16 == ("training through a sampling stage is built on the fp32 data path; exact and split run", False)
    assert methods.by_name("avit").cli_bf16 == ("training through a ragged block is built on the fp32 data path; exact and split run, "
                                                "--eval-only runs in all three", True)
    assert methods.by_name("ats").bf16_refusal is None and methods.by_name("avit").bf16_refusal is None


def test_ragged_and_run_keywords():
    from d2s import functional_ats as AF
    from d2s import functional_avit as VF
    from d2s import lib
    p = inspect.signature(AF._Ragged.__init__).parameters
    assert list(p)[-2:] == ["bf16", "stage_bf16"] and p["stage_bf16"].default is False and p["bf16"].default is False
    cu = torch.tensor([0, 3], dtype=torch.int32)
    assert AF._Ragged(cu, 1, 3, 2, 0.125, None, 2, 4, None).K == 2                # the positional layout of the existing callers
    r = AF._Ragged(cu, 1, 3, 2, 0.125, None, 2, 4, None, bf16=True, stage_bf16=True)
    assert r.bf16 is True and r.stage_bf16 is True and AF._Ragged(cu, 1, 3, 2, 0.125, bf16=True).stage_bf16 is False
    assert callable(r.sample_bwd_bf16) and list(inspect.signature(r.sample_bwd_bf16).parameters) == ["g1", "g1h"]
    # stage_bf16 without bf16 is refused before anything touches a device, in every arithmetic mode
    x = torch.zeros((3, 128), requires_grad=True)
    params = [torch.zeros(1)] * 12
    with pytest.raises(lib.D2SError, match="stage_bf16=True needs bf16=True"):
        AF.ragged_block_train(x, params, 1e-6, AF._Ragged(cu, 1, 3, 2, 0.125, None, 2, 4, None, stage_bf16=True))
    with pytest.raises(lib.D2SError, match="stage_bf16=True needs bf16=True"):
        AF.ragged_block_train(x, params, 1e-6, AF._Ragged(cu, 1, 3, 2, 0.125, stage_bf16=True))
    p = inspect.signature(VF.AViTRun.__init__).parameters
    assert list(p)[-1] == "bf16" and p["bf16"].default is False and list(p)[1:9] == ["B", "N", "D", "L", "gamma", "beta", "eps_halt", "device"]
