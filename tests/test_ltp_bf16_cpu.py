"""CPU tier of LTP in the bf16 arithmetic mode (train_bf16=True / --ltp-bf16; DESIGN.md section 27, "In the bf16 arithmetic mode"): the
closed header and its binding table, the command line, the constructor keyword and the factories, TrainStep's config key and the refusals
that stay, and the float64 restatement of the score on the bf16-rounded operands (tests/ltp_bf16_ref.py)."""
import inspect
import json
import os
import re
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import ltp_bf16_ref as RB
from tests import ltp_ref as R
from tests.test_ltp_cpu import MICRO, SCALE, make_policy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["d2s_ltp_score_bf16", "d2s_ltp_score_bf16_workspace_bytes"]


# ---- the header and the binding (tests/test_abi_cpu.py compares the two entry by entry) ----
def test_header_declares_the_two_entries_and_the_older_tables_are_what_they_were():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ltp_bf16.h")).read()
    assert NEW == lib.symbols("d2s_hip_ltp_bf16.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    # the signatures: the fp32 score pair's
    assert lib.signature("d2s_ltp_score_bf16") == lib.signature("d2s_ltp_score_f32")
    assert lib.signature("d2s_ltp_score_bf16_workspace_bytes") == lib.signature("d2s_ltp_score_workspace_bytes")
    assert lib.query("d2s_ltp_score_bf16_workspace_bytes", 197 * 128, 6) == 197 * 128 * 6 * 4
    assert lib.query("d2s_ltp_score_bf16_workspace_bytes", 0, 6) == 0 and lib.query("d2s_ltp_score_bf16_workspace_bytes", 5, 0) == 0
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "ltp_bf16.hip")).read()
    for name in NEW:
        assert len(re.findall(rf"^(?:int|size_t) {name}\(", src, flags=re.M)) == 1, name
    assert "atomic" not in src.lower().replace("no atomics", "") and "memset" not in src.lower().replace("no memset", "")
    assert "v_mfma_f32_32x32x16_bf16" in src and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in src
    p = inspect.signature(ops.ltp_score).parameters                               # one wrapper, dispatching on qkv's dtype
    assert list(p) == ["qkv", "lse", "B", "n", "H", "scale", "policy", "cinv", "cu", "total"]
    mk = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "Makefile")).read()
    assert "resources-%: %.hip" in mk and "ltp_bf16 (27)" in mk                   # `make resources-ltp_bf16` reports the kernels' registers


# ---- command line ----
LTP = ["--method", "ltp", "--pruning-locs", "3", "6", "9"]
PINNED = ("--method ltp with --gemm-mode bf16 (the score is recomputed from the fp32 attention's log-sum-exp, and both phases train on the "
          "fp32 data path; exact and split run)")


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_the_flag_in_every_phase_and_names_the_data_path(capsys):
    import utils
    assert "ltp_bf16" not in vars(utils.parse_args([]))                           # the namespace of every other command line is what it was
    for extra in (["--student-checkpoint", "w.pt"], ["--ltp-phase", "hard", "--dist-weight", "0"],
                  ["--eval-only", "--student-checkpoint", "w.pt"], ["--gemm-mode", "exact"]):
        a = _check(LTP + ["--ltp-bf16"] + extra)
        assert a.ltp_bf16 is True and a.gemm_mode == "exact"                      # the flag, not --gemm-mode, selects the path
        out = capsys.readouterr().out
        assert "Attention: --ltp-bf16: every phase and the evaluation run in the bf16 arithmetic mode on the bf16 data path" in out
    _check(LTP)
    assert "--ltp-bf16" not in capsys.readouterr().out                            # without the flag: the lines that were there


@pytest.mark.parametrize("argv,fragment", [
    (["--ltp-bf16"], "--ltp-bf16 with --method d2s"),
    (["--method", "avit", "--ltp-bf16"], "--ltp-bf16 with --method avit"),
    (["--method", "dynamicvit", "--ltp-bf16"], "--ltp-bf16 with --method dynamicvit"),
    (LTP + ["--ltp-bf16", "--gemm-mode", "split"], "--ltp-bf16 with --gemm-mode split"),
    (LTP + ["--gemm-mode", "bf16"], PINNED),
    (LTP + ["--ltp-bf16", "--gemm-mode", "bf16"], PINNED),
    (LTP + ["--eval-only", "--student-checkpoint", "w.pt", "--gemm-mode", "bf16"], PINNED),
    (LTP + ["--ltp-bf16", "--eval-only", "--student-checkpoint", "w.pt", "--gemm-mode", "bf16"], PINNED),
    (LTP + ["--ltp-bf16", "--drop-path", "0.1"], "--method ltp with --drop-path 0.1"),
    (LTP + ["--ltp-bf16", "--warmup-steps", "3"], "--method ltp with --warmup-steps 3"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_the_pinned_refusal_is_the_same_text_with_and_without_the_flag():
    texts = []
    for flag in ([], ["--ltp-bf16"]):
        with pytest.raises(SystemExit) as e:
            _check(LTP + flag + ["--gemm-mode", "bf16"])
        texts.append(str(e.value))
    assert texts[0] == texts[1] and PINNED in texts[0]


def test_build_models_passes_the_keyword_only_under_the_flag(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(checkpoint_path=None, **kw):
        seen["kw"] = kw
        return vit_models.VisionTransformerLTP(**MICRO, **kw)
    monkeypatch.setattr(vit_models, "ltp_deit_tiny_patch16_224", factory)
    base = dict(arch="deit_tiny", method="ltp", student_checkpoint=None, resume=None, teacher_checkpoint=None, dist_weight=0.0,
                device=torch.device("cpu"), pruning_locs=[0, 2])
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**base))
    assert "train_bf16" not in seen["kw"] and m.train_bf16 is False
    m, _ = mask_predictor.build_models(types.SimpleNamespace(**base, ltp_bf16=True, ltp_phase="hard"))
    assert seen["kw"]["train_bf16"] is True and m.train_bf16 is True and m.ltp_phase == "hard"
    capsys.readouterr()
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "mask_predictor.py")).read()
    assert re.search(r'own_bf16 = any\(.*"ltp_bf16"', src)                        # the flag sets the bf16 arithmetic mode itself


# ---- constructor, factories, TrainStep, checkpoints ----
def test_constructor_keyword_and_factories():
    import vit_models
    from vit_models import ltp
    p = inspect.signature(ltp.VisionTransformerLTP.__init__).parameters
    assert p["train_bf16"].default is False and list(p).index("train_bf16") == list(p).index("ltp_phase") + 1
    on = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1], train_bf16=True)
    off = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1])
    assert on.train_bf16 is True and off.train_bf16 is False and list(on.state_dict()) == list(off.state_dict())
    for factory in (vit_models.ltp_deit_tiny_patch16_224, vit_models.ltp_deit_small_patch16_224, vit_models.ltp_deit_base_patch16_224):
        with pytest.raises(ValueError, match="ltp_temperature"):                   # the three factories hand the keyword through
            factory(train_bf16=True, ltp_temperature=0.0)
    assert vit_models.ltp_deit_tiny_patch16_224(train_bf16=True).train_bf16 is True
    assert vit_models.ltp_deit_tiny_patch16_224().train_bf16 is False


def test_ragged_and_block_keywords():
    from d2s import functional_ats as AF
    from d2s import functional_ltp as LF
    from d2s import lib
    p = inspect.signature(LF._RaggedLTP.__init__).parameters
    assert list(p)[-2:] == ["plan", "bf16"] and p["bf16"].default is False and p["plan"].default is None
    cu = torch.tensor([0, 3], dtype=torch.int32)
    th = torch.zeros(1)
    r = LF._RaggedLTP(cu, 1, 3, 2, 0.125, None, th, 2)
    assert (r.bf16, r.stage_bf16, r.K, r.T) == (False, False, 2, 2)
    r = LF._RaggedLTP(cu, 1, 3, 2, 0.125, None, th, 2, None, bf16=True)
    assert (r.bf16, r.stage_bf16, r.K, r.T) == (True, True, 2, 2) and callable(r.sample_bwd_bf16)
    assert inspect.signature(LF.soft_block).parameters["bf16"].default is False
    assert list(inspect.signature(LF.soft_block).parameters)[-1] == "bf16"
    # a stage with bf16=True outside the bf16 mode is refused before anything touches a device, with the ragged block's text
    x = torch.zeros((3, 128), requires_grad=True)
    with pytest.raises(lib.D2SError) as e:
        LF.stage_block(x, [torch.zeros(1)] * 12, 1e-6, r)
    assert str(e.value) == AF._BF16_MODE_REFUSAL


def _cfg(s):
    from d2s import engine
    return engine.TrainStep.config(types.SimpleNamespace(student=s, args=types.SimpleNamespace(mask_loss_type="kl_div")))


def test_train_step_config_key_and_the_refusals_that_stay():
    import vit_models
    from d2s import engine, lib, ops
    make = lambda **kw: vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1], **kw)
    a, b = _cfg(make(train_bf16=True)), _cfg(make())
    # the key is recorded where it is on; without it - the default, every older checkpoint - it counts as off
    assert a["train_bf16"] is True and "train_bf16" not in b and b.get("train_bf16", False) is False
    assert {k: v for k, v in a.items() if k != "train_bf16"} == b and list(a)[:-1] == list(b)
    assert json.loads(json.dumps(a)) == a
    assert engine.checkpoint_config(b).get("train_bf16", False) is False and engine.checkpoint_config(a)["train_bf16"] is True
    args = types.SimpleNamespace(mixup=0.0)
    with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an LTP student"):
        engine.TrainStep(make(train_bf16=True), None, args, graph=True)
    with pytest.raises(ValueError, match="warmup_steps 2 with an LTP student"):
        engine.TrainStep(make(train_bf16=True), None, args, warmup_steps=2)
    m = make(train_bf16=True)
    m.drop_path_rate = 0.1
    with pytest.raises(lib.D2SError, match="drop_path_rate > 0"):
        engine.TrainStep(m, None, args)
    # a default-built student in the bf16 mode: the old refusals with the old text, from TrainStep and from the model
    from d2s.functional_ltp import BF16_REFUSAL
    assert BF16_REFUSAL == ("LTP runs in the fp32 arithmetic modes (exact, split): the score is recomputed from the fp32 attention's "
                            "log-sum-exp and training through a ragged or a policy block with a learnt policy is built on the fp32 data path")
    with ops.gemm_mode(ops.GEMM_BF16):
        for phase in ("soft", "hard"):
            with pytest.raises(lib.D2SError) as e:
                engine.TrainStep(make(ltp_phase=phase), None, args)
            assert str(e.value) == "TrainStep with an LTP student in the bf16 arithmetic mode: " + BF16_REFUSAL
        for m in (make().eval(), make().train(), make(ltp_phase="hard").train()):
            with pytest.raises(lib.D2SError) as e:
                m(torch.zeros(1, 3, 64, 64))
            assert str(e.value) == BF16_REFUSAL


def test_checkpoint_mismatch_of_the_key_is_refused_both_ways():
    """TrainStep.load_state_dict's two checks on the key, stated on the configs (the GPU tier loads real checkpoints)"""
    import vit_models
    make = lambda **kw: vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1], **kw)
    on, off = _cfg(make(train_bf16=True)), _cfg(make())
    assert any(k not in off or off[k] != on[k] for k in on)                        # this run on, the checkpoint off: the loop over `ours`
    assert bool(on.get("train_bf16", False)) and not off.get("train_bf16", False)  # the checkpoint on, this run off: the explicit check
    import methods
    m = methods.by_name("ltp")
    assert m.bf16_refusal is not None and m.cli_bf16[1] is False and m.no_graph   # methods.py keeps every field value


# ---- the float64 restatement on the bf16-rounded operands ----
def test_operands_are_rounded_as_the_kernel_rounds_them():
    qkv = RB.make_qkv(7, 2, 3)
    assert torch.equal(qkv.float().bfloat16().double(), qkv)                       # on the bf16 grid
    for scale in (0.125, 0.11):
        q, ks = RB.round_operands(qkv, scale)
        assert torch.equal(q, qkv[:, 0])
        want = (qkv[:, 1].float() * torch.tensor(scale, dtype=torch.float32)).bfloat16().double()
        assert torch.equal(ks, want) and torch.equal(ks.float().bfloat16().double(), ks)
    _, ks = RB.round_operands(qkv, 0.125)
    assert torch.equal(ks, qkv[:, 1] * 0.125)                                      # a power of two: the scaling is exact
    _, ks = RB.round_operands(qkv, 0.11)
    assert not torch.equal(ks, qkv[:, 1] * 0.11)                                   # otherwise the rounding is visible
    with pytest.raises(AssertionError, match="bf16 grid"):
        RB.round_operands(qkv + 1e-5, 0.125)


@pytest.mark.parametrize("scale", [0.125, 0.11])
@pytest.mark.parametrize("B,n,H", [(1, 2, 1), (3, 33, 2), (2, 65, 6)])
def test_every_images_scores_sum_to_one_in_the_three_forms(B, n, H, scale):
    qkv = RB.make_qkv(B * n, H, 7 * n + H)
    one = torch.ones(B, dtype=torch.float64)
    plain = RB.score_plain(qkv, B, n, H, scale)
    assert torch.allclose(plain.sum(dim=1), one, rtol=1e-12, atol=0)
    for kind in ("ones", "mixed", "cls_only"):
        for eps in (0.0, 1e-6):
            s = RB.score_policy(qkv, make_policy(kind, B, n, n), B, n, H, scale, eps)
            assert torch.allclose(s.sum(dim=1), one, rtol=1e-12, atol=0), (kind, eps)
    assert torch.allclose(RB.score_policy(qkv, make_policy("ones", B, n, 0), B, n, H, scale, 0.0), plain, rtol=1e-13, atol=0)
    v = RB.score_varlen(qkv, [n] * B, H, scale)
    assert torch.equal(v, plain.reshape(-1))
    lens = [1, 2, n]
    s = RB.score_varlen(RB.make_qkv(sum(lens), H, 5), lens, H, scale)
    assert float(s[0]) == 1.0 and abs(float(s[1:3].sum()) - 1.0) < 1e-12 and abs(float(s[3:].sum()) - 1.0) < 1e-12


@pytest.mark.parametrize("B,n,H", [(1, 2, 1), (3, 33, 2), (2, 65, 6)])
def test_at_a_power_of_two_scale_the_restatement_is_ltp_refs_on_the_same_inputs(B, n, H):
    """scale = 2^-3: bf16(fp32(k) * scale) = k * scale exactly, so the rounded operands are ltp_ref's operands"""
    qkv = RB.make_qkv(B * n, H, 11 * n + H)
    assert torch.allclose(RB.score_plain(qkv, B, n, H, SCALE), R.score_plain(qkv, B, n, H, SCALE), rtol=1e-12, atol=0)
    pol = make_policy("mixed", B, n, n + 1)
    assert torch.allclose(RB.score_policy(qkv, pol, B, n, H, SCALE, 1e-6), R.score_policy(qkv, pol, B, n, H, SCALE, 1e-6), rtol=1e-12, atol=0)
    lens = [n] * (B - 1) + [1, 2]
    q2 = RB.make_qkv(sum(lens), H, 13)
    assert torch.allclose(RB.score_varlen(q2, lens, H, SCALE), R.score_varlen(q2, lens, H, SCALE), rtol=1e-12, atol=0)
    # and the statistics handed in are the statistics used: the restatement's own lse gives its own score
    lse = RB.stats_varlen(q2, lens, H, SCALE)
    assert torch.equal(RB.score_varlen(q2, lens, H, SCALE, lse=lse), RB.score_varlen(q2, lens, H, SCALE))
