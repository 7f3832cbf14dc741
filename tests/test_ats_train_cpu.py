"""Training through adaptive token sampling (--method ats --ats-train), the parts that need no GPU: the closed-form
backward of the re-pack and of the CLS gather of tests/ats_train_ref.py against torch autograd, the restated varlen attention against
dense attention, the batch the GPU test trains on shown to be ragged, the fifth header and binding table, the command line, build_models,
the constructor and TrainStep's refusals, and the checkpoint config."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import ats_ref as R
from tests import ats_train_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_attn_varlen_bwd_f32", "d2s_attn_varlen_fwd_lse_f32", "d2s_ragged_cls_scatter", "d2s_ragged_repack_bwd"]

# the truly ragged training batch (tests/test_ats_train_gpu.py trains on it): test_ats_gpu.py's construction
RAGGED = dict(name="micro1", locs=[1, 2, 3], K=16, factors=(2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0))
_RAGGED = {}


def sharpened(name, factor):
    """The case's teacher state dict with the query and key rows of every block's qkv scaled: attention logits grow by factor ** 2"""
    case = cases.MODEL_CASES[name]
    D = case["cfg"]["dim"]
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)).clone() for k, v in cases.make_weights(case)[1].items()}
    for k in sd:
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            sd[k][:2 * D] *= factor
    return sd


def ragged_case():
    """(state dict, images, factor, the reference's token counts after the last stage): the first factor at which the float64 reference,
    selecting by its own scores, ends with more than one distinct count.  Built once."""
    if not _RAGGED:
        case = cases.MODEL_CASES[RAGGED["name"]]
        images = torch.from_numpy(cases.make_images(case))
        for factor in RAGGED["factors"]:
            sd = sharpened(RAGGED["name"], factor)
            _, used = R.model_forward(sd, images, case["cfg"], RAGGED["locs"], tokens=[RAGGED["K"]] * len(RAGGED["locs"]))
            counts = [len(ids) - 1 for ids in used[-1]]
            if len(set(counts)) > 1:
                break
        _RAGGED.update(sd=sd, images=images, factor=factor, counts=counts)
    return _RAGGED["sd"], _RAGGED["images"], _RAGGED["factor"], _RAGGED["counts"]


def test_the_ragged_training_batch_is_ragged():
    _, _, factor, counts = ragged_case()
    print(f"factor {factor}: reference token counts after the last stage {counts}")
    assert len(set(counts)) > 1, "no factor made the reference ragged"


# ---- the two row moves ----
FLAGS = {"mixed": lambda g, n: (torch.rand(n, generator=g) < 0.5).float(), "all": lambda g, n: torch.ones(n), "none": lambda g, n: torch.zeros(n)}


@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("lens", [(17, 5, 2), (1, 9, 1), (300, 70)], ids=str)
def test_closed_form_repack_backward_equals_autograd(lens, flags):
    g = torch.Generator().manual_seed(31 + sum(lens))
    total, D = sum(lens), 8
    cu = [0] + list(np.cumsum(lens))
    keep = FLAGS[flags](g, total)
    x = torch.randn((total, D), generator=g, dtype=torch.float64, requires_grad=True)
    out, cu_new, idx = T.repack(x, keep, cu)
    assert cu_new[-1] == out.shape[0] and all(int(idx[cu_new[b]]) == cu[b] for b in range(len(lens)))      # CLS first, always kept
    if flags == "all":
        assert torch.equal(out, x.detach())
    if flags == "none":
        assert out.shape[0] == len(lens)
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(out, x, gy)
    got = T.repack_backward(gy.numpy(), keep.numpy(), cu, cu_new)
    assert np.array_equal(got, want.numpy())
    # the adjoint identity <g_old, x> = <g_new, repack(x)>
    assert float((torch.from_numpy(got) * x.detach()).sum()) == pytest.approx(float((gy * out.detach()).sum()), rel=1e-12)


@pytest.mark.parametrize("lens", [(17, 5, 2), (1, 9, 1), (4,)], ids=str)
def test_closed_form_cls_scatter_equals_autograd(lens):
    g = torch.Generator().manual_seed(5 + sum(lens))
    total, D = sum(lens), 8
    cu = torch.tensor([0] + list(np.cumsum(lens)))
    x = torch.randn((total, D), generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn((len(lens), D), generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(x[cu[:-1]], x, gy)
    got = T.cls_scatter(gy.numpy(), cu.tolist(), total)
    assert np.array_equal(got, want.numpy())
    assert int((got != 0).any(axis=1).sum()) == len(lens)


def test_restated_varlen_attention_is_dense_attention_per_image():
    g = torch.Generator().manual_seed(9)
    lens, H = (7, 1, 4), 2
    cu = [0] + list(np.cumsum(lens))
    qkv = torch.randn((sum(lens), 3 * H * 64), generator=g, dtype=torch.float64)
    dout = torch.randn((sum(lens), H * 64), generator=g, dtype=torch.float64)
    out, lse, cls_row = T.varlen_attention(qkv, cu, H, 0.125)
    dq = T.varlen_attention_grad(qkv, cu, H, 0.125, dout)
    for b, n in enumerate(lens):
        lo, hi = cu[b], cu[b + 1]
        q = qkv[lo:hi].reshape(1, n, 3, H, 64).clone().requires_grad_(True)
        qq, kk, vv = (q[:, :, i].transpose(1, 2) for i in range(3))
        P = torch.softmax((qq @ kk.transpose(-1, -2)) * 0.125, dim=-1)
        want = (P @ vv).transpose(1, 2).reshape(n, H * 64)
        torch.testing.assert_close(out[lo:hi], want.detach(), rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(cls_row[:, lo:hi], P[0, :, 0].detach(), rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(lse[:, lo:hi].exp(), torch.exp((qq @ kk.transpose(-1, -2)) * 0.125).sum(-1)[0].detach(), rtol=1e-12, atol=0)
        want.backward(dout[lo:hi])
        torch.testing.assert_close(dq[lo:hi], q.grad.reshape(n, -1), rtol=1e-12, atol=1e-13)
    one = slice(cu[1], cu[2])                                               # a one-row image: softmax of one score, out = v, dq = dk = 0, dv = dout
    assert torch.equal(out[one], qkv[one, 2 * H * 64:]) and float(dq[one, :2 * H * 64].abs().max()) == 0.0
    assert torch.equal(dq[one, 2 * H * 64:], dout[one])


# ---- header and binding ----
def test_ragged_train_header_and_binding_tables():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ragged_train.h")).read()
    assert NEW == lib.symbols("d2s_hip_ragged_train.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) >= 1 + len(NEW)               # the file's own comment and one per entry
    for fn in ("attn_varlen_fwd_lse", "attn_varlen_bwd", "ragged_repack_bwd", "ragged_cls_scatter"):
        assert callable(getattr(ops, fn))
    from d2s import functional_ats
    assert callable(functional_ats.RaggedBlockFn.apply) and callable(functional_ats.ats_block_forward)


# ---- command line ----
TRAIN = ["--method", "ats", "--ats-train"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_ats_train():
    import utils
    assert utils.parse_args([]).ats_train is False and utils.parse_args([]).warmup_steps == 5
    for mode in ("exact", "split"):
        a = _check(TRAIN + ["--pruning-locs", "3", "6", "9", "--ats-tokens", "64", "--student-checkpoint", "w.pt", "--gemm-mode", mode])
        assert a.ats_train and a.method == "ats" and not a.eval_only and a.warmup_steps == 0 and a.ats_tokens == [64]
    assert _check(TRAIN + ["--warmup-steps", "0"]).warmup_steps == 0
    assert _check(TRAIN + ["--dist-weight", "0"]).dist_weight == 0
    assert _check(["--warmup-steps", "5"]).warmup_steps == 5                         # the other methods keep their warm-up


@pytest.mark.parametrize("argv,fragment", [
    (["--method", "ats", "--student-checkpoint", "w.pt"], "--method ats without --eval-only"),                 # untouched
    (["--ats-train"], "--ats-train with --method d2s"),
    (["--ats-train", "--method", "dynamicvit"], "--ats-train with --method dynamicvit"),
    (["--ats-train", "--method", "tome", "--tome-r", "2", "--tome-train"], "--ats-train with --method tome"),
    (TRAIN + ["--eval-only", "--student-checkpoint", "w.pt"], "--ats-train with --eval-only"),
    (TRAIN + ["--gemm-mode", "bf16"], "--ats-train with --gemm-mode bf16"),
    (TRAIN + ["--drop-path", "0.1"], "--ats-train with --drop-path 0.1"),
    (TRAIN + ["--torch-optim"], "--ats-train with --torch-optim"),
    (TRAIN + ["--warmup-steps", "3"], "--ats-train with --warmup-steps 3"),
    (TRAIN + ["--warmup-steps", "5"], "--ats-train with --warmup-steps 5"),
    (TRAIN + ["--topk-selection"], "--method ats with --topk-selection"),
    (TRAIN + ["--pruning-locs", "3", "6", "9", "--ats-tokens", "64", "32"], "--ats-tokens with 2 values for 3 stages"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_the_inference_refusal_keeps_its_text():
    with pytest.raises(SystemExit) as e:
        _check(["--method", "ats", "--student-checkpoint", "w.pt"])
    assert "--method ats without --eval-only (adaptive token sampling is built for inference: a sampling stage has no backward)" in str(e.value)


def test_build_models_passes_train_sample_only_under_the_flag(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(ats_locs=(), ats_tokens=None, checkpoint_path=None, **kw):
        seen.update(ats_locs=ats_locs, ats_tokens=ats_tokens, kw=kw)
        return vit_models.VisionTransformerATS(ats_locs=ats_locs, ats_tokens=ats_tokens, **MICRO, **kw)

    def teacher_factory(checkpoint_path=None):
        seen["teacher_checkpoint"] = checkpoint_path
        return vit_models.VisionTransformerTeacher(**MICRO)
    monkeypatch.setattr(vit_models, "ats_deit_tiny_patch16_224", factory)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_teacher", teacher_factory)
    base = dict(arch="deit_tiny", method="ats", pruning_locs=[1, 3], ats_tokens=[8, 4], student_checkpoint=None, resume=None,
                teacher_checkpoint=None, device=torch.device("cpu"))
    for off in (dict(), dict(ats_train=False, dist_weight=0.5)):
        student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, **off))
        assert teacher is None and seen["kw"] == {} and student.train_sample is False
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, ats_train=True, dist_weight=0.5))
    assert seen["kw"] == {"train_sample": True} and student.train_sample is True and student.ats_locs == [1, 3] and student.ats_tokens == [8, 4]
    assert isinstance(teacher, vit_models.VisionTransformerTeacher) and "teacher_checkpoint" in seen
    seen.pop("teacher_checkpoint")
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, ats_train=True, dist_weight=0.0))
    assert teacher is None and student.train_sample is True and "teacher_checkpoint" not in seen          # --dist-weight 0: no teacher is built


# ---- constructor, TrainStep ----
def test_constructor_opt_in_and_the_pinned_refusal():
    import vit_models
    from vit_models import ats
    from d2s import ops
    m = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1, 2], ats_tokens=4, train_sample=True)
    assert m.train_sample and m.grad_ready_hook is None
    assert list(m.state_dict()) == list(vit_models.VisionTransformerTeacher(**MICRO).state_dict())
    assert vit_models.ats_deit_tiny_patch16_224((3,), 8, train_sample=True).train_sample
    assert not vit_models.ats_deit_small_patch16_224((3,), 8).train_sample and not vit_models.VisionTransformerATS(**MICRO).train_sample
    with pytest.raises(ValueError, match="drop_path_rate"):
        vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], train_sample=True, drop_path_rate=0.1)
    d = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1]).train()            # the default still refuses, with the pinned text
    with pytest.raises(NotImplementedError) as e:
        d(torch.zeros(1, 3, 64, 64))
    assert str(e.value) == ats.ATS_TRAINING_ERROR
    with ops.gemm_mode(ops.GEMM_BF16):                                            # before any launch: nothing here is on a device
        with pytest.raises(NotImplementedError, match="bf16 arithmetic mode"):
            m.train()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="plans"):
        m.train()(torch.zeros(1, 3, 64, 64), plans=[None])


def test_train_step_refusals_come_before_the_device():
    import vit_models
    from d2s import lib
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    m = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1, 2], ats_tokens=4, train_sample=True)
    with pytest.raises(lib.D2SError, match="graph=True.*Adaptive Token Sampling"):
        TrainStep(m, None, args, graph=True)
    with pytest.raises(ValueError, match="warmup_steps 1 with an Adaptive Token Sampling student"):
        TrainStep(m, None, args, warmup_steps=1)
    with pytest.raises(lib.D2SError, match="train_sample=True"):
        TrainStep(vit_models.VisionTransformerATS(**MICRO, ats_locs=[1]), None, args)
    dp = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], train_sample=True)
    dp.drop_path_rate = 0.1                                                       # the constructor refuses it; a model altered afterwards
    with pytest.raises(lib.D2SError, match="drop_path_rate > 0"):
        TrainStep(dp, None, args)
    # the messages the other students reach are what they were
    with pytest.raises(lib.D2SError) as e:
        TrainStep(vit_models.VisionTransformerTeacher(**MICRO), None, args)
    assert str(e.value) == "TrainStep without a teacher: only a Token Merging student trains without one"
    with pytest.raises(lib.D2SError) as e:
        TrainStep(vit_models.VisionTransformerATS(**MICRO), None, args)           # no stage: the dense trunk, where it was
    assert str(e.value) == "TrainStep without a teacher: only a Token Merging student trains without one"
    with pytest.raises(lib.D2SError, match="TrainStep with a merging VisionTransformerToMe needs train_merge=True"):
        TrainStep(vit_models.VisionTransformerToMe(**MICRO, tome_r=2), None, args)


# ---- checkpoints ----
def test_checkpoint_config_records_the_sampling_student():
    import vit_models
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    a = cfg(vit_models.VisionTransformerATS(**MICRO, ats_locs=[1, 3], ats_tokens=[8, 4], train_sample=True))
    b = cfg(vit_models.VisionTransformerATS(**MICRO, ats_locs=[2], ats_tokens=5))
    c = cfg(vit_models.VisionTransformerTeacher(**MICRO))
    assert (a["ats_locs"], a["ats_tokens"], a["train_sample"]) == ([1, 3], [8, 4], True) and a["model"] == "VisionTransformerATS"
    assert (b["ats_locs"], b["ats_tokens"], b["train_sample"]) == ([2], [5], False)
    assert (c["ats_locs"], c["ats_tokens"], c["train_sample"]) == ([], [], False)
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in a.items() if k not in ("ats_locs", "ats_tokens", "train_sample")}
    filled = engine.checkpoint_config(old)
    assert (filled["ats_locs"], filled["ats_tokens"], filled["train_sample"]) == ([], [], False) and "ats_locs" not in old
    assert engine.checkpoint_config(a) == a
