"""Training through token merging (--method tome --tome-train), the parts that need no GPU: the closed-form merge
backward of tests/tome_train_ref.py against autograd through tests/tome_ref.py's merge and through the literal transcription of the
published merge_wavg, the restated block's pieces against tome_ref, the objective against torch's losses, the command line, the
constructor and TrainStep's refusals, the checkpoint config, and the library binding."""
import json
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import tome_ref as R
from tests import tome_train_ref as T
from tests.test_tome_cpu import MICRO, published_bipartite_soft_matching, published_merge_wavg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 9, 3, 2), (2, 10, 2, 4), (3, 65, 3, 16), (2, 66, 1, 32), (2, 197, 6, 13), (2, 17, 2, 100)]      # tests/test_tome_cpu.py's six


# ---- merge backward ----
@pytest.mark.parametrize("B,n,H,r", SHAPES)
def test_closed_form_merge_backward_equals_autograd(B, n, H, r):
    gen = torch.Generator().manual_seed(177 + n)
    qkv = torch.randn((B, n, 3, H, 64), generator=gen)
    x = torch.randn((B, n, 32), generator=gen, dtype=torch.float64)
    size = torch.randint(1, 6, (B, n), generator=gen).double()
    plan = R.match(qkv, r)[2:]
    re_ = R.clip_r(r, n)
    dy = torch.randn((B, n - re_, 32), generator=gen, dtype=torch.float64)
    pub_merge = published_bipartite_soft_matching(qkv[:, :, 1].double().mean(dim=2), r)[0]
    for s in (None, size):
        xr = x.clone().requires_grad_(True)
        out, size_out, _, _ = R.merge(xr, s, *plan)
        (want,) = torch.autograd.grad(out, xr, dy)
        got = T.merge_backward(dy, s, size_out, plan)
        torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)
        # ... and through the published merge_wavg (its plan is the same set of edges, test_tome_cpu.py)
        xp = x.clone().requires_grad_(True)
        out_p, _ = published_merge_wavg(pub_merge, xp, None if s is None else s[..., None])
        (want_p,) = torch.autograd.grad(out_p, xp, dy)
        torch.testing.assert_close(got, want_p, rtol=1e-12, atol=1e-13)
        # the vectorised restatement the block reference uses is tome_ref.merge
        out_v, size_v = T.merge(x, s, plan)
        torch.testing.assert_close(out_v, out.detach(), rtol=1e-13, atol=1e-13)
        assert torch.equal(size_v, size_out)
        # the adjoint identity <dx, x> = <dy, merge(x)>
        assert float((got * x).sum()) == pytest.approx(float((dy * out.detach()).sum()), rel=1e-11)


def test_restated_attention_and_block_agree_with_tome_ref():
    gen = torch.Generator().manual_seed(3)
    B, n, H = 2, 13, 2
    qkv = torch.randn((B, n, 3, H, 64), generator=gen, dtype=torch.float64)
    w = torch.randint(1, 5, (B, n), generator=gen).double()
    torch.testing.assert_close(T.keyw_attention(qkv, w, 0.125), R.keyw_attention(qkv, w, 0.125)[0], rtol=1e-12, atol=1e-12)
    dout = torch.randn((B, n, H * 64), generator=gen, dtype=torch.float64)
    q = qkv.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(T.keyw_attention(q, w, 0.125), q, dout)
    torch.testing.assert_close(T.keyw_attention_grad(qkv, w, 0.125, dout), want, rtol=1e-11, atol=1e-12)


# ---- loss ----
@pytest.mark.parametrize("soft", [False, True])
def test_tome_loss_against_torch(soft):
    gen = torch.Generator().manual_seed(11)
    ls, lt = torch.randn((6, 10), generator=gen, dtype=torch.float64), torch.randn((6, 10), generator=gen, dtype=torch.float64)
    labels = torch.softmax(torch.randn((6, 10), generator=gen, dtype=torch.float64), dim=-1) if soft else torch.randint(0, 10, (6,), generator=gen)
    ce = F.cross_entropy(ls, labels)
    kl = F.kl_div(torch.log_softmax(ls, -1), torch.log_softmax(lt, -1), reduction="batchmean", log_target=True)
    assert float(T.tome_loss(ls, lt, labels, 1.0, 0.5)) == pytest.approx(float(ce + 0.5 * kl), rel=1e-12)
    assert float(T.tome_loss(ls, lt, labels, 0.7, 2.0)) == pytest.approx(float(0.7 * ce + 2.0 * kl), rel=1e-12)
    assert float(T.tome_loss(ls, None, labels, 1.0, 0.5)) == pytest.approx(float(ce), rel=1e-12)
    assert float(T.tome_loss(ls, lt, labels, 1.0, 0.0)) == pytest.approx(float(ce), rel=1e-12)


# ---- command line ----
def test_check_supported_accepts_and_refuses_tome_train(capsys):
    import mask_predictor
    import utils
    assert utils.parse_args([]).tome_train is False
    for mode in ("exact", "split"):
        a = utils.parse_args(["--method", "tome", "--tome-train", "--tome-r", "13", "--student-checkpoint", "w.pt", "--gemm-mode", mode])
        mask_predictor.check_supported(a)
        assert a.tome_train and a.method == "tome" and not a.eval_only and a.warmup_steps == 0
    refusals = ((["--method", "tome", "--student-checkpoint", "w.pt"], "--method tome without --eval-only"),                 # untouched
                (["--tome-train"], "--tome-train with --method d2s"),
                (["--tome-train", "--method", "dynamicvit"], "--tome-train with --method dynamicvit"),
                (["--method", "tome", "--tome-train", "--drop-path", "0.1"], "--tome-train with --drop-path 0.1"),
                (["--method", "tome", "--tome-train", "--gemm-mode", "bf16"], "--method tome with --gemm-mode bf16"))
    for extra, needle in refusals:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert str(e.value).startswith("not on the accelerated path: ") and needle in str(e.value), (extra, str(e.value))
    with pytest.raises(SystemExit) as e:
        mask_predictor.check_supported(utils.parse_args(["--method", "tome", "--student-checkpoint", "w.pt"]))
    assert "token merging is built for inference: training through a merge needs the merge's backward and key weights in both " \
           "attention-backward kernels" in str(e.value)
    capsys.readouterr()
    a = utils.parse_args(["--method", "tome", "--tome-train", "--warmup-steps", "3"])
    mask_predictor.check_supported(a)
    assert a.warmup_steps == 0 and "Attention: --tome-train" in capsys.readouterr().out


# ---- constructor, TrainStep ----
def test_constructor_opt_in_and_train_step_refusals():
    import vit_models
    from vit_models import tome
    from d2s import lib
    from d2s.engine import TrainStep
    m = vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_merge=True)
    assert m.train_merge and m.tome_r == [3, 3, 3, 3] and m.grad_ready_hook is None
    assert list(m.state_dict()) == list(vit_models.VisionTransformerTeacher(**MICRO).state_dict())
    assert vit_models.tome_deit_tiny_patch16_224(2, train_merge=True).train_merge and not vit_models.tome_deit_small_patch16_224(2).train_merge
    with pytest.raises(ValueError, match="drop_path_rate"):
        vit_models.VisionTransformerToMe(**MICRO, tome_r=3, train_merge=True, drop_path_rate=0.1)
    d = vit_models.VisionTransformerToMe(**MICRO, tome_r=3).train()            # the default still refuses, with the pinned text
    assert not d.train_merge
    with pytest.raises(NotImplementedError) as e:
        d(torch.zeros(1, 3, 64, 64))
    assert str(e.value) == tome.TOME_TRAINING_ERROR
    args = types.SimpleNamespace(mixup=0.0)
    with pytest.raises(lib.D2SError, match="graph=True"):                      # refusals come before anything touches the device
        TrainStep(m, None, args, graph=True)
    with pytest.raises(ValueError, match="warmup_steps"):
        TrainStep(m, None, args, warmup_steps=1)
    with pytest.raises(lib.D2SError, match="train_merge=True"):
        TrainStep(d, None, args)
    with pytest.raises(lib.D2SError, match="without a teacher"):
        TrainStep(vit_models.VisionTransformerTeacher(**MICRO), None, args)


def test_checkpoint_config_records_the_merging_student():
    import vit_models
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    a = cfg(vit_models.VisionTransformerToMe(**MICRO, tome_r=[2, 1, 0, 3], prop_attn=False, train_merge=True))
    b = cfg(vit_models.VisionTransformerToMe(**MICRO, tome_r=2))
    assert (a["tome_r"], a["prop_attn"], a["train_merge"]) == ([2, 1, 0, 3], False, True) and a["model"] == "VisionTransformerToMe"
    assert (b["tome_r"], b["prop_attn"], b["train_merge"]) == ([2, 2, 2, 2], True, False)
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in a.items() if k not in ("tome_r", "prop_attn", "train_merge")}
    filled = engine.checkpoint_config(old)
    assert (filled["tome_r"], filled["prop_attn"], filled["train_merge"]) == ([], False, False) and "tome_r" not in old


def test_tome_loss_module_reads_its_weights():
    from losses import ToMeLoss
    fn = ToMeLoss(types.SimpleNamespace(mixup=0.8, cls_weight=0.7, dist_weight=0.0))
    assert fn.soft_targets and fn.cls_weight == 0.7 and fn.dist_weight == 0.0
    fn = ToMeLoss(types.SimpleNamespace())
    assert not fn.soft_targets and fn.cls_weight == 1.0 and fn.dist_weight == 0.5


# ---- binding ----
def test_library_binding_declares_the_two_backward_entries_once():
    from d2s import lib, ops
    header = open(os.path.join(REPO, "include", "d2s_hip.h")).read()
    for name in ("d2s_tome_merge_bwd", "d2s_attn_keyw_bwd_f32"):
        assert name in lib.symbols("d2s_hip.h") and "int " + name + "(" in header
    assert callable(ops.tome_merge_bwd) and callable(ops.attn_keyw_bwd)
    from d2s import functional_tome
    assert callable(functional_tome.ToMeBlockFn.apply) and callable(functional_tome.tome_block_forward)


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
