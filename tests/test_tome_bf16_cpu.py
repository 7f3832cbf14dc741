"""Token merging on the bf16 data path (--tome-bf16), the parts that need no GPU: the extension header and its
binding table, the command line's acceptance and refusals, the constructor keyword, the validity of the float64 test's bounds (a CPU
emulation of the weighted kernel's roundings on the very inputs of the GPU test), and that the package imports neither oracle/ nor tests/."""
import os
import re

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import tome_bf16_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_attn_keyw_fwd_bf16", "d2s_tome_match_bf16"]


# ---- header and binding ----
def test_extension_header_and_binding_table():
    from d2s import lib, ops
    ext = open(os.path.join(REPO, "include", "d2s_hip_ext.h")).read()
    assert NEW == lib.symbols("d2s_hip_ext.h")
    assert len(re.findall(r"^/\* ", ext, flags=re.M)) >= 1 + len(NEW)          # the file's own comment and one per entry
    assert callable(ops.attn_keyw_fwd_bf16io) and callable(ops.tome_match_bf16)
    from d2s import functional_tome
    assert callable(functional_tome.tome_block_forward_bf16)


# ---- command line ----
def test_check_supported_accepts_and_refuses_tome_bf16():
    import mask_predictor
    import utils
    assert utils.parse_args([]).tome_bf16 is False
    base = ["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt"]
    a = utils.parse_args(base + ["--tome-r", "13", "--tome-bf16"])
    mask_predictor.check_supported(a)
    assert a.tome_bf16 is True and a.gemm_mode in ("exact", "split")
    refusals = ((["--tome-bf16", "--eval-only", "--student-checkpoint", "w.pt"], "--tome-bf16 with --method d2s"),
                (["--method", "dynamicvit", "--tome-bf16", "--eval-only", "--student-checkpoint", "w.pt"], "--tome-bf16 with --method dynamicvit"),
                (["--method", "tome", "--tome-train", "--tome-bf16", "--student-checkpoint", "w.pt"], "--tome-bf16 with --tome-train"),
                (["--method", "tome", "--tome-train", "--tome-bf16", "--student-checkpoint", "w.pt"], "--tome-bf16 without --eval-only"),
                (base + ["--gemm-mode", "bf16"], "--method tome with --gemm-mode bf16 (the key-weighted attention is an fp32 kernel; exact and split run)"),
                (base + ["--tome-bf16", "--gemm-mode", "bf16"], "--method tome with --gemm-mode bf16"))
    for extra, needle in refusals:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert str(e.value).startswith("not on the accelerated path: ") and needle in str(e.value), (extra, str(e.value))
    mask_predictor.check_supported(utils.parse_args(base + ["--tome-r", "13"]))                      # the fp32 route is untouched


# ---- constructor ----
def test_constructor_takes_the_bf16_keyword():
    import vit_models
    m = vit_models.VisionTransformerToMe(**MICRO, tome_r=3, bf16=True)
    assert m.bf16 is True and m.tome_r == [3] * 4 and not m.train_merge
    assert vit_models.VisionTransformerToMe(**MICRO, tome_r=3).bf16 is False
    with pytest.raises(ValueError):
        vit_models.VisionTransformerToMe(**MICRO, tome_r=3, bf16=True, train_merge=True)
    for factory in (vit_models.tome_deit_tiny_patch16_224, vit_models.tome_deit_small_patch16_224):
        assert factory(2, bf16=True).bf16 is True and factory(2).bf16 is False
    import inspect
    from vit_models import tome
    assert "bf16" in inspect.signature(tome.VisionTransformerToMe.__init__).parameters
    assert inspect.signature(vit_models.tome_deit_base_patch16_224).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "bf16" not in inspect.signature(tome._tome).parameters               # the three factories hand it through **kwargs
    m.train()
    with pytest.raises(NotImplementedError) as e:                               # raised before anything touches the device
        m(torch.zeros(1, 3, 64, 64))
    assert str(e.value) == tome.TOME_TRAINING_ERROR


# ---- the bounds of the GPU float64 test hold for the kernel's roundings ----
@pytest.mark.parametrize("n,H", C.KEYW_SHAPES)
def test_bounds_hold_for_an_emulation_of_the_kernels_roundings(n, H):
    case = C.keyw_case(n, H)
    w = case["w"]
    assert bool((w >= 1).all()) and bool((w == w.round()).all()) and bool((w.max(dim=1).values >= max(n // 2, 1)).all())
    assert torch.equal(case["qkv"], case["qkv"].bfloat16().float())
    out, out16, lse = C.emulate_kernel(case)
    fr = C.fractions(case, out, out16, lse)
    print(f"emulated keyw attention n {n} H {H}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    for k, v in fr.items():
        assert v <= 1.0, (k, n, H, v)


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
