"""Stochastic depth (DropPath), the parts that need no GPU: the command-line flag, the modules the constructors build, the per-block
rates, the unchanged state-dict keys, and the float64 restatement in tests/droppath_ref.py against the reference's formula."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests import droppath_ref as R

MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


def test_drop_path_flag_parses_and_is_range_checked():
    import utils
    import mask_predictor
    assert utils.parse_args([]).drop_path == 0.0
    assert utils.parse_args(["--drop-path", "0.1"]).drop_path == pytest.approx(0.1)
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit, match="--drop-path"):
            mask_predictor.check_supported(utils.parse_args(["--drop-path", bad]))
    mask_predictor.check_supported(utils.parse_args(["--drop-path", "0.1"]))


def test_block_builds_drop_path_or_identity():
    import vit_models
    from vit_models import transformer_block
    for cls in (vit_models.Block, transformer_block.Block):
        blk = cls(128, 2, qkv_bias=True, drop_path=0.1)
        assert isinstance(blk.drop_path, vit_models.DropPath) and blk.drop_path.drop_prob == 0.1
        assert isinstance(cls(128, 2, qkv_bias=True).drop_path, nn.Identity)
    assert not list(vit_models.DropPath(0.3).parameters())


def test_drop_path_module_is_identity_in_eval():
    import vit_models
    m = vit_models.DropPath(0.5).eval()
    x = torch.randn(3, 5, 7)
    assert m(x) is x


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_student_and_teacher_blocks_carry_the_linspace_rates(rate):
    import vit_models
    student = vit_models.VisionTransformerDiffPruning(pruning_loc=[1], token_ratio=[0.5], topk_selection=True, predictor_loss_type="kl_div",
                                                      drop_path_rate=rate, **MICRO)
    teacher = vit_models.VisionTransformerTeacher(drop_path_rate=rate, **MICRO)
    want = [x.item() for x in torch.linspace(0, rate, MICRO["depth"])]
    for model in (student, teacher):
        assert isinstance(model.blocks[0].drop_path, nn.Identity)
        got = [0.0] + [b.drop_path.drop_prob for b in model.blocks[1:]]
        assert got == want
    assert student.drop_path_rate == rate and student.drop_path_masks is None


def test_t2t_models_accept_a_rate():
    import vit_models
    m = vit_models.T2T_ViT(img_size=64, tokens_type="performer", embed_dim=128, depth=3, num_heads=2, mlp_ratio=3.0, num_classes=10,
                           drop_path_rate=0.2)
    assert [getattr(b.drop_path, "drop_prob", 0.0) for b in m.blocks] == [x.item() for x in torch.linspace(0, 0.2, 3)]
    assert set(m.state_dict()) == set(vit_models.T2T_ViT(img_size=64, tokens_type="performer", embed_dim=128, depth=3, num_heads=2,
                                                         mlp_ratio=3.0, num_classes=10).state_dict())


def test_state_dict_keys_do_not_change():
    import vit_models
    kw = dict(pruning_loc=[1], token_ratio=[0.5], topk_selection=True, predictor_loss_type="kl_div", **MICRO)
    a = vit_models.VisionTransformerDiffPruning(**kw).state_dict()
    b = vit_models.VisionTransformerDiffPruning(drop_path_rate=0.3, **kw).state_dict()
    assert list(a) == list(b)


def test_rates_outside_the_unit_interval_are_refused():
    import vit_models
    with pytest.raises(AssertionError):
        vit_models.VisionTransformerTeacher(drop_path_rate=1.0, **MICRO)
    with pytest.raises(AssertionError):
        vit_models.Block(128, 2, qkv_bias=True, drop_path=-0.1)


def test_fixture_masks_are_not_vacuous():
    g = cases.load_golden("droppath_micro")
    for prefix in ("", "thr_"):
        masks, rates = g[prefix + "masks"], g[prefix + "rates"]
        assert masks.shape == (8, int(g[prefix + "batch"])) and set(np.unique(masks)) <= {0.0, 1.0}
        assert list(rates) == R.rates(R.fixture_case(g, prefix)[0]["cfg"], 0.5)
        live = masks[rates > 0]
        assert np.all(masks[rates == 0] == 1)
        assert sum(0 < r.sum() < r.size for r in live) * 2 >= len(live) and np.all(live.sum(axis=0) > 0)
    assert int(g["batch"]) >= 4


@pytest.mark.parametrize("prefix", ["", "thr_"])
def test_restatement_reproduces_the_reference_run_with_drop_path(prefix):
    """tests/droppath_ref.py with the fixture's masks injected, evaluated in the reference's own arithmetic (float32 on the CPU, as
    tests/test_oracle_golden.py evaluates the oracle: those tolerances bound the difference of two fp32 runs of the same operations; a
    float64 run differs from the recorded fp32 outputs by the reference's own rounding, 3.6e-6 on pred_logits of O(1)), against what the reference's own student produced at
    drop_path_rate 0.5 (tools/gen_droppath_fixture.py): the selection exactly, logits / features / pred_logits / probe loss and every
    parameter gradient to the tolerances tests/test_oracle_golden.py applies to the same kind of case (model cases: 1e-5 / 1e-6 and
    norms 2e-4, heads 2e-3; threshold cases: 1e-4 / 1e-5 (features 2e-5) and norms 2e-3).  This pins the restatement - the linspace rule
    through the whole student, the row order 2i / 2i + 1, the place of the scale, pruning and the policy softmax - before any GPU test
    relies on it."""
    g = cases.load_golden("droppath_micro")
    out = R.run_fixture_case(g, prefix, dtype=torch.float32)
    thr = bool(prefix)
    tol = dict(rtol=1e-4, atol=1e-5) if thr else dict(rtol=1e-5, atol=1e-6)
    i = 0
    while f"{prefix}kept_{i}" in g.files:
        np.testing.assert_array_equal(out["sel"][i].detach().numpy().astype(np.float64), g[f"{prefix}kept_{i}"].astype(np.float64))
        np.testing.assert_allclose(out["pred_logits"][i].numpy(), g[f"{prefix}pred_logits_{i}"], **tol)
        i += 1
    assert i == len(out["sel"]) >= 1
    np.testing.assert_allclose(out["logits"].numpy(), g[prefix + "logits"], **tol)
    assert list(out["features"].shape) == list(g[prefix + "features_shape"])
    np.testing.assert_allclose(out["features"][:, :4, :16].numpy(), g[prefix + "features_slice"], rtol=tol["rtol"], atol=2e-5 if thr else 1e-6)
    np.testing.assert_allclose(out["features"].sum(dim=(1, 2)).numpy(), g[prefix + "features_sum"], rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(float(out["loss"]), float(g[prefix + "probe_loss"]), rtol=1e-5)
    seen = 0
    for n, ref_norm, ref_head in zip([str(s) for s in g[prefix + "grad_names"]], g[prefix + "grad_norms"], g[prefix + "grad_heads"]):
        gr = out["grads"][n]
        if ref_norm < 0:
            assert gr is None or float(gr.abs().max()) == 0.0, n
            continue
        gf = gr.flatten()
        np.testing.assert_allclose(float(gf.norm()), ref_norm, rtol=2e-3 if thr else 2e-4, atol=1e-6 if thr else 5e-8, err_msg=n)
        if not thr:
            m = min(8, gf.numel())
            np.testing.assert_allclose(gf[:m].numpy(), ref_head[:m], rtol=2e-3, atol=1e-7, err_msg=n)
        seen += 1
    assert seen > 40


def test_restatement_without_masks_dropped_is_the_oracle():
    """all-ones masks at rate 0 are the oracle's own student (itself pinned to the reference by tests/test_oracle_golden.py)"""
    import oracle.d2s_oracle as O
    case = cases.MODEL_CASES["micro1"]
    sd = {k: torch.from_numpy(v).double() for k, v in cases.make_weights(case)[0].items()}
    x = torch.from_numpy(cases.make_images(case)).double()
    (lo, fe, _, kept), _ = O.student_forward(sd, x, case["cfg"])
    lo2, fe2, _, kept2 = R.student_forward(sd, x, case["cfg"], torch.ones(8, x.shape[0]), 0.0)
    assert torch.equal(lo, lo2) and torch.equal(fe, fe2) and torch.equal(kept[0], kept2[0])
