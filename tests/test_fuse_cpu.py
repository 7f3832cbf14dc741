"""Token fusion (fuse_dropped), the parts that need no GPU: the torch restatement in tests/fuse_ref.py against gradcheck and against the
closed-form backward the kernel implements, the command line, the constructor's refusals, the checkpoint config key, the library
binding, and the sequence-length bookkeeping of a three-stage student."""
import json
import os
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import fuse_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


def _inputs(B, n, t, k, D, seed=0, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    T = n - 1 - t
    x = torch.randn((B, n, D), generator=gen, dtype=dtype)
    p = torch.softmax(torch.randn((B, T), generator=gen, dtype=dtype), dim=-1)
    kept, dropped = R.topk_ids(p, k)
    g = torch.randn((B, k + t + 2, D), generator=gen, dtype=dtype)
    return x, p, kept, dropped, g


def test_reference_passes_gradcheck_in_float64():
    x, p, kept, dropped, _ = _inputs(2, 7, 1, 2, 8)
    x.requires_grad_(True), p.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: R.fuse_forward(a, b, kept, dropped, 1), (x, p), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("n,t,k", [(7, 1, 2), (6, 0, 1), (6, 0, 4), (6, 0, 5), (18, 1, 8), (70, 2, 30)])
def test_closed_form_backward_is_the_autograd_backward(n, t, k):
    x, p, kept, dropped, g = _inputs(3, n, t, k, 8, seed=n)
    y, dx, dp = R.fuse_autograd(x, p, kept, dropped, t, g)
    cdx, cdp = R.fuse_closed_form_backward(x, p, kept, dropped, t, g)
    T = n - 1 - t
    assert y.shape == (3, k + t + 2, 8) and dx.shape == x.shape and dp.shape == (3, T)
    torch.testing.assert_close(cdx, dx, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(cdp, dp, rtol=1e-10, atol=1e-12)
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(y[:, 1 + k:1 + k + t], x[:, 1 + T:])       # copies, bit for bit
    assert bool((torch.gather(dp, 1, kept) == 0).all())
    if k == T:                                                                                         # empty dropped set
        assert bool((y[:, -1] == 0).all()) and bool((dp == 0).all())
    else:
        assert float(dp.abs().max()) > 0


def test_zero_probability_mass_on_the_dropped_set_gives_a_zero_row():
    x, p, kept, dropped, g = _inputs(2, 7, 1, 2, 8, seed=5)
    p = p.scatter(1, dropped, 0.0)
    y, dx, dp = R.fuse_autograd(x, p, kept, dropped, 1, g)
    assert bool((y[:, -1] == 0).all()) and bool((dp == 0).all()) and bool(torch.isfinite(dx).all())


def test_cli_accepts_the_flag_and_check_supported_refuses_what_it_cannot_combine():
    import mask_predictor
    import utils
    assert utils.parse_args([]).fuse_dropped is False
    a = utils.parse_args(["--topk-selection", "--fuse-dropped"])
    assert a.fuse_dropped is True and a.topk_selection is True
    mask_predictor.check_supported(a)
    with pytest.raises(SystemExit) as e:
        mask_predictor.check_supported(utils.parse_args(["--method", "dynamicvit", "--fuse-dropped"]))
    assert "--method dynamicvit with --fuse-dropped" in str(e.value)
    for extra, needle in ((["--fuse-dropped"], "--topk-selection"),
                          (["--topk-selection", "--fuse-dropped", "--patch-score-threshold", "0.5"], "--patch-score-threshold"),
                          (["--topk-selection", "--fuse-dropped", "--diff-topk"], "--fuse-dropped with --diff-topk")):
        with pytest.raises(SystemExit, match=needle):
            mask_predictor.check_supported(utils.parse_args(extra))


def _student(**kw):
    import vit_models
    return vit_models.VisionTransformerDiffPruning(pruning_loc=[1], token_ratio=[0.05], distill=True, topk_selection=True,
                                                   predictor_loss_type="kl_div", **MICRO, **kw)


def test_constructor_default_and_refusals():
    from vit_models import dynamic_vit
    off, on = _student(), _student(fuse_dropped=True)
    assert off.fuse_dropped is False and on.fuse_dropped is True
    assert list(off.state_dict()) == list(on.state_dict())                    # no parameters are added
    with pytest.raises(ValueError) as e:
        _student(fuse_dropped=True, patch_score_threshold=0.5)
    assert str(e.value) == dynamic_vit.FUSE_DROPPED_THRESHOLD_ERROR and "patch_score_threshold" in str(e.value)
    with pytest.raises(ValueError) as e:
        _student(fuse_dropped=True, diff_topk=True)
    assert str(e.value) == dynamic_vit.FUSE_DROPPED_DIFF_TOPK_ERROR and "diff_topk" in str(e.value)
    import vit_models
    with pytest.raises(ValueError) as e:
        vit_models.VisionTransformerDiffPruning(pruning_loc=[1], token_ratio=[0.05], fuse_dropped=True, **MICRO)
    assert str(e.value) == dynamic_vit.FUSE_DROPPED_TOPK_SELECTION_ERROR and "topk_selection" in str(e.value)
    small = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, fuse_dropped=True)
    assert small.fuse_dropped                                                 # the factories forward **kwargs


def test_checkpoint_config_records_the_flag():
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfgs = [TrainStep.config(types.SimpleNamespace(student=s, args=args)) for s in (_student(), _student(fuse_dropped=True))]
    assert cfgs[0]["fuse_dropped"] is False and cfgs[1]["fuse_dropped"] is True
    for c in cfgs:
        assert json.loads(json.dumps(c)) == c
    assert {k for k in cfgs[0] if cfgs[0][k] != cfgs[1][k]} == {"fuse_dropped"}
    keys = list(cfgs[0])
    assert keys.index("fuse_dropped") == keys.index("mask_loss_type") + 1


def test_library_binding_declares_the_two_entries():
    from d2s import lib
    header = open(os.path.join(REPO, "include", "d2s_hip.h")).read()
    for name in ("d2s_gather_fuse_fwd", "d2s_gather_fuse_bwd"):
        assert name in lib.symbols("d2s_hip.h") and name + "(" in header
        assert hasattr(lib.load(), name)


def test_sequence_lengths_of_a_three_stage_student():
    """--pruning-locs 3 6 9 --keep-ratios 0.7 0.5 0.3: stage s (0-based) scores n - 1 - s rows, keeps k_s = int(init_n * ratio_s) of
    them and hands on 1 + k_s + s + 1 rows, of which the last s + 1 are package tokens; the earlier ones among them are copies."""
    import utils
    a = utils.parse_args(["--topk-selection", "--fuse-dropped", "--pruning-locs", "3", "6", "9", "--keep-ratios", "0.7", "0.5", "0.3"])
    assert list(a.pruning_locs) == [3, 6, 9] and list(a.keep_ratios) == [0.7, 0.5, 0.3]
    student = _student_for(a)
    assert student.fuse_dropped and student.pruning_loc == [3, 6, 9]
    init_n, ratios = student.init_n, student.token_ratio
    want = R.stage_lengths(init_n, ratios, True)
    assert want == [1 + int(init_n * r) + s + 1 for s, r in enumerate(ratios)]
    assert want == [139, 101, 62] and R.stage_lengths(init_n, ratios, False) == [138, 99, 59]
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((2, init_n + 1, 8), generator=gen, dtype=torch.float64)
    for s, r in enumerate(ratios):
        T = x.shape[1] - 1 - s
        p = torch.softmax(torch.randn((2, T), generator=gen, dtype=torch.float64), dim=-1)
        kept, dropped = R.topk_ids(p, int(init_n * r))
        y = R.fuse_forward(x, p, kept, dropped, s)
        assert y.shape[1] == want[s]
        assert torch.equal(y[:, y.shape[1] - 1 - s:y.shape[1] - 1], x[:, x.shape[1] - s:])
        x = y


def _student_for(a):
    import vit_models
    return vit_models.VisionTransformerDiffPruning(pruning_loc=list(a.pruning_locs), token_ratio=list(a.keep_ratios), distill=True,
                                                   topk_selection=a.topk_selection, predictor_loss_type=a.mask_loss_type,
                                                   fuse_dropped=a.fuse_dropped, img_size=224, patch_size=16, embed_dim=64, depth=10,
                                                   num_heads=1, mlp_ratio=1.0, qkv_bias=True, num_classes=10)
