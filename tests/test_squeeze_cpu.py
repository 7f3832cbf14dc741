"""Pruning and squeezing (squeeze_dropped), the parts that need no GPU: the closed-form backward of
tests/squeeze_ref.py against float64 autograd, the qualification of the GPU test's match inputs (every dropped token's best cosine leads
its second best by four times the fp32 worst case), the validity of the merge's bound (an emulation of the kernel's roundings on the GPU
test's very inputs), and the host side: command line, constructor, factories, checkpoint config, header and binding tables."""
import inspect
import json
import os
import re
import types

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import squeeze_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
NEW = ["d2s_gather_squeeze_bwd", "d2s_gather_squeeze_fwd", "d2s_squeeze_match"]


# ---- the reference ----
@pytest.mark.parametrize("shape", R.SHAPES[:5], ids=str)
def test_closed_form_backward_is_float64_autograd_with_the_plan_held_constant(shape):
    x, kept, dropped, g = R.inputs(shape)
    x, g = x.double(), g.double()
    dst, sim = R.match(x, kept, dropped)
    y, Z, dx = R.merge_autograd(x, kept, dropped, dst, sim, g)
    closed = R.merge_backward(g, kept, dropped, dst, sim, x.shape[1])
    torch.testing.assert_close(closed, dx, rtol=1e-12, atol=1e-14)
    assert y.shape == (shape[0], shape[2] + 1, shape[3]) and Z.shape == (shape[0], shape[2])
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(dx[:, 0], g[:, 0])
    hit = torch.zeros(kept.shape, dtype=torch.bool).scatter(1, dst.long(), torch.ones(dst.shape, dtype=torch.bool))
    assert torch.equal(y[:, 1:][~hit], R.rows(x, kept)[~hit]) and bool((Z[~hit] == R.E).all()) and bool((Z[hit] > R.E).all())
    assert torch.equal(R.rows(dx, kept)[~hit], g[:, 1:][~hit])                       # a kept row without a source: its row of g, bit for bit
    assert float(R.rows(dx, dropped).abs().min()) > 0                                # every dropped row receives a gradient
    lhs, rhs = float((dx * x).sum()), float((g * y).sum())                           # the merge is linear in x for a fixed plan
    assert lhs == pytest.approx(rhs, rel=1e-12)


def test_reference_degenerate_stages_and_the_tie_rule():
    x, kept, dropped, g = R.inputs(R.SHAPES[2])
    x = x.double()
    T = x.shape[1] - 1
    everyone = torch.arange(T).expand(x.shape[0], -1).contiguous()
    nobody = torch.empty((x.shape[0], 0), dtype=torch.int64)
    dst, sim = R.match(x, everyone, nobody)
    y, Z = R.merge(x, everyone, nobody, dst, sim)
    assert dst.shape == (x.shape[0], 0) and torch.equal(y, x) and bool((Z == R.E).all())      # m == 0: the gather
    xd, kd, dd, pos = R.duplicate_inputs()
    dst, sim = R.match(xd.double(), kd, dd)
    assert [int(dst[0, i]) for i in pos] == [4, 4]                                   # rows 4 and 11 are bit-identical: the lower position
    xz = x.clone()
    xz[0, 1 + dropped[0, 0]] = 0
    xz[1, 1 + kept[1, 0]] = 0
    dst, sim = R.match(xz, kept, dropped)
    assert float(sim[0, 0]) == 0 and int(dst[0, 0]) == 0 and bool(torch.isfinite(sim).all())  # a zero row: every cosine is 0


# ---- the GPU test's match inputs ----
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_every_match_of_the_gpu_inputs_is_separated_by_four_times_the_fp32_worst_case(shape):
    B, T, k, D = shape
    x, kept, dropped, _ = R.inputs(shape)
    gaps = R.gaps(x, kept, dropped)
    assert gaps.shape == (B, T - k)                                                  # no dropped token is left out
    print(f"{shape}: smallest gap {float(gaps.min()):.3e}, required {R.margin(D):.3e}")
    assert float(gaps.min()) >= R.margin(D) == 4 * (2 * D + 8) * 2.0 ** -24
    assert R.find_seed(*shape) == R.SEEDS[shape]                                     # the fixed seed is the first that qualifies
    assert torch.equal(torch.sort(torch.cat([kept, dropped], dim=1), dim=1)[0], torch.arange(T).expand(B, -1))


# ---- the merge's bound ----
@pytest.mark.parametrize("ulps", [-1, 0, 1])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_merge_bound_holds_for_an_emulation_of_the_kernels_roundings(shape, ulps):
    x, kept, dropped, _ = R.inputs(shape)
    dst, sim64 = R.match(x.double(), kept, dropped)
    sim = sim64.float()                                                              # the plan as the match kernel hands it on: fp32
    y, Z = R.emulate_merge(x, kept, dropped, dst, sim, expf_ulps=ulps)
    y64, Z64 = R.merge(x.double(), kept, dropped, dst, sim.double())
    by, bz, s = R.merge_bounds(x.double(), kept, dropped, dst, sim.double())
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(y[:, 1:][s == 0], R.rows(x, kept)[s == 0])
    assert int(s.sum()) == dropped.numel() and int(s.max()) >= 1
    fy = float(((y[:, 1:].double() - y64[:, 1:]).abs() / by.clamp_min(1e-300))[s > 0].max())
    fz = float(((Z.double() - Z64).abs() / bz)[s > 0].max())
    print(f"{shape} expf {ulps:+d} ulp: up to {int(s.max())} sources per row; err / bound: y {fy:.3f}, Z {fz:.3f}")
    assert fy <= 1.0 and fz <= 1.0


def test_merge_bound_holds_with_ten_sources_on_one_row():
    x, kept, dropped, _ = R.inputs((2, 17, 8, 192))
    T, k = 17, 7
    kept, dropped = torch.arange(k).expand(2, -1).contiguous(), torch.arange(k, T).expand(2, -1).contiguous()
    dst = torch.tensor([[3] * 10, [6] * 10], dtype=torch.int32)
    sim = torch.linspace(-1, 1, 10).expand(2, -1).contiguous()
    y, Z = R.emulate_merge(x, kept, dropped, dst, sim)
    y64, Z64 = R.merge(x.double(), kept, dropped, dst, sim.double())
    by, bz, s = R.merge_bounds(x.double(), kept, dropped, dst, sim.double())
    assert s.tolist() == [[0, 0, 0, 10, 0, 0, 0], [0, 0, 0, 0, 0, 0, 10]]
    assert bool(((y[:, 1:].double() - y64[:, 1:]).abs() <= by)[s > 0].all()) and bool(((Z.double() - Z64).abs() <= bz).all())


# ---- command line ----
def test_cli_accepts_the_flag_and_check_supported_refuses_what_it_cannot_combine():
    import mask_predictor
    import utils
    assert utils.parse_args([]).squeeze_dropped is False
    a = utils.parse_args(["--topk-selection", "--squeeze-dropped"])
    assert a.squeeze_dropped is True and a.fuse_dropped is False
    mask_predictor.check_supported(a)
    mask_predictor.check_supported(utils.parse_args(["--topk-selection", "--squeeze-dropped", "--attn-selection", "--pruning-locs", "3",
                                                     "--keep-ratios", "0.5"]))
    refusals = ((["--squeeze-dropped"], "--squeeze-dropped without --topk-selection"),
                (["--topk-selection", "--squeeze-dropped", "--fuse-dropped"], "--squeeze-dropped with --fuse-dropped"),
                (["--topk-selection", "--squeeze-dropped", "--diff-topk"], "--squeeze-dropped with --diff-topk"),
                (["--topk-selection", "--squeeze-dropped", "--patch-score-threshold", "0.5"], "--squeeze-dropped with --patch-score-threshold"),
                (["--method", "dynamicvit", "--squeeze-dropped"], "--squeeze-dropped with --method dynamicvit"),
                (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--squeeze-dropped"], "--squeeze-dropped with --method tome"))
    for extra, needle in refusals:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert str(e.value).startswith("not on the accelerated path: ") and needle in str(e.value), (extra, str(e.value))


def test_the_refusals_of_fuse_dropped_keep_their_texts():
    import mask_predictor
    import utils
    texts = ((["--fuse-dropped"], "--fuse-dropped without --topk-selection (the package token is weighted by the score predictor's keep probabilities)"),
             (["--topk-selection", "--fuse-dropped", "--patch-score-threshold", "0.5"],
              "--fuse-dropped with --patch-score-threshold (no token is removed there: nothing to fuse)"),
             (["--topk-selection", "--fuse-dropped", "--diff-topk"], "--fuse-dropped with --diff-topk (the soft gather has no dropped set)"),
             (["--method", "dynamicvit", "--fuse-dropped"],
              "--method dynamicvit with --fuse-dropped (the baseline keeps tokens by its own Gumbel decision and predictor)"))
    for extra, text in texts:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert text in str(e.value).split("not on the accelerated path: ", 1)[1].split("; ")
    mask_predictor.check_supported(utils.parse_args(["--topk-selection", "--fuse-dropped"]))


# ---- constructor and factories ----
def _student(**kw):
    import vit_models
    kw.setdefault("topk_selection", True)
    return vit_models.VisionTransformerDiffPruning(pruning_loc=[1], token_ratio=[0.05], distill=True, predictor_loss_type="kl_div", **MICRO, **kw)


def test_constructor_keyword_its_position_and_its_refusals():
    import vit_models
    from vit_models import dynamic_vit
    names = list(inspect.signature(vit_models.VisionTransformerDiffPruning.__init__).parameters)
    assert names.index("squeeze_dropped") == names.index("fuse_dropped") + 1 and names[-3:] == ["init_n", "diff_topk", "topk_num_samples"]
    assert inspect.signature(vit_models.VisionTransformerDiffPruning.__init__).parameters["squeeze_dropped"].default is False
    off, on = _student(), _student(squeeze_dropped=True)
    assert off.squeeze_dropped is False and on.squeeze_dropped is True and on.squeeze_plans == [] and on.squeeze_plan_override is None
    assert list(off.state_dict()) == list(on.state_dict())                           # no parameters are added
    assert _student(squeeze_dropped=True, attn_selection=True).attn_selection is True
    for kw, text in ((dict(fuse_dropped=True), dynamic_vit.SQUEEZE_DROPPED_FUSE_ERROR),
                     (dict(diff_topk=True), dynamic_vit.SQUEEZE_DROPPED_DIFF_TOPK_ERROR),
                     (dict(patch_score_threshold=0.5), dynamic_vit.SQUEEZE_DROPPED_THRESHOLD_ERROR),
                     (dict(topk_selection=False), dynamic_vit.SQUEEZE_DROPPED_TOPK_SELECTION_ERROR)):
        with pytest.raises(ValueError) as e:
            _student(squeeze_dropped=True, **kw)
        assert str(e.value) == text and "squeeze_dropped" in text


@pytest.mark.parametrize("factory", ["dynamic_vit_tiny_patch16_224_student", "dynamic_vit_small_patch16_224_student",
                                     "dynamic_vit_base_patch16_224_student"])
def test_factories_hand_the_keyword_through(factory):
    import vit_models
    f = getattr(vit_models, factory)
    assert "squeeze_dropped" not in inspect.signature(f).parameters                  # through **kwargs
    assert f([3], [0.5], topk_selection=True, squeeze_dropped=True).squeeze_dropped is True
    assert f([3], [0.5], topk_selection=True).squeeze_dropped is False


def test_build_models_passes_the_flag_on():
    import mask_predictor
    import utils
    a = utils.parse_args(["--arch", "deit_tiny", "--topk-selection", "--squeeze-dropped", "--pruning-locs", "3", "--keep-ratios", "0.5"])
    a.device = "cpu"
    student, _ = mask_predictor.build_models(a)
    assert student.squeeze_dropped is True and student.fuse_dropped is False


# ---- checkpoints ----
def test_checkpoint_config_records_the_flag_last_and_old_checkpoints_count_as_off():
    from d2s.engine import TrainStep, checkpoint_config
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfgs = [TrainStep.config(types.SimpleNamespace(student=s, args=args)) for s in (_student(), _student(squeeze_dropped=True))]
    assert cfgs[0]["squeeze_dropped"] is False and cfgs[1]["squeeze_dropped"] is True
    assert list(cfgs[0])[-1] == "squeeze_dropped" and {k for k in cfgs[0] if cfgs[0][k] != cfgs[1][k]} == {"squeeze_dropped"}
    for c in cfgs:
        assert json.loads(json.dumps(c)) == c
    old = {k: v for k, v in cfgs[0].items() if k != "squeeze_dropped"}
    assert checkpoint_config(old)["squeeze_dropped"] is False and "squeeze_dropped" not in old
    assert checkpoint_config(cfgs[1])["squeeze_dropped"] is True


# ---- header and binding ----
def test_squeeze_header_and_binding_tables():
    from d2s import lib, ops
    import d2s.functional as DF
    text = open(os.path.join(REPO, "include", "d2s_hip_squeeze.h")).read()
    assert NEW == lib.symbols("d2s_hip_squeeze.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) >= 1 + len(NEW)               # the file's own comment and one per entry
    assert callable(ops.squeeze_match) and callable(ops.gather_squeeze_fwd) and callable(ops.gather_squeeze_bwd)
    assert issubclass(DF.GatherSqueezeFn, torch.autograd.Function)
