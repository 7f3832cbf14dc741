"""CPU tier of ragged inference through every threshold stage (--ragged-cascade): the restatement the GPU tier is
checked against (tests/ragged_cascade_ref.py) agrees with the oracle where the oracle is defined (one stage), keeps everything at
threshold 0, selects the same ids in fp32 and in fp64 on the GPU tier's cases - the precondition for demanding exact ids there - and the
command line accepts the combination only with the flag.  PARITY UNPINNED for the later stages: the reference's second stage cannot run."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import ragged_cascade_ref as R
from oracle import d2s_oracle as O

CASES = R.cascade_cases()
# per-image non-CLS tokens entering each stage, then the survivors of the last one (fp32 == fp64)
COUNTS = {
    "micro_thr2": [[16, 16, 16], [7, 8, 7], [2, 3, 3]],
    "small_thr3": [[196, 196, 196], [73, 70, 67], [26, 29, 30], [12, 11, 13]],
    "micro_thr3s": [[36, 36, 36, 36], [21, 20, 20, 21], [13, 12, 12, 12], [8, 8, 8, 8]],
}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(case):
    sd_s, _ = cases.make_weights(case)
    return {k: _t(v) for k, v in sd_s.items()}, _t(cases.make_images(case))


def test_one_stage_restatement_is_the_oracle():
    case = cases.THRESHOLD_CASES["micro_thr1"]
    sd, x = _inputs(case)
    with torch.no_grad():
        logits, feats, stages = R.cascade_forward(sd, x, case["cfg"], case["threshold"])
        ologits, ofeats, oscores, omask = O.student_forward_threshold_eval(sd, x, case["cfg"], case["threshold"])
    np.testing.assert_allclose(logits.numpy(), ologits.numpy(), rtol=0, atol=1e-6)
    assert len(stages) == 1
    np.testing.assert_array_equal(R.dense_masks(stages, case["cfg"]["n_patches"])[0].numpy(), omask.numpy())
    for b, f in enumerate(ofeats):
        np.testing.assert_allclose(feats[b].numpy(), f.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(stages[0][b][2].numpy(), oscores[b].numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", ["micro_thr2", "micro_thr3s"])
def test_threshold_zero_keeps_everything_and_is_the_dense_forward(name):
    case = CASES[name]
    sd, x = _inputs(case)
    N = case["cfg"]["n_patches"]
    logits, feats, stages = R.reference(name, threshold=0.0)
    assert len(stages) == len(case["cfg"]["pruning_loc"])
    for per_image in stages:
        for T, ids, scores in per_image:
            assert T == N and ids.tolist() == list(range(N)) and scores.shape == (N,)
    with torch.no_grad():
        dlogits, dtokens, _ = O.teacher_forward(sd, x, case["cfg"])      # the same blocks, no stage: the dense forward
    # two fp32 evaluations of the same blocks (per image vs the whole batch: another summation order inside the GEMMs): the tolerance
    # the suite holds such pairs to (tests/test_threshold_gpu.py)
    np.testing.assert_allclose(logits.numpy(), dlogits.numpy(), rtol=1e-4, atol=2e-5)
    for b in range(x.shape[0]):
        np.testing.assert_allclose(feats[b][1:].numpy(), dtokens[b].numpy(), rtol=1e-4, atol=3e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_and_fp64_select_identical_ids_at_every_stage(name):
    """What lets the GPU tier demand exact ids: no token of these cases sits within fp32 noise of the threshold."""
    case = CASES[name]
    _, _, s32 = R.reference(name, torch.float32)
    _, _, s64 = R.reference(name, torch.float64)
    S = len(case["cfg"]["pruning_loc"])
    assert len(s32) == len(s64) == S
    for s in range(S):
        for b in range(case["batch"]):
            assert s32[s][b][0] == s64[s][b][0] == COUNTS[name][s][b], (s, b, s32[s][b][0], s64[s][b][0])
            assert s32[s][b][1].tolist() == s64[s][b][1].tolist(), (s, b)
            np.testing.assert_allclose(s32[s][b][2].numpy(), s64[s][b][2].numpy(), rtol=1e-4, atol=2e-5)
    last = [int(ids.numel()) for _, ids, _ in s32[-1]]
    assert last == COUNTS[name][S], last
    ragged = [len(set(int(ids.numel()) for _, ids, _ in per_image)) > 1 for per_image in s32]
    assert any(ragged), "the case should be genuinely ragged at some stage"


def test_cli_accepts_several_threshold_stages_only_with_the_flag():
    import mask_predictor
    import utils
    line = ["--patch-score-threshold", "0.4", "--pruning-locs", "3", "6", "9", "--keep-ratios", "0.7", "0.5", "0.3"]
    assert utils.parse_args([]).ragged_cascade is False
    a = utils.parse_args(line + ["--ragged-cascade"])
    assert a.ragged_cascade is True
    mask_predictor.check_supported(a)
    with pytest.raises(SystemExit, match="not on the accelerated path"):
        mask_predictor.check_supported(utils.parse_args(line))
    with pytest.raises(SystemExit, match="not on the accelerated path"):
        mask_predictor.check_supported(utils.parse_args(line + ["--ragged-cascade", "--predictor-bn"]))
    mask_predictor.check_supported(utils.parse_args(["--patch-score-threshold", "0.4", "--pruning-locs", "3", "--keep-ratios", "0.5",
                                                     "--ragged-cascade", "--predictor-bn"]))      # one stage: either predictor


def test_cli_names_the_definition(capsys):
    import mask_predictor
    import utils
    mask_predictor.check_supported(utils.parse_args(["--patch-score-threshold", "0.4", "--pruning-locs", "3", "6", "--keep-ratios", "0.7", "0.5",
                                                     "--ragged-cascade"]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Attention: --ragged-cascade")]
    assert len(lines) == 1 and "DESIGN.md section 10" in lines[0]
