"""The similarity stage after attention ranking (--sim-prune R), the parts that need no GPU: the float64 restatement
in tests/sim_prune_ref.py on hand-built cases (every tie rule, r = 0, r = c_a, c = 2, a zero key row) and its properties, the
constructor's and the command line's refusals with their messages, build_models, the checkpoint config key, TrainStep's refusal in the
bf16 arithmetic mode, the header and binding tables - and the model cases of the GPU tests with the conditions on their inputs asserted
in float64: every decision the stage takes (the candidate cut, the A/B boundary, every A row's partner, the pruned cut) has a margin of
more than twice what the GPU may be off by, and the stage keeps other tokens than plain attention selection does."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import attnsel_ref
from tests import sim_prune_ref as R
from tests.test_graph_rank_cpu import GR_CASES, MICRO, PROB_BOUND, REPO, built

# ---- the model cases of the GPU tests: micro1 / micro2 of tests/test_graph_rank_cpu.py (seed 400, qkv gain 10, B 3, n 17, k = 9 then 5) ----
MODEL_R = (1, 2, 3)
MODEL_ITERS = (0, 3)
COS_BOUND = 1.0e-4        # what the GPU may be off by on a cosine at model level, absolute: section 27's model tolerance
_F64 = {}


def float64_forward(name, sim_r, iters, mean_heads):
    key = (name, sim_r, iters, mean_heads)
    if key not in _F64:
        sd, _, images, _ = built(name)
        with torch.no_grad():
            _F64[key] = R.model_forward(sd, images, GR_CASES[name]["cfg"], sim_r, iters, mean_heads)
    return _F64[key]


def check_margins(out):
    """every stage, every image -> the smallest margin as a multiple of its requirement; asserts every one is above 1"""
    worst = float("inf")

    def need(gap, req, what):
        nonlocal worst
        assert gap > req, (what, gap, req)
        worst = min(worst, gap / req)
    for probs, cand, r, st in zip(out["probs"], out["cand"], out["r"], out["stages"]):
        assert r > 0 and st is not None
        B, T = probs.shape
        c = cand.shape[1]
        c_a, c_b = c // 2, c - c // 2
        for b in range(B):
            v = torch.sort(probs[b], descending=True)[0]
            if c < T:                                                    # the candidate cut: the (k + r)-th and (k + r + 1)-th probability
                need(float(v[c - 1] - v[c]), 2.0 * PROB_BOUND * float(v[c - 1]), "candidate cut")
            need(float(v[c_b - 1] - v[c_b]), 2.0 * PROB_BOUND * float(v[c_b - 1]), "A/B boundary")      # both are candidates: c_b < c
            best, second = st["best"][b], st["second"][b]
            for x, y in zip(best, second):                               # every A row's partner
                need(x - y, 2.0 * COS_BOUND, "best against second best")
            if r < c_a:                                                  # the pruned cut
                s = sorted(best, reverse=True)
                need(s[r - 1] - s[r], 2.0 * COS_BOUND, "r-th against (r + 1)-th best")
    return worst


# ---- 1. the restatement on hand-built cases ----
def _unit(*pairs):
    """a 64-vector with the given (index, value) entries"""
    v = np.zeros(64, dtype=np.float32)
    for i, x in pairs:
        v[i] = x
    return v


def _case(rows, probs, cand, r, lead=1, tail=0):
    """one image: the metric rows of its T scored tokens (fp32), placed behind `lead` rows of 7s and before `tail` rows of 7s"""
    T = len(rows)
    metric = np.full((1, lead + T + tail, 64), 7.0, dtype=np.float32)
    metric[0, lead:lead + T] = np.stack(rows)
    return dict(metric=torch.from_numpy(metric), probs=torch.tensor([probs], dtype=torch.float32),
                cand=torch.tensor([cand], dtype=torch.int64), lead=lead, r=r)


E0, E1, E2, E3 = _unit((0, 1.0)), _unit((1, 1.0)), _unit((2, 1.0)), _unit((3, 1.0))
M68, M86 = _unit((0, 0.6), (1, 0.8)), _unit((0, 0.8), (1, 0.6))
# name -> (case, expected kept, dropped, pruned, partner, sim)
TIE_CASES = {
    # B = {1, 3} hold the same row: both score 0.6 against token 0, the lower id is its partner; token 2 scores 0
    "identical_b_rows": (_case([M68, E0, E2, E0], [0.1, 0.4, 0.2, 0.3], [0, 1, 2, 3], 1), [[1, 2, 3]], [[0]], [[0]], [[1]], [[0.6]]),
    # A = {1, 3, 5}: 5 scores 0.8, 1 and 3 hold the same row and score 0.6; r = 2 prunes 5 and, of the two equal ones, the lower id
    "identical_a_rows_at_the_r_boundary": (_case([E0, M68, E2, M68, E3, M86], [0.30, 0.05, 0.25, 0.04, 0.20, 0.03], [0, 1, 2, 3, 4, 5], 2),
                                           [[0, 2, 3, 4]], [[1, 5]], [[1, 5]], [[0, 0]], [[0.6, 0.8]]),
    # probs of 1, 2, 3 are equal and c_b = 2: token 1 (the lowest id) joins 0 in B, A = {2, 3}; token 2 scores 0.8 against 1, token 3 nothing
    "equal_probs_at_the_ab_boundary": (_case([E0, E1, M68, E2], [0.4, 0.2, 0.2, 0.2], [0, 1, 2, 3], 1, tail=2),
                                       [[0, 1, 3]], [[2]], [[2]], [[1]], [[0.8]]),
    "r_zero": (_case([E0, E1, M68, M86, E2], [0.3, 0.1, 0.25, 0.15, 0.2], [0, 2, 3, 4], 0), [[0, 2, 3, 4]], [[1]], [[]], [[]], [[]]),
    # r = c_a = 2: every A row goes, whatever it scores; A = {1, 3}
    "r_is_c_a": (_case([E0, E1, M68, E2], [0.4, 0.1, 0.3, 0.2], [0, 1, 2, 3], 2), [[0, 2]], [[1, 3]], [[1, 3]], [[2, 0]], [[0.8, 0.0]]),
    # c = 2: B is the more important candidate, A the other one, and r = 1 prunes it
    "c_is_two": (_case([M68, E2, M86], [0.3, 0.5, 0.2], [0, 2], 1, lead=2), [[0]], [[1, 2]], [[2]], [[0]], [[0.96]]),
}
NAN_ROW = np.full(64, np.nan, dtype=np.float32)      # what the metric of a zero key row is
# a NaN row in B (token 1) is never a partner: 2 and 3 pair with 0; a NaN row in A (token 3) keeps best = -inf and goes last
NAN_CASES = {
    "nan_b_row": (_case([E0, NAN_ROW, M68, M86], [0.4, 0.3, 0.2, 0.1], [0, 1, 2, 3], 1), [[0, 1, 2]], [[3]], [[3]], [[0]], [[0.8]]),
    "nan_a_row_r1": (_case([E0, E1, M68, NAN_ROW], [0.4, 0.3, 0.2, 0.1], [0, 1, 2, 3], 1), [[0, 1, 3]], [[2]], [[2]], [[1]], [[0.8]]),
    "nan_a_row_r2": (_case([E0, E1, M68, NAN_ROW], [0.4, 0.3, 0.2, 0.1], [0, 1, 2, 3], 2), [[0, 1]], [[2, 3]], [[2, 3]], [[1, 0]],
                     [[0.8, -math.inf]]),
}


def check_case(out, want):
    kept, dropped, pruned, partner, sim = want
    for key, w in (("kept", kept), ("dropped", dropped), ("pruned", pruned), ("partner", partner)):
        assert torch.as_tensor(out[key]).cpu().tolist() == w, (key, torch.as_tensor(out[key]).tolist(), w)
    got = torch.as_tensor(out["sim"]).cpu().double()
    assert got.shape == (1, len(sim[0]))
    for g, w in zip(got[0].tolist(), sim[0]):
        assert g == w if math.isinf(w) else abs(g - w) <= 5e-7, (g, w)      # fp32 0.6, 0.8 and their products


@pytest.mark.parametrize("name", sorted(TIE_CASES) + sorted(NAN_CASES))
def test_ref_on_hand_built_cases(name):
    case, *want = {**TIE_CASES, **NAN_CASES}[name]
    check_case(R.stage(**case), want)


def test_ref_metric_of_a_zero_row_is_nan_and_of_any_other_a_unit_vector():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn((2 * 5, 3, 3, 64), generator=g, dtype=torch.float64)
    qkv[4, 1] = 0.0
    m = R.key_metric(qkv, 2, 5, 3)
    assert m.shape == (2, 5, 64) and bool(torch.isnan(m[0, 4]).all()) and int(torch.isnan(m).sum()) == 64
    ok = torch.ones(10, dtype=torch.bool)
    ok[4] = False
    assert torch.allclose(m.reshape(10, 64)[ok].norm(dim=-1), torch.ones(9, dtype=torch.float64), rtol=1e-14, atol=0)
    want = qkv[7, 1].mean(dim=0)
    assert torch.allclose(m[1, 2], want / want.norm(), rtol=1e-13, atol=0)
    assert R.clip_r(5, 9, 16) == 5 and R.clip_r(12, 9, 16) == 7 and R.clip_r(12, 3, 16) == 3 and R.clip_r(4, 8, 8) == 0


def random_stage_inputs(B, H, n, lead, T, c, seed):
    """fp32 inputs of one stage call: unit metric rows, positive probabilities summing to 1, the c candidates by probability"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn((B, n, 64), generator=g, dtype=torch.float64) + 0.5
    metric = (m / m.norm(dim=-1, keepdim=True)).float()
    p = torch.rand((B, T), generator=g, dtype=torch.float64) + 0.05
    probs = (p / p.sum(dim=1, keepdim=True)).float()
    cand, _ = attnsel_ref.stable_topk(probs, c)
    return metric, probs, cand


@pytest.mark.parametrize("B,n,lead,T,c,r", [(2, 18, 1, 16, 10, 1), (1, 17, 1, 16, 16, 8), (3, 40, 1, 37, 21, 5), (1, 3, 1, 2, 2, 1),
                                            (2, 9, 1, 8, 5, 0)])
def test_ref_properties(B, n, lead, T, c, r):
    metric, probs, cand = random_stage_inputs(B, 1, n, lead, T, c, 11 * T + c)
    out = R.stage(metric, probs, cand, lead, r)
    k = c - r
    assert out["kept"].shape == (B, k) and out["dropped"].shape == (B, T - k) and out["pruned"].shape == (B, r)
    for b in range(B):
        kept, dropped, cands = set(out["kept"][b].tolist()), set(out["dropped"][b].tolist()), set(cand[b].tolist())
        assert kept <= cands and len(kept) == k and kept | dropped == set(range(T)) and not kept & dropped
        assert out["kept"][b].tolist() == sorted(kept) and out["dropped"][b].tolist() == sorted(dropped)
        a_ids, b_ids = set(out["a_ids"][b]), set(out["b_ids"][b])
        assert a_ids | b_ids == cands and not a_ids & b_ids and len(a_ids) == c // 2
        assert min(float(probs[b, t]) for t in b_ids) >= max([float(probs[b, t]) for t in a_ids] or [0.0])
        assert set(out["pruned"][b].tolist()) <= a_ids and set(out["partner"][b].tolist()) <= b_ids
        assert cands - kept == set(out["pruned"][b].tolist()) and out["pruned"][b].tolist() == sorted(out["pruned"][b].tolist())
        if 0 < r < c // 2:                                               # nothing unpruned scores above anything pruned
            left = [v for a, v in zip(out["a_ids"][b], out["best"][b]) if a not in set(out["pruned"][b].tolist())]
            assert max(left) <= float(out["sim"][b].min())


# ---- 2. the model cases ----
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_the_model_cases_have_the_margins_and_keep_other_tokens_than_plain_selection(name):
    for mean in (False, True):
        for iters in MODEL_ITERS:
            plain = float64_forward(name, 0, iters, mean)
            assert plain["stages"] == [None] * len(plain["r"]) and all(r == 0 for r in plain["r"])
            for sim_r in MODEL_R:
                out = float64_forward(name, sim_r, iters, mean)
                margin = check_margins(out)
                print(f"{name} R={sim_r} T={iters} mean={mean}: smallest margin {margin:.1f} x the requirement, r = {out['r']}")
                assert out["kept"][0].shape == plain["kept"][0].shape
                assert not torch.equal(out["kept"][0], plain["kept"][0]), "the similarity stage kept exactly the importance ranking's tokens"


# ---- 3. constructor ----
def _student(**kw):
    import vit_models
    kw.setdefault("topk_selection", True)
    kw.setdefault("pruning_loc", [1])
    kw.setdefault("token_ratio", [0.05] * len(kw["pruning_loc"]))
    return vit_models.VisionTransformerDiffPruning(distill=True, predictor_loss_type="kl_div", **MICRO, **kw)


def test_constructor_default_and_refusals():
    import inspect
    import vit_models
    from vit_models import dynamic_vit
    off, on = _student(attn_selection=True), _student(attn_selection=True, sim_prune=3)
    assert off.sim_prune == 0 and on.sim_prune == 3 and on.sim_plans == [] and on.sim_prune_counts == [] and _student().sim_prune == 0
    assert list(off.state_dict()) == list(on.state_dict())
    assert _student(attn_selection=True, sim_prune=2, graph_rank_iters=3).graph_rank_iters == 3
    for kw, msg in ((dict(attn_selection=True, sim_prune=-1), dynamic_vit.SIM_PRUNE_NEGATIVE_ERROR),
                    (dict(sim_prune=-2), dynamic_vit.SIM_PRUNE_NEGATIVE_ERROR),
                    (dict(sim_prune=2), dynamic_vit.SIM_PRUNE_ATTN_SELECTION_ERROR)):
        with pytest.raises(ValueError) as e:
            _student(**kw)
        assert str(e.value) == msg
    assert "sim_prune" in msg and "attn_selection" in msg
    small = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, attn_selection=True, sim_prune=2)
    assert small.sim_prune == 2                                               # the factories forward **kwargs
    assert "sim_prune" in vit_models.VisionTransformerDiffPruning.__doc__ and "sim_plans" in vit_models.VisionTransformerDiffPruning.__doc__
    from vit_models import t2t_vit
    t2t = [c for _, c in inspect.getmembers(t2t_vit, inspect.isclass) if c.__module__ == t2t_vit.__name__]
    assert t2t and all("sim_prune" not in inspect.signature(c.__init__).parameters for c in t2t)      # the T2T student does not take it


# ---- 4. command line ----
BASE = ["--topk-selection", "--attn-selection"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_default_namespace_is_unchanged_and_the_flag_is_accepted(capsys):
    import utils
    assert "sim_prune" not in vars(utils.parse_args([])) and "sim_prune" not in vars(utils.parse_args(BASE))
    assert utils.parse_args(["--sim-prune", "4"]).sim_prune == 4
    capsys.readouterr()
    for mode in ("exact", "split"):
        a = _check(BASE + ["--sim-prune", "3", "--gemm-mode", mode, "--warmup-steps", "5"])
        out = capsys.readouterr().out
        assert a.sim_prune == 3 and a.warmup_steps == 0
        lines = [line for line in out.splitlines() if line.startswith("Attention:") and "--sim-prune" in line]
        assert len(lines) == 1 and "--sim-prune 3" in lines[0] and "Zero-TPrune" in lines[0]
    _check(BASE + ["--sim-prune", "1", "--fuse-dropped", "--mean-heads", "--drop-path", "0.1"])
    _check(BASE + ["--sim-prune", "2", "--squeeze-dropped"])
    capsys.readouterr()
    _check(BASE + ["--sim-prune", "8", "--graph-rank", "5"])
    out = capsys.readouterr().out
    assert len([line for line in out.splitlines() if line.startswith("Attention:") and "--sim-prune" in line]) == 1
    assert len([line for line in out.splitlines() if line.startswith("Attention:") and "--graph-rank 5" in line]) == 1
    _check(BASE)
    assert "sim-prune" not in capsys.readouterr().out                         # nothing new without the flag


@pytest.mark.parametrize("argv,fragment", [
    (BASE + ["--sim-prune", "0"], "--sim-prune 0 (at least 1 candidate pruned by similarity)"),
    (BASE + ["--sim-prune", "-2"], "--sim-prune -2 (at least 1 candidate pruned by similarity)"),
    (["--topk-selection", "--sim-prune", "2"], "--sim-prune without --attn-selection"),
    (["--sim-prune", "2"], "--sim-prune without --attn-selection"),
    (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--sim-prune", "2"], "--sim-prune with --method tome"),
    (["--method", "evo", "--sim-prune", "2"], "--sim-prune with --method evo"),
    (["--method", "dynamicvit", "--sim-prune", "2"], "--sim-prune with --method dynamicvit"),
    (BASE + ["--sim-prune", "2", "--gemm-mode", "bf16"], "--sim-prune with --gemm-mode bf16"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_build_models_passes_the_flag(monkeypatch):
    import mask_predictor
    import utils
    import vit_models
    seen = {}

    def fake_student(locs, ratios, **kw):
        seen.clear()
        seen.update(kw)
        return torch.nn.Identity()
    monkeypatch.setattr(vit_models, "dynamic_vit_small_patch16_224_student", fake_student)
    monkeypatch.setattr(vit_models, "dynamic_vit_small_patch16_224_teacher", lambda **kw: torch.nn.Identity())
    for flags, want, rank in ((BASE + ["--sim-prune", "5"], 5, 0), (BASE + ["--sim-prune", "2", "--graph-rank", "4"], 2, 4), (BASE, 0, 0),
                              (["--topk-selection"], 0, 0)):
        a = utils.parse_args(["--arch", "deit_small"] + flags)
        a.device = "cpu"
        mask_predictor.build_models(a)
        assert seen.get("sim_prune", 0) == want and seen.get("graph_rank_iters", 0) == rank
        assert seen["attn_selection"] == ("--attn-selection" in flags)


# ---- 5. checkpoint config, TrainStep ----
def test_checkpoint_config_records_the_key_only_when_positive():
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    off, on = cfg(_student(attn_selection=True)), cfg(_student(attn_selection=True, sim_prune=3))
    both = cfg(_student(attn_selection=True, sim_prune=3, graph_rank_iters=2))
    assert "sim_prune" not in off and "sim_prune" not in cfg(_student()) and on["sim_prune"] == 3
    assert list(on)[:-1] == list(off) and list(on)[-1] == "sim_prune"                  # every recorded key keeps its place
    assert list(both)[:-2] == list(off) and list(both)[-2:] == ["graph_rank_iters", "sim_prune"]
    assert {k for k in off if off[k] != on[k]} == set() and json.loads(json.dumps(on)) == on
    assert engine.sim_prune(off) == 0 and engine.sim_prune(on) == 3 and engine.sim_prune(both) == 3 and engine.graph_rank_iters(both) == 2
    plain = cfg(_student())
    old = {k: v for k, v in plain.items() if k not in ("attn_selection", "mean_heads")}    # a checkpoint written before either feature
    assert engine.sim_prune(engine.checkpoint_config(old)) == 0 and engine.checkpoint_config(old) == plain
    assert engine.checkpoint_config(on) == on


def test_train_step_refuses_the_bf16_mode_before_the_device():
    from d2s import functional_sim_prune as SF
    from d2s import lib, ops
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            TrainStep(_student(attn_selection=True, sim_prune=2), torch.nn.Identity(), args)
        assert str(e.value) == SF.SIM_PRUNE_BF16_ERROR
        with pytest.raises(lib.D2SError) as e:                                  # the block itself, whoever calls it
            SF.refuse_bf16()
        assert str(e.value) == SF.SIM_PRUNE_BF16_ERROR
    SF.refuse_bf16()
    assert "sim_prune" in SF.SIM_PRUNE_BF16_ERROR and "--sim-prune" in SF.SIM_PRUNE_BF16_ERROR
    with pytest.raises(ValueError, match="warmup_steps"):                         # inherited from attention selection
        TrainStep(_student(attn_selection=True, sim_prune=2), torch.nn.Identity(), args, warmup_steps=1)


# ---- 6. header and binding ----
def test_header_and_binding_list_the_same_entries():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_sim_prune.h")).read()
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 3                       # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "sim_prune.hip")).read()
    for name in lib.symbols("d2s_hip_sim_prune.h"):
        assert lib.signature(name)[0] is lib.I and len(re.findall(rf"^int {name}\(", src, flags=re.M)) == 1
    low = src.lower().replace("no atomics", "").replace("no memset", "")
    assert "atomic" not in low and "memset" not in low and "asm" not in low
    assert callable(ops.key_metric) and callable(ops.sim_prune) and ops.sim_prune_clip_r(12, 9, 16) == 7
