"""Graph ranking (--graph-rank T), the parts that need no GPU: the float64 restatement in tests/graph_rank_ref.py on
hand-computed graphs and its properties (uniform attention, mass, T = 1, the composition identity), the constructor's and the command
line's refusals with their messages, build_models, the checkpoint config key, TrainStep's refusal in the bf16 arithmetic mode, the header
and binding tables - and the model cases of the GPU tests with the conditions on their inputs asserted: in float64 every image's k-th and
(k + 1)-th probability are further apart than twice what the GPU may be off by, and the ranked ids are not the CLS-attention ids."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import graph_rank_ref as R
from tests.test_ltp_cpu import make_qkv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 0.125
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)

# ---- the model cases of the GPU tests ----
# The micro1 / micro2 geometries of tests/test_attnsel_gpu.py (D 128, H 2, depth 4, N 17, B 3; one stage at block 1, two at blocks 1 and 2).
# Random 0.02-std weights give near-uniform attention, so the qkv weights are scaled by 10 (as tests/test_ltp_cpu.py does); the seed was
# picked on the CPU with the float64 restatement alone so that check_gaps holds.
QKV_GAIN = 10.0
GR_CASES = {name: dict(cfg=cases.MODEL_CASES[name]["cfg"], batch=3, seed=400) for name in ("micro1", "micro2")}
MODEL_ITERS = (1, 3)
# What the GPU may be off by on a stage's probability, relative: the model tests hold graph_ranks to rtol 1e-4 against float64 (the
# tolerance of the model tests of tests/test_ltp_gpu.py), a probability is one reduced rank over the sum of the reduced ranks - 1e-4 from
# the numerator, 1e-4 from the normaliser - and d2s_select_cls_attn adds (H + T + 2) 2^-24 < 2e-6 of its own (tests/test_attnsel_gpu.py).
PROB_BOUND = 2.0e-4 + 2.0e-6
_BUILT = {}


def built(name):
    """(state dict fp32 with the scaled qkv weights, teacher state dict, images, labels) of a model case, once"""
    if name not in _BUILT:
        case = GR_CASES[name]
        sd_s, sd_t = cases.make_weights(case)
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_s.items()}
        for k in sd:
            if k.endswith("attn.qkv.weight"):
                sd[k] = sd[k] * QKV_GAIN
        sd_t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_t.items()}
        _BUILT[name] = (sd, sd_t, torch.from_numpy(cases.make_images(case)), torch.from_numpy(cases.make_labels(case)).long())
    return _BUILT[name]


_F64 = {}


def float64_forward(name, iters, mean_heads):
    key = (name, iters, mean_heads)
    if key not in _F64:
        sd, _, images, _ = built(name)
        with torch.no_grad():
            _F64[key] = R.model_forward(sd, images, GR_CASES[name]["cfg"], iters, mean_heads)
    return _F64[key]


def check_gaps(out):
    """every stage, every image: p_(k) - p_(k+1) > 2 PROB_BOUND p_(k) -> the smallest such margin as a multiple of the requirement"""
    worst = float("inf")
    for probs, kept in zip(out["probs"], out["kept"]):
        k = kept.shape[1]
        top = torch.sort(probs, dim=1, descending=True)[0][:, k - 1]
        need = 2.0 * PROB_BOUND * top
        gap = R.kth_gap(probs, k)
        assert bool((gap > need).all()), (gap.tolist(), need.tolist())
        worst = min(worst, float((gap / need).min()))
    return worst


# ---- 1. the restatement ----
def test_ref_on_a_two_node_graph_and_a_three_node_chain():
    P = torch.tensor([[[[0.5, 0.5], [0.25, 0.75]]]], dtype=torch.float64)
    s1, s2 = R.iterate(P, 2, trace=True)
    assert s1.tolist() == [[[0.375, 0.625]]] and s2.tolist() == [[[0.34375, 0.65625]]]
    assert R.iterate(P, 1, w0=torch.tensor([[[1.0, 0.0]]])).tolist() == [[[0.5, 0.5]]]
    # 0 -> 1 -> 2 -> 2: the mass walks down the chain and stays at its end
    chain = torch.tensor([[[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]]], dtype=torch.float64)
    third = 1.0 / 3.0
    s1, s2, s3 = R.iterate(chain, 3, trace=True)
    assert s1.tolist() == [[[0.0, third, third + third]]]
    assert s2[0, 0, :2].tolist() == [0.0, 0.0] and abs(float(s2[0, 0, 2]) - 1.0) < 1e-15 and torch.equal(s3, s2)


@pytest.mark.parametrize("B,n,H", [(1, 2, 1), (2, 33, 2), (1, 65, 3)])
def test_ref_properties(B, n, H):
    qkv = make_qkv(B * n, H, 5 * n + H)
    P = R.probabilities(qkv, B, n, H, SCALE)
    assert P.shape == (B, H, n, n) and torch.allclose(P.sum(dim=-1), torch.ones((B, H, n), dtype=torch.float64), rtol=1e-13, atol=0)
    for s in R.iterate(P, 6, trace=True):                       # mass 1 after every iteration, no renormalisation
        assert torch.allclose(s.sum(dim=-1), torch.ones((B, H), dtype=torch.float64), rtol=1e-12, atol=0) and bool((s > 0).all())
    assert torch.allclose(R.rank(qkv, B, n, H, SCALE, 1), P.mean(dim=2), rtol=1e-13, atol=0)      # T = 1: the per-head mean of P's columns
    zero_q = qkv.clone()
    zero_q[:, 0] = 0.0                                           # q = 0: uniform P, and 1 / n is its fixed point
    for T in (1, 2, 7):
        assert torch.allclose(R.rank(zero_q, B, n, H, SCALE, T), torch.full((B, H, n), 1.0 / n, dtype=torch.float64), rtol=1e-13, atol=0)
    for a, b in ((1, 1), (2, 3), (4, 1)):                       # rank(T = a + b) = rank(T = b, w0 = rank(T = a))
        assert torch.allclose(R.rank(qkv, B, n, H, SCALE, a + b), R.rank(qkv, B, n, H, SCALE, b, w0=R.rank(qkv, B, n, H, SCALE, a)),
                              rtol=1e-13, atol=0)
    if n > 2:
        assert not torch.allclose(R.rank(qkv, B, n, H, SCALE, 1), R.rank(qkv, B, n, H, SCALE, 5), rtol=1e-3, atol=0)      # the iteration moves


# ---- 2. the model cases ----
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_the_model_cases_have_the_gaps_and_rank_differently_from_the_cls_row(name):
    differs = False
    for mean in (False, True):
        cls = float64_forward(name, 0, mean)
        for iters in MODEL_ITERS:
            out = float64_forward(name, iters, mean)
            margin = check_gaps(out)
            print(f"{name} T={iters} mean={mean}: smallest k-th gap {margin:.1f} x the requirement")
            for r in out["ranks"]:
                assert torch.allclose(r.sum(dim=-1), torch.ones(r.shape[:2], dtype=torch.float64), rtol=1e-12, atol=0)
            differs = differs or not torch.equal(out["kept"][0], cls["kept"][0])
    assert differs, "graph ranking kept exactly the CLS row's tokens for every image: the flag would do nothing"


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
    off, on = _student(attn_selection=True), _student(attn_selection=True, graph_rank_iters=3)
    assert off.graph_rank_iters == 0 and on.graph_rank_iters == 3 and on.graph_ranks == [] and _student().graph_rank_iters == 0
    assert list(off.state_dict()) == list(on.state_dict())
    for kw, msg in ((dict(attn_selection=True, graph_rank_iters=-1), dynamic_vit.GRAPH_RANK_NEGATIVE_ERROR),
                    (dict(graph_rank_iters=-2), dynamic_vit.GRAPH_RANK_NEGATIVE_ERROR),
                    (dict(graph_rank_iters=2), dynamic_vit.GRAPH_RANK_ATTN_SELECTION_ERROR)):
        with pytest.raises(ValueError) as e:
            _student(**kw)
        assert str(e.value) == msg
    assert "graph_rank_iters" in msg and "attn_selection" in msg
    small = vit_models.dynamic_vit_small_patch16_224_student([3], [0.5], topk_selection=True, attn_selection=True, graph_rank_iters=2)
    assert small.graph_rank_iters == 2                                        # the factories forward **kwargs
    assert "graph_rank_iters" in vit_models.VisionTransformerDiffPruning.__doc__
    from vit_models import t2t_vit
    t2t = [c for _, c in inspect.getmembers(t2t_vit, inspect.isclass) if c.__module__ == t2t_vit.__name__]
    assert t2t and all("graph_rank_iters" not in inspect.signature(c.__init__).parameters for c in t2t)      # the T2T student does not take it


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
    assert "graph_rank" not in vars(utils.parse_args([])) and "graph_rank" not in vars(utils.parse_args(BASE))
    assert utils.parse_args(["--graph-rank", "4"]).graph_rank == 4
    capsys.readouterr()
    for mode in ("exact", "split"):
        a = _check(BASE + ["--graph-rank", "3", "--gemm-mode", mode, "--warmup-steps", "5"])
        out = capsys.readouterr().out
        assert a.graph_rank == 3 and a.warmup_steps == 0
        lines = [line for line in out.splitlines() if line.startswith("Attention:") and "--graph-rank" in line]
        assert len(lines) == 1 and "--graph-rank 3" in lines[0] and "PageRank" in lines[0]
    _check(BASE + ["--graph-rank", "1", "--fuse-dropped", "--mean-heads", "--drop-path", "0.1"])
    capsys.readouterr()
    _check(BASE)
    assert "graph-rank" not in capsys.readouterr().out                       # nothing new without the flag


@pytest.mark.parametrize("argv,fragment", [
    (BASE + ["--graph-rank", "0"], "--graph-rank 0 (at least 1 PageRank iteration)"),
    (BASE + ["--graph-rank", "-2"], "--graph-rank -2 (at least 1 PageRank iteration)"),
    (["--topk-selection", "--graph-rank", "2"], "--graph-rank without --attn-selection"),
    (["--graph-rank", "2"], "--graph-rank without --attn-selection"),
    (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--graph-rank", "2"], "--graph-rank with --method tome"),
    (["--method", "evo", "--graph-rank", "2"], "--graph-rank with --method evo"),
    (["--method", "dynamicvit", "--graph-rank", "2"], "--graph-rank with --method dynamicvit"),
    (BASE + ["--graph-rank", "2", "--gemm-mode", "bf16"], "--graph-rank with --gemm-mode bf16"),
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
    for flags, want in ((BASE + ["--graph-rank", "5"], 5), (BASE, 0), (["--topk-selection"], 0)):
        a = utils.parse_args(["--arch", "deit_small"] + flags)
        a.device = "cpu"
        mask_predictor.build_models(a)
        assert seen.get("graph_rank_iters", 0) == want and seen["attn_selection"] == ("--attn-selection" in flags)


# ---- 5. checkpoint config, TrainStep ----
def test_checkpoint_config_records_the_key_only_when_positive():
    from d2s import engine
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    cfg = lambda s: engine.TrainStep.config(types.SimpleNamespace(student=s, args=args))
    off, on = cfg(_student(attn_selection=True)), cfg(_student(attn_selection=True, graph_rank_iters=3))
    assert "graph_rank_iters" not in off and "graph_rank_iters" not in cfg(_student()) and on["graph_rank_iters"] == 3
    assert list(on)[:-1] == list(off) and list(on)[-1] == "graph_rank_iters"         # every recorded key keeps its place
    assert {k for k in off if off[k] != on[k]} == set() and json.loads(json.dumps(on)) == on
    assert engine.graph_rank_iters(off) == 0 and engine.graph_rank_iters(on) == 3
    plain = cfg(_student())
    old = {k: v for k, v in plain.items() if k not in ("attn_selection", "mean_heads")}    # a checkpoint written before either feature
    assert engine.graph_rank_iters(engine.checkpoint_config(old)) == 0 and engine.checkpoint_config(old) == plain
    assert engine.checkpoint_config(on) == on


def test_train_step_refuses_the_bf16_mode_before_the_device():
    from d2s import functional_graph_rank as GF
    from d2s import lib, ops
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            TrainStep(_student(attn_selection=True, graph_rank_iters=2), torch.nn.Identity(), args)
        assert str(e.value) == GF.GRAPH_RANK_BF16_ERROR
        with pytest.raises(lib.D2SError) as e:                                  # the block itself, whoever calls it
            GF.refuse_bf16()
        assert str(e.value) == GF.GRAPH_RANK_BF16_ERROR
    GF.refuse_bf16()
    with pytest.raises(ValueError, match="warmup_steps"):                         # inherited from attention selection
        TrainStep(_student(attn_selection=True, graph_rank_iters=2), torch.nn.Identity(), args, warmup_steps=1)


# ---- 6. header and binding ----
def test_header_and_binding_list_the_same_entry():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_graph_rank.h")).read()
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 2                       # the file's comment and the entry's
    assert "D2S_ERR_ARG" in text
    assert lib.symbols("d2s_hip_graph_rank.h") == ["d2s_graph_rank_f32"] and lib.signature("d2s_graph_rank_f32")[0] is lib.I
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "graph_rank.hip")).read()
    assert len(re.findall(r"^int d2s_graph_rank_f32\(", src, flags=re.M)) == 1
    low = src.lower().replace("no atomics", "").replace("no memset", "")
    assert "atomic" not in low and "memset" not in low and "asm" not in low
    assert callable(ops.graph_rank)
