"""The similarity stage after attention ranking on the GPU (--sim-prune R) against the float64 restatement of
tests/sim_prune_ref.py.
The metric kernel: every component within (H + 4) 2^-24 of float64, a zero key row NaN, two calls bit for bit.
The stage kernels on exact fp32 inputs whose float64 scores have gaps of at least 2 E between every A row's best and second best and at
the pruned cut, E = (64 + H + 4) 2^-24 with H = 1 (section 22's bound for a 64-term dot of unit vectors, whatever the summation order;
the stage call has no H of its own, so the tightest one is used): sim within E, every list equal to float64 - at c_a, c_b on both sides
of 32 and 64, r in {1, c_a - 1, c_a}, trailing unscored rows, and one large case.  The tie rules and the NaN rows of
tests/test_sim_prune_cpu.py on the device, d2s_select_topk on the emitted best, two calls bit for bit, guard bands, every refusal.
The model in the micro1 / micro2 geometries (tests/test_sim_prune_cpu.py asserts the conditions on their inputs): lists and plans
against float64 on every image, the metric against float64 from the block's own input, the route against the plain attention-selecting
model bit for bit under one replayed selection (with stochastic depth too), token fusion, squeezing, graph ranking, the argument at 0.
TrainStep (three steps, two runs, save and resume, the captured step, the bf16 refusal) and the command line."""
import math
import os

import pytest
import torch

from tests import sim_prune_ref as R
from tests.test_graph_rank_cpu import GR_CASES, built, make_qkv
from tests.test_graph_rank_gpu import _common, _gm, _run, _teacher
from tests.test_model_gpu import make_args
from tests.test_sim_prune_cpu import MODEL_ITERS, MODEL_R, NAN_CASES, TIE_CASES, check_case, float64_forward, random_stage_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = 2.0 ** -24
E_DOT = (64 + 1 + 4) * EPS
GUARD, POISON, UNSET = 64, 1234.5, -7777      # an int64 buffer holds int(POISON) in its guard bands
TOL = 1e-4          # a cosine (and a metric component) computed from the model's own activations: section 27's model tolerance
MODES = ("exact", "split")
SIM_R = 2
WORST = {}


def _note(tag, v):
    WORST[tag] = max(WORST.get(tag, 0.0), float(v))
    print(f"  {tag}: {float(v):.3e} (worst over the tests so far {WORST[tag]:.3e})")


# ---- 1. the metric kernel ----
@pytest.mark.parametrize("B,H,n", [(1, 1, 1), (1, 6, 1), (3, 1, 17), (3, 6, 17), (1, 6, 197), (3, 1, 32), (1, 12, 577)])
def test_metric_against_float64(B, H, n):
    from d2s import ops
    qkv64 = make_qkv(B * n, H, 100 * n + 10 * H + B)
    qkv = qkv64.float().reshape(B * n, -1).contiguous().to(DEV)
    got = ops.key_metric(qkv, B, n, H)
    assert got.shape == (B, n, 64) and got.dtype == torch.float32
    err = (got.double().cpu() - R.key_metric(qkv64, B, n, H)).abs().max()
    _note(f"metric H={H}, in units of (H + 4) 2^-24", err / ((H + 4) * EPS))
    assert bool(torch.isfinite(got).all()) and float(err) <= (H + 4) * EPS
    assert torch.equal(ops.key_metric(qkv, B, n, H), got)                                   # two calls: the same bits
    q0 = qkv.clone().view(B * n, 3, H, 64)
    q0[B * n - 1, 1] = 0.0                                                                   # a zero key row: NaN, and only there
    nan = torch.isnan(ops.key_metric(q0.view(B * n, -1), B, n, H)).view(B * n, 64)
    assert bool(nan[B * n - 1].all()) and int(nan.sum()) == 64


def test_metric_refusals_and_guard_bands():
    from d2s import lib
    B, H, n = 2, 2, 17
    qkv = make_qkv(B * n, H, 8).float().reshape(B * n, -1).contiguous().to(DEV)
    size = B * n * 64
    out = torch.full((size + 2 * GUARD,), POISON, dtype=torch.float32, device=DEV)
    fn = lib._fn("d2s_key_metric_f32")
    good = dict(qkv=lib.ptr(qkv), B=B, n=n, H=H, metric=lib.ptr(out[GUARD:]))
    for change in (dict(qkv=None), dict(metric=None), dict(B=0), dict(B=-1), dict(n=0), dict(H=0), dict(metric=lib.ptr(qkv)),
                   dict(metric=lib.ptr(qkv.view(-1)[64:]))):
        a = dict(good, **change)
        assert fn(a["qkv"], a["B"], a["n"], a["H"], a["metric"], lib.stream()) == -1, sorted(change)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert fn(good["qkv"], B, n, H, good["metric"], lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == POISON).all()) and bool((out[GUARD + size:] == POISON).all())
    assert bool(torch.isfinite(out[GUARD:GUARD + size]).all()) and not bool((out[GUARD:GUARD + size] == POISON).any())


# ---- 2. the stage kernels against float64 ----
def _stage_shapes():
    shapes = [(T + 1, 1, T, c, r) for (T, c, r) in ((1, 1, 0), (2, 2, 1), (16, 10, 1), (16, 16, 8))]
    for c in (63, 64, 65, 66, 127, 129, 130):
        for r in (1, c // 2 - 1, c // 2):
            shapes.append((c + 5 + 1 + 2, 1, c + 5, c, r))                                  # lead 1, two trailing unscored rows
    return [(B,) + s for B in (1, 3) for s in shapes] + [(1, 577, 1, 576, 400, 100)]


_STAGE = {}


def _gaps_ok(ref, r):
    """every A row's best against its second best, and the r-th against the (r + 1)-th best, at least 2 E_DOT apart"""
    for best, second in zip(ref["best"], ref["second"]):
        if any(x - y < 2 * E_DOT for x, y in zip(best, second)):
            return False
        s = sorted(best, reverse=True)
        if 0 < r < len(s) and s[r - 1] - s[r] < 2 * E_DOT:
            return False
    return True


def _stage_case(B, n, lead, T, c, r):
    """(metric, probs, cand fp32 / int64 on the CPU, the float64 result), once per shape; the seed is the first from the shape's base
    whose float64 scores have the gaps - picked with the restatement alone"""
    key = (B, n, lead, T, c, r)
    if key not in _STAGE:
        base = 7 * T + 3 * c + r + B
        for seed in range(base, base + 20):
            metric, probs, cand = random_stage_inputs(B, 1, n, lead, T, c, seed)
            ref = R.stage(metric, probs, cand, lead, max(r, 0))
            if _gaps_ok(ref, r):
                break
        else:
            raise AssertionError(f"no seed with the gaps for {key}")
        _STAGE[key] = (metric, probs, cand, ref)
    return _STAGE[key]


def _same_lists(got, ref):
    kept, dropped, pruned, partner, sim = got
    for name, g in (("kept", kept), ("dropped", dropped), ("pruned", pruned), ("partner", partner)):
        assert g.dtype == torch.int64 and torch.equal(g.cpu(), ref[name]), (name, g.cpu().tolist(), ref[name].tolist())
    assert sim.dtype == torch.float32 and sim.shape == ref["sim"].shape


@pytest.mark.parametrize("B,n,lead,T,c,r", _stage_shapes())
def test_stage_against_float64(B, n, lead, T, c, r):
    from d2s import ops
    metric, probs, cand, ref = _stage_case(B, n, lead, T, c, r)
    dev = (metric.to(DEV), probs.to(DEV), cand.to(DEV))
    got = ops.sim_prune(*dev, lead, r)
    torch.cuda.synchronize()
    if r > 0:
        err = (got[4].double().cpu() - ref["sim"]).abs().max()
        _note("sim in units of E", err / E_DOT)
        assert float(err) <= E_DOT
    _same_lists(got, ref)
    again = ops.sim_prune(*dev, lead, r)                                                   # two calls: the same bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if r == c // 2 and r > 1:
        # r = c_a emits every A row's best, in ascending id: d2s_select_topk on it picks the pruned set of any smaller count bit for bit
        for r2 in {1, r - 1}:
            less = ops.sim_prune(*dev, lead, r2)
            pos = ops.select_topk(got[4], r2)[0]
            assert torch.equal(torch.gather(got[2], 1, pos), less[2]) and torch.equal(torch.gather(got[3], 1, pos), less[3])
            assert torch.equal(torch.gather(got[4], 1, pos), less[4])


@pytest.mark.parametrize("name", sorted(TIE_CASES) + sorted(NAN_CASES))
def test_tie_rules_and_nan_rows_on_the_device(name):
    from d2s import ops
    case, *want = {**TIE_CASES, **NAN_CASES}[name]
    got = ops.sim_prune(case["metric"].to(DEV), case["probs"].to(DEV), case["cand"].to(DEV), case["lead"], case["r"])
    torch.cuda.synchronize()
    check_case(dict(zip(("kept", "dropped", "pruned", "partner", "sim"), got)), want)


NAMES = ("kept", "dropped", "pruned", "partner", "sim")


def _buffers(B, T, c, r):
    """the five outputs of one legal call, unset (ids UNSET, sim NaN) between poisoned guard bands -> ({name: whole buffer}, {name: length})"""
    sizes = dict(kept=B * (c - r), dropped=B * (T - c + r), pruned=B * r, partner=B * r, sim=B * r)
    bufs = {}
    for k, size in sizes.items():
        t = (torch.full((size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV) if k == "sim"
             else torch.full((size + 2 * GUARD,), UNSET, dtype=torch.int64, device=DEV))
        t[:GUARD] = POISON
        t[GUARD + size:] = POISON
        bufs[k] = t
    return bufs, sizes


def _call(ins, counts, bufs, null=(), alias=None):
    """the C entry on `bufs` with any counts (B, n, lead, T, c, r) -> rc"""
    from d2s import lib
    ptrs = {k: (None if k in null else lib.ptr(bufs[k][GUARD:])) for k in NAMES}
    ptrs.update(alias or {})
    rc = lib._fn("d2s_sim_prune_f32")(*(lib.ptr(t) for t in ins), *counts, *(ptrs[k] for k in NAMES), lib.stream())
    torch.cuda.synchronize()
    return rc


def _guards_intact(bufs, sizes):
    return all(bool((t[:GUARD] == int(POISON)).all()) and bool((t[GUARD + sizes[k]:] == int(POISON)).all()) if k != "sim" else
               bool((t[:GUARD] == POISON).all()) and bool((t[GUARD + sizes[k]:] == POISON).all()) for k, t in bufs.items())


def _untouched(bufs, sizes):
    bodies = {k: t[GUARD:GUARD + sizes[k]] for k, t in bufs.items()}
    return _guards_intact(bufs, sizes) and all(bool((torch.isnan(b) if k == "sim" else b == UNSET).all()) for k, b in bodies.items())


@pytest.mark.parametrize("B,n,lead,T,c,r", [(3, 19, 1, 16, 10, 1), (3, 72, 1, 69, 64, 32), (1, 3, 1, 2, 2, 1), (3, 19, 1, 16, 10, 0)])
def test_only_the_outputs_are_written(B, n, lead, T, c, r):
    from d2s import ops
    metric, probs, cand, _ = _stage_case(B, n, lead, T, c, r)
    dev = (metric.to(DEV), probs.to(DEV), cand.to(DEV))
    bufs, sizes = _buffers(B, T, c, r)
    assert _call(dev, (B, n, lead, T, c, r), bufs) == 0 and _guards_intact(bufs, sizes)
    want = dict(zip(NAMES, ops.sim_prune(*dev, lead, r)))
    for k, t in bufs.items():
        assert torch.equal(t[GUARD:GUARD + sizes[k]], want[k].reshape(-1)), k              # every element written, nothing else
    if r == 0:
        assert torch.equal(want["kept"], dev[2])                                            # r == 0 copies cand to kept
        bufs, sizes = _buffers(B, T, c, r)
        assert _call(dev, (B, n, lead, T, c, r), bufs, null=("pruned", "partner", "sim")) == 0      # ... and needs no plan
        assert torch.equal(bufs["kept"][GUARD:GUARD + sizes["kept"]], dev[2].reshape(-1)) and _guards_intact(bufs, sizes)


def test_refusals_leave_the_outputs_alone():
    from d2s import lib
    B, n, lead, T, c, r = 2, 19, 1, 16, 10, 3
    ins = tuple(t.to(DEV) for t in random_stage_inputs(B, 1, n, lead, T, c, 5))
    metric, probs, cand = ins
    good = dict(B=B, n=n, lead=lead, T=T, c=c, r=r)
    order = ("B", "n", "lead", "T", "c", "r")
    # the buffers keep the good call's sizes: a refused call writes nothing whatever its counts say
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(lead=-1), dict(lead=4), dict(n=16), dict(T=1025, n=1026), dict(T=9), dict(c=0),
           dict(c=17), dict(r=-1), dict(r=6), dict(null=("kept",)), dict(null=("dropped",)), dict(null=("pruned",)), dict(null=("partner",)),
           dict(null=("sim",)), dict(alias=dict(kept=lib.ptr(cand))), dict(alias=dict(dropped=lib.ptr(cand.view(-1)[3:]))),
           dict(alias=dict(sim=lib.ptr(probs))), dict(alias=dict(partner=lib.ptr(metric))), dict(alias=dict(pruned=lib.ptr(probs.view(-1)[8:]))),
           dict(ins=(None, probs, cand)), dict(ins=(metric, None, cand)), dict(ins=(metric, probs, None))]
    before = [t.clone() for t in ins]
    for change in bad:
        counts = tuple(dict(good, **{k: v for k, v in change.items() if k in good})[k] for k in order)
        bufs, sizes = _buffers(B, T, c, r)
        rc = _call(change.get("ins", ins), counts, bufs, null=change.get("null", ()), alias=change.get("alias"))
        assert rc == -1, (sorted(change), rc)
        assert _untouched(bufs, sizes), sorted(change)
    assert all(torch.equal(a, b) for a, b in zip(before, ins))                             # ... the aliased inputs included
    bufs, sizes = _buffers(B, T, c, r)
    assert _call(ins, (B, n, lead, T, c, r), bufs) == 0 and not _untouched(bufs, sizes)    # the same call, legal
    bufs, sizes = _buffers(B, T, c, 5)
    assert _call(ins, (B, n, lead, T, c, 5), bufs) == 0                                    # r = c / 2 is the limit


# ---- 3. the model, micro geometries ----
def _student(name, **kw):
    """The case's weights in an attention-selecting student built with **kw"""
    import vit_models
    cfg = GR_CASES[name]["cfg"]
    kw.setdefault("pruning_loc", list(cfg["pruning_loc"]))
    kw.setdefault("token_ratio", list(cfg["token_ratio"]))
    kw.setdefault("init_n", cfg["init_n"])
    kw.setdefault("attn_selection", True)
    m = vit_models.VisionTransformerDiffPruning(distill=True, topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                small_predictor=cfg["small_predictor"], **_common(cfg), **kw)
    m.load_state_dict(built(name)[0], strict=True)
    return m.to(DEV)


def _images(name):
    return built(name)[2].to(DEV)


def _spy_metric_block(monkeypatch):
    """records (input x, metric) of every block that emits a metric, in stage order"""
    from d2s import functional_sim_prune as SF
    seen, orig = [], SF.metric_block

    def spy(x, *a, **kw):
        out = orig(x, *a, **kw)
        seen.append((x.detach().clone(), out[2]))
        return out
    monkeypatch.setattr(SF, "metric_block", spy)
    return seen


@pytest.mark.parametrize("iters", MODEL_ITERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_student_prunes_by_similarity(name, mode, iters, monkeypatch):
    from d2s import ops
    from tests import graph_rank_ref
    cfg = GR_CASES[name]["cfg"]
    locs = list(cfg["pruning_loc"])
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    sd64 = {k: v.double() for k, v in built(name)[0].items()}
    x = _images(name)
    seen = _spy_metric_block(monkeypatch)
    for sim_r in MODEL_R:
        for mean in (False, True):
            student = _student(name, sim_prune=sim_r, graph_rank_iters=iters, mean_heads=mean).eval()
            del seen[:]
            with ops.gemm_mode(_gm(mode)), torch.no_grad():
                out = student(x)
            torch.cuda.synchronize()
            pred, kept = out[2], out[3]
            want = float64_forward(name, sim_r, iters, mean)
            assert bool(torch.isfinite(out[0]).all()) and len(student.sim_plans) == len(pred) == len(kept) == len(seen) == len(locs)
            assert student.sim_prune_counts == want["r"] and len(student.graph_ranks) == (len(locs) if iters else 0)
            for s, loc in enumerate(locs):
                xin, metric = seen[s]
                B, n, _ = xin.shape
                T, r, st = n - 1, want["r"][s], want["stages"][s]
                assert metric.shape == (B, n, 64) and not metric.requires_grad and pred[s].shape == (B, T) and kept[s].shape == (B, ks[s])
                # float64 from the block's own input: LayerNorm 1, the qkv projection, the metric
                ref = R.key_metric(graph_rank_ref.block_qkv(sd64, loc - 1, xin.cpu().double(), cfg), B, n, cfg["heads"])
                err = (metric.double().cpu() - ref).abs().max()
                _note(f"{name} {mode} stage {s} metric", err)
                assert float(err) <= TOL
                pruned, partner, sim = student.sim_plans[s]
                assert not sim.requires_grad and pruned.shape == partner.shape == sim.shape == (B, r)
                _same_lists((kept[s], student.dropped_token_indices[s], pruned, partner, sim), st)      # every image, float64 all the way
                err = (sim.double().cpu() - st["sim"]).abs().max()
                _note(f"{name} {mode} stage {s} sim", err)
                assert float(err) <= TOL
                assert torch.equal(kept[s].cpu(), want["kept"][s])
                # the stage is these two calls on the model's own row and metric
                row, lead = (student.graph_ranks[s], 1) if iters else (student.cls_attns[loc - 1].contiguous(), 0)
                p2, c2, _ = ops.select_cls_attn(row, lead, T, ks[s] + r, mean)
                again = ops.sim_prune(metric, p2, c2, 1, r)
                assert torch.equal(p2, pred[s]) and torch.equal(again[0], kept[s]) and torch.equal(again[1], student.dropped_token_indices[s])


@pytest.mark.parametrize("drop_path", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_the_metric_route_does_not_move_the_block(name, drop_path):
    """the same replayed selection in a similarity-pruning model and in a plain attention-selecting one: the block before a stage runs
    through the per-op sequence in one and through the one-call composite in the other, and nothing downstream may tell"""
    cfg = GR_CASES[name]["cfg"]
    x = _images(name)
    override = [k.clone() for k in float64_forward(name, SIM_R, 0, False)["kept"]]
    g = torch.Generator().manual_seed(3)
    w = torch.randn((x.shape[0], cfg["num_classes"]), generator=g).to(DEV)
    masks = None
    if drop_path > 0:      # the fixed table of tests/test_graph_rank_gpu.py: micro2's block 1 loses one image's attention branch, another's MLP
        masks = (torch.rand((2 * cfg["depth"], x.shape[0]), generator=g) < 0.5).float()
        masks[2:4] = torch.tensor([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0]])
    results = []
    for sim_r in (SIM_R, 0):
        student = _student(name, sim_prune=sim_r, drop_path_rate=drop_path)
        student.kept_token_override = override
        results.append(_run(student, x, w, masks))
        assert len(student.sim_plans) == (len(cfg["pruning_loc"]) if sim_r else 0)
        student.eval()
        with torch.no_grad():
            results[-1] += (student(x)[0], [c.clone() for c in student.cls_attns])
    (la, ca, ga, ea, eca), (lb, cb, gb, eb, ecb) = results
    assert torch.equal(la, lb) and torch.equal(ea, eb)
    assert len(ca) == len(cb) == cfg["depth"] and all(torch.equal(p, q) for p, q in zip(ca, cb)) and all(torch.equal(p, q) for p, q in zip(eca, ecb))
    assert set(ga) == set(gb)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            assert torch.equal(ga[k], gb[k]), k
    assert sum(v is not None and float(v.abs().max()) > 0 for v in ga.values()) >= 12 * cfg["depth"]


@pytest.mark.parametrize("extra", [dict(fuse_dropped=True), dict(squeeze_dropped=True), dict(graph_rank_iters=3),
                                   dict(fuse_dropped=True, graph_rank_iters=3)], ids=lambda e: "+".join(sorted(e)))
def test_the_lists_keep_their_contract_with_fusion_squeezing_and_graph_ranking(extra):
    from d2s import ops
    cfg = GR_CASES["micro2"]["cfg"]
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    x = _images("micro2")
    student = _student("micro2", sim_prune=SIM_R, **extra).train()
    logits, _, pred, kept = student(x)
    logits.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and student.sim_prune_counts == [SIM_R, SIM_R]
    want = float64_forward("micro2", SIM_R, extra.get("graph_rank_iters", 0), False)
    assert torch.equal(kept[0].cpu(), want["kept"][0])                                     # stage 0 sees none of the extras
    for s, (k, d, p) in enumerate(zip(kept, student.dropped_token_indices, pred)):
        T = p.shape[1]
        assert T == (16 if s == 0 else ks[0])                                              # a carried package row is not scored
        assert k.dtype == d.dtype == torch.int64 and k.shape == (3, ks[s]) and d.shape == (3, T - ks[s])
        both = torch.sort(torch.cat([k, d], dim=1), dim=1)[0].cpu()
        assert torch.equal(both, torch.arange(T).expand(3, T))                             # a partition of [0, T)
        assert bool((k[:, 1:] > k[:, :-1]).all()) and bool((d[:, 1:] > d[:, :-1]).all())   # both ascending
        pruned, partner, sim = student.sim_plans[s]
        gone = torch.zeros((3, T), dtype=torch.bool, device=DEV).scatter_(1, d, True)
        assert bool(torch.gather(gone, 1, pruned).all()) and not bool(torch.gather(gone, 1, partner).any())      # partners are never pruned
        assert bool((sim.abs() <= 1.0 + 1e-6).all())
    if extra.get("squeeze_dropped"):
        assert len(student.squeeze_plans) == 2
    assert all(p.grad is None for p in student.score_predictor.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for k, p in student.named_parameters() if k.startswith("blocks."))


def test_zero_is_the_default_model_bit_for_bit(monkeypatch):
    from d2s import functional_sim_prune as SF
    monkeypatch.setattr(SF, "metric_block", None)                                          # never reached
    x = _images("micro2")
    for extra in (dict(), dict(graph_rank_iters=3)):
        base, off = _student("micro2", **extra), _student("micro2", sim_prune=0, **extra)
        for train in (False, True):
            outs = []
            for m in (base, off):
                m.train(train)
                with torch.no_grad():
                    outs.append(m(x))
                assert m.sim_plans == [] and m.sim_prune_counts == []
            a, b = outs
            assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
            assert all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


# ---- 4. TrainStep ----
def _step_pair(name="micro1", graph=False, sim_prune=SIM_R, **kw):
    """micro1's weights in a student whose init_n is its own token count (16), keep 0.5: the stage keeps 8 ids and MaskLoss ranks 8"""
    from d2s.engine import TrainStep
    student = _student(name, sim_prune=sim_prune, **kw)
    args = make_args(GR_CASES[name]["cfg"])
    args.keep_ratios = list(kw.get("token_ratio", GR_CASES[name]["cfg"]["token_ratio"]))
    return TrainStep(student, _teacher(name), args, warmup_steps=0, graph=graph), student


def _xy(name="micro1"):
    return built(name)[2].to(DEV), built(name)[3].to(DEV)


def _train(steps):
    ts, student = _step_pair(init_n=16, token_ratio=[0.5])
    before = {n: p.detach().clone() for n, p in student.named_parameters()}
    x, y = _xy()
    torch.manual_seed(5)
    infos = []
    for _ in range(steps):
        info = ts(x, y)
        torch.cuda.synchronize()
        infos.append(dict(loss=info["loss"].detach().clone(), mask_loss=info["mask_loss"].detach().clone(), kept=[k.clone() for k in info["kept"]]))
    return ts, student, before, infos


def test_three_train_steps_two_runs_and_a_resume():
    from d2s import lib
    ts, student, before, infos = _train(3)
    after = dict(student.named_parameters())
    pred = [n for n in before if n.startswith("score_predictor.")]
    for n in pred:                                                                 # the predictors: bit-unchanged, no gradient
        assert torch.equal(after[n].detach(), before[n]) and after[n].grad is None, n
    moved = [n for n in before if n.startswith("blocks.") and not torch.equal(after[n].detach(), before[n])]
    assert len(moved) == sum(n.startswith("blocks.") for n in before) and not torch.equal(after["head.weight"].detach(), before["head.weight"])
    assert all(math.isfinite(float(i["loss"])) and float(i["mask_loss"]) == 0.0 for i in infos)
    assert infos[0]["kept"][0].shape == (3, 8) and student.sim_prune_counts == [SIM_R] and student.sim_plans[0][0].shape == (3, SIM_R)
    cfg = ts.config()
    assert cfg["attn_selection"] is True and cfg["sim_prune"] == SIM_R and "graph_rank_iters" not in cfg and ts.graph is False
    ts2, _, _, infos2 = _train(3)                                                  # a second identical run: the same bits
    assert torch.equal(ts.arena.params, ts2.arena.params)
    assert all(torch.equal(a["loss"], b["loss"]) and torch.equal(a["kept"][0], b["kept"][0]) for a, b in zip(infos, infos2))
    # 2 steps, a checkpoint, 1 more step = 3 straight steps
    two, _, _, _ = _train(2)
    saved = two.state_dict()
    assert saved["config"]["sim_prune"] == SIM_R
    resumed, _ = _step_pair(init_n=16, token_ratio=[0.5])
    assert resumed.load_state_dict(saved) == saved["epoch"]
    x, y = _xy()
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, ts.arena.params)
    for other_r in (0, 1):                                                          # another rule: a resume is refused
        other, _ = _step_pair(init_n=16, token_ratio=[0.5], sim_prune=other_r)
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: sim_prune"):
            other.load_state_dict(saved)


def test_graph_step_is_bit_identical_to_the_eager_step():
    """nothing in a similarity stage synchronises with the host: the captured step replays the same bits (micro2, two stages)"""
    from tests.test_graph_gpu import _batches, _same_step
    case = GR_CASES["micro2"]
    (eager, _), (graph, _) = [_step_pair("micro2", graph=gr) for gr in (False, True)]
    for i, (x, y) in enumerate(_batches(case, eager.GRAPH_WARM_STEPS + 2, DEV)):
        _same_step(eager, graph, x, y, f"step {i}")
    assert graph.last_step_captured and not eager.last_step_captured
    for k, v in eager.metrics.items():
        assert float(v) == float(graph.metrics[k]), k


def test_the_bf16_mode_is_refused():
    from d2s import functional_sim_prune as SF
    from d2s import lib, ops
    from d2s.engine import TrainStep
    student = _student("micro1", sim_prune=SIM_R)
    args = make_args(GR_CASES["micro1"]["cfg"])
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            TrainStep(student, _teacher("micro1"), args, warmup_steps=0)
        assert str(e.value) == SF.SIM_PRUNE_BF16_ERROR
        for train in (False, True):
            with pytest.raises(lib.D2SError) as e, torch.set_grad_enabled(train):
                student.train(train)(_images("micro1"))
            assert str(e.value) == SF.SIM_PRUNE_BF16_ERROR
    with torch.no_grad():                                                           # the same model in an fp32 mode runs
        assert bool(torch.isfinite(student.eval()(_images("micro1"))[0]).all())


# ---- 5. command line ----
def test_cli_trains_one_tiny_epoch_and_evaluates(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    common = ["--arch", "deit_tiny", "--topk-selection", "--attn-selection", "--sim-prune", "4", "--pruning-locs", "3", "6", "--keep-ratios", "0.7",
              "0.5", "--batch-size", "4", "--val-steps", "1", "--teacher-checkpoint", path]
    acc = mask_predictor.main(common + ["--epochs", "1", "--steps-per-epoch", "2", "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Attention: --sim-prune 4 lets" in out and "Start training" in out and "val loss:" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert cfg["sim_prune"] == 4 and cfg["attn_selection"] is True and cfg["pruning_loc"] == [3, 6] and "graph_rank_iters" not in cfg
    acc2 = mask_predictor.main(common + ["--eval-only", "--resume", os.path.join(out_dir, "last.pt")])
    out = capsys.readouterr().out
    assert isinstance(acc2, float) and 0.0 <= acc2 <= 1.0 and "eval only:" in out
