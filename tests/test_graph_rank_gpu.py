"""Graph ranking on the GPU (--graph-rank T) against the float64 restatement of tests/graph_rank_ref.py.
The kernel (csrc/graph_rank.hip on the f32-input matrix pipe), fed with the lse the attention forward of the same qkv wrote: every entry
within relative iters * 1e-5 of float64 - the project's rule for one pass of these probabilities is 1e-5 (tests/test_ltp_gpu.py), and
every pass is a sum of non-negative terms, so the relative errors add - every (image, head) within iters * 1e-5 of mass 1, the head mean
at iters = 1 against ops.ltp_score, iters = 5 against 2 then 3 bit for bit, two calls bit for bit, NaN-filled outputs with guard bands, a
start vector with exact zeros, every refusal with poisoned outputs untouched.
The model in the micro1 / micro2 geometries (tests/test_graph_rank_cpu.py asserts the conditions on their inputs): the stage's outputs
against ops.select_cls_attn of the model's own rank bit for bit, the rank against float64 from the block's own input, the kept ids
against float64 on every image, the ranked route against the plain attention-selecting model bit for bit under one replayed selection
(logits, CLS rows, every parameter gradient; with stochastic depth too), token fusion, squeezing, the flag at 0.
TrainStep (three steps, two runs, save and resume, the captured step, the bf16 refusal) and the command line."""
import math
import os

import numpy as np
import pytest
import torch

from tests import attnsel_ref
from tests import cases
from tests import fuse_ref
from tests import graph_rank_ref as R
from tests.test_graph_rank_cpu import GR_CASES, SCALE, built, float64_forward, make_qkv
from tests.test_model_gpu import make_args

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = 2.0 ** -24
GUARD, POISON = 64, 1234.5
ITERS = (1, 2, 5)
SHAPES = [(B, H, n) for (B, H) in ((1, 1), (3, 6)) for n in (1, 2, 31, 32, 33, 65, 128, 129, 197, 200)] + [(1, 12, 577)]
WORST = {}
_REF = {}


def _note(tag, v):
    WORST[tag] = max(WORST.get(tag, 0.0), float(v))
    print(f"  {tag}: {float(v):.3e} (worst over the tests so far {WORST[tag]:.3e})")


def _rel(tag, got, ref, rtol):
    """|got - ref| <= rtol |ref| elementwise against float64; the worst relative error is printed before the assertion"""
    got, ref = got.double().cpu(), ref.double()
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    _note(tag, err)
    assert bool(torch.isfinite(got).all()) and float(err) <= rtol, (tag, float(err), rtol)


def _case(B, H, n):
    """(qkv float64 on the fp32 grid, P float64, the float64 ranks s^1 .. s^5), computed once per shape"""
    key = (B, H, n)
    if key not in _REF:
        qkv = make_qkv(B * n, H, 1000 * n + 10 * H + B)
        P = R.probabilities(qkv, B, n, H, SCALE)
        _REF[key] = (qkv, P, R.iterate(P, max(ITERS), trace=True))
    return _REF[key]


def _dev_qkv(qkv64):
    return qkv64.float().reshape(qkv64.shape[0], -1).contiguous().to(DEV)


def _attn_fwd(qkv, B, n, H):
    """the dense fp32 attention forward -> lse [B, H, n]"""
    from d2s import lib
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=DEV)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=DEV)
    lib.call("d2s_attn_fwd_f32", lib.ptr(qkv), lib.ptr(out), lib.ptr(lse), None, B, n, H, SCALE)
    return lse


# ---- 1. the kernel ----
@pytest.mark.parametrize("B,H,n", SHAPES)
def test_rank_against_float64(B, H, n):
    from d2s import ops
    qkv64, _, steps = _case(B, H, n)
    qkv = _dev_qkv(qkv64)
    lse = _attn_fwd(qkv, B, n, H)
    got = {}
    for iters in ITERS:
        r = got[iters] = ops.graph_rank(qkv, lse, B, n, H, SCALE, iters)
        assert r.shape == (B, H, n) and r.dtype == torch.float32
        _rel(f"rank iters={iters}", r, steps[iters - 1], iters * 1e-5)
        mass = (r.double().sum(dim=-1) - 1.0).abs().max()
        _note(f"|sum - 1| iters={iters}", mass)
        assert float(mass) <= iters * 1e-5
        assert torch.equal(ops.graph_rank(qkv, lse, B, n, H, SCALE, iters), r)                   # two calls: the same bits
    # iters = 1 is the received attention per head: its head mean is the LTP score (another kernel, heads folded there)
    score = ops.ltp_score(qkv, lse, B, n, H, SCALE).reshape(B, n).double()
    mean1 = got[1].double().mean(dim=1)
    err = ((mean1 - score).abs() / score).max()
    _note("head mean of iters=1 against ltp_score", err)
    assert float(err) <= 2e-5
    # 5 = 2 then 3 from the caller's vector, bit for bit: the ping-pong ends in `rank` for either parity
    assert torch.equal(ops.graph_rank(qkv, lse, B, n, H, SCALE, 3, w0=got[2]), got[5])
    assert torch.equal(ops.graph_rank(qkv, lse, B, n, H, SCALE, 1, w0=ops.graph_rank(qkv, lse, B, n, H, SCALE, 1)), got[2])


def _raw(qkv, lse, w0, B, n, H, iters, with_ws=True, fill=float("nan")):
    """the C entry on NaN-filled (or poisoned) outputs with guard bands -> (rc, rank, ws)"""
    from d2s import lib
    size = B * H * n
    rank = torch.full((size + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    ws = torch.full((size + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    for t in (rank, ws):
        t[:GUARD] = POISON
        t[GUARD + size:] = POISON
    rc = lib._fn("d2s_graph_rank_f32")(lib.ptr(qkv), lib.ptr(lse), lib.ptr(w0), lib.ptr(rank[GUARD:]), lib.ptr(ws[GUARD:]) if with_ws else None,
                                       B, n, H, SCALE, iters, lib.stream())
    torch.cuda.synchronize()
    return rc, rank, ws


def _guards_intact(t, size):
    return bool((t[:GUARD] == POISON).all()) and bool((t[GUARD + size:] == POISON).all())


@pytest.mark.parametrize("B,H,n", [(3, 6, 33), (1, 1, 1), (3, 6, 129)])
def test_only_the_outputs_are_written(B, H, n):
    from d2s import ops
    qkv = _dev_qkv(_case(B, H, n)[0])
    lse = _attn_fwd(qkv, B, n, H)
    size = B * H * n
    for iters in (1, 2, 3):
        rc, rank, ws = _raw(qkv, lse, None, B, n, H, iters)
        assert rc == 0 and _guards_intact(rank, size) and _guards_intact(ws, size)
        body = rank[GUARD:GUARD + size]
        assert bool(torch.isfinite(body).all()) and torch.equal(body.view(B, H, n), ops.graph_rank(qkv, lse, B, n, H, SCALE, iters))
        inner = ws[GUARD:GUARD + size]
        if iters == 1:
            assert bool(torch.isnan(inner).all())                                         # one launch: the workspace is not touched
        else:
            assert torch.equal(inner.view(B, H, n), ops.graph_rank(qkv, lse, B, n, H, SCALE, iters - 1))      # it holds s^(iters - 1)
    rc, rank, _ = _raw(qkv, lse, None, B, n, H, 1, with_ws=False)                          # iters == 1 needs no workspace
    assert rc == 0 and _guards_intact(rank, size) and bool(torch.isfinite(rank[GUARD:GUARD + size]).all())


@pytest.mark.parametrize("B,H,n", [(3, 6, 65), (1, 1, 2), (3, 6, 200)])
def test_a_start_vector_with_exact_zeros(B, H, n):
    from d2s import ops
    qkv64, P, _ = _case(B, H, n)
    qkv = _dev_qkv(qkv64)
    lse = _attn_fwd(qkv, B, n, H)
    g = torch.Generator().manual_seed(n)
    w0 = torch.rand((B, H, n), generator=g).float()
    w0[torch.rand((B, H, n), generator=g) < 0.4] = 0.0
    w0[:, :, 0] = 0.5                                                                     # no all-zero vector
    if n > 1:
        w0[:, :, 1] = 0.0
    for iters in ITERS:
        r = ops.graph_rank(qkv, lse, B, n, H, SCALE, iters, w0=w0.to(DEV))
        ref = R.iterate(P, iters, w0=w0)
        _rel(f"rank from w0 iters={iters}", r, ref, iters * 1e-5)
        mass = ((r.double().cpu().sum(dim=-1) - w0.double().sum(dim=-1)).abs() / w0.double().sum(dim=-1)).max()
        assert float(mass) <= iters * 1e-5                                                # the start vector's mass is kept
    onehot = torch.zeros((B, H, n))
    onehot[:, :, n - 1] = 1.0                                                             # all the mass on the last token: row n - 1 of P
    _rel("rank from a one-hot start", ops.graph_rank(qkv, lse, B, n, H, SCALE, 1, w0=onehot.to(DEV)), P[:, :, n - 1], 1e-5)


def test_refusals_leave_the_outputs_alone():
    from d2s import lib
    B, H, n = 2, 2, 17
    qkv = _dev_qkv(make_qkv(B * n, H, 8))
    lse = torch.zeros((B, H, n), dtype=torch.float32, device=DEV)
    w0 = torch.ones((B, H, n), dtype=torch.float32, device=DEV)
    rank = torch.full((B * H * n,), POISON, dtype=torch.float32, device=DEV)
    ws = torch.full((B * H * n,), POISON, dtype=torch.float32, device=DEV)
    good = dict(qkv=qkv, lse=lse, w0=None, rank=rank, ws=ws, B=B, n=n, H=H, iters=3)
    bad = [dict(qkv=None), dict(lse=None), dict(rank=None), dict(ws=None), dict(ws=None, iters=2), dict(B=0), dict(B=-1), dict(H=0), dict(n=0),
           dict(n=8193), dict(iters=0), dict(iters=-1), dict(iters=1025), dict(w0=rank), dict(w0=ws)]
    fn = lib._fn("d2s_graph_rank_f32")
    for change in bad:
        a = dict(good, **change)
        rc = fn(lib.ptr(a["qkv"]), lib.ptr(a["lse"]), lib.ptr(a["w0"]), lib.ptr(a["rank"]), lib.ptr(a["ws"]), a["B"], a["n"], a["H"], SCALE,
                a["iters"], lib.stream())
        assert rc == -1, (sorted(change), rc)
    torch.cuda.synchronize()
    assert bool((rank == POISON).all()) and bool((ws == POISON).all())
    for change in (dict(), dict(w0=w0), dict(ws=None, iters=1), dict(iters=1024, B=1, n=2, H=1)):      # the same calls, legal
        a = dict(good, **change)
        assert fn(lib.ptr(a["qkv"]), lib.ptr(a["lse"]), lib.ptr(a["w0"]), lib.ptr(a["rank"]), lib.ptr(a["ws"]), a["B"], a["n"], a["H"], SCALE,
                  a["iters"], lib.stream()) == 0
    torch.cuda.synchronize()


# ---- 2. the model, micro geometries ----
TOL = 1e-4          # the model tests of tests/test_ltp_gpu.py hold a score computed from the model's own activations to this, in both modes
MODES = ("exact", "split")
T_MODEL = 3


def _gm(mode):
    from d2s import ops
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[mode]


def _common(cfg):
    return dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])


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


def _teacher(name):
    import vit_models
    t = vit_models.VisionTransformerTeacher(**_common(GR_CASES[name]["cfg"]))
    t.load_state_dict(built(name)[1], strict=True)
    return t.to(DEV)


def _images(name):
    return built(name)[2].to(DEV)


def _spy_rank_block(monkeypatch):
    """records the input of every block that ranks -> the list of x [B, n, D] (detached), in stage order"""
    from d2s import functional_graph_rank as GF
    seen, orig = [], GF.rank_block

    def spy(x, *a, **kw):
        seen.append(x.detach().clone())
        return orig(x, *a, **kw)
    monkeypatch.setattr(GF, "rank_block", spy)
    return seen


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_student_selects_by_the_rank(name, mode, monkeypatch):
    from d2s import ops
    cfg = GR_CASES[name]["cfg"]
    locs = list(cfg["pruning_loc"])
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    sd64 = {k: v.double() for k, v in built(name)[0].items()}
    x = _images(name)
    seen = _spy_rank_block(monkeypatch)
    for train in (False, True):
        for mean in (False, True):
            student = _student(name, graph_rank_iters=T_MODEL, mean_heads=mean).train(train)
            del seen[:]
            with ops.gemm_mode(_gm(mode)), torch.set_grad_enabled(train):
                out = student(x)
            torch.cuda.synchronize()
            pred, kept = out[2], out[3]
            ranks = student.graph_ranks
            assert bool(torch.isfinite(out[0]).all()) and len(ranks) == len(pred) == len(kept) == len(seen) == len(locs)
            want = float64_forward(name, T_MODEL, mean)
            for s, loc in enumerate(locs):
                B, n, _ = seen[s].shape
                assert ranks[s].shape == (B, cfg["heads"], n) and not ranks[s].requires_grad and not pred[s].requires_grad
                p2, k2, d2 = ops.select_cls_attn(ranks[s], 1, n - 1, ks[s], mean)               # the stage is this call, unchanged
                assert torch.equal(pred[s], p2) and torch.equal(kept[s], k2) and torch.equal(student.dropped_token_indices[s], d2)
                # float64 from the block's own input: LayerNorm 1, the qkv projection, the iteration
                ref = R.block_rank(sd64, loc - 1, seen[s].cpu(), cfg, T_MODEL)
                _rel(f"{name} {mode} stage {s} rank", ranks[s], ref, TOL)
                assert float((ranks[s].double().sum(dim=-1) - 1.0).abs().max()) <= TOL
                _, kept64, dropped64 = attnsel_ref.select(ref, 1, n - 1, ks[s], mean)
                assert torch.equal(kept[s].cpu(), kept64) and torch.equal(student.dropped_token_indices[s].cpu(), dropped64)      # every image
                assert torch.equal(kept[s].cpu(), want["kept"][s])                              # ... and float64 all the way
            # replaying the recorded selection gives the same logits
            student.kept_token_override = [k.clone() for k in kept]
            with ops.gemm_mode(_gm(mode)), torch.set_grad_enabled(train):
                again = student(x)
            assert torch.equal(again[0], out[0])


def _run(student, x, w, masks=None):
    """one training forward and backward under the loss <w, logits> -> (logits, cls_attns, {name: grad})"""
    from d2s import ops
    student.train()
    student.drop_path_masks = masks
    logits = student(x)[0]
    cls = [c.clone() for c in student.cls_attns]
    (logits * w).sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    return logits.detach(), cls, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in student.named_parameters()}


@pytest.mark.parametrize("drop_path", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(GR_CASES))
def test_the_ranked_route_does_not_move_the_block(name, drop_path):
    """the same replayed selection in a ranking model and in a plain attention-selecting one: the block before a stage runs through the
    per-op sequence in one and through the one-call composite in the other, and nothing downstream may tell"""
    cfg = GR_CASES[name]["cfg"]
    x = _images(name)
    override = [k.clone() for k in float64_forward(name, T_MODEL, False)["kept"]]
    g = torch.Generator().manual_seed(3)
    w = torch.randn((x.shape[0], cfg["num_classes"]), generator=g).to(DEV)
    masks = None
    if drop_path > 0:
        # a fixed table; the rates are linspace(0, 0.5, 4), so block 0 has none and micro2's ranked block 1 (rate 1/6) is the case that
        # matters: one image loses its attention branch there, another its MLP branch, the third keeps both
        masks = (torch.rand((2 * cfg["depth"], x.shape[0]), generator=g) < 0.5).float()
        masks[2:4] = torch.tensor([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0]])
        assert 0 < int(masks.sum()) < masks.numel()
    results = []
    for iters in (T_MODEL, 0):
        student = _student(name, graph_rank_iters=iters, drop_path_rate=drop_path)
        student.kept_token_override = override
        results.append(_run(student, x, w, masks))
        assert len(student.graph_ranks) == (len(cfg["pruning_loc"]) if iters else 0)
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


def test_with_token_fusion_the_package_row_is_weighted_by_the_ranked_probs(monkeypatch):
    """micro2: the second stage carries a package row (t = 1), which is a node of the graph and is not scored.  The bound is
    tests/test_fuse_gpu.py's for f: 4 (m + 2) u sum_j |w_j x_jc| with m dropped tokens."""
    import d2s.functional as DF
    from d2s import ops
    x = _images("micro2")
    student = _student("micro2", graph_rank_iters=T_MODEL, fuse_dropped=True).train()
    calls = []
    orig = DF.GatherFuseFn.apply

    def spy(xs, p, kept, dropped, t):
        y = orig(xs, p, kept, dropped, t)
        calls.append((xs, p, kept, dropped, t, y))
        return y
    monkeypatch.setattr(DF.GatherFuseFn, "apply", staticmethod(spy))
    logits, _, pred, kept_all = student(x)
    logits.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert [c[4] for c in calls] == [0, 1]
    for s, (xs, p, kept, dropped, t, y) in enumerate(calls):
        n = xs.shape[1]
        assert student.graph_ranks[s].shape[-1] == n                               # carried rows are nodes of the graph ...
        p2, k2, _ = ops.select_cls_attn(student.graph_ranks[s], 1, n - 1 - t, kept.shape[1], False)
        assert p is pred[s] and torch.equal(p, p2) and torch.equal(kept, k2) and p.shape[1] == n - 1 - t      # ... and are not scored
        xc, pc, kc, dc = xs.detach().cpu(), p.cpu(), kept.cpu(), dropped.cpu()
        want = fuse_ref.fuse_forward_f64(xc, pc, kc, dc, t)
        Bc, m, D = xc.shape[0], dc.shape[1], xc.shape[2]
        pd = torch.gather(pc.double(), 1, dc)
        wts = pd / pd.sum(dim=1, keepdim=True)
        xd = torch.gather(xc.double()[:, 1:n - t], 1, dc[:, :, None].expand(Bc, m, D))
        bound = 4.0 * (m + 2) * EPS * (wts[:, :, None] * xd).abs().sum(dim=1)
        err = (y[:, -1].detach().cpu().double() - want[:, -1]).abs()
        print(f"[graph rank fuse stage {s}] largest fraction of the bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        assert torch.equal(y[:, :-1].detach().cpu(), want[:, :-1].float())         # CLS, kept and carried rows are copies
    assert all(p.grad is None for p in student.score_predictor.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for k, p in student.named_parameters() if k.startswith("blocks."))


def test_with_squeezing_the_forward_and_one_backward_run():
    from d2s import ops
    x = _images("micro2")
    student = _student("micro2", graph_rank_iters=T_MODEL, squeeze_dropped=True).train()
    logits, _, pred, kept = student(x)
    logits.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and len(student.squeeze_plans) == 2 and len(student.graph_ranks) == 2
    assert all(torch.equal(k, float64_forward("micro2", T_MODEL, False)["kept"][s].to(DEV)) for s, k in enumerate(kept[:1]))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for k, p in student.named_parameters() if k.startswith("blocks."))


def test_zero_iterations_is_the_default_model_bit_for_bit():
    x = _images("micro2")
    base, off = _student("micro2"), _student("micro2", graph_rank_iters=0)
    for train in (False, True):
        outs = []
        for m in (base, off):
            m.train(train)
            with torch.no_grad():
                outs.append(m(x))
            assert m.graph_ranks == []
        a, b = outs
        assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


# ---- 3. TrainStep ----
def _step_pair(name="micro1", graph=False, **kw):
    """micro1's weights in a student whose init_n is its own token count (16), keep 0.5: the stage keeps 8 ids and MaskLoss ranks 8"""
    from d2s.engine import TrainStep
    student = _student(name, graph_rank_iters=T_MODEL, **kw)
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
    assert len(pred) == 24
    for n in pred:                                                                 # the predictors: bit-unchanged, no gradient
        assert torch.equal(after[n].detach(), before[n]) and after[n].grad is None and not bool(ts.arena.grad_views[n].any()), n
    moved = [n for n in before if n.startswith("blocks.") and not torch.equal(after[n].detach(), before[n])]
    assert len(moved) == sum(n.startswith("blocks.") for n in before) and not torch.equal(after["head.weight"].detach(), before["head.weight"])
    assert all(math.isfinite(float(i["loss"])) and float(i["mask_loss"]) == 0.0 for i in infos)
    assert float(ts.metrics["train_mask_loss"]) == 0.0 and infos[0]["kept"][0].shape == (3, 8)
    cfg = ts.config()
    assert cfg["attn_selection"] is True and cfg["graph_rank_iters"] == T_MODEL and ts.graph is False
    ts2, _, _, infos2 = _train(3)                                                  # a second identical run: the same bits
    assert torch.equal(ts.arena.params, ts2.arena.params)
    assert all(torch.equal(a["loss"], b["loss"]) and torch.equal(a["kept"][0], b["kept"][0]) for a, b in zip(infos, infos2))
    # 2 steps, a checkpoint, 1 more step = 3 straight steps
    two, _, _, _ = _train(2)
    saved = two.state_dict()
    assert saved["config"]["graph_rank_iters"] == T_MODEL
    resumed, _ = _step_pair(init_n=16, token_ratio=[0.5])
    assert resumed.load_state_dict(saved) == saved["epoch"]
    x, y = _xy()
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, ts.arena.params)
    from d2s.engine import TrainStep
    args = make_args(GR_CASES["micro1"]["cfg"])
    args.keep_ratios = [0.5]
    for iters in (0, 1):                                                            # another rule: a resume is refused
        other = TrainStep(_student("micro1", graph_rank_iters=iters, init_n=16, token_ratio=[0.5]), _teacher("micro1"), args, warmup_steps=0, graph=False)
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: graph_rank_iters"):
            other.load_state_dict(saved)


def test_graph_step_is_bit_identical_to_the_eager_step():
    """nothing in a ranked stage synchronises with the host: the captured step replays the same bits (micro2, two stages)"""
    from tests.test_graph_gpu import _batches, _same_step
    case = GR_CASES["micro2"]
    (eager, _), (graph, _) = [_step_pair("micro2", graph=gr) for gr in (False, True)]
    for i, (x, y) in enumerate(_batches(case, eager.GRAPH_WARM_STEPS + 2, DEV)):
        _same_step(eager, graph, x, y, f"step {i}")
    assert graph.last_step_captured and not eager.last_step_captured
    for k, v in eager.metrics.items():
        assert float(v) == float(graph.metrics[k]), k


def test_the_bf16_mode_is_refused():
    from d2s import functional_graph_rank as GF
    from d2s import lib, ops
    from d2s.engine import TrainStep
    student = _student("micro1", graph_rank_iters=T_MODEL)
    args = make_args(GR_CASES["micro1"]["cfg"])
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            TrainStep(student, _teacher("micro1"), args, warmup_steps=0)
        assert str(e.value) == GF.GRAPH_RANK_BF16_ERROR
        for train in (False, True):
            with pytest.raises(lib.D2SError) as e, torch.set_grad_enabled(train):
                student.train(train)(_images("micro1"))
            assert str(e.value) == GF.GRAPH_RANK_BF16_ERROR
    with torch.no_grad():                                                           # the same model in an fp32 mode runs
        assert bool(torch.isfinite(student.eval()(_images("micro1"))[0]).all())


# ---- 4. command line ----
def test_cli_trains_one_tiny_epoch_and_evaluates(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    common = ["--arch", "deit_tiny", "--topk-selection", "--attn-selection", "--graph-rank", "3", "--pruning-locs", "3", "6", "--keep-ratios", "0.7",
              "0.5", "--batch-size", "4", "--val-steps", "1", "--teacher-checkpoint", path]
    acc = mask_predictor.main(common + ["--epochs", "1", "--steps-per-epoch", "2", "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Attention: --graph-rank 3 ranks" in out and "Start training" in out and "val loss:" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert cfg["graph_rank_iters"] == 3 and cfg["attn_selection"] is True and cfg["pruning_loc"] == [3, 6]
    acc2 = mask_predictor.main(common + ["--eval-only", "--resume", os.path.join(out_dir, "last.pt")])
    out = capsys.readouterr().out
    assert isinstance(acc2, float) and 0.0 <= acc2 <= 1.0 and "eval only:" in out
