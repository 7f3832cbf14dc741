"""The Evo-ViT baseline (--method evo) on the GPU: the four kernels of csrc/evo.hip alone against the restatement of
tests/evo_ref.py, their refusals, the model in all three arithmetic modes against float64 (selections, logits, loss, every parameter
gradient), TrainStep (determinism, resume, accumulation, the captured step, refusals, the gradient hook) and one tiny epoch of the CLI."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import evo_ref as R
from tests.test_evo_cpu import EVO_CASES, built, check_condition

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = R.U
POISON = -77.25


def _ks(T):
    return sorted({1, T - 1, max(1, T // 2)})


def _lists(B, T, k, gen):
    return R.topk_rule(torch.rand(B, T, generator=gen, dtype=torch.float64), k)


def _frac(tag, err, bound):
    """print the worst error as a fraction of its bound, then assert"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"  {tag}: worst error / bound = {frac:.3f}")
    assert bool((err <= bound).all()), (tag, frac)


# ---- 1. the kernels alone ----
SHAPES = [(B, T, D) for T in (2, 9, 65, 196) for B in (1, 3) for D in (64, 384, 1024)]


@pytest.mark.parametrize("T", [2, 9, 65, 196])
def test_scatter_fwd_bit_for_bit(T):
    from d2s import ops
    for B, _, D in [s for s in SHAPES if s[1] == T]:
        for k in _ks(T):
            gen = torch.Generator().manual_seed(1000 * T + 10 * k + B)
            kept, dropped = _lists(B, T, k, gen)
            X = torch.randn(B, 1 + T, D, generator=gen)
            yc, xc = torch.randn(B, k + 2, D, generator=gen), torch.randn(B, k + 2, D, generator=gen)
            want = R.scatter_fwd(X, yc, xc, kept, dropped)                    # fp32 on the CPU: one subtraction, one addition
            Xd = X.to(DEV)
            got = ops.evo_scatter_fwd(Xd, yc.to(DEV), xc.to(DEV), kept.to(DEV), dropped.to(DEV))
            assert got is Xd and torch.equal(got.cpu(), want), (B, T, k, D)


@pytest.mark.parametrize("T", [2, 9, 65, 196])
def test_scatter_bwd_against_float64(T):
    from d2s import ops
    for B, _, D in [s for s in SHAPES if s[1] == T]:
        for k in _ks(T):
            gen = torch.Generator().manual_seed(2000 * T + 10 * k + B)
            kept, dropped = _lists(B, T, k, gen)
            m = T - k
            dX = torch.randn(B, 1 + T, D, generator=gen)
            want = R.scatter_bwd(dX, kept, dropped)
            got = ops.evo_scatter_bwd(dX.to(DEV), kept.to(DEV), dropped.to(DEV)).cpu()
            assert torch.equal(got[:, :k + 1].double(), want[:, :k + 1]), (B, T, k, D)          # copied rows
            mag = torch.stack([dX[b, 1 + dropped[b]].double().abs().sum(dim=0) for b in range(B)])
            err = (got[:, k + 1].double() - want[:, k + 1]).abs()
            assert bool((err <= (m - 1) * U * mag).all()), (B, T, k, D, float((err / ((m - 1) * U * mag + 1e-300)).max()))
            dXi = torch.randint(-8, 9, (B, 1 + T, D), generator=gen).float()                    # integers: every order gives the same sum
            goti = ops.evo_scatter_bwd(dXi.to(DEV), kept.to(DEV), dropped.to(DEV)).cpu()
            assert torch.equal(goti.double(), R.scatter_bwd(dXi, kept, dropped)), (B, T, k, D)


@pytest.mark.parametrize("T", [2, 9, 65, 196])
def test_gather_bwd_against_float64(T):
    from d2s import ops
    worst = 0.0
    for B, _, D in [s for s in SHAPES if s[1] == T]:
        for k in _ks(T):
            gen = torch.Generator().manual_seed(3000 * T + 10 * k + B)
            kept, dropped = _lists(B, T, k, gen)
            dX, dxc, dyc = torch.randn(B, 1 + T, D, generator=gen), torch.randn(B, k + 2, D, generator=gen), torch.randn(B, k + 2, D, generator=gen)
            g = torch.rand(B, T, generator=gen) + 0.01
            S = torch.gather(g, 1, dropped).sum(dim=1)                            # an fp32 S, as the forward hands one over
            want = R.gather_bwd(dX, dxc, dyc[:, k + 1], g, S, kept, dropped)
            bound = R.gather_bwd_bound(dX, dxc, dyc[:, k + 1], g, S, dropped)
            dXd = dX.to(DEV)
            got = ops.evo_gather_bwd(dXd, dxc.to(DEV), dyc.to(DEV), g.to(DEV), S.to(DEV), kept.to(DEV), dropped.to(DEV))
            assert got is dXd
            got = got.cpu().double()
            for b in range(B):
                assert torch.equal(got[b, 0], want[b, 0]) and torch.equal(got[b, 1 + kept[b]], want[b, 1 + kept[b]]), (B, T, k, D)
                err = (got[b, 1 + dropped[b]] - want[b, 1 + dropped[b]]).abs()
                worst = max(worst, float((err / bound[b]).max()))
                assert bool((err <= bound[b]).all()), (B, T, k, D, worst)
    print(f"  T {T}: worst error / bound of a dropped row {worst:.3f}")


def test_gather_bwd_with_a_zero_sum_passes_the_dropped_rows_through():
    from d2s import ops
    gen = torch.Generator().manual_seed(5)
    B, T, k, D = 2, 9, 4, 64
    kept, dropped = _lists(B, T, k, gen)
    dX, dxc, dyc = torch.randn(B, 1 + T, D, generator=gen), torch.randn(B, k + 2, D, generator=gen), torch.randn(B, k + 2, D, generator=gen)
    g = torch.rand(B, T, generator=gen)
    got = ops.evo_gather_bwd(dX.to(DEV), dxc.to(DEV), dyc.to(DEV), g.to(DEV), torch.zeros(B, device=DEV), kept.to(DEV), dropped.to(DEV)).cpu()
    for b in range(B):
        assert torch.equal(got[b, 1 + dropped[b]], dX[b, 1 + dropped[b]]) and torch.equal(got[b, 1 + kept[b]], dxc[b, 1:k + 1])


def _check_select(g_in, kept_prev, cls_row, tau, k, tag):
    from d2s import ops
    dev = lambda t: None if t is None else t.to(DEV)
    g_out, kept, dropped = ops.evo_select(dev(cls_row), k, tau, dev(g_in), dev(kept_prev))
    want_g, _, _ = R.select(None if g_in is None else g_in.double(), kept_prev, cls_row.double(), tau, k)
    ek, ed = ops.select_topk(g_out, k)
    assert torch.equal(kept, ek) and torch.equal(dropped, ed), tag                       # d2s_select_topk's ids, bit for bit
    rk, rd = R.topk_rule(g_out.cpu(), k)                                                 # ... which are the rule's
    assert torch.equal(kept.cpu(), rk) and torch.equal(dropped.cpu(), rd), tag
    err = (g_out.cpu().double() - want_g).abs()
    assert float(err.max()) <= 4 * U * float(want_g.abs().max()), (tag, float(err.max()))
    if kept_prev is not None:
        mask = torch.ones_like(g_in, dtype=torch.bool)
        mask.scatter_(1, kept_prev, False)
        assert torch.equal(g_out.cpu()[mask], g_in[mask]), tag                           # the dropped entries keep their bits
    return g_out.cpu(), kept.cpu()


@pytest.mark.parametrize("T", [2, 9, 65, 196])
def test_select_against_float64_and_select_topk(T):
    H = 3
    for B in (1, 3):
        for k in _ks(T):
            gen = torch.Generator().manual_seed(4000 * T + 10 * k + B)
            a0 = torch.softmax(torch.randn(B, H, 1 + T, generator=gen), dim=-1)
            g0, kept0 = _check_select(None, None, a0, 0.5, k, ("start", B, T, k))
            a1 = torch.softmax(torch.randn(B, H, k + 2, generator=gen), dim=-1)
            g1, kept1 = _check_select(g0, kept0, a1, 0.5, k, ("evolve", B, T, k))
            _check_select(g1, kept1, torch.softmax(torch.randn(B, H, k + 2, generator=gen), dim=-1), 0.9, k, ("evolve again", B, T, k))
            # deliberate ties: a few levels, exactly representable, tau = 0.5 keeps them exact
            q0 = torch.randint(1, 4, (B, H, 1 + T), generator=gen).float() / 8
            q0[:, 1:] = q0[:, :1]                                                        # every head the same: the mean is the level itself
            gq, keptq = _check_select(None, None, q0, 0.5, k, ("ties start", B, T, k))
            if T > 2:
                assert any(len(set(row)) < T for row in gq.tolist())
            q1 = torch.randint(1, 4, (B, H, k + 2), generator=gen).float() / 8
            q1[:, 1:] = q1[:, :1]
            _check_select(gq, keptq, q1, 0.5, k, ("ties evolve", B, T, k))
    # all scores equal: the lowest indices are kept
    g_out, kept = _check_select(None, None, torch.full((2, H, 1 + T), 0.25), 0.5, 1, ("flat", T))
    assert kept.tolist() == [[0], [0]]


def test_refusals_leave_poisoned_outputs_untouched():
    from d2s import lib
    lib.load()
    B, T, k, D, H = 2, 5, 2, 8, 2
    f = lambda n: torch.full((n,), POISON, device=DEV)
    i = lambda n: torch.full((n,), 12345, dtype=torch.int64, device=DEV)
    P, st = lib.ptr, lib.stream()
    g_in, kp, cls, g_out, kept, dropped = f(B * T), torch.tensor([[0, 1], [2, 3]], device=DEV), f(B * H * (k + 2)), f(B * T), i(B * k), i(B * (T - k))
    good = [P(g_in), P(kp), P(cls), P(g_out), P(kept), P(dropped), B, H, T, k, 0.5]
    fn = lib._fn("d2s_evo_select")
    for pos, val in [(0, None), (2, None), (3, None), (4, None), (5, None), (6, 0), (7, 0), (8, 1), (8, 4096), (9, 0), (9, T), (10, -0.1), (10, 1.5)]:
        a = list(good)
        a[pos] = val
        assert fn(*a, st) == -1, ("select", pos, val)
    yc, xc, X = f(B * (k + 2) * D), f(B * (k + 2) * D), f(B * (T + 1) * D)
    keptv, droppedv = torch.tensor([[0, 1], [2, 3]], device=DEV), torch.tensor([[2, 3, 4], [0, 1, 4]], device=DEV)
    dims = [(-4, 0), (-3, 1), (-3, 4096), (-2, 0), (-2, T), (-1, 6), (-1, 0), (-1, 1028)]       # B, T, k = 0, k = T, D % 4, D = 0, D > 1024
    goods = [P(yc), P(xc), P(keptv), P(droppedv), P(X), B, T, k, D]
    fs = lib._fn("d2s_evo_scatter_fwd")
    for pos, val in [(p, None) for p in range(5)] + dims:
        a = list(goods)
        a[pos] = val
        assert fs(*a, st) == -1, ("scatter_fwd", pos, val)
    dX, dyc = f(B * (T + 1) * D), f(B * (k + 2) * D)
    goodb = [P(dX), P(keptv), P(droppedv), P(dyc), B, T, k, D]
    fb = lib._fn("d2s_evo_scatter_bwd")
    for pos, val in [(p, None) for p in range(4)] + dims:
        a = list(goodb)
        a[pos] = val
        assert fb(*a, st) == -1, ("scatter_bwd", pos, val)
    dxc, g, S = f(B * (k + 2) * D), f(B * T), f(B)
    goodg = [P(dxc), P(dyc), P(g), P(S), P(keptv), P(droppedv), P(dX), B, T, k, D]
    fg = lib._fn("d2s_evo_gather_bwd")
    for pos, val in [(p, None) for p in range(7)] + dims:
        a = list(goodg)
        a[pos] = val
        assert fg(*a, st) == -1, ("gather_bwd", pos, val)
    torch.cuda.synchronize()
    for t in (g_out, kept, dropped, X, dyc, dX):
        assert bool((t == (12345 if t.dtype == torch.int64 else POISON)).all())


# ---- 2. the model, micro geometry ----
def _geom(name):
    cfg = EVO_CASES[name]["case"]["cfg"]
    return dict(img_size=cfg["img_size"], patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


def _model(name, **kw):
    import vit_models
    sd = built(name)[0]
    c = EVO_CASES[name]
    m = vit_models.VisionTransformerEvo(**_geom(name), evo_start=c["start"], evo_keep=c["keep"], evo_tradeoff=c["tau"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


def _ref(name, sd, images, **kw):
    c = EVO_CASES[name]
    return R.forward(sd, images, c["case"]["cfg"], c["start"], c["keep"], c["tau"], **kw)


TOL = {"exact": (1e-4, 2e-5), "split": (1e-4, 2e-5), "bf16": (3e-2, 3e-2)}     # tests/test_avit_gpu.py's, per arithmetic mode


def _gm(mode):
    from d2s import ops
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}[mode]


@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
@pytest.mark.parametrize("name", sorted(EVO_CASES))
def test_model_forward_against_float64(name, mode):
    import vit_models
    from d2s import ops
    sd, images, _, out = built(name)
    c = EVO_CASES[name]
    cfg = c["case"]["cfg"]
    check_condition(out)
    m = _model(name).eval()
    T = cfg["n_patches"]
    with ops.gemm_mode(_gm(mode)), torch.no_grad():
        logits = m(images.to(DEV))
        kept = [t.cpu() for t in m.evo_kept]
        tokens, score, per_block = m.tokens.cpu(), m.global_score.cpu(), list(m.tokens_per_block)
        alone = []
        for b in range(images.shape[0]):
            alone.append(m(images[b:b + 1].to(DEV)))
            if mode != "bf16":
                assert all(torch.equal(t.cpu()[0], u[b]) for t, u in zip(m.evo_kept, kept))
    k = m.evo_k
    assert len(kept) == cfg["depth"] - c["start"] and all(t.shape == (images.shape[0], k) and t.dtype == torch.int64 for t in kept)
    assert per_block == [T + 1] * c["start"] + [k + 2] * (cfg["depth"] - c["start"])
    assert tokens.shape == (images.shape[0], T + 1, cfg["dim"]) and score.shape == (images.shape[0], T)
    if mode != "bf16":
        assert all(torch.equal(a, b) for a, b in zip(kept, out["kept"]))       # the selection of every block, exactly
        ref = out
    else:                                                                   # bf16 noise may move a selection: the GPU's own are replayed
        print(f"  bf16: {sum(int((a != b).any(dim=1).sum()) for a, b in zip(kept, out['kept']))} kept lists differ from the float64 selection")
        with torch.no_grad():
            ref = _ref(name, {k_: v.double() for k_, v in sd.items()}, images, kept_forced=kept)
    for t in kept:                                                          # absolute patch ids: patch_drop_mask applies
        mask = vit_models.patch_drop_mask([t.to(DEV)], T)[0].cpu()
        assert mask.shape == (images.shape[0], T) and bool((mask.sum(dim=1) == k).all()) and bool(torch.gather(mask, 1, t).bool().all())
    tol = TOL[mode]
    print(f"{name} {mode}: tokens per block {per_block}, max |logits - ref| {float((logits.cpu().double() - ref['logits']).abs().max()):.3e}, "
          f"max |tokens - ref| {float((tokens.double() - ref['tokens']).abs().max()):.3e}")
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"].numpy(), rtol=tol[0], atol=tol[1])
    np.testing.assert_allclose(torch.cat(alone).cpu().numpy(), logits.cpu().numpy(), rtol=tol[0], atol=tol[1])
    np.testing.assert_allclose(score.numpy(), ref["g"].numpy(), rtol=tol[0], atol=tol[1])


def test_training_forward_is_the_eval_forward():
    _, images, _, _ = built("evo2")
    m = _model("evo2")
    x = images.to(DEV)
    a = m.train()(x)
    kept = [t.clone() for t in m.evo_kept]
    with torch.no_grad():
        b = m.eval()(x)
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), b) and a.requires_grad and not b.requires_grad
    assert len(kept) == len(m.evo_kept) == 3 and all(torch.equal(s, t) for s, t in zip(kept, m.evo_kept))


def test_start_at_depth_is_the_teacher_bit_for_bit():
    import vit_models
    sd, images, _, _ = built("evodense")
    m = _model("evodense").eval()
    teacher = vit_models.VisionTransformerTeacher(**_geom("evodense"))
    teacher.load_state_dict(sd)
    teacher = teacher.to(DEV).eval()
    with torch.no_grad():
        a = m(images.to(DEV))
        b, tokens, _ = teacher(images.to(DEV))
    assert torch.equal(a, b) and m.evo_kept == [] and m.global_score.shape == (images.shape[0], 16)


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("name", ["evo1", "evo2", "evo80"])
def test_model_gradients_and_loss_against_float64(name, mode):
    from d2s import ops
    from losses import ToMeLoss
    sd, images, labels, _ = built(name)
    m = _model(name).train()
    fn = ToMeLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0))
    with ops.gemm_mode(_gm(mode)):
        logits = m(images.to(DEV))
        loss = fn(logits, None, labels.to(DEV), {})
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    out = _ref(name, sd64, images)
    want = torch.nn.functional.cross_entropy(out["logits"], labels)
    names = list(sd64)
    grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(m.evo_kept, out["kept"]))
    print(f"{name} {mode}: loss {float(loss.detach()):.7f} float64 {float(want.detach()):.7f}")
    np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4)
    worst = 0.0
    for k, p in m.named_parameters():
        ref = grads[k]
        assert p.grad is not None and ref is not None, k
        rel = float((p.grad.detach().cpu().double() - ref).norm() / ref.norm())
        worst = max(worst, rel)
        assert rel <= 1e-3, (k, rel)
    print(f"  worst relative L2 error of a parameter gradient {worst:.2e}")


def test_bf16_forward_and_backward_run_and_repeat_bit_for_bit():
    from d2s import ops
    from losses import ToMeLoss
    _, images, labels, _ = built("evo1")
    runs = []
    for _ in range(2):
        m = _model("evo1").train()
        fn = ToMeLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0))
        with ops.gemm_mode(ops.GEMM_BF16):
            logits = m(images.to(DEV))
            loss = fn(logits, None, labels.to(DEV), {})
            loss.backward()
            ops.join_weight_grads()
            torch.cuda.synchronize()
        runs.append((logits.detach().clone(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and bool(torch.isfinite(runs[0][0]).all())
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(runs[0][1], runs[1][1]))


# ---- 3. TrainStep ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **kw)


def _step(with_teacher=False, student=None, **kw):
    import vit_models
    from d2s.engine import TrainStep
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**_geom("evo1"))
        teacher.load_state_dict(built("evo1")[0])
        teacher = teacher.to(DEV)
    student = _model("evo1") if student is None else student
    return TrainStep(student, teacher, _args(), lr=1e-3, **kw)


def _xy():
    _, images, labels, _ = built("evo1")
    return images.to(DEV), labels.to(DEV)


@pytest.mark.parametrize("with_teacher", [False, True])
def test_train_step_two_runs_bit_identical_and_resume(with_teacher):
    import vit_models
    from d2s import lib
    x, y = _xy()
    runs = []
    for _ in range(2):
        ts = _step(with_teacher)
        assert ts.method.name == "evo" and ts.logits_only
        losses = [float(ts(x, y)["loss"]) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((losses, ts.arena.params.clone(), ts))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert all(math.isfinite(v) for v in runs[0][0])
    ts = runs[1][2]
    for k in ("train_tome_loss", "train_cls_loss"):
        assert k in ts.metrics and math.isfinite(float(ts.metrics[k])), k
    saved = ts.state_dict()
    cfg = saved["config"]
    assert (cfg["model"], cfg["evo_start"], cfg["evo_keep"], cfg["evo_tradeoff"]) == ("VisionTransformerEvo", 2, 0.5, 0.5)
    ts(x, y)
    torch.cuda.synchronize()
    three = ts.arena.params.clone()
    resumed = _step(with_teacher)
    assert resumed.load_state_dict(saved) == saved["epoch"]
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three)                          # 2 steps, a checkpoint, 1 more step = 3 straight steps
    other = vit_models.VisionTransformerEvo(**_geom("evo1"), evo_start=2, evo_keep=0.25).to(DEV)
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: evo_keep"):
        _step(with_teacher, student=other).load_state_dict(saved)


def test_train_step_accumulation_with_clipping():
    x, y = _xy()
    ts = _step(accum_steps=2, clip_grad=0.5)
    before = ts.arena.params.clone()
    a = ts(x, y)
    assert a["stepped"] is False and torch.equal(ts.arena.params, before)
    b = ts(x, y)
    torch.cuda.synchronize()
    assert b["stepped"] is True and not torch.equal(ts.arena.params, before) and float(b["grad_norm"]) > 0
    assert math.isfinite(float(b["loss"])) and float(a["loss"]) == float(b["loss"])          # the same batch before any update


@pytest.mark.parametrize("with_teacher", [False, True])
def test_graph_step_is_bit_identical_to_eager(with_teacher):
    x, y = _xy()
    eager, graph = _step(with_teacher, graph=False), _step(with_teacher, graph=True)
    assert eager.graph is False and graph.graph is True
    captured = []
    for i in range(graph.GRAPH_WARM_STEPS + 2):                              # the warm steps run eagerly, then two replays
        ie, ig = eager(x, y), graph(x, y)
        torch.cuda.synchronize()
        assert torch.equal(ie["loss"], ig["loss"]) and torch.equal(ie["logits_s"].detach(), ig["logits_s"].detach()), i
        assert torch.equal(eager.arena.grads, graph.arena.grads), i
        assert torch.equal(eager.arena.params, graph.arena.params), i
        captured.append(graph.last_step_captured)
        assert not eager.last_step_captured
    assert captured == [False] * graph.GRAPH_WARM_STEPS + [True, True], captured
    for k, v in eager.metrics.items():
        assert float(v) == float(graph.metrics[k]), k


def test_train_step_refusals_by_message():
    from d2s import lib
    from d2s.engine import TrainStep
    m = _model("evo1")
    with pytest.raises(ValueError, match="warmup_steps 2 with an Evo-ViT student"):
        TrainStep(m, None, _args(), warmup_steps=2)
    m.drop_path_rate = 0.1
    with pytest.raises(lib.D2SError, match="Evo-ViT student and drop_path_rate > 0"):
        TrainStep(m, None, _args())


def test_grad_ready_hook_once_per_block_in_descending_order():
    from losses import ToMeLoss
    _, images, labels, _ = built("evo1")
    m = _model("evo1").train()
    seen = []
    m.grad_ready_hook = seen.append
    loss = ToMeLoss(types.SimpleNamespace(mixup=0.0, dist_weight=0.0))(m(images.to(DEV)), None, labels.to(DEV), {})
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [3, 2, 1, 0], seen


# ---- 4. command line ----
def test_cli_trains_one_tiny_epoch_and_evaluates_the_checkpoint(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "evo", "--evo-start", "10", "--evo-keep", "0.25", "--epochs", "1",
                               "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--student-checkpoint", path,
                               "--dist-weight", "0", "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Start training" in out and "val loss:" in out
    assert "--method evo --evo-start 10 --evo-keep 0.25 --evo-tradeoff 0.5: tokens per block [197, 197, 197, 197, 197, 197, 197, 197, 197, 197, 51, 51]" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert (cfg["model"], cfg["evo_start"], cfg["evo_keep"], cfg["evo_tradeoff"]) == ("VisionTransformerEvo", 10, 0.25, 0.5)
    acc2 = mask_predictor.main(["--arch", "deit_tiny", "--method", "evo", "--evo-start", "10", "--evo-keep", "0.25", "--eval-only",
                                "--resume", os.path.join(out_dir, "last.pt"), "--val-steps", "1", "--batch-size", "4", "--dist-weight", "0"])
    out = capsys.readouterr().out
    assert "eval only:" in out and isinstance(acc2, float) and 0.0 <= acc2 <= 1.0
