"""Token fusion (fuse_dropped) on the GPU: the two kernels of csrc/fuse.hip against the float64 restatement (tests/fuse_ref.py) with
derived bounds, their copy rows bit for bit, determinism, the student with DF.GatherFuseFn against the same student with that one
Function replaced by torch ops, TrainStep (the new gradient path, the flag off = the parent's path, graph mode), the C entries' refusal of
an unsupported width and the checkpoint round trip.  Every shape is the smallest that reaches its code path."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import fuse_ref as R
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
B = 3

# (n, t, k): one dropped token / one kept token / an empty dropped set / a carried row / a dropped set that crosses a wavefront and
# leaves the four waves unequal quarters / DeiT-S at keep 0.5 (more than one 16-row workgroup of the backward) / a second stage of it
SHAPES = [(6, 0, 1), (6, 0, 4), (6, 0, 5), (18, 1, 8), (70, 2, 30), (197, 0, 98), (100, 1, 49)]


def _ops():
    from d2s import ops
    return ops


def _inputs(n, t, k, D, seed=0, tiny=False):
    """p: a softmax of random scores; kept / dropped from the library's own top-k.  tiny: image 0's dropped probabilities are 1e-30 of
    what they were (the selection is unchanged), so S ~ 1e-32 and the 1 / S path runs far from 1."""
    import d2s.functional as DF
    gen = torch.Generator().manual_seed(seed + 1000 * n + 10 * k + t)
    T = n - 1 - t
    x = torch.randn((B, n, D), generator=gen)
    p = torch.softmax(torch.randn((B, T), generator=gen), dim=-1)
    g = torch.randn((B, k + t + 2, D), generator=gen)
    kept, dropped = DF.select_topk(p.to(DEV), k)
    if tiny:
        scale = torch.ones_like(p)
        scale[0].scatter_(0, dropped[0].cpu(), 1e-30)
        p = p * scale
        k2, d2 = DF.select_topk(p.to(DEV), k)
        assert torch.equal(k2, kept) and torch.equal(d2, dropped)
    return x, p, g, kept, dropped


def _check_against_float64(n, t, k, D, tiny=False):
    """Bounds.  u = 2^-24, m = T - k dropped tokens.  A sum of L fp32 products in any order errs by at most (L + 2) u sum|terms| (one
    rounding per product, L - 1 per addition chain, to first order); 4 x that is allowed, which also covers second-order terms and the
    few u that the weights carry (below).
      f_c   = sum_j w_j x_jc                       4 (m + 2) u sum_j |w_j x_jc|
      dp_j  = (<x_j, g_f> - <f, g_f>) / S          4 (2 D + 2) u (sum_c |x_jc g_c| + sum_c |f_c g_c|) / S
      dx_jc = w_j g_c  (dropped j)                 (ceil(m / 256) + 10) u |w_j g_c|: one product of w_j = p_j / S.  S is a sum of positive
              terms taken as per-thread partials (ceil(m / 256) - 1 additions), a 6-step wave butterfly and 2 additions across the waves,
              so its relative error is at most (ceil(m / 256) + 7) u; the division and the product add one rounding each, and one u is
              left for second-order terms.  No factor 4 here.
    CLS, kept and carried rows are copies: exact.  dp at kept ids is exactly 0."""
    ops = _ops()
    x, p, g, kept, dropped = _inputs(n, t, k, D, tiny=tiny)
    T, m = n - 1 - t, n - 1 - t - k
    xd, pd, gd = x.to(DEV), p.to(DEV), g.to(DEV)
    y, S = ops.gather_fuse_fwd(xd, pd, kept, dropped, t)
    dx, dp = ops.gather_fuse_bwd(gd, xd, pd, S, y, kept, dropped, t)
    torch.cuda.synchronize()
    y, S, dx, dp, kc, dc = y.cpu(), S.cpu(), dx.cpu(), dp.cpu(), kept.cpu(), dropped.cpu()
    assert y.shape == (B, k + t + 2, D) and S.shape == (B,) and dx.shape == (B, n, D) and dp.shape == (B, T)
    # ---- copies, bit for bit
    rows = lambda a, ids: torch.gather(a, 1, ids[:, :, None].expand(B, ids.shape[1], D))
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(y[:, 1:1 + k], rows(x[:, 1:1 + T], kc))
    assert torch.equal(y[:, 1 + k:1 + k + t], x[:, 1 + T:])
    assert torch.equal(dx[:, 0], g[:, 0]) and torch.equal(rows(dx[:, 1:1 + T], kc), g[:, 1:1 + k])
    assert torch.equal(dx[:, 1 + T:], g[:, 1 + k:1 + k + t])
    assert bool((torch.gather(dp, 1, kc) == 0).all())
    # ---- float64
    x64, p64, g64 = x.double(), p.double(), g.double()
    y64, dx64, dp64 = R.fuse_autograd(x64, p64, kc, dc, t, g64)
    if m == 0:
        assert bool((y[:, -1] == 0).all()) and bool((dp == 0).all()) and bool((S == 0).all())
        return
    pd64 = torch.gather(p64, 1, dc)
    S64 = pd64.sum(dim=1, keepdim=True)
    w64 = pd64 / S64
    xd64 = rows(x64[:, 1:1 + T], dc)
    f64, gf64 = y64[:, -1], g64[:, -1]
    np.testing.assert_allclose(S.double().numpy(), S64[:, 0].numpy(), rtol=(m + 2) * EPS)
    checks = [("f", y[:, -1], f64, (w64[:, :, None] * xd64).abs().sum(dim=1), 4.0 * (m + 2)),
              ("dx dropped", rows(dx[:, 1:1 + T], dc), rows(dx64[:, 1:1 + T], dc), (w64[:, :, None] * gf64[:, None, :]).abs(),
               float((m + 255) // 256 + 10)),
              ("dp", torch.gather(dp, 1, dc), torch.gather(dp64, 1, dc),
               ((xd64 * gf64[:, None, :]).abs().sum(-1) + (f64 * gf64).abs().sum(-1, keepdim=True)) / S64, 4.0 * (2 * D + 2))]
    for name, got, want, mag, units in checks:
        bound = units * EPS * mag
        err = (got.double() - want).abs()
        frac = float((err / bound.clamp_min(1e-300)).max())
        print(f"[fuse n={n} t={t} k={k} D={D} tiny={tiny}] {name}: largest fraction of the bound {frac:.3f}, max abs err {float(err.max()):.3e}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (name, frac)


# ---- 1. kernels against float64 ----
@pytest.mark.parametrize("D", [64, 192, 384])
@pytest.mark.parametrize("n,t,k", SHAPES)
def test_kernels_against_float64_within_the_derived_bounds(n, t, k, D):
    _check_against_float64(n, t, k, D)


def test_kernels_with_a_vanishing_dropped_mass():
    _check_against_float64(70, 2, 30, 192, tiny=True)


# ---- 2. determinism ----
def test_two_runs_are_bit_identical():
    ops = _ops()
    n, t, k, D = 197, 0, 98, 384
    x, p, g, kept, dropped = _inputs(n, t, k, D, seed=2)
    x, p, g = x.to(DEV), p.to(DEV), g.to(DEV)

    def run():
        y, S = ops.gather_fuse_fwd(x, p, kept, dropped, t)
        return (y, S) + ops.gather_fuse_bwd(g, x, p, S, y, kept, dropped, t)
    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


# ---- 3. the model ----
def _student(case, fuse=None, **kw):
    """fuse None: the constructor is called without the argument at all"""
    import vit_models
    cfg = case["cfg"]
    student, teacher, _, _ = build_models(case, torch.device(DEV))
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    if fuse is not None:
        kw["fuse_dropped"] = fuse
    m = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
                                                topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                small_predictor=cfg["small_predictor"], init_n=cfg["init_n"], **common, **kw)
    m.load_state_dict(student.state_dict(), strict=True)
    return m.to(DEV), teacher


def _probe_run(case, x, monkeypatch, torch_fn):
    """logits, features and the gradients of a fixed linear probe on both"""
    import d2s.functional as DF
    ops = _ops()
    student, _ = _student(case, True)
    student.train()
    if torch_fn:
        monkeypatch.setattr(DF, "GatherFuseFn", R.TorchGatherFuse)
    logits, features, pred_logits, kept = student(x)
    gen = torch.Generator().manual_seed(21)
    wl, wf = torch.randn(logits.shape, generator=gen).to(DEV), torch.randn(features.shape, generator=gen).to(DEV)
    ((logits * wl).sum() + (features * wf).sum()).backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {n: p.grad.detach().cpu().clone() for n, p in student.named_parameters()
             if n.startswith(("score_predictor.", "blocks.0.")) and p.grad is not None}
    return logits.detach().cpu(), features.detach().cpu(), [k.cpu() for k in kept], grads


def test_student_matches_the_torch_restatement_of_the_one_function(monkeypatch):
    """micro2: two stages, so the second one carries a package row (t = 1).  Everything but GatherFuseFn is the same HIP path in both
    runs; tolerances are those of tests/test_model_gpu.py's train-step parity (logits rtol 1e-4 / atol 2e-5, tokens atol 3e-5, gradient
    norms rtol 1e-3, full gradient tensors 3e-3 relative L2)."""
    case = cases.MODEL_CASES["micro2"]
    cfg = case["cfg"]
    x = _t(cases.make_images(case)).to(DEV)
    la, fa, ka, ga = _probe_run(case, x, monkeypatch, False)
    lb, fb, kb, gb = _probe_run(case, x, monkeypatch, True)
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    assert fa.shape == (case["batch"], ks[-1], cfg["dim"])                     # k_S feature rows: the package rows are left out
    assert all(torch.equal(a, b) for a, b in zip(ka, kb)) and [k.shape[1] for k in ka] == ks
    np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(fa.numpy(), fb.numpy(), rtol=1e-4, atol=3e-5)
    names = sorted(ga)
    assert names == sorted(gb) and sum(n.startswith("score_predictor.") for n in names) == 48 and any(n.startswith("blocks.0.") for n in names)
    for n in names:
        a, b = ga[n].double().flatten(), gb[n].double().flatten()
        np.testing.assert_allclose(float(a.norm()), float(b.norm()), rtol=1e-3, atol=1e-6, err_msg=n)
        assert float((a - b).norm()) <= 3e-3 * float(b.norm()) + 1e-6, n
    # the probe reads no mask loss: whatever reaches stage 0's predictor came through the fusion weights (a few of its gradients are
    # exactly zero in exact arithmetic - the keep probabilities do not move with a constant added to every score)
    assert any(float(ga[n].abs().max()) > 0 for n in names if n.startswith("score_predictor.0."))


def test_eval_tuple_shapes():
    """eval(): (logits, cls_attns, pred_logits, kept) with the package rows in the sequence - after stage s it has 1 + k_s + s + 1 rows,
    so a block's CLS row without its own column has k_s + s + 1 entries; pred_logits and kept keep their shapes"""
    case = cases.MODEL_CASES["micro2"]
    cfg = case["cfg"]
    x = _t(cases.make_images(case)).to(DEV)
    student, _ = _student(case, True)
    student.eval()
    with torch.no_grad():
        logits, cls_attns, pred_logits, kept = student(x)
    Bc, N = case["batch"], (cfg["img_size"] // cfg["patch"]) ** 2
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    assert logits.shape == (Bc, cfg["num_classes"])
    want, n = [], N + 1
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            s = list(cfg["pruning_loc"]).index(i)
            n = 1 + ks[s] + s + 1
        want.append(n - 1)
    assert [c.shape[-1] for c in cls_attns] == want == [16, 10, 7, 7]
    assert [tuple(k.shape) for k in kept] == [(Bc, k) for k in ks]
    assert [tuple(pl.shape) for pl in pred_logits] == [(Bc, N), (Bc, ks[0])]
    assert [tuple(d.shape) for d in student.dropped_token_indices] == [(Bc, N - ks[0]), (Bc, ks[0] - ks[1])]
    student.kept_token_override = [k.clone() for k in kept]                  # replaying the selection: dropped is derived from it
    with torch.no_grad():
        again = student(x)[0]
    assert torch.equal(again, logits)


# ---- 4. TrainStep ----
def _steps(case, fuse, n, graph=False, parent_head=False, spy=None):
    import d2s.functional as DF
    from d2s.engine import TrainStep
    student, teacher = _student(case, fuse)
    if parent_head:          # the head call as it was before the feature: no tail argument at all
        student._head = lambda x, tail=0: DF.run(DF.HeadFn, x, student.norm.weight, student.norm.bias, student.head.weight,
                                                 student.head.bias, student.norm.eps)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=graph)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(5)
    rec = []
    for _ in range(n):
        info = ts(x, y)
        torch.cuda.synchronize()
        pred = torch.cat([ts.arena.grad_views[nm].flatten() for nm, _ in student.named_parameters() if nm.startswith("score_predictor.")])
        rec.append((info["loss"].detach().clone(), ts.arena.params.clone(), pred.clone()))
    return rec, ts


def test_train_steps_are_finite_and_the_predictor_gets_the_new_gradient():
    case = cases.MODEL_CASES["micro2"]
    on, _ = _steps(case, True, 3)
    off, _ = _steps(case, False, 3)
    assert all(bool(torch.isfinite(r[0])) and bool(torch.isfinite(r[1]).all()) for r in on)
    assert not torch.equal(on[0][2], off[0][2]), "the task loss must reach the predictor through the fusion weights"
    assert bool(torch.isfinite(on[0][2]).all()) and not torch.equal(on[2][1], off[2][1])


def test_flag_off_is_the_parent_path_bit_for_bit(monkeypatch):
    """fuse_dropped=False against the constructor called without the argument, its head called the way it was before the feature, and
    GatherFuseFn made unusable: GatherFn runs once per stage and step, and losses and parameters are the same bits."""
    import d2s.functional as DF
    case = cases.MODEL_CASES["micro2"]
    off, _ = _steps(case, False, 3)
    calls = []
    orig = DF.GatherFn.apply

    class Never:
        @staticmethod
        def apply(*a):
            raise AssertionError("GatherFuseFn must not run with the flag off")
    monkeypatch.setattr(DF, "GatherFuseFn", Never)
    monkeypatch.setattr(DF.GatherFn, "apply", staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    parent, _ = _steps(case, None, 3, parent_head=True)
    assert len(calls) == 3 * len(case["cfg"]["pruning_loc"])
    for a, b in zip(off, parent):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_graph_step_is_bit_identical_to_the_eager_step():
    from d2s.engine import TrainStep
    from tests.test_graph_gpu import _same_step, _batches
    case = cases.MODEL_CASES["micro2"]
    eager, graph = [TrainStep(*_student(case, True), make_args(case["cfg"]), warmup_steps=0, graph=gr) for gr in (False, True)]
    for i, (x, y) in enumerate(_batches(case, eager.GRAPH_WARM_STEPS + 1, torch.device(DEV))):
        _same_step(eager, graph, x, y, f"step {i}")
    assert graph.last_step_captured and not eager.last_step_captured


# ---- 5. boundary ----
def test_c_entries_refuse_an_unsupported_width_without_launching():
    """D = 72 is a multiple of 4 (the neighbours would take it) but not of 64: D2S_ERR_ARG (-1) from both entries, before any launch -
    the outputs keep their fill and the device reports no error afterwards"""
    from d2s import lib
    n, t, k, D = 6, 0, 2, 72
    x, p, g = torch.randn((B, n, D), device=DEV), torch.softmax(torch.randn((B, 5), device=DEV), -1), torch.randn((B, 4, D), device=DEV)
    kept = torch.tensor([[0, 1]] * B, device=DEV)
    dropped = torch.tensor([[2, 3, 4]] * B, device=DEV)
    y, S = torch.full((B, 4, D), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    dx, dp = torch.full((B, n, D), 7.0, device=DEV), torch.full((B, 5), 7.0, device=DEV)
    fn = lib.load()
    rc = fn.d2s_gather_fuse_fwd(lib.ptr(x), lib.ptr(p), lib.ptr(kept), lib.ptr(dropped), lib.ptr(y), lib.ptr(S), B, n, t, k, D, lib.stream())
    assert rc == -1
    rc = fn.d2s_gather_fuse_bwd(lib.ptr(g), lib.ptr(x), lib.ptr(p), lib.ptr(S), lib.ptr(y), lib.ptr(kept), lib.ptr(dropped), lib.ptr(dx),
                                lib.ptr(dp), B, n, t, k, D, lib.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in (y, S, dx, dp))
    with pytest.raises(lib.D2SError, match="d2s_gather_fuse_fwd failed with code -1"):
        _ops().gather_fuse_fwd(x, p, kept, dropped, t)


def test_checkpoint_round_trips_the_flag():
    from d2s import lib
    case = cases.MODEL_CASES["micro1"]
    rec, ts = _steps(case, True, 2)
    sd = ts.state_dict(epoch=0)
    assert sd["config"]["fuse_dropped"] is True
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    want = ts(x, y)["loss"].detach().clone()
    _, ts2 = _steps(case, True, 0)
    ts2.load_state_dict(sd)
    assert ts2.student.fuse_dropped is True and torch.equal(ts2.arena.params, rec[1][1])
    got = ts2(x, y)["loss"].detach()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    _, ts0 = _steps(case, False, 0)
    with pytest.raises(lib.D2SError, match="fuse_dropped"):
        ts0.load_state_dict(sd)
    old = dict(sd, config={k: v for k, v in sd["config"].items() if k != "fuse_dropped"})
    with pytest.raises(lib.D2SError, match="fuse_dropped"):
        ts2.load_state_dict(old)                 # a checkpoint written before the flag existed counts as off
    ts0.load_state_dict(dict(old, config=dict(old["config"])))
