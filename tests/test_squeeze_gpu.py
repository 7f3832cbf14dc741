"""Pruning and squeezing (squeeze_dropped) on the GPU: the three kernels of csrc/squeeze.hip against the float64
restatement (tests/squeeze_ref.py) - the match exactly, the merge and its backward within bounds derived from the kernels' roundings
(squeeze_ref.C_MERGE / C_BWD, validated on these very inputs by tests/test_squeeze_cpu.py) -, their copies bit for bit, determinism, the
entries' refusals, the student against the float64 forward with ids and plans replayed, TrainStep and the command line.  Inputs and
seeds are squeeze_ref's; every shape is the smallest that reaches its code path."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests import squeeze_ref as R
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
E32 = 2.71828174591064453125          # expf(1.0f): the weight of a kept token, and Z of a row without a source
_CACHE = {}


def _ops():
    from d2s import ops
    return ops


def _case(shape):
    """One run of the three kernels per shape and its float64 references, shared by the tests below (never modified)"""
    if shape not in _CACHE:
        ops = _ops()
        x, kept, dropped, g = R.inputs(shape)
        xd, kd, dd, gd = x.to(DEV), kept.to(DEV), dropped.to(DEV), g.to(DEV)
        dst, sim = ops.squeeze_match(xd, kd, dd)
        buf = torch.full((xd.shape[0] * (shape[2] + 1) * shape[3] + 4096,), 7.0, device=DEV)          # y followed by a guard band
        y, Z = ops.gather_squeeze_fwd(xd, kd, dd, dst, sim)
        from d2s import lib
        Zg = torch.empty_like(Z)
        rc = lib._fn("d2s_gather_squeeze_fwd")(lib.ptr(xd), lib.ptr(kd), lib.ptr(dd), lib.ptr(dst), lib.ptr(sim), shape[0], shape[1] + 1,
                                               shape[2], shape[3], lib.ptr(buf), lib.ptr(Zg), lib.stream())
        dx = torch.full((shape[0], shape[1] + 1, shape[3]), float("nan"), device=DEV)
        rcb = lib._fn("d2s_gather_squeeze_bwd")(lib.ptr(gd), lib.ptr(kd), lib.ptr(dd), lib.ptr(dst), lib.ptr(sim), lib.ptr(Z), shape[0],
                                                shape[1] + 1, shape[2], shape[3], lib.ptr(dx), lib.stream())
        torch.cuda.synchronize()
        again = ops.squeeze_match(xd, kd, dd) + ops.gather_squeeze_fwd(xd, kd, dd, dst, sim) + (ops.gather_squeeze_bwd(gd, kd, dd, dst, sim, Z, shape[1] + 1),)
        torch.cuda.synchronize()
        x64 = x.double()
        dst64, sim64 = R.match(x64, kept, dropped)
        _CACHE[shape] = dict(x=x, kept=kept, dropped=dropped, g=g, dst=dst.cpu(), sim=sim.cpu(), y=y.cpu(), Z=Z.cpu(), dx=dx.cpu(),
                             rc=(rc, rcb), buf=buf.cpu(), Zg=Zg.cpu(), again=[t.cpu() for t in again], dst64=dst64, sim64=sim64)
    return _CACHE[shape]


# ---- 1. match ----
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_match_is_the_float64_argmax_and_two_runs_are_bit_identical(shape):
    """dst: exactly the float64 argmax on every dropped token (the inputs separate best and second best by 4 x the fp32 worst case:
    tests/test_squeeze_cpu.py); sim: within (2 D + 8) 2^-24 of the float64 cosine, squeeze_ref.margin's derivation"""
    B, T, k, D = shape
    c = _case(shape)
    assert c["dst"].dtype == torch.int32 and c["dst"].shape == (B, T - k) and c["sim"].shape == (B, T - k)
    assert torch.equal(c["dst"], c["dst64"])
    err = float((c["sim"].double() - c["sim64"]).abs().max())
    print(f"match {shape}: max |sim - float64| {err:.3e} = {err / ((2 * D + 8) * U):.3f} of the bound")
    assert err <= (2 * D + 8) * U
    for a, b in zip(c["again"], (c["dst"], c["sim"], c["y"], c["Z"], c["dx"])):
        assert torch.equal(a, b)


def test_match_resolves_bit_identical_kept_rows_to_the_lower_position_and_a_zero_row_to_zero():
    ops = _ops()
    x, kept, dropped, pos = R.duplicate_inputs()
    x[0, 1 + dropped[0, 5]] = 0                                   # a zero dropped row: every cosine 0, the first position
    x[0, 1 + kept[0, 0]] = 0                                      # a zero kept row: cosine 0 with everyone
    dst, sim = ops.squeeze_match(x.to(DEV), kept.to(DEV), dropped.to(DEV))
    dst, sim = dst.cpu(), sim.cpu()
    d64, s64 = R.match(x.double(), kept, dropped)
    assert [int(dst[0, i]) for i in pos] == [4, 4] == [int(d64[0, i]) for i in pos]
    assert float(sim[0, 5]) == 0.0 and int(dst[0, 5]) == 0
    assert bool(torch.isfinite(sim).all()) and float((sim.double() - s64).abs().max()) <= (2 * x.shape[-1] + 8) * U
    # the tie is exact in the kernel too: the duplicate wins when the lower position is taken away
    kept2 = torch.cat([kept[:, :4], kept[:, 5:]], dim=1).contiguous()
    dropped2 = torch.sort(torch.cat([dropped, kept[:, 4:5]], dim=1), dim=1)[0].contiguous()
    dst2, sim2 = ops.squeeze_match(x.to(DEV), kept2.to(DEV), dropped2.to(DEV))
    where = [int((dropped2[0] == dropped[0, i]).nonzero()) for i in pos]
    assert [int(dst2[0, w]) for w in where] == [10, 10] and [float(sim2[0, w]) for w in where] == [float(sim[0, i]) for i in pos]


# ---- 2. merge forward ----
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_merge_forward_on_the_kernels_own_plans(shape):
    """Rows without a source and the CLS row bit for bit; a row with s sources within (s + C_MERGE) 2^-24 (sum_i w_i |x_i|) / Z of float64
    (squeeze_ref derives C_MERGE = 8; the float64 merge takes the kernel's fp32 sim as given); Z by the same rule; nothing behind y"""
    B, T, k, D = shape
    c = _case(shape)
    x, kept, dropped, dst, sim = c["x"], c["kept"], c["dropped"], c["dst"], c["sim"]
    y64, Z64 = R.merge(x.double(), kept, dropped, dst, sim.double())
    by, bz, s = R.merge_bounds(x.double(), kept, dropped, dst, sim.double())
    y, Z = c["y"], c["Z"]
    assert y.shape == (B, k + 1, D) and Z.shape == (B, k) and int(s.sum()) == B * (T - k)
    assert torch.equal(y[:, 0], x[:, 0]) and torch.equal(y[:, 1:][s == 0], R.rows(x, kept)[s == 0])
    assert bool((Z[s == 0] == E32).all())
    fy = float(((y[:, 1:].double() - y64[:, 1:]).abs() / by.clamp_min(1e-300))[s > 0].max())
    fz = float(((Z.double() - Z64).abs() / bz)[s > 0].max())
    print(f"merge {shape}: up to {int(s.max())} sources per row; max err / bound: y {fy:.3f}, Z {fz:.3f}")
    assert bool(torch.isfinite(y).all()) and fy <= 1.0 and fz <= 1.0
    n_out = B * (k + 1) * D
    assert c["rc"] == (0, 0) and torch.equal(c["buf"][:n_out].reshape(B, k + 1, D), y) and torch.equal(c["Zg"], Z)
    assert bool((c["buf"][n_out:] == 7).all())


def test_an_empty_dropped_set_is_gather_pack_bit_for_bit():
    ops = _ops()
    B, T, D = 2, 33, 128
    x = torch.randn((B, T + 1, D), generator=torch.Generator().manual_seed(5)).to(DEV)
    kept = torch.arange(T, device=DEV).expand(B, -1).contiguous()
    nobody = torch.empty((B, 0), dtype=torch.int64, device=DEV)
    dst, sim = ops.squeeze_match(x, kept, nobody)
    y, Z = ops.gather_squeeze_fwd(x, kept, nobody, dst, sim)
    assert dst.shape == (B, 0) and torch.equal(y, ops.gather_pack(x, kept)) and bool((Z == E32).all())
    g = torch.randn_like(y)
    assert torch.equal(ops.gather_squeeze_bwd(g, kept, nobody, dst, sim, Z, T + 1), ops.scatter_unpack(g, kept, T + 1))


def test_a_stage_that_keeps_no_token_is_gather_fn():
    """k == 0: there is nothing to squeeze into - GatherSqueezeFn hands the stage to the kernels of GatherFn, forward and backward"""
    import d2s.functional as DF
    B, T, D = 2, 5, 64
    x = torch.randn((B, T + 1, D), generator=torch.Generator().manual_seed(6)).to(DEV).requires_grad_(True)
    nobody = torch.empty((B, 0), dtype=torch.int64, device=DEV)
    everyone = torch.arange(T, device=DEV).expand(B, -1).contiguous()
    y, dst, sim = DF.GatherSqueezeFn.apply(x, nobody, everyone, None)
    want = DF.GatherFn.apply(x, nobody)
    assert y.shape == (B, 1, D) and torch.equal(y, want) and dst.shape == (B, 0) and sim.shape == (B, 0)
    g = torch.randn_like(y)
    (dx,), (dx_want,) = torch.autograd.grad(y, x, g), torch.autograd.grad(want, x, g)
    assert torch.equal(dx, dx_want) and torch.equal(dx[:, 0], g[:, 0]) and bool((dx[:, 1:] == 0).all())


# ---- 3. merge backward ----
def _check_backward(x, kept, dropped, dst, sim, g, y, dx):
    """dx against the closed form in float64.  A scaled row is fl(fl(a / Z) g): one rounding for the ratio, one for the product, and 6 u
    carried by the operands (squeeze_ref.C_BWD = 8); copied rows (CLS, kept rows without a source) are g's rows bit for bit; and
    <dx, x> = <g, y> - the forward is linear in x for a fixed plan - from the kernels' outputs, summed in float64"""
    ref = R.merge_backward(g.double(), kept, dropped, dst, sim.double(), x.shape[1])
    _, _, s = R.merge_bounds(x.double(), kept, dropped, dst, sim.double())
    got = dx.double()
    assert bool(torch.isfinite(dx).all())                                            # every element of the poisoned buffer was overwritten
    err = (got - ref).abs()
    worst = float((err / (ref.abs() + 1e-300)).max())
    print(f"  backward: worst relative error {worst / U:.3f} u (bound {R.C_BWD} u)")
    assert bool((err <= R.C_BWD * U * ref.abs()).all())
    assert torch.equal(dx[:, 0], g[:, 0]) and torch.equal(R.rows(dx, kept)[s == 0], g[:, 1:][s == 0])
    lhs, rhs = float((got * x.double()).sum()), float((g.double() * y.double()).sum())
    print(f"  <dx, x> = {lhs:.9e}, <g, y> = {rhs:.9e}")
    assert lhs == pytest.approx(rhs, rel=1e-5)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_merge_backward_against_the_closed_form_in_float64(shape):
    c = _case(shape)
    assert c["dx"].shape == c["x"].shape
    _check_backward(c["x"], c["kept"], c["dropped"], c["dst"], c["sim"], c["g"], c["y"], c["dx"])
    assert float(R.rows(c["dx"], c["dropped"]).abs().sum(-1).min()) > 0              # every dropped token receives a gradient


def test_ten_dropped_tokens_on_one_destination_and_entries_that_are_no_plan():
    ops = _ops()
    x, _, _, _ = R.inputs((2, 17, 8, 192))
    T, k, D = 17, 7, 192
    kept, dropped = torch.arange(k).expand(2, -1).contiguous(), torch.arange(k, T).expand(2, -1).contiguous()
    dst = torch.tensor([[3] * 10, [6] * 10], dtype=torch.int32)
    sim = torch.linspace(-1, 1, 10).expand(2, -1).contiguous()
    g = torch.randn((2, k + 1, D), generator=torch.Generator().manual_seed(8))
    dev = lambda *ts: [t.to(DEV) for t in ts]
    xd, kd, dd, dstd, simd, gd = dev(x, kept, dropped, dst, sim, g)
    y, Z = ops.gather_squeeze_fwd(xd, kd, dd, dstd, simd)
    dx = ops.gather_squeeze_bwd(gd, kd, dd, dstd, simd, Z, T + 1)
    y64, Z64 = R.merge(x.double(), kept, dropped, dst, sim.double())
    by, bz, s = R.merge_bounds(x.double(), kept, dropped, dst, sim.double())
    assert int(s.max()) == 10 and bool(((y.cpu()[:, 1:].double() - y64[:, 1:]).abs() <= by).all()) and bool(((Z.cpu().double() - Z64).abs() <= bz).all())
    _check_backward(x, kept, dropped, dst, sim, g, y.cpu(), dx.cpu())
    # no plan: a dst outside [0, k), a dropped id outside [0, T) and a kept id outside it contribute nothing and are never dereferenced
    bad_dst, bad_drop, bad_kept = dst.clone(), dropped.clone(), kept.clone()
    bad_dst[0, 0], bad_dst[0, 1], bad_drop[1, 2], bad_kept[1, 0] = -1, 99, 1 << 40, -5
    kb, db, tb = dev(bad_kept, bad_drop, bad_dst)
    mdst, msim = ops.squeeze_match(xd, kb, db)
    y2, Z2 = ops.gather_squeeze_fwd(xd, kb, db, tb, simd)
    dx2 = torch.full((2, T + 1, D), float("nan"), device=DEV)
    from d2s import lib
    rc = lib._fn("d2s_gather_squeeze_bwd")(lib.ptr(gd), lib.ptr(kb), lib.ptr(db), lib.ptr(tb), lib.ptr(simd), lib.ptr(Z2), 2, T + 1, k, D,
                                           lib.ptr(dx2), lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(y2).all()) and bool(torch.isfinite(dx2).all()) and bool(torch.isfinite(msim).all())
    assert int(mdst[1, 2]) == -1 and float(msim[1, 2]) == 0 and bool((mdst[1, [0, 1, 3]] >= 1).all())   # kept position 0 of image 1 is no candidate
    keep = torch.ones(10, dtype=torch.bool)
    keep[:2] = False
    rest = (x[:1].double(), kept[:1], dropped[:1][:, keep], dst[:1][:, keep], sim[:1][:, keep].double())
    assert bool(((y2[:1].cpu()[:, 1:].double() - R.merge(*rest)[0][:, 1:]).abs() <= R.merge_bounds(*rest)[0]).all())   # image 0: the two entries are in no sum
    assert bool((dx2[0, 1 + k] == 0).all()) and bool((dx2[0, 2 + k] == 0).all()) and bool((dx2[1, 1 + k + 2] == 0).all())
    assert bool((dx2[1, 1] == 0).all())                                              # token 0 of image 1 is in neither list now


# ---- 4. refusals ----
def test_the_three_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, n, k, D = 2, 9, 3, 128
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    x, g, sim, Z, y, dx = f(B, 5000, D), f(B, 5000, D), f(B, 5000), f(B, 5000), f(B, 5000, D), f(B, 5000, D)
    kept, dropped = torch.zeros((B, 5000), dtype=torch.int64, device=DEV), torch.zeros((B, 5000), dtype=torch.int64, device=DEV)
    dst = torch.full((B, 5000), 7, dtype=torch.int32, device=DEV)
    p, s = lib.ptr, lib.stream()

    def match(x_=x, k_=kept, d_=dropped, B_=B, n_=n, kk=k, D_=D, o1=dst, o2=sim):
        return lib._fn("d2s_squeeze_match")(p(x_), p(k_), p(d_), B_, n_, kk, D_, p(o1), p(o2), s)

    def fwd(x_=x, k_=kept, d_=dropped, t_=dst, s_=sim, B_=B, n_=n, kk=k, D_=D, o1=y, o2=Z):
        return lib._fn("d2s_gather_squeeze_fwd")(p(x_), p(k_), p(d_), p(t_), p(s_), B_, n_, kk, D_, p(o1), p(o2), s)

    def bwd(g_=g, k_=kept, d_=dropped, t_=dst, s_=sim, z_=Z, B_=B, n_=n, kk=k, D_=D, o=dx):
        return lib._fn("d2s_gather_squeeze_bwd")(p(g_), p(k_), p(d_), p(t_), p(s_), p(z_), B_, n_, kk, D_, p(o), s)

    shapes = [dict(B_=0), dict(B_=-1), dict(kk=0), dict(kk=n), dict(n_=1, kk=1), dict(D_=72), dict(D_=0), dict(D_=1088), dict(n_=4097, kk=5)]
    bad = [fn(**kw) for fn in (match, fwd, bwd) for kw in shapes]
    bad += [match(x_=None), match(k_=None), match(d_=None), match(o1=None), match(o2=None),
            fwd(x_=None), fwd(k_=None), fwd(d_=None), fwd(t_=None), fwd(s_=None), fwd(o1=None), fwd(o2=None),
            bwd(g_=None), bwd(k_=None), bwd(d_=None), bwd(t_=None), bwd(s_=None), bwd(z_=None), bwd(o=None)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert bool((dst == 7).all()) and all(bool((t == 7).all()) for t in (sim, Z, y, dx))      # nothing was launched
    assert match(n_=577, kk=288, D_=192, B_=1) == 0                                  # n = 577 is inside the limit
    with pytest.raises(lib.D2SError, match="d2s_squeeze_match failed with code -1"):
        _ops().squeeze_match(f(B, n, 72), kept[:, :3].contiguous(), dropped[:, :5].contiguous())


# ---- 5. the model ----
def _student(case, squeeze=None, **kw):
    """squeeze None: the constructor is called without the argument at all"""
    import vit_models
    cfg = case["cfg"]
    student, teacher, sd_s, _ = build_models(case, torch.device(DEV))
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    if squeeze is not None:
        kw["squeeze_dropped"] = squeeze
    m = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
                                                topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                small_predictor=cfg["small_predictor"], init_n=cfg["init_n"], **common, **kw)
    m.load_state_dict(student.state_dict(), strict=True)
    return m.to(DEV), teacher, sd_s


@pytest.mark.parametrize("name,attn", [("micro1", False), ("micro2", False), ("micro1", True), ("micro2", True)])
def test_student_against_the_float64_forward_with_ids_and_plans_replayed(name, attn, monkeypatch):
    """Eval logits at tests/test_fuse_gpu.py's model tolerance (rtol 1e-4 / atol 2e-5); the sequence lengths of plain pruning; training
    mode = eval mode bit for bit on the same ids and plans; per-parameter gradient norms of logits.sum() at tests/test_tome_train_gpu.py's
    model rule (norms rtol 1e-3 / atol 1e-6, leading elements rtol 5e-3); and the gradient that reaches the dropped tokens' rows of a
    stage's input, which plain pruning leaves at zero"""
    import d2s.functional as DF
    ops = _ops()
    case = cases.MODEL_CASES[name]
    cfg = case["cfg"]
    images = _t(cases.make_images(case))
    m, _, sd = _student(case, True, attn_selection=attn)
    plain, _, _ = _student(case, False, attn_selection=attn)
    m.eval(), plain.eval()
    with torch.no_grad():
        logits, cls_attns, _, kept = m(images.to(DEV))
        _, cls_plain, _, kept_plain = plain(images.to(DEV))
    torch.cuda.synchronize()
    stages = len(cfg["pruning_loc"])
    plans = list(m.squeeze_plans)
    assert len(plans) == stages and all(d.dtype == torch.int32 and not d.requires_grad and not s.requires_grad for d, s in plans)
    assert [c.shape for c in cls_attns] == [c.shape for c in cls_plain] and torch.equal(kept[0], kept_plain[0])
    assert [tuple(d.shape) for d, _ in plans] == [tuple(x.shape) for x in m.dropped_token_indices]
    ids, cpu_plans = [k_.cpu() for k_ in kept], [(d.cpu(), s.cpu()) for d, s in plans]
    ref_logits, ref_grads = R.model_grads(sd, images, cfg, ids, cpu_plans)
    _, lengths, _ = R.student_forward({k_: _t(v).double() for k_, v in sd.items()}, images.double(), cfg, ids, cpu_plans)
    assert lengths == [1 + int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    print(f"{name} attn={attn}: max |logits - float64| {float((logits.cpu().double() - ref_logits).abs().max()):.3e}")
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.numpy(), rtol=1e-4, atol=2e-5)
    # training mode on the replayed ids and plans: the same bits, and the gradients
    seen = []
    orig = DF.GatherSqueezeFn.apply

    def spy(x, kept_, dropped_, plan):
        if x.requires_grad:
            x.register_hook(lambda g_, d=dropped_: seen.append((g_.detach().clone(), d)))
        return orig(x, kept_, dropped_, plan)
    monkeypatch.setattr(DF.GatherSqueezeFn, "apply", staticmethod(spy))
    m.train()
    m.kept_token_override, m.squeeze_plan_override = [k_.clone() for k_ in kept], plans
    out = m(images.to(DEV))[0]
    assert torch.equal(out.detach(), logits)
    out.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen) == stages
    for gx, dropped_ in seen:
        assert float(R.rows(gx.cpu(), dropped_.cpu()).abs().sum(-1).min()) > 0       # every dropped row of the stage input has a gradient
    checked = 0
    for k_, p_ in m.named_parameters():
        want = ref_grads[k_]
        if want is None or float(want.abs().max()) == 0:                             # the selector: no gradient through a hard selection
            assert p_.grad is None or float(p_.grad.abs().max()) == 0, k_
            continue
        gf, wf = p_.grad.detach().flatten().cpu(), want.flatten()
        np.testing.assert_allclose(float(gf.double().norm()), float(wf.norm()), rtol=1e-3, atol=1e-6, err_msg=k_)
        h = min(8, gf.numel())
        np.testing.assert_allclose(gf[:h].numpy(), wf[:h].numpy(), rtol=5e-3, atol=5e-4 * float(wf[:h].abs().max()) + 2e-6, err_msg=k_)
        checked += 1
    assert checked >= 12 * cfg["depth"]
    # plain pruning: the dropped rows of the stage input get exactly zero
    seen_plain = []
    orig_g = DF.GatherFn.apply

    def spy_g(x, kept_):
        if x.requires_grad:
            x.register_hook(lambda g_, kk=kept_: seen_plain.append((g_.detach().clone(), kk)))
        return orig_g(x, kept_)
    monkeypatch.setattr(DF.GatherFn, "apply", staticmethod(spy_g))
    plain.train()
    plain(images.to(DEV))[0].sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen_plain) == stages
    for gx, kk in seen_plain:
        dropped_ = R.complement(kk.cpu(), gx.shape[1] - 1)
        assert float(R.rows(gx.cpu(), dropped_).abs().max()) == 0


def test_flag_off_is_the_constructor_without_it_bit_for_bit(monkeypatch):
    import d2s.functional as DF
    case = cases.MODEL_CASES["micro2"]
    images = _t(cases.make_images(case)).to(DEV)

    class Never:
        @staticmethod
        def apply(*a):
            raise AssertionError("GatherSqueezeFn must not run with the flag off")
    monkeypatch.setattr(DF, "GatherSqueezeFn", Never)
    outs = []
    for squeeze in (False, None):
        m, _, _ = _student(case, squeeze)
        m.eval()
        with torch.no_grad():
            outs.append(m(images)[0])
        assert m.squeeze_dropped is False and m.squeeze_plans == []
    assert torch.equal(outs[0], outs[1])
    a, b = _steps(case, False, 2)[0], _steps(case, None, 2)[0]
    for u, v in zip(a, b):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])


# ---- 6. TrainStep ----
def _steps(case, squeeze, n):
    from d2s.engine import TrainStep
    student, teacher, _ = _student(case, squeeze)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=False)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(5)
    rec = []
    for _ in range(n):
        info = ts(x, y)
        torch.cuda.synchronize()
        rec.append((info["loss"].detach().clone(), ts.arena.params.clone()))
    return rec, ts


def test_train_steps_are_deterministic_and_resume_from_a_checkpoint():
    from d2s import lib
    case = cases.MODEL_CASES["micro2"]
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    a, ts = _steps(case, True, 3)
    b, _ = _steps(case, True, 3)
    off, _ = _steps(case, False, 3)
    for u, v in zip(a, b):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])                  # two runs of 3 steps: the same bits
    assert all(bool(torch.isfinite(u[0])) and bool(torch.isfinite(u[1]).all()) for u in a)
    assert not torch.equal(a[0][0], off[0][0]) and not torch.equal(a[2][1], off[2][1])          # the flag changes what is trained
    assert len(ts.student.squeeze_plans) == 2 and ts.config()["squeeze_dropped"] is True
    two, ts2 = _steps(case, True, 2)
    sd = ts2.state_dict(epoch=0)
    assert sd["config"]["squeeze_dropped"] is True
    _, resumed = _steps(case, True, 0)
    resumed.load_state_dict(sd)
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, a[2][1])                                # 2 steps, a checkpoint, 1 more = 3 straight steps
    _, ts_off = _steps(case, False, 0)
    with pytest.raises(lib.D2SError, match="squeeze_dropped"):
        ts_off.load_state_dict(sd)                                                   # a run and a checkpoint that disagree on the flag
    old = dict(sd, config={k_: v for k_, v in sd["config"].items() if k_ != "squeeze_dropped"})
    with pytest.raises(lib.D2SError, match="squeeze_dropped"):
        resumed.load_state_dict(old)                                                 # a checkpoint without the key counts as off
    ts_off.load_state_dict(dict(old, config=dict(old["config"])))


# ---- 7. command line ----
def test_cli_trains_and_evaluates_a_saved_checkpoint_with_the_flag(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path, out_dir = os.path.join(tmp_path, "deit_tiny.pt"), os.path.join(tmp_path, "run")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    base = ["--arch", "deit_tiny", "--pruning-locs", "3", "--keep-ratios", "0.5", "--warmup-steps", "0", "--batch-size", "4", "--steps-per-epoch", "2",
            "--val-steps", "1", "--topk-selection", "--squeeze-dropped"]
    acc = mask_predictor.main(base + ["--eval-only", "--student-checkpoint", path])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0 and "val loss:" in out and "Epoch 1/" not in out
    best = mask_predictor.main(base + ["--epochs", "1", "--student-checkpoint", path, "--teacher-checkpoint", path, "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert 0.0 <= best <= 1.0 and "Epoch 1/1" in out and "Training complete" in out
    sd = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)
    assert sd["config"]["squeeze_dropped"] is True
    with pytest.raises(SystemExit, match="not on the accelerated path: --squeeze-dropped without --topk-selection"):
        mask_predictor.main(["--arch", "deit_tiny", "--squeeze-dropped"])
