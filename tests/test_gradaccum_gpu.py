"""GPU tier of gradient accumulation and global-norm clipping inside the fused step: the three entry points on their own (exact
statements against numpy fp32 / the plain AdamW entry; the norm against float64 within the bound that follows from the kernel's stated
reduction depth, tests/gradaccum_ref.py), then the window through d2s.engine.TrainStep, the callers and two data-parallel ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases, gradaccum_ref as R
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu
CH = 1024
HP = dict(lr=5e-4, min_lr=1e-5, weight_decay=0.05, epochs=25)


def _dev():
    return torch.device("cuda:0")


def _desc(active, lr=1e-3, wd=0.05):
    return torch.from_numpy(R.chunk_desc(lr, wd, np.asarray(active, dtype=np.int32))).to(_dev())


def _mask(active):
    return np.repeat(np.asarray(active, dtype=bool), CH)


# ---------------------------------------------------------------- kernels ----------------------------------------------------------------
def test_grad_accumulate_modes_are_numpy_fp32_addition():
    from d2s import ops
    rng = np.random.default_rng(5)
    active = [1, 0, 1, 1, 0, 1, 1]
    n, m = len(active), _mask(active)
    a = (rng.standard_normal(n * CH) * 10.0 ** rng.uniform(-6, 2, n * CH)).astype(np.float32)
    g = (rng.standard_normal(n * CH) * 10.0 ** rng.uniform(-6, 2, n * CH)).astype(np.float32)
    desc = _desc(active)
    for mode in (0, 1, 2):
        acc, grd = torch.from_numpy(a.copy()).to(_dev()), torch.from_numpy(g.copy()).to(_dev())
        ops.grad_accumulate(acc, grd, desc, n, mode)
        torch.cuda.synchronize()
        want_acc, want_g = a.copy(), g.copy()
        if mode == 0:
            want_acc[m] = g[m]
        elif mode == 1:
            want_acc[m] = (a[m] + g[m]).astype(np.float32)
        else:
            want_g[m] = (a[m] + g[m]).astype(np.float32)
        np.testing.assert_array_equal(acc.cpu().numpy().view(np.uint32), want_acc.view(np.uint32), err_msg=f"acc, mode {mode}")
        np.testing.assert_array_equal(grd.cpu().numpy().view(np.uint32), want_g.view(np.uint32), err_msg=f"g, mode {mode}")
    with pytest.raises(Exception):
        ops.grad_accumulate(acc, grd, desc, n, 3)


def test_grad_accumulate_refuses_arenas_that_overlap():
    """Both arenas are __restrict__ in the kernel: the entry point refuses the same arena and a partial overlap in either order, launches
    nothing, and accepts two arenas that touch."""
    from d2s import lib
    buf = torch.ones(3 * CH, dtype=torch.float32, device=_dev())
    desc = _desc([1, 1])
    for acc, g in ((buf, buf), (buf[:2 * CH], buf[CH:]), (buf[CH:], buf[:2 * CH])):
        for mode in (0, 1, 2):
            with pytest.raises(lib.D2SError):
                lib.call("d2s_grad_accumulate", lib.ptr(acc), lib.ptr(g), lib.ptr(desc), 2, mode)
    torch.cuda.synchronize()
    assert bool((buf == 1).all())
    lib.call("d2s_grad_accumulate", lib.ptr(buf[:CH]), lib.ptr(buf[CH:]), lib.ptr(desc), 1, 1)
    torch.cuda.synchronize()
    assert bool((buf[:CH] == 2).all()) and bool((buf[CH:] == 1).all())


@pytest.mark.parametrize("coef", [1.0, 0.37109375, 0.123456789])
@pytest.mark.parametrize("ema", [False, True])
def test_adamw_step_clip_equals_plain_entry_with_host_scale(coef, ema):
    from d2s import ops
    rng = np.random.default_rng(9)
    active = [1, 1, 0, 1, 0, 1]
    n = len(active)
    desc = _desc(active, lr=np.float32([1e-3, 5e-4, 0, 1e-3, 0, 5e-6]), wd=np.float32([0.05, 0, 0, 0.05, 0, 0.05]))
    s = np.float32(1.0 / 3.0)
    host_scale = float(np.float32(s * np.float32(coef)))
    init = {k: (rng.standard_normal(n * CH) * sc).astype(np.float32) for k, sc in (("p", 0.5), ("g", 2.0), ("m", 0.1), ("e", 0.5))}
    init["v"] = (rng.random(n * CH) * 1e-2).astype(np.float32)
    steps0 = np.int32([3, 0, 0, 7, 0, 1])
    out = []
    for clip in (False, True):
        t = {k: torch.from_numpy(v.copy()).to(_dev()) for k, v in init.items()}
        cs = torch.from_numpy(steps0.copy()).to(_dev())
        for it in range(2):
            if clip:
                cd = torch.tensor([123.0, coef], dtype=torch.float32, device=_dev())      # {norm, coef}: the launch reads the second float
                ops.adamw_step_clip(t["p"], t["g"], t["m"], t["v"], desc, n, 0.9, 0.999, 1e-8, it + 1, cd[1:], ema=t["e"] if ema else None,
                                    ema_decay=0.99, grad_scale=float(s), chunk_steps=cs)
            elif ema:
                ops.adamw_step_ema(t["p"], t["g"], t["m"], t["v"], desc, n, 0.9, 0.999, 1e-8, it + 1, t["e"], 0.99, grad_scale=host_scale, chunk_steps=cs)
            else:
                ops.adamw_step(t["p"], t["g"], t["m"], t["v"], desc, n, 0.9, 0.999, 1e-8, it + 1, grad_scale=host_scale, chunk_steps=cs)
        torch.cuda.synchronize()
        out.append({**{k: v.cpu().numpy() for k, v in t.items()}, "steps": cs.cpu().numpy()})
    for k in ("p", "m", "v", "e", "g"):
        np.testing.assert_array_equal(out[0][k].view(np.uint32), out[1][k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(out[0]["steps"], out[1]["steps"])
    np.testing.assert_array_equal(out[1]["steps"], steps0 + 2 * np.int32(active))
    frozen = ~_mask(active)
    np.testing.assert_array_equal(out[1]["p"][frozen], init["p"][frozen])
    if not ema:
        np.testing.assert_array_equal(out[1]["e"], init["e"])            # never touched without EMA
    assert not np.array_equal(out[1]["p"][~frozen], init["p"][~frozen])


@pytest.mark.parametrize("n_chunks,seed", [(7, 1), (300, 2), (2049, 3)])
def test_clip_norm_and_coefficient_against_float64(n_chunks, seed):
    from d2s import ops
    rng = np.random.default_rng(seed)
    active = (rng.random(n_chunks) < 0.7).astype(np.int32)
    active[0] = 1
    m = _mask(active)
    g = (rng.standard_normal(n_chunks * CH) * 10.0 ** rng.uniform(-6, 2, n_chunks * CH)).astype(np.float32)
    g[~m] = np.nan                                   # a chunk that is not active is not read
    desc = _desc(active)
    gd = torch.from_numpy(g).to(_dev())
    partials = torch.empty(n_chunks, dtype=torch.float32, device=_dev())
    s = R.window_scale(3, 2)
    want = R.norm64(g, s, m)
    worst = 0.0
    for max_norm in (want * 4.0, want * 0.25, want * 1e-4):
        out = torch.zeros(2, dtype=torch.float32, device=_dev())
        out2 = torch.zeros(2, dtype=torch.float32, device=_dev())
        ops.grad_clip_coef(gd, desc, n_chunks, float(s), max_norm, partials, out)
        p1 = partials.clone()
        ops.grad_clip_coef(gd, desc, n_chunks, float(s), max_norm, partials, out2)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(p1, partials), "two launches must be bit-identical"
        norm, coef = (float(v) for v in out.cpu().numpy().astype(np.float64))
        assert np.isfinite(norm)
        rel = abs(norm - want) / want
        worst = max(worst, rel)
        assert rel <= R.NORM_REL_BOUND, (rel, R.NORM_REL_BOUND)
        if max_norm > want:
            assert coef == 1.0
        else:
            want_c = float(np.float32(max_norm)) / (want + 1e-6)
            rel_c = abs(coef - want_c) / want_c
            assert rel_c <= R.COEF_REL_BOUND, (rel_c, R.COEF_REL_BOUND)
            assert coef == float(R.clip_coef(np.float32(norm), max_norm)), "coef is the fp32 expression of the stored norm"
        # per-chunk partials: sum of squares within (L + 1) 2^-24; 0 for chunks that are not active
        pc = partials.cpu().numpy().astype(np.float64)
        exact = (g.astype(np.float64) ** 2).reshape(n_chunks, CH)
        exact[active == 0] = 0.0
        exact = exact.sum(1)
        assert (pc[active == 0] == 0).all()
        relp = np.abs(pc - exact)[active == 1] / exact[active == 1]
        assert relp.max() <= R.SUMSQ_REL_BOUND, relp.max()
    print(f"[clip norm] {n_chunks} chunks: worst relative error of the norm {worst:.3e} = {worst / R.NORM_REL_BOUND:.3f} of the bound "
          f"{R.NORM_REL_BOUND:.3e}; per-chunk sums {relp.max():.3e} = {relp.max() / R.SUMSQ_REL_BOUND:.3f} of {R.SUMSQ_REL_BOUND:.3e}")


# ---------------------------------------------------------------- step level -------------------------------------------------------------
def _step(name, **kw):
    from d2s.engine import TrainStep
    case = cases.MODEL_CASES[name]
    s, t, _, _ = build_models(case, _dev())
    kw.setdefault("warmup_steps", 0)
    return TrainStep(s, t, make_args(case["cfg"]), graph=False, **HP, **kw)


def _batches(name, n):
    from d2s import synth
    case = cases.MODEL_CASES[name]
    cfg = case["cfg"]
    return [(_t(synth.images(case["batch"], 3, cfg["img_size"], seed=900 + i)).to(_dev()),
             _t(synth.labels(case["batch"], cfg["num_classes"], seed=900 + i)).to(_dev())) for i in range(n)]


def _state(ts):
    torch.cuda.synchronize()
    return {"params": ts.arena.params.clone(), "exp_avg": ts.opt.exp_avg.clone(), "exp_avg_sq": ts.opt.exp_avg_sq.clone(),
            "chunk_steps": ts.opt.chunk_steps.clone(), "steps": ts.opt.steps}


def _assert_same_state(a, b, what):
    for k in ("params", "exp_avg", "exp_avg_sq", "chunk_steps"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs ({int((a[k] != b[k]).sum())} elements)"
    assert a["steps"] == b["steps"], what


def _active_mask(ts):
    d = ts.opt.desc().cpu().numpy().view(np.dtype([("lr", "<f4"), ("wd", "<f4"), ("active", "<i4"), ("pad", "<i4")]))
    return np.repeat(d["active"] != 0, CH)


@pytest.mark.parametrize("name", ["micro1", "micro2"])
def test_defaults_and_unbinding_clip_are_the_plain_step(name):
    data = _batches(name, 3)
    plain, same, loose = _step(name), _step(name, accum_steps=1, clip_grad=None), _step(name, clip_grad=1e30)
    for x, y in data:
        a, b, c = plain(x, y), same(x, y), loose(x, y)
        assert b["stepped"] is True and c["stepped"] is True and a["stepped"] is True
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["loss"], c["loss"])
        _assert_same_state(_state(plain), _state(same), "accum_steps=1, clip_grad=None")
        _assert_same_state(_state(plain), _state(loose), "clip_grad=1e30")
        assert float(loose.last_clip[1]) == 1.0 and float(c["grad_norm"]) == float(loose.last_clip[0]) > 0
    assert same._acc is None and same.last_clip is None and plain._acc is None, "nothing is allocated when the feature is off"
    assert loose._acc is None


@pytest.mark.parametrize("name", ["micro1", "micro2"])
def test_same_batch_twice_is_one_step_on_that_batch(name):
    (x, y), = _batches(name, 1)
    plain, twice = _step(name), _step(name, accum_steps=2)
    plain(x, y)
    i1 = twice(x, y)
    assert i1["stepped"] is False
    _assert_same_state(_state(twice), {**_state(_step(name)), "steps": 0}, "a non-final micro-step must not update")
    i2 = twice(x, y)
    assert i2["stepped"] is True and twice._pending == 0
    _assert_same_state(_state(plain), _state(twice), "(g + g) * 0.5")
    # binding clip: sum (2g)^2 = 4 sum g^2 and its square root, halved, are exact
    probe = _step(name, clip_grad=1e30)
    probe(x, y)
    M = 0.25 * float(probe.last_clip[0])
    one, two = _step(name, clip_grad=M), _step(name, accum_steps=2, clip_grad=M)
    one(x, y)
    two(x, y)
    two(x, y)
    assert float(one.last_clip[1]) < 1.0, "the clip must bind"
    assert torch.equal(one.last_clip, two.last_clip)
    _assert_same_state(_state(one), _state(two), "clipped (g + g) * 0.5")
    assert not torch.equal(one.arena.params, plain.arena.params)


def test_window_of_three_batches_with_binding_clip():
    from d2s import ops
    name = "micro2"
    data = _batches(name, 3)
    probe = _step(name, clip_grad=1e30)
    probe(*data[0])
    M = 0.3 * float(probe.last_clip[0])
    ts, twin = _step(name, accum_steps=3, clip_grad=M), _step(name, accum_steps=4)
    gs = []
    for x, y in data:
        info = twin(x, y)
        assert info["stepped"] is False
        torch.cuda.synchronize()
        gs.append(twin.arena.grads.cpu().numpy().copy())
    for i, (x, y) in enumerate(data):
        if i == 2:
            pre = _state(ts)
        info = ts(x, y)
        torch.cuda.synchronize()
        assert info["stepped"] is (i == 2)
        if i < 2:        # the contract: a non-final micro-step leaves its own gradient in the gradient arena
            np.testing.assert_array_equal(ts.arena.grads.cpu().numpy().view(np.uint32), gs[i].view(np.uint32))
            assert "grad_norm" not in info
    m = _active_mask(ts)
    assert m.any() and not m.all()
    S = R.window_sum(gs)
    got = ts.arena.grads.cpu().numpy()
    np.testing.assert_array_equal(got[m].view(np.uint32), S[m].view(np.uint32), err_msg="combined gradient, arrival order")
    np.testing.assert_array_equal(got[~m].view(np.uint32), gs[2][~m].view(np.uint32), err_msg="chunks outside the optimiser are untouched")
    s = R.window_scale(3)
    norm, coef = (float(v) for v in ts.last_clip.cpu().numpy().astype(np.float64))
    want = R.norm64(S, s, m)
    rel = abs(norm - want) / want
    print(f"[window of 3] pre-clip norm {norm:.6e} (float64 {want:.6e}, relative error {rel:.2e} = {rel / R.NORM_REL_BOUND:.3f} of the bound), coef {coef:.6f}")
    assert rel <= R.NORM_REL_BOUND
    assert coef < 1.0 and abs(coef - M / (want + 1e-6)) / coef <= R.COEF_REL_BOUND + 2.0 ** -24      # M itself is rounded to fp32
    assert float(info["grad_norm"]) == norm
    # the update: the plain entry on the pre-step state with the host scale fl(s * coef read back)
    host_scale = float(np.float32(s * np.float32(coef)))
    ops.adamw_step(pre["params"], ts.arena.grads, pre["exp_avg"], pre["exp_avg_sq"], ts.opt.desc(), ts.arena.n_chunks, ts.opt.betas[0],
                   ts.opt.betas[1], ts.opt.eps, pre["steps"] + 1, grad_scale=host_scale, chunk_steps=pre["chunk_steps"])
    pre["steps"] += 1
    _assert_same_state(pre, _state(ts), "AdamW on S with fl(s * coef)")
    assert ts.opt.steps == 1 and int(ts.opt.chunk_steps.max()) == 1
    assert ts.grad_norm_mean() == pytest.approx(norm, rel=1e-6) and ts.grad_norm_mean() is None
    for x, y in data:                                   # a second window: an info kept from the first one keeps its own norm
        later = ts(x, y)
    assert float(later["grad_norm"]) == float(ts.last_clip[0]) != norm and float(info["grad_norm"]) == norm


def test_flush_closes_a_short_window_and_the_norm_follows_the_live_set():
    from d2s import lib
    name = "micro2"
    data = _batches(name, 3)
    ts = _step(name, accum_steps=3, clip_grad=1e-3, warmup_steps=1)
    assert ts.flush() is False
    a = ts.arena
    pred = np.zeros(a.total, dtype=bool)
    for i, (n, g) in enumerate(zip(a.names, ts.opt.groups)):
        c0, c1 = a.chunk_range(i)
        if g == "predictor":
            pred[c0 * CH:c1 * CH] = True
        else:
            a.grads[c0 * CH:c1 * CH] = 1e3            # frozen in epoch 0: backward does not write here, and the window must not read it
    poisoned = a.grads.clone()
    before = _state(ts)
    for x, y in data[:2]:
        assert ts(x, y)["stepped"] is False
    for fn in (lambda: ts.set_epoch(1), lambda: ts.state_dict(), lambda: ts.load_state_dict({})):
        with pytest.raises(lib.D2SError, match="flush"):
            fn()
    _assert_same_state(before, _state(ts), "nothing is applied before the flush")
    assert ts.flush() is True and ts._pending == 0 and ts.opt.steps == 1
    torch.cuda.synchronize()
    assert np.array_equal(_active_mask(ts), pred), "epoch 0 of a warm-up run: the optimiser's chunks are the predictor's"
    S = a.grads.cpu().numpy()
    np.testing.assert_array_equal(S[~pred], poisoned.cpu().numpy()[~pred])
    norm = float(ts.last_clip[0])
    want = R.norm64(S, R.window_scale(2), pred)
    assert abs(norm - want) / want <= R.NORM_REL_BOUND, (norm, want)
    after = _state(ts)
    assert not torch.equal(after["params"], before["params"])
    assert torch.equal(after["params"][torch.from_numpy(~pred).to(_dev())], before["params"][torch.from_numpy(~pred).to(_dev())])
    assert ts.flush() is False
    _assert_same_state(after, _state(ts), "a second flush does nothing")
    ts.state_dict()
    ts.set_epoch(1)                                   # everything trains: the norm covers every chunk the optimiser now updates
    a.grads.zero_()
    for i, (x, y) in enumerate(data):
        info = ts(x, y)
        assert info["stepped"] is (i == 2)
    torch.cuda.synchronize()
    m = _active_mask(ts)
    assert m.sum() > pred.sum()
    S = a.grads.cpu().numpy()
    want = R.norm64(S, R.window_scale(3), m)
    assert abs(float(ts.last_clip[0]) - want) / want <= R.NORM_REL_BOUND
    assert want > R.norm64(S, R.window_scale(3), pred)
    steps = ts.opt.chunk_steps.cpu().numpy()
    assert set(np.unique(steps[pred[::CH]])) == {2} and set(np.unique(steps[m[::CH] & ~pred[::CH]])) == {1}


def test_graph_mode_is_refused_with_accumulation_and_with_clipping():
    from d2s import lib
    from d2s.engine import TrainStep
    case = cases.MODEL_CASES["micro1"]
    for kw in (dict(accum_steps=2), dict(clip_grad=1.0)):
        s, t, _, _ = build_models(case, _dev())
        with pytest.raises(lib.D2SError, match="graph=True"):
            TrainStep(s, t, make_args(case["cfg"]), graph=True, **kw)
    for kw in (dict(accum_steps=0), dict(accum_steps=1.5), dict(clip_grad=0.0), dict(clip_grad=-1.0)):
        s, t, _, _ = build_models(case, _dev())
        with pytest.raises(lib.D2SError):
            TrainStep(s, t, make_args(case["cfg"]), **kw)


def test_torch_recipe_and_fused_step_agree_with_accumulation_and_clipping():
    """train_one_epoch over 4 batches = two optimiser steps of a window of 2, clipped: the fused arena step against the same window spelled
    out with torch (backward into .grad, grad.mul_(s), clip_grad_norm_, torch.optim.AdamW).  Tolerances: those of
    tests/test_callers_gpu.py for the two recipes without the feature (train_loss rtol 1e-4; every parameter within 2 lr per optimiser step);
    the mean gradient norm is a scalar of the same two computations and is held to the loss's rtol 1e-4, no tolerance of its own."""
    from d2s.engine import TrainStep
    from train import train_one_epoch
    import utils
    dev = _dev()
    case = cases.MODEL_CASES["micro1"]
    cfg = case["cfg"]
    clip = 1e-3

    def args():
        a = make_args(cfg)
        a.device, a.warmup_steps, a.weight_decay, a.lr, a.min_lr, a.epochs, a.is_sbatch = dev, 0, 0.05, 5e-4, 1e-5, 25, False
        a.accum_steps, a.clip_grad = 2, clip
        return a
    loader = lambda: utils.SyntheticLoader(4, 4, img_size=cfg["img_size"], num_classes=cfg["num_classes"], seed=5, device=dev)
    s1, t1, _, _ = build_models(case, dev)
    a1 = args()
    step = TrainStep(s1, t1, a1, lr=a1.lr, min_lr=a1.min_lr, weight_decay=a1.weight_decay, epochs=a1.epochs, warmup_steps=0,
                     accum_steps=2, clip_grad=clip)
    m1 = train_one_epoch(a1, s1, t1, loader(), step)
    assert step.opt.steps == 2 and step._pending == 0
    s2, t2, _, _ = build_models(case, dev)
    a2 = args()
    groups = utils.get_param_groups(s2, a2)
    opt = torch.optim.AdamW([g for g in groups if g["params"]], lr=a2.lr, weight_decay=a2.weight_decay)
    utils.adjust_learning_rate(opt.param_groups, a2, 0, s2)
    for p in t2.parameters():
        p.requires_grad_(False)
    m2 = train_one_epoch(a2, s2, t2, loader(), opt)
    assert set(m1) == set(m2) and "train_grad_norm" in m1
    assert m1["train_grad_norm"] > clip, "the clip must bind"
    print(f"[recipes] train_grad_norm fused {m1['train_grad_norm']:.6e}, torch {m2['train_grad_norm']:.6e}")
    np.testing.assert_allclose(m1["train_loss"], m2["train_loss"], rtol=1e-4)
    np.testing.assert_allclose(m1["train_grad_norm"], m2["train_grad_norm"], rtol=1e-4)
    for (n, p), (_, q) in zip(s1.named_parameters(), s2.named_parameters()):
        d = (p.detach() - q.detach()).abs().max().item()
        assert d <= 2 * 2 * a1.lr * 1.01, (n, d)


@pytest.mark.parametrize("collective,port", [("allreduce", 29561), ("rs_ag", 29563)])
def test_two_ranks_accumulating_and_clipping_match_a_single_process(collective, port):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(cases.REPO, "tools", "ddp_check.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", D2S_DDP_COLLECTIVE=collective, D2S_DDP_ACCUM="2", D2S_DDP_CLIP="0.001")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "[ddp_check] accum 2 clip 0.001" in out.stdout
    print(out.stdout[-1500:])
