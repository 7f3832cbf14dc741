"""GPU tier: the fused AdamW launches (csrc/loss.hip: d2s_adamw_step, d2s_adamw_step_ema, d2s_adamw_step_clip) against AdamW itself -
tests/losspath_ref.py adamw_step / ema_step in float64 on the same fp32 state and the same fp32 hyper-parameters (the C ABI takes floats:
beta1 = fl32(0.9) IS the beta of the launch, and the reference uses that number, not 0.9).  tests/test_gradaccum_gpu.py shows that the
three entries agree with each other bit for bit; this file shows what they compute.

p may be 4 times as far from float64 as the fp32 restatement by max |p - p64| / (|p_old| + |p64 - p_old|), m, v and the EMA by the
relative 2-norm, or 3e-7.  Chunks that are not active keep p, m, v and their counter bit for bit, and their EMA still advances."""
import numpy as np
import pytest
import torch

from tests import gradaccum_ref as G, losspath_ref as R

pytestmark = pytest.mark.gpu

CH = 1024
ACTIVE = np.int32([1, 1, 0, 1, 0, 1])
N = len(ACTIVE)
LR = np.float32([1e-3, 0.0, 1e-3, 5e-4, 0.0, 5e-6])           # an active chunk with lr = 0: its moments move, its parameters do not
WD = np.float32([0.05, 0.05, 0.05, 0.0, 0.0, 0.05])
B1, B2, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
STEPS0 = np.int32([0, 3, 0, 7, 0, 1])
COEF = 0.37109375
ENTRIES = ("plain", "ema99", "ema0", "clip", "clip_ema")
DECAY = {"plain": None, "ema99": float(np.float32(0.99)), "ema0": 0.0, "clip": None, "clip_ema": float(np.float32(0.99))}


def _dev():
    return torch.device("cuda:0")


def _el(per_chunk):
    return torch.from_numpy(np.repeat(np.asarray(per_chunk), CH))


def _state(seed, warm):
    rng = np.random.default_rng(seed)
    st = {"p": (rng.standard_normal(N * CH) * 0.5).astype(np.float32), "e": (rng.standard_normal(N * CH) * 0.5).astype(np.float32)}
    st["p"][st["p"] == 0] = 0.25
    if warm:
        st["m"] = (rng.standard_normal(N * CH) * 0.1).astype(np.float32)
        st["v"] = (rng.random(N * CH) * 1e-2).astype(np.float32)
    else:
        st["m"], st["v"] = np.zeros(N * CH, np.float32), np.zeros(N * CH, np.float32)
    return {k: torch.from_numpy(v) for k, v in st.items()}


def _grad(seed):
    rng = np.random.default_rng(1000 + seed)
    g = (rng.standard_normal(N * CH) * 10.0 ** rng.uniform(-6, 2, N * CH)).astype(np.float32)
    g[::17] = 0.0
    return torch.from_numpy(g)


def _launch(ops, entry, d, g, desc, step, scale, cs):
    """one call of the entry under test on device state d = {p, m, v, e}; all arenas are N * CH floats"""
    assert all(d[k].numel() == N * CH for k in "pmve") and g.numel() == N * CH and desc.numel() == N * 16
    if entry == "plain":
        ops.adamw_step(d["p"], g, d["m"], d["v"], desc, N, B1, B2, EPS, step, grad_scale=scale, chunk_steps=cs)
    elif entry in ("ema99", "ema0"):
        ops.adamw_step_ema(d["p"], g, d["m"], d["v"], desc, N, B1, B2, EPS, step, d["e"], DECAY[entry], grad_scale=scale, chunk_steps=cs)
    else:
        cd = torch.tensor([123.0, COEF], dtype=torch.float32, device=_dev())          # {norm, coef}: the launch reads the second float
        ops.adamw_step_clip(d["p"], g, d["m"], d["v"], desc, N, B1, B2, EPS, step, cd[1:], ema=d["e"] if entry == "clip_ema" else None,
                            ema_decay=DECAY[entry] or 0.0, grad_scale=scale, chunk_steps=cs)


def _reference(st, g, t_chunk, eff_scale, decay, dtype):
    """the state after one step in `dtype`: AdamW on the active chunks, nothing on the others, the EMA on all of them"""
    act = _el(ACTIVE).bool()
    c = lambda x: x.to(dtype)
    p, m, v = R.adamw_step(c(st["p"]), c(g), c(st["m"]), c(st["v"]), _el(LR), _el(WD), B1, B2, EPS, _el(np.maximum(t_chunk, 1)), eff_scale)
    out = {"p": torch.where(act, p, c(st["p"])), "m": torch.where(act, m, c(st["m"])), "v": torch.where(act, v, c(st["v"]))}
    out["e"] = c(st["e"]) if decay is None else R.ema_step(c(st["e"]), out["p"], decay)
    return out


def _p_err(p, p64, p_old):
    den = p_old.double().abs() + (p64 - p_old.double()).abs()
    assert bool((den > 0).all())
    return float(((p.double() - p64).abs() / den).max())


def _check(what, got, ref64, ref32, p_old, decay):
    e_hip, e_cpu = _p_err(got["p"], ref64["p"], p_old), _p_err(ref32["p"], ref64["p"], p_old)
    print(f"[parity] {what} p: err_hip {e_hip:.3e}  err_cpu32 {e_cpu:.3e}  ratio {e_hip / e_cpu if e_cpu else 0.0:.2f}")
    assert e_hip <= max(R.ERR_FACTOR * e_cpu, R.ERR_FLOOR), (what, e_hip, e_cpu)
    for k in ("m", "v") + (("e",) if decay is not None else ()):
        R.assert_close_as_fp32(f"{what} {k}", got[k], ref64[k], ref32[k])


@pytest.mark.parametrize("steps", ["global1", "global2", "global1000", "chunk_steps"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_one_step_is_adamw(entry, steps):
    """One launch from a fresh (m = v = 0) and from a warm state, grad_scale 1 and 1/3, per-chunk lr / wd with zeros, gradients with exact
    zeros and magnitudes from 1e-6 to 1e2.  Measured on the MI355X, largest over all cases (hip / cpu fp32): p 1.7e-7 / 2.8e-7,
    m 5.0e-8 / 5.3e-8, v 7.2e-8 / 7.2e-8, EMA 6.3e-8 / 7.7e-8; err_hip / err_cpu32 between 0.86 and 1.10, all below the 3e-7 floor."""
    from d2s import ops
    dev = _dev()
    desc = torch.from_numpy(G.chunk_desc(LR, WD, ACTIVE)).to(dev)
    inactive = ~_el(ACTIVE).bool()
    for warm in (False, True):
        for scale in (1.0, float(np.float32(1.0 / 3.0))):
            st, g = _state(7 + warm, warm), _grad(3 + warm)
            d = {k: v.clone().to(dev) for k, v in st.items()}
            cs = torch.from_numpy(STEPS0.copy()).to(dev) if steps == "chunk_steps" else None
            step = 1 if cs is not None else int(steps[6:])
            t_chunk = STEPS0 + 1 if cs is not None else np.full(N, step)
            eff = float(np.float32(np.float32(scale) * np.float32(COEF))) if entry.startswith("clip") else scale
            _launch(ops, entry, d, g.to(dev), desc, step, scale, cs)
            torch.cuda.synchronize()
            got = {k: v.cpu() for k, v in d.items()}
            decay = DECAY[entry]
            ref64, ref32 = (_reference(st, g, t_chunk, eff, decay, dt) for dt in (torch.float64, torch.float32))
            _check(f"adamw {entry} {steps} warm {int(warm)} scale {scale:.3f}", got, ref64, ref32, st["p"], decay)
            for k in "pmv":                                                       # chunks that are not active: bit-unchanged
                assert torch.equal(got[k][inactive].view(torch.int32), st[k][inactive].view(torch.int32)), k
            if decay is None:
                assert torch.equal(got["e"].view(torch.int32), st["e"].view(torch.int32))          # no EMA entry: the arena is not touched
            else:
                assert not torch.equal(got["e"][inactive], st["e"][inactive])     # the average of a frozen chunk still moves
            if decay == 0.0:
                assert torch.equal(got["e"].view(torch.int32), got["p"].view(torch.int32))         # decay 0: the average is the new weights
            lr0 = _el(LR == 0) & ~inactive
            assert torch.equal(got["p"][lr0], st["p"][lr0]) and not torch.equal(got["m"][lr0], st["m"][lr0])
            if cs is not None:
                assert cs.cpu().numpy().tolist() == (STEPS0 + ACTIVE).tolist()    # +1 where active, unchanged elsewhere


@pytest.mark.parametrize("entry", ENTRIES)
def test_three_chained_steps(entry):
    """Three launches with fresh gradients and per-chunk counters against three reference steps in float64 from the same start.
    Measured err_hip / err_cpu32 on the MI355X: p 0.61-0.63 (1.7e-7 against 2.8e-7), m 0.91-0.94, v 0.98-1.00, EMA 0.66-0.82."""
    from d2s import ops
    dev = _dev()
    desc = torch.from_numpy(G.chunk_desc(LR, WD, ACTIVE)).to(dev)
    st = _state(21, True)
    d = {k: v.clone().to(dev) for k, v in st.items()}
    cs = torch.from_numpy(STEPS0.copy()).to(dev)
    scale = float(np.float32(1.0 / 3.0))
    eff = float(np.float32(np.float32(scale) * np.float32(COEF))) if entry.startswith("clip") else scale
    ref64 = {k: v.double() for k, v in st.items()}
    ref32 = {k: v.clone() for k, v in st.items()}
    for it in range(3):
        g = _grad(50 + it)
        _launch(ops, entry, d, g.to(dev), desc, it + 1, scale, cs)
        ref64 = _reference(ref64, g, STEPS0 + (it + 1) * ACTIVE, eff, DECAY[entry], torch.float64)
        ref32 = _reference(ref32, g, STEPS0 + (it + 1) * ACTIVE, eff, DECAY[entry], torch.float32)
        assert cs.cpu().numpy().tolist() == (STEPS0 + (it + 1) * ACTIVE).tolist()
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in d.items()}
    _check(f"adamw {entry} 3 steps", got, ref64, ref32, st["p"], DECAY[entry])
    inactive = ~_el(ACTIVE).bool()
    for k in "pmv":
        assert torch.equal(got[k][inactive].view(torch.int32), st[k][inactive].view(torch.int32)), k


def test_ema_entries_reject_aliasing_and_decay_one():
    """The average must not be the parameter arena and the decay must be in [0, 1): refused before any launch, state untouched"""
    from d2s import lib
    dev = _dev()
    desc = torch.from_numpy(G.chunk_desc(LR, WD, ACTIVE)).to(dev)
    st = _state(31, True)
    d = {k: v.clone().to(dev) for k, v in st.items()}
    g = _grad(31).to(dev)
    coef = torch.ones(1, dtype=torch.float32, device=dev)
    base = (lib.ptr(d["p"]), lib.ptr(g), lib.ptr(d["m"]), lib.ptr(d["v"]), lib.ptr(desc), N, B1, B2, EPS, 1, 1.0, None)
    for ema, decay in ((d["p"], 0.99), (d["e"], 1.0), (d["e"], -0.5), (None, 0.99)):
        with pytest.raises(lib.D2SError):
            lib.call("d2s_adamw_step_ema", *base, lib.ptr(ema), decay)
    for ema, decay in ((d["p"], 0.99), (d["e"], 1.0)):
        with pytest.raises(lib.D2SError):
            lib.call("d2s_adamw_step_clip", *base, lib.ptr(ema), decay, lib.ptr(coef))
    with pytest.raises(lib.D2SError):
        lib.call("d2s_adamw_step", *base[:9], 0, 1.0, None)                       # global step 0 without per-chunk counters
    torch.cuda.synchronize()
    for k in "pmve":
        assert torch.equal(d[k].cpu(), st[k]), k
