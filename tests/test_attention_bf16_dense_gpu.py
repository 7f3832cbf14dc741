"""The dense bf16 attention kernels (csrc/attention_bf16.hip: d2s_attn_fwd_bf16, d2s_attn_fwd_bf16_bf16out, d2s_attn_bwd_bf16,
d2s_attn_bwd_bf16_bf16out) against float64, at the edges of 32-key tiles, 64-key tiles and 128-query workgroups and in both tile forms of
the forward.  The policy, ragged and key-weighted variants are anchored bit for bit to these kernels; this module is what anchors them.

Inputs, reference, bounds and the rounding emulation are tests/attention_bf16_ref.py (derivation in its docstring; checked on their own
by tests/test_attention_bf16_ref_cpu.py).  Five sections:
  1. per-element bounds: forward and backward as in training (the kernel's own out and lse feed its backward), |got - ref| / bound <= 1
     for out, lse, cls_row, dq, dk, dv, through ops.attn_fwd / ops.attn_bwd in the bf16 arithmetic mode and through the _bf16out entries.
  2. yardstick: the absolute-value sums make the dQ / dK bounds ~20x the true error, so one dropped key at n = 577 hides under them.
     Per (b, h) slice of out, dq, dk, dv the relative L2 error against float64 is at most 2x the emulation's on that slice plus the
     fp32 floor 2 (n + 64 + 2) 2^-24 (stated on the absolute errors, |got - ref| <= 2 |emu - ref| + floor |ref|, the same inequality
     times |ref|: dq and dk are exactly zero at n = 1).  The 2: the emulation rounds e against the final maximum, the kernel against the
     running one - the same distribution, other binade positions - and the fp32 chains are not emulated.
  3. the forms of the entries agree bit for bit at every shape, the in-kernel fp32 -> bf16 conversion rounds ties as torch does.
  4. the whole module again in a child process per forced tile form (D2S_ATTN_BF16_T64 = 0, then 2; it is read once per process).
  5. argument checks of the four entries.

Measured on an MI355X, largest value over the 54 cases (section 1: max err / bound; section 2: (|got - ref| - floor |ref|) / |emu - ref|):
    tile form (D2S_ATTN_BF16_T64)   err / bound:  out    lse    cls_row  dq     dk     dv       L2 ratio:  out    dq     dk     dv
    by length (unset)                             0.391  0.008  0.008    0.056  0.060  0.705               0.994  1.027  1.081  0.997
    32-key tiles (0)                              0.391  0.008  0.008    0.056  0.060  0.705               0.994  1.026  1.038  0.997
    64-key tiles (2)                              0.391  0.008  0.008    0.056  0.060  0.705               0.994  1.027  1.081  0.997
  (out at n = 17 normal, dv at n = 2 sink, dq / dk at n = 127 and n = 31 last; the emulation alone: out 0.391, dq 0.051, dk 0.060, dv 0.705.)
  The kernels sit on the emulation - L2 ratios of 0.96 .. 1.08 wherever the error is above the fp32 floor - so the factor 2 is what a
  wrong tail has to beat: one key counted twice, or one dS left alive past the sequence, gives ratios of 7 and more (measured on
  scratch builds) and fails sections 1 and 2 at every n that is no multiple of the tile.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import attention_bf16_ref as AR
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = AR.SCALE
ERR_ARG = -1
ENTRIES = ("mode", "bf16out")


def _fwd_bwd(ops, qkv, dout, B, H, n, entry="bf16out", want_f32=True):
    """forward, then the backward from that forward's own out and lse -> dict of device tensors"""
    with ops.gemm_mode(ops.GEMM_BF16):
        if entry == "mode":                  # d2s_attn_fwd_bf16 / d2s_attn_bwd_bf16
            out, lse, cls_row = ops.attn_fwd(qkv, B, n, H, SCALE, want_cls=True)
            return dict(out=out, lse=lse, cls_row=cls_row, dqkv=ops.attn_bwd(qkv, out, dout, lse, B, n, H, SCALE))
        out, lse, cls_row, out16 = ops.attn_fwd_bf16io(qkv, B, n, H, SCALE, want_cls=True)
        dqkv16 = torch.empty(qkv.shape, dtype=torch.bfloat16, device=qkv.device)
        dqkv = ops.attn_bwd(qkv, out, dout, lse, B, n, H, SCALE, dqkv16=dqkv16, want_f32=want_f32)
        return dict(out=out, lse=lse, cls_row=cls_row, out16=out16, dqkv=dqkv, dqkv16=dqkv16)


_GOT = {}


def _got(B, H, n, kind, entry):
    """one GPU run per case and entry, on the CPU in the reference's layout; shared by sections 1 and 2"""
    key = (B, H, n, kind, entry)
    if key not in _GOT:
        from d2s import ops
        qkv, dout = AR.inputs(B, H, n, kind)
        g = _fwd_bwd(ops, qkv.to(DEV), dout.to(DEV), B, H, n, entry)
        torch.cuda.synchronize()
        dq, dk, dv = AR.split(g["dqkv"].cpu(), B, H, n)
        _GOT[key] = dict(out=AR.heads(g["out"].cpu(), B, H, n), lse=g["lse"].cpu(), cls_row=g["cls_row"].cpu(), dq=dq, dk=dk, dv=dv)
    return _GOT[key]


# ---- 1. per-element bounds ----
@pytest.mark.parametrize("B,H,n", AR.SHAPES)
@pytest.mark.parametrize("kind", AR.KINDS)
def test_forward_and_backward_within_the_derived_bounds(B, H, n, kind):
    ref = AR.reference(B, H, n, kind)
    for entry in ENTRIES:
        got = _got(B, H, n, kind, entry)
        for name in AR.OUTPUTS:
            assert got[name].shape == ref[name].shape and bool(torch.isfinite(got[name]).all()), (entry, name)
        fracs = AR.bound_fractions(got, ref)
        print(f"dense attention bf16 B{B} H{H} n{n} {kind} {entry}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
        for k, v in fracs.items():
            assert v <= 1.0, (entry, k, v)


# ---- 2. yardstick ----
@pytest.mark.parametrize("B,H,n", AR.SHAPES)
@pytest.mark.parametrize("kind", AR.KINDS)
def test_relative_l2_error_within_twice_the_emulations(B, H, n, kind):
    ref, emu = AR.reference(B, H, n, kind), AR.emulate(B, H, n, kind)
    floor = AR.l2_floor(n)
    for entry in ENTRIES:
        got = _got(B, H, n, kind, entry)
        ratios, bad = {}, []
        for name in AR.L2_OUTPUTS:
            e_got, norm = AR.l2_errors(got, ref, name)
            e_emu, _ = AR.l2_errors(emu, ref, name)
            over = (e_got - floor * norm).clamp(min=0.0)
            ratios[name] = float(torch.where(over > 0, over / e_emu, torch.zeros_like(over)).max())
            if not bool((e_got <= 2.0 * e_emu + floor * norm).all()):
                bad.append((name, (e_got / norm).tolist(), (e_emu / norm).tolist()))
        print(f"dense attention bf16 B{B} H{H} n{n} {kind} {entry}: L2 error over the emulation's " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        assert not bad, (entry, bad)


# ---- 3. consistency ----
def _same(a, b, what, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{what} differ in {k}"


def _with_ties(B, H, n):
    """fp32 qkv that is not bf16-representable, with exact round-to-nearest-even ties planted in q, k and v"""
    from d2s import synth
    qkv = torch.from_numpy(synth.normal(f"da16/ties/{B}/{H}/{n}", (B * n, 3 * H * 64), std=0.7, seed=7)).view(B, n, 3, H, 64).clone()
    lo, hi = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8           # -> 1 and 1 + 2^-6: the even neighbour, once below and once above
    ties = torch.tensor([lo, hi, -lo, -hi, 0.5 * lo, 4.0 * hi], dtype=torch.float32)
    for part in range(3):
        qkv[0, 0, part, 0, :6] = ties
        qkv[B - 1, n - 1, part, H - 1, 58:] = ties
    qkv = qkv.view(B * n, 3 * H * 64).contiguous()
    assert not torch.equal(qkv, qkv.bfloat16().float())
    assert qkv.bfloat16().float().view(B, n, 3, H, 64)[0, 0, 0, 0, :6].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, -1.0 - 2.0 ** -6, 0.5, 4.0 + 2.0 ** -4]
    return qkv


@pytest.mark.parametrize("i,shape", list(enumerate(AR.SHAPES)))
def test_forms_of_the_entries_agree_bit_for_bit(i, shape):
    from d2s import ops
    B, H, n = shape
    qkv, dout = AR.inputs(B, H, n, AR.KINDS[i % 3])
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    every = ("out", "lse", "cls_row", "out16", "dqkv", "dqkv16")
    a = _fwd_bwd(ops, qkv, dout, B, H, n)
    b = _fwd_bwd(ops, qkv.bfloat16(), dout, B, H, n)
    again = _fwd_bwd(ops, qkv, dout, B, H, n)
    plain = _fwd_bwd(ops, qkv, dout, B, H, n, entry="mode")
    only16 = _fwd_bwd(ops, qkv, dout, B, H, n, want_f32=False)
    with ops.gemm_mode(ops.GEMM_BF16):
        fwd16 = ops.attn_fwd_bf16io(qkv, B, n, H, SCALE, want_cls=True, want_f32=False)
    tq = _with_ties(B, H, n).to(DEV)
    t32, t16 = _fwd_bwd(ops, tq, dout, B, H, n), _fwd_bwd(ops, tq.bfloat16(), dout, B, H, n)
    torch.cuda.synchronize()
    _same(a, b, "fp32 and bf16 qkv", every)
    _same(a, again, "two launches", every)
    _same(a, plain, "d2s_attn_*_bf16 and d2s_attn_*_bf16_bf16out", ("out", "lse", "cls_row", "dqkv"))
    assert torch.equal(a["out16"], a["out"].bfloat16()) and torch.equal(a["dqkv16"], a["dqkv"].bfloat16())
    assert fwd16[0] is None and torch.equal(fwd16[3], a["out16"]) and torch.equal(fwd16[1], a["lse"]) and torch.equal(fwd16[2], a["cls_row"])
    assert only16["dqkv"] is None and torch.equal(only16["dqkv16"], a["dqkv16"])
    _same(t32, t16, "fp32 qkv with rounding ties and its bfloat16()", every)
    assert bool(torch.isfinite(t32["dqkv"]).all()) and float(t32["dqkv"].abs().max()) > 0


# ---- 4. both tile forms ----
def test_module_passes_in_both_forced_tile_forms():
    """D2S_ATTN_BF16_T64 = 0: every length, n >= 384 included, runs the 32-key-tile forward; = 2: every length runs the 64-key-tile forward,
    n = 1 .. 63 with one mostly masked tile.  One child at a time; the second starts only after the first passed."""
    for mode in ("0", "2"):
        env = dict(os.environ, D2S_ATTN_BF16_T64=mode)
        res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", "not both_forced_tile_forms"],
                             env=env, capture_output=True, text=True, timeout=900, cwd=cases.REPO)
        for line in res.stdout.splitlines():
            if line.startswith("dense attention bf16"):
                print(f"T64={mode} {line}")
        rc = res.returncode
        assert rc == 0 and rc not in (124, 134, 137, 139) and rc >= 0, (mode, rc, res.stdout[-3000:] + res.stderr[-1000:])
        assert " passed" in res.stdout and "skipped" not in res.stdout.splitlines()[-1], res.stdout[-500:]


# ---- 5. argument checks ----
def test_the_four_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    B, H, n = 2, 2, 17
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    h = lambda *shape: torch.full(shape, 7.0, dtype=torch.bfloat16, device=DEV)
    qkv, dout, fout = torch.full((B * n, 3 * H * 64), 0.5, device=DEV), f(B * n, H * 64), f(B * n, H * 64)      # inputs: scores of 2.0
    out, out16, lse, cls_row, dqkv, dqkv16, delta = f(B * n, H * 64), h(B * n, H * 64), f(B, H, n), f(B, H, n), f(B * n, 3 * H * 64), h(B * n, 3 * H * 64), f(B, H, n)
    outputs = (out, out16, lse, cls_row, dqkv, dqkv16, delta)
    p, s, sc = lib.ptr, lib.stream(), ctypes.c_float(SCALE)

    def fwd(q=qkv, o=out, l=lse, n_=n):
        return lib._fn("d2s_attn_fwd_bf16")(p(q), p(o), p(l), p(cls_row), B, n_, H, sc, s)

    def fwd16(q=qkv, o=out, o16=out16, l=lse, n_=n):
        return lib._fn("d2s_attn_fwd_bf16_bf16out")(p(q), 0, p(o), p(o16), p(l), p(cls_row), B, n_, H, sc, s)

    def bwd(q=qkv, l=lse, dq=dqkv, ws=delta, n_=n):
        return lib._fn("d2s_attn_bwd_bf16")(p(q), p(fout), p(dout), p(l), p(dq), p(ws), B, n_, H, sc, s)

    def bwd16(q=qkv, l=lse, dq=dqkv, dq16=dqkv16, ws=delta, n_=n):
        return lib._fn("d2s_attn_bwd_bf16_bf16out")(p(q), 0, p(fout), p(dout), p(l), p(dq), p(dq16), p(ws), B, n_, H, sc, s)

    bad = [fwd(q=None), fwd(o=None), fwd(l=None), fwd(n_=0), fwd(n_=8193),
           fwd16(q=None), fwd16(o16=None), fwd16(l=None), fwd16(n_=0), fwd16(n_=8193),
           bwd(q=None), bwd(l=None), bwd(dq=None), bwd(ws=None), bwd(n_=0),
           bwd16(q=None), bwd16(l=None), bwd16(dq16=None), bwd16(dq=None, dq16=None), bwd16(ws=None), bwd16(n_=0)]
    torch.cuda.synchronize()
    assert bad == [ERR_ARG] * len(bad), bad
    for t in outputs:                                     # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    with pytest.raises(lib.D2SError):
        lib.call("d2s_attn_fwd_bf16", None, p(out), p(lse), None, B, n, H, SCALE)
    assert fwd() == 0 and fwd16() == 0 and fwd16(o=None) == 0       # the accepted forms launch and write (lse first: the backward reads it)
    assert bwd() == 0 and bwd16() == 0 and bwd16(dq=None) == 0
    torch.cuda.synchronize()
    for t in outputs:
        assert bool(torch.isfinite(t.float()).all()) and not bool((t == 7).all())
