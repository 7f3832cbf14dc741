"""GPU tier of training on the ragged packed batch in the bf16 arithmetic mode (ragged_bf16=True / --ragged-bf16):
d2s_attn_varlen_fwd_lse_bf16 and d2s_attn_varlen_bwd_bf16 (csrc/attention_bf16.hip, include/d2s_hip_ragged_bf16.h), RaggedBlockFn and
RaggedPredictorFn on the bf16 data path, the student, TrainStep and the command line.

The kernels are anchored twice.  Bit for bit: the forward's out / out_bf16 / cls_row to d2s_attn_varlen_fwd_bf16, each image's lse to
d2s_attn_policy_fwd_bf16 on that image alone with an all-ones policy and eps = 0 (the 32-key-tile kernel at every n; the dense entry
switches to 64-key tiles by length), each image's rows of dqkv / dqkv_bf16 to d2s_attn_bwd_bf16_bf16out on that image alone, fed the
same out, lse and dout.  Against float64: inputs, reference, per-element bounds and the rounding emulation are
tests/attention_bf16_ref.py, one image at a time (B = 1) - a packed batch is the concatenation of inputs(1, H, n_b, kind); the CPU tier
(tests/test_ragged_bf16_train_cpu.py) shows that the emulation alone stays inside the bounds at these lengths.  The relative-L2
criterion is the dense test's: |got - ref| <= 2 |emu - ref| + l2_floor(n) |ref| per (image, head) slice; where |ref| = 0 (dQ and dK
of a CLS-only image) the kernel must write exact zeros, and so must the dense entry at n = 1 (the ONE_KEY instantiations; without them
the tile loop leaves one bf16 rounding of dO there, 3.9e-3 to 1.1e-2, as tests/attention_bf16_ref.emulate does).

Lengths: (a) a CLS-only image, partial and full key tiles, and with the loose bound 64 whole workgroups that return early; (b) a second
workgroup that owns one query / key, B * H = 12 blocks per grid row (no multiple of the 8 XCDs); (c) DeiT's own length beside a short
image.

The block: D 128, 2 heads, hidden 512 (tests/test_ragged_bf16_gpu.py's geometry).  At equal lengths RaggedBlockFn(bf16=True) and BlockFn
run the same per-op sequence; where the dense forward is the 32-key-tile kernel too (n = 17, 65) y and all 13 gradients are bit-equal.
At n = 33 the dense entry runs its 64-key-tile forward (64-key tiles pad no more than 32-key tiles there), a launch the ragged form
does not have: that length is held to the float64 block reference instead, like the ragged lengths (5, 33) - y within the project's
bf16 model tolerance (3e-2, 3e-2), the gradients by the criteria of tests/test_model_gpu.py::test_bf16_gemm_mode_model_parity
(cosine > 0.97, norm within 10 %, relative L2 below 25 %, median below 8 %).  The model is held to the same two, with the GPU's own
masks replayed into the float64 restatement (tests/ragged_train_ref.py) as the fp32 tier does."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import attention_bf16_ref as AR
from tests import cases
from tests import ragged_train_ref as R
from oracle import d2s_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = AR.SCALE
ERR_ARG = -1                                   # D2S_ERR_ARG (include/d2s_hip.h)
SETS = {"a": ((1, 2, 17, 32, 33), 2, (33, 64)), "b": ((128, 129, 1, 97), 3, (129, 256)), "c": ((197, 70), 2, (197,))}
PACKED = [(name, max_n) for name in sorted(SETS) for max_n in SETS[name][2]]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cu(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)


def _packed(name, kind):
    """-> lengths, H, cu (device), qkv [total, 3*H*64], dout [total, H*64] (device): inputs(1, H, n_b, kind) image after image"""
    lengths, H, _ = SETS[name]
    parts = [AR.inputs(1, H, n, kind) for n in lengths]
    return lengths, H, _cu(lengths).to(DEV), torch.cat([p[0] for p in parts]).to(DEV), torch.cat([p[1] for p in parts]).to(DEV)


_FWD = {}


def _forward(name, max_n, kind):
    """one forward per case, shared by the tests that need it and never modified -> dict(out, lse, cls_row, out16) on the device"""
    key = (name, max_n, kind)
    if key not in _FWD:
        from d2s import ops
        lengths, H, cu, qkv, _ = _packed(name, kind)
        out, lse, cls_row, out16 = ops.attn_varlen_fwd_lse_bf16io(qkv, cu, len(lengths), qkv.shape[0], max_n, H, SCALE, want_cls=True)
        _FWD[key] = dict(out=out, lse=lse, cls_row=cls_row, out16=out16)
    return _FWD[key]


# ---- 1. forward ----
@pytest.mark.parametrize("kind", AR.KINDS)
@pytest.mark.parametrize("name,max_n", PACKED)
def test_forward_is_the_inference_entry_and_its_lse_the_32_key_tile_kernels(name, max_n, kind):
    from d2s import ops
    lengths, H, cu, qkv, _ = _packed(name, kind)
    B, total = len(lengths), qkv.shape[0]
    got = _forward(name, max_n, kind)
    out, cls_row, out16 = ops.attn_varlen_fwd_bf16io(qkv, cu, B, total, max_n, H, SCALE, want_cls=True)
    assert torch.equal(got["out"], out) and torch.equal(got["out16"], out16) and torch.equal(got["cls_row"], cls_row)
    assert tuple(got["lse"].shape) == (H, total) and bool(torch.isfinite(got["lse"]).all())
    # qkv in bf16 (the qkv GEMM's c16), the forms without the fp32 output and without the CLS row
    h = ops.attn_varlen_fwd_lse_bf16io(qkv.bfloat16(), cu, B, total, max_n, H, SCALE, want_cls=True)
    o16 = ops.attn_varlen_fwd_lse_bf16io(qkv, cu, B, total, max_n, H, SCALE, want_cls=False, want_f32=False)
    for a, b in zip(h, (got["out"], got["lse"], got["cls_row"], got["out16"])):
        assert torch.equal(a, b), "fp32 and bf16 qkv"
    assert o16[0] is None and o16[2] is None and torch.equal(o16[1], got["lse"]) and torch.equal(o16[3], got["out16"])
    worst = 0.0
    for b, n in enumerate(lengths):
        r0 = int(cu[b])
        _, lse32, _, _, _ = ops.attn_policy_fwd_bf16io(qkv[r0:r0 + n].contiguous(), torch.ones((1, n), device=DEV), 1, n, H, SCALE, eps=0.0,
                                                       want_bf16=False)
        assert torch.equal(got["lse"][:, r0:r0 + n], lse32[0]), f"image {b} (n {n}): lse of the 32-key-tile kernel on that image alone"
        ref = AR.reference(1, H, n, kind)
        frac = float(((got["lse"][:, r0:r0 + n].cpu().double() - ref["lse"][0]).abs() / ref["lse_bound"][0]).max())
        worst = max(worst, frac)
        assert frac <= 1.0, (b, n, frac)
    print(f"varlen lse bf16 set {name} max_n {max_n} {kind}: max err / bound {worst:.3f}")


# ---- 2. backward ----
def _bwd_raw(qkv, cu, out, dout, lse, B, total, max_n, H, dqkv, dqkv16):
    """the entry itself, into buffers of the caller's (a poisoned guard band behind them)"""
    from d2s import lib
    delta = torch.empty((H, total), dtype=torch.float32, device=DEV)
    lib.call("d2s_attn_varlen_bwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(cu), lib.ptr(out), lib.ptr(dout), lib.ptr(lse),
             lib.ptr(dqkv), lib.ptr(dqkv16), lib.ptr(delta), B, total, max_n, H, float(SCALE))


@pytest.mark.parametrize("kind", AR.KINDS)
@pytest.mark.parametrize("name,max_n", PACKED)
def test_backward_is_the_dense_backward_per_image_and_within_the_float64_bounds(name, max_n, kind):
    from d2s import ops
    lengths, H, cu, qkv, dout = _packed(name, kind)
    B, total, W = len(lengths), qkv.shape[0], 3 * H * 64
    fwd = _forward(name, max_n, kind)
    out, lse = fwd["out"], fwd["lse"]
    GUARD = 3
    poison = lambda dtype: torch.full((total + GUARD, W), 7.0, dtype=dtype, device=DEV)
    dqkv, dqkv16 = poison(torch.float32), poison(torch.bfloat16)
    _bwd_raw(qkv, cu, out, dout, lse, B, total, max_n, H, dqkv, dqkv16)
    # the op (its own buffers), a second launch, bf16 qkv, the bf16-only form
    d16 = torch.empty((total, W), dtype=torch.bfloat16, device=DEV)
    again = ops.attn_varlen_bwd_bf16io(qkv, cu, out, dout, lse, B, total, max_n, H, SCALE, dqkv16=d16)
    h16 = torch.empty((total, W), dtype=torch.bfloat16, device=DEV)
    from_h = ops.attn_varlen_bwd_bf16io(qkv.bfloat16(), cu, out, dout, lse, B, total, max_n, H, SCALE, dqkv16=h16)
    only16 = torch.full((total, W), 7.0, dtype=torch.bfloat16, device=DEV)
    none = ops.attn_varlen_bwd_bf16io(qkv, cu, out, dout, lse, B, total, max_n, H, SCALE, dqkv16=only16, want_f32=False)
    only32 = ops.attn_varlen_bwd_bf16io(qkv, cu, out, dout, lse, B, total, max_n, H, SCALE)
    torch.cuda.synchronize()
    assert bool((dqkv[total:] == 7).all()) and bool((dqkv16[total:] == 7).all()), "the guard band behind dqkv / dqkv_bf16"
    g, g16 = dqkv[:total], dqkv16[:total]
    assert bool(torch.isfinite(g).all())
    assert torch.equal(again, g) and torch.equal(d16, g16), "two launches"
    assert torch.equal(from_h, g) and torch.equal(h16, g16), "fp32 and bf16 qkv"
    assert none is None and torch.equal(only16, g16), "the bf16-only form"
    assert torch.equal(only32, g), "the fp32-only form"
    assert torch.equal(g16, g.bfloat16()), "dqkv_bf16 is dqkv rounded as torch rounds"
    fracs, ratios = {}, {}
    for b, n in enumerate(lengths):
        r0 = int(cu[b])
        rows = slice(r0, r0 + n)
        # bit for bit the dense backward on that image alone, fed the same out, lse and dout
        dense16 = torch.empty((n, W), dtype=torch.bfloat16, device=DEV)
        with ops.gemm_mode(ops.GEMM_BF16):
            dense = ops.attn_bwd(qkv[rows].contiguous(), out[rows].contiguous(), dout[rows].contiguous(), lse[:, rows].contiguous().view(1, H, n),
                                 1, n, H, SCALE, dqkv16=dense16)
        assert torch.equal(g[rows], dense) and torch.equal(g16[rows], dense16), f"image {b} (n {n})"
        # float64: per-element bounds and the relative-L2 criterion of the dense test
        ref, emu = AR.reference(1, H, n, kind), AR.emulate(1, H, n, kind)
        dq, dk, dv = AR.split(g[rows].cpu(), 1, H, n)
        got = dict(dq=dq, dk=dk, dv=dv)
        floor = AR.l2_floor(n)
        for k in ("dq", "dk", "dv"):
            frac = float(((got[k].double() - ref[k]).abs() / ref[k + "_bound"]).max()) if float(ref[k + "_bound"].max()) > 0 else 0.0
            fracs[k] = max(fracs.get(k, 0.0), frac)
            assert frac <= 1.0, (b, n, k, frac)
            e_got, norm = AR.l2_errors(got, ref, k)
            e_emu, _ = AR.l2_errors(emu, ref, k)
            for h in range(H):
                if float(norm[0, h]) == 0.0:                                   # dQ = dK = 0 exactly at n = 1 (one key: P = 1, dS = 0)
                    assert n == 1 and k in ("dq", "dk") and bool((got[k][0, h] == 0).all()), (b, n, k, h)
                    continue
                assert float(e_got[0, h]) <= 2.0 * float(e_emu[0, h]) + floor * float(norm[0, h]), (b, n, k, h, float(e_got[0, h]), float(e_emu[0, h]),
                                                                                                  float(norm[0, h]))
                over = max(float(e_got[0, h]) - floor * float(norm[0, h]), 0.0)
                if over > 0:
                    ratios[k] = max(ratios.get(k, 0.0), over / float(e_emu[0, h]))
    print(f"varlen bwd bf16 set {name} max_n {max_n} {kind}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fracs.items())
          + "; L2 error over the emulation's " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("name,max_n", [("a", 33), ("b", 256)])
def test_rows_that_cu_seqlens_does_not_cover_stay_untouched(name, max_n):
    """cu_seqlens over a prefix of `total` (the last image left out): its rows keep the poison, the covered rows their bits"""
    lengths, H, cu, qkv, dout = _packed(name, "normal")
    B, total, W = len(lengths), qkv.shape[0], 3 * H * 64
    fwd = _forward(name, max_n, "normal")
    full, full16 = torch.empty((total, W), device=DEV), torch.empty((total, W), dtype=torch.bfloat16, device=DEV)
    _bwd_raw(qkv, cu, fwd["out"], dout, fwd["lse"], B, total, max_n, H, full, full16)
    part, part16 = torch.full((total, W), 7.0, device=DEV), torch.full((total, W), 7.0, dtype=torch.bfloat16, device=DEV)
    _bwd_raw(qkv, cu[:B].contiguous(), fwd["out"], dout, fwd["lse"], B - 1, total, max_n, H, part, part16)
    torch.cuda.synchronize()
    covered = int(cu[B - 1])
    assert 0 < covered < total
    assert torch.equal(part[:covered], full[:covered]) and torch.equal(part16[:covered], full16[:covered])
    assert bool((part[covered:] == 7).all()) and bool((part16[covered:] == 7).all())


def test_a_cls_only_image_gets_exact_zeros_in_dq_and_dk():
    """At n = 1 the softmax row is P = 1, so dS = P (dP - delta) = 0 and dQ = dK = 0 exactly: the ragged entry writes exact zeros on a
    CLS-only image's rows, and d2s_attn_bwd_bf16_bf16out on that image alone (B = 1, n = 1) writes the same, for every kind of input.
    (The tile loop alone leaves dS = (rb(dO) - dO) . v there - dP multiplies the bf16-rounded dO, delta the unrounded one: max |dq|
    3.9e-3 to 1.1e-2, max |dk| 4.1e-3 to 6.0e-3 on these inputs, what emulate() gives; the ONE_KEY instantiations write the exact value.)
    dV = P^T dO = dO rounded to bf16 is untouched."""
    from d2s import ops
    for kind in AR.KINDS:
        lengths, H, cu, qkv, dout = _packed("a", kind)
        assert lengths[0] == 1
        fwd = _forward("a", 33, kind)
        g = ops.attn_varlen_bwd_bf16io(qkv, cu, fwd["out"], dout, fwd["lse"], len(lengths), qkv.shape[0], 33, H, SCALE)
        d16 = torch.empty((1, 3 * H * 64), dtype=torch.bfloat16, device=DEV)
        with ops.gemm_mode(ops.GEMM_BF16):
            dense = ops.attn_bwd(qkv[:1].contiguous(), fwd["out"][:1].contiguous(), dout[:1].contiguous(), fwd["lse"][:, :1].contiguous().view(1, H, 1),
                                 1, 1, H, SCALE, dqkv16=d16)
            plain = ops.attn_bwd(qkv[:1].contiguous(), fwd["out"][:1].contiguous(), dout[:1].contiguous(), fwd["lse"][:, :1].contiguous().view(1, H, 1),
                                 1, 1, H, SCALE)
        torch.cuda.synchronize()
        ref = AR.reference(1, H, 1, kind)
        assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0
        for what, t in (("ragged", g[:1]), ("dense bf16out", dense), ("dense", plain), ("dense bf16 form", d16.float())):
            dq, dk, dv = AR.split(t.cpu(), 1, H, 1)
            assert bool((dq == 0).all()) and bool((dk == 0).all()), (kind, what, float(dq.abs().max()), float(dk.abs().max()))
            assert float(dv.abs().max()) > 0, (kind, what)
        assert torch.equal(g[:1], dense) and torch.equal(dense, plain)


# ---- 3. refusals ----
def test_both_entries_refuse_bad_arguments_without_launching():
    from d2s import lib
    lib.load()
    lengths, H = (5, 12), 2
    B, total, max_n = len(lengths), sum(lengths), 12
    cu = _cu(lengths).to(DEV)
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    h = lambda *shape: torch.full(shape, 7.0, dtype=torch.bfloat16, device=DEV)
    qkv, dout, fout = torch.full((total, 3 * H * 64), 0.5, device=DEV), f(total, H * 64), f(total, H * 64)
    out, out16, lse, cls_row, dqkv, dqkv16, delta = f(total, H * 64), h(total, H * 64), f(H, total), f(H, total), f(total, 3 * H * 64), \
        h(total, 3 * H * 64), f(H, total)
    outputs = (out, out16, lse, cls_row, dqkv, dqkv16, delta)
    p, s, sc = lib.ptr, lib.stream(), ctypes.c_float(SCALE)

    def fwd(q=qkv, c=cu, o=out, o16=out16, l=lse, dims=(B, total, max_n, H)):
        return lib._fn("d2s_attn_varlen_fwd_lse_bf16")(p(q), 0, p(c), p(o), p(o16), p(l), p(cls_row), *dims, sc, s)

    def bwd(q=qkv, c=cu, o=fout, do=dout, l=lse, dq=dqkv, dq16=dqkv16, ws=delta, dims=(B, total, max_n, H)):
        return lib._fn("d2s_attn_varlen_bwd_bf16")(p(q), 0, p(c), p(o), p(do), p(l), p(dq), p(dq16), p(ws), *dims, sc, s)

    bad_dims = [(0, total, max_n, H), (B, 0, max_n, H), (B, total, 0, H), (B, total, max_n, 0), (-1, total, max_n, H), (B, total, 8193, H)]
    bad = [fwd(q=None), fwd(c=None), fwd(o=None, o16=None), fwd(l=None)] + [fwd(dims=d) for d in bad_dims]
    bad += [bwd(q=None), bwd(c=None), bwd(o=None), bwd(do=None), bwd(l=None), bwd(ws=None), bwd(dq=None, dq16=None)] + [bwd(dims=d) for d in bad_dims]
    torch.cuda.synchronize()
    assert bad == [ERR_ARG] * len(bad), bad
    for t in outputs:                                     # nothing was launched: no output buffer was touched
        assert bool((t == 7).all())
    with pytest.raises(lib.D2SError):
        lib.call("d2s_attn_varlen_fwd_lse_bf16", p(qkv), 0, p(cu), p(out), p(out16), None, None, B, total, max_n, H, SCALE)
    # the accepted forms launch and write: either output form alone, the CLS row optional; max_n = 8192 is inside the limit
    assert fwd() == 0 and fwd(o=None) == 0 and fwd(o16=None) == 0 and fwd(dims=(B, total, 8192, H)) == 0
    assert bwd(l=lse) == 0 and bwd(dq=None) == 0 and bwd(dq16=None) == 0
    torch.cuda.synchronize()
    for t in outputs:
        assert bool(torch.isfinite(t.float()).all()) and not bool((t == 7).all())


# ---- 4. RaggedBlockFn on the bf16 data path ----
_NAMES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
BLOCK_D, BLOCK_H, BLOCK_HID = 128, 2, 512
BLOCK_CFG = dict(dim=BLOCK_D, heads=BLOCK_H, ln_eps=1e-6)


def _block_params():
    """the block of tests/test_ragged_bf16_gpu.py"""
    from d2s import synth
    D, hid = BLOCK_D, BLOCK_HID
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hid, D), (hid,), (D, hid), (D,)]
    p = [_t(synth.normal(f"rg16/block/p{i}", s, std=0.05 if len(s) == 2 else 0.1, seed=11)) for i, s in enumerate(shapes)]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    return p


def _block_inputs(lengths, tag):
    from d2s import synth
    total = sum(lengths)
    x = _t(synth.normal(f"rg16t/{tag}/x", (total, BLOCK_D), seed=21))
    gy = _t(synth.normal(f"rg16t/{tag}/gy", (total, BLOCK_D), seed=22))
    return x, gy


def _ragged_block_run(lengths, x, gy, bf16=True, mode=None, stage=False):
    """RaggedBlockFn forward and backward -> (y, [gx, 12 parameter gradients]) on the device"""
    from d2s import ops
    from d2s import functional_ats as AF
    mode = ops.GEMM_BF16 if mode is None else mode
    B = len(lengths)
    cu = _cu(lengths).to(DEV)
    p = [t.to(DEV).requires_grad_(True) for t in _block_params()]
    xd = x.to(DEV).requires_grad_(True)
    with ops.gemm_mode(mode):
        if stage:
            row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
            r = AF._Ragged(cu, B, max(lengths), BLOCK_H, SCALE, row_src, 4, max(lengths) - 1, None, bf16=bf16)
        else:
            r = AF._Ragged(cu, B, max(lengths), BLOCK_H, SCALE, bf16=bf16)
        y = AF.ragged_block_train(xd, p, 1e-6, r)
        grads = torch.autograd.grad(y, [xd] + p, gy.to(DEV))
        ops.join_weight_grads()
    torch.cuda.synchronize()
    return y.detach(), [g.detach() for g in grads]


def _block_float64(lengths, x, gy):
    """the float64 block (the oracle's, which tests/ragged_train_ref.py is built from) image by image -> (y, [gx, 12 gradients])"""
    sd = {"blocks.0." + k: t.double().requires_grad_(True) for k, t in zip(_NAMES, _block_params())}
    xr = x.double().requires_grad_(True)
    cu = _cu(lengths)
    y = torch.cat([O.block(sd, 0, xr[int(cu[b]):int(cu[b + 1])][None], BLOCK_CFG)[0][0] for b in range(len(lengths))])
    grads = torch.autograd.grad(y, [xr] + [sd["blocks.0." + k] for k in _NAMES], gy.double())
    return y.detach(), list(grads)


def _assert_bf16_parity(what, y, grads, y64, grads64):
    """the project's bf16 tolerances: y (3e-2, 3e-2); gradients as tests/test_model_gpu.py::test_bf16_gemm_mode_model_parity"""
    np.testing.assert_allclose(y.cpu().numpy(), y64.float().numpy(), rtol=3e-2, atol=3e-2)
    errs = []
    for name, g, w in zip(("x",) + _NAMES, grads, grads64):
        gd, go = g.cpu().double().flatten(), w.flatten()
        assert float(go.norm()) >= 1e-6, name
        err = float((gd - go).norm() / go.norm())
        cos = float((gd @ go) / (gd.norm() * go.norm()))
        errs.append(err)
        assert cos > 0.97, (what, name, cos)
        np.testing.assert_allclose(float(gd.norm()), float(go.norm()), rtol=1e-1, err_msg=f"{what} {name}")
    print(f"{what}: max |y - float64| {float((y.cpu().double() - y64).abs().max()):.3e}; relative L2 gradient error vs float64: median "
          f"{np.median(errs):.3e}, worst {max(errs):.3e}")
    assert max(errs) < 0.25 and np.median(errs) < 0.08, (what, max(errs), float(np.median(errs)))


def _dense_runs_32_key_tiles(n):
    """the rule of the dense entry (attention_bf16.hip, attn_t64, default setting)"""
    return not (n >= 384 or (n + 63) // 64 * 64 == (n + 31) // 32 * 32)


@pytest.mark.parametrize("n", [17, 33, 65])
def test_block_on_equal_lengths_against_the_dense_block(n):
    from d2s import ops
    from d2s import functional as DF
    B = 3
    lengths = [n] * B
    x, gy = _block_inputs(lengths, f"eq{n}")
    y, grads = _ragged_block_run(lengths, x, gy)
    p = [t.to(DEV).requires_grad_(True) for t in _block_params()]
    xd = x.to(DEV).view(B, n, BLOCK_D).requires_grad_(True)
    with ops.gemm_mode(ops.GEMM_BF16):
        yd, _ = DF.run(DF.BlockFn, xd, *p, BLOCK_H, 1e-6, False, None)
        gd = torch.autograd.grad(yd, [xd] + p, gy.to(DEV).view(B, n, BLOCK_D))
        ops.join_weight_grads()
    torch.cuda.synchronize()
    same = [torch.equal(y, yd.detach().view(B * n, BLOCK_D))] + [torch.equal(a, b.detach().reshape(a.shape)) for a, b in zip(grads, gd)]
    print(f"ragged block bf16 on equal lengths n {n}: bit-equal to BlockFn: y {same[0]}, gradients {sum(same[1:])}/13")
    if _dense_runs_32_key_tiles(n):
        assert all(same), same
    else:      # n = 33: the dense forward is the 64-key-tile kernel there, the one launch the ragged form does not have
        y64, g64 = _block_float64(lengths, x, gy)
        _assert_bf16_parity(f"ragged block bf16 n {n}", y, grads, y64, g64)
        _assert_bf16_parity(f"dense block bf16 n {n}", yd.detach().view(B * n, BLOCK_D), [g.detach().reshape(a.shape) for g, a in zip(gd, grads)],
                            y64, g64)


def test_block_on_ragged_lengths_against_float64_and_two_runs():
    lengths = (5, 33)
    x, gy = _block_inputs(lengths, "rg")
    y, grads = _ragged_block_run(lengths, x, gy)
    y2, grads2 = _ragged_block_run(lengths, x, gy)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two runs"
    y64, g64 = _block_float64(lengths, x, gy)
    _assert_bf16_parity("ragged block bf16 lengths (5, 33)", y, grads, y64, g64)


def test_block_refusals():
    from d2s import lib, ops
    from d2s import functional_ats as AF
    lengths = (5, 9)
    x, gy = _block_inputs(lengths, "refuse")
    with pytest.raises(lib.D2SError) as e:
        _ragged_block_run(lengths, x, gy, stage=True)
    assert str(e.value) == AF._BF16_STAGE_REFUSAL and "sample_bwd" in str(e.value)
    for mode in (ops.GEMM_EXACT, ops.GEMM_SPLIT):
        with pytest.raises(lib.D2SError) as e:
            _ragged_block_run(lengths, x, gy, mode=mode)
        assert str(e.value) == AF._BF16_MODE_REFUSAL
    with pytest.raises(lib.D2SError) as e:
        _ragged_block_run(lengths, x, gy, bf16=False)
    assert str(e.value) == AF._BF16_REFUSAL
    with pytest.raises(lib.D2SError) as e:                                     # a stage block without the flag: the text it had
        _ragged_block_run(lengths, x, gy, bf16=False, stage=True)
    assert str(e.value) == AF._BF16_REFUSAL
    y, _ = _ragged_block_run(lengths, x, gy, bf16=False, mode=ops.GEMM_EXACT)   # and the fp32 route is what it was
    assert bool(torch.isfinite(y).all())


# ---- 5. the model and the step ----
def _student(case, **kw):
    import vit_models
    cfg = case["cfg"]
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    args = dict(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True,
                predictor_loss_type=cfg["loss_type"], small_predictor=cfg["small_predictor"], patch_score_threshold=case["threshold"])
    args.update(kw)
    student = vit_models.VisionTransformerDiffPruning(**args, **common)
    sd_s, sd_t = cases.make_weights(case)
    student.load_state_dict({k: _t(v) for k, v in sd_s.items()}, strict=True)
    teacher = vit_models.VisionTransformerTeacher(**common)
    teacher.load_state_dict({k: _t(v) for k, v in sd_t.items()}, strict=True)
    return student.to(DEV), teacher.to(DEV).eval()


def _args(case, **kw):
    cfg = case["cfg"]
    return types.SimpleNamespace(keep_ratios=list(cfg["token_ratio"]), mask_loss_type=cfg["loss_type"], mixup=0.0,
                                 patch_score_threshold=case["threshold"], ragged_train=True, step=0, **kw)


@pytest.mark.parametrize("name", ["micro_thr2", "micro_thr3s"])
def test_model_forward_and_gradients_against_float64(name):
    from d2s import ops
    from losses import MaskLoss, BackboneLoss
    case, _, _, x, y = R.case_tensors(name)
    cfg = case["cfg"]
    B, N, S = case["batch"], cfg["n_patches"], len(cfg["pruning_loc"])
    student, teacher = _student(case, ragged_train=True, ragged_bf16=True)
    student.train()
    args = _args(case)
    with ops.gemm_mode(ops.GEMM_BF16):
        with torch.no_grad():
            logits_t, token_t, cls_attn = teacher(x.to(DEV))
        logits, xn, pred_logits, masks = student(x.to(DEV))
        metrics = {}
        ragged = (list(student.cu_seqlens_per_stage), list(student.ragged_row_src_per_stage))
        mask_loss = MaskLoss(args, "train")(pred_logits, cls_attn, masks, metrics, ragged=ragged)
        backbone_loss = BackboneLoss(args)(logits, xn, logits_t, token_t, masks, y.to(DEV), metrics,
                                           ragged=(student.cu_seqlens, student.ragged_row_src))
        loss = mask_loss + backbone_loss
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    gpu_masks = [m.detach().cpu() for m in masks]
    assert len(masks) == len(pred_logits) == len(student.cu_seqlens_per_stage) == S
    assert tuple(xn.shape) == (int(student.cu_seqlens[-1]), cfg["dim"]) and int(student.cu_seqlens[-1]) < B * (N + 1), "the packed route ran"
    # float64 with the GPU's own masks
    out, want_loss, ref_grads, (want_mask, want_bb, _) = R.model_grads(name, masks=gpu_masks)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), out["logits"].detach().float().numpy(), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(xn.detach().cpu().numpy(), R.packed(out["feats"]).detach().float().numpy(), rtol=3e-2, atol=3e-2)
    errs, worst_name = [], ""
    for k, p in student.named_parameters():
        want = ref_grads[k]
        if want is None or float(want.norm()) < 1e-6:
            continue
        assert p.grad is not None, k
        gd, go = p.grad.detach().cpu().double().flatten(), want.flatten()
        err = float((gd - go).norm() / go.norm())
        cos = float((gd @ go) / (gd.norm() * go.norm()))
        if not errs or err > max(errs):
            worst_name = k
        errs.append(err)
        assert cos > 0.97, (k, cos)
        np.testing.assert_allclose(float(gd.norm()), float(go.norm()), rtol=1e-1, err_msg=k)
    print(f"{name} ragged bf16: loss {float(loss.detach()):.6f} (float64 {float(want_loss):.6f}), rows per stage "
          f"{[int(c[-1]) for c in student.cu_seqlens_per_stage]}; relative L2 gradient error vs float64: median {np.median(errs):.3e}, worst "
          f"{max(errs):.3e} ({worst_name})")
    assert max(errs) < 0.25 and np.median(errs) < 0.08, (max(errs), float(np.median(errs)), worst_name)
    later = [p.grad for k, p in student.named_parameters() if k.startswith(f"score_predictor.{S - 1}.")]
    assert later and all(g is not None and float(g.abs().max()) > 0 for g in later), "a later stage's predictor takes a gradient"


def test_keyword_changes_nothing_in_eval_or_in_an_fp32_mode_and_without_it_the_refusal_stands():
    from d2s import lib, ops
    from d2s.functional_ats import _BF16_REFUSAL
    case, _, _, x, _ = R.case_tensors("micro_thr2")
    on, _ = _student(case, ragged_train=True, ragged_bf16=True)
    off, _ = _student(case, ragged_train=True)
    plain, _ = _student(case)
    for mode in (ops.GEMM_BF16, ops.GEMM_EXACT):
        with ops.gemm_mode(mode), torch.no_grad():
            a, b = on.eval()(x.to(DEV)), plain.eval()(x.to(DEV))
        assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
        assert torch.equal(on.ragged_features, plain.ragged_features) and torch.equal(on.cu_seqlens, plain.cu_seqlens)
    with ops.gemm_mode(ops.GEMM_EXACT):                                        # an fp32 mode: the keyword changes nothing
        a, b = on.train()(x.to(DEV)), off.train()(x.to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:
            off.train()(x.to(DEV))
    assert str(e.value) == _BF16_REFUSAL


def _step(name="micro_thr2", bf16=True, **kw):
    from d2s.engine import TrainStep
    case = R.train_cases()[name]
    student, teacher = _student(case, ragged_train=True, **({"ragged_bf16": True} if bf16 else {}))
    return TrainStep(student, teacher, _args(case), lr=1e-3, **kw), case


def test_train_step_two_runs_resume_and_refusals():
    from d2s import lib, ops
    ops.set_gemm_mode(ops.GEMM_BF16)
    try:
        ts, case = _step()
        assert ts.ragged_train and ts.graph is False
        x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
        info = ts(x, y)
        torch.cuda.synchronize()
        assert np.isfinite(float(info["loss"]))
        masks = [m.detach().cpu() for m in info["kept"]]
        _, want, _, _ = R.model_grads("micro_thr2", masks=masks)
        print(f"train step ragged bf16: loss {float(info['loss']):.6f}, float64 {float(want):.6f}")
        np.testing.assert_allclose(float(info["loss"]), float(want), rtol=3e-2)
        saved = ts.state_dict()
        assert saved["config"]["ragged_bf16"] is True and saved["config"]["ragged_train"] is True and saved["config"]["gemm_mode"] == ops.GEMM_BF16
        l2 = float(ts(x, y)["loss"])
        torch.cuda.synchronize()
        two = ts.arena.params.clone()
        again, _ = _step()
        la = [float(again(x, y)["loss"]), float(again(x, y)["loss"])]
        torch.cuda.synchronize()
        assert la == [float(info["loss"]), l2] and torch.equal(again.arena.params, two), "a second run of two steps: bit-identical"
        resumed, _ = _step()
        assert resumed.load_state_dict(saved) == saved["epoch"]
        assert float(resumed(x, y)["loss"]) == l2
        torch.cuda.synchronize()
        assert torch.equal(resumed.arena.params, two), "save after step 1, resume, step 2: bit for bit"
        off, _ = _step(bf16=False)                                             # built without the keyword: never run in this mode, only loaded into
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ragged_bf16"):
            off.load_state_dict(saved)
        old = dict(saved, config={k: v for k, v in saved["config"].items() if k != "ragged_bf16"})      # written before the key existed: off
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ragged_bf16"):
            resumed.load_state_dict(old)
        assert off.load_state_dict(old) == saved["epoch"]
        with pytest.raises(lib.D2SError, match=r"graph=True\) with ragged_train"):
            _step(graph=True)
    finally:
        ops.set_gemm_mode(ops.GEMM_EXACT)


def test_cli_trains_on_the_ragged_batch_in_the_bf16_mode(tmp_path, capsys):
    import mask_predictor
    import vit_models
    from d2s import ops
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    try:
        acc = mask_predictor.main(["--arch", "deit_tiny", "--topk-selection", "--patch-score-threshold", "0.4", "--pruning-locs", "3", "6",
                                   "--keep-ratios", "0.7", "0.5", "--ragged-cascade", "--ragged-train", "--ragged-bf16", "--warmup-steps", "1",
                                   "--epochs", "2", "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--teacher-checkpoint", path,
                                   "--output-dir", out_dir])
        mode = ops.get_gemm_mode()
    finally:
        ops.set_gemm_mode(ops.GEMM_EXACT)                                       # main sets the process's mode: the other tests' default back
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0 and mode == ops.GEMM_BF16
    assert "Attention: --ragged-bf16: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    assert "Start training" in out and "val loss:" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert cfg["ragged_bf16"] is True and cfg["ragged_train"] is True and cfg["gemm_mode"] == ops.GEMM_BF16
