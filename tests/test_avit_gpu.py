"""The A-ViT baseline on the GPU: the four kernels of csrc/avit.hip against the float64 loops of tests/avit_ref.py
(bounds c * 2^-24 * sum |summands| per output, two launches bit-equal, refusals with poisoned outputs, a guard band behind every output),
the model in the micro geometry against the dense masked float64 restatement (halting layers exactly, logits per arithmetic mode, every
image alone, every parameter gradient and the loss), TrainStep (bit-identical runs, save and resume, accumulation with clipping, the
refusals) and the command line."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import avit_ref as R
from tests.test_avit_cpu import AVIT_CASES, CFG, EPS, built, check_condition

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
LENS = [1, 2, 17, 33, 197]
N_TOK = 197
GUARD, POISON = 64, 1234.5
WORST = {}
SEEDS = {128: 500, 192: 504, 384: 500}     # picked on the CPU with the float64 loops: every decision at least 1e-3 from the threshold


def _frac(tag, err, bound):
    """err <= bound elementwise; the worst observed fraction of the bound is printed and kept"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    f = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    WORST[tag] = max(WORST.get(tag, 0.0), f)
    print(f"  {tag}: worst fraction of the bound {f:.3f} (over the tests so far {WORST[tag]:.3f})")
    assert f <= 1.0, (tag, f)


# ---- 1. the halting step ----
def _scenario(kind, D, seed):
    """-> dict: y0 [total, D] fp32 of the first layer, cu, row_src, state arrays (fp32 / int32), gamma, beta, L"""
    g = torch.Generator().manual_seed(seed)
    total = sum(LENS)
    cu = np.asarray([0] + list(np.cumsum(LENS)), dtype=np.int32)
    row_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), torch.sort(torch.randperm(N_TOK - 1, generator=g)[:n - 1])[0] + 1))
                         for n in LENS]).int().numpy()
    B = len(LENS)
    c = (0.7 * torch.rand((B, N_TOK), generator=g)).float().numpy()
    if kind == "spread":
        gamma, beta, L = 2.0, 1.0, 3
        c[1, 0] = 0.95            # image 1: its CLS halts in layer 1 while its patch is live, a finished image from layer 2 on
        c[3, 0] = 0.6             # image 3: its CLS halts in layer 2 (see _layer_input) while patches are live
        c[4, 0] = 0.0             # image 4 keeps tokens to the last layer
        c[0, 0] = 0.1             # image 0 is its CLS alone and stays live
    elif kind == "all_halt":          # gamma = 0, h = sigmoid(10): everything halts in layer 1 by its score; layer 2 sees finished images only
        gamma, beta, L = 0.0, -10.0, 2
    else:                             # gamma = 0, h = sigmoid(-30): nothing halts in layer 1; layer 2 carries the last-layer flag
        gamma, beta, L = 0.0, 30.0, 2
    return dict(kind=kind, D=D, g=g, cu=cu, row_src=row_src, c=c, gamma=gamma, beta=beta, L=L, total=total)


def _layer_input(sc, rows, row_src, cu):
    """y [rows, D] fp32 of one layer; channel 0 shaped so that halting spreads and the CLS rows do what _scenario says"""
    y = torch.randn((rows, sc["D"]), generator=sc["g"]).float()
    y[:, 0] = 0.8 * y[:, 0]
    if sc["kind"] == "spread":
        for b, v in ((1, 0.5), (3, 0.1), (4, -1.5), (0, -1.0)):
            y[int(cu[b]), 0] = v
    return y.numpy()


def _raw_halt(y, cu, row_src, st, layer, last, gamma, beta, save=True):
    """d2s_avit_halt through lib.call on buffers with a poisoned guard band behind every output; st: device tensors, updated in place.
    -> dict of the outputs (device, guard included)"""
    from d2s import lib
    total, D = y.shape
    B, N = st["c"].shape

    def buf(n, dtype=torch.float32):
        return torch.full((n + GUARD,), POISON if dtype == torch.float32 else 12345, dtype=dtype, device=DEV)
    o = dict(h=buf(total), w=buf(B), ycls=buf(B * D), keep=buf(total), counts=buf(B, torch.int32), part=buf(B * 3))
    thr = float(np.float32(1.0) - np.float32(EPS))
    lib.call("d2s_avit_halt", lib.ptr(y), lib.ptr(cu), lib.ptr(row_src), lib.ptr(st["c"]), lib.ptr(st["R"]), lib.ptr(st["nh"]),
             lib.ptr(o["h"]) if save else None, lib.ptr(o["w"]), lib.ptr(st["acc"]), lib.ptr(o["ycls"]) if save else None,
             lib.ptr(st["ysave"]) if save else None, lib.ptr(o["keep"]), lib.ptr(o["counts"]), lib.ptr(o["part"]), B, N, D, total,
             int(layer), int(last), float(gamma), float(beta), thr)
    torch.cuda.synchronize()
    return o


def _dev_state(c, D):
    """device state with a guard band behind each array (views of padded buffers)"""
    B, N = c.shape
    pad = lambda n, dtype, fill: torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    raw = dict(c=pad(B * N, torch.float32, POISON), R=pad(B * N, torch.float32, POISON), nh=pad(B * N, torch.int32, 12345),
               acc=pad(B * D, torch.float32, POISON), ysave=pad(B * D, torch.float32, POISON))
    st = dict(c=raw["c"][:B * N].view(B, N), R=raw["R"][:B * N].view(B, N), nh=raw["nh"][:B * N].view(B, N),
              acc=raw["acc"][:B * D].view(B, D), ysave=raw["ysave"][:B * D].view(B, D))
    st["c"].copy_(torch.from_numpy(c))
    st["R"].zero_(), st["nh"].zero_(), st["ysave"].zero_()
    st["acc"].copy_(torch.randn((B, D), generator=torch.Generator().manual_seed(3)))
    return st, raw


def _guards_intact(bufs, sizes):
    for k, n in sizes.items():
        tail = bufs[k][n:]
        want = 12345 if tail.dtype == torch.int32 else POISON
        assert bool((tail == want).all()), f"guard band behind {k} was written"


def _run_sequence(kind, D, seed):
    """The scenario on the GPU and in float64, layer by layer.  -> per layer records for the backward test"""
    from d2s import ops
    sc = _scenario(kind, D, seed)
    B, L, gamma, beta = len(LENS), sc["L"], sc["gamma"], sc["beta"]
    st, raw = _dev_state(sc["c"], D)
    ref = dict(c=sc["c"].astype(np.float64), R=np.zeros((B, N_TOK)), nh=np.zeros((B, N_TOK), dtype=np.int64),
               acc=st["acc"].cpu().double().numpy().copy(), ysave=np.zeros((B, D)))
    cu, row_src = sc["cu"], sc["row_src"]
    records, parts = [], []
    ctol, acc_tol = np.zeros((B, N_TOK)), np.zeros((B, D))
    y = _layer_input(sc, sc["total"], row_src, cu)
    for layer in range(1, L + 1):
        last = layer == L
        total = y.shape[0]
        yd, cud, rsd = torch.from_numpy(y).to(DEV), torch.from_numpy(cu).to(DEV), torch.from_numpy(row_src).to(DEV)
        before = {k: v.clone() for k, v in st.items()}
        o = _raw_halt(yd, cud, rsd, st, layer, last, gamma, beta)
        # two launches are bit-equal: the same step again from the same state
        st2, _ = _dev_state(sc["c"], D)
        for k in st2:
            st2[k].copy_(before[k])
        o2 = _raw_halt(yd, cud, rsd, st2, layer, last, gamma, beta)
        for k in o:
            assert torch.equal(o[k], o2[k]), k
        for k in st:
            assert torch.equal(st[k], st2[k]), k
        _guards_intact(o, dict(h=total, w=B, ycls=B * D, keep=total, counts=B, part=B * 3))
        _guards_intact(raw, dict(c=B * N_TOK, R=B * N_TOK, nh=B * N_TOK, acc=B * D, ysave=B * D))
        r = R.halt_step(y, cu, row_src, ref, layer, last, gamma, beta, EPS)
        assert r["margin"] >= 1e-4, (kind, layer, r["margin"])               # the condition on the inputs: a decision is never a near tie
        h = o["h"][:total].cpu().double().numpy()
        z = np.abs(gamma * y[:, 0].astype(np.float64)) + abs(beta)
        tol_h = 8 * U * (r["h"] + r["h"] * (1 - r["h"]) * z)
        print(f"{kind} D={D} layer {layer}: rows {total}, counts {r['counts'].tolist()}, margin {r['margin']:.2e}")
        _frac("h", np.abs(h - r["h"]), tol_h)
        assert np.array_equal(o["keep"][:total].cpu().numpy(), r["keep"].astype(np.float32))
        assert np.array_equal(o["counts"][:B].cpu().numpy(), r["counts"])
        assert np.array_equal(st["nh"].cpu().numpy(), ref["nh"])
        assert np.array_equal(o["ycls"][:B * D].view(B, D).cpu().numpy(), r["ycls"].astype(np.float32))
        # per token: the state carries the tolerance of every h added so far and one rounding per addition (ctol, before this layer);
        # a remainder and a halting CLS weight are 1 - c with one more rounding
        tol_tok = np.zeros((B, N_TOK))
        for b in range(B):
            if ref["nh"][b, 0] == 0 or ref["nh"][b, 0] == layer:
                for rr in range(int(cu[b]), int(cu[b + 1])):
                    tol_tok[b, int(row_src[rr])] = tol_h[rr]
        ctol_before = ctol.copy()
        ctol += tol_tok + 2 * U * np.abs(ref["c"]) * (tol_tok > 0)
        _frac("c", np.abs(st["c"].cpu().double().numpy() - ref["c"]), ctol)
        _frac("R", np.abs(st["R"].cpu().double().numpy() - ref["R"]), (ctol_before + 2 * U * np.abs(ref["R"])) * (ref["nh"] > 0))
        tol_w = np.asarray([(ctol_before[b, 0] + 2 * U * abs(r["w"][b])) if ref["nh"][b, 0] == layer else tol_h[int(cu[b])] for b in range(B)])
        _frac("w", np.abs(o["w"][:B].cpu().double().numpy() - r["w"]), tol_w)
        acc_tol += tol_w[:, None] * np.abs(r["ycls"])
        _frac("acc", np.abs(st["acc"].cpu().double().numpy() - ref["acc"]), 8 * U * r["abs_acc"] + acc_tol)
        part = o["part"][:B * 3].view(B, 3).cpu().double().numpy()
        tol_rows = np.asarray([tol_h[int(cu[b]):int(cu[b + 1])].sum() for b in range(B)])
        _frac("part.h", np.abs(part[:, 0] - r["part"][:, 0]), 8 * U * r["abs_part"][:, 0] + tol_rows)
        assert np.array_equal(part[:, 1], r["part"][:, 1])
        _frac("part.rho", np.abs(part[:, 2] - r["part"][:, 2]), 8 * U * r["abs_part"][:, 2] + (ctol_before * (ref["nh"] == layer)).sum(axis=1))
        ys = st["ysave"].cpu().numpy()
        for b in range(B):
            if ref["nh"][b, 0] == layer:
                assert np.array_equal(ys[b], y[int(cu[b])])
        records.append(dict(layer=layer, y=y, cu=cu, row_src=row_src, h=o["h"][:total].clone(), w=o["w"][:B].clone(),
                            ycls=o["ycls"][:B * D].view(B, D).clone(), keep=o["keep"][:total].clone()))
        parts.append(o["part"][:B * 3].view(B, 3).clone())
        if last:
            break
        # the re-pack: GPU against plain indexing, then the next layer's input on the rows that go on
        cu_new = ops.ragged_offsets(o["counts"][:B].contiguous(), extra=1)
        y2, rs2, cu2 = R.repack(y, row_src, r["keep"], cu)
        assert cu_new.cpu().tolist() == cu2.tolist()
        xp, rsn = ops.ragged_repack(yd, o["keep"][:total].contiguous(), cud, cu_new, rsd, int(cu2[-1]), B)
        assert np.array_equal(xp.cpu().numpy(), y2) and np.array_equal(rsn.cpu().numpy(), rs2)
        cu, row_src = cu2, rs2
        y = _layer_input(sc, int(cu[-1]), row_src, cu)
    return sc, st, ref, records, torch.stack(parts)


@pytest.mark.parametrize("D", [128, 192, 384])
@pytest.mark.parametrize("kind", ["spread", "all_halt", "none_halt"])
def test_halting_step_and_backward_against_float64(kind, D):
    from d2s import lib, ops
    sc, st, ref, records, part = _run_sequence(kind, D, seed=SEEDS[D])
    B, L, gamma = len(LENS), sc["L"], sc["gamma"]
    nh = ref["nh"]
    if kind == "spread":
        assert nh[1, 0] == 1 and nh[3, 0] == 2 and nh[4, 0] == 3 and nh[0, 0] == 3          # finished early / CLS before its patches / to the end
        assert (nh[3, 1:][nh[3, 1:] > 0] <= 2).all() and (nh[4] == 3).any() and len(np.unique(nh[nh > 0])) == 3
    elif kind == "all_halt":
        assert (nh[nh > 0] == 1).all() and int((nh > 0).sum()) == sum(LENS) and records[1]["y"].shape[0] == B       # dead rows only
    else:
        assert int(records[0]["keep"].sum()) == sum(LENS) and (nh[nh > 0] == 2).all()          # nothing halts before the last-layer flag
    # ---- the penalty terms, forward and backward
    tgt = R.target(L, 1.0)
    out, hbar, cnt = ops.avit_penalty_fwd(part.contiguous(), tgt.float().to(DEV), N_TOK)
    out2, hbar2, _ = ops.avit_penalty_fwd(part.contiguous(), tgt.float().to(DEV), N_TOK)
    assert torch.equal(out, out2) and torch.equal(hbar, hbar2)
    p64 = part.cpu().double()
    nl = p64[:, :, 1].sum(1)
    hb = torch.where(nl > 0, p64[:, :, 0].sum(1) / nl.clamp(min=1), torch.zeros_like(nl))
    q = torch.clamp(hb / hb.sum(), 0.01, 0.99)
    P = R.prior(hb, tgt)
    rho = p64[:, :, 2].sum() / (B * N_TOK)
    assert torch.equal(cnt.cpu().double(), nl)
    _frac("hbar", (hbar.cpu().double() - hb).abs().numpy(), (8 * U * p64[:, :, 0].abs().sum(1) / nl.clamp(min=1)).numpy() + 1e-30)
    _frac("ponder", abs(float(out[0]) - float(rho)), 8 * U * float(p64[:, :, 2].abs().sum()) / (B * N_TOK))
    _frac("prior", abs(float(out[1]) - float(P)), 8 * U * float((tgt * (tgt.log().abs() + q.log().abs() + 8)).sum()) / L)
    dpn, dpr = torch.tensor([0.37], device=DEV), torch.tensor([-1.3], device=DEV)
    gsc = ops.avit_penalty_bwd(hbar, cnt, tgt.float().to(DEV), dpn, dpr, B, N_TOK)
    assert torch.equal(gsc, ops.avit_penalty_bwd(hbar, cnt, tgt.float().to(DEV), dpn, dpr, B, N_TOK))
    hbg = hb.clone().requires_grad_(True)
    (dP,) = torch.autograd.grad(R.prior(hbg, tgt), hbg)
    assert torch.allclose(dP, R.prior_grad_closed_form(hb, tgt), rtol=1e-9, atol=1e-14)
    S = hb.sum()
    a = torch.where((hb / S >= 0.01) & (hb / S <= 0.99), tgt / (L * (hb / S)), torch.zeros_like(hb))
    mag = (a / S + (a * hb).sum() / (S * S)) * 1.3 / nl.clamp(min=1)
    want = torch.cat((-1.3 * dP / nl.clamp(min=1) * (nl > 0), torch.tensor([0.37 / (B * N_TOK)], dtype=torch.float64)))
    _frac("gsc", (gsc.cpu().double() - want).abs().numpy(), np.concatenate(((32 * U * mag).numpy() + 1e-30, [4 * U * 0.37 / (B * N_TOK)])))
    # ---- the backward of every layer, on the GPU's own saved h / w / ycls / ysave
    g = torch.Generator().manual_seed(9)
    dacc = torch.randn((B, D), generator=g)
    gs = (0.01 * torch.randn(L + 1, generator=g)).float()
    dacc_d, gs_d = dacc.to(DEV), gs.to(DEV)
    for rec in reversed(records):
        layer, total = rec["layer"], rec["y"].shape[0]
        cud, rsd = torch.from_numpy(rec["cu"]).to(DEV), torch.from_numpy(rec["row_src"]).to(DEV)
        gin = None if layer == L else torch.randn((total, D), generator=g)
        got = []
        for _ in range(2):
            buf = torch.full((total * D + GUARD,), POISON, device=DEV)
            view = buf[:total * D].view(total, D)
            if gin is not None:
                view.copy_(gin)
            lib.call("d2s_avit_halt_bwd", lib.ptr(buf), lib.ptr(rec["h"]), lib.ptr(cud), lib.ptr(rsd), lib.ptr(st["nh"]), lib.ptr(rec["w"]),
                     lib.ptr(dacc_d), lib.ptr(rec["ycls"]), lib.ptr(st["ysave"]), lib.ptr(gs_d), B, N_TOK, D, total, layer, L,
                     int(gin is None), float(gamma))
            torch.cuda.synchronize()
            assert bool((buf[total * D:] == POISON).all())
            got.append(view.clone())
        assert torch.equal(got[0], got[1])
        want_g, ab = R.halt_step_bwd(np.zeros((total, D)) if gin is None else gin.double().numpy(), rec["h"].cpu().double().numpy(), rec["cu"],
                                     rec["row_src"], ref["nh"], rec["w"].cpu().double().numpy(), dacc.double().numpy(),
                                     rec["ycls"].cpu().double().numpy(), st["ysave"].cpu().double().numpy(), gs.double().numpy(), layer, gamma)
        assert not bool(torch.isnan(got[0]).any()) and not bool((got[0] == POISON).any())       # fresh: every element written
        _frac("g_y", np.abs(got[0].cpu().double().numpy() - want_g), 8 * U * ab + 1e-30)
        wrapped = ops.avit_halt_bwd(None if gin is None else gin.to(DEV).clone(), rec["h"], cud, rsd, st, rec["w"], dacc_d, rec["ycls"], gs_d, layer,
                                    gamma)
        assert torch.equal(wrapped, got[0])


def test_refusals_leave_poisoned_outputs_untouched():
    from d2s import lib
    lib.load()
    B, N, D, total, L = 2, 5, 8, 6, 3
    f = lambda n: torch.full((n,), POISON, device=DEV)
    i = lambda n: torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    y, cu, rs = f(total * D), torch.tensor([0, 3, 6], dtype=torch.int32, device=DEV), torch.tensor([0, 1, 2, 0, 3, 4], dtype=torch.int32, device=DEV)
    c, Rm, nh, h, w, acc, ycls, ysave, keep, counts, part = f(B * N), f(B * N), i(B * N), f(total), f(B), f(B * D), f(B * D), f(B * D), f(total), i(B), f(B * 3)
    outs = [c, Rm, nh, h, w, acc, ycls, ysave, keep, counts, part]
    P = lib.ptr
    good = [P(y), P(cu), P(rs), P(c), P(Rm), P(nh), P(h), P(w), P(acc), P(ycls), P(ysave), P(keep), P(counts), P(part), B, N, D, total, 1, 0,
            1.0, 0.0, 0.99]
    fn, st = lib._fn("d2s_avit_halt"), lib.stream()
    for pos, val in [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, None), (11, None), (12, None), (13, None),
                     (14, 0), (15, 0), (16, 0), (17, 0), (18, 0), (19, 2)]:
        a = list(good)
        a[pos] = val
        assert fn(*a, st) == -1, pos
    g, dacc, gsc = f(total * D), f(B * D), f(L + 1)
    goodb = [P(g), P(h), P(cu), P(rs), P(nh), P(w), P(dacc), P(ycls), P(ysave), P(gsc), B, N, D, total, 1, L, 0, 1.0]
    fb = lib._fn("d2s_avit_halt_bwd")
    for pos, val in [(k, None) for k in range(10)] + [(10, 0), (11, 0), (12, 0), (13, 0), (14, 0), (14, L + 1), (15, 65), (16, 2)]:
        a = list(goodb)
        a[pos] = val
        assert fb(*a, st) == -1, pos
    out, hbar, cnt, tgt = f(2), f(L), f(L), f(L)
    fp = lib._fn("d2s_avit_penalty_fwd")
    goodp = [P(part), P(tgt), P(out), P(hbar), P(cnt), L, B, N]
    for pos, val in [(k, None) for k in range(5)] + [(5, 0), (5, 65), (6, 0), (7, 0)]:
        a = list(goodp)
        a[pos] = val
        assert fp(*a, st) == -1, pos
    fq = lib._fn("d2s_avit_penalty_bwd")
    goodq = [P(hbar), P(cnt), P(tgt), P(out), P(out), P(gsc), L, B, N]
    for pos, val in [(k, None) for k in range(6)] + [(6, 0), (6, 65), (7, 0), (8, 0)]:
        a = list(goodq)
        a[pos] = val
        assert fq(*a, st) == -1, pos
    torch.cuda.synchronize()
    for t in outs + [g, out, hbar, cnt, gsc]:
        assert bool((t == (12345 if t.dtype == torch.int32 else POISON)).all())


# ---- 2. the model, micro geometry ----
_GEOM = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


def _model(name, **kw):
    import vit_models
    sd = built(name)[0]
    c = AVIT_CASES[name]
    m = vit_models.VisionTransformerAViT(**_GEOM, gate_scale=c["gamma"], gate_center=c["beta"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV)


def _rows_per_layer(n):
    """[L][B]: the rows of every image in every block, from halting layers [B, N]: its live tokens, or its dead CLS row"""
    L = CFG["depth"]
    return [[int((n[b] > l - 1).sum()) if int(n[b, 0]) > l - 1 else 1 for b in range(n.shape[0])] for l in range(1, L + 1)]


TOL = {"exact": (1e-4, 2e-5), "split": (1e-4, 2e-5), "bf16": (3e-2, 3e-2)}     # tests/test_ats_gpu.py's, per arithmetic mode


@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_model_forward_against_float64(name, mode):
    from d2s import ops
    sd, images, _, out = built(name)
    c = AVIT_CASES[name]
    check_condition(out, CFG["depth"])
    m = _model(name).eval()
    gm = {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}[mode]
    with ops.gemm_mode(gm), torch.no_grad():
        logits = m(images.to(DEV))
        n = m.halt_layer.cpu().long()
        per_layer, counts, depth = list(m.tokens_per_layer), m.tokens_per_layer_counts.tolist(), float(m.avg_depth)
        pen = (float(m.ponder_loss), float(m.prior_loss))
        alone = []
        for b in range(images.shape[0]):
            alone.append(m(images[b:b + 1].to(DEV)))
            if mode != "bf16":
                assert torch.equal(m.halt_layer.cpu().long()[0], n[b])
    if mode != "bf16":
        assert torch.equal(n, out["n"])                                     # the halting layers, exactly
        ref = out
    else:                                                                   # bf16 noise may move a decision: the GPU's own are replayed
        print(f"  bf16: {int((n != out['n']).sum())} of {n.numel()} halting layers differ from the float64 decisions")
        with torch.no_grad():
            ref = R.forward({k: v.double() for k, v in sd.items()}, images, CFG, c["gamma"], c["beta"], EPS, n_forced=n)
    assert counts == _rows_per_layer(n) and per_layer == [sum(r) for r in counts]
    assert abs(depth - float(n.double().mean())) < 1e-5
    print(f"{name} {mode}: tokens per layer {per_layer}, CLS halts at {n[:, 0].tolist()}, "
          f"max |logits - ref| {float((logits.cpu().double() - ref['logits']).abs().max()):.3e}")
    tol = TOL[mode]
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"].numpy(), rtol=tol[0], atol=tol[1])
    np.testing.assert_allclose(torch.cat(alone).cpu().numpy(), logits.cpu().numpy(), rtol=tol[0], atol=tol[1])     # cu indexing
    tgt = R.target(CFG["depth"], m.target_depth)
    np.testing.assert_allclose(pen[0], float(R.ponder(ref)), rtol=tol[0])
    np.testing.assert_allclose(pen[1], float(R.prior(R.hbar(ref), tgt)), rtol=max(tol[0], 1e-4), atol=tol[1])


PEN = dict(avit_ponder_scale=5e-2, avit_prior_alpha=0.3)       # larger than the defaults so that the penalty gradients are visible


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_model_gradients_and_loss_against_float64(name, mode):
    from d2s import ops
    from losses import AViTLoss
    sd, images, labels, _ = built(name)
    c = AVIT_CASES[name]
    m = _model(name, target_depth=2.0).train()
    fn = AViTLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, **PEN))
    gm = {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[mode]
    with ops.gemm_mode(gm):
        logits = m(images.to(DEV))
        loss = fn(logits, None, labels.to(DEV), {}, m.ponder_loss, m.prior_loss, m.avg_depth)
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    out = R.forward(sd64, images, CFG, c["gamma"], c["beta"], EPS)
    want, terms = R.objective(out, labels, ponder_scale=PEN["avit_ponder_scale"], prior_alpha=PEN["avit_prior_alpha"], target_depth=2.0)
    names = list(sd64)
    grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
    assert torch.equal(m.halt_layer.cpu().long(), out["n"])
    print(f"{name} {mode}: loss {float(loss.detach()):.7f} float64 {float(want.detach()):.7f} (ponder {float(terms['ponder'].detach()):.4f}, prior {float(terms['prior'].detach()):.4f})")
    np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4)
    worst = 0.0
    for k, p in m.named_parameters():
        ref = grads[k]
        assert p.grad is not None and ref is not None, k
        rel = float((p.grad.detach().cpu().double() - ref).norm() / ref.norm())
        worst = max(worst, rel)
        assert rel <= 1e-3, (k, rel)
    print(f"  worst relative L2 error of a parameter gradient {worst:.2e}")
    # a bf16 training forward is RaggedBlockFn's own refusal
    from d2s.lib import D2SError
    with ops.gemm_mode(ops.GEMM_BF16), pytest.raises(D2SError, match="fp32 arithmetic modes"):
        m(images.to(DEV))


def test_training_forward_is_the_eval_forward():
    _, images, _, _ = built("avit1")
    m = _model("avit1")
    x = images.to(DEV)
    a = m.train()(x)
    n = m.halt_layer.clone()
    with torch.no_grad():
        b = m.eval()(x)
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), b) and torch.equal(n, m.halt_layer) and a.requires_grad and not b.requires_grad


# ---- 3. TrainStep ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **PEN, **kw)


def _step(with_teacher=False, student=None, **kw):
    import vit_models
    from d2s.engine import TrainStep
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**_GEOM)
        teacher.load_state_dict(built("avit1")[0])
        teacher = teacher.to(DEV)
    student = _model("avit1", target_depth=2.0) if student is None else student
    return TrainStep(student, teacher, _args(), lr=1e-3, **kw)


def _xy():
    _, images, labels, _ = built("avit1")
    return images.to(DEV), labels.to(DEV)


@pytest.mark.parametrize("with_teacher", [False, True])
def test_train_step_two_runs_bit_identical_and_resume(with_teacher):
    from d2s import lib
    x, y = _xy()
    runs = []
    for _ in range(2):
        ts = _step(with_teacher)
        assert ts.method.name == "avit" and ts.logits_only and ts.graph is False
        losses = [float(ts(x, y)["loss"]) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((losses, ts.arena.params.clone(), ts))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert all(math.isfinite(v) for v in runs[0][0])
    ts = runs[1][2]
    for k in ("train_avit_loss", "train_cls_loss", "train_ponder_loss", "train_prior_loss", "train_avg_depth"):
        assert k in ts.metrics and math.isfinite(float(ts.metrics[k])), k
    assert 1.0 <= float(ts.metrics["train_avg_depth"]) <= CFG["depth"]
    saved = ts.state_dict()
    cfg = saved["config"]
    c = AVIT_CASES["avit1"]
    assert (cfg["model"], cfg["avit_gate_scale"], cfg["avit_gate_center"], cfg["avit_eps_halt"]) == ("VisionTransformerAViT", c["gamma"], c["beta"], EPS)
    ts(x, y)
    torch.cuda.synchronize()
    three = ts.arena.params.clone()
    resumed = _step(with_teacher)
    assert resumed.load_state_dict(saved) == saved["epoch"]
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three)                          # 2 steps, a checkpoint, 1 more step = 3 straight steps
    import vit_models
    other = vit_models.VisionTransformerAViT(**_GEOM, gate_scale=c["gamma"], gate_center=c["beta"] + 1.0).to(DEV)
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: avit_gate_center"):
        _step(with_teacher, student=other).load_state_dict(saved)
    dense = vit_models.VisionTransformerATS(**_GEOM, ats_locs=[1], ats_tokens=4, train_sample=True).to(DEV)
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: model"):
        _step(with_teacher, student=dense).load_state_dict(saved)


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


def test_train_step_refusals_by_message():
    from d2s import lib
    from d2s.engine import TrainStep
    m = _model("avit1")
    with pytest.raises(ValueError, match="warmup_steps 2 with an A-ViT student"):
        TrainStep(m, None, _args(), warmup_steps=2)
    with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an A-ViT student"):
        TrainStep(m, None, _args(), graph=True)
    m.drop_path_rate = 0.1
    with pytest.raises(lib.D2SError, match="A-ViT student and drop_path_rate > 0"):
        TrainStep(m, None, _args())


# ---- 4. command line ----
def test_cli_trains_one_tiny_epoch(tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    acc = mask_predictor.main(["--arch", "deit_tiny", "--method", "avit", "--avit-gate-scale", "4", "--avit-gate-center", "1", "--epochs", "1",
                               "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4", "--student-checkpoint", path,
                               "--dist-weight", "0", "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Start training" in out and "--method avit: tokens per layer [" in out and "val loss:" in out and "train_avg_depth=" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert (cfg["model"], cfg["avit_gate_scale"], cfg["avit_gate_center"]) == ("VisionTransformerAViT", 4.0, 1.0)
