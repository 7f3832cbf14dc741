"""The LTP kernels on the GPU against the float64 loops of tests/ltp_ref.py.
The score (csrc/ltp.hip on the f32-input matrix pipe), its three forms fed with the lse / cinv the attention forward of the same qkv wrote:
rtol 1e-5 against float64 - the project's rule for the ATS score, a product of the same probabilities - every image's sum within 1e-5 of 1,
the policy form with an all-ones policy and eps = 0 and the varlen form on equal lengths bit for bit the plain form, two launches bit for
bit, NaN-filled outputs with a guard band, a cu_seqlens of garbage, every refusal with poisoned outputs untouched.
The decision and the soft mask: keep / counts exactly (score == theta included), M, m, gM, gm, dtheta within 8 * 2^-24 * sum |summands|.
The model in the micro geometry against the dense masked float64 restatement: the hard phase in the exact and the split mode (kept sets and
rows per block exactly, logits with the GPU's decisions replayed, every image alone, theta = 0 against the dense trunk, the all-CLS case,
loss and every parameter gradient, no gradient on the thresholds), the soft phase (loss, every parameter gradient, dtheta), TrainStep in
both phases (bit-identical runs, save and resume, the refused phase, accumulation with clipping, the soft-to-hard hand-over) and the
command line."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import ltp_ref as R
from tests.test_ltp_cpu import CFG, LOCS, LTP_CASES, MICRO, PRUNING, SCALE, SOFT, built, check_condition, make_policy, make_qkv, soft_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
GUARD, POISON = 64, 1234.5
LENS = [1, 2, 17, 33, 197]
EPS = 1e-6
WORST = {}
_REF = {}


def _note(tag, v):
    WORST[tag] = max(WORST.get(tag, 0.0), float(v))
    print(f"  {tag}: {float(v):.3e} (worst over the tests so far {WORST[tag]:.3e})")


def _rel(tag, got, ref, rtol=1e-5):
    """|got - ref| <= rtol |ref| elementwise against float64; the worst relative error is printed before the assertion"""
    got, ref = got.double().cpu(), ref.double()
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    _note(tag, err)
    assert bool(torch.isfinite(got).all()) and float(err) <= rtol, (tag, float(err))


def _frac(tag, err, bound):
    """err <= bound elementwise; the worst observed fraction of the bound is printed before the assertion"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    f = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    _note(tag + " (fraction of the bound)", f)
    assert f <= 1.0, (tag, f)


def _dense_case(B, n, H):
    """(qkv float64 on the fp32 grid, float64 plain score), computed once per shape"""
    key = (B, n, H)
    if key not in _REF:
        qkv = make_qkv(B * n, H, 1000 * n + 10 * H + B)
        _REF[key] = (qkv, R.score_plain(qkv, B, n, H, SCALE))
    return _REF[key]


def _attn_fwd(qkv, B, n, H):
    """the dense fp32 attention forward, whatever arithmetic mode the process is in -> lse [B, H, n]"""
    from d2s import lib
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=DEV)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=DEV)
    lib.call("d2s_attn_fwd_f32", lib.ptr(qkv), lib.ptr(out), lib.ptr(lse), None, B, n, H, SCALE)
    return lse


def _dev_qkv(qkv64):
    return qkv64.float().reshape(qkv64.shape[0], -1).contiguous().to(DEV)


# ---- 1. the score, dense forms ----
@pytest.mark.parametrize("H", [1, 2, 6])
@pytest.mark.parametrize("n", [2, 31, 32, 33, 65, 197])
@pytest.mark.parametrize("B", [1, 3])
def test_score_dense_forms(B, n, H):
    from d2s import ops
    qkv64, ref = _dense_case(B, n, H)
    qkv = _dev_qkv(qkv64)
    lse = _attn_fwd(qkv, B, n, H)
    s = ops.ltp_score(qkv, lse, B, n, H, SCALE)
    _rel("score plain", s.reshape(B, n), ref)
    _note("score plain |sum - 1|", (s.double().reshape(B, n).sum(dim=1) - 1.0).abs().max())
    assert float((s.double().reshape(B, n).sum(dim=1) - 1.0).abs().max()) <= 1e-5
    assert torch.equal(ops.ltp_score(qkv, lse, B, n, H, SCALE), s)                                  # two launches
    # all-ones policy, eps = 0: lse and cinv from the policy attention itself; bit for bit the plain form
    ones = torch.ones((B, n), dtype=torch.float32, device=DEV)
    _, lse1, cinv1, _ = ops.attn_policy_fwd(qkv, ones, B, n, H, SCALE, eps=0.0)
    assert torch.equal(ops.ltp_score(qkv, lse1, B, n, H, SCALE, policy=ones, cinv=cinv1), s)
    # varlen on equal lengths: bit for bit the plain form, with max_n an upper bound only
    cu = (torch.arange(B + 1, dtype=torch.int32) * n).to(DEV)
    _, lse_v, _ = ops.attn_varlen_fwd_lse(qkv, cu, B, B * n, n + 7, H, SCALE)
    assert torch.equal(ops.ltp_score(qkv, lse_v, B, n + 7, H, SCALE, cu=cu, total=B * n), s)
    # policies with exact 0, exact 1 and values in between, and only CLS kept
    for kind in ("mixed", "cls_only"):
        pol64 = make_policy(kind, B, n, 3 * n + H)
        pol = pol64.float().to(DEV)
        _, lse_p, cinv_p, _ = ops.attn_policy_fwd(qkv, pol, B, n, H, SCALE, eps=EPS)
        sp = ops.ltp_score(qkv, lse_p, B, n, H, SCALE, policy=pol, cinv=cinv_p)
        _rel(f"score policy {kind}", sp.reshape(B, n), R.score_policy(qkv64, pol64, B, n, H, SCALE, EPS))
        assert float((sp.double().reshape(B, n).sum(dim=1) - 1.0).abs().max()) <= 1e-5
        assert torch.equal(ops.ltp_score(qkv, lse_p, B, n, H, SCALE, policy=pol, cinv=cinv_p), sp)


# ---- 2. the score, ragged ----
@pytest.mark.parametrize("H", [1, 2, 6])
def test_score_varlen(H):
    from d2s import ops
    B, total = len(LENS), sum(LENS)
    qkv64 = make_qkv(total, H, 77 + H)
    qkv = _dev_qkv(qkv64)
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=DEV)
    _, lse, _ = ops.attn_varlen_fwd_lse(qkv, cu, B, total, 300, H, SCALE)
    s = ops.ltp_score(qkv, lse, B, 300, H, SCALE, cu=cu, total=total)
    _rel("score varlen", s, R.score_varlen(qkv64, LENS, H, SCALE))
    assert torch.equal(ops.ltp_score(qkv, lse, B, 300, H, SCALE, cu=cu, total=total), s)
    assert float(s[0]) == 1.0                                    # an image that is its CLS row alone
    r0 = 0
    for n in LENS:                                               # every image alone, as a dense batch of one: the same bits
        assert abs(float(s[r0:r0 + n].double().sum()) - 1.0) <= 1e-5
        one = qkv[r0:r0 + n].contiguous()
        assert torch.equal(ops.ltp_score(one, _attn_fwd(one, 1, n, H), 1, n, H, SCALE), s[r0:r0 + n])
        r0 += n


# ---- 3. raw calls: guard bands, NaN-filled outputs, a cu_seqlens of garbage, refusals ----
def _raw_score(qkv, lse, B, n, total, H, policy=None, cinv=None, cu=None, ws_floats=None, fill=float("nan")):
    from d2s import lib
    need = lib.query("d2s_ltp_score_workspace_bytes", total, H)
    ws_floats = need // 4 if ws_floats is None else ws_floats
    score = torch.full((total + GUARD,), fill, dtype=torch.float32, device=DEV)
    score[total:] = POISON
    ws = torch.full((ws_floats + GUARD,), POISON, dtype=torch.float32, device=DEV)
    rc = lib._fn("d2s_ltp_score_f32")(lib.ptr(qkv), lib.ptr(lse), lib.ptr(policy), lib.ptr(cinv), lib.ptr(cu), lib.ptr(score), lib.ptr(ws),
                                      ws_floats * 4, B, n, total, H, SCALE, lib.stream())
    torch.cuda.synchronize()
    return rc, score, ws, ws_floats


def test_score_writes_every_row_and_nothing_else():
    from d2s import ops
    B, n, H = 3, 33, 2
    qkv = _dev_qkv(_dense_case(B, n, H)[0])
    lse = _attn_fwd(qkv, B, n, H)
    rc, score, ws, wf = _raw_score(qkv, lse, B, n, B * n, H)
    assert rc == 0 and bool(torch.isfinite(score[:B * n]).all()) and torch.equal(score[:B * n], ops.ltp_score(qkv, lse, B, n, H, SCALE))
    assert bool((score[B * n:] == POISON).all()) and bool((ws[wf:] == POISON).all()) and bool((ws[:wf] != POISON).all())
    total = sum(LENS)
    qkv = _dev_qkv(make_qkv(total, H, 5))
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=DEV)
    _, lse, _ = ops.attn_varlen_fwd_lse(qkv, cu, len(LENS), total, 197, H, SCALE)
    rc, score, ws, wf = _raw_score(qkv, lse, len(LENS), 256, total, H, cu=cu)
    assert rc == 0 and bool(torch.isfinite(score[:total]).all()) and bool((score[total:] == POISON).all()) and bool((ws[wf:] == POISON).all())


def test_score_clamps_a_cu_seqlens_of_garbage():
    """segments are clamped to [0, total) and to max_n rows: whatever cu_seqlens holds, only score [total] and the workspace are written"""
    H, total = 2, 100
    qkv = _dev_qkv(make_qkv(total, H, 6))
    lse = torch.zeros((H, total), dtype=torch.float32, device=DEV)
    for vals in ([-50, 20, 10, 400, 2 ** 31 - 1], [0, 0, 0, 0, 0], [90, 300, -7, 64, 100]):
        cu = torch.tensor(vals, dtype=torch.int32, device=DEV)
        rc, score, ws, wf = _raw_score(qkv, lse, 4, 64, total, H, cu=cu, fill=POISON)
        assert rc == 0 and bool((score[total:] == POISON).all()) and bool((ws[wf:] == POISON).all())


def test_score_refusals_leave_the_outputs_alone():
    from d2s import lib
    B, n, H = 2, 17, 2
    total = B * n
    qkv = _dev_qkv(make_qkv(total, H, 8))
    lse = torch.zeros((B, H, n), dtype=torch.float32, device=DEV)
    pol = torch.ones((B, n), dtype=torch.float32, device=DEV)
    cu = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=DEV)
    need = lib.query("d2s_ltp_score_workspace_bytes", total, H)
    score = torch.full((total,), POISON, dtype=torch.float32, device=DEV)
    ws = torch.full((need // 4,), POISON, dtype=torch.float32, device=DEV)
    good = dict(qkv=qkv, lse=lse, policy=None, cinv=None, cu=None, score=score, ws=ws, wsb=need, B=B, n=n, total=total, H=H)
    bad = [dict(qkv=None), dict(lse=None), dict(score=None), dict(B=0), dict(n=0), dict(n=8193), dict(total=0), dict(H=0),
           dict(policy=pol), dict(cinv=lse), dict(policy=pol, cinv=lse, cu=cu), dict(total=total + 1), dict(n=n + 1)]
    for change in bad + [dict(ws=None), dict(wsb=need - 4)]:
        a = dict(good, **change)
        rc = lib._fn("d2s_ltp_score_f32")(lib.ptr(a["qkv"]), lib.ptr(a["lse"]), lib.ptr(a["policy"]), lib.ptr(a["cinv"]), lib.ptr(a["cu"]),
                                          lib.ptr(a["score"]), lib.ptr(a["ws"]), a["wsb"], a["B"], a["n"], a["total"], a["H"], SCALE, lib.stream())
        assert rc == (-2 if ("ws" in change or "wsb" in change) else -1), (change.keys(), rc)
    torch.cuda.synchronize()
    assert bool((score == POISON).all()) and bool((ws == POISON).all())
    # the other three entries
    keep = torch.full((total,), POISON, dtype=torch.float32, device=DEV)
    counts = torch.full((B,), 12345, dtype=torch.int32, device=DEV)
    th = torch.zeros((1,), dtype=torch.float32, device=DEV)
    sel = lib._fn("d2s_ltp_select")
    P = lib.ptr
    for args in [(None, P(cu), None, P(th), P(keep), P(counts), None, B, 0, total), (P(score), None, None, P(th), P(keep), P(counts), None, B, 0, total),
                 (P(score), P(cu), None, None, P(keep), P(counts), None, B, 0, total), (P(score), P(cu), None, P(th), None, P(counts), None, B, 0, total),
                 (P(score), P(cu), None, P(th), P(keep), None, None, B, 0, total), (P(score), P(cu), None, P(th), P(keep), P(counts), None, 0, 0, total),
                 (P(score), P(cu), None, P(th), P(keep), P(counts), None, B, 0, 0), (P(score), P(cu), None, P(th), P(keep), P(counts), P(ws), B, 16, total)]:
        assert sel(*args, lib.stream()) == -1
    M = torch.full((B, n), POISON, dtype=torch.float32, device=DEV)
    msum = torch.full((B,), POISON, dtype=torch.float32, device=DEV)
    fwd, bwd = lib._fn("d2s_ltp_soft_mask_fwd"), lib._fn("d2s_ltp_soft_mask_bwd")
    for args in [(None, None, P(th), P(M), P(keep), P(msum), B, n, 1.0), (P(pol), None, None, P(M), P(keep), P(msum), B, n, 1.0),
                 (P(pol), None, P(th), None, P(keep), P(msum), B, n, 1.0), (P(pol), None, P(th), P(M), None, P(msum), B, n, 1.0),
                 (P(pol), None, P(th), P(M), P(keep), None, B, n, 1.0), (P(pol), None, P(th), P(M), P(keep), P(msum), 0, n, 1.0),
                 (P(pol), None, P(th), P(M), P(keep), P(msum), B, 1, 1.0), (P(pol), None, P(th), P(M), P(keep), P(msum), B, n, 0.0),
                 (P(pol), None, P(th), P(M), P(keep), P(msum), B, n, float("nan"))]:
        assert fwd(*args, lib.stream()) == -1
    dth = torch.full((1,), POISON, dtype=torch.float32, device=DEV)
    ok = [P(pol), P(pol), None, None, P(M), None, P(dth), P(msum), B, n, 1.0, 0, 0]
    for i, v in [(0, None), (1, None), (4, None), (6, None), (7, None), (8, 0), (9, 1), (10, 0.0), (10, -1.0), (11, 2), (12, -1)]:
        args = list(ok)
        args[i] = v
        assert bwd(*args, lib.stream()) == -1, i
    torch.cuda.synchronize()
    assert bool((keep == POISON).all()) and bool((counts == 12345).all()) and bool((M == POISON).all()) and bool((msum == POISON).all())
    assert float(dth) == POISON


# ---- 4. the decision ----
def test_select_exact_with_scores_on_the_threshold():
    from d2s import ops
    B, total, T = len(LENS), sum(LENS), 196
    g = torch.Generator().manual_seed(9)
    score = (torch.rand((total,), generator=g) * 0.01).float()
    theta = float(np.float32(0.005))
    score[[3, 25, 60, 200]] = theta                       # deliberate equality: kept
    score[[4, 26]] = float(np.nextafter(np.float32(theta), np.float32(0)))      # one ulp below: dropped
    score[[0, 1, 3 + 17]] = 0.0                           # CLS rows (0, 1, 3, 20, 53) are kept whatever their score
    row_src = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), torch.sort(torch.randperm(T, generator=g)[:n - 1])[0] + 1))
                         for n in LENS]).int()
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32)
    for th in (theta, 0.0, 1.0):
        want_keep, want_counts = R.select(score.double(), LENS, float(np.float32(th)))
        k, c, dense = ops.ltp_select(score.to(DEV), cu.to(DEV), torch.tensor([th], dtype=torch.float32, device=DEV), B,
                                     row_src=row_src.to(DEV), T=T)
        assert torch.equal(k.cpu().double(), want_keep) and c.cpu().tolist() == want_counts, th
        want_dense = torch.zeros((B, T))
        r0 = 0
        for b, n in enumerate(LENS):
            for r in range(r0 + 1, r0 + n):
                if want_keep[r]:
                    want_dense[b, int(row_src[r]) - 1] = 1.0
            r0 += n
        assert torch.equal(dense.cpu(), want_dense), th
        if th == 1.0:
            assert c.cpu().tolist() == [0] * B
        if th == 0.0:
            assert c.cpu().tolist() == [n - 1 for n in LENS]
        k2, c2, none = ops.ltp_select(score.to(DEV), cu.to(DEV), torch.tensor([th], dtype=torch.float32, device=DEV), B)
        assert none is None and torch.equal(k2, k) and torch.equal(c2, c)
    # garbage in cu_seqlens: clamped, nothing outside keep [total] and counts [B] is written
    from d2s import lib
    keep = torch.full((total + GUARD,), POISON, dtype=torch.float32, device=DEV)
    counts = torch.full((B + GUARD,), 12345, dtype=torch.int32, device=DEV)
    bad = torch.tensor([-5, 40, 20, 2 ** 31 - 1, 3, total + 9], dtype=torch.int32, device=DEV)
    th = torch.tensor([theta], dtype=torch.float32, device=DEV)
    lib.call("d2s_ltp_select", lib.ptr(score.to(DEV)), lib.ptr(bad), None, lib.ptr(th), lib.ptr(keep), lib.ptr(counts), None, B, 0, total)
    torch.cuda.synchronize()
    assert bool((keep[total:] == POISON).all()) and bool((counts[B:] == 12345).all())


# ---- 5. the soft mask ----
@pytest.mark.parametrize("B,N,seed", [(4, 17, 1), (3, 197, 2), (2, 300, 3)])
def test_soft_mask_forward_and_backward(B, N, seed):
    """The bounds count roundings, 8 of them allowed per output (u = 2^-24).  M: the sigmoid's own (relative to M) plus those of its
    argument z = (s - theta) / tau, which reach M through dM/dz = M (1 - M) with |z| <= (|s| + |theta|) / tau.  m = m_in M inherits M's and
    adds its own; the sums take 8 u of the sum of the magnitudes of what they add; gM's summands are g m_in and the regulariser's share."""
    from d2s import ops
    c = soft_case(B, N, seed)
    tau, lam = c["tau"], c["lam"]
    g = torch.Generator().manual_seed(seed + 50)
    th32 = np.float32(c["theta"][1])
    theta = torch.tensor([th32], dtype=torch.float32, device=DEV)
    score, m_in = c["score"][1], torch.rand((B, N), generator=g, dtype=torch.float64).float().double()
    m_in[:, 0] = 1.0
    score[0, 3] = float(th32)                               # M = 1/2 exactly
    M64, m64, msum64 = R.soft_mask(score, m_in, float(th32), tau)
    for mi in (m_in, None):
        M, m_out, msum = ops.ltp_soft_mask_fwd(score.float().to(DEV), None if mi is None else mi.float().to(DEV), theta, tau)
        bM = 8 * U * (M64 + M64 * (1 - M64) * (score.abs() + float(th32)) / tau)
        _frac("M", (M.cpu().double() - M64).abs(), bM)
        assert bool((M[:, 0] == 1.0).all()) and float(M[0, 3]) == 0.5
        mref = m64 if mi is not None else M64
        _frac("m_out", (m_out.cpu().double() - mref).abs(), (1.0 if mi is None else mi) * bM + 8 * U * mref)
        _frac("msum", (msum.cpu().double() - msum64).abs(), bM[:, 1:].sum(dim=1) + 8 * U * msum64)
    # backward, on the kernel's own M (an input of the backward)
    M32 = M.cpu()
    g_out = torch.randn((B, N), generator=g, dtype=torch.float64).float().double() + 0.3
    share = lam / (c["S"] * B * (N - 1))                     # the regulariser's share; per image here, to show nothing assumes it uniform
    gr = (share * (1.0 + torch.arange(B, dtype=torch.float64))).float().double().reshape(B, 1)
    greg = gr.float().reshape(B).to(DEV)
    gM64, gm64, dth64, _ = R.soft_mask_bwd(g_out, M32.double(), m_in, tau, gr)
    dth = torch.full((1,), POISON, dtype=torch.float32, device=DEV)
    gM, gm = ops.ltp_soft_mask_bwd(g_out.float().to(DEV), M, m_in.float().to(DEV), tau, dth, greg=greg)
    mag_gM = (g_out * m_in).abs() + gr
    _frac("gM", (gM.cpu().double() - gM64).abs()[:, 1:], 8 * U * mag_gM[:, 1:])
    assert bool((gM[:, 0] == 0.0).all())
    _frac("gm", (gm.cpu().double() - gm64).abs(), 8 * U * gm64.abs())
    mag_dth = float((mag_gM * M32.double() * (1 - M32.double()))[:, 1:].sum() / tau)
    print(f"  dtheta {float(dth):.6e} float64 {float(dth64):.6e} sum |summands| {mag_dth:.3e}")
    _frac("dtheta", abs(float(dth) - float(dth64)), 8 * U * mag_dth)
    assert abs(float(dth64)) >= 1e-2 * mag_dth                           # the case is no cancellation
    # the accumulating forms: gm_in and dtheta are added to what they hold; two launches bit-equal
    dth2 = dth.clone()
    prev = torch.randn((B, N), generator=g).float()
    gm_acc = prev.clone().to(DEV)
    gM2, gm2 = ops.ltp_soft_mask_bwd(g_out.float().to(DEV), M, m_in.float().to(DEV), tau, dth2, greg=greg, gm_in=gm_acc,
                                     accumulate_dtheta=True)
    assert torch.equal(gM2, gM) and gm2 is gm_acc
    _frac("gm accumulated", (gm_acc.cpu().double() - (prev.double() + gm64)).abs(), 8 * U * (prev.double().abs() + gm64.abs()))
    _frac("dtheta accumulated", abs(float(dth2) - 2.0 * float(dth64)), 8 * U * 2.0 * mag_dth)
    # the first stage: no incoming policy, no regulariser share, no gm wanted
    dth3 = torch.full((1,), POISON, dtype=torch.float32, device=DEV)
    gM3, none = ops.ltp_soft_mask_bwd(g_out.float().to(DEV), M, None, tau, dth3, want_gm=False)
    g3, _, d3, mag3 = R.soft_mask_bwd(g_out, M32.double(), torch.ones_like(m_in), tau, 0.0)
    assert none is None
    _frac("gM first stage", (gM3.cpu().double() - g3).abs(), 8 * U * g_out.abs())
    _frac("dtheta first stage", abs(float(dth3) - float(d3)), 8 * U * float(mag3))


# ---- 6. the model, micro geometry ----
TOL = (1e-4, 2e-5)
MODES = ("exact", "split")


def _gm(mode):
    from d2s import ops
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}[mode]


def _model(name, phase="hard", **kw):
    import vit_models
    sd = built(name)[0]
    m = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=LOCS, ltp_phase=phase, **kw)
    m.load_state_dict(sd)
    with torch.no_grad():
        m.ltp_threshold.copy_(torch.tensor(LTP_CASES[name]["theta"], dtype=torch.float32))
    return m.to(DEV)


def _replay(kept):
    """the model's per-stage [B, T] masks -> the restatement's [B, N] bool rows (CLS first)"""
    return [torch.cat((torch.ones((k.shape[0], 1)), k.cpu()), dim=1).bool() for k in kept]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_hard_forward_against_float64(name, mode):
    from d2s import ops
    sd, images, _, out = built(name)
    check_condition(name, out)
    m = _model(name).eval()
    x = images.to(DEV)
    with ops.gemm_mode(_gm(mode)), torch.no_grad():
        logits = m(x)
        kept, counts, per_block, plans = list(m.ltp_kept), m.tokens_per_block_counts.tolist(), list(m.tokens_per_block), list(m.ltp_plans)
        avg = m.avg_tokens
        for k, s in enumerate(m.ltp_scores):                     # the scores of the rows that entered the stage sum to 1 per image
            assert s.numel() == per_block[LOCS[k]]
        again = m(x, plans=plans)                                # the decisions replayed: the same launches, the same bits
        assert m.ltp_kept == [None] * len(LOCS) and m.tokens_per_block_counts.tolist() == counts
        alone = [m(x[b:b + 1]) for b in range(x.shape[0])]
    assert not logits.requires_grad and torch.equal(again, logits)
    live = _replay(kept)
    assert all(torch.equal(a, b) for a, b in zip(live, out["live"]))                         # the kept sets, exactly
    assert counts == [c.tolist() for c in out["counts"]] and per_block == [sum(c) for c in counts]
    assert abs(avg - sum(per_block) / (len(per_block) * x.shape[0])) < 1e-9
    with torch.no_grad():
        ref = R.model_hard({k: v.double() for k, v in sd.items()}, images, CFG, LOCS, LTP_CASES[name]["theta"], replay=live)
    print(f"{name} {mode}: rows per block {per_block}, max |logits - float64| {float((logits.cpu().double() - ref['logits']).abs().max()):.3e}")
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"].numpy(), rtol=TOL[0], atol=TOL[1])
    np.testing.assert_allclose(torch.cat(alone).cpu().numpy(), logits.cpu().numpy(), rtol=TOL[0], atol=TOL[1])        # cu indexing
    if name == "keep_all":                                      # theta = 0: nothing leaves, the dense trunk
        import vit_models
        dense = vit_models.VisionTransformerTeacher(**MICRO)
        dense.load_state_dict(sd)
        with ops.gemm_mode(_gm(mode)), torch.no_grad():
            want = dense.to(DEV).eval()(x)[0]
        np.testing.assert_allclose(logits.cpu().numpy(), want.cpu().numpy(), rtol=TOL[0], atol=TOL[1])
        assert per_block == [17 * 4] * 4
    if name == "all_cls":                                       # from stage 1 on every image is its CLS row alone
        assert counts[2] == [1] * 4 and counts[3] == [1] * 4 and per_block[3] == 4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_hard_training_loss_and_gradients_against_float64(name, mode):
    from d2s import ops
    from losses import LTPLoss
    sd, images, labels, out = built(name)
    m = _model(name).train()
    assert not m.ltp_threshold.requires_grad
    fn = LTPLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, ltp_lambda=0.5))
    with ops.gemm_mode(_gm(mode)):
        logits = m(images.to(DEV))
        loss = fn(logits, None, labels.to(DEV), {}, m.ltp_reg, m.avg_tokens)
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    live = _replay(m.ltp_kept)
    assert all(torch.equal(a, b) for a, b in zip(live, out["live"]))
    assert m.ltp_threshold.grad is None                                                      # constants of the hard phase
    kept_fraction = sum(int(l[:, 1:].sum()) for l in live) / (3 * 4 * 16)
    assert abs(float(m.ltp_reg) - kept_fraction) < 1e-6
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.model_hard(sd64, images, CFG, LOCS, LTP_CASES[name]["theta"], replay=live)
    want = R.objective(ref["logits"], labels, 0.0, 0.0)
    names = list(sd64)
    grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
    print(f"{name} {mode}: loss {float(loss.detach()):.7f} float64 {float(want.detach()):.7f}")
    np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4)
    worst = 0.0
    for k, p in m.named_parameters():
        if k == "ltp_threshold":
            continue
        g = grads[k]
        if g is None or float(g.norm()) == 0.0:                 # all-CLS: the last block's key and query weights see one token per image
            assert p.grad is None or float(p.grad.abs().max()) == 0.0 or float(p.grad.norm()) < 1e-6, k
            continue
        assert p.grad is not None, k
        rel = float((p.grad.detach().cpu().double() - g).norm() / g.norm())
        worst = max(worst, rel)
        assert rel <= 1e-3, (k, rel)
    print(f"  worst relative L2 error of a parameter gradient {worst:.2e}")


def test_hard_training_forward_is_the_eval_forward():
    _, images, _, _ = built("ltp1")
    m = _model("ltp1")
    x = images.to(DEV)
    a = m.train()(x)
    kept = [k.clone() for k in m.ltp_kept]
    b = m.eval()(x)
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), b) and all(torch.equal(p, q) for p, q in zip(kept, m.ltp_kept)) and a.requires_grad and not b.requires_grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", PRUNING)
def test_soft_training_loss_gradients_and_dtheta_against_float64(name, mode):
    from d2s import ops
    from losses import LTPLoss
    sd, images, labels, _ = built(name)
    tau, lam = SOFT["tau"], SOFT["lam"]
    m = _model(name, phase="soft", ltp_temperature=tau).train()
    fn = LTPLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, ltp_lambda=lam))
    with ops.gemm_mode(_gm(mode)):
        logits = m(images.to(DEV))
        assert m.ltp_reg.requires_grad and m.tokens_per_block == [17 * 4] * 4
        loss = fn(logits, None, labels.to(DEV), {}, m.ltp_reg, m.avg_tokens)
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    theta = [torch.tensor(float(np.float32(t)), dtype=torch.float64, requires_grad=True) for t in LTP_CASES[name]["theta"]]
    ref = R.model_soft(sd64, images, CFG, LOCS, theta, tau)
    want = R.objective(ref["logits"], labels, ref["reg"], lam)
    names = list(sd64)
    grads = torch.autograd.grad(want, [sd64[k] for k in names] + theta, allow_unused=True)
    gtheta = torch.stack(grads[len(names):])
    grads = dict(zip(names, grads[:len(names)]))
    # the model's scores come from activations that carry the fp32 error of the blocks before them (the restatement's are float64 all
    # the way), so they are held to the logits' relative tolerance, not to the kernel's 1e-5 on identical inputs (section 1 above)
    for k, s in enumerate(m.ltp_scores):
        _rel(f"soft score stage {k}", s.reshape(4, 17), ref["scores"][k], rtol=TOL[0])
        assert float((s.double().reshape(4, 17).sum(dim=1) - 1.0).abs().max()) <= 1e-5
    print(f"{name} {mode}: loss {float(loss.detach()):.7f} float64 {float(want.detach()):.7f}, R {float(m.ltp_reg.detach()):.5f} float64 {float(ref['reg'].detach()):.5f}")
    print(f"  dtheta {m.ltp_threshold.grad.cpu().tolist()} float64 {gtheta.tolist()}")
    np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4)
    np.testing.assert_allclose(m.ltp_threshold.grad.cpu().double().numpy(), gtheta.numpy(), rtol=1e-3)
    worst = 0.0
    for k, p in m.named_parameters():
        if k == "ltp_threshold":
            continue
        assert p.grad is not None and grads[k] is not None, k
        rel = float((p.grad.detach().cpu().double() - grads[k]).norm() / grads[k].norm())
        worst = max(worst, rel)
        assert rel <= 1e-3, (k, rel)
    print(f"  worst relative L2 error of a parameter gradient {worst:.2e}")
    with torch.no_grad():                                       # eval() runs the hard forward whatever the phase
        m.eval()(images.to(DEV))
    assert m.tokens_per_block[-1] < 17 * 4


# ---- 7. TrainStep ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, ltp_lambda=SOFT["lam"], **kw)


def _step(phase, with_teacher=False, student=None, **kw):
    import vit_models
    from d2s.engine import TrainStep
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**MICRO)
        teacher.load_state_dict(built("ltp1")[0])
        teacher = teacher.to(DEV)
    student = _model("ltp1", phase=phase, ltp_temperature=SOFT["tau"]) if student is None else student
    return TrainStep(student, teacher, _args(), lr=1e-3, **kw)


def _xy():
    _, images, labels, _ = built("ltp1")
    return images.to(DEV), labels.to(DEV)


@pytest.mark.parametrize("phase,with_teacher", [("soft", True), ("hard", False)])
def test_train_step_two_runs_bit_identical_and_resume(phase, with_teacher):
    from d2s import lib
    x, y = _xy()
    runs = []
    for _ in range(2):
        ts = _step(phase, with_teacher)
        assert ts.method.name == "ltp" and ts.logits_only and ts.graph is False
        losses = [float(ts(x, y)["loss"]) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((losses, ts.arena.params.clone(), ts))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert all(math.isfinite(v) for v in runs[0][0])
    ts = runs[1][2]
    for k in ("train_ltp_loss", "train_cls_loss", "train_ltp_reg", "train_avg_tokens"):
        assert k in ts.metrics and math.isfinite(float(ts.metrics[k])), k
    th0 = torch.tensor(LTP_CASES["ltp1"]["theta"], dtype=torch.float32)
    moved = not torch.equal(ts.student.ltp_threshold.detach().cpu(), th0)
    assert moved == (phase == "soft")                           # the thresholds learn in the soft phase and only there
    assert ("ltp_threshold" in ts.frozen) == (phase == "hard")
    assert float(ts.metrics["train_avg_tokens"]) == 17.0 if phase == "soft" else float(ts.metrics["train_avg_tokens"]) < 17.0
    saved = ts.state_dict()
    cfg = saved["config"]
    assert (cfg["model"], cfg["ltp_phase"], cfg["ltp_temperature"], cfg["ltp_lambda"]) == ("VisionTransformerLTP", phase, SOFT["tau"], SOFT["lam"])
    assert "ltp_threshold" in saved["model"]
    ts(x, y)
    torch.cuda.synchronize()
    three = ts.arena.params.clone()
    resumed = _step(phase, with_teacher)
    assert resumed.load_state_dict(saved) == saved["epoch"]
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three)                          # 2 steps, a checkpoint, 1 more step = 3 straight steps
    other = "hard" if phase == "soft" else "soft"
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: ltp_phase"):
        _step(other, with_teacher).load_state_dict(saved)
    import vit_models
    dense = vit_models.VisionTransformerATS(**MICRO, ats_locs=[1], ats_tokens=4, train_sample=True).to(DEV)
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: model"):
        _step(phase, with_teacher, student=dense).load_state_dict(saved)


@pytest.mark.parametrize("phase", ["soft", "hard"])
def test_train_step_accumulation_with_clipping(phase):
    x, y = _xy()
    ts = _step(phase, accum_steps=2, clip_grad=0.5)
    before = ts.arena.params.clone()
    a = ts(x, y)
    assert a["stepped"] is False and torch.equal(ts.arena.params, before)
    b = ts(x, y)
    torch.cuda.synchronize()
    assert b["stepped"] is True and not torch.equal(ts.arena.params, before) and float(b["grad_norm"]) > 0
    assert math.isfinite(float(b["loss"])) and float(a["loss"]) == float(b["loss"])          # the same batch before any update


def test_soft_to_hard_hand_over_through_a_student_checkpoint(tmp_path, monkeypatch, capsys):
    """two soft steps, the checkpoint's 'model' loaded as --student-checkpoint does it: the hard phase starts from the learnt thresholds"""
    import mask_predictor
    import vit_models
    x, y = _xy()
    ts = _step("soft")
    for _ in range(2):
        ts(x, y)
    torch.cuda.synchronize()
    learnt = ts.student.ltp_threshold.detach().cpu().clone()
    path = os.path.join(tmp_path, "soft.pt")
    torch.save(ts.state_dict(), path)
    monkeypatch.setattr(vit_models, "ltp_deit_tiny_patch16_224", lambda checkpoint_path=None, **kw: vit_models.VisionTransformerLTP(**MICRO, **kw))
    args = types.SimpleNamespace(arch="deit_tiny", method="ltp", resume=None, teacher_checkpoint=None, device=DEV, pruning_locs=LOCS,
                                 dist_weight=0.0, ltp_phase="hard", student_checkpoint=path)
    hard, teacher = mask_predictor.build_models(args)
    capsys.readouterr()
    assert teacher is None and hard.ltp_phase == "hard" and torch.equal(hard.ltp_threshold.detach().cpu(), learnt)
    assert not torch.equal(learnt, torch.tensor(LTP_CASES["ltp1"]["theta"], dtype=torch.float32))
    ts2 = _step("hard", student=hard)
    info = ts2(x, y)
    torch.cuda.synchronize()
    assert math.isfinite(float(info["loss"])) and torch.equal(hard.ltp_threshold.detach().cpu(), learnt)      # fixed from here on
    assert hard.tokens_per_block[-1] <= 17 * 4


# ---- 8. command line ----
@pytest.mark.parametrize("phase", ["soft", "hard"])
def test_cli_trains_one_tiny_epoch_and_evaluates(phase, tmp_path, capsys):
    import mask_predictor
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    common = ["--arch", "deit_tiny", "--method", "ltp", "--ltp-phase", phase, "--pruning-locs", "1", "4", "--batch-size", "4", "--val-steps", "1",
              "--dist-weight", "0"]
    acc = mask_predictor.main(common + ["--epochs", "1", "--steps-per-epoch", "2", "--student-checkpoint", path, "--output-dir", out_dir])
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    assert "Start training" in out and f"--method ltp --ltp-phase {phase}" in out and "val loss:" in out
    assert "train_ltp_reg=" in out and "train_avg_tokens=" in out and "val_avg_tokens=" in out
    cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
    assert (cfg["model"], cfg["ltp_phase"], cfg["pruning_loc"]) == ("VisionTransformerLTP", phase, [1, 4])
    acc2 = mask_predictor.main(common + ["--eval-only", "--resume", os.path.join(out_dir, "last.pt")])
    out = capsys.readouterr().out
    assert isinstance(acc2, float) and "eval only:" in out and "val_avg_tokens=" in out
