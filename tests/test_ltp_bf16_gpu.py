"""GPU tier of LTP in the bf16 arithmetic mode (train_bf16=True / --ltp-bf16; DESIGN.md section 27, "In the bf16 arithmetic mode").

The score kernel (csrc/ltp_bf16.hip, v_mfma_f32_32x32x16_bf16) against the float64 loops of tests/ltp_bf16_ref.py on the identical
bf16-rounded operands (q as it lies in the bf16 qkv, k as bf16(fp32(k) * scale)):
(a) fed with the float64 lse / cinv of those operands: 1e-5 relative per entry, the rule tests/test_ltp_gpu.py holds the fp32 kernel to -
    products of bf16 values are exact in fp32 and both kernels accumulate in fp32 - at scale 2^-3 and at 0.11;
(b) fed with what the GPU's own bf16 forward entries wrote (the varlen LSE forward, the policy forward) at scale 2^-3, where forward and
    score kernel round the same operands: every image's sum within 1e-5 of 1 and 1e-5 per entry against float64 with that very lse;
(c) bit for bit: an all-ones policy with eps = 0 against the plain form, varlen on equal lengths against dense, every image of a ragged
    batch alone against the batch, two launches;
(d) NaN-filled outputs and workspace, a guard band behind score, a cu_seqlens of garbage, every refusal with poisoned outputs untouched.
Blocks and models in tests/test_ltp_gpu.py's micro geometry against float64 with the GPU's own decisions replayed; the bar is twice the
worst relative-L2 figure of the same trunk trained dense in the bf16 mode (BlockFn) against its float64 restatement, measured in the same
test (DESIGN.md section 24's rule).  TrainStep in both phases and the command line."""
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import ltp_bf16_ref as RB
from tests import ltp_ref as R
from tests.test_ltp_cpu import CFG, LOCS, LTP_CASES, MICRO, PRUNING, SCALE, SOFT, built, make_policy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, POISON = 64, 1234.5
LENS = [1, 2, 17, 33, 129, 197]
MAX_N = 300
EPS = 1e-6
ODD_SCALE = 0.11                               # not a power of two: bf16(fp32(k) * scale) rounds
ERR_ARG = -1
WORST = {}
_REF = {}


def _note(tag, v):
    WORST[tag] = max(WORST.get(tag, 0.0), float(v))
    print(f"  {tag}: {float(v):.3e} (worst over the tests so far {WORST[tag]:.3e})")


def _rel(tag, got, ref, rtol=1e-5):
    """|got - ref| <= rtol |ref| elementwise against float64; the worst relative error is printed before the assertion"""
    got, ref = got.double().cpu().reshape(ref.shape), ref.double()
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    _note(tag, err)
    assert bool(torch.isfinite(got).all()) and float(err) <= rtol, (tag, float(err))


def _sums_to_one(tag, s, B, n):
    dev = (s.double().cpu().reshape(B, n).sum(dim=1) - 1.0).abs().max()
    _note(tag + " |sum - 1|", dev)
    assert float(dev) <= 1e-5, (tag, float(dev))


def _dev16(qkv64):
    return qkv64.float().bfloat16().reshape(qkv64.shape[0], -1).contiguous().to(DEV)


def _f32(t):
    return t.float().contiguous().to(DEV)


def _dense_case(B, n, H):
    """qkv float64 on the bf16 grid and, per scale, the float64 lse and plain score of its rounded operands; once per shape"""
    key = (B, n, H)
    if key not in _REF:
        qkv = RB.make_qkv(B * n, H, 1000 * n + 10 * H + B)
        _REF[key] = (qkv, {sc: (RB.stats_plain(qkv, B, n, H, sc), RB.score_plain(qkv, B, n, H, sc)) for sc in (SCALE, ODD_SCALE)})
    return _REF[key]


def test_the_inputs_put_max_abs_s_between_5_and_10():
    qkv = RB.make_qkv(197, 2, 1)
    q, ks = RB.round_operands(qkv, SCALE)
    top = max(float((q[:, h] @ ks[:, h].T).abs().max()) for h in range(2))
    assert 5.0 <= top <= 10.0, top


# ---- 1. the score, dense forms ----
@pytest.mark.parametrize("H", [1, 2, 6])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 65, 128, 129, 197])
@pytest.mark.parametrize("B", [1, 3])
def test_score_dense_forms(B, n, H):
    """Observed on an MI355X: see DESIGN.md section 27 ("In the bf16 arithmetic mode")."""
    from d2s import ops
    qkv64, per_scale = _dense_case(B, n, H)
    qkv = _dev16(qkv64)
    ones = torch.ones((B, n), dtype=torch.float32, device=DEV)
    # (a) float64 statistics of the same operands
    for sc in (SCALE, ODD_SCALE):
        lse64, ref = per_scale[sc]
        s = ops.ltp_score(qkv, _f32(lse64), B, n, H, sc)
        assert s.dtype == torch.float32 and tuple(s.shape) == (B * n,)
        _rel(f"(a) plain scale {sc}", s, ref)
        _sums_to_one(f"(a) plain scale {sc}", s, B, n)
        assert torch.equal(ops.ltp_score(qkv, _f32(lse64), B, n, H, sc), s)                         # (c) two launches
        for kind in (("mixed", "cls_only") if sc == SCALE else ("mixed",)):
            pol64 = make_policy(kind, B, n, 3 * n + H)
            l64, c64 = RB.stats_policy(qkv64, pol64, B, n, H, sc, EPS)
            sp = ops.ltp_score(qkv, _f32(l64), B, n, H, sc, policy=_f32(pol64), cinv=_f32(c64))
            _rel(f"(a) policy {kind} scale {sc}", sp, RB.score_policy(qkv64, pol64, B, n, H, sc, EPS))
            _sums_to_one(f"(a) policy {kind} scale {sc}", sp, B, n)
            assert torch.equal(ops.ltp_score(qkv, _f32(l64), B, n, H, sc, policy=_f32(pol64), cinv=_f32(c64)), sp)
    # (b) the GPU's own bf16 policy forward at scale 2^-3: all-ones with eps = 0 (the plain softmax), then real policies
    _, lse1, cinv1, _, _ = ops.attn_policy_fwd_bf16io(qkv, ones, B, n, H, SCALE, eps=0.0)
    assert not bool(cinv1.any())
    s = ops.ltp_score(qkv, lse1, B, n, H, SCALE)
    _sums_to_one("(b) plain", s, B, n)
    _rel("(b) plain", s, RB.score_from_stats(qkv64, B, n, H, SCALE, lse1.cpu()))
    # (c) all-ones policy, eps = 0: bit for bit the plain form
    assert torch.equal(ops.ltp_score(qkv, lse1, B, n, H, SCALE, policy=ones, cinv=cinv1), s)
    # (c) varlen on equal lengths (the same statistics in the [H, total] layout, max_n an upper bound only): bit for bit the dense form
    cu = (torch.arange(B + 1, dtype=torch.int32) * n).to(DEV)
    lse_v = lse1.permute(1, 0, 2).reshape(H, B * n).contiguous()
    assert torch.equal(ops.ltp_score(qkv, lse_v, B, n + 7, H, SCALE, cu=cu, total=B * n), s)
    for kind in ("mixed", "cls_only"):
        pol64 = make_policy(kind, B, n, 3 * n + H)
        pol = _f32(pol64)
        _, lse_p, cinv_p, _, _ = ops.attn_policy_fwd_bf16io(qkv, pol, B, n, H, SCALE, eps=EPS)
        sp = ops.ltp_score(qkv, lse_p, B, n, H, SCALE, policy=pol, cinv=cinv_p)
        _sums_to_one(f"(b) policy {kind}", sp, B, n)
        _rel(f"(b) policy {kind}", sp, RB.score_from_stats(qkv64, B, n, H, SCALE, lse_p.cpu(), pol64, cinv_p.cpu()))


# ---- 2. the score, ragged ----
@pytest.mark.parametrize("H", [1, 2, 6])
def test_score_varlen(H):
    """Observed on an MI355X: see DESIGN.md section 27 ("In the bf16 arithmetic mode")."""
    from d2s import ops
    B, total = len(LENS), sum(LENS)
    qkv64 = RB.make_qkv(total, H, 77 + H)
    qkv = _dev16(qkv64)
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=DEV)
    for sc in (SCALE, ODD_SCALE):                                                # (a)
        s = ops.ltp_score(qkv, _f32(RB.stats_varlen(qkv64, LENS, H, sc)), B, MAX_N, H, sc, cu=cu, total=total)
        _rel(f"(a) varlen scale {sc}", s, RB.score_varlen(qkv64, LENS, H, sc))
    _, lse, _, _ = ops.attn_varlen_fwd_lse_bf16io(qkv, cu, B, total, MAX_N, H, SCALE)      # (b)
    s = ops.ltp_score(qkv, lse, B, MAX_N, H, SCALE, cu=cu, total=total)
    _rel("(b) varlen", s, RB.score_varlen(qkv64, LENS, H, SCALE, lse=lse.cpu()))
    assert torch.equal(ops.ltp_score(qkv, lse, B, MAX_N, H, SCALE, cu=cu, total=total), s)  # (c) two launches
    assert torch.equal(ops.ltp_score(qkv, lse, B, 8192, H, SCALE, cu=cu, total=total), s)   # max_n is an upper bound only
    # (an image that is its CLS row alone scores 2^(fma(S, log2 e, -fl(lse log2 e))), the backward's P: 1 within an ulp, not always 1.0)
    r0 = 0
    for n in LENS:                                               # (c) every image alone, as a dense batch of one: the same bits
        dev = abs(float(s[r0:r0 + n].double().sum()) - 1.0)
        _note("(b) varlen |sum - 1|", dev)
        assert dev <= 1e-5
        one = qkv[r0:r0 + n].contiguous()
        assert torch.equal(ops.ltp_score(one, lse[:, r0:r0 + n].contiguous().view(1, H, n), 1, n, H, SCALE), s[r0:r0 + n])
        r0 += n


# ---- 3. raw calls: guard bands, NaN-filled outputs, a cu_seqlens of garbage, refusals ----
def _raw_score(qkv, lse, B, n, total, H, policy=None, cinv=None, cu=None, fill=float("nan")):
    from d2s import lib
    need = lib.query("d2s_ltp_score_bf16_workspace_bytes", total, H)
    wf = need // 4
    score = torch.full((total + GUARD,), fill, dtype=torch.float32, device=DEV)
    score[total:] = POISON
    ws = torch.full((wf + GUARD,), fill, dtype=torch.float32, device=DEV)
    ws[wf:] = POISON
    rc = lib._fn("d2s_ltp_score_bf16")(lib.ptr(qkv), lib.ptr(lse), lib.ptr(policy), lib.ptr(cinv), lib.ptr(cu), lib.ptr(score), lib.ptr(ws),
                                       need, B, n, total, H, SCALE, lib.stream())
    torch.cuda.synchronize()
    return rc, score, ws, wf


def test_score_writes_every_row_once_and_nothing_else():
    from d2s import ops
    B, n, H = 3, 33, 2
    qkv = _dev16(_dense_case(B, n, H)[0])
    ones = torch.ones((B, n), dtype=torch.float32, device=DEV)
    _, lse, cinv, _, _ = ops.attn_policy_fwd_bf16io(qkv, ones, B, n, H, SCALE, eps=EPS)
    for kw in (dict(), dict(policy=ones, cinv=cinv)):
        rc, score, ws, wf = _raw_score(qkv, lse, B, n, B * n, H, **kw)
        assert rc == 0 and bool(torch.isfinite(score[:B * n]).all()) and bool(torch.isfinite(ws[:wf]).all())      # NaN-filled: all overwritten
        assert torch.equal(score[:B * n], ops.ltp_score(qkv, lse, B, n, H, SCALE, **kw))
        assert bool((score[B * n:] == POISON).all()) and bool((ws[wf:] == POISON).all())
    total = sum(LENS)
    qkv = _dev16(RB.make_qkv(total, H, 5))
    cu = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=DEV)
    _, lse, _, _ = ops.attn_varlen_fwd_lse_bf16io(qkv, cu, len(LENS), total, 197, H, SCALE)
    rc, score, ws, wf = _raw_score(qkv, lse, len(LENS), 256, total, H, cu=cu)
    assert rc == 0 and bool(torch.isfinite(score[:total]).all()) and bool(torch.isfinite(ws[:wf]).all())
    assert bool((score[total:] == POISON).all()) and bool((ws[wf:] == POISON).all())
    # rows no segment covers keep what they held
    short = cu.clone()
    short[-1] = total - 50
    rc, score2, _, _ = _raw_score(qkv, lse, len(LENS), 256, total, H, cu=short, fill=POISON)
    assert rc == 0 and bool((score2[total - 50:] == POISON).all()) and torch.equal(score2[:total - 197], score[:total - 197])


def test_score_clamps_a_cu_seqlens_of_garbage():
    """segments are clamped to [0, total) and to max_n rows: whatever cu_seqlens holds, only score [total] and the workspace are written"""
    H, total = 2, 100
    qkv = _dev16(RB.make_qkv(total, H, 6))
    lse = torch.zeros((H, total), dtype=torch.float32, device=DEV)
    for vals in ([-50, 20, 10, 400, 2 ** 31 - 1], [0, 0, 0, 0, 0], [90, 300, -7, 64, 100], [-2 ** 31, 2 ** 31 - 1, -1, 100, 99]):
        cu = torch.tensor(vals, dtype=torch.int32, device=DEV)
        rc, score, ws, wf = _raw_score(qkv, lse, 4, 64, total, H, cu=cu, fill=POISON)
        assert rc == 0 and bool((score[total:] == POISON).all()) and bool((ws[wf:] == POISON).all())


def test_score_refusals_leave_the_outputs_alone():
    from d2s import lib
    B, n, H = 2, 17, 2
    total = B * n
    qkv = _dev16(RB.make_qkv(total, H, 8))
    lse = torch.zeros((B, H, n), dtype=torch.float32, device=DEV)
    pol = torch.ones((B, n), dtype=torch.float32, device=DEV)
    cu = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=DEV)
    need = lib.query("d2s_ltp_score_bf16_workspace_bytes", total, H)
    score = torch.full((total,), POISON, dtype=torch.float32, device=DEV)
    ws = torch.full((need // 4,), POISON, dtype=torch.float32, device=DEV)
    good = dict(qkv=qkv, lse=lse, policy=None, cinv=None, cu=None, score=score, ws=ws, wsb=need, B=B, n=n, total=total, H=H)
    bad = [dict(qkv=None), dict(lse=None), dict(score=None), dict(ws=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(n=8193),
           dict(total=0), dict(H=0), dict(H=-2), dict(wsb=need - 4), dict(wsb=0), dict(policy=pol), dict(cinv=lse),
           dict(policy=pol, cinv=lse, cu=cu), dict(total=total + 1), dict(n=n + 1), dict(cu=cu, n=8193)]
    fn = lib._fn("d2s_ltp_score_bf16")
    for change in bad:
        a = dict(good, **change)
        rc = fn(lib.ptr(a["qkv"]), lib.ptr(a["lse"]), lib.ptr(a["policy"]), lib.ptr(a["cinv"]), lib.ptr(a["cu"]), lib.ptr(a["score"]),
                lib.ptr(a["ws"]), a["wsb"], a["B"], a["n"], a["total"], a["H"], SCALE, lib.stream())
        assert rc == ERR_ARG, (list(change), rc)
    torch.cuda.synchronize()
    assert bool((score == POISON).all()) and bool((ws == POISON).all())


# ---- 4. a stage block on the bf16 data path ----
def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("lengths", [(5, 33), (2, 17, 18)], ids=str)
def test_stage_block_that_keeps_every_row_is_the_stage_less_block_bit_for_bit(lengths):
    """the ATS precedent (tests/test_stage_bf16_gpu.py): a replayed plan that keeps every row -> y and all 13 gradients are the bits of
    functional_ats.RaggedBlockFn on a stage-less bf16 block"""
    from d2s import functional_ltp as LF
    from d2s import ops
    from tests import test_ragged_bf16_train_gpu as RG
    x, gy = RG._block_inputs(lengths, f"ltp{len(lengths)}")
    B = len(lengths)
    cu = RG._cu(lengths).to(DEV)
    row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
    plan = (torch.ones(sum(lengths), device=DEV), torch.tensor([n - 1 for n in lengths], dtype=torch.int32, device=DEV))
    theta = torch.full((1,), 0.5, device=DEV)                    # replaying: never read

    def run():
        p = [t.to(DEV).requires_grad_(True) for t in RG._block_params()]
        xd = x.to(DEV).requires_grad_(True)
        with ops.gemm_mode(ops.GEMM_BF16):
            r = LF._RaggedLTP(cu, B, max(lengths), RG.BLOCK_H, RG.SCALE, row_src, theta, max(lengths) - 1, plan, bf16=True)
            y = LF.stage_block(xd, p, 1e-6, r)
            assert r.rows == list(lengths) and r.score is None
            grads = torch.autograd.grad(y, [xd] + p, gy.to(DEV))
            ops.join_weight_grads()
        torch.cuda.synchronize()
        return y.detach(), [g.detach() for g in grads]
    y, grads = run()
    yb, gb = RG._ragged_block_run(lengths, x, gy)
    assert _same_bits(y, yb), "y"
    for name, a, b in zip(("x",) + RG._NAMES, grads, gb):
        assert _same_bits(a, b), name
    y2, grads2 = run()
    assert _same_bits(y, y2) and all(_same_bits(a, b) for a, b in zip(grads, grads2)), "two runs"


def test_stage_block_refusals():
    from d2s import functional_ats as AF
    from d2s import functional_ltp as LF
    from d2s import lib, ops
    from tests import test_ragged_bf16_train_gpu as RG
    lengths = (5, 9)
    x, _ = RG._block_inputs(lengths, "ltprefuse")
    cu = RG._cu(lengths).to(DEV)
    row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
    p = [t.to(DEV).requires_grad_(True) for t in RG._block_params()]
    xd = x.to(DEV).requires_grad_(True)
    theta = torch.zeros((1,), device=DEV)
    stage = lambda **kw: LF._RaggedLTP(cu, 2, 9, RG.BLOCK_H, RG.SCALE, row_src, theta, 8, **kw)
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:                                   # without the keyword: the text it had
            LF.stage_block(xd, p, 1e-6, stage())
        assert str(e.value) == LF.BF16_REFUSAL
        with pytest.raises(lib.D2SError) as e:
            LF.soft_block(xd.view(1, 14, -1), p, RG.BLOCK_H, 1e-6, RG.SCALE, None, True)
        assert str(e.value) == LF.BF16_REFUSAL
    for mode in (ops.GEMM_EXACT, ops.GEMM_SPLIT):
        with ops.gemm_mode(mode), pytest.raises(lib.D2SError) as e:
            LF.stage_block(xd, p, 1e-6, stage(bf16=True))
        assert str(e.value) == AF._BF16_MODE_REFUSAL


# ---- 5. the model, micro geometry ----
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


def _ce(labels):
    return lambda ls: torch.nn.functional.cross_entropy(ls, labels.to(ls.device))


def _grad_errors(m, ref_grads, skip=("ltp_threshold",)):
    out = {}
    for k, p in m.named_parameters():
        if k in skip:
            continue
        want = ref_grads[k]
        assert p.grad is not None and want is not None, k
        out[k] = float((p.grad.detach().cpu().double() - want).norm()) / float(want.norm())
    return out


def _rel_l2(got, ref):
    return float((got.detach().cpu().double() - ref).norm()) / float(ref.norm())


_DENSE = {}


def _dense_yardstick(name):
    """the same trunk trained dense in the bf16 mode (BlockFn) against its float64 restatement, CE on the case's labels -> (worst
    relative-L2 error of a parameter gradient, relative-L2 error of the logits, |loss - float64|); once per case"""
    import vit_models
    from d2s import ops
    if name not in _DENSE:
        sd, images, labels, _ = built(name)
        dense = vit_models.VisionTransformerATS(**MICRO)
        dense.load_state_dict(sd)
        dense = dense.to(DEV).train()
        with ops.gemm_mode(ops.GEMM_BF16):
            logits = dense(images.to(DEV))
            loss = _ce(labels)(logits)
            loss.backward()
            ops.join_weight_grads()
            torch.cuda.synchronize()
        sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        ref = R.model_hard(sd64, images, CFG, LOCS, [0.0, 0.0, 0.0])
        want = _ce(labels)(ref["logits"])
        names = list(sd64)
        grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
        errs = _grad_errors(dense, grads)
        _DENSE[name] = (max(errs.values()), _rel_l2(logits, ref["logits"].detach()), abs(float(loss.detach()) - float(want.detach())))
        print(f"dense trunk bf16 ({name}): worst relative L2 gradient error {_DENSE[name][0]:.3e} ({max(errs, key=errs.get)}), "
              f"logits {_DENSE[name][1]:.3e}, |loss - float64| {_DENSE[name][2]:.3e}")
    return _DENSE[name]


def _stage_rows(counts, k):
    """first row of every image among the rows that entered stage k, from the model's per-block row counts"""
    return np.concatenate([[0], np.cumsum(counts[LOCS[k]])])[:-1]


@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_hard_decisions_are_score_against_threshold_exactly(name):
    """eval() in the bf16 mode: keep == (score >= theta) from the model's own ltp_scores and ltp_plans, CLS kept whatever its score, every
    image's scores summing to 1; the plans replayed give the same bits; the logits against float64 with the decisions replayed"""
    from d2s import ops
    sd, images, _, _ = built(name)
    m = _model(name, train_bf16=True).eval()
    x = images.to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16), torch.no_grad():
        logits = m(x)
        plans, scores, kept = list(m.ltp_plans), list(m.ltp_scores), list(m.ltp_kept)
        counts = m.tokens_per_block_counts.tolist()
        again = m(x, plans=plans)
    assert torch.equal(again, logits) and not logits.requires_grad
    theta = torch.tensor(LTP_CASES[name]["theta"], dtype=torch.float32)
    for k, ((keep, cnt), s) in enumerate(zip(plans, scores)):
        first = _stage_rows(counts, k)
        assert s.dtype == torch.float32 and s.numel() == sum(counts[LOCS[k]]) == keep.numel()
        want = (s.cpu() >= theta[k]).float()
        want[torch.from_numpy(first).long()] = 1.0
        assert torch.equal(keep.cpu(), want), (name, k)
        bounds = list(first) + [s.numel()]
        for b, (r0, r1) in enumerate(zip(bounds, bounds[1:])):
            assert abs(float(s[r0:r1].double().sum()) - 1.0) <= 1e-5, (name, k, b)
            assert int(cnt[b]) == int(want[r0 + 1:r1].sum())
    live = _replay(kept)
    with torch.no_grad():
        ref = R.model_hard({k: v.double() for k, v in sd.items()}, images, CFG, LOCS, LTP_CASES[name]["theta"], replay=live)
    _, dense_logit, _ = _dense_yardstick(name)
    le = _rel_l2(logits, ref["logits"])
    print(f"{name} eval bf16: rows per block {[sum(c) for c in counts]}; logits relative L2 {le:.3e} (dense {dense_logit:.3e})")
    assert le <= 2.0 * dense_logit, (le, dense_logit)


def test_with_every_threshold_zero_the_logits_are_the_bf16_ragged_trunks():
    from d2s import functional_ats as AF
    from d2s import ops
    _, images, _, _ = built("keep_all")
    m = _model("keep_all", train_bf16=True).train()
    x = images.to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        logits = m(x)
        assert m.tokens_per_block == [17 * 4] * 4 and all(bool((k == 1).all()) for k in m.ltp_kept)
        t = m._embed(x)
        B, n, D = t.shape
        t = t.contiguous().view(B * n, D)
        cu = (torch.arange(B + 1, dtype=torch.int32) * n).to(DEV)
        for blk in m.blocks:
            a = blk.attn
            t = AF.ragged_block_train(t, blk._params(), blk.norm1.eps, AF._Ragged(cu, B, n, a.num_heads, a.scale, bf16=True))
        want = m._head(AF.ClsGatherFn.apply(t, cu).view(B, 1, D))[0]
        with torch.no_grad():
            ev = m.eval()(x)
    torch.cuda.synchronize()
    assert torch.equal(logits.detach(), want.detach()) and torch.equal(ev, logits.detach())


@pytest.mark.parametrize("name", PRUNING)
def test_hard_training_against_float64_with_the_plans_replayed(name):
    """Observed on an MI355X: see DESIGN.md section 27 ("In the bf16 arithmetic mode")."""
    from d2s import ops
    sd, images, labels, _ = built(name)
    dense_grad, dense_logit, _ = _dense_yardstick(name)
    ce = _ce(labels)
    x = images.to(DEV)
    B = x.shape[0]
    m = _model(name, train_bf16=True).train()
    assert not m.ltp_threshold.requires_grad
    with ops.gemm_mode(ops.GEMM_BF16):
        hits = ops.shadow_hits
        logits = m(x)
        kept = [k.clone() for k in m.ltp_kept]
        per_block = list(m.tokens_per_block)
        ce(logits).backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        hits = ops.shadow_hits - hits
        with torch.no_grad():                                   # eval in this process: the training forward's bits
            assert torch.equal(m.eval()(x), logits.detach()) and all(torch.equal(a, b) for a, b in zip(kept, m.ltp_kept))
        m.train()
    # every block but the last finds the bf16 form of its gy: the last one's arrives from the CLS scatter
    assert hits == CFG["depth"] - 1, hits
    assert m.ltp_threshold.grad is None                         # constants of the hard phase
    assert per_block[-1] < per_block[0]
    # under an fp32 mode the keyword changes no bit
    with ops.gemm_mode(ops.GEMM_EXACT):
        a, b = _model(name, train_bf16=True).train(), _model(name).train()
        la, lb = a(x), b(x)
        fp32_kept = [k.clone() for k in b.ltp_kept]
        ce(la).backward()
        ce(lb).backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        assert torch.equal(la.detach(), lb.detach())
        for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            assert (pa.grad is None and pb.grad is None) or torch.equal(pa.grad, pb.grad), k
    moved = sum(int(not torch.equal(p[i], q[i])) for p, q in zip(kept, fp32_kept) for i in range(B))
    live = _replay(kept)
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.model_hard(sd64, images, CFG, LOCS, LTP_CASES[name]["theta"], replay=live)
    want = ce(ref["logits"])
    names = list(sd64)
    ref_grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
    errs = _grad_errors(m, ref_grads)
    le = _rel_l2(logits, ref["logits"].detach())
    worst = max(errs, key=errs.get)
    print(f"LTP hard bf16 {name}: rows per block {per_block}; {moved} of {len(LOCS) * B} kept sets differ from the fp32-mode selection; "
          f"logits {le:.3e} (dense {dense_logit:.3e}); worst relative L2 gradient error {errs[worst]:.3e} ({worst}); dense worst "
          f"{dense_grad:.3e}, bar {2 * dense_grad:.3e}")
    assert le <= 2.0 * dense_logit, (le, dense_logit)
    for k, e in errs.items():
        assert e <= 2.0 * dense_grad, (k, e, dense_grad)


@pytest.mark.parametrize("name", PRUNING)
def test_soft_training_against_float64_with_the_gpus_scores_as_constants(name):
    """Observed on an MI355X: see DESIGN.md section 27 ("In the bf16 arithmetic mode")."""
    from d2s import ops
    from losses import LTPLoss
    sd, images, labels, _ = built(name)
    dense_grad, dense_logit, dense_loss = _dense_yardstick(name)
    tau, lam = SOFT["tau"], SOFT["lam"]
    x = images.to(DEV)
    m = _model(name, phase="soft", ltp_temperature=tau, train_bf16=True).train()
    fn = LTPLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, ltp_lambda=lam))
    with ops.gemm_mode(ops.GEMM_BF16):
        logits = m(x)
        assert m.ltp_reg.requires_grad and m.tokens_per_block == [17 * 4] * 4
        scores = [s.detach().clone() for s in m.ltp_scores]
        loss = fn(logits, None, labels.to(DEV), {}, m.ltp_reg, m.avg_tokens)
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
    for k, s in enumerate(scores):
        assert s.dtype == torch.float32 and tuple(s.shape) == (4, 17)
        _sums_to_one(f"soft score stage {k}", s, 4, 17)
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    theta = [torch.tensor(float(np.float32(t)), dtype=torch.float64, requires_grad=True) for t in LTP_CASES[name]["theta"]]
    ref = RB.model_soft_given(sd64, images, CFG, LOCS, theta, tau, [s.cpu().double() for s in scores])
    want = R.objective(ref["logits"], labels, ref["reg"], lam)
    names = list(sd64)
    grads = torch.autograd.grad(want, [sd64[k] for k in names] + theta, allow_unused=True)
    gtheta = torch.stack(grads[len(names):])
    ref_grads = dict(zip(names, grads[:len(names)]))
    with torch.no_grad():                                       # recorded, not asserted: the scores against a float64 forward of its own
        own = R.model_soft({k: v.double() for k, v in sd.items()}, images, CFG, LOCS, LTP_CASES[name]["theta"], tau)
    drift = [float(((s.cpu().double() - o).abs() / o.abs()).max()) for s, o in zip(scores, own["scores"])]
    errs = _grad_errors(m, ref_grads)
    got_theta = m.ltp_threshold.grad.cpu().double()
    eth = [abs(float(got_theta[k]) - float(gtheta[k])) / abs(float(gtheta[k])) for k in range(len(LOCS))]
    eth_l2 = float((got_theta - gtheta).norm() / gtheta.norm())
    le = _rel_l2(logits, ref["logits"].detach())
    dl = abs(float(loss.detach()) - float(want.detach()))
    worst = max(errs, key=errs.get)
    print(f"LTP soft bf16 {name}: loss {float(loss.detach()):.7f} float64 {float(want.detach()):.7f} (|diff| {dl:.3e}, dense {dense_loss:.3e}); "
          f"logits {le:.3e} (dense {dense_logit:.3e}); worst relative L2 gradient error {errs[worst]:.3e} ({worst}); dense worst "
          f"{dense_grad:.3e}, bar {2 * dense_grad:.3e}")
    print(f"  dtheta {got_theta.tolist()} float64 {gtheta.tolist()}; relative error per stage {[f'{e:.3e}' for e in eth]}, relative L2 {eth_l2:.3e}")
    print(f"  worst relative deviation of a stage's scores from a float64 forward of its own: {[f'{d:.3e}' for d in drift]}")
    assert dl <= 2.0 * dense_loss, (dl, dense_loss)
    assert le <= 2.0 * dense_logit, (le, dense_logit)
    for k, e in errs.items():
        assert e <= 2.0 * dense_grad, (k, e, dense_grad)
    for k, e in enumerate(eth):
        assert e <= 2.0 * dense_grad, (f"dtheta_{k}", e, dense_grad)


# ---- 6. TrainStep ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, ltp_lambda=SOFT["lam"], **kw)


def _step(phase, with_teacher, bf16=True, **kw):
    import vit_models
    from d2s.engine import TrainStep
    teacher = None
    if with_teacher:
        teacher = vit_models.VisionTransformerTeacher(**MICRO)
        teacher.load_state_dict(built("ltp1")[0])
        teacher = teacher.to(DEV)
    student = _model("ltp1", phase=phase, ltp_temperature=SOFT["tau"], **({"train_bf16": True} if bf16 else {}))
    return TrainStep(student, teacher, _args(), lr=1e-3, **kw)


@pytest.mark.parametrize("phase,with_teacher", [("soft", True), ("hard", False)])
def test_train_step_two_runs_bit_identical_resume_and_refusals(phase, with_teacher):
    from d2s import lib, ops
    _, images, labels, _ = built("ltp1")
    x, y = images.to(DEV), labels.to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        runs = []
        for _ in range(2):
            ts = _step(phase, with_teacher)
            assert ts.method.name == "ltp" and ts.logits_only and ts.graph is False
            first = float(ts(x, y)["loss"])
            saved = ts.state_dict()
            second = float(ts(x, y)["loss"])
            torch.cuda.synchronize()
            runs.append(([first, second], ts.arena.params.clone(), saved, ts))
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])                  # two runs of two steps
        assert all(math.isfinite(v) for v in runs[0][0])
        ts, saved = runs[1][3], runs[1][2]
        cfg = ts.config()
        assert cfg["train_bf16"] is True and cfg["ltp_phase"] == phase and cfg["gemm_mode"] == ops.GEMM_BF16
        assert saved["config"]["train_bf16"] is True
        th0 = torch.tensor(LTP_CASES["ltp1"]["theta"], dtype=torch.float32)
        assert (not torch.equal(ts.student.ltp_threshold.detach().cpu(), th0)) == (phase == "soft")
        resumed = _step(phase, with_teacher)
        resumed.load_state_dict(saved)
        resumed(x, y)
        torch.cuda.synchronize()
        assert torch.equal(resumed.arena.params, runs[1][1])                                     # 1 step, a checkpoint, 1 more step
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16"):        # a checkpoint without the key: off
            _step(phase, with_teacher).load_state_dict(dict(saved, config={k: v for k, v in saved["config"].items() if k != "train_bf16"}))
        with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an LTP student"):
            _step(phase, with_teacher, graph=True)
        with pytest.raises(lib.D2SError, match="LTP student in the bf16 arithmetic mode"):       # a default-built student: the old refusal
            _step(phase, with_teacher, bf16=False)
    # a step without the keyword (it exists in an fp32 mode only, so the checkpoint's recorded mode is set to that one's)
    with ops.gemm_mode(ops.GEMM_EXACT):
        with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16: the checkpoint has True, this run has False"):
            _step(phase, with_teacher, bf16=False).load_state_dict(dict(saved, config=dict(saved["config"], gemm_mode=ops.GEMM_EXACT)))


# ---- 7. the command line ----
@pytest.mark.parametrize("phase", ["soft", "hard"])
def test_cli_trains_one_tiny_epoch_and_evaluates_in_bf16(phase, tmp_path, capsys):
    import mask_predictor
    import vit_models
    from d2s import ops
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    out_dir = os.path.join(tmp_path, "run")
    common = ["--arch", "deit_tiny", "--method", "ltp", "--ltp-bf16", "--ltp-phase", phase, "--pruning-locs", "1", "4", "--batch-size", "4",
              "--val-steps", "1", "--dist-weight", "0"]
    before = ops._default_mode
    try:
        acc = mask_predictor.main(common + ["--epochs", "1", "--steps-per-epoch", "2", "--student-checkpoint", path, "--output-dir", out_dir])
        assert ops.get_gemm_mode() == ops.GEMM_BF16          # the flag set the mode itself
        out = capsys.readouterr().out
        assert isinstance(acc, float) and 0.0 <= acc <= 1.0
        assert "Attention: --ltp-bf16: every phase and the evaluation run in the bf16 arithmetic mode on the bf16 data path" in out
        assert "Start training" in out and f"--method ltp --ltp-phase {phase}" in out and "val loss:" in out
        cfg = torch.load(os.path.join(out_dir, "last.pt"), map_location="cpu", weights_only=True)["config"]
        assert (cfg["model"], cfg["ltp_phase"], cfg["train_bf16"]) == ("VisionTransformerLTP", phase, True)
        ops.set_gemm_mode(before)
        acc2 = mask_predictor.main(common + ["--eval-only", "--resume", os.path.join(out_dir, "last.pt")])
        assert ops.get_gemm_mode() == ops.GEMM_BF16
        out = capsys.readouterr().out
        assert isinstance(acc2, float) and "eval only:" in out and "val_avg_tokens=" in out and "Attention: --ltp-bf16" in out
    finally:
        ops.set_gemm_mode(before)
