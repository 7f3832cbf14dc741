"""GPU tier of training ATS and A-ViT in the bf16 arithmetic mode (train_bf16=True / --ats-train-bf16, --avit-bf16; DESIGN.md sections 24
and 25): the two backward row moves of csrc/ragged_stage_bf16.hip, a block with a sampling stage on the bf16 data path, the two models,
TrainStep and the command line.

The kernels are held bit for bit: g_old to the fp32 entries they restate (d2s_ragged_repack_bwd; d2s_ragged_repack_bwd followed by
d2s_avit_halt_bwd), g_old_bf16 to torch's round-to-nearest-even of g_old, and for planted values to the bf16 patterns written out here.
Lengths [1, 2, 17, 33, 300] and D in {128, 192, 384}; the kernels' chunk is 64 rows and a workgroup takes every 8th chunk of its image,
so a second set with a 600-row image makes one workgroup run its loop twice.  A guard band behind both outputs.

Blocks and models against float64 with the GPU's own decisions replayed.  Every bound is twice the relative-L2 error that existing bf16
code shows against float64 on the same inputs, measured in the same run, and - DESIGN.md section 22's precedent - the worst figure
over the quantities compared (y, dx and the 12 parameter gradients of a block; every parameter of a model): the stage-less bf16 ragged
block for a block with a stage, the dense trunk in the bf16 mode (BlockFn) for the models.  The factor 2 stands for the one extra bf16
rounding on the hook's rows."""
import os
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import ats_ref as AR
from tests import ats_train_ref as T
from tests import avit_ref as R
from tests.test_avit_cpu import AVIT_CASES, CFG, EPS, built
from oracle import d2s_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, POISON = 64, 1234.5
ERR_ARG = -1
LENS = {"issue": [1, 2, 17, 33, 300], "slots": [600, 65]}
DIMS = [128, 192, 384]
# fp32 bit pattern -> the bf16 pattern round-to-nearest-even gives: ties of both parities and both signs, the two zeros, two roundings
# that carry into the exponent, the largest finite fp32 (-> inf)
PLANTED = [(0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0x00000000, 0x0000),
           (0x80000000, 0x8000), (0x3FFF8000, 0x4000), (0x3F7FFFFF, 0x3F80), (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80)]


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits32(a) if a.dtype == torch.float32 else _bits16(a),
                                                                      _bits32(b) if b.dtype == torch.float32 else _bits16(b))


def _plant(t, rows, col0=0):
    """the PLANTED fp32 patterns into t[row, col0:col0 + len] for every row of rows"""
    v = torch.tensor([p[0] - (1 << 32) if p[0] >= (1 << 31) else p[0] for p in PLANTED], dtype=torch.int32).view(torch.float32)
    for r in rows:
        t[r, col0:col0 + len(PLANTED)] = v
    return t


def _planted_bf16():
    return torch.tensor([p[1] - (1 << 16) if p[1] >= (1 << 15) else p[1] for p in PLANTED], dtype=torch.int16)


def _outputs(total, D):
    """poisoned fp32 and bf16 output buffers with a guard band -> (buf, buf16)"""
    return (torch.full((total * D + GUARD,), POISON, dtype=torch.float32, device=DEV),
            torch.full((total * D + GUARD,), POISON, dtype=torch.bfloat16, device=DEV))


def _guards_intact(buf, buf16, total, D):
    assert bool((buf[total * D:] == POISON).all()), "guard band behind g_old was written"
    assert torch.equal(buf16[total * D:], torch.full((GUARD,), POISON, dtype=torch.bfloat16, device=DEV)), "guard band behind g_old_bf16 was written"


def _cu(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)


def test_the_planted_patterns_are_what_torch_rounds_them_to():
    """the table above against torch's own conversion (a CPU statement; it sits here because only this tier reads the table)"""
    v = _plant(torch.zeros((1, 16)), [0])[0, :len(PLANTED)]
    assert torch.equal(_bits16(v.bfloat16()), _planted_bf16())


# ---- 1. d2s_ragged_repack_bwd_bf16out ----
def _keep_pattern(kind, lengths, g):
    total = sum(lengths)
    cu = np.concatenate([[0], np.cumsum(lengths)])
    if kind == "all":
        keep = torch.ones(total)
    elif kind == "cls_only":
        keep = torch.zeros(total)
    else:
        keep = (torch.rand(total, generator=g) < 0.5).float()
    if kind == "first_zero":                   # the flag of every CLS row is 0: the row is kept all the same
        keep[torch.from_numpy(cu[:-1]).long()] = 0.0
    elif kind != "cls_only":
        keep[torch.from_numpy(cu[:-1]).long()] = 1.0
    counts = [sum(1 for i in range(n) if i == 0 or float(keep[cu[b] + i]) != 0.0) for b, n in enumerate(lengths)]
    if kind == "short":                        # a cu_new shorter than the flags imply: the last kept rows of an image find no row
        counts = [max(1, c - 2) for c in counts]
    return keep, counts


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", ["all", "cls_only", "random", "first_zero", "short"])
@pytest.mark.parametrize("lens", sorted(LENS))
def test_repack_backward_bf16out_bit_for_bit(lens, kind, D):
    from d2s import lib, ops
    lengths = LENS[lens]
    B, total = len(lengths), sum(lengths)
    g = torch.Generator().manual_seed(1000 + D + len(kind))
    keep, counts = _keep_pattern(kind, lengths, g)
    cu_old, cu_new = _cu(lengths), _cu(counts)
    total_new = int(cu_new[-1])
    g_new = _plant(torch.randn((total_new, D), generator=g), [0, total_new // 2, total_new - 1], col0=3)
    gd, kd, co, cn = g_new.to(DEV), keep.to(DEV), cu_old.to(DEV), cu_new.to(DEV)
    want = ops.ragged_repack_bwd(gd, kd, co, cn, total, B)                      # (a) the sibling's bits
    got = []
    for _ in range(2):
        buf, buf16 = _outputs(total, D)
        lib.call("d2s_ragged_repack_bwd_bf16out", lib.ptr(gd), lib.ptr(kd), lib.ptr(co), lib.ptr(cn), lib.ptr(buf), lib.ptr(buf16), B, D)
        torch.cuda.synchronize()
        _guards_intact(buf, buf16, total, D)
        got.append((buf[:total * D].view(total, D).clone(), buf16[:total * D].view(total, D).clone()))
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[0][1], got[1][1]), "two launches"
    g32, g16 = got[0]
    assert _same_bits(g32, want), "(a) g_old is d2s_ragged_repack_bwd's"
    assert _same_bits(g16, g32.bfloat16()), "(b) g_old_bf16 is g_old rounded once, to nearest even"
    # (c) and the move itself, from the flags: a kept position inside the new segment takes that row, everything else zeros
    c32, c16 = g32.cpu(), g16.cpu()
    zero_rows = moved = 0
    for b, n in enumerate(lengths):
        p = 0
        for i in range(n):
            row = int(cu_old[b]) + i
            if i == 0 or float(keep[row]) != 0.0:
                if p < counts[b]:
                    assert _same_bits(c32[row], g_new[int(cu_new[b]) + p]), (b, i)
                    moved += 1
                else:
                    assert not bool(c32[row].any()) and not bool(_bits16(c16[row]).any()), (b, i)      # (c): +0 in both forms
                    zero_rows += 1
                p += 1
            else:
                assert not bool(c32[row].any()) and not bool(_bits16(c16[row]).any()), (b, i)
    assert moved == total_new and (zero_rows > 0) == (kind == "short")
    assert torch.equal(_bits16(c16[0, 3:3 + len(PLANTED)]), _planted_bf16())     # row 0 is image 0's CLS row: always moved
    wrapped16 = ops.bf16_buffer(total, D, DEV)
    wrapped = ops.ragged_repack_bwd(gd, kd, co, cn, total, B, g16=wrapped16)
    torch.cuda.synchronize()
    assert _same_bits(wrapped, g32) and _same_bits(wrapped16, g16)


def test_repack_backward_bf16out_refusals_leave_the_outputs_untouched():
    from d2s import lib
    lib.load()
    B, D, lengths = 2, 8, [3, 2]
    total = sum(lengths)
    g_new, keep = torch.ones((total, D), device=DEV), torch.ones(total, device=DEV)
    cu = _cu(lengths).to(DEV)
    buf, buf16 = _outputs(total, D)
    P = lib.ptr
    good = [P(g_new), P(keep), P(cu), P(cu), P(buf), P(buf16), B, D]
    fn, st = lib._fn("d2s_ragged_repack_bwd_bf16out"), lib.stream()
    for pos, val in [(k, None) for k in range(6)] + [(6, 0), (6, -1), (7, 0), (7, -4), (7, 6), (7, 9)]:
        a = list(good)
        a[pos] = val
        assert fn(*a, st) == ERR_ARG, (pos, val)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and torch.equal(buf16, torch.full_like(buf16, POISON))
    assert fn(*good, st) == 0
    torch.cuda.synchronize()
    assert bool((buf[:total * D] == 1).all()) and bool((buf16[:total * D] == 1).all())
    _guards_intact(buf, buf16, total, D)


# ---- 2. d2s_avit_halt_repack_bwd_bf16out ----
def _fused_raw(g_new, keep, cu_new, h, cu, rs, nh, w, dacc, ycls, ysave, gsc, B, N, D, total, layer, L, gamma):
    """two launches on poisoned, guarded outputs -> (g_old, g_old_bf16) of the first, after checking the second gave the same bits"""
    from d2s import lib
    got = []
    for _ in range(2):
        buf, buf16 = _outputs(total, D)
        lib.call("d2s_avit_halt_repack_bwd_bf16out", lib.ptr(g_new), lib.ptr(keep), lib.ptr(cu_new), lib.ptr(h), lib.ptr(cu), lib.ptr(rs),
                 lib.ptr(nh), lib.ptr(w), lib.ptr(dacc), lib.ptr(ycls), lib.ptr(ysave), lib.ptr(gsc), lib.ptr(buf), lib.ptr(buf16), B, N, D,
                 total, int(layer), int(L), float(gamma))
        torch.cuda.synchronize()
        _guards_intact(buf, buf16, total, D)
        got.append((buf[:total * D].view(total, D).clone(), buf16[:total * D].view(total, D).clone()))
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[0][1], got[1][1]), "two launches"
    return got[0]


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", ["spread", "all_halt", "none_halt"])
def test_boundary_backward_replays_the_halting_scenarios_bit_for_bit(kind, D):
    """tests/test_avit_gpu.py's scenarios, layer by layer from the last: an image that is its CLS row alone, an image already finished, a
    CLS that halts while its patches are live (spread), a layer where every token halts (all_halt), a layer where none does (none_halt),
    the last layer (nothing arrives), gamma = 0 (the last two).  (d) against the two fp32 entries chained, (e) against torch's rounding."""
    from d2s import ops
    from tests import test_avit_gpu as AG
    sc, st, ref, records, _ = AG._run_sequence(kind, D, seed=AG.SEEDS[D])
    B, L, gamma, N = len(AG.LENS), sc["L"], sc["gamma"], AG.N_TOK
    g = torch.Generator().manual_seed(9)
    dacc = torch.randn((B, D), generator=g).to(DEV)
    gsc = (0.01 * torch.randn(L + 1, generator=g)).float().to(DEV)
    dead_images = live_cls_halts = 0
    for k in reversed(range(len(records))):
        rec = records[k]
        layer, total = rec["layer"], rec["y"].shape[0]
        cu, rs = torch.from_numpy(rec["cu"]).to(DEV), torch.from_numpy(rec["row_src"]).to(DEV)
        nh = ref["nh"]
        dead_images += int((nh[:, 0] < layer).sum())
        live_cls_halts += int(((nh[:, 0] == layer) & ((nh[:, 1:] == layer).sum(1) > 0)).sum())
        if layer == L:
            g_new = keep = cu_new = None
            want = ops.avit_halt_bwd(None, rec["h"], cu, rs, st, rec["w"], dacc, rec["ycls"], gsc, layer, gamma)
        else:
            cu_new = torch.from_numpy(records[k + 1]["cu"]).to(DEV)
            total_new = records[k + 1]["y"].shape[0]
            keep = rec["keep"].contiguous()
            g_new = _plant(torch.randn((total_new, D), generator=g), [0, total_new // 2, total_new - 1], col0=3).to(DEV)
            gin = ops.ragged_repack_bwd(g_new, keep, cu, cu_new, total, B)
            want = ops.avit_halt_bwd(gin, rec["h"], cu, rs, st, rec["w"], dacc, rec["ycls"], gsc, layer, gamma)
        torch.cuda.synchronize()
        g32, g16 = _fused_raw(g_new, keep, cu_new, rec["h"], cu, rs, st["nh"], rec["w"], dacc, rec["ycls"], st["ysave"], gsc, B, N, D, total,
                              layer, L, gamma)
        assert _same_bits(g32, want), f"(d) {kind} layer {layer}"
        assert _same_bits(g16, g32.bfloat16()), f"(e) {kind} layer {layer}"
        w32, w16 = ops.avit_halt_repack_bwd_bf16io(g_new, keep, cu_new, rec["h"], cu, rs, st, rec["w"], dacc, rec["ycls"], gsc, layer, gamma)
        torch.cuda.synchronize()
        assert _same_bits(w32, g32) and _same_bits(w16, g16)
    if kind == "spread":
        assert dead_images > 0 and live_cls_halts > 0, (dead_images, live_cls_halts)
    if kind == "all_halt":
        assert dead_images == B                 # layer 2 sees finished images only


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("fresh", [False, True])
def test_boundary_backward_on_long_images_bit_for_bit(fresh, D):
    """images of 300 and 600 rows (several chunks; one workgroup runs its loop twice) with a state made at random: a finished image, dead
    rows (row_src 0 behind the CLS row), tokens that halt here, earlier and later.  The contract is equality with the chain, so the
    state need not come from a forward."""
    from d2s import ops
    lengths = [1, 2, 17, 33, 300, 600]
    B, N, L, layer, gamma = len(lengths), 700, 3, 2, 1.7
    total = sum(lengths)
    g = torch.Generator().manual_seed(31 + D)
    cu = _cu(lengths)
    rs = torch.cat([torch.cat((torch.zeros(1, dtype=torch.long), torch.sort(torch.randperm(N - 1, generator=g)[:n - 1])[0] + 1))
                    for n in lengths]).int()
    rs[int(cu[4]) + 5] = 0                      # a row that names no token: it takes what arrived and no term of its own
    nh = torch.randint(1, L + 1, (B, N), generator=g).int()
    nh[:, 0] = torch.tensor([3, 2, 1, 3, 2, 3])   # image 2 finished in layer 1; images 1 and 4 halt here; the others go on
    st = dict(c=torch.zeros((B, N), device=DEV), nh=nh.to(DEV), ysave=torch.randn((B, D), generator=g).to(DEV))
    h = torch.rand(total, generator=g).to(DEV)
    w, dacc, ycls = torch.rand(B, generator=g).to(DEV), torch.randn((B, D), generator=g).to(DEV), torch.randn((B, D), generator=g).to(DEV)
    gsc = (0.01 * torch.randn(L + 1, generator=g)).float().to(DEV)
    cud, rsd = cu.to(DEV), rs.to(DEV)
    if fresh:
        g_new = keep = cu_new = None
        want = ops.avit_halt_bwd(None, h, cud, rsd, st, w, dacc, ycls, gsc, layer, gamma)
    else:
        keep, counts = _keep_pattern("random", lengths, g)
        cu_new = _cu(counts).to(DEV)
        total_new = int(cu_new[-1])
        keep = keep.to(DEV)
        g_new = _plant(torch.randn((total_new, D), generator=g), [0, total_new // 2, total_new - 1], col0=3).to(DEV)
        want = ops.avit_halt_bwd(ops.ragged_repack_bwd(g_new, keep, cud, cu_new, total, B), h, cud, rsd, st, w, dacc, ycls, gsc, layer, gamma)
    torch.cuda.synchronize()
    g32, g16 = _fused_raw(g_new, keep, cu_new, h, cud, rsd, st["nh"], w, dacc, ycls, st["ysave"], gsc, B, N, D, total, layer, L, gamma)
    assert _same_bits(g32, want), "(d)"
    assert _same_bits(g16, g32.bfloat16()), "(e)"
    assert not bool((g32 == POISON).any())                                      # every element written


def test_boundary_backward_refusals_leave_the_outputs_untouched():
    from d2s import lib
    lib.load()
    B, N, D, total, L = 2, 5, 8, 6, 3
    f = lambda n: torch.ones((n,), device=DEV)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32, device=DEV)
    rs = torch.tensor([0, 1, 2, 0, 3, 4], dtype=torch.int32, device=DEV)
    nh = torch.full((B * N,), 3, dtype=torch.int32, device=DEV)
    g_new, keep, h, w, dacc, ycls, ysave, gsc = f(total * D), f(total), f(total) * 0.5, f(B), f(B * D), f(B * D), f(B * D), f(L + 1)
    buf, buf16 = _outputs(total, D)
    P = lib.ptr
    good = [P(g_new), P(keep), P(cu), P(h), P(cu), P(rs), P(nh), P(w), P(dacc), P(ycls), P(ysave), P(gsc), P(buf), P(buf16), B, N, D, total,
            1, L, 1.0]
    fn, st = lib._fn("d2s_avit_halt_repack_bwd_bf16out"), lib.stream()
    bad = [{k: None} for k in range(3, 14)]                                       # d2s_avit_halt_bwd's pointers and the two outputs
    bad += [{0: None}, {1: None}, {2: None}, {0: None, 1: None}, {0: None, 2: None}, {1: None, 2: None}]      # the triple given only in part
    bad += [{14: 0}, {15: 0}, {16: 0}, {16: 6}, {17: 0}, {18: 0}, {18: L + 1}, {19: 65}, {19: 0}]
    for change in bad:
        a = list(good)
        for pos, val in change.items():
            a[pos] = val
        assert fn(*a, st) == ERR_ARG, change
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and torch.equal(buf16, torch.full_like(buf16, POISON))
    fresh = list(good)
    fresh[0] = fresh[1] = fresh[2] = None
    assert fn(*good, st) == 0 and fn(*fresh, st) == 0                             # all three, or none
    torch.cuda.synchronize()
    _guards_intact(buf, buf16, total, D)
    assert not bool((buf[:total * D] == POISON).any())


# ---- 3. a block with a sampling stage on the bf16 data path ----
BLOCK_LENGTHS = [(5, 33), (2, 17, 18)]


def _stage_block_run(lengths, x, gy_full, K=None, plan=None, below=False):
    """RaggedBlockFn with a stage (bf16=True, stage_bf16=True) in the bf16 mode, optionally stacked on a stage-less bf16 ragged block
    -> (y, [gx, 12 gradients of the stage block], the kept rows as indices into the rows that entered, shadow hits of the backward)"""
    from d2s import functional_ats as AF
    from d2s import ops
    from tests import test_ragged_bf16_train_gpu as RB
    B = len(lengths)
    cu = _cu(lengths).to(DEV)
    p = [t.to(DEV).requires_grad_(True) for t in RB._block_params()]
    xd = x.to(DEV).requires_grad_(True)
    row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        xin = xd
        if below:
            p0 = [t.to(DEV).requires_grad_(True) for t in RB._block_params()]
            xin = AF.ragged_block_train(xd, p0, 1e-6, AF._Ragged(cu, B, max(lengths), RB.BLOCK_H, RB.SCALE, bf16=True))
        r = AF._Ragged(cu, B, max(lengths), RB.BLOCK_H, RB.SCALE, row_src, max(lengths) if K is None else K, max(lengths) - 1, plan,
                       bf16=True, stage_bf16=True)
        y = AF.ragged_block_train(xin, p, 1e-6, r)
        keep = r.plan[0].cpu()
        idx = torch.tensor([int(cu[b]) + i for b, n in enumerate(lengths) for i in range(n) if i == 0 or float(keep[int(cu[b]) + i]) != 0.0])
        assert y.shape[0] == idx.numel() == int(r.cu_new[-1])
        hits = ops.shadow_hits
        grads = torch.autograd.grad(y, [xd] + p, gy_full[idx].to(DEV))
        ops.join_weight_grads()
        hits = ops.shadow_hits - hits
    torch.cuda.synchronize()
    return y.detach(), [t.detach() for t in grads], idx, hits


def _rel_l2(got, want):
    return [float((a.cpu().double().flatten() - b.flatten()).norm()) / float(b.norm()) for a, b in zip(got, want)]


@pytest.mark.parametrize("lengths", BLOCK_LENGTHS, ids=str)
def test_stage_block_that_keeps_every_row_is_the_stage_less_block_bit_for_bit(lengths):
    from tests import test_ragged_bf16_train_gpu as RB
    x, gy = RB._block_inputs(lengths, f"st{len(lengths)}")
    plan = (torch.ones(sum(lengths), device=DEV), torch.tensor([n - 1 for n in lengths], dtype=torch.int32, device=DEV))
    y, grads, idx, _ = _stage_block_run(lengths, x, gy, plan=plan)
    assert idx.tolist() == list(range(sum(lengths)))
    yb, gb = RB._ragged_block_run(lengths, x, gy)
    assert _same_bits(y, yb), "y"
    for name, a, b in zip(("x",) + RB._NAMES, grads, gb):
        assert _same_bits(a, b), name
    y2, grads2, _, _ = _stage_block_run(lengths, x, gy, plan=plan)
    assert _same_bits(y, y2) and all(_same_bits(a, b) for a, b in zip(grads, grads2)), "two runs"


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("lengths", BLOCK_LENGTHS, ids=str)
def test_stage_block_that_selects_against_float64(lengths, K):
    """Observed on an MI355X: see DESIGN.md section 24 ("Training in the bf16 arithmetic mode")."""
    from tests import test_ragged_bf16_train_gpu as RB
    x, gy = RB._block_inputs(lengths, f"st{len(lengths)}")
    names = ("y", "x") + RB._NAMES
    # the yardstick: the stage-less bf16 ragged block against float64 on the same inputs
    yb, gb = RB._ragged_block_run(lengths, x, gy)
    y64, g64 = RB._block_float64(lengths, x, gy)
    base = _rel_l2([yb] + gb, [y64] + g64)
    bar = 2.0 * max(base)
    y, grads, idx, _ = _stage_block_run(lengths, x, gy, K=K)
    kept = [int(((idx >= a) & (idx < b)).sum()) for a, b in zip(_cu(lengths)[:-1].tolist(), _cu(lengths)[1:].tolist())]
    assert all(1 <= k <= min(K + 1, n) for k, n in zip(kept, lengths)) and idx.numel() < sum(lengths), kept
    # the float64 block with the GPU's plan replayed: attention over every row that entered, the MLP half (row-wise) on the kept rows
    sd = {"blocks.0." + k: t.double().requires_grad_(True) for k, t in zip(RB._NAMES, RB._block_params())}
    xr = x.double().requires_grad_(True)
    cu = _cu(lengths)
    full = torch.cat([O.block(sd, 0, xr[int(cu[b]):int(cu[b + 1])][None], RB.BLOCK_CFG)[0][0] for b in range(len(lengths))])
    want_y = full[idx]
    want_g = torch.autograd.grad(want_y, [xr] + [sd["blocks.0." + k] for k in RB._NAMES], gy[idx].double())
    errs = _rel_l2([y] + grads, [want_y.detach()] + list(want_g))
    print(f"stage block bf16 lengths {lengths} K {K}: kept {kept}; relative L2 error " + " ".join(f"{k} {v:.2e}" for k, v in zip(names, errs)))
    print(f"  stage-less bf16 ragged block, same inputs: " + " ".join(f"{k} {v:.2e}" for k, v in zip(names, base)) + f" | bar {bar:.2e}")
    for name, e in zip(names, errs):
        assert e <= bar, (name, e, bar)


def test_stage_block_hands_the_bf16_gradient_to_the_block_below():
    """a stage block stacked on a plain bf16 ragged block: the plain block's backward finds the shadow of its gy (ops.shadow_hits grows)"""
    from tests import test_ragged_bf16_train_gpu as RB
    lengths = (5, 33)
    x, gy = RB._block_inputs(lengths, "st2")
    _, grads, _, hits = _stage_block_run(lengths, x, gy, K=8, below=True)
    assert hits == 1 and bool(torch.isfinite(grads[0]).all())


def test_stage_block_refusals():
    from d2s import functional_ats as AF
    from d2s import lib, ops
    from tests import test_ragged_bf16_train_gpu as RB
    lengths = (5, 9)
    x, _ = RB._block_inputs(lengths, "refuse")
    cu = _cu(lengths).to(DEV)
    row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
    p = [t.to(DEV).requires_grad_(True) for t in RB._block_params()]
    xd = x.to(DEV).requires_grad_(True)
    stage = lambda **kw: AF._Ragged(cu, 2, 9, RB.BLOCK_H, RB.SCALE, row_src, 4, 8, None, **kw)
    with ops.gemm_mode(ops.GEMM_BF16):
        with pytest.raises(lib.D2SError) as e:                                   # bf16=True alone: the text it had
            AF.ragged_block_train(xd, p, 1e-6, stage(bf16=True))
        assert str(e.value) == AF._BF16_STAGE_REFUSAL
        with pytest.raises(lib.D2SError, match="stage_bf16=True needs bf16=True"):
            AF.ragged_block_train(xd, p, 1e-6, stage(stage_bf16=True))
        with pytest.raises(lib.D2SError) as e:
            AF.ragged_block_train(xd, p, 1e-6, stage())
        assert str(e.value) == AF._BF16_REFUSAL
    for mode in (ops.GEMM_EXACT, ops.GEMM_SPLIT):
        with ops.gemm_mode(mode), pytest.raises(lib.D2SError) as e:
            AF.ragged_block_train(xd, p, 1e-6, stage(bf16=True, stage_bf16=True))
        assert str(e.value) == AF._BF16_MODE_REFUSAL


# ---- 4. the models ----
def _grad_errors(m, ref_grads):
    out = {}
    for k, p in m.named_parameters():
        want = ref_grads[k]
        assert p.grad is not None and want is not None, k
        out[k] = float((p.grad.detach().cpu().double() - want).norm()) / float(want.norm())
    return out


def _logit_error(logits, ref):
    return float((logits.detach().cpu().double() - ref).norm()) / float(ref.norm())


_DENSE = {}


def _dense_yardstick(tag, sd, images, cfg, geom, scalar_of):
    """the same trunk trained dense in the bf16 mode (BlockFn) against its float64 restatement -> (worst relative-L2 error of a parameter
    gradient, relative-L2 error of the logits); once per case"""
    import vit_models
    from d2s import ops
    if tag not in _DENSE:
        dense = vit_models.VisionTransformerATS(**geom)
        dense.load_state_dict(sd)
        dense = dense.to(DEV).train()
        with ops.gemm_mode(ops.GEMM_BF16):
            logits = dense(images.to(DEV))
            scalar_of(logits).backward()
            ops.join_weight_grads()
            torch.cuda.synchronize()
        ref_logits, _, ref_grads = T.model_grads(sd, images, cfg, [], [], loss_of=lambda ls: scalar_of(ls))
        errs = _grad_errors(dense, ref_grads)
        _DENSE[tag] = (max(errs.values()), _logit_error(logits, ref_logits))
        print(f"dense trunk bf16 ({tag}): worst relative L2 gradient error {_DENSE[tag][0]:.3e} ({max(errs, key=errs.get)}), "
              f"logits {_DENSE[tag][1]:.3e}")
    return _DENSE[tag]


def _weight(B, C):
    return torch.randn((B, C), generator=torch.Generator().manual_seed(77))


@pytest.mark.parametrize("locs,K", [([1, 2, 3], [12, 8, 4]), ([0], 8)], ids=str)
def test_ats_model_trains_through_the_stages_in_bf16(locs, K):
    """Observed on an MI355X: see DESIGN.md section 24 ("Training in the bf16 arithmetic mode")."""
    import vit_models
    from d2s import ops
    from tests import test_ats_train_gpu as AT
    sd, images, geom = AT._models("micro1")
    cfg = cases.MODEL_CASES["micro1"]["cfg"]
    B = images.shape[0]
    W = _weight(B, cfg["num_classes"])
    scalar_of = lambda ls: (ls * W.to(device=ls.device, dtype=ls.dtype)).sum()
    dense_grad, dense_logit = _dense_yardstick("micro1", sd, images, cfg, geom, scalar_of)
    m = AT._ats("micro1", ats_locs=locs, ats_tokens=K, train_sample=True, train_bf16=True).train()
    x = images.to(DEV)
    with ops.gemm_mode(ops.GEMM_BF16):
        hits = ops.shadow_hits
        logits = m(x)
        kept = AT._kept_sets(m, B)
        plans = list(m.ats_plans)
        scalar_of(logits).backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        hits = ops.shadow_hits - hits
        # eval in this process takes the existing bf16 inference route: the plans replayed give the training forward's bits
        plain = AT._ats("micro1", ats_locs=locs, ats_tokens=K).eval()
        assert torch.equal(plain(x, plans=plans), m.eval()(x, plans=plans))
        m.train()
        # without the keyword the bf16 mode raises what it raised
        with pytest.raises(NotImplementedError, match="train_sample in the bf16 arithmetic mode"):
            AT._ats("micro1", ats_locs=locs, ats_tokens=K, train_sample=True).train()(x)
    # every block but the last finds the bf16 form of its gy: the last one's arrives from the CLS scatter
    assert hits == cfg["depth"] - 1, hits
    # under an fp32 mode the keyword changes no bit
    with ops.gemm_mode(ops.GEMM_EXACT):
        a = AT._ats("micro1", ats_locs=locs, ats_tokens=K, train_sample=True, train_bf16=True).train()
        b = AT._ats("micro1", ats_locs=locs, ats_tokens=K, train_sample=True).train()
        la, lb = a(x), b(x)
        fp32_kept = AT._kept_sets(b, B)
        scalar_of(la).backward()
        scalar_of(lb).backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        assert torch.equal(la.detach(), lb.detach())
        for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(pa.grad, pb.grad), k
    moved = sum(int(not torch.equal(i, j)) for s, t in zip(kept, fp32_kept) for i, j in zip(s, t))
    ref_logits, _, ref_grads = T.model_grads(sd, images, cfg, locs, kept, logit_weight=W)
    errs = _grad_errors(m, ref_grads)
    le = _logit_error(logits, ref_logits)
    worst = max(errs, key=errs.get)
    print(f"ATS bf16 locs {locs} K {K}: tokens per stage {[c.cpu().tolist() for c in m.tokens_per_stage]}; {moved} of {len(locs) * B} kept "
          f"sets differ from the fp32 selection; logits {le:.3e} (dense {dense_logit:.3e}); worst relative L2 gradient error "
          f"{errs[worst]:.3e} ({worst}); dense worst {dense_grad:.3e}, bar {2 * dense_grad:.3e}")
    assert le <= 2.0 * dense_logit, (le, dense_logit)
    for k, e in errs.items():
        assert e <= 2.0 * dense_grad, (k, e, dense_grad)


PEN = dict(avit_ponder_scale=5e-2, avit_prior_alpha=0.3)       # tests/test_avit_gpu.py's: the penalty gradients are visible


def _avit(name, **kw):
    import vit_models
    from tests.test_avit_gpu import _GEOM
    c = AVIT_CASES[name]
    m = vit_models.VisionTransformerAViT(**_GEOM, gate_scale=c["gamma"], gate_center=c["beta"], **kw)
    m.load_state_dict(built(name)[0])
    return m.to(DEV)


@pytest.mark.parametrize("name", sorted(AVIT_CASES))
def test_avit_model_trains_in_bf16(name):
    """Observed on an MI355X: see DESIGN.md section 25 ("Training in the bf16 arithmetic mode")."""
    from d2s import lib, ops
    from losses import AViTLoss
    from tests.test_avit_gpu import _GEOM
    sd, images, labels, out64 = built(name)
    c = AVIT_CASES[name]
    L = CFG["depth"]
    ce = lambda ls: torch.nn.functional.cross_entropy(ls, labels.to(ls.device))
    dense_grad, dense_logit = _dense_yardstick(name, sd, images, CFG, _GEOM, ce)
    fn = AViTLoss(types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.0, **PEN))
    x = images.to(DEV)
    m = _avit(name, target_depth=2.0, train_bf16=True).train()
    with ops.gemm_mode(ops.GEMM_BF16):
        hits = ops.shadow_hits
        logits = m(x)
        n = m.halt_layer.cpu().long()
        rows = [list(r) for r in m.avit_run.rows_per_layer]
        loss = fn(logits, None, labels.to(DEV), {}, m.ponder_loss, m.prior_loss, m.avg_depth)
        loss.backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        hits = ops.shadow_hits - hits
        # eval in this process takes the existing bf16 inference route, and the training forward is that forward
        with torch.no_grad():
            assert torch.equal(_avit(name, target_depth=2.0).eval()(x), logits.detach())
        # without the keyword the bf16 mode raises what it raised
        with pytest.raises(lib.D2SError, match="fp32 arithmetic modes"):
            _avit(name, target_depth=2.0).train()(x)
    assert hits == L, hits                                                       # one per block: no block casts its gy
    assert m.avit_run.bf16 is True
    assert any(1 in r for r in rows[1:]) and bool((n[:, 0] < L).any())            # 1-row segments: dead CLS rows of finished images
    with ops.gemm_mode(ops.GEMM_EXACT):                                          # under an fp32 mode the keyword changes no bit
        a, b = _avit(name, target_depth=2.0, train_bf16=True).train(), _avit(name, target_depth=2.0).train()
        la, lb = a(x), b(x)
        assert a.avit_run.bf16 is False
        fn(la, None, labels.to(DEV), {}, a.ponder_loss, a.prior_loss, a.avg_depth).backward()
        fn(lb, None, labels.to(DEV), {}, b.ponder_loss, b.prior_loss, b.avg_depth).backward()
        ops.join_weight_grads()
        torch.cuda.synchronize()
        assert torch.equal(la.detach(), lb.detach())
        for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(pa.grad, pb.grad), k
    moved = int((n != out64["n"]).sum())
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.forward(sd64, images, CFG, c["gamma"], c["beta"], EPS, n_forced=n)
    want, _ = R.objective(ref, labels, ponder_scale=PEN["avit_ponder_scale"], prior_alpha=PEN["avit_prior_alpha"], target_depth=2.0)
    names = list(sd64)
    ref_grads = dict(zip(names, torch.autograd.grad(want, [sd64[k] for k in names], allow_unused=True)))
    errs = _grad_errors(m, ref_grads)
    le = _logit_error(logits, ref["logits"].detach())
    worst = max(errs, key=errs.get)
    print(f"A-ViT bf16 {name}: rows per layer {[sum(r) for r in rows]}, CLS halts at {n[:, 0].tolist()}; {moved} of {n.numel()} halting "
          f"layers differ from the float64 decisions; loss {float(loss.detach()):.6f} float64 {float(want.detach()):.6f}; logits {le:.3e} "
          f"(dense {dense_logit:.3e}); worst relative L2 gradient error {errs[worst]:.3e} ({worst}); dense worst {dense_grad:.3e}, "
          f"bar {2 * dense_grad:.3e}")
    assert le <= 2.0 * dense_logit, (le, dense_logit)
    for k, e in errs.items():
        assert e <= 2.0 * dense_grad, (k, e, dense_grad)


# ---- 5. TrainStep ----
def _args(**kw):
    return types.SimpleNamespace(mixup=0.0, cls_weight=1.0, dist_weight=0.5, step=0, **PEN, **kw)


def _dense_step_deviation(sd, images, labels, geom, cfg):
    """the dense trunk's bf16 step (a merging student with r = 0: the logits-only route, CE alone) -> |first loss - float64|"""
    import vit_models
    from d2s.engine import TrainStep
    from tests.tome_train_ref import tome_loss
    student = vit_models.VisionTransformerToMe(**geom, train_merge=True, tome_r=0, train_bf16=True)
    student.load_state_dict(sd)
    loss = float(TrainStep(student.to(DEV), None, _args(), lr=1e-3)(images.to(DEV), labels.to(DEV))["loss"])
    want = float(tome_loss(AR.model_forward(sd, images, cfg, [])[0], None, labels, 1.0, 0.5))
    return abs(loss - want), loss


def _three_steps_and_a_checkpoint(make_step, x, y):
    """-> (the first step's info, the student of that step, the checkpoint after 2 steps); two runs of 3 steps and 2 + 1 steps through
    the checkpoint give the same parameters bit for bit"""
    ts = make_step()
    info = ts(x, y)
    torch.cuda.synchronize()
    first = dict(info)
    state = ts.student
    record = (state.halt_layer.cpu().long() if hasattr(state, "halt_layer") else None)
    ts(x, y)
    saved = ts.state_dict()
    ts(x, y)
    torch.cuda.synchronize()
    three = ts.arena.params.clone()
    again = make_step()
    for _ in range(3):
        again(x, y)
    torch.cuda.synchronize()
    assert torch.equal(again.arena.params, three), "two runs of 3 steps"
    resumed = make_step()
    resumed.load_state_dict(saved)
    resumed(x, y)
    torch.cuda.synchronize()
    assert torch.equal(resumed.arena.params, three), "2 steps, a checkpoint, 1 more step"
    return first, record, saved


def _mismatch_both_ways(make_on, make_off, saved):
    from d2s import lib
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16"):          # a step without the keyword
        make_off().load_state_dict(saved)
    old = dict(saved, config={k: v for k, v in saved["config"].items() if k != "train_bf16"})
    with pytest.raises(lib.D2SError, match="checkpoint config mismatch: train_bf16"):          # a checkpoint without the key: off
        make_on().load_state_dict(old)


def test_ats_train_step_in_bf16():
    """Observed on an MI355X: see DESIGN.md section 24 ("Training in the bf16 arithmetic mode")."""
    from d2s import lib, ops
    from d2s.engine import TrainStep
    from tests import test_ats_train_gpu as AT
    from tests.tome_train_ref import tome_loss
    sd, images, geom = AT._models("micro1")
    case = cases.MODEL_CASES["micro1"]
    labels = torch.from_numpy(cases.make_labels(case))
    x, y = images.to(DEV), labels.to(DEV)
    locs, toks = [1, 2, 3], [12, 8, 4]
    student = lambda **kw: AT._ats("micro1", ats_locs=locs, ats_tokens=toks, train_sample=True, **kw)
    make = lambda **kw: TrainStep(student(train_bf16=True), None, _args(), lr=1e-3, **kw)
    with ops.gemm_mode(ops.GEMM_BF16):
        dense_dev, dense_loss = _dense_step_deviation(sd, images, labels, geom, case["cfg"])
        ts = make()
        assert ts.method.name == "ats" and ts.graph is False
        info = ts(x, y)
        torch.cuda.synchronize()
        kept = AT._kept_sets(ts.student, images.shape[0])
        cfg = ts.config()
        assert cfg["train_bf16"] is True and cfg["train_sample"] is True and cfg["gemm_mode"] == ops.GEMM_BF16
        _, want, _ = T.model_grads(sd, images, case["cfg"], locs, kept, loss_of=lambda ls: tome_loss(ls, None, labels, 1.0, 0.5))
        dev = abs(float(info["loss"]) - float(want))
        print(f"ATS bf16 train step: loss {float(info['loss']):.7f}, float64 {float(want):.7f}, deviation {dev:.3e}; dense step "
              f"{dense_loss:.7f}, deviation {dense_dev:.3e}, tolerance {2 * dense_dev:.3e}")
        _, _, saved = _three_steps_and_a_checkpoint(make, x, y)
        assert saved["config"]["train_bf16"] is True
        _mismatch_both_ways(make, lambda: TrainStep(student(), None, _args(), lr=1e-3), saved)
        with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an Adaptive Token Sampling student"):
            make(graph=True)
        assert dev <= 2 * dense_dev, (dev, dense_dev)


def test_avit_train_step_in_bf16():
    """Observed on an MI355X: see DESIGN.md section 25 ("Training in the bf16 arithmetic mode")."""
    from d2s import lib, ops
    from d2s.engine import TrainStep
    from tests.test_avit_gpu import _GEOM
    sd, images, labels, _ = built("avit1")
    c = AVIT_CASES["avit1"]
    x, y = images.to(DEV), labels.to(DEV)
    make = lambda **kw: TrainStep(_avit("avit1", target_depth=2.0, train_bf16=True), None, _args(), lr=1e-3, **kw)
    with ops.gemm_mode(ops.GEMM_BF16):
        dense_dev, dense_loss = _dense_step_deviation(sd, images, labels, _GEOM, CFG)
        ts = make()
        assert ts.method.name == "avit" and ts.graph is False
        info = ts(x, y)
        torch.cuda.synchronize()
        n = ts.student.halt_layer.cpu().long()
        cfg = ts.config()
        assert cfg["train_bf16"] is True and cfg["model"] == "VisionTransformerAViT" and cfg["gemm_mode"] == ops.GEMM_BF16
        with torch.no_grad():
            ref = R.forward({k: v.double() for k, v in sd.items()}, images, CFG, c["gamma"], c["beta"], EPS, n_forced=n)
            want, _ = R.objective(ref, labels, ponder_scale=PEN["avit_ponder_scale"], prior_alpha=PEN["avit_prior_alpha"], target_depth=2.0)
        dev = abs(float(info["loss"]) - float(want))
        print(f"A-ViT bf16 train step: loss {float(info['loss']):.7f}, float64 {float(want):.7f}, deviation {dev:.3e}; dense step "
              f"{dense_loss:.7f}, deviation {dense_dev:.3e}, tolerance {2 * dense_dev:.3e}")
        _, _, saved = _three_steps_and_a_checkpoint(make, x, y)
        assert saved["config"]["train_bf16"] is True
        _mismatch_both_ways(make, lambda: TrainStep(_avit("avit1", target_depth=2.0), None, _args(), lr=1e-3), saved)
        with pytest.raises(lib.D2SError, match=r"TrainStep\(graph=True\) with an A-ViT student"):
            make(graph=True)
        assert dev <= 2 * dense_dev, (dev, dense_dev)


# ---- 6. the command line ----
def _tiny_checkpoint(tmp_path):
    import vit_models
    torch.manual_seed(0)
    path = os.path.join(tmp_path, "deit_tiny.pt")
    torch.save({"model": vit_models.dynamic_vit_tiny_patch16_224_teacher().state_dict()}, path)
    return path


@pytest.mark.parametrize("method", ["ats", "avit"])
def test_cli_trains_one_tiny_epoch_in_bf16(method, tmp_path, capsys):
    import mask_predictor
    from d2s import ops
    path = _tiny_checkpoint(tmp_path)
    argv = {"ats": ["--method", "ats", "--ats-train", "--ats-train-bf16", "--pruning-locs", "3", "6", "9", "--ats-tokens", "8"],
            "avit": ["--method", "avit", "--avit-bf16", "--avit-gate-scale", "4", "--avit-gate-center", "1"]}[method]
    before = ops._default_mode
    try:
        acc = mask_predictor.main(["--arch", "deit_tiny"] + argv + ["--epochs", "1", "--steps-per-epoch", "2", "--val-steps", "1", "--batch-size", "4",
                                                                   "--dist-weight", "0", "--student-checkpoint", path])
        assert ops.get_gemm_mode() == ops.GEMM_BF16          # the flag set the mode itself
    finally:
        ops.set_gemm_mode(before)
    out = capsys.readouterr().out
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0
    flag = {"ats": "--ats-train-bf16", "avit": "--avit-bf16"}[method]
    assert f"Attention: {flag}: the step runs in the bf16 arithmetic mode on the bf16 data path" in out
    assert "Start training" in out and "val loss:" in out
    assert {"ats": "--ats-train: ats tokens per stage: mean [", "avit": "--method avit: tokens per layer ["}[method] in out
