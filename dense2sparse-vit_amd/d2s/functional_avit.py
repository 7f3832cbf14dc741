"""A-ViT (Yin et al. 2022; DESIGN.md section 25 - the build's own definition, PARITY UNPINNED): per-token adaptive depth on the ragged
packed batch.  Every block is functional_ats.RaggedBlockFn without a stage; what is stated here is what follows a block: the halting
step (ops.avit_halt) and the re-pack that takes the halted tokens out of the batch, as one differentiable Function, and the two penalty
terms of the objective as another.

The halting decisions carry no gradient; everything else is smooth.  A block's backward needs quantities of later layers - each token's
halting layer, the gradient of the accumulator, the CLS row at its image's halting layer - and all of them exist once the forward has
finished: they live on the AViTRun the Functions of one forward share, so one backward launch per block suffices.  The order is fixed by
the graph: the last block's Function returns the accumulator AND the per-layer partial sums, the penalty Function reads the latter, so
its backward (which leaves the per-layer factors on the run) has run before any halting step's backward starts.

One host read per block: the new offsets (B + 1 ints) size the next block's launches, as at an ATS stage.

Training in the bf16 arithmetic mode (AViTRun(..., bf16=True)): the blocks are functional_ats._Ragged(bf16=True)
ones, and a boundary's backward is ONE launch (ops.avit_halt_repack_bwd_bf16io: the re-pack's backward, the halting step's terms and the
bf16 form of the result), parked as the gradient's shadow so that the block in front finds it and casts nothing."""
import math

import torch

from . import functional as DF
from . import ops


def target_distribution(L, target_depth):
    """tgt_l proportional to N(l - 1; target_depth, 1), normalised over the L layers (float64 on the host, then fp32)"""
    v = [math.exp(-0.5 * (l - float(target_depth)) ** 2) for l in range(L)]
    s = sum(v)
    return torch.tensor([x / s for x in v], dtype=torch.float32)


class AViTRun:
    """What the Functions of one forward share.  B images of N tokens (CLS included), D channels, L blocks.  cu / row_src / max_n describe
    the packed batch as it stands; rows_per_layer[l - 1] is the list of every image's rows in block l (a finished image: its dead CLS
    row).  After the forward: st["nh"] the halting layers [B, N], st["R"] the remainders, st["acc"] the accumulator; after the
    penalty's backward: gsc."""

    def __init__(self, B, N, D, L, gamma, beta, eps_halt, device, bf16=False):
        self.B, self.N, self.D, self.L = int(B), int(N), int(D), int(L)
        self.bf16 = bool(bf16)               # the boundaries' backward hands on the bf16 form of the gradient too
        self.gamma, self.beta, self.eps_halt = float(gamma), float(beta), float(eps_halt)
        self.st = ops.avit_state(B, N, D, L, device)
        self.cu = ops.ragged_offsets(torch.full((B,), N - 1, dtype=torch.int32, device=device), extra=1)      # arange(B + 1) * N
        self.row_src = torch.arange(N, dtype=torch.int32, device=device).repeat(B)
        self.max_n = int(N)
        self.rows_per_layer = [[int(N)] * int(B)]
        self.dacc = self.gsc = None


class AViTHaltFn(torch.autograd.Function):
    """The halting step of block `layer` and the re-pack: y [total, D] -> the packed batch of the tokens that go on, [total', D] (the
    run's cu / row_src / max_n move with it).  The last layer has nothing to re-pack: it returns (acc [B, D], part [L, B, 3])."""

    @staticmethod
    def forward(ctx, y, run, layer):
        train = DF.wants_grad(ctx)
        y = y.contiguous()
        last = layer == run.L
        cu, row_src = run.cu, run.row_src
        keep, counts, w, h, ycls = ops.avit_halt(y, cu, row_src, run.st, layer, last, run.gamma, run.beta, run.eps_halt, save=train)
        if train:
            ctx.run, ctx.layer, ctx.kept = run, layer, (keep, cu, row_src, w, h, ycls, y.shape[0])
        if last:
            return run.st["acc"], run.st["part"]
        cu_new = ops.ragged_offsets(counts, extra=1)
        off = cu_new.tolist()                 # the one device sync of a block: the packed row counts size every later launch
        rows = [b - a for a, b in zip(off, off[1:])]
        x, run.row_src = ops.ragged_repack(y, keep, cu, cu_new, row_src, off[-1], run.B)
        run.cu, run.max_n = cu_new, max(rows)
        run.rows_per_layer.append(rows)
        if train:
            ctx.cu_new = cu_new
        return x

    @staticmethod
    def backward(ctx, g, gpart=None):
        run, layer = ctx.run, ctx.layer
        keep, cu, row_src, w, h, ycls, total = ctx.kept
        last = layer == run.L
        if last:
            run.dacc = g.contiguous()
            if run.gsc is None:               # the penalties took no part in the loss
                run.gsc = torch.zeros((run.L + 1,), dtype=torch.float32, device=g.device)
        if run.bf16:                          # one launch: the re-pack's backward (nothing arrives at the last layer), the step's terms, both forms
            arrived = (None, None, None) if last else (g.contiguous(), keep, ctx.cu_new)
            gy, gy16 = ops.avit_halt_repack_bwd_bf16io(*arrived, h, cu, row_src, run.st, w, run.dacc, ycls, run.gsc, layer, run.gamma)
            ops.shadow_put(gy, gy16)          # the block in front takes it (ops.shadow_take): no cast of the [total, D] gradient
            return gy, None, None
        gin = None if last else ops.ragged_repack_bwd(g.contiguous(), keep, cu, ctx.cu_new, total, run.B)
        gy = ops.avit_halt_bwd(gin, h, cu, row_src, run.st, w, run.dacc, ycls, run.gsc, layer, run.gamma)
        return gy, None, None


class AViTPenaltyFn(torch.autograd.Function):
    """part [L, B, 3] (the last AViTHaltFn's second output), tgt [L] -> [2] = {ponder mean, distribution prior}.  The backward leaves the
    per-layer factors on the run for the halting steps' backward; `part` itself gets no gradient (it is a side product of the kernels)."""

    @staticmethod
    def forward(ctx, part, tgt, run):
        out, hbar, cnt = ops.avit_penalty_fwd(part, tgt, run.N)
        if DF.wants_grad(ctx):
            ctx.run, ctx.kept = run, (hbar, cnt, tgt)
        run.hbar, run.live_rows = hbar, cnt
        return out

    @staticmethod
    def backward(ctx, g):
        run = ctx.run
        hbar, cnt, tgt = ctx.kept
        g = g.contiguous()
        run.gsc = ops.avit_penalty_bwd(hbar, cnt, tgt, g[0:1], g[1:2], run.B, run.N)
        return None, None, None


def halt(y, run, layer):
    return DF.run(AViTHaltFn, y, run, layer)


def penalties(part, tgt, run):
    return DF.run(AViTPenaltyFn, part, tgt, run)
