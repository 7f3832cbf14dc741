"""Evo-ViT (Xu et al. 2022; DESIGN.md section 26 - the build's own definition, PARITY UNPINNED): the slow-fast token update.  A slow-fast
block keeps the full token tensor X [B, 1+T, D]; it runs the ordinary block on xc = [CLS | the k tokens of the highest global score | one
representative row r of the rest] and writes the result back into X, the other rows moving by (y_r - r).

Two Functions surround the block and they form a CHAIN, not two branches that meet at X:

    EvoGatherFn(X)                 -> (xc, Xa)      Xa is X again, an alias that carries this Function's node
    BlockFn(xc)                    -> (yc, cls row)
    EvoScatterFn(yc, Xa, xc)       -> X'            Xa updated in place and marked dirty

so the backward of a block is  scatter (dX' -> dyc; dX' itself goes on as the gradient of Xa), block (dyc -> dxc), gather (dxc and the
buffer dX' -> dX, in place).  No full-size add is issued, no copy of X is saved: a block keeps xc (BlockFn saves it anyway), g, S and the
id lists.  The alias is X.detach(): it shares X's storage AND version counter, so autograd still sees the in-place write (nothing saves
X: EvoGatherFn's backward is linear in the gradients for fixed weights) and no copy of X is needed anywhere, the first block included.

g, the selection and the weights g_j / S carry no gradient."""
import torch

from . import functional as DF
from . import ops


class EvoLink:
    """What the two Functions of one slow-fast block share in the backward: dyc, whose last row is delta (the gather's backward reads it)."""
    __slots__ = ("dyc",)

    def __init__(self):
        self.dyc = None


class EvoGatherFn(torch.autograd.Function):
    """X [B,1+T,D], g [B,T], kept [B,k], dropped [B,T-k] -> (xc [B,k+2,D] = ops.gather_fuse_fwd(X, g, kept, dropped, 0), X aliased)."""

    @staticmethod
    def forward(ctx, X, g, kept, dropped, link):
        assert X.is_contiguous(), "the slow-fast update writes X in place: it must be contiguous"
        xc, S = ops.gather_fuse_fwd(X, g, kept, dropped, 0)
        if DF.wants_grad(ctx):
            ctx.save_for_backward(g, S, kept, dropped)
            ctx.link = link
        return xc, X.detach()

    @staticmethod
    def backward(ctx, dxc, dX):
        g, S, kept, dropped = ctx.saved_tensors
        link = ctx.link
        dyc, link.dyc = link.dyc, None
        return ops.evo_gather_bwd(dX.contiguous(), dxc.contiguous(), dyc, g, S, kept, dropped), None, None, None, None


class EvoScatterFn(torch.autograd.Function):
    """yc [B,k+2,D], Xa (EvoGatherFn's second output), xc, the id lists -> Xa written back in place (ops.evo_scatter_fwd).  The gradient of
    xc - minus delta on its last row - is applied by EvoGatherFn's backward, which owns that row's weights."""

    @staticmethod
    def forward(ctx, yc, Xa, xc, kept, dropped, link):
        ops.evo_scatter_fwd(Xa, yc.contiguous(), xc, kept, dropped)
        ctx.mark_dirty(Xa)
        if DF.wants_grad(ctx):
            ctx.save_for_backward(kept, dropped)
            ctx.link = link
        return Xa

    @staticmethod
    def backward(ctx, dX):
        kept, dropped = ctx.saved_tensors
        dX = dX.contiguous()
        ctx.link.dyc = dyc = ops.evo_scatter_bwd(dX, kept, dropped)
        return dyc, dX, None, None, None, None


def slow_fast_block(X, g, kept, dropped, block):
    """One slow-fast block on X in place.  block(xc) -> (yc, cls_row [B,H,k+2]).  -> (X, cls_row)"""
    link = EvoLink()
    xc, Xa = DF.run(EvoGatherFn, X, g, kept, dropped, link)
    yc, cls_row = block(xc)
    return DF.run(EvoScatterFn, yc, Xa, xc, kept, dropped, link), cls_row
