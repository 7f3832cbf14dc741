"""Plain torch restatement of LayerNorm and its gradient (csrc/layernorm.hip), written from the formulas of nn.LayerNorm and not from
the kernels.  Nothing here imports the package under test.

Every function works in the dtype of its tensor arguments, like tests/losspath_ref.py: with float64 inputs it is the reference of the
kernel tests, with the same inputs in float32 it is their yardstick.  eps is a Python float; a test hands in the value the C ABI
receives, i.e. already rounded to fp32.

A row map is (rows_per_group, group_stride, row_stride, offset) in elements: logical row r of a flat buffer starts at
(r // rows_per_group) * group_stride + offset + (r % rows_per_group) * row_stride."""
import torch

from tests.losspath_ref import ERR_FACTOR, ERR_FLOOR, rel_err  # noqa: F401  (the error measure and the acceptance rule's constants)

BWD_MAX_BLOCKS, BWD_ROWS_PER_BLOCK = 768, 32      # the documented chunking rule of the backward (LayerNorm row)


# ---------------------------------------------------------------------------------------------------------------- row maps
def contiguous_map(rows, D):
    return (rows, 0, D, 0)


def skip_cls_map(n, D, tail=0):
    """rows 1 .. n - 1 - tail of every image of a contiguous [B, n, D] buffer"""
    return (n - 1 - tail, n * D, D, D)


def row_starts(rowmap, rows):
    rpg, gs, rs, off = rowmap
    r = torch.arange(rows, dtype=torch.int64)
    return (r // rpg) * gs + off + (r % rpg) * rs


def map_extent(rowmap, rows, D):
    """number of elements a buffer must have for the map to stay inside it"""
    return int(row_starts(rowmap, rows).max()) + D


def _index(rowmap, rows, D):
    return row_starts(rowmap, rows)[:, None] + torch.arange(D, dtype=torch.int64)[None, :]


def map_rows(buf, rowmap, rows, D):
    """the [rows, D] logical rows of `buf` (any shape, read flat) under the map; a copy"""
    flat = buf.reshape(-1)
    assert map_extent(rowmap, rows, D) <= flat.numel(), (rowmap, rows, D, flat.numel())
    return flat[_index(rowmap, rows, D)]


def scatter_rows(buf, rowmap, rows_t):
    """the inverse of map_rows: a copy of `buf` whose mapped rows are rows_t [rows, D]; everything else as it was"""
    rows, D = rows_t.shape
    out = buf.clone()
    flat = out.view(-1)
    assert map_extent(rowmap, rows, D) <= flat.numel(), (rowmap, rows, D, flat.numel())
    flat[_index(rowmap, rows, D)] = rows_t.to(out.dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd(x_rows, w, b, eps):
    """-> (y [rows, D], mean [rows], rstd [rows]); two passes: the mean, then the mean of the squared deviations (biased variance)"""
    mean = x_rows.mean(dim=1)
    dev = x_rows - mean[:, None]
    var = (dev * dev).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return dev * rstd[:, None] * w + b, mean, rstd


def ln_bwd(x_rows, dy, w, mean, rstd, add_rows=None, relu_mask=False):
    """-> (dx_rows, dw, db) of y = xhat * w + b, xhat = (x - mean) * rstd, from the saved statistics:
         dx = rstd * (dy w - mean_D(dy w) - xhat * mean_D(dy w xhat))
       times [x > 0] when relu_mask (x is then the output of a ReLU and dx the gradient of its input), plus add_rows;
       dw = sum_r dy xhat, db = sum_r dy."""
    xhat = (x_rows - mean[:, None]) * rstd[:, None]
    g = dy * w
    dx = rstd[:, None] * (g - g.mean(dim=1, keepdim=True) - xhat * (g * xhat).mean(dim=1, keepdim=True))
    if relu_mask:
        dx = dx * (x_rows > 0).to(dx.dtype)
    if add_rows is not None:
        dx = dx + add_rows
    return dx, (dy * xhat).sum(0), dy.sum(0)


# ---------------------------------------------------------------------------------------------------------------- backward chunking
def bwd_chunking(rows):
    """-> (blocks launched, rows per block) of the backward: min(768, ceil(rows / 32)) blocks are asked for, a block owns
    ceil(rows / blocks) consecutive rows, and as many blocks as that chunk needs are launched (= the number of dw / db partials
    the fold adds)"""
    asked = max(1, min(BWD_MAX_BLOCKS, -(-rows // BWD_ROWS_PER_BLOCK)))
    per_block = -(-rows // asked)
    return -(-rows // per_block), per_block
