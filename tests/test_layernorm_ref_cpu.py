"""The yardstick of the LayerNorm kernel tests, tested: tests/layernorm_ref.py in float64 against F.layer_norm + autograd, its row
maps against tensor slicing, and the backward's row chunking rule that tests/test_layernorm_gpu.py picks its row counts from.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import layernorm_ref as R

SHAPES = [(1, 1), (3, 1), (1, 147), (5, 147), (7, 6), (33, 96), (4, 384), (2, 1028)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(rows, D, seed):
    g = _gen(seed)
    x = torch.randn(rows, D, generator=g, dtype=torch.float64) * 2 + 0.3
    w = 1 + 0.2 * torch.randn(D, generator=g, dtype=torch.float64)
    b = 0.2 * torch.randn(D, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, D, generator=g, dtype=torch.float64)
    return x, w, b, dy


def _close(got, want, tol=1e-12):
    assert got.dtype == torch.float64 and got.shape == want.shape
    scale = max(float(want.abs().max()), 1.0)
    assert float((got - want).abs().max()) <= tol * scale, float((got - want).abs().max())


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("rows,D", SHAPES)
def test_restatement_against_layer_norm_autograd(rows, D, eps):
    x, w, b, dy = _inputs(rows, D, rows * 10000 + D)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    ref = F.layer_norm(xr, (D,), wr, br, eps)
    gx, gw, gb = torch.autograd.grad(ref, (xr, wr, br), dy)
    y, mean, rstd = R.ln_fwd(x, w, b, eps)
    _close(y, ref.detach())
    _close(mean, x.mean(dim=1))
    _close(rstd, 1.0 / torch.sqrt(x.var(dim=1, unbiased=False) + eps), 1e-11)      # torch's variance, not the restatement's
    dx, dw, db = R.ln_bwd(x, dy, w, mean, rstd)
    # D = 1: the variance is 0 and rstd = eps^-1/2 amplifies the cancellation in dx (exactly 0 in exact arithmetic)
    _close(dx, gx, 1e-12 if D > 1 else 1e-9)
    _close(dw, gw)
    _close(db, gb)
    add = torch.randn(rows, D, generator=_gen(5), dtype=torch.float64)
    dx2, dw2, db2 = R.ln_bwd(x, dy, w, mean, rstd, add_rows=add)
    assert torch.equal(dx2, dx + add) and torch.equal(dw2, dw) and torch.equal(db2, db)


def test_restatement_d1_is_the_bias():
    x, w, b, dy = _inputs(4, 1, 11)
    y, mean, rstd = R.ln_fwd(x, w, b, 1e-5)
    assert torch.equal(y, b.expand(4, 1)) and torch.equal(mean, x[:, 0])
    assert torch.equal(rstd, torch.full((4,), 1.0 / torch.sqrt(torch.tensor(1e-5, dtype=torch.float64)).item(), dtype=torch.float64))
    assert torch.equal(R.ln_bwd(x, dy, w, mean, rstd)[0], torch.zeros(4, 1, dtype=torch.float64))


@pytest.mark.parametrize("rows,D", [(1, 1), (5, 147), (9, 96), (6, 384)])
def test_relu_mask_against_autograd_through_relu(rows, D):
    """relu_mask: x of the LayerNorm is relu(z); the masked dx is d/dz, and z == +0.0 and z == -0.0 both get no gradient"""
    z, w, b, dy = _inputs(rows, D, rows * 77 + D)
    flat = z.view(-1)
    flat[::5] = 0.0
    flat[2::7] = -0.0
    if D > 1:
        assert bool((flat == 0).any()) and bool((torch.signbit(flat) & (flat == 0)).any()) and bool((flat > 0).any())
    zr = z.clone().requires_grad_(True)
    ref = F.layer_norm(F.relu(zr), (D,), w, b, 1e-5)
    (gz,) = torch.autograd.grad(ref, zr, dy)
    x = F.relu(z)
    _, mean, rstd = R.ln_fwd(x, w, b, 1e-5)
    add = torch.randn(rows, D, generator=_gen(3), dtype=torch.float64)
    dx, dw, db = R.ln_bwd(x, dy, w, mean, rstd, relu_mask=True)
    _close(dx, gz, 1e-12 if D > 1 else 1e-9)
    assert bool((dx.view(-1)[flat <= 0] == 0).all())
    dx_add, dw2, db2 = R.ln_bwd(x, dy, w, mean, rstd, add_rows=add, relu_mask=True)
    assert torch.equal(dx_add, dx + add), "the mask applies before the add"
    xhat = (x - mean[:, None]) * rstd[:, None]
    _close(dw, (dy * xhat).sum(0))
    assert torch.equal(dw, dw2) and torch.equal(db, dy.sum(0)) and torch.equal(db, db2)      # the mask does not touch dw / db


@pytest.mark.parametrize("n,D", [(6, 8), (7, 147), (2, 4)])
def test_row_maps_against_slicing(n, D):
    from d2s import ops
    B = 3
    buf = torch.randn(B, n, D, generator=_gen(n * D), dtype=torch.float64)
    views = [(R.contiguous_map(B * n, D), buf.reshape(-1, D), ops.contiguous_map(B * n, D)),
             (R.skip_cls_map(n, D), buf[:, 1:].reshape(-1, D), ops.skip_cls_map(n, D))]
    if n > 2:
        views.append((R.skip_cls_map(n, D, tail=1), buf[:, 1:n - 1].reshape(-1, D), ops.skip_cls_map(n, D, tail=1)))
    for m, want, ops_map in views:
        assert tuple(m) == tuple(ops_map)
        rows = want.shape[0]
        assert R.map_extent(m, rows, D) <= buf.numel()
        assert torch.equal(R.map_rows(buf, m, rows, D), want)
        new = torch.randn(rows, D, generator=_gen(1), dtype=torch.float64)
        out = R.scatter_rows(buf, m, new)
        assert out.shape == buf.shape and torch.equal(R.map_rows(out, m, rows, D), new)
    # what the maps leave out stays: CLS rows, and with tail=1 the last row of every image
    new = torch.full((B * (n - 1), D), 7.0, dtype=torch.float64)
    out = R.scatter_rows(buf, R.skip_cls_map(n, D), new)
    assert torch.equal(out[:, 0], buf[:, 0]) and bool((out[:, 1:] == 7.0).all())
    if n > 2:
        out = R.scatter_rows(buf, R.skip_cls_map(n, D, tail=1), new[:B * (n - 2)])
        assert torch.equal(out[:, 0], buf[:, 0]) and torch.equal(out[:, -1], buf[:, -1]) and bool((out[:, 1:-1] == 7.0).all())


def test_unaligned_map_against_slicing():
    rows, D = 5, 8
    flat = torch.arange(1 + rows * (D + 1), dtype=torch.float64)
    m = (rows, 0, D + 1, 1)
    want = flat[1:].view(rows, D + 1)[:, :D]
    assert torch.equal(R.map_rows(flat, m, rows, D), want)
    out = R.scatter_rows(flat, m, -want)
    assert torch.equal(out[1:].view(rows, D + 1)[:, :D], -want) and torch.equal(out[1:].view(rows, D + 1)[:, D], flat[1:].view(rows, D + 1)[:, D])
    assert out[0] == flat[0]


def test_backward_chunking_rule():
    """blocks = min(768, ceil(rows / 32)), rows per block = ceil(rows / blocks).  The GPU cases pick 2081 rows for "more than 64
    partials in the fold" and 24577 rows for "a block owns more than 32 rows"; if the rule is retuned, move those shapes."""
    assert R.bwd_chunking(2081) == (66, 32)
    assert R.bwd_chunking(2048) == (64, 32)                  # the last row count with at most 64 partials
    assert R.bwd_chunking(24577) == (745, 33)
    assert R.bwd_chunking(24576) == (768, 32)                # the last row count at which a block owns 32 rows
    assert R.bwd_chunking(128 * 197) == (765, 33)            # DeiT-S at batch 128: the benchmark's shape is in the capped regime
    for rows in (1, 2, 3, 5, 33, 77):
        blocks, per = R.bwd_chunking(rows)
        assert per <= 32 and blocks <= 3 and (blocks - 1) * per < rows <= blocks * per
    # the workspace the entry asks for covers the partials of every launched block
    for rows in (1, 33, 2081, 24577, 100000):
        blocks, per = R.bwd_chunking(rows)
        assert blocks <= min(768, -(-rows // 32)) and blocks * per >= rows
