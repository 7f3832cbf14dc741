"""GPU tier: the row moves (csrc/select.hip: d2s_copy_rows, d2s_assemble_tokens, d2s_batch_sum; csrc/gemm_f32.hip: d2s_transpose_f32).
These kernels move floats and add them in fp32 in a fixed order, so every check is bit-exact.

A row map is (rows_per_group, group_stride, row_stride, offset) in floats: row r lives at (r // rows_per_group) * group_stride + offset +
(r % rows_per_group) * row_stride.  The kernels trust their maps, so every buffer here has the size its map addresses and that is
asserted before the call; destination buffers carry a sentinel wherever the map does not reach."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_TOK = 3, 5
SENTINEL = -777.25


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from d2s import ops as _ops
    return _ops


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).float()


def _row_starts(m, rows):
    rpg, gs, rs, off = m
    r = np.arange(rows)
    return (r // rpg) * gs + off + (r % rpg) * rs


def _extent(m, rows, D):
    return int(_row_starts(m, rows).max()) + D


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _maps(ops, D):
    """(name, map, rows) of the views of a contiguous [B, n, D] buffer that the models use"""
    n = N_TOK
    return [("contiguous", ops.contiguous_map(B * n, D), B * n),
            ("skip_cls", ops.skip_cls_map(n, D), B * (n - 1)),
            ("skip_cls_tail1", ops.skip_cls_map(n, D, tail=1), B * (n - 2)),
            ("cls", (1, n * D, D, 0), B)]


@pytest.mark.parametrize("D", [4, 64, 384])
def test_copy_rows_source_maps(ops, D):
    x = _rand((B, N_TOK, D), D)
    xd = x.to(_dev())
    want = {"contiguous": x.reshape(-1, D), "skip_cls": x[:, 1:].reshape(-1, D), "skip_cls_tail1": x[:, 1:-1].reshape(-1, D), "cls": x[:, 0]}
    for name, m, rows in _maps(ops, D):
        assert all(v % 4 == 0 for v in m[1:]) and _extent(m, rows, D) <= xd.numel()
        got = ops.copy_rows(xd, m, rows, D)
        assert got.shape == (rows, D) and torch.equal(_bits(got), _bits(want[name])), name
        assert np.array_equal(x.reshape(-1).numpy()[_row_starts(m, rows)], want[name][:, 0].numpy())      # the map formula itself


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("D", [4, 64, 384])
def test_copy_rows_destination_maps(ops, D, accumulate):
    """contiguous rows into the same views of a [B, n, D] buffer: overwritten or added to (fp32 addition commutes, so old + new is exact);
    every element outside the view keeps its sentinel"""
    for name, m, rows in _maps(ops, D):
        src = _rand((rows, D), D + rows)
        old = _rand((B, N_TOK, D), 7 * D + rows) if accumulate else torch.full((B, N_TOK, D), SENTINEL)
        touched = torch.zeros(B * N_TOK * D, dtype=torch.bool)
        idx = torch.from_numpy(_row_starts(m, rows))[:, None] + torch.arange(D)[None, :]
        touched[idx.reshape(-1)] = True
        want = old.clone().reshape(-1)
        want[idx.reshape(-1)] = (old.reshape(-1)[idx.reshape(-1)] + src.reshape(-1)) if accumulate else src.reshape(-1)
        dst = old.clone().to(_dev())
        assert all(v % 4 == 0 for v in m[1:]) and _extent(m, rows, D) <= dst.numel()
        out = ops.copy_rows(src.to(_dev()), ops.contiguous_map(rows, D), rows, D, dst=dst, dst_map=m, accumulate=accumulate)
        assert out is dst and torch.equal(_bits(dst).reshape(-1), _bits(want)), name
        assert torch.equal(dst.cpu().reshape(-1)[~touched], old.reshape(-1)[~touched])


def test_copy_rows_both_maps_and_the_v_slice(ops):
    """a strided source into a strided destination, and the skip connection of the token transformer's backward: gy [M, 64] added into
    columns 128..191 of dqkv [M, 192] through the map (M, 0, 192, 128)"""
    D, n = 64, N_TOK
    x = _rand((B, n, D), 1)
    dst = torch.full((B, n, D), SENTINEL).to(_dev())
    sm, dm, rows = ops.skip_cls_map(n, D), ops.skip_cls_map(n, D, tail=1), B * (n - 2)
    assert _extent(dm, rows, D) <= x.numel() and _extent(dm, rows, D) <= dst.numel()
    ops.copy_rows(x.to(_dev()), dm, rows, D, dst=dst, dst_map=dm)
    want = torch.full((B, n, D), SENTINEL)
    want[:, 1:-1] = x[:, 1:-1]
    assert torch.equal(_bits(dst), _bits(want))
    # the CLS-less rows (four per image) into a buffer of exactly that many rows
    dst2 = torch.full((B, n - 1, D), SENTINEL).to(_dev())
    rows2 = B * (n - 1)
    assert _extent(sm, rows2, D) <= x.numel() and _extent(ops.contiguous_map(rows2, D), rows2, D) <= dst2.numel()
    ops.copy_rows(x.to(_dev()), sm, rows2, D, dst=dst2, dst_map=ops.contiguous_map(rows2, D))
    assert torch.equal(_bits(dst2), _bits(x[:, 1:]))
    M = 7
    gy, dqkv = _rand((M, 64), 2), _rand((M, 192), 3)
    vm = (M, 0, 192, 128)
    d = dqkv.clone().to(_dev())
    assert _extent(vm, M, 64) <= d.numel()
    ops.copy_rows(gy.to(_dev()), ops.contiguous_map(M, 64), M, 64, dst=d, dst_map=vm, accumulate=True)
    want = dqkv.clone()
    want[:, 128:] = dqkv[:, 128:] + gy
    assert torch.equal(_bits(d), _bits(want))


def test_copy_rows_rejects_unaligned(ops):
    """16-byte accesses: a width or a map term that is no multiple of 4 floats is refused before the launch"""
    from d2s import lib
    x = torch.zeros((4, 8), dtype=torch.float32, device=_dev())
    out = torch.full((4, 8), SENTINEL, device=_dev())
    with pytest.raises(lib.D2SError):
        ops.copy_rows(x, ops.contiguous_map(4, 6), 4, 6, dst=out)
    with pytest.raises(lib.D2SError):
        ops.copy_rows(x, (4, 0, 8, 2), 3, 4, dst=out)                        # source offset 2
    with pytest.raises(lib.D2SError):
        ops.copy_rows(x, ops.contiguous_map(3, 4), 3, 4, dst=out, dst_map=(3, 0, 6, 0))      # destination row stride 6
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("Bn,T,D", [(2, 1, 4), (3, 16, 128), (2, 196, 384)])
def test_assemble_tokens(Bn, T, D):
    """out = cat(cls, tok) + pos: one fp32 addition per element"""
    from d2s import lib
    tok, cls, pos = _rand((Bn, T, D), 1), _rand((1, 1, D), 2), _rand((1, T + 1, D), 3)
    out = torch.empty((Bn, T + 1, D), dtype=torch.float32, device=_dev())
    td, cd, pd = tok.to(_dev()), cls.to(_dev()), pos.to(_dev())
    lib.call("d2s_assemble_tokens", lib.ptr(td), lib.ptr(cd), lib.ptr(pd), lib.ptr(out), Bn, T, D)
    want = torch.cat([cls.expand(Bn, 1, D), tok], dim=1) + pos
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("Bn", [1, 5])
def test_batch_sum(ops, Bn):
    """The position-table and CLS-token gradients of the embedding's backward: out[e] = sum_b g[b, e] over a whole image (count = stride =
    (T + 1) D) and over its first row (count = D, same stride).  fp32, b ascending from 0, the old value added last."""
    T, D = 7, 36                                                    # 288 elements per image: two workgroups, the second ragged
    g = _rand((Bn, T + 1, D), Bn)
    gd = g.to(_dev())

    def ref(count, old):
        s = np.zeros(count, dtype=np.float32)
        for b in range(Bn):
            s = (s + g[b].reshape(-1).numpy()[:count]).astype(np.float32)
        return s if old is None else (old.numpy() + s).astype(np.float32)

    for count in ((T + 1) * D, D):
        stride = (T + 1) * D
        assert (Bn - 1) * stride + count <= gd.numel()
        out = torch.full((count + 8,), SENTINEL).to(_dev())
        ops.batch_sum(gd, out, Bn, count, stride)
        assert np.array_equal(out.cpu().numpy()[:count].view(np.uint32), ref(count, None).view(np.uint32))
        assert bool((out[count:] == SENTINEL).all())
        old = _rand((count,), 9 + count)
        acc = old.clone().to(_dev())
        ops.batch_sum(gd, acc, Bn, count, stride, accumulate=True)
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), ref(count, old).view(np.uint32))


@pytest.mark.parametrize("R_,C", [(1, 1), (5, 3), (64, 64), (65, 33), (384, 1536)])
def test_transpose_f32(R_, C):
    from d2s import lib
    src = _rand((R_, C), R_ * 7 + C)
    sd = src.to(_dev())
    dst = torch.full((C * R_ + 8,), SENTINEL).to(_dev())
    lib.call("d2s_transpose_f32", lib.ptr(sd), lib.ptr(dst), R_, C)
    assert torch.equal(_bits(dst[:C * R_].view(C, R_)), _bits(src.t().contiguous()))
    assert bool((dst[C * R_:] == SENTINEL).all())
