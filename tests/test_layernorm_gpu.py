"""GPU tier: every dispatch branch of csrc/layernorm.hip against the float64 restatement of tests/layernorm_ref.py.

The host code picks a kernel from the width D (scalar kernels for D % 4 != 0, the two-rows-per-wave pair kernels at D = 384,
ln_*_kernel<NV> with NV = 1, 2, 4, 8, 16 from D = 4, 260, 516, 1028, 2052), from the alignment of the row map (a stride or offset that
is no multiple of 4 forces the scalar kernels) and, in the backward, from the row count: min(768, ceil(rows / 32)) blocks of
ceil(rows / blocks) rows each, whose dw / db partials a fold kernel adds 64 at a time (tests/test_layernorm_ref_cpu.py restates the rule).

Acceptance of every floating-point output (y, mean, rstd, dx, dw, db), over the whole tensor:
    rel_err(kernel, ref64) <= max(ERR_FACTOR * rel_err(restatement in fp32, ref64), ERR_FLOOR).
Kernel and fp32 restatement start from the same fp32 inputs; the backward is fed the statistics the kernel's own forward wrote, as the
model does, the fp32 yardstick uses its own fp32 statistics.  Copies and roundings (the bf16 outputs, stats=False, rows outside a map)
are bit-exact.  Every case prints its worst ratio kernel error / yardstick error."""
import math

import pytest
import torch

from tests import layernorm_ref as R
from tests.losspath_ref import assert_close_as_fp32

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SCALAR_D = [1, 6, 130, 147]
VECTOR_D = [4, 96, 256, 260, 384, 512, 516, 768, 1024, 1028, 2048, 2052, 4096]
DISPATCH = [(D, rows) for D in SCALAR_D + VECTOR_D for rows in ((1, 2, 3, 5, 33) if D in (147, 96, 384) else (5, 33))]


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from d2s import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from d2s import lib as _lib
    return _lib


def _f32(v):
    """the value the C ABI receives for a float argument"""
    return float(torch.tensor(v, dtype=torch.float32))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _inputs(rows, D, seed, shape=None, integer_dy=False):
    """x ~ 2 N(0,1) + 0.3 (in `shape` when the rows live in a larger buffer), w ~ 1 + 0.2 N, b ~ 0.2 N, dy ~ N(0,1) or uniform on
    {-1, 0, 1}, add ~ N(0,1) shaped like x"""
    g = _gen(rows, D, seed)
    shape = (rows, D) if shape is None else shape
    x = torch.randn(shape, generator=g) * 2 + 0.3
    w = 1 + 0.2 * torch.randn(D, generator=g)
    b = 0.2 * torch.randn(D, generator=g)
    dy = torch.randint(-1, 2, (rows, D), generator=g).float() if integer_dy else torch.randn(rows, D, generator=g)
    add = torch.randn(shape, generator=g)
    return x, w, b, dy, add


class _Worst:
    """collects err_hip / err_cpu32 of a case's outputs and prints the largest"""

    def __init__(self, what):
        self.what, self.worst, self.name = what, 0.0, "-"

    def check(self, name, got, ref64, ref32):
        ratio = assert_close_as_fp32(f"{self.what} {name}", got.cpu(), ref64, ref32)
        if ratio > self.worst:
            self.worst, self.name = ratio, name
        return ratio

    def report(self):
        print(f"[layernorm] {self.what}: worst ratio {self.worst:.2f} ({self.name})")


def _fwd_refs(x_rows, w, b, eps):
    return R.ln_fwd(x_rows.double(), w.double(), b.double(), eps), R.ln_fwd(x_rows, w, b, eps)


def _bwd_refs(x_rows, dy, w, b, eps, add_rows=None, relu_mask=False):
    """float64 backward from float64 statistics, fp32 backward from its own fp32 statistics"""
    x64, w64 = x_rows.double(), w.double()
    _, m64, r64 = R.ln_fwd(x64, w64, b.double(), eps)
    _, m32, r32 = R.ln_fwd(x_rows, w, b, eps)
    ref64 = R.ln_bwd(x64, dy.double(), w64, m64, r64, None if add_rows is None else add_rows.double(), relu_mask)
    ref32 = R.ln_bwd(x_rows, dy, w, m32, r32, add_rows, relu_mask)
    return ref64, ref32


def _check_fwd(worst, got, refs):
    for name, g, r64, r32 in zip(("y", "mean", "rstd"), got, *refs):
        worst.check(name, g, r64, r32)


def _check_bwd(worst, got, refs, names=("dx", "dw", "db")):
    for name, g, r64, r32 in zip(("dx", "dw", "db"), got, *refs):
        if name in names:
            worst.check(name, g, r64, r32)


# ------------------------------------------------------------------------------------------------ dispatch by width
@pytest.mark.parametrize("D,rows", DISPATCH)
def test_dispatch_fwd_bwd(ops, D, rows):
    """every kernel family and every NV at both sides of its boundary, rows below / above one block of four waves, both eps the models
    use; contiguous map, add_src given, dw / db wanted.  Forward also with stats=False and, where D % 4 == 0, through the bf16 entry."""
    x, w, b, dy, add = _inputs(rows, D, 1)
    xd, wd, bd, dyd, addd = (t.to(_dev()) for t in (x, w, b, dy, add))
    cmap = ops.contiguous_map(rows, D)
    assert tuple(cmap) == R.contiguous_map(rows, D)
    for eps in (_f32(1e-6), _f32(1e-5)):
        worst = _Worst(f"dispatch D={D} rows={rows} eps={eps:.0e}")
        y, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
        refs = _fwd_refs(x, w, b, eps)
        _check_fwd(worst, (y, mean, rstd), refs)
        if D == 1:      # the variance is 0: y = b and rstd = eps^-1/2, whatever x
            assert torch.equal(y.cpu(), b.expand(rows, 1)) and torch.equal(mean.cpu(), x[:, 0])
            assert float((rstd.cpu().double() * math.sqrt(eps) - 1).abs().max()) <= 3e-7
        y2, m2, r2 = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps, stats=False)
        assert m2 is None and r2 is None and _same_bits(y2, y), "stats=False changes y"
        if D % 4 == 0:
            y3, m3, r3, y16 = ops.layernorm_fwd_bf16(xd, cmap, wd, bd, rows, D, eps)
            assert _same_bits(y3, y) and _same_bits(m3, mean) and _same_bits(r3, rstd)
            assert y16.dtype == torch.bfloat16 and _same_bits(y16, y.bfloat16())
            y4, m4, r4, y16b = ops.layernorm_fwd_bf16(xd, cmap, wd, bd, rows, D, eps, stats=False, want_f32=False)
            assert y4 is None and m4 is None and _same_bits(y16b, y16)
        dx = torch.full((rows, D), SENTINEL, device=_dev())
        dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
        ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx, addd, dw, db, rows, D)
        _check_bwd(worst, (dx, dw, db), _bwd_refs(x, dy, w, b, eps, add))
        if D % 4 == 0:
            dx2, dw2, db2 = torch.empty_like(dx), torch.empty_like(dw), torch.empty_like(db)
            dx16 = torch.empty((rows, D), dtype=torch.bfloat16, device=_dev())
            ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx2, addd, dw2, db2, rows, D, dx16=dx16)
            assert _same_bits(dx2, dx) and _same_bits(dw2, dw) and _same_bits(db2, db) and _same_bits(dx16, dx.bfloat16())
        worst.report()


# ------------------------------------------------------------------------------------------------ row count regimes
@pytest.mark.parametrize("D", [96, 384, 147])
@pytest.mark.parametrize("rows", [2081, 24577])
def test_row_count_regimes(ops, lib, rows, D):
    """2081 rows: 66 partial blocks, so the fold's strided loop takes a second trip; 24577 rows: the block count is capped at 768 and a
    block owns 33 rows (the regime of DeiT-S at batch 128).  Through the pipelined vector loop (D = 96), the pair kernel (384) and the
    scalar kernel (147).  dy is drawn from {-1, 0, 1}: db is a sum of small integers, exact in fp32 in any order, and must be bit-exact -
    every row exactly once, whatever the tolerance of dw."""
    blocks, per_block = R.bwd_chunking(rows)
    assert (blocks > 64 and per_block == 32) if rows == 2081 else (blocks <= 768 and per_block > 32)
    asked = min(R.BWD_MAX_BLOCKS, -(-rows // R.BWD_ROWS_PER_BLOCK))
    assert lib.query("d2s_layernorm_bwd_workspace_bytes", rows, D) == asked * 2 * D * 4, "the chunking rule moved: see test_layernorm_ref_cpu"
    x, w, b, dy, add = _inputs(rows, D, 2, integer_dy=True)
    eps = _f32(1e-6)
    xd, wd, bd = x.to(_dev()), w.to(_dev()), b.to(_dev())
    cmap = ops.contiguous_map(rows, D)
    worst = _Worst(f"rows={rows} D={D}")
    y, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
    _check_fwd(worst, (y, mean, rstd), _fwd_refs(x, w, b, eps))
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
    ops.layernorm_bwd(xd, cmap, dy.to(_dev()), wd, mean, rstd, dx, add.to(_dev()), dw, db, rows, D)
    want_db = dy.double().sum(0)
    assert float(want_db.abs().max()) < 2 ** 24 and torch.equal(db.cpu().double(), want_db), "db: a row dropped or counted twice"
    _check_bwd(worst, (dx, dw, db), _bwd_refs(x, dy, w, b, eps, add))
    worst.report()


# ------------------------------------------------------------------------------------------------ flags
FLAG_D, FLAG_ROWS = [147, 192, 384], 77


def _flag_case(D, zeros):
    x, w, b, dy, add = _inputs(FLAG_ROWS, D, 3)
    if zeros:      # about 1 % of the entries exactly +0.0 and 1 % exactly -0.0
        g = _gen(D, 99)
        u = torch.rand(x.shape, generator=g)
        x[u < 0.01] = 0.0
        x[u > 0.99] = -0.0
        assert int((x == 0).sum()) > 0 and int(((x == 0) & torch.signbit(x)).sum()) > 0 and int(((x == 0) & ~torch.signbit(x)).sum()) > 0
    return x, w, b, dy, add


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("D", FLAG_D)
def test_relu_mask(ops, D, with_add):
    """relu_mask: dx is zero wherever x <= 0, +0.0 and -0.0 included, and the mask applies BEFORE add_src is added; dw / db see no mask"""
    x, w, b, dy, add = _flag_case(D, zeros=True)
    rows, eps = FLAG_ROWS, _f32(1e-5)
    xd, wd, bd = x.to(_dev()), w.to(_dev()), b.to(_dev())
    cmap = ops.contiguous_map(rows, D)
    worst = _Worst(f"relu_mask D={D} add={with_add}")
    _, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
    ops.layernorm_bwd(xd, cmap, dy.to(_dev()), wd, mean, rstd, dx, add.to(_dev()) if with_add else None, dw, db, rows, D, relu_mask=True)
    _check_bwd(worst, (dx, dw, db), _bwd_refs(x, dy, w, b, eps, add if with_add else None, relu_mask=True))
    off = x <= 0
    want_off = add[off] if with_add else torch.zeros(int(off.sum()))
    assert torch.equal(dx.cpu()[off], want_off), "masked entries: exactly add_src (or 0)"
    if D % 4 == 0:
        dx2 = torch.empty_like(dx)
        dx16 = torch.empty((rows, D), dtype=torch.bfloat16, device=_dev())
        ops.layernorm_bwd(xd, cmap, dy.to(_dev()), wd, mean, rstd, dx2, add.to(_dev()) if with_add else None, None, None, rows, D,
                          relu_mask=True, dx16=dx16)
        assert _same_bits(dx2, dx) and _same_bits(dx16, dx.bfloat16())
    worst.report()


@pytest.mark.parametrize("D", FLAG_D)
def test_accumulate_wb(ops, D):
    """accumulate_wb: dw / db are added to what the buffers hold"""
    x, w, b, dy, add = _flag_case(D, zeros=False)
    rows, eps = FLAG_ROWS, _f32(1e-6)
    g = _gen(D, 5)
    dw0, db0 = torch.randn(D, generator=g) * 3, torch.randn(D, generator=g) * 3
    xd, wd, bd = x.to(_dev()), w.to(_dev()), b.to(_dev())
    cmap = ops.contiguous_map(rows, D)
    worst = _Worst(f"accumulate_wb D={D}")
    _, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = dw0.to(_dev()), db0.to(_dev())
    ops.layernorm_bwd(xd, cmap, dy.to(_dev()), wd, mean, rstd, dx, add.to(_dev()), dw, db, rows, D, accumulate_wb=True)
    (dx64, dw64, db64), (dx32, dw32, db32) = _bwd_refs(x, dy, w, b, eps, add)
    _check_bwd(worst, (dx, dw, db), ((dx64, dw0.double() + dw64, db0.double() + db64), (dx32, dw0 + dw32, db0 + db32)))
    worst.report()


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("D", FLAG_D)
def test_no_weight_gradients(ops, lib, D, with_add):
    """dw = db = NULL: dx as before (bit for bit), and the C ABI then needs no workspace; dw without db is an argument error"""
    x, w, b, dy, add = _flag_case(D, zeros=False)
    rows, eps = FLAG_ROWS, _f32(1e-6)
    xd, wd, bd, dyd = x.to(_dev()), w.to(_dev()), b.to(_dev()), dy.to(_dev())
    addd = add.to(_dev()) if with_add else None
    cmap = ops.contiguous_map(rows, D)
    worst = _Worst(f"no dw/db D={D} add={with_add}")
    _, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx, addd, None, None, rows, D)
    _check_bwd(worst, (dx, None, None), _bwd_refs(x, dy, w, b, eps, add if with_add else None), names=("dx",))
    dx_ws = torch.full((rows, D), SENTINEL, device=_dev())
    lib.call("d2s_layernorm_bwd", lib.ptr(xd), *cmap, lib.ptr(dyd), lib.ptr(wd), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx_ws), lib.ptr(addd),
             None, None, 0, 0, rows, D, None, 0)
    assert _same_bits(dx_ws, dx), "dx without a workspace differs"
    dx_full = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = torch.empty((D,), device=_dev()), torch.empty((D,), device=_dev())
    ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx_full, addd, dw, db, rows, D)
    assert _same_bits(dx_full, dx), "dx depends on whether dw / db are wanted"
    dx_err = torch.full((rows, D), SENTINEL, device=_dev())
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx_err, addd, dw, None, rows, D)
    torch.cuda.synchronize()
    assert bool((dx_err == SENTINEL).all()), "a refused call wrote dx"
    worst.report()


# ------------------------------------------------------------------------------------------------ row maps
def _mapped_mask(numel, rowmap, rows, D):
    m = torch.zeros(numel, dtype=torch.bool)
    m[(R.row_starts(rowmap, rows)[:, None] + torch.arange(D)[None, :]).reshape(-1)] = True
    return m


def _rowmap_case(ops, what, xbuf, gbuf, rowmap, rows, D, w, b, dy, eps, bf16):
    """forward from the mapped rows of xbuf; backward with dx and add_src both the gradient buffer gbuf (the predictor's in-place add);
    whatever the map does not address keeps its bits; with bf16 also the dense dx16 copy by logical row"""
    assert R.map_extent(rowmap, rows, D) <= xbuf.numel() == gbuf.numel()
    worst = _Worst(what)
    x_rows, add_rows = R.map_rows(xbuf, rowmap, rows, D), R.map_rows(gbuf, rowmap, rows, D)
    xd, wd, bd, dyd = xbuf.to(_dev()), w.to(_dev()), b.to(_dev()), dy.to(_dev())
    y, mean, rstd = ops.layernorm_fwd(xd, rowmap, wd, bd, rows, D, eps)
    _check_fwd(worst, (y, mean, rstd), _fwd_refs(x_rows, w, b, eps))
    assert _same_bits(xd, xbuf)
    refs = _bwd_refs(x_rows, dy, w, b, eps, add_rows)
    mapped = _mapped_mask(gbuf.numel(), rowmap, rows, D)
    assert int(mapped.sum()) == rows * D and int((~mapped).sum()) > 0
    results = []
    for with16 in ((False, True) if bf16 else (False,)):
        gd = gbuf.to(_dev())
        dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
        dx16 = torch.full((rows, D), SENTINEL, dtype=torch.bfloat16, device=_dev()) if with16 else None
        ops.layernorm_bwd(xd, rowmap, dyd, wd, mean, rstd, gd, gd, dw, db, rows, D, dx16=dx16)
        after = gd.cpu()
        dx_rows = R.map_rows(after, rowmap, rows, D)
        _check_bwd(worst, (dx_rows, dw, db), refs)
        assert torch.equal(_bits(after).reshape(-1)[~mapped], _bits(gbuf).reshape(-1)[~mapped]), "a row outside the map was written"
        if with16:
            assert _same_bits(dx16, dx_rows.bfloat16()), "dx16 is the dense copy of dx by logical row"
        results.append((after, dw.cpu(), db.cpu()))
    if bf16:
        assert all(_same_bits(p, q) for p, q in zip(*results)), "the bf16out entry changes the fp32 outputs"
    worst.report()


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("D", [128, 384])
def test_skip_cls_row_maps(ops, D, n, tail):
    """x[:, 1:n - tail] of a [B, n, D] buffer: n - 1 - tail rows per image, odd and even, so that at D = 384 the two rows of a pair lie
    in different images; CLS rows and, with tail = 1, the last row of every image are not written"""
    B = 3
    rows = B * (n - 1 - tail)
    rowmap = ops.skip_cls_map(n, D, tail=tail)
    assert tuple(rowmap) == R.skip_cls_map(n, D, tail)
    xbuf, w, b, dy, gbuf = _inputs(rows, D, 10 * n + tail, shape=(B, n, D))
    _rowmap_case(ops, f"skip_cls D={D} n={n} tail={tail}", xbuf, gbuf, rowmap, rows, D, w, b, dy, _f32(1e-5), bf16=True)


def test_unaligned_map_takes_the_scalar_path(ops):
    """row stride D + 1 and offset 1 over a flat buffer: D = 128 is a multiple of 4, the addresses are not, so the scalar kernels must
    run; the bf16 entries have no scalar form and must refuse, writing nothing"""
    rows, D = 9, 128
    rowmap = (rows, 0, D + 1, 1)
    xbuf, w, b, dy, gbuf = _inputs(rows, D, 4, shape=(1 + rows * (D + 1),))
    eps = _f32(1e-5)
    _rowmap_case(ops, f"unaligned map D={D}", xbuf, gbuf, rowmap, rows, D, w, b, dy, eps, bf16=False)
    _bf16_entries_refuse(ops, xbuf, gbuf, rowmap, rows, D, w, b, dy, eps)


def test_bf16_entries_refuse_odd_width(ops):
    rows, D = 5, 147
    xbuf, w, b, dy, gbuf = _inputs(rows, D, 5)
    _bf16_entries_refuse(ops, xbuf, gbuf, ops.contiguous_map(rows, D), rows, D, w, b, dy, _f32(1e-5))


def _bf16_entries_refuse(ops, xbuf, gbuf, rowmap, rows, D, w, b, dy, eps):
    xd, wd, bd, dyd, gd = (t.to(_dev()) for t in (xbuf, w, b, dy, gbuf))
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd_bf16(xd, rowmap, wd, bd, rows, D, eps)
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd_bf16(xd, rowmap, wd, bd, rows, D, eps, want_f32=False)
    _, mean, rstd = ops.layernorm_fwd(xd, rowmap, wd, bd, rows, D, eps)
    dx16 = torch.full((rows, D), SENTINEL, dtype=torch.bfloat16, device=_dev())
    dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(xd, rowmap, dyd, wd, mean, rstd, gd, gd, dw, db, rows, D, dx16=dx16)
    torch.cuda.synchronize()
    assert _same_bits(gd, gbuf) and bool((dx16 == SENTINEL).all()) and bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ entry limits
def test_entry_limits(ops):
    """D = 4096 is the widest row (test_dispatch_fwd_bwd runs it), D = 4097 and rows = 0 are argument errors that write nothing"""
    rows, D = 5, 4097
    x, w, b, dy, add = _inputs(rows, D, 6)
    xd, wd, bd, dyd = x.to(_dev()), w.to(_dev()), b.to(_dev()), dy.to(_dev())
    cmap = ops.contiguous_map(rows, D)
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, 1e-5)
    stat = torch.ones(rows, device=_dev())
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(xd, cmap, dyd, wd, stat, stat, dx, None, dw, db, rows, D)
    D = 96
    x, w, b, dy, add = _inputs(rows, D, 6)
    xd, wd, bd, dyd = x.to(_dev()), w.to(_dev()), b.to(_dev()), dy.to(_dev())
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd(xd, (1, 0, D, 0), wd, bd, 0, D, 1e-5)
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd_bf16(xd, (1, 0, D, 0), wd, bd, 0, D, 1e-5)
    dx96 = torch.full((rows, D), SENTINEL, device=_dev())
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(xd, (1, 0, D, 0), dyd, wd, stat, stat, dx96, None, None, None, 0, D)
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all()) and bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all()) and bool((dx96 == SENTINEL).all())


def test_wide_scalar_backward_is_refused(ops):
    """D = 4094: the scalar backward would need 4 * 2 * D floats = 131 KB of LDS.  include/d2s_hip.h: the scalar backward supports
    D <= 2048 and refuses wider rows with an argument error before anything is launched; the forward has no such limit.  D = 2046, the
    widest the scalar backward takes (64 KB less 64 B of LDS), gives the right answer."""
    rows = 5
    for D, refused in ((4094, True), (2046, False)):
        x, w, b, dy, add = _inputs(rows, D, 7)
        eps = _f32(1e-5)
        xd, wd, bd, dyd, addd = (t.to(_dev()) for t in (x, w, b, dy, add))
        cmap = ops.contiguous_map(rows, D)
        worst = _Worst(f"scalar D={D}")
        y, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
        _check_fwd(worst, (y, mean, rstd), _fwd_refs(x, w, b, eps))
        dx = torch.full((rows, D), SENTINEL, device=_dev())
        dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
        if refused:
            for dwb in ((dw, db), (None, None)):
                with pytest.raises(RuntimeError, match="code -1"):      # D2S_ERR_ARG, not D2S_ERR_LAUNCH (-3)
                    ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx, addd, *dwb, rows, D)
            torch.cuda.synchronize()
            assert bool((dx == SENTINEL).all()) and bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())
        else:
            ops.layernorm_bwd(xd, cmap, dyd, wd, mean, rstd, dx, addd, dw, db, rows, D)
            _check_bwd(worst, (dx, dw, db), _bwd_refs(x, dy, w, b, eps, add))
        worst.report()


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("D", [147, 384, 768])
def test_large_mean_small_spread(ops, D):
    """x = 1000 + 0.5 N(0,1): the variance must come from the squared deviations (two passes).  E[x^2] - mean^2 in fp32 loses all of
    it at this offset (x^2 = 1e6 has an ulp of 0.06 against a variance of 0.25) - off by tens of percent or NaN - while the two-pass
    fp32 yardstick is about 1e-4 from float64, the rounding of the mean against the spread."""
    rows, eps = 64, _f32(1e-6)
    x, w, b, dy, add = _inputs(rows, D, 8)
    x = 1000.0 + 0.5 * torch.randn(rows, D, generator=_gen(D, 1000))
    xd, wd, bd = x.to(_dev()), w.to(_dev()), b.to(_dev())
    cmap = ops.contiguous_map(rows, D)
    worst = _Worst(f"conditioning D={D}")
    y, mean, rstd = ops.layernorm_fwd(xd, cmap, wd, bd, rows, D, eps)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(rstd).all())
    _check_fwd(worst, (y, mean, rstd), _fwd_refs(x, w, b, eps))
    dx = torch.full((rows, D), SENTINEL, device=_dev())
    dw, db = torch.full((D,), SENTINEL, device=_dev()), torch.full((D,), SENTINEL, device=_dev())
    ops.layernorm_bwd(xd, cmap, dy.to(_dev()), wd, mean, rstd, dx, add.to(_dev()), dw, db, rows, D)
    _check_bwd(worst, (dx, dw, db), _bwd_refs(x, dy, w, b, eps, add))
    worst.report()
