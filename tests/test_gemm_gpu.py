"""GPU tier: the exact fp32 GEMM (csrc/gemm_f32.hip, mode 0) against the float64 restatement of tests/gemm_ref.py - every tile, each of the
three main loops, the K split with every epilogue through its combine, the weight gradient with both combines, the column sums, the output
row remap and the argument checks.

Every case
  - asserts with the plan query (d2s_gemm_f32_plan) that it reached the tile and the slice count it names, and prints a [plan] line that
    also names the main loop the host code chooses for the call's alignment (restated in _loop below from the rules of gemm_impl:
    "rk" = gemm_f32_rk_kernel, the [row][k] LDS image; "fast" = gemm_f32_kernel<FAST = true>; "guarded" = gemm_f32_kernel<FAST = false>)
    and the store ("vec" = 16-byte epilogue, "dword", "combine" = splitk_reduce_epi_kernel; the weight gradient: "single", "vec-combine",
    "scalar-combine");
  - passes rules (a) and (b) of tests/gemm_ref.py against float64;
  - starts from buffers filled with a sentinel and finds the sentinel, bit for bit, wherever the call must not write: gap columns of a
    leading dimension larger than the row, the rows a remap skips, rows past M, operands' own padding;
  - runs twice from the same start and requires the same bits (no atomics, an ordered combine);
  - prints its worst kernel error / yardstick ratio and the largest share of the per-element bound it used."""
import pytest
import torch

from tests import gemm_cases as C, gemm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
ERR_ARG, ERR_WORKSPACE = -1, -2
EPI_NAME = {0: "none", 1: "bias", 2: "bias-relu", 3: "bias-gelu", 4: "bias-resid", 5: "gelu-grad", 6: "relu-mask", 7: "rowadd", 8: "accum",
            11: "rowscale"}


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from d2s import ops as _ops
    assert _ops.get_gemm_mode() == _ops.GEMM_EXACT
    return _ops


@pytest.fixture(scope="module")
def lib():
    from d2s import lib as _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _plan(lib, layout, M, N, K):
    v = lib.query("d2s_gemm_f32_plan", layout, M, N, K, 0)
    return (v & 0xffff, (v >> 16) & 0xffff), v >> 32


class Buf:
    """A 2-D operand as the call sees it: `cols` values per row, rows `ld` floats apart, the first `off` floats past the start of a flat
    buffer whose every other float is the sentinel.  .view is the strided CPU view the reference reads, .dev() a fresh device copy."""

    def __init__(self, values, ld=None, off=0, extra_rows=0):
        rows, cols = values.shape
        self.rows, self.cols, self.ld, self.off = rows, cols, ld or cols, off
        assert self.ld >= cols
        self.flat = torch.full((off + (rows + extra_rows) * self.ld,), SENTINEL)
        self.view = self.flat[off:].view(rows + extra_rows, self.ld)[:rows, :cols]
        self.view.copy_(values)

    def dev(self):
        self.d = self.flat.to(_dev())
        return self.d[self.off:]          # data_ptr of this slice is what the C ABI receives

    def written(self, row_index=None):
        """mask over the flat buffer of the floats that belong to the view (rows moved to row_index when given)"""
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        total_rows = (self.flat.numel() - self.off) // self.ld
        v = m[self.off:].view(total_rows, self.ld)
        v[torch.arange(self.rows) if row_index is None else row_index, :self.cols] = True
        return m


def _aligned(t):
    return t is None or t.data_ptr() % 16 == 0


def _loop(layout, M, N, K, slices, A, lda, B, ldb, Cd, ldc, bias=None, aux=None, ldaux=0, aux_out=None):
    """the main loop and the store that gemm_impl chooses for these device operands (restated from its alignment rules)"""
    a_rows_contig, b_rows_contig = layout == C.TN, layout != C.NT
    vec_a = _aligned(A) and lda % 4 == 0 and (M % 4 == 0 if a_rows_contig else K % 4 == 0)
    vec_b = _aligned(B) and ldb % 4 == 0 and (N % 4 == 0 if b_rows_contig else K % 4 == 0)
    fast = vec_a and vec_b and K % 16 == 0 and (not a_rows_contig or M >= 4) and (not b_rows_contig or N >= 4)
    if slices > 1:          # the slabs are dense [M][N] in the (aligned) workspace; the epilogue operands still count
        vec_epi = N % 4 == 0 and (M * N) % 4 == 0
    else:
        vec_epi = N % 4 == 0 and ldc % 4 == 0 and _aligned(Cd)
    vec_epi = vec_epi and _aligned(bias) and (aux is None or (ldaux % 4 == 0 and _aligned(aux))) and _aligned(aux_out)
    loop = "rk" if (fast and vec_epi and layout != C.TN) else "fast" if fast else "guarded"
    return loop, ("vec" if vec_epi else "dword")


_BASE = {}


def _base(layout, M, N, K, lda=None, ldb=None, a_off=0):
    """operands as strided buffers and the three products every epilogue of a shape shares: float64, fp32 on the CPU, magnitudes"""
    key = (layout, M, N, K, lda, ldb, a_off)
    if key not in _BASE:
        if len(_BASE) >= 2:
            _BASE.clear()
        a, b = C.operands(layout, M, N, K)
        A, B = Buf(a, lda, a_off), Buf(b, ldb)
        _BASE[key] = (A, B, R.product(layout, A.view.double(), B.view.double()), R.product(layout, A.view, B.view),
                      R.magnitude(layout, A.view, B.view))
    return _BASE[key]


def run_gemm(ops, lib, layout, M, N, K, epi=0, lda=None, ldb=None, ldc=None, ldaux=None, a_off=0, aux_rows=0, remap=(0, 0), tile=None,
             slices=None, loop=None, store=None, zero_scales=False, tag=""):
    """one NT / NN case through ops.gemm; -> (ratio of rule (a), share of the bound of rule (b))"""
    assert layout in (C.NT, C.NN)
    what = f"{C.LAYOUT_NAME[layout]} {M}x{N}x{K} epi {EPI_NAME[epi]}{' ' + tag if tag else ''}"
    got_tile, got_slices = _plan(lib, layout, M, N, K)
    assert tile is None or got_tile == tile, (what, got_tile, tile)
    assert slices is None or (got_slices > 1 if slices == ">1" else got_slices == slices), (what, got_slices, slices)
    A, B, acc64, acc32, mag = _base(layout, M, N, K, lda, ldb, a_off)
    g = C.gen(M, N, K, epi, 7)
    bias = torch.randn(N, generator=g) if epi in R.HAS_BIAS else None
    aux = c_old = rowscale = None
    rpg = 0
    if epi in (4, 5, 6, 11):
        aux = Buf(torch.randn(M, N, generator=g), ldaux)
    if epi == 7:
        aux = Buf(torch.randn(aux_rows, N, generator=g), ldaux)
    if epi == 8:
        c_old = torch.randn(M, N, generator=g)
    if epi == 11:
        rpg = max(1, M // 5)
        rowscale = 1.0 + torch.rand((M + rpg - 1) // rpg, generator=g)
        if zero_scales:
            rowscale[::2] = 0.0
    kw = dict(bias=bias, aux=None if aux is None else aux.view, aux_rows=aux_rows, c_old=c_old, rowscale=rowscale, rows_per_group=rpg)
    f64 = lambda t: None if t is None else t.double()
    kw64 = {k: (f64(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    ref64, pre64 = R.epilogue(acc64, epi, **kw64)
    ref32, pre32 = R.epilogue(acc32, epi, **kw)
    bound, pre_bound = R.elem_bound(K, got_slices, mag, epi, acc64=acc64, what=what, **kw)
    # the output buffer: rows moved by the remap, three rows past the last one, gap columns when ldc > N
    rows_idx = R.remap_index(M, *remap)
    out_rows = int(rows_idx[-1]) + 1
    Cb = Buf(torch.full((out_rows, N), SENTINEL), ldc, extra_rows=3)
    if epi == 8:
        Cb.view.copy_(c_old)
    Pb = Buf(torch.full((M, N), SENTINEL), ldc, extra_rows=1) if epi == 3 else None      # the pre-activation copy shares C's leading dimension
    outs = []
    for rep in range(2):
        dA, dB, dC = A.dev(), B.dev(), Cb.dev()
        dbias = None if bias is None else bias.to(_dev())
        daux = None if aux is None else aux.dev()
        dpre = None if Pb is None else Pb.dev()
        dscale = None if rowscale is None else rowscale.to(_dev())
        if rep == 0:
            lp, st = _loop(layout, M, N, K, got_slices, dA, A.ld, dB, B.ld, dC, Cb.ld, dbias, daux, aux.ld if aux else 0, dpre)
            st = "combine" if got_slices > 1 else st
            print(f"\n[plan] {what}: tile {got_tile[0]}x{got_tile[1]} slices {got_slices} loop {lp} store {st} lda {A.ld} ldb {B.ld} ldc {Cb.ld}")
            assert loop is None or lp == loop, (what, lp, loop)
            assert store is None or st == store, (what, st, store)
        ops.gemm(layout, dA, A.ld, dB, B.ld, dC, Cb.ld, M, N, K, epi=epi, bias=dbias, aux=daux, ldaux=aux.ld if aux else 0, aux_out=dpre,
                 aux_rows=aux_rows, remap_rows=remap[0], remap_skip=remap[1], accumulate=(epi == 8), rowscale=dscale, rows_per_group=rpg)
        torch.cuda.synchronize()
        outs.append((Cb.d.cpu(), None if Pb is None else Pb.d.cpu(), A.d.cpu(), B.d.cpu(), None if aux is None else aux.d.cpu()))
    for first, second in zip(outs[0], outs[1]):
        assert first is None or _same_bits(first, second), f"{what}: two runs differ"
    flatC, flatP, flatA, flatB, flatX = outs[0]
    assert _same_bits(flatA, A.flat) and _same_bits(flatB, B.flat) and (aux is None or _same_bits(flatX, aux.flat)), f"{what}: an operand changed"
    wr = Cb.written(rows_idx)
    assert _same_bits(flatC[~wr], torch.full_like(flatC[~wr], SENTINEL)), f"{what}: a store outside the result"
    got = flatC[Cb.off:].view(-1, Cb.ld)[rows_idx, :N]
    res = [R.check(what, got, ref64, ref32, bound)]
    if Pb is not None:
        assert _same_bits(flatP[~Pb.written()], torch.full_like(flatP[~Pb.written()], SENTINEL)), f"{what}: a store outside the pre-activation"
        res.append(R.check(what + " pre-activation", flatP[Pb.off:].view(-1, Pb.ld)[:M, :N], pre64, pre32, pre_bound))
    if epi == 11 and zero_scales:
        dropped = (R.group_scale(rowscale, M, rpg)[:, 0] == 0)
        assert bool(dropped.any()) and _same_bits(got[dropped], aux.view[dropped]), f"{what}: a zero-scale row is not a bit copy of aux"
    return max(r[0] for r in res), max(r[1] for r in res)


class Worst:
    def __init__(self, what):
        self.what, self.ratio, self.used = what, 0.0, 0.0

    def add(self, res):
        self.ratio, self.used = max(self.ratio, res[0]), max(self.used, res[1])

    def report(self):
        print(f"[worst] {self.what}: kernel / yardstick ratio {self.ratio:.2f}, {100 * self.used:.1f} % of the per-element bound")


# ------------------------------------------------------------------------------------------------ tiles x loops
@pytest.mark.parametrize("layout", [C.NT, C.NN], ids=["NT", "NN"])
@pytest.mark.parametrize("tile", list(C.TILE_SHAPES), ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("loop,K,dword,a_off", C.TILE_LOOPS, ids=lambda v: str(v))
def test_every_tile_and_main_loop(ops, lib, layout, tile, loop, K, dword, a_off):
    M, N = C.TILE_SHAPES[tile]
    ldc = None
    if dword and layout == C.NT:
        N -= 1                      # an odd width: the B operand stays k-contiguous and aligned, the store falls back to dwords
    elif dword:
        ldc = N + 1                 # NN needs N % 4 == 0 for its 16-byte loads of B: a leading dimension that is no multiple of 4 instead
    w = Worst(f"{C.LAYOUT_NAME[layout]} tile {tile[0]}x{tile[1]} loop {loop} K {K}")
    w.add(run_gemm(ops, lib, layout, M, N, K, epi=R.EPI_BIAS, ldc=ldc, a_off=1 if a_off else 0, tile=tile, slices=1, loop=loop,
                   store="dword" if dword else "vec"))
    w.report()


# ------------------------------------------------------------------------------------------------ workgroup order
def test_workgroup_order_every_residue(ops, lib):
    """64x64 tiles, M = 64 i - 1: the bijective XCD remap of the workgroup index for nwg & 7 = 0 .. 7; every element written once and
    correctly (the sentinel outside, the reference inside)"""
    w = Worst("workgroup order")
    seen = set()
    for (M, N, K) in C.WG_ORDER:
        seen.add(((M + 63) // 64) & 7)
        w.add(run_gemm(ops, lib, C.NT, M, N, K, tile=(64, 64), slices=1, loop="rk"))
    assert seen == set(range(8))
    w.add(run_gemm(ops, lib, C.NN, 64 * 11 - 1, 132, 16, tile=(64, 64), slices=1))      # two tile columns: nwg = 33
    w.report()


# ------------------------------------------------------------------------------------------------ small edges
@pytest.mark.parametrize("layout", [C.NT, C.NN], ids=["NT", "NN"])
def test_small_edges(ops, lib, layout):
    """M, N in {1, 3, 4, 5}: rows clamped to the last valid row in the guard-free loads, the N >= 4 fallback of the n-contiguous B"""
    w = Worst(f"{C.LAYOUT_NAME[layout]} small edges")
    loops = set()
    for (M, N, K) in C.SMALL_EDGES:
        want = "guarded" if (K % 16 or (layout == C.NN and N % 4)) else "rk" if N % 4 == 0 else "fast"
        w.add(run_gemm(ops, lib, layout, M, N, K, epi=R.EPI_BIAS, tile=(64, 64), slices=1, loop=want))
        loops.add(want)
    assert loops == {"guarded", "rk"} | ({"fast"} if layout == C.NT else set())
    w.report()


# ------------------------------------------------------------------------------------------------ K split
@pytest.mark.parametrize("layout", [C.NT, C.NN], ids=["NT", "NN"])
@pytest.mark.parametrize("M,N,K", C.KSPLIT_SHAPES)
def test_k_split_every_epilogue_through_the_combine(ops, lib, layout, M, N, K):
    """the slabs are summed in slab order and the combine applies the epilogue of the single-pass store; K = 1544 is no multiple of 16
    (the guarded loop, a shorter last slice)"""
    w = Worst(f"{C.LAYOUT_NAME[layout]} K split {M}x{N}x{K}")
    loop = "guarded" if K % 16 else None
    if (M, N, K) == (64, 64, 4096):
        assert _plan(lib, layout, M, N, K)[1] == 6
    for epi in R.EPILOGUES:
        kw = dict(aux_rows=max(1, M // 3), remap=(max(1, M // 3), 2)) if epi == 7 else {}
        w.add(run_gemm(ops, lib, layout, M, N, K, epi=epi, ldc=N + 4, ldaux=N + 8, slices=">1", loop=loop, store="combine",
                       zero_scales=True, tag="ld", **kw))
    for epi in (1, 4, 7):           # and dense, the way the model calls them; 7 without a remap
        w.add(run_gemm(ops, lib, layout, M, N, K, epi=epi, slices=">1", store="combine", aux_rows=M if epi == 7 else 0, tag="dense"))
    w.report()


# ------------------------------------------------------------------------------------------------ epilogues, single pass
@pytest.mark.parametrize("layout", [C.NT, C.NN], ids=["NT", "NN"])
@pytest.mark.parametrize("N,store", [(132, "vec"), (131, "dword")])
def test_single_pass_every_epilogue(ops, lib, layout, N, store):
    """every epilogue through both stores of the single-pass kernels, with leading dimensions larger than the rows; accumulate (8) on a
    pre-filled C; zero row scales (11)"""
    M, K = 300, 48
    if layout == C.NN and store == "dword":
        N = 132
    w = Worst(f"{C.LAYOUT_NAME[layout]} single pass, {store} store")
    for epi in R.EPILOGUES:
        ldc = N + (4 if store == "vec" else 5)
        kw = dict(aux_rows=7, remap=(0, 0)) if epi == 7 else {}
        w.add(run_gemm(ops, lib, layout, M, N, K, epi=epi, lda=K + 4, ldb=(K if layout == C.NT else N) + 8, ldc=ldc, ldaux=N + 8,
                       tile=(64, 64), slices=1, store=store, zero_scales=True, tag="ld", **kw))
    w.report()


# ------------------------------------------------------------------------------------------------ remap
@pytest.mark.parametrize("rows_per_img,skip,N", C.REMAP_CASES)
def test_output_row_remap_single_pass(ops, lib, rows_per_img, skip, N):
    """row m of the result goes to buffer row m + (m // rows_per_img + 1) * skip, the skipped (CLS) rows keep the sentinel; M is no
    multiple of rows_per_img; N = 132: 16-byte store, 131: dword store"""
    w = Worst(f"remap rows_per_img {rows_per_img} skip {skip} N {N}")
    for layout in (C.NT, C.NN) if N % 4 == 0 else (C.NT,):
        w.add(run_gemm(ops, lib, layout, C.REMAP_M, N, C.REMAP_K, epi=7, aux_rows=rows_per_img, remap=(rows_per_img, skip), tile=(64, 64),
                       slices=1, store="vec" if N % 4 == 0 else "dword"))
    w.report()


# ------------------------------------------------------------------------------------------------ weight gradient
def run_wgrad(ops, lib, tokens, n_out, n_in, with_db, accumulate, strided, w):
    """strided: 0 = dense operands, else the padding of dW's rows (3: the scalar combine, 4: still the 16-byte one), dy and x padded too"""
    what = f"TN tokens {tokens} dW {n_out}x{n_in}{' db' if with_db else ''}{' accumulate' if accumulate else ''}{' strided' if strided else ''}"
    tile, slices = _plan(lib, C.TN, n_out, n_in, tokens)
    assert tile == (128, 128) and (slices > 1) == (tokens > 256), (what, tile, slices)
    lddy, ldx, lddw = (n_out + 4, n_in + 8, n_in + strided) if strided else (None, None, None)
    DY, X, acc64, acc32, mag = _base(C.TN, n_out, n_in, tokens, lddy, ldx)
    g = C.gen(tokens, n_out, n_in, 11)
    w_old, b_old = torch.randn(n_out, n_in, generator=g), torch.randn(n_out, generator=g)
    W = Buf(w_old, lddw, extra_rows=2)
    Bb = Buf(b_old[None, :], extra_rows=1)
    zero = torch.zeros((), dtype=torch.float64)
    ref64 = acc64 + (w_old.double() if accumulate else zero)
    ref32 = acc32 + (w_old if accumulate else 0.0)
    bound = (tokens + slices + 4) * R.F32_EPS * (mag + (w_old.double().abs() if accumulate else zero))
    db64 = R.colsum(DY.view.double()) + (b_old.double() if accumulate else zero)
    db32 = R.colsum(DY.view) + (b_old if accumulate else 0.0)
    db_bound = (tokens + slices + 4) * R.F32_EPS * (DY.view.double().abs().sum(dim=0) + (b_old.double().abs() if accumulate else zero))
    need = lib.query("d2s_linear_wgrad_workspace_bytes", tokens, n_out, n_in, 0)
    assert (need > 0) == (slices > 1)
    outs = []
    for rep in range(2):
        dDY, dX, dW, dB = DY.dev(), X.dev(), W.dev(), Bb.dev()
        ws = ops.workspace(need, _dev()) if need else None
        if rep == 0:
            lp, _ = _loop(C.TN, n_out, n_in, tokens, slices, dDY, DY.ld, dX, X.ld, dW, W.ld)
            vec = n_in % 4 == 0 and W.ld % 4 == 0 and _aligned(dW) and _aligned(ws) and (n_out * n_in) % 4 == 0
            comb = "single" if slices == 1 else "vec-combine" if vec else "scalar-combine"
            print(f"\n[plan] {what}: tile 128x128 slices {slices} loop {lp} store {comb} lddy {DY.ld} ldx {X.ld} lddw {W.ld}")
            w.seen.add((slices > 1, comb, lp))
        lib.call("d2s_linear_wgrad_f32", lib.ptr(dDY), DY.ld, lib.ptr(dX), X.ld, lib.ptr(dW), W.ld, lib.ptr(dB) if with_db else None, tokens,
                 n_out, n_in, int(accumulate), 0, lib.ptr(ws), ws.numel() if ws is not None else 0)
        torch.cuda.synchronize()
        outs.append((W.d.cpu(), Bb.d.cpu(), DY.d.cpu(), X.d.cpu()))
    for first, second in zip(outs[0], outs[1]):
        assert _same_bits(first, second), f"{what}: two runs differ"
    fW, fB, fDY, fX = outs[0]
    assert _same_bits(fDY, DY.flat) and _same_bits(fX, X.flat), f"{what}: an operand changed"
    assert _same_bits(fW[~W.written()], torch.full_like(fW[~W.written()], SENTINEL)), f"{what}: a store outside dW"
    w.add(R.check(what + " dW", fW[W.off:].view(-1, W.ld)[:n_out, :n_in], ref64, ref32, bound))
    if with_db:
        assert _same_bits(fB[~Bb.written()], torch.full_like(fB[~Bb.written()], SENTINEL)), f"{what}: a store outside db"
        w.add(R.check(what + " db", fB[:n_out], db64, db32, db_bound))
    else:
        assert _same_bits(fB, Bb.flat), f"{what}: db written without being asked for"


@pytest.mark.parametrize("n_out,n_in", C.WGRAD_SHAPES)
def test_weight_gradient(ops, lib, n_out, n_in):
    """dW = dy^T x with the bias gradient folded out of the dy tiles, one slice and many, both combines, accumulate on both paths,
    strided dy / x / dW; without db nothing else is written"""
    w = Worst(f"TN dW {n_out}x{n_in}")
    w.seen = set()
    for tokens in C.WGRAD_TOKENS:
        run_wgrad(ops, lib, tokens, n_out, n_in, with_db=True, accumulate=False, strided=False, w=w)
        run_wgrad(ops, lib, tokens, n_out, n_in, with_db=True, accumulate=True, strided=3, w=w)
        run_wgrad(ops, lib, tokens, n_out, n_in, with_db=False, accumulate=tokens % 2 == 1, strided=4 if tokens % 2 == 0 else 0, w=w)
    assert {s[0] for s in w.seen} == {False, True}                       # 1 and > 1 slices
    assert {s[1] for s in w.seen} == {"single", "vec-combine", "scalar-combine"}
    # the guard-free loop: tokens % 16 == 0 and 16-byte loads along n_out / n_in, which 10 and 130 do not allow
    assert {s[2] for s in w.seen} == ({"fast", "guarded"} if n_out % 4 == 0 else {"guarded"})
    assert ((True, "vec-combine", "fast") in w.seen) == (n_out % 4 == 0)      # the model's own path: many slices, guard-free loop
    w.report()


def test_small_edges_weight_gradient(ops, lib):
    """n_out, n_in in {1, 3, 4, 5}: the rows - 4 clamp of the m-contiguous guard-free loads, and the M >= 4 / N >= 4 fallbacks"""
    w = Worst("TN small edges")
    w.seen = set()
    for (n_out, n_in, tokens) in C.SMALL_EDGES:
        run_wgrad(ops, lib, tokens, n_out, n_in, with_db=True, accumulate=False, strided=0, w=w)
    assert {s[2] for s in w.seen} == {"fast", "guarded"} and {s[1] for s in w.seen} == {"single"}
    w.report()


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("M,N", C.COLSUM_SHAPES)
def test_colsum_strided(ops, lib, M, N):
    w = Worst(f"colsum {M}x{N}")
    g = C.gen(M, N, 5)
    X = Buf(torch.randn(M, N, generator=g), N + 3)
    old = torch.randn(N, generator=g)
    need = lib.query("d2s_colsum_workspace_bytes", M, N)
    for accumulate in (0, 1):
        what = f"colsum {M}x{N} ldx {X.ld} accumulate {accumulate}"
        ref64 = R.colsum(X.view.double()) + (old.double() if accumulate else 0.0)
        ref32 = R.colsum(X.view) + (old if accumulate else 0.0)
        slices = min(128, (M + 511) // 512)
        bound = (M + slices + 4) * R.F32_EPS * (X.view.double().abs().sum(dim=0) + (old.double().abs() if accumulate else 0.0))
        outs = []
        for rep in range(2):
            O = Buf(old[None, :], extra_rows=1)
            dX, dO = X.dev(), O.dev()
            ws = ops.workspace(need, _dev())
            lib.call("d2s_colsum_f32", lib.ptr(dX), X.ld, M, N, lib.ptr(dO), accumulate, lib.ptr(ws), ws.numel())
            torch.cuda.synchronize()
            outs.append((O.d.cpu(), X.d.cpu()))
        assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], X.flat), what
        assert _same_bits(outs[0][0][N:], torch.full((N,), SENTINEL)), f"{what}: a store past out[N]"
        w.add(R.check(what, outs[0][0][:N], ref64, ref32, bound))
    w.report()


# ------------------------------------------------------------------------------------------------ arguments
def _raw_gemm(lib, layout, A, lda, B, ldb, Cd, ldc, M, N, K, epi=0, bias=None, aux=None, ldaux=0, aux_out=None, aux_rows=0, remap=(0, 0),
              accumulate=0, mode=0, ws=None, ws_bytes=None):
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.query("d2s_gemm_f32", layout, p(A), lda, p(B), ldb, p(Cd), ldc, M, N, K, epi, p(bias), p(aux), ldaux, p(aux_out), aux_rows,
                   remap[0], remap[1], accumulate, mode, p(ws), (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes,
                   lib.stream())
    torch.cuda.synchronize()
    return rc


def test_argument_checks(ops, lib):
    d = _dev()
    M, N, K = 40, 36, 32
    a, b = torch.randn(M, K, device=d), torch.randn(N, K, device=d)
    bias, aux = torch.randn(N, device=d), torch.randn(M, N, device=d)
    c = torch.full((2 * M + 2, N), SENTINEL, device=d)
    untouched = lambda: _same_bits(c, torch.full((2 * M + 2, N), SENTINEL))
    assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=1, bias=bias) == 0 and not untouched()
    for mode in (0, 1, 2):
        ws = ops.workspace(lib.query("d2s_gemm_f32_workspace_bytes", 0, M, N, K, mode), d)
        for layout, bb, ldb in ((0, b, K), (1, b.t().contiguous(), N)):
            c.fill_(SENTINEL)
            # accumulate is epilogue 8: with a bias / residual / activation epilogue it is refused, in every mode
            for epi in (1, 2, 3, 4, 5, 6, 7):
                rc = _raw_gemm(lib, layout, a, K, bb, ldb, c, N, M, N, K, epi=epi, bias=bias, aux=aux, ldaux=N, aux_rows=M, accumulate=1,
                               mode=mode, ws=ws)
                assert rc == ERR_ARG, (mode, layout, epi, rc)
            # the row remap belongs to epilogue 7
            for epi in (0, 1, 2, 3, 4, 5, 6, 8):
                rc = _raw_gemm(lib, layout, a, K, bb, ldb, c, N, M, N, K, epi=epi, bias=bias, aux=aux, ldaux=N, remap=(4, 1),
                               accumulate=int(epi == 8), mode=mode, ws=ws)
                assert rc == ERR_ARG, (mode, layout, epi, rc)
            assert untouched(), (mode, layout)
    # what stays allowed: accumulate with epilogue 0 and 8 (the same call), the remap with epilogue 7
    c.fill_(1.0)
    assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=0, accumulate=1) == 0
    first = c[:M].clone()
    c.fill_(1.0)
    assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=8, accumulate=1) == 0 and _same_bits(first, c[:M])
    assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=7, bias=bias, aux=aux, ldaux=N, aux_rows=M, remap=(4, 1)) == 0
    # the same two rules on a shape that splits K: neither path runs
    Ms, Ns, Ks = C.KSPLIT_SHAPES[2]
    need = lib.query("d2s_gemm_f32_workspace_bytes", 0, Ms, Ns, Ks, 0)
    assert need > 0
    a2, b2, aux2 = torch.randn(Ms, Ks, device=d), torch.randn(Ns, Ks, device=d), torch.randn(Ms, Ns, device=d)
    c2 = torch.full((Ms, Ns), SENTINEL, device=d)
    ws = ops.workspace(need, d)
    assert _raw_gemm(lib, 0, a2, Ks, b2, Ks, c2, Ns, Ms, Ns, Ks, epi=4, bias=None, aux=aux2, ldaux=Ns, accumulate=1, ws=ws) == ERR_ARG
    assert _raw_gemm(lib, 0, a2, Ks, b2, Ks, c2, Ns, Ms, Ns, Ks, epi=1, remap=(4, 1), ws=ws) == ERR_ARG
    # a workspace one byte short, or none
    assert _raw_gemm(lib, 0, a2, Ks, b2, Ks, c2, Ns, Ms, Ns, Ks, ws=ws, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _raw_gemm(lib, 0, a2, Ks, b2, Ks, c2, Ns, Ms, Ns, Ks, ws=None, ws_bytes=need) == ERR_WORKSPACE
    assert _raw_gemm(lib, 1, a2, Ks, b2.t().contiguous(), Ns, c2, Ns, Ms, Ns, Ks, ws=ws, ws_bytes=need - 1) == ERR_WORKSPACE
    assert _same_bits(c2, torch.full((Ms, Ns), SENTINEL))
    assert _raw_gemm(lib, 0, a2, Ks, b2, Ks, c2, Ns, Ms, Ns, Ks, ws=ws, ws_bytes=need) == 0
    tok, no, ni = 1000, 10, 24
    wneed = lib.query("d2s_linear_wgrad_workspace_bytes", tok, no, ni, 0)
    assert wneed > 0
    dy, x, dw = torch.randn(tok, no, device=d), torch.randn(tok, ni, device=d), torch.full((no, ni), SENTINEL, device=d)
    wargs = (lib.ptr(dy), no, lib.ptr(x), ni, lib.ptr(dw), ni, None, tok, no, ni, 0, 0)
    assert lib.query("d2s_linear_wgrad_f32", *wargs, lib.ptr(ws), wneed - 1, lib.stream()) == ERR_WORKSPACE
    assert lib.query("d2s_linear_wgrad_f32", *wargs, None, wneed, lib.stream()) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _same_bits(dw, torch.full((no, ni), SENTINEL))
    # the older checks of gemm_impl: null operands, epilogues 4..7 without aux, an epilogue outside 0..8, sizes, layout, mode
    c.fill_(SENTINEL)
    assert _raw_gemm(lib, 0, None, K, b, K, c, N, M, N, K) == ERR_ARG
    assert _raw_gemm(lib, 0, a, K, None, K, c, N, M, N, K) == ERR_ARG
    assert _raw_gemm(lib, 0, a, K, b, K, None, N, M, N, K) == ERR_ARG
    for epi in (4, 5, 6, 7):
        assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=epi, bias=bias, aux=None, aux_rows=M) == ERR_ARG, epi
    for epi in (-1, 9, 10, 11, 12):          # 9 / 10 belong to the bf16 entry, 11 to d2s_gemm_f32_rowscale
        assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, epi=epi, bias=bias, aux=aux, ldaux=N) == ERR_ARG, epi
    for (m, n, k) in ((0, N, K), (M, 0, K), (M, N, 0), (-1, N, K)):
        assert _raw_gemm(lib, 0, a, K, b, K, c, N, m, n, k) == ERR_ARG
    assert _raw_gemm(lib, 3, a, K, b, K, c, N, M, N, K) == ERR_ARG and _raw_gemm(lib, -1, a, K, b, K, c, N, M, N, K) == ERR_ARG
    assert _raw_gemm(lib, 0, a, K, b, K, c, N, M, N, K, mode=3) == ERR_ARG
    assert untouched()
