"""CPU tier of the fp32 GEMM parity suite: the float64 restatement (tests/gemm_ref.py) against torch's own operators, the index rules of the
row-add and the output row remap on small integer matrices, the plan query and its header / binding bookkeeping, and torch's fp32 CPU
product held to the per-element bound on every shape tests/test_gemm_gpu.py multiplies (a correct fp32 GEMM has room under it)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import cases, gemm_cases as C, gemm_ref as R

REPO = cases.REPO
NEW = ["d2s_gemm_f32_plan"]


def _ops(M, N, K, seed, aux_rows=0):
    g = C.gen(M, N, K, seed)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    aux = torch.randn(aux_rows if aux_rows else M, N, generator=g, dtype=torch.float64)
    return x, w, b, aux


# ---- the restatement against torch's operators, float64 ----
@pytest.mark.parametrize("M,N,K", [(5, 7, 3), (33, 20, 48)])
def test_restatement_matches_torch_float64(M, N, K):
    x, w, b, aux = _ops(M, N, K, 0)
    tol = dict(rtol=1e-12, atol=1e-12)
    lin = F.linear(x, w, b)
    assert torch.allclose(R.gemm_ref(R.NT, x, w)[0], F.linear(x, w), **tol)
    assert torch.allclose(R.gemm_ref(R.NN, x, w.t().contiguous())[0], F.linear(x, w), **tol)
    assert torch.allclose(R.gemm_ref(R.TN, x.t().contiguous(), w.t().contiguous())[0], F.linear(x, w), **tol)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_BIAS, bias=b)[0], lin, **tol)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_BIAS_RELU, bias=b)[0], torch.relu(lin), **tol)
    out, pre = R.gemm_ref(R.NT, x, w, R.EPI_BIAS_GELU, bias=b)
    assert torch.allclose(out, F.gelu(lin), **tol) and torch.allclose(pre, lin, **tol)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_BIAS_RESID, bias=b, aux=aux)[0], lin + aux, **tol)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_ACCUM, c_old=aux)[0], aux + F.linear(x, w), **tol)
    # the two backward masks: autograd through gelu / relu of the saved tensor, upstream gradient = the product
    z = aux.clone().requires_grad_(True)
    dy = F.linear(x, w)
    (gg,) = torch.autograd.grad(F.gelu(z), z, dy)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_MUL_GELU_GRAD, aux=aux)[0], gg, **tol)
    z = aux.clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(torch.relu(z), z, dy)
    assert torch.allclose(R.gemm_ref(R.NT, x, w, R.EPI_MUL_RELU_MASK, aux=aux)[0], gr, **tol)
    # the weight gradient pair of F.linear by autograd
    xx, ww, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    up = aux
    dx, dw, db = torch.autograd.grad((F.linear(xx, ww, bb) * up).sum(), (xx, ww, bb))
    assert torch.allclose(R.gemm_ref(R.TN, up, x)[0], dw, **tol)             # dW = dy^T x: A = dy [tokens, n_out], B = x [tokens, n_in]
    assert torch.allclose(R.colsum(up), db, **tol)
    assert torch.allclose(R.gemm_ref(R.NN, up, w)[0], dx, **tol)             # dx = dy W
    assert max(float(R.gelu_grad(torch.linspace(-6, 6, 100001, dtype=torch.float64)).abs().max()), 1.0) <= R.GELU_SLOPE


def test_restatement_reads_strided_views():
    x, w, b, aux = _ops(6, 5, 8, 1)
    wide = torch.full((6, 11), 1e30, dtype=torch.float64)
    wide[:, :8] = x
    flat = torch.full((1 + 5 * 9,), 1e30, dtype=torch.float64)
    wv = flat[1:].view(5, 9)[:, :8]
    wv.copy_(w)
    assert torch.equal(R.gemm_ref(R.NT, wide[:, :8], wv, R.EPI_BIAS, bias=b)[0], R.gemm_ref(R.NT, x, w, R.EPI_BIAS, bias=b)[0])
    assert torch.equal(R.magnitude(R.NT, wide[:, :8], wv), R.magnitude(R.NT, x, w))


def test_rowscale_zero_is_a_copy_of_aux():
    x, w, b, aux = _ops(7, 4, 5, 2)
    s = torch.tensor([0.0, 1.25, 0.0], dtype=torch.float64)                  # groups of 3 rows, the last group ragged
    x[0, 0] = float("inf")                                                   # whatever the branch holds
    out, _ = R.gemm_ref(R.NT, x, w, R.EPI_BIAS_RESID_ROWSCALE, bias=b, aux=aux, rowscale=s, rows_per_group=3)
    assert torch.equal(out[0:3], aux[0:3]) and torch.equal(out[6:], aux[6:])
    assert torch.allclose(out[3:6], 1.25 * F.linear(x[3:6], w, b) + aux[3:6], rtol=1e-12, atol=1e-12)


def test_index_rules_on_integer_matrices():
    """exact arithmetic: small integers, so every dtype gives the same numbers"""
    M, N, K, rows, skip = 7, 3, 2, 3, 2
    x = torch.arange(M * K, dtype=torch.float64).view(M, K)
    w = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
    pos = 100.0 * torch.arange(1, rows + 1, dtype=torch.float64)[:, None] + torch.arange(N, dtype=torch.float64)
    out, _ = R.gemm_ref(R.NT, x, w, R.EPI_BIAS_ROWADD, bias=torch.zeros(N, dtype=torch.float64), aux=pos, aux_rows=rows)
    for m in range(M):
        want = torch.tensor([x[m, 0], x[m, 1], x[m, 0] + x[m, 1]]) + pos[m % rows]
        assert torch.equal(out[m], want), m
    assert R.rowadd_index(7, 3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    # image b owns buffer rows b * (rows + skip) .. ; its first `skip` rows (CLS) are left alone, token t goes to row b * (rows + skip) + skip + t
    assert R.remap_index(7, 3, 2).tolist() == [2, 3, 4, 7, 8, 9, 12]
    assert R.remap_index(4, 1, 1).tolist() == [1, 3, 5, 7]
    assert R.remap_index(5, 196, 1).tolist() == [1, 2, 3, 4, 5]
    assert R.remap_index(3, 0, 5).tolist() == [0, 1, 2]
    for rpi in (1, 3, 196):
        for sk in (1, 2):
            idx = R.remap_index(C.REMAP_M, rpi, sk)
            assert idx.tolist() == [m + (m // rpi + 1) * sk for m in range(C.REMAP_M)] and len(set(idx.tolist())) == C.REMAP_M
    assert R.group_scale(torch.tensor([5.0, 6.0]), 5, 3)[:, 0].tolist() == [5.0, 5.0, 5.0, 6.0, 6.0]


def test_bound_terms():
    """the per-element bound counts K + slices + 4 roundings over the magnitudes the epilogue adds, and nothing else"""
    x, w, b, aux = _ops(4, 3, 8, 3)
    mag = R.magnitude(R.NT, x, w)
    u = R.F32_EPS
    assert torch.equal(R.elem_bound(8, 1, mag)[0], 13 * u * mag)
    assert torch.equal(R.elem_bound(8, 3, mag, R.EPI_BIAS, bias=b)[0], 15 * u * (mag + b.abs()))
    assert torch.equal(R.elem_bound(8, 1, mag, R.EPI_BIAS_RESID, bias=b, aux=aux)[0], 13 * u * (mag + b.abs() + aux.abs()))
    assert torch.equal(R.elem_bound(8, 1, mag, R.EPI_ACCUM, c_old=aux)[0], 13 * u * (mag + aux.abs()))
    assert torch.equal(R.elem_bound(8, 1, mag, R.EPI_MUL_RELU_MASK, aux=aux)[0], 13 * u * mag * (aux > 0))
    s = torch.tensor([0.0, 2.0], dtype=torch.float64)
    got = R.elem_bound(8, 1, mag, R.EPI_BIAS_RESID_ROWSCALE, bias=b, aux=aux, rowscale=s, rows_per_group=2)[0]
    assert torch.equal(got[:2], 13 * u * aux[:2].abs()) and torch.equal(got[2:], 13 * u * ((mag[2:] + b.abs()) * 2.0 + aux[2:].abs()))
    acc = R.product(R.NT, x, w)
    gb, pb = R.elem_bound(8, 1, mag, R.EPI_BIAS_GELU, bias=b, acc64=acc, what="cpu")
    assert bool((gb > R.GELU_SLOPE * pb).all()) and torch.equal(pb, 13 * u * (mag + b.abs()))
    with pytest.raises(AssertionError, match="per-element bound"):            # a doubled product in one element: rule (b) sees it
        bad = acc.clone().float()
        bad[2, 1] += float(x[2, 0] * w[1, 0]) if abs(float(x[2, 0] * w[1, 0])) > 1e-3 else 1.0
        R.check_elements("doubled product", bad, acc, R.elem_bound(8, 1, mag)[0])


# ---- torch's own fp32 product under rule (b), every shape of the GPU test ----
def _fp32_product_share(M, N, K):
    a, b = C.operands(R.NT, M, N, K)
    ref64 = R.product(R.NT, a.double(), b.double())
    bound = R.elem_bound(K, 1, R.magnitude(R.NT, a, b))[0]
    err = (R.product(R.NT, a, b).double() - ref64).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def _group(name):
    small = [s for s in C.all_shapes() if s[0] * s[1] * s[2] <= 5e7]
    big = [s for s in C.all_shapes() if s[0] * s[1] * s[2] > 5e7]
    return small if name == "small" else big[int(name)::4]


@pytest.mark.parametrize("group", ["small", "0", "1", "2", "3"])
def test_torch_fp32_product_passes_the_element_bound(group):
    worst, at = 0.0, None
    shapes = _group(group)
    assert shapes
    for (M, N, K) in shapes:
        used = _fp32_product_share(M, N, K)
        if used > worst:
            worst, at = used, (M, N, K)
    print(f"[bound] torch fp32 CPU product, {len(shapes)} shapes: at most {100 * worst:.1f} % of the per-element bound, at {at}")
    assert worst < 0.5, (worst, at)          # a correct fp32 GEMM has at least half the bound to spare


# ---- plan query, header and binding ----
def _plan(lib, layout, M, N, K, mode=0):
    v = lib.query("d2s_gemm_f32_plan", layout, M, N, K, mode)
    return (v & 0xffff, (v >> 16) & 0xffff, v >> 32)


def test_plan_query_names_the_tiles_and_slices_the_gpu_cases_expect():
    from d2s import lib
    for tile, (M, N) in C.TILE_SHAPES.items():
        for layout in (C.NT, C.NN):
            for n in (N, N - 1):
                for K in (16, 20, 48):
                    assert _plan(lib, layout, M, n, K) == (tile[0], tile[1], 1), (layout, M, n, K)
    for (M, N, K) in C.WG_ORDER + C.SMALL_EDGES:
        assert _plan(lib, C.NT, M, N, K) == (64, 64, 1) == _plan(lib, C.NN, M, N, K)
    for (M, N, K) in C.KSPLIT_SHAPES:
        for layout in (C.NT, C.NN):
            bm, bn, sl = _plan(lib, layout, M, N, K)
            assert sl > 1 and lib.query("d2s_gemm_f32_workspace_bytes", layout, M, N, K, 0) == sl * M * N * 4
            kper = -(-(-(-K // sl)) // 16) * 16                    # a slice's share, rounded up to whole K-steps ...
            assert -(-K // kper) == sl                             # ... leaves the slice count the query reports
    assert _plan(lib, C.NT, 64, 64, 4096)[2] == 6
    for t in C.WGRAD_TOKENS:
        for (no, ni) in C.WGRAD_SHAPES:
            bm, bn, sl = _plan(lib, C.TN, no, ni, t)
            assert (bm, bn) == (128, 128) and (sl > 1) == (t > 256)
            need = lib.query("d2s_linear_wgrad_workspace_bytes", t, no, ni, 0)
            assert need == (0 if sl == 1 else (sl * no * ni + sl * no) * 4)
            assert _plan(lib, C.TN, no, ni, t, 1) == (bm, bn, sl)                          # mode 1 keeps the exact weight-gradient kernel
    for args in ((3, 8, 8, 8, 0), (-1, 8, 8, 8, 0), (0, 0, 8, 8, 0), (0, 8, 0, 8, 0), (0, 8, 8, 0, 0), (0, 8, 8, 8, 3), (0, 8, 8, 8, -1),
                 (0, 64, 64, 64, 1), (1, 64, 64, 64, 2), (0, 64, 64, 64, 2), (1, 64, 64, 64, 1), (2, 64, 64, 64, 2)):
        assert lib.query("d2s_gemm_f32_plan", *args) == 0, args


def test_gemm_plan_header_and_binding_tables():
    from d2s import lib
    text = open(os.path.join(REPO, "include", "d2s_hip_gemm_plan.h")).read()
    assert NEW == lib.symbols("d2s_hip_gemm_plan.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    res, argt = lib.signature("d2s_gemm_f32_plan")
    assert res is lib.Z and argt == lib.signature("d2s_gemm_f32_workspace_bytes")[1]      # a size_t query: no stream is appended
    params = re.search(r"d2s_gemm_f32_plan\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert len(params) == len(argt) and "stream" not in "".join(params)
    # the launch, the workspace query and the plan query read tile, slices and workspace bytes from one helper: its definition, one
    # call in each of the three, and nothing else chooses a tile or a slice count
    csrc = os.path.join(REPO, "dense2sparse-vit_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_f32.hip")).read()
    assert src.count("exact_plan(") == 4 and src.count("pick_tile(") == 2 and src.count("nt_slices(") == 2
    # the same for the two plans of the bf16 / bf16x3 paths: defined beside their kernels, called by the workspace query and by the launch
    # (run_gemm, which hands the plan to the launcher), and nowhere else
    split = open(os.path.join(csrc, "gemm_split.hip")).read()
    for plan in ("split_plan(", "wgrad16_plan("):
        assert split.count(plan) == 1 and src.count(plan) == 2, plan
        query = src[src.index("size_t d2s_gemm_f32_workspace_bytes("):src.index("size_t d2s_gemm_f32_plan(")]
        run = src[src.index("static int run_gemm("):src.index("int d2s_gemm_f32(int layout")]
        assert query.count(plan) == 1 and run.count(plan) == 1, plan
    # the weight gradient's LDS-DMA predicate: its definition and one evaluation, inside wgrad16_plan
    assert split.count("split_tn_use_dma(") == 2 and src.count("split_tn_use_dma(") == 0
    body = split[split.index("Wgrad16Plan wgrad16_plan("):split.index("int launch_wgrad16_matrix(")]
    assert body.count("split_tn_use_dma(") == 1


def test_workspace_queries_return_the_recorded_sizes():
    """tests/golden/gemm_workspace_bytes.json: what the two queries returned before the GEMM host code was rewritten around one plan per
    path (tools/gen_golden.py gemm_workspace; host arithmetic at the fallback CU count 256, which is also the MI355X's)."""
    import json
    from d2s import lib
    rec = json.load(open(os.path.join(REPO, "tests", "golden", "gemm_workspace_bytes.json")))
    assert len(rec["d2s_gemm_f32_workspace_bytes"]) > 1500 and len(rec["d2s_linear_wgrad_workspace_bytes"]) == 108
    for name, rows in rec.items():
        for *args, want in rows:
            assert lib.query(name, *args) == want, (name, args, want)
