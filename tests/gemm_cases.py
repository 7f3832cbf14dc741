"""The shapes of tests/test_gemm_gpu.py, in one place so that the CPU tier (tests/test_gemm_ref_cpu.py) can hold torch's own fp32 product to
the same per-element bound on every one of them.  Shapes are the smallest that still reach the branch they name: the tile choice of
csrc/gemm_f32.hip leaves 64x64 only once a launch has several thousand tiles, so the three larger tiles need tens of thousands of rows, at
a short K.  Each is confirmed at run time by the plan query (d2s_gemm_f32_plan)."""
import torch

NT, NN, TN = 0, 1, 2
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}

# tile -> (M, N): ragged against both tile edges, N % 4 == 0 (the 16-byte epilogue); N - 1 is the odd width of the dword epilogue
TILE_SHAPES = {(64, 64): (300, 132), (128, 64): (27272, 132), (64, 128): (9736, 580), (128, 128): (27272, 324)}
# the three main loops: (name, K, N shrinks by one for NT / ldc grows by one for NN, A starts one float past a 16-byte boundary)
TILE_LOOPS = [("rk", 16, False, False), ("rk", 48, False, False), ("fast", 16, True, False), ("fast", 48, True, False),
              ("guarded", 20, False, False), ("guarded", 48, False, True)]

WG_ORDER = [(64 * i - 1, 64, 16) for i in range(1, 18)]          # nwg & 7 takes every residue (and 0 twice)
SMALL_EDGES = [(M, N, K) for M in (1, 3, 4, 5) for N in (1, 3, 4, 5) for K in (16, 20)]
KSPLIT_SHAPES = [(600, 384, 1536), (3168, 384, 1536), (257, 96, 2048), (1000, 200, 1024), (64, 64, 4096), (257, 96, 1544)]
WGRAD_TOKENS = (1, 15, 16, 255, 256, 257, 1000, 4099, 1024)        # 1024: the only count that splits K AND keeps the guard-free loop
WGRAD_SHAPES = ((4, 4), (10, 24), (130, 132), (384, 96))          # (n_out, n_in)
COLSUM_SHAPES = [(M, N) for M in (1, 63, 64, 65, 5000) for N in (1, 70, 384)]
REMAP_CASES = [(rpi, skip, N) for rpi in (1, 3, 196) for skip in (1, 2) for N in (132, 131)]
REMAP_M, REMAP_K = 400, 16                                        # 400 is no multiple of 3 or 196


def tile_case_shapes():
    """(M, N, K) of every tile / loop case, both N forms"""
    out = []
    for (M, N) in TILE_SHAPES.values():
        for _, K, odd, _ in TILE_LOOPS:
            out.append((M, N - 1 if odd else N, K))
            out.append((M, N, K))
    return sorted(set(out))


def all_shapes():
    """every (M, N, K) the GPU test multiplies, the weight gradient as (n_out, n_in, tokens)"""
    s = set(tile_case_shapes()) | set(WG_ORDER) | set(SMALL_EDGES) | set(KSPLIT_SHAPES)
    s |= {(no, ni, t) for t in WGRAD_TOKENS for (no, ni) in WGRAD_SHAPES}
    s |= {(REMAP_M, N, REMAP_K) for _, _, N in REMAP_CASES}
    return sorted(s)


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def operands(layout, M, N, K):
    """fp32 A, B of the layout's shapes: A ~ N(0, 1), B ~ N(0, 1) / 4"""
    g = gen(layout, M, N, K)
    a_shape = (K, M) if layout == TN else (M, K)
    b_shape = (N, K) if layout == NT else (K, N)
    return torch.randn(a_shape, generator=g), torch.randn(b_shape, generator=g) * 0.25
