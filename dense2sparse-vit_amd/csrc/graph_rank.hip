// Graph ranking of a block's tokens (--graph-rank T; DESIGN.md section 29 - the build's own definition): T steps of the unnormalised
// PageRank iteration over the block's attention graph, per image and head,
//   s^{t+1}[j] = sum_i s^t[i] P[i, j],   P[i, j] = exp(scale q_i . k_j - lse_i),   s^0 = 1 / n (or the caller's vector).
//   graph_rank_kernel   ONE application of s_out = s_in P; the C entry issues it T times, ping-ponging between the workspace and the output
// The kernel is ltp_score_kernel<false, false> (ltp.hip) with a weight on every query row: a wave keeps 32 scaled keys in registers while
// the 32-row query tiles of the image stream through LDS (the next tile prefetched through registers), S = Q K^T runs on the f32-input
// MFMA (the lane owns ONE key and 16 of the tile's 32 query rows), P is recomputed from the saved log-sum-exp by the attention
// backward's own expression.  The tile's 32 weights travel with its 32 lse values; the lane's column sum is col = fma(w_i, p, col) in a
// fixed order - 16 rows per tile in register order, tiles ascending, then the two half-waves added once - and goes straight to
// s_out[(b H + h) n + j]: the rank stays per head, so there are no partials and no fold.  The helpers are copies of ltp.hip's (which
// copied them from attention_f32.hip), so that both files compile exactly as they did.
// Grid: key tile of 128 x (image, head).  fp32 only, no atomics, no memset, fixed summation orders: two calls on equal inputs give the
// same bits.
#include "d2s_common.h"
#include "d2s_hip_graph_rank.h"

namespace {

constexpr int DH = 64;
constexpr int PITCH = 68;  // floats; 16-B aligned rows, conflict-free ds_read_b128 for 16 distinct rows

// operand fragment of one token row for lane (row, half): r[t] = base[row][8t + 4half .. +3] * scale
__device__ __forceinline__ void load_rows_regs(const float* __restrict__ base, long ld, int row, int nrows, int half, float scale,
                                               f32x4 (&r)[8]) {
    if (row < nrows) {
        const float* p = base + (long)row * ld + 4 * half;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            r[t] = *reinterpret_cast<const f32x4*>(p + 8 * t);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[t][j] *= scale;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) r[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// cooperative load of a 32-row x 64-float tile (rows row0.., zero-filled beyond nrows) by 256 threads: 2 float4 each
__device__ __forceinline__ void tile_load(const float* __restrict__ base, long ld, int row0, int nrows, int tid, f32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256, row = row0 + (f >> 4), d4 = (f & 15) * 4;
        r[i] = row < nrows ? *reinterpret_cast<const f32x4*>(base + (long)row * ld + d4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
__device__ __forceinline__ void tile_store(float* __restrict__ S, int tid, const f32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256;
        *reinterpret_cast<f32x4*>(&S[(f >> 4) * PITCH + (f & 15) * 4]) = r[i];
    }
}

// acc[r] += sum_d X[rowlane][d] * Yreg[d]  : A operand from an LDS tile (row = lane&31), B operand from registers
__device__ __forceinline__ void mma_lds_reg(const float* __restrict__ S, int l31, int half, const f32x4 (&y)[8], f32x16& acc) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&S[l31 * PITCH + 8 * t + 4 * half]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(a[j], y[t][j], acc);
    }
}

struct GraphRankArgs {
    const float* qkv; const float* lse; const float* s_in; float* s_out;
    int n, H; float scale;
};

// s_in, s_out: [B, H, n], the layout of lse.  UNIFORM: s_in is not read, every query row weighs 1 / n - the unweighted column sum,
// multiplied by 1.f / n once.
template <bool UNIFORM>
__global__ __launch_bounds__(256, 3) void graph_rank_kernel(GraphRankArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[32 * PITCH];
    __shared__ float lse_s[32], w_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all key tiles of one head on one XCD (they stream the same Q panel)
    const int H = a.H, n = a.n;
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    if (bx * 128 >= n) return;                          // block-uniform (the grid has no such tile; kept with the loop it came from)
    const long stat0 = ((long)b * H + h) * n;
    const float* qb = a.qkv + (long)b * n * ld + h * DH;
    const float* kb = qb + (long)H * DH;
    const float* lse_b = a.lse + stat0;
    const float* w_b = UNIFORM ? nullptr : a.s_in + stat0;
    const int k0 = bx * 128 + wave * 32;
    const bool active = k0 < n;

    f32x4 kreg[8];
    load_rows_regs(kb, ld, k0 + l31, n, half, a.scale, kreg);  // scaled keys, as the backward scales them

    const int ntiles = (n + 31) / 32;
    f32x4 qr[2];
    float lr = 0.f, wr = 0.f;
    float col = 0.f;
    tile_load(qb, ld, 0, n, tid, qr);
    if (tid < 32) {
        lr = tid < n ? lse_b[tid] : INFINITY;
        if (!UNIFORM) wr = tid < n ? w_b[tid] : 0.f;
    }
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        tile_store(Qs, tid, qr);
        if (tid < 32) { lse_s[tid] = lr; if (!UNIFORM) w_s[tid] = wr; }
        __syncthreads();
        if (t + 1 < ntiles) {       // the next tile's rows travel through registers while this tile is multiplied
            tile_load(qb, ld, (t + 1) * 32, n, tid, qr);
            if (tid < 32) {
                const int qi = (t + 1) * 32 + tid;
                lr = qi < n ? lse_b[qi] : INFINITY;
                if (!UNIFORM) wr = qi < n ? w_b[qi] : 0.f;
            }
        }
        if (!active) continue;
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        mma_lds_reg(Qs, l31, half, kreg, s);   // S[query = row(r,half)][key = l31], scaled
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = mfma32_row(r, half);
            const float p = __expf(s[r] - lse_s[qi]);  // rows beyond n carry lse = +inf -> p = 0, and weight 0
            if (UNIFORM) col += p;
            else col = fmaf(w_s[qi], p, col);
        }
    }
    if (!active) return;
    col += __shfl_xor(col, 32, 64);      // the other half-wave's 16 rows of every tile (commutative: both halves hold the same bits)
    if (UNIFORM) col *= 1.f / (float)n;
    if (half == 0 && k0 + l31 < n) a.s_out[stat0 + k0 + l31] = col;
}

}  // namespace

extern "C" {

int d2s_graph_rank_f32(const float* qkv, const float* lse, const float* w0, float* rank, float* ws, int B, int n, int H, float scale,
                       int iters, hipStream_t stream) {
    if (!qkv || !lse || !rank || B <= 0 || H <= 0 || n < 1 || n > 8192 || iters < 1 || iters > 1024) return D2S_ERR_ARG;
    if (iters >= 2 && !ws) return D2S_ERR_ARG;
    if (w0 && (w0 == rank || w0 == ws)) return D2S_ERR_ARG;      // a launch never reads the vector it writes
    const dim3 grid((n + 127) / 128, B * H), block(256);
    const float* src = w0;
    for (int t = 0; t < iters; ++t) {
        float* dst = ((iters - 1 - t) & 1) ? ws : rank;          // the last launch writes rank for either parity of iters
        const GraphRankArgs a{qkv, lse, src, dst, n, H, scale};
        if (src) hipLaunchKernelGGL(graph_rank_kernel<false>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(graph_rank_kernel<true>, grid, block, 0, stream, a);
        src = dst;
    }
    return d2s_check_launch();
}

}  // extern "C"
