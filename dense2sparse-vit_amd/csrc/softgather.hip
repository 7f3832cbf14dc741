// Soft (differentiable) token gather of the perturbed top-k training mode - the product the reference states in comments only
// (vit_models/dynamic_vit.py:896-900: `spatial_x = pred_score @ spatial_x  # shape: (B, K, D)`, `x = torch.cat((cls_x, spatial_x), dim=1)`):
//
//   forward   y[b, 1 + i, :] = sum_j ind[b, i, j] * x[b, 1 + j, :]      y[b, 0, :] = x[b, 0, :]          [k x N] . [N x D]
//   backward  dx[b, 1 + j, :] = sum_i ind[b, i, j] * g[b, 1 + i, :]     dx[b, 0, :] = g[b, 0, :]         [N x k] . [k x D]
//             dind[b, i, j]   = sum_d g[b, 1 + i, d] * x[b, 1 + j, d]                                    [k x D] . [D x N]
//
// One launch per product, the batch on blockIdx.z.  Exact fp32 on v_mfma_f32_32x32x2_f32, operand order and LDS images as in
// gemm_f32.hip: a reduction-contiguous operand ([row][K] in memory) keeps the [row][16 k] image with 16-byte chunks XOR-swizzled by
// (row >> 2) & 3, a row-contiguous one ([K][row]) the [k][row] image with the row swizzled by ((k >> 2) & 3) << 3 ^ (k & 1) << 4; MFMA step
// s of a 16-deep K-step multiplies k = s (lanes 0-31) and k = 8 + s (lanes 32-63) of BOTH operands.  Tile 64 x 128 x 16, 256 threads =
// 2 x 2 waves of 32 x 64.  None of k / N (137, 98, 58, 172, 8 ...) is a multiple of the tile: every global access is guarded, the
// padding is zeros.  No atomics, no split-K (the reductions are at most 768 deep), every output element is written exactly once by
// one thread in a fixed accumulation order - the same (x, ind) gives the same bits on every run.
// A one-hot `ind` makes the forward a sum of 1.0 * x and exact zeros: it then equals d2s_gather_pack_fwd bit for bit.
#include "d2s_common.h"

namespace {

constexpr int BK = 16, BM = 64, BN = 128, WM = 32, WN = 64, NT = WN / 32;

struct SoftGatherArgs {
    const float* A; const float* B; float* C;      // per image: C[M][N] = op(A) . op(B), reduction length K
    long lda, ldb, ldc;
    long sA, sB, sC;                               // elements between consecutive images
    int M, N, K;
    int vecA, vecB;                                // 16-byte loads allowed (leading dimension, image stride and base all 16-byte aligned)
    const float* cls_src; float* cls_dst;          // row 0 of every image (the CLS token / its gradient) passes through; null: nothing
    long s_cls_src, s_cls_dst;
};

// LAY 0: operand stored [rows][K] (k contiguous);  LAY 1: stored [K][rows] (row contiguous).  BR rows x 16 k, BR / 64 float4 per thread.
template <int LAY, int BR>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, long ld, int row0, int k0, int rows, int kend, int vec, int tid,
                                          f32x4 (&r)[BR / 64]) {
#pragma unroll
    for (int i = 0; i < BR / 64; ++i) {
        const int f = tid + i * 256;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (LAY == 0) {
            const int row = row0 + (f >> 2), k = k0 + (f & 3) * 4;
            if (row < rows) {
                const float* p = P + (long)row * ld + k;
                if (vec && k + 3 < kend) {
                    v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (k + 0 < kend) v[0] = p[0];
                    if (k + 1 < kend) v[1] = p[1];
                    if (k + 2 < kend) v[2] = p[2];
                    if (k + 3 < kend) v[3] = p[3];
                }
            }
        } else {
            const int k = k0 + f / (BR / 4), row = row0 + (f % (BR / 4)) * 4;
            if (k < kend) {
                const float* p = P + (long)k * ld + row;
                if (vec && row + 3 < rows) {
                    v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    if (row + 0 < rows) v[0] = p[0];
                    if (row + 1 < rows) v[1] = p[1];
                    if (row + 2 < rows) v[2] = p[2];
                    if (row + 3 < rows) v[3] = p[3];
                }
            }
        }
        r[i] = v;
    }
}

template <int LAY, int BR>
__device__ __forceinline__ void store_tile(float* __restrict__ S, int tid, const f32x4 (&r)[BR / 64]) {
#pragma unroll
    for (int i = 0; i < BR / 64; ++i) {
        const int f = tid + i * 256;
        if (LAY == 0) {      // [row][16 k], chunk kq of a row at (kq ^ ((row >> 2) & 3)) << 2
            const int row = f >> 2, kq = f & 3;
            *reinterpret_cast<f32x4*>(&S[row * BK + ((kq ^ ((row >> 2) & 3)) << 2)]) = r[i];
        } else {             // [k][row], element (k, row) at k * BR + (row ^ swizzle(k)); the swizzle keeps groups of 4 rows together
            const int k = f / (BR / 4), row = (f % (BR / 4)) * 4;
            *reinterpret_cast<f32x4*>(&S[k * BR + (row ^ (((k >> 2) & 3) << 3) ^ ((k & 1) << 4))]) = r[i];
        }
    }
}

// the 8 k-values a lane feeds to the 8 MFMA steps of a K-step: k = 8 * half + s of tile row `row`
template <int LAY, int BR>
__device__ __forceinline__ void read_frag(const float* __restrict__ S, int row, int half, float (&v)[8]) {
    if (LAY == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(&S[row * BK + (((2 * half + c) ^ ((row >> 2) & 3)) << 2)]);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * c + j] = q[j];
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = 8 * half + s;
            v[s] = S[k * BR + (row ^ (((k >> 2) & 3) << 3) ^ ((k & 1) << 4))];
        }
    }
}

template <int ALAY, int BLAY>
__global__ __launch_bounds__(256) void soft_gather_kernel(SoftGatherArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (BM + BN)];
    float* As = smem;                 // [2][BM x BK]
    float* Bs = smem + 2 * BK * BM;   // [2][BN x BK]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
    const long img = blockIdx.z;
    const float* A = p.A + img * p.sA;
    const float* B = p.B + img * p.sB;
    float* C = p.C + img * p.sC;

    if (p.cls_src && blockIdx.y == 0) {      // the CLS row of this workgroup's columns
        const int c = col0 + tid;
        if (tid < BN && c < p.N) p.cls_dst[img * p.s_cls_dst + c] = p.cls_src[img * p.s_cls_src + c];
    }

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int nk = (p.K + BK - 1) / BK;
    f32x4 ra[BM / 64], rb[BN / 64];
    load_tile<ALAY, BM>(A, p.lda, row0, 0, p.M, p.K, p.vecA, tid, ra);
    load_tile<BLAY, BN>(B, p.ldb, col0, 0, p.N, p.K, p.vecB, tid, rb);
    store_tile<ALAY, BM>(As, tid, ra);
    store_tile<BLAY, BN>(Bs, tid, rb);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {      // tile kt + 1 travels from memory under the MFMAs of tile kt
            load_tile<ALAY, BM>(A, p.lda, row0, (kt + 1) * BK, p.M, p.K, p.vecA, tid, ra);
            load_tile<BLAY, BN>(B, p.ldb, col0, (kt + 1) * BK, p.N, p.K, p.vecB, tid, rb);
        }
        float a[8], b[NT][8];
        read_frag<ALAY, BM>(As + cur * BK * BM, wm * WM + l31, half, a);
#pragma unroll
        for (int j = 0; j < NT; ++j) read_frag<BLAY, BN>(Bs + cur * BK * BN, wn * WN + j * 32 + l31, half, b[j]);
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = mfma32(a[s], b[j][s], acc[j]);
        if (kt + 1 < nk) {
            store_tile<ALAY, BM>(As + (cur ^ 1) * BK * BM, tid, ra);
            store_tile<BLAY, BN>(Bs + (cur ^ 1) * BK * BN, tid, rb);
        }
        __syncthreads();
    }

    // C/D register r of lane l: row (r & 3) + 8 * (r >> 2) + 4 * half, column l & 31: a half-wave stores 32 consecutive floats of a row
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = col0 + wn * WN + j * 32 + l31;
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = row0 + wm * WM + mfma32_row(r, half);
            if (m < p.M) C[(long)m * p.ldc + n] = acc[j][r];
        }
    }
}

// dz[r][t] = p[r][t] * (g[r][t] - sum_u g[r][u] p[r][u]): the softmax of the keep probabilities (F.softmax, dynamic_vit.py:551) backward.
// One workgroup per row, fixed reduction order.
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ dz, int T) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pr = p + (long)blockIdx.x * T;
    const float* gr = g + (long)blockIdx.x * T;
    float dot = 0.f;
    for (int t = tid; t < T; t += 256) dot += pr[t] * gr[t];
    dot = wave_sum(dot);
    if (lane == 0) red[wave] = dot;
    __syncthreads();
    dot = (red[0] + red[1]) + (red[2] + red[3]);
    for (int t = tid; t < T; t += 256) dz[(long)blockIdx.x * T + t] = pr[t] * (gr[t] - dot);
}

inline int vec_ok(const void* base, long ld, long stride) {
    return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && ld % 4 == 0 && stride % 4 == 0;
}

template <int ALAY, int BLAY>
int launch(SoftGatherArgs& a, int batch, hipStream_t stream) {
    a.vecA = vec_ok(a.A, a.lda, a.sA);
    a.vecB = vec_ok(a.B, a.ldb, a.sB);
    const dim3 grid((a.N + BN - 1) / BN, (a.M + BM - 1) / BM, batch);
    hipLaunchKernelGGL((soft_gather_kernel<ALAY, BLAY>), grid, dim3(256), 0, stream, a);
    return d2s_check_launch();
}

inline bool bad_shape(int B, int n, int k, int D) { return B <= 0 || B > 65535 || n < 2 || k <= 0 || k > n - 1 || D <= 0; }

}  // namespace

extern "C" {

// x [B,n,D], ind [B,k,n-1] -> y [B,k+1,D]
int d2s_soft_gather_fwd(const float* x, const float* ind, float* y, int B, int n, int k, int D, hipStream_t stream) {
    if (!x || !ind || !y || bad_shape(B, n, k, D)) return D2S_ERR_ARG;
    const int N = n - 1;
    SoftGatherArgs a{};
    a.A = ind; a.lda = N; a.sA = (long)k * N;                    // [k][N], reduction contiguous
    a.B = x + D; a.ldb = D; a.sB = (long)n * D;                  // [N][D] = [K][cols]
    a.C = y + D; a.ldc = D; a.sC = (long)(k + 1) * D;
    a.M = k; a.N = D; a.K = N;
    a.cls_src = x; a.s_cls_src = a.sB; a.cls_dst = y; a.s_cls_dst = a.sC;
    return launch<0, 1>(a, B, stream);
}

// g [B,k+1,D], ind [B,k,n-1] -> dx [B,n,D]; every row of dx is written (a token no sample selected gets its zeros from the product)
int d2s_soft_gather_bwd_x(const float* g, const float* ind, float* dx, int B, int n, int k, int D, hipStream_t stream) {
    if (!g || !ind || !dx || bad_shape(B, n, k, D)) return D2S_ERR_ARG;
    const int N = n - 1;
    SoftGatherArgs a{};
    a.A = ind; a.lda = N; a.sA = (long)k * N;                    // ind^T: stored [K = k][rows = N]
    a.B = g + D; a.ldb = D; a.sB = (long)(k + 1) * D;            // [k][D] = [K][cols]
    a.C = dx + D; a.ldc = D; a.sC = (long)n * D;
    a.M = N; a.N = D; a.K = k;
    a.cls_src = g; a.s_cls_src = a.sB; a.cls_dst = dx; a.s_cls_dst = a.sC;
    return launch<1, 1>(a, B, stream);
}

// g [B,k+1,D], x [B,n,D] -> dind [B,k,n-1]
int d2s_soft_gather_bwd_ind(const float* g, const float* x, float* dind, int B, int n, int k, int D, hipStream_t stream) {
    if (!g || !x || !dind || bad_shape(B, n, k, D)) return D2S_ERR_ARG;
    const int N = n - 1;
    SoftGatherArgs a{};
    a.A = g + D; a.lda = D; a.sA = (long)(k + 1) * D;            // [k][D], reduction contiguous
    a.B = x + D; a.ldb = D; a.sB = (long)n * D;                  // [N][D], reduction contiguous
    a.C = dind; a.ldc = N; a.sC = (long)k * N;
    a.M = k; a.N = N; a.K = D;
    return launch<0, 0>(a, B, stream);
}

// probs, grad_probs [rows,T] -> grad_scores [rows,T]
int d2s_softmax_rows_bwd(const float* probs, const float* grad_probs, float* grad_scores, int rows, int T, hipStream_t stream) {
    if (!probs || !grad_probs || !grad_scores || rows <= 0 || T <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3(rows), dim3(256), 0, stream, probs, grad_probs, grad_scores, T);
    return d2s_check_launch();
}

}  // extern "C"
