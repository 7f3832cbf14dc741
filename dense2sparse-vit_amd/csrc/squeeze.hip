// Pruning and squeezing at a pruning stage (--squeeze-dropped): the selector's kept / dropped lists decide who
// survives, and every dropped token is folded into the ONE kept token it resembles most (cosine of the fp32 rows), weighted by
// exp(cosine) against the kept token's own weight E = exp(1).  No counterpart in the reference (TPS, Wei et al. CVPR 2023, restated for
// this selector).  Row layout of one image:  x = [CLS | T scored tokens] (n = T + 1 rows),  y = [CLS | k kept tokens] (k + 1 rows).
//   match     grid (32-row tile of the dropped list, image): a wave owns 32-column tiles of the kept list and takes the 32 x 32 dots on the
//             fp32 matrix cores; squared norms ride along in the same loop; the m x k similarities live in registers only.
//   forward   grid (4 output rows, image): the image's dst / weight / id lists staged once per workgroup in LDS, one wave per output
//             row, sources added in ascending list order (ballot scan): fixed-order sums, no atomics.
//   backward  grid (16 dx rows, image): the source row and coefficient of each dx row found once per workgroup, one wave per row; every
//             row of dx written exactly once.
// All accesses to token rows are 16 bytes per lane; results are bit-identical run to run.
#include "d2s_common.h"
#include "d2s_hip_squeeze.h"
#include <limits.h>

namespace {

constexpr int SQ_ROWS = 16;      // dx rows per workgroup of the backward
constexpr int SQ_FWD_ROWS = 4;   // output rows per workgroup of the forward: one per wave, as in gather_pack_kernel (16 and 8 measured slower)
constexpr int SQ_MAXV = 4;       // 16-byte vectors per lane and row: D <= 4 * 64 * 4 = 1024
constexpr int SQ_MAXN = 4096;    // longest sequence: 12 bytes of dynamic LDS per dropped token in the forward, < 48 KiB
constexpr int SQ_TILE = 32;      // dropped rows per workgroup and kept rows per wave step of the match (one 32x32x2 MFMA tile)
constexpr float SQ_E = 2.71828174591064453125f;      // expf(1.0f), correctly rounded: the kept token's own weight

__device__ __forceinline__ f32x4 fma4(float w, f32x4 v, f32x4 acc) {
    acc[0] = fmaf(w, v[0], acc[0]); acc[1] = fmaf(w, v[1], acc[1]); acc[2] = fmaf(w, v[2], acc[2]); acc[3] = fmaf(w, v[3], acc[3]);
    return acc;
}
__device__ __forceinline__ float inv_norm(float ss) { return ss > 0.f ? 1.0f / sqrtf(ss) : 0.f; }
// (c, j) beats (bc, bj): a larger cosine, or the same cosine at a lower position
__device__ __forceinline__ bool beats(float c, int j, float bc, int bj) { return c > bc || (c == bc && j < bj); }

// ---------------------------------------------------------------------------------------------------------
// match.  Lane l of a wave holds row (l & 31) of the dropped tile (A) and of the current kept tile (B), columns 8 c + 4 (l >> 5) .. + 3 of
// chunk c: MFMA q of a chunk multiplies columns 8 c + q and 8 c + 4 + q, so every dot runs over the D columns in one fixed order whatever
// its position - bit-identical rows give bit-identical dots, norms and cosines.  A row past the end of a list or with an id outside
// [0, T) reads the CLS row instead (in bounds, never its own address) and is masked out afterwards.  Each lane keeps the running best of
// its 16 accumulator rows over its column (ascending kept tiles, strict >: the lowest position stays); one butterfly over the 32 columns
// and one LDS step over the 4 waves finish it.  dst = -1, sim = 0 for a dropped id outside [0, T) or when no kept id is valid.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void squeeze_match_kernel(const float* __restrict__ x, const long long* __restrict__ kept,
                                                            const long long* __restrict__ dropped, int* __restrict__ dst,
                                                            float* __restrict__ sim, int n, int k, int D) {
    __shared__ float wc[4][SQ_TILE];
    __shared__ int wj[4][SQ_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * SQ_TILE;
    const int T = n - 1, m = T - k, nchunk = D >> 3;
    const float* xb = x + (long)b * n * D;
    const long long did = i0 + r < m ? dropped[(long)b * m + i0 + r] : -1;
    const bool dok = did >= 0 && did < T;
    const f32x4* ap = reinterpret_cast<const f32x4*>(xb + (dok ? 1 + did : 0) * (long)D) + half;
    float bestc[16];
    int bestj[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { bestc[q] = -INFINITY; bestj[q] = INT_MAX; }
    for (int j0 = wave * SQ_TILE; j0 < k; j0 += 4 * SQ_TILE) {
        const int j = j0 + r;
        const long long kid = j < k ? kept[(long)b * k + j] : -1;
        const bool kok = kid >= 0 && kid < T;
        const f32x4* bp = reinterpret_cast<const f32x4*>(xb + (kok ? 1 + kid : 0) * (long)D) + half;
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        float ssa = 0.f, ssb = 0.f;
        for (int c0 = 0; c0 < nchunk; c0 += 4) {      // D is a multiple of 64: 4 chunks = one 128-byte line of each row per step
            f32x4 a[4], bv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { a[c] = ap[2 * (c0 + c)]; bv[c] = bp[2 * (c0 + c)]; }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc = mfma32(a[c][q], bv[c][q], acc);
                    ssa = fmaf(a[c][q], a[c][q], ssa);
                    ssb = fmaf(bv[c][q], bv[c][q], ssb);
                }
        }
        ssa += __shfl_xor(ssa, 32, 64);      // the two column halves of a row: both lanes get the same bits
        ssb += __shfl_xor(ssb, 32, 64);
        const float ra = inv_norm(ssa), rb = inv_norm(ssb);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float rd = __shfl(ra, mfma32_row(q, half), 64);
            const float c = acc[q] * rd * rb;
            if (kok && c > bestc[q]) { bestc[q] = c; bestj[q] = j; }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float oc = __shfl_xor(bestc[q], o, 64);
            const int oj = __shfl_xor(bestj[q], o, 64);
            if (beats(oc, oj, bestc[q], bestj[q])) { bestc[q] = oc; bestj[q] = oj; }
        }
        if (r == 0) { wc[wave][mfma32_row(q, half)] = bestc[q]; wj[wave][mfma32_row(q, half)] = bestj[q]; }
    }
    __syncthreads();
    if (tid < SQ_TILE && i0 + tid < m) {      // wave 0, half 0: lane tid holds dropped row tid's dok
        float c = wc[0][tid];
        int j = wj[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (beats(wc[w][tid], wj[w][tid], c, j)) { c = wc[w][tid]; j = wj[w][tid]; }
        const bool ok = dok && j != INT_MAX;
        dst[(long)b * m + i0 + tid] = ok ? j : -1;
        sim[(long)b * m + i0 + tid] = ok ? c : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// forward.  y row 0 = CLS; y row 1 + j = (E x_kept(j) + sum_{i: dst_i = j} w_i x_dropped(i)) / Z_j, w_i = expf(sim_i), Z_j = E + sum w_i,
// the row itself first and the sources in ascending i; a row without a source is copied bit for bit (Z = E).  Z is summed with its
// rounding errors carried along (Fast2Sum) and added at the end, so its error does not grow with the number of sources and y's is the
// numerator chain's.  A list entry whose id or dst is out of range is staged as dst = -1 and matches no row; a kept id out of range
// contributes a zero row of its own.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_squeeze_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ kept,
                                                                 const long long* __restrict__ dropped, const int* __restrict__ dst,
                                                                 const float* __restrict__ sim, float* __restrict__ y,
                                                                 float* __restrict__ Z, int n, int k, int D) {
    extern __shared__ __attribute__((aligned(16))) float sh[];      // [m] weights, [m] dst, [m] dropped ids (both as int)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, r0 = blockIdx.x * SQ_FWD_ROWS;
    const int T = n - 1, m = T - k, nvec = D >> 2;
    float* w = sh;
    int* dj = reinterpret_cast<int*>(sh + m);
    int* id = reinterpret_cast<int*>(sh + 2 * m);
    for (int i = tid; i < m; i += 256) {
        const long long d = dropped[(long)b * m + i];
        const int t = dst[(long)b * m + i];
        const bool ok = d >= 0 && d < T && t >= 0 && t < k;
        id[i] = ok ? (int)d : 0;
        dj[i] = ok ? t : -1;
        w[i] = ok ? expf(sim[(long)b * m + i]) : 0.f;
    }
    __syncthreads();
    const float* xb = x + (long)b * n * D;
    {
        const int row = r0 + wave;      // wave-uniform
        if (row > k) return;
        bool own = true;
        int srow = 0;
        if (row > 0) {
            const long long kid = kept[(long)b * k + row - 1];
            own = kid >= 0 && kid < T;
            srow = own ? 1 + (int)kid : 0;
        }
        const f32x4* xs = reinterpret_cast<const f32x4*>(xb + (long)srow * D);
        f32x4* od = reinterpret_cast<f32x4*>(y + ((long)b * (k + 1) + row) * D);
        f32x4 v[SQ_MAXV], acc[SQ_MAXV];
#pragma unroll
        for (int u = 0; u < SQ_MAXV; ++u) {
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (own && u * 64 + lane < nvec) v[u] = xs[u * 64 + lane];
        }
        float zs = SQ_E, zc = 0.f;      // Z as a compensated sum: zs >= E >= w_i, so (w_i - (t - zs)) is the addition's exact error
        bool any = false;
        if (row > 0) {
            for (int base = 0; base < m; base += 64) {
                const int i = base + lane;
                unsigned long long hits = __ballot(i < m && dj[i] == row - 1);
                while (hits) {
                    const int ii = base + __ffsll((long long)hits) - 1;
                    hits &= hits - 1;
                    const float wi = w[ii];
                    const f32x4* sp = reinterpret_cast<const f32x4*>(xb + (long)(1 + id[ii]) * D);
                    if (!any) {
#pragma unroll
                        for (int u = 0; u < SQ_MAXV; ++u) acc[u] = f32x4{SQ_E * v[u][0], SQ_E * v[u][1], SQ_E * v[u][2], SQ_E * v[u][3]};
                        any = true;
                    }
                    const float t = zs + wi;
                    zc += wi - (t - zs);
                    zs = t;
#pragma unroll
                    for (int u = 0; u < SQ_MAXV; ++u)
                        if (u * 64 + lane < nvec) acc[u] = fma4(wi, sp[u * 64 + lane], acc[u]);
                }
            }
            zs += zc;
            if (lane == 0) Z[(long)b * k + row - 1] = zs;
        }
#pragma unroll
        for (int u = 0; u < SQ_MAXV; ++u)
            if (u * 64 + lane < nvec)
                od[u * 64 + lane] = any ? f32x4{acc[u][0] / zs, acc[u][1] / zs, acc[u][2] / zs, acc[u][3] / zs} : v[u];
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward (dst and sim are constants).  dx row 0 = g row 0; a kept token at position j gets (E / Z_j) g[1 + j], or g[1 + j] bit for bit
// when Z_j == E (no source: the forward copied it); a dropped token at list position i gets (w_i / Z_dst) g[1 + dst_i]; a row in neither
// list, or whose list entry is out of range, gets zeros.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_squeeze_bwd_kernel(const float* __restrict__ g, const long long* __restrict__ kept,
                                                                 const long long* __restrict__ dropped, const int* __restrict__ dst,
                                                                 const float* __restrict__ sim, const float* __restrict__ Z,
                                                                 float* __restrict__ dx, int n, int k, int D) {
    __shared__ int src[SQ_ROWS];        // >= 0: row of g, -1: zeros
    __shared__ float coef[SQ_ROWS];     // < 0: copy the row, else multiply by it (every coefficient is a ratio of positive weights)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, r0 = blockIdx.x * SQ_ROWS;
    const int T = n - 1, m = T - k, nvec = D >> 2;
    if (tid < SQ_ROWS) {
        src[tid] = r0 + tid == 0 ? 0 : -1;
        coef[tid] = -1.f;
    }
    __syncthreads();
    for (int j = tid; j < k; j += 256) {
        const long long d = kept[(long)b * k + j];
        if (d >= 0 && d < T && d + 1 >= r0 && d + 1 < r0 + SQ_ROWS) {
            const float z = Z[(long)b * k + j];
            src[(int)d + 1 - r0] = 1 + j;
            coef[(int)d + 1 - r0] = z == SQ_E ? -1.f : SQ_E / z;
        }
    }
    for (int i = tid; i < m; i += 256) {
        const long long d = dropped[(long)b * m + i];
        if (d >= 0 && d < T && d + 1 >= r0 && d + 1 < r0 + SQ_ROWS) {
            const int t = dst[(long)b * m + i];
            if (t >= 0 && t < k) {
                src[(int)d + 1 - r0] = 1 + t;
                coef[(int)d + 1 - r0] = expf(sim[(long)b * m + i]) / Z[(long)b * k + t];
            }
        }
    }
    __syncthreads();
    constexpr int NQ = SQ_ROWS / 4;
    int sq[NQ];
    f32x4 v[NQ][SQ_MAXV];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {      // this wave's rows r0 + wave + 4 q: all their loads are issued before the first is used
        const int i = r0 + wave + 4 * q;
        sq[q] = i < n ? src[wave + 4 * q] : -1;
#pragma unroll
        for (int u = 0; u < SQ_MAXV; ++u) {
            v[q][u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (sq[q] >= 0 && u * 64 + lane < nvec)
                v[q][u] = reinterpret_cast<const f32x4*>(g + ((long)b * (k + 1) + sq[q]) * D)[u * 64 + lane];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = r0 + wave + 4 * q;
        if (i >= n) break;
        const float cf = coef[wave + 4 * q];
        f32x4* od = reinterpret_cast<f32x4*>(dx + ((long)b * n + i) * D);
#pragma unroll
        for (int u = 0; u < SQ_MAXV; ++u)
            if (u * 64 + lane < nvec)
                od[u * 64 + lane] = (sq[q] < 0 || cf < 0.f) ? v[q][u] : f32x4{cf * v[q][u][0], cf * v[q][u][1], cf * v[q][u][2], cf * v[q][u][3]};
    }
}

bool squeeze_args_ok(int B, int n, int k, int D) {
    if (B <= 0 || B > 65535 || n < 2 || n > SQ_MAXN) return false;
    if (k < 1 || k > n - 1) return false;
    return D >= 64 && D <= 256 * SQ_MAXV && (D & 63) == 0;      // d2s_gather_fuse_fwd's rule
}

}  // namespace

extern "C" {

// x [B,n,D], kept [B,k], dropped [B,m] (m = n-1-k) -> dst [B,m] int32 (position in kept), sim [B,m]
int d2s_squeeze_match(const float* x, const long long* kept, const long long* dropped, int B, int n, int k, int D, int* dst, float* sim,
                      hipStream_t stream) {
    if (!squeeze_args_ok(B, n, k, D)) return D2S_ERR_ARG;
    const int m = n - 1 - k;
    if (!x || !kept || ((!dropped || !dst || !sim) && m > 0)) return D2S_ERR_ARG;
    if (m == 0) return D2S_OK;
    hipLaunchKernelGGL(squeeze_match_kernel, dim3((m + SQ_TILE - 1) / SQ_TILE, B), dim3(256), 0, stream, x, kept, dropped, dst, sim, n, k,
                       D);
    return d2s_check_launch();
}

// x, the id lists and a plan (dst, sim) [B,m] -> y [B,k+1,D], Z [B,k]
int d2s_gather_squeeze_fwd(const float* x, const long long* kept, const long long* dropped, const int* dst, const float* sim, int B, int n,
                           int k, int D, float* y, float* Z, hipStream_t stream) {
    if (!squeeze_args_ok(B, n, k, D)) return D2S_ERR_ARG;
    const int m = n - 1 - k;
    if (!x || !kept || !y || !Z || ((!dropped || !dst || !sim) && m > 0)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gather_squeeze_fwd_kernel, dim3((k + 1 + SQ_FWD_ROWS - 1) / SQ_FWD_ROWS, B), dim3(256), (size_t)3 * m * sizeof(float),
                       stream, x, kept, dropped, dst, sim, y, Z, n, k, D);
    return d2s_check_launch();
}

// g [B,k+1,D], the id lists, the plan and the forward's Z -> dx [B,n,D] (every element written)
int d2s_gather_squeeze_bwd(const float* g, const long long* kept, const long long* dropped, const int* dst, const float* sim,
                           const float* Z, int B, int n, int k, int D, float* dx, hipStream_t stream) {
    if (!squeeze_args_ok(B, n, k, D)) return D2S_ERR_ARG;
    const int m = n - 1 - k;
    if (!g || !kept || !Z || !dx || ((!dropped || !dst || !sim) && m > 0)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gather_squeeze_bwd_kernel, dim3((n + SQ_ROWS - 1) / SQ_ROWS, B), dim3(256), 0, stream, g, kept, dropped, dst, sim,
                       Z, dx, n, k, D);
    return d2s_check_launch();
}

}  // extern "C"
