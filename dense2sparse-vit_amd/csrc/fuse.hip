// Token fusion at a pruning stage (--fuse-dropped): the kept-token gather of select.hip plus ONE extra row per image, the "package token"
// f = sum_{j in dropped} (p_j / S) x_j with S = sum_{j in dropped} p_j and p the stage's keep probabilities, and the backward of both.
// No counterpart in the reference (EViT's fused token / SPViT's package token, restated for this selector): DESIGN.md section 20.
// Row layout of one image:  x = [CLS | T scored tokens | t package tokens of earlier stages]          (n = 1 + T + t rows)
//                           y = [CLS | k kept tokens   | t package tokens, copied | f]                (k + t + 2 rows)
// HBM-bound row moves like gather_pack_kernel / scatter_unpack_kernel: 16-byte accesses, one wave per copied row, ids and weights of
// the dropped set staged once per workgroup in LDS, every sum taken in a fixed order (no atomics): results are bit-identical run to run.
#include "d2s_common.h"

namespace {

constexpr int FROWS = 16;     // dx rows per workgroup of the backward
constexpr int FMAXV = 4;      // 16-byte vectors per lane and row in the backward: D <= 4 * 64 * 4 = 1024

__device__ __forceinline__ f32x4 fma4(float w, f32x4 v, f32x4 acc) {
    acc[0] = fmaf(w, v[0], acc[0]); acc[1] = fmaf(w, v[1], acc[1]); acc[2] = fmaf(w, v[2], acc[2]); acc[3] = fmaf(w, v[3], acc[3]);
    return acc;
}
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float acc) {
    return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], fmaf(a[0], b[0], acc))));
}

// ---------------------------------------------------------------------------------------------------------
// forward, one launch.  The first B * nchunk workgroups make the package rows: workgroup (b, chunk) stages image b's dropped ids and
// weights in LDS (S by a fixed-order wave / LDS reduction, w_j = p_j / S), then its four waves each reduce a contiguous quarter of the
// dropped rows over the chunk's 256 columns (a lane owns 4 columns, ascending j, fused multiply-adds) and wave 0 adds the four partial
// rows as (0 + 1) + (2 + 3).  They come first in the grid because they are the longest.  Every other workgroup copies 4 rows, one wave
// per row, exactly like gather_pack_kernel.  An empty dropped set, or one whose probabilities sum to 0, gives f = 0.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_fuse_fwd_kernel(const float* __restrict__ x, const float* __restrict__ p,
                                                              const long long* __restrict__ kept, const long long* __restrict__ dropped,
                                                              float* __restrict__ y, float* __restrict__ S_out, int n, int t, int k, int D,
                                                              int nchunk, int fused_blocks, long copy_rows_total) {
    extern __shared__ __attribute__((aligned(16))) float sh[];   // [m] weights, then [m] dropped ids (as int)
    __shared__ float red[4];
    __shared__ f32x4 part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = n - 1 - t, m = T - k, R = k + t + 2, nvec = D >> 2;
    if ((int)blockIdx.x >= fused_blocks) {
        const long row = ((long)blockIdx.x - fused_blocks) * 4 + wave;     // copied row index over the whole batch
        if (row >= copy_rows_total) return;
        const int b = (int)(row / (R - 1)), r = (int)(row - (long)b * (R - 1));
        int srow = 0;
        if (r > k) srow = 1 + T + (r - 1 - k);
        else if (r > 0) srow = 1 + min(max((int)kept[(long)b * k + (r - 1)], 0), T - 1);
        const f32x4* xs = reinterpret_cast<const f32x4*>(x + ((long)b * n + srow) * D);
        f32x4* od = reinterpret_cast<f32x4*>(y + ((long)b * R + r) * D);
        f32x4 v[FMAXV];
#pragma unroll
        for (int u = 0; u < FMAXV; ++u)
            if (u * 64 + lane < nvec) v[u] = xs[u * 64 + lane];
#pragma unroll
        for (int u = 0; u < FMAXV; ++u)
            if (u * 64 + lane < nvec) od[u * 64 + lane] = v[u];
        return;
    }
    const int b = (int)blockIdx.x / nchunk, chunk = (int)blockIdx.x - b * nchunk;
    float* w = sh;
    int* id = reinterpret_cast<int*>(sh + m);
    float s = 0.f;
    for (int j = tid; j < m; j += 256) {
        const long long d = dropped[(long)b * m + j];
        const bool ok = d >= 0 && d < T;
        const float pv = ok ? p[(long)b * T + d] : 0.f;
        id[j] = ok ? (int)d : 0;
        w[j] = pv;
        s += pv;
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float S = (red[0] + red[1]) + (red[2] + red[3]);
    for (int j = tid; j < m; j += 256) w[j] = S > 0.f ? w[j] / S : 0.f;     // each thread rewrites the entries it wrote
    if (chunk == 0 && tid == 0) S_out[b] = S;
    __syncthreads();
    const int c = chunk * 64 + lane;
    const bool active = c < nvec;
    const int seg = (m + 3) >> 2;
    const int j0 = min(m, wave * seg), j1 = min(m, j0 + seg);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4* xb = reinterpret_cast<const f32x4*>(x + ((long)b * n + 1) * D) + c;
        int j = j0;
        for (; j + 4 <= j1; j += 4) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = xb[(long)id[j + u] * nvec];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (w[j + u] != 0.f) acc = fma4(w[j + u], v[u], acc);      // wave-uniform; a zero weight (an id out of range, S = 0) adds nothing
        }
        for (; j < j1; ++j)
            if (w[j] != 0.f) acc = fma4(w[j], xb[(long)id[j] * nvec], acc);
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (part[0][lane][q] + part[1][lane][q]) + (part[2][lane][q] + part[3][lane][q]);
        reinterpret_cast<f32x4*>(y + ((long)b * R + (R - 1)) * D)[c] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward, one launch, grid (ceil(n / FROWS), B): a workgroup owns FROWS consecutive rows of dx and the matching entries of dp, a wave
// four of them.  The source of each row is found once per workgroup (LDS): CLS, kept and carried rows copy their row of g; a
// dropped row j gets w_j * g_f and dp_j = (<x_j, g_f> - <f, g_f>) / S (g_f, the last row of g, stays in registers; <f, g_f> is taken by
// every wave in the same lane order, so all workgroups of an image use the same bits); a row in neither list gets zeros.  Every row of
// dx and every entry of dp is written exactly once: no memset, no atomics.  f is read back from the forward's y.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_fuse_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                              const float* __restrict__ p, const float* __restrict__ S,
                                                              const float* __restrict__ y, const long long* __restrict__ kept,
                                                              const long long* __restrict__ dropped, float* __restrict__ dx,
                                                              float* __restrict__ dp, int n, int t, int k, int D) {
    __shared__ int src[FROWS];    // >= 0: row of g to copy, -1: zeros, -2: dropped
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, r0 = blockIdx.x * FROWS;
    const int T = n - 1 - t, m = T - k, R = k + t + 2, nvec = D >> 2;
    // g_f, f and S do not depend on the ids: their loads are in flight while the source table is built
    const float Sb = S[b];
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + (long)b * R * D);
    const f32x4* gfp = gb + (long)(R - 1) * nvec;
    const f32x4* fp = reinterpret_cast<const f32x4*>(y + ((long)b * R + (R - 1)) * D);
    f32x4 gf[FMAXV];
    float cpart = 0.f;
#pragma unroll
    for (int u = 0; u < FMAXV; ++u) {
        gf[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (u * 64 + lane < nvec) {
            gf[u] = gfp[u * 64 + lane];
            cpart = dot4(fp[u * 64 + lane], gf[u], cpart);
        }
    }
    if (tid < FROWS) {
        const int i = r0 + tid;
        src[tid] = i == 0 ? 0 : (i > T ? 1 + k + (i - 1 - T) : -1);
    }
    __syncthreads();
    for (int j = tid; j < k; j += 256) {
        const long long d = kept[(long)b * k + j];
        if (d >= 0 && d < T && d + 1 >= r0 && d + 1 < r0 + FROWS) src[(int)d + 1 - r0] = 1 + j;
    }
    for (int j = tid; j < m; j += 256) {
        const long long d = dropped[(long)b * m + j];
        if (d >= 0 && d < T && d + 1 >= r0 && d + 1 < r0 + FROWS) src[(int)d + 1 - r0] = -2;
    }
    __syncthreads();
    const float fg = wave_sum(cpart);
    // this wave's rows are r0 + wave + 4 q: all their loads are issued before the first of them is used
    constexpr int NQ = FROWS / 4;
    int sq[NQ];
    float pj[NQ];
    f32x4 v[NQ][FMAXV];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = r0 + wave + 4 * q;
        const int s = i < n ? src[wave + 4 * q] : -1;
        sq[q] = s;
        pj[q] = 0.f;
        if (i < n && s != -1) {
            const f32x4* rp = s >= 0 ? gb + (long)s * nvec : reinterpret_cast<const f32x4*>(x + ((long)b * n + i) * D);
#pragma unroll
            for (int u = 0; u < FMAXV; ++u)
                if (u * 64 + lane < nvec) v[q][u] = rp[u * 64 + lane];
            if (s == -2) pj[q] = p[(long)b * T + (i - 1)];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int i = r0 + wave + 4 * q;
        if (i >= n) break;
        const int s = sq[q];
        f32x4* od = reinterpret_cast<f32x4*>(dx + ((long)b * n + i) * D);
        float dpv = 0.f;
        if (s >= 0) {
#pragma unroll
            for (int u = 0; u < FMAXV; ++u)
                if (u * 64 + lane < nvec) od[u * 64 + lane] = v[q][u];
        } else if (s == -1) {
#pragma unroll
            for (int u = 0; u < FMAXV; ++u)
                if (u * 64 + lane < nvec) od[u * 64 + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            const float wj = Sb > 0.f ? pj[q] / Sb : 0.f;
            float dpart = 0.f;
#pragma unroll
            for (int u = 0; u < FMAXV; ++u)
                if (u * 64 + lane < nvec) {
                    dpart = dot4(v[q][u], gf[u], dpart);
                    od[u * 64 + lane] = f32x4{wj * gf[u][0], wj * gf[u][1], wj * gf[u][2], wj * gf[u][3]};
                }
            const float xg = wave_sum(dpart);
            dpv = Sb > 0.f ? (xg - fg) / Sb : 0.f;
        }
        if (lane == 0 && i >= 1 && i <= T) dp[(long)b * T + (i - 1)] = dpv;
    }
}

bool fuse_args_ok(int B, int n, int t, int k, int D) {
    if (B <= 0 || B > 65535 || t < 0 || k < 0 || n <= 0 || n > 4096) return false;     // forward: 8 bytes of dynamic LDS per dropped token, < 32 KiB
    if (n - 1 - t < 1 || k > n - 1 - t) return false;
    return D >= 64 && D <= 256 * FMAXV && (D & 63) == 0;      // the widths the model produces: multiples of one 64-wide head up to 1024
}

}  // namespace

extern "C" {

// x [B,n,D], p [B,T], kept [B,k], dropped [B,T-k] (T = n-1-t) -> y [B,k+t+2,D], S [B]
int d2s_gather_fuse_fwd(const float* x, const float* p, const long long* kept, const long long* dropped, float* y, float* S_out, int B,
                        int n, int t, int k, int D, hipStream_t stream) {
    if (!fuse_args_ok(B, n, t, k, D)) return D2S_ERR_ARG;
    const int m = n - 1 - t - k;
    if (!x || !p || !y || !S_out || (!kept && k > 0) || (!dropped && m > 0)) return D2S_ERR_ARG;
    const int nchunk = (D + 255) >> 8;
    const int fused_blocks = B * nchunk;
    const long copy_rows = (long)B * (k + t + 1);
    const long blocks = fused_blocks + (copy_rows + 3) / 4;
    if (blocks > 0x7fffffffL) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gather_fuse_fwd_kernel, dim3((unsigned)blocks), dim3(256), (size_t)2 * m * sizeof(float), stream, x, p, kept,
                       dropped, y, S_out, n, t, k, D, nchunk, fused_blocks, copy_rows);
    return d2s_check_launch();
}

// g [B,k+t+2,D], the forward's x, p, S, y and id lists -> dx [B,n,D], dp [B,T] (every element of both written)
int d2s_gather_fuse_bwd(const float* g, const float* x, const float* p, const float* S, const float* y, const long long* kept,
                        const long long* dropped, float* dx, float* dp, int B, int n, int t, int k, int D, hipStream_t stream) {
    if (!fuse_args_ok(B, n, t, k, D)) return D2S_ERR_ARG;
    const int m = n - 1 - t - k;
    if (!g || !x || !p || !S || !y || !dx || !dp || (!kept && k > 0) || (!dropped && m > 0)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gather_fuse_bwd_kernel, dim3((n + FROWS - 1) / FROWS, B), dim3(256), 0, stream, g, x, p, S, y, kept, dropped,
                       dx, dp, n, t, k, D);
    return d2s_check_launch();
}

}  // extern "C"
