// Evo-ViT baseline (--method evo; DESIGN.md section 26 - the build's own definition, no counterpart in the reference): slow-fast token
// update.  Every token stays in the full tensor X [B, 1+T, D]; a slow-fast block runs on [CLS | the k tokens of the highest global score g
// | one representative row r of the other m = T - k] (d2s_gather_fuse_fwd, unchanged) and what is stated here surrounds it:
//
//   d2s_evo_select       the score evolution  g[kept_i] = (1 - tau) g[kept_i] + tau mean_h a[h, 1+i]  (or its start, g = mean_h a[h, 1+t])
//                        and the re-selection among ALL T tokens, d2s_select_topk's rule, in one launch
//   d2s_evo_scatter_fwd  the write-back into X: CLS and kept rows replaced, every other row += (y_r - r), the "fast update"
//   d2s_evo_scatter_bwd  its backward in the block's output: rows copied, the gradient of y_r = delta = the sum of the dropped rows
//   d2s_evo_gather_bwd   the backward of the gather AND of the fast update's -r term, in place on the gradient of X
//
// HBM-bound row moves like fuse.hip / select.hip: one wave per row, 16-byte accesses, a row's id is one wave-uniform load (the delta row
// stages the dropped ids in LDS), every sum in a fixed order, no atomics, no memset, nothing read back by the host, every output element
// written exactly once: results are bit-identical run to run and the launches are legal inside a captured step.  fp32 in every
// arithmetic mode (the residual stream).
#include "d2s_common.h"
#include "d2s_hip_evo.h"

namespace {

constexpr int EMAXV = 4;      // 16-byte vectors per lane and row: D <= 4 * 64 * 4 = 1024
constexpr int EMAXT = 4095;   // 1 + T <= 4096 rows, as d2s_gather_fuse_fwd takes them: 2 T floats of LDS stay under 32 KiB

// ---------------------------------------------------------------------------------------------------------
// score evolution and re-selection, one workgroup per image.  The scores are staged in LDS (from the CLS row, or from g_in and then
// updated at the previous kept ids - distinct, so every entry has one writer), written out, ranked by counting (value descending, equal
// values lowest index first) and compacted by wave ballots exactly as select_topk_kernel does on the emitted fp32 values.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void evo_select_kernel(const float* __restrict__ g_in, const long long* __restrict__ kept_prev,
                                                         const float* __restrict__ cls_row, float* __restrict__ g_out,
                                                         long long* __restrict__ kept, long long* __restrict__ dropped, int H, int T, int k,
                                                         float tau) {
    extern __shared__ __attribute__((aligned(16))) float sh[];  // [T] scores, then [T] keep flags (as int)
    float* ps = sh;
    int* flag = reinterpret_cast<int*>(sh + T);
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    if (!kept_prev) {
        const float* ab = cls_row + (long)b * H * (1 + T) + 1;
        for (int t = tid; t < T; t += 256) {
            float s = 0.f;
            for (int h = 0; h < H; ++h) s += ab[(long)h * (1 + T) + t];
            ps[t] = s / (float)H;
        }
    } else {
        for (int t = tid; t < T; t += 256) ps[t] = g_in[(long)b * T + t];
        __syncthreads();
        const float* ab = cls_row + (long)b * H * (k + 2) + 1;
        const float keep_w = 1.0f - tau;
        for (int i = tid; i < k; i += 256) {
            const long long id = kept_prev[(long)b * k + i];
            if (id < 0 || id >= T) continue;
            float s = 0.f;
            for (int h = 0; h < H; ++h) s += ab[(long)h * (k + 2) + i];
            ps[id] = fmaf(tau, s / (float)H, keep_w * ps[id]);
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) g_out[(long)b * T + t] = ps[t];
    for (int i = tid; i < T; i += 256) {
        const float v = ps[i];
        int cnt = 0;
        for (int j = 0; j < T; ++j) {
            const float u = ps[j];
            cnt += (u > v) || (u == v && j < i);
        }
        flag[i] = cnt < k;
    }
    __syncthreads();
    long long* ko = kept + (long)b * k;
    long long* dr = dropped + (long)b * (T - k);
    int base = 0;  // number of kept ids among indices below the current 256-chunk
    for (int c0 = 0; c0 < T; c0 += 256) {
        const int i = c0 + tid;
        const int f = (i < T) ? flag[i] : 0;
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_tot[w];
        const int pos = base + woff + before;
        if (i < T) {
            if (f) { if (pos < k) ko[pos] = i; }
            else if (i - pos < T - k) dr[i - pos] = i;       // a NaN score ranks below nothing: never past the lists' ends
        }
        base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
}

// A row of the lists: unit u of image b is CLS (u = 0), kept[u - 1] (u <= k) or dropped[u - 1 - k].  -> the row of X, or -1 for an id
// outside [0, T) (nothing is dereferenced for it).
__device__ __forceinline__ int evo_unit_row(const long long* __restrict__ kept, const long long* __restrict__ dropped, int b, int u, int T,
                                            int k) {
    if (u == 0) return 0;
    const long long id = u <= k ? kept[(long)b * k + (u - 1)] : dropped[(long)b * (T - k) + (u - 1 - k)];
    return (id < 0 || id >= T) ? -1 : 1 + (int)id;
}

// ---------------------------------------------------------------------------------------------------------
// write-back, one wave per unit (4 per workgroup): X[CLS] = yc[0], X[1 + kept_i] = yc[1 + i], X[1 + dropped_j] += yc[k + 1] - xc[k + 1]
// (one subtraction, then one addition).  The lists partition the T tokens, so every row of X has exactly one writer, which is also the
// only reader of that row: in place without a hazard.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 6) void evo_scatter_fwd_kernel(const float* __restrict__ yc, const float* __restrict__ xc,
                                                              const long long* __restrict__ kept, const long long* __restrict__ dropped,
                                                              float* __restrict__ X, int T, int k, int D, long units_total) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= units_total) return;
    const int b = (int)(unit / (T + 1)), u = (int)(unit - (long)b * (T + 1));
    const int row = evo_unit_row(kept, dropped, b, u, T, k);
    if (row < 0) return;
    const int nvec = D >> 2, R = k + 2;
    f32x4* xd = reinterpret_cast<f32x4*>(X + ((long)b * (T + 1) + row) * D);
    const f32x4* ys = reinterpret_cast<const f32x4*>(yc + ((long)b * R + min(u, k + 1)) * D);
    f32x4 v[EMAXV];
#pragma unroll
    for (int q = 0; q < EMAXV; ++q)
        if (q * 64 + lane < nvec) v[q] = ys[q * 64 + lane];
    if (u > k) {
        const f32x4* rs = reinterpret_cast<const f32x4*>(xc + ((long)b * R + (k + 1)) * D);
        f32x4 r[EMAXV], o[EMAXV];
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) { r[q] = rs[q * 64 + lane]; o[q] = xd[q * 64 + lane]; }
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) {
                const f32x4 d = v[q] - r[q];
                v[q] = o[q] + d;
            }
    }
#pragma unroll
    for (int q = 0; q < EMAXV; ++q)
        if (q * 64 + lane < nvec) xd[q * 64 + lane] = v[q];
}

// ---------------------------------------------------------------------------------------------------------
// backward of the write-back in yc, one launch.  The first B * nchunk workgroups make the delta rows as gather_fuse_fwd_kernel makes the
// package row with every weight 1: workgroup (b, chunk) stages image b's dropped ids in LDS, its four waves each add a contiguous quarter
// of the dropped rows over the chunk's 256 columns in ascending j, and wave 0 adds the four partial rows as (0 + 1) + (2 + 3).  Every
// other workgroup copies 4 rows, one wave per row: dyc[0] = dX[CLS], dyc[1 + i] = dX[1 + kept_i].
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void evo_scatter_bwd_kernel(const float* __restrict__ dX, const long long* __restrict__ kept,
                                                              const long long* __restrict__ dropped, float* __restrict__ dyc, int T, int k,
                                                              int D, int nchunk, int delta_blocks, long copy_rows_total) {
    extern __shared__ __attribute__((aligned(16))) int id[];    // [m] dropped ids, -1: out of range
    __shared__ f32x4 part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = T - k, R = k + 2, nvec = D >> 2;
    if ((int)blockIdx.x >= delta_blocks) {
        const long row = ((long)blockIdx.x - delta_blocks) * 4 + wave;
        if (row >= copy_rows_total) return;
        const int b = (int)(row / (k + 1)), r = (int)(row - (long)b * (k + 1));
        const int srow = r == 0 ? 0 : 1 + min(max((int)kept[(long)b * k + (r - 1)], 0), T - 1);
        const f32x4* xs = reinterpret_cast<const f32x4*>(dX + ((long)b * (T + 1) + srow) * D);
        f32x4* od = reinterpret_cast<f32x4*>(dyc + ((long)b * R + r) * D);
        f32x4 v[EMAXV];
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) v[q] = xs[q * 64 + lane];
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) od[q * 64 + lane] = v[q];
        return;
    }
    const int b = (int)blockIdx.x / nchunk, chunk = (int)blockIdx.x - b * nchunk;
    for (int j = tid; j < m; j += 256) {
        const long long d = dropped[(long)b * m + j];
        id[j] = (d >= 0 && d < T) ? (int)d : -1;
    }
    __syncthreads();
    const int c = chunk * 64 + lane;
    const bool active = c < nvec;
    const int seg = (m + 3) >> 2;
    const int j0 = min(m, wave * seg), j1 = min(m, j0 + seg);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4* xb = reinterpret_cast<const f32x4*>(dX + ((long)b * (T + 1) + 1) * D) + c;
        int j = j0;
        for (; j + 4 <= j1; j += 4) {
            f32x4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = xb[(long)max(id[j + q], 0) * nvec];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (id[j + q] >= 0) acc += v[q];           // wave-uniform
        }
        for (; j < j1; ++j)
            if (id[j] >= 0) acc += xb[(long)id[j] * nvec];
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (part[0][lane][q] + part[1][lane][q]) + (part[2][lane][q] + part[3][lane][q]);
        reinterpret_cast<f32x4*>(dyc + ((long)b * R + (R - 1)) * D)[c] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward of the gather and of the fast update's -r term, in place on dX (on entry the gradient of the written-back X, whose CLS and
// kept rows are dead: the write-back replaced them).  One wave per unit: dX[CLS] = dxc[0], dX[1 + kept_i] = dxc[1 + i],
// dX[1 + dropped_j] += (g_j / S) (dxc[k + 1] - delta), delta = dyc[k + 1]; the weight is formed as gather_fuse_fwd_kernel forms it.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 6) void evo_gather_bwd_kernel(const float* __restrict__ dxc, const float* __restrict__ dyc,
                                                             const float* __restrict__ g, const float* __restrict__ S,
                                                             const long long* __restrict__ kept, const long long* __restrict__ dropped,
                                                             float* __restrict__ dX, int T, int k, int D, long units_total) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= units_total) return;
    const int b = (int)(unit / (T + 1)), u = (int)(unit - (long)b * (T + 1));
    const int row = evo_unit_row(kept, dropped, b, u, T, k);
    if (row < 0) return;
    const int nvec = D >> 2, R = k + 2;
    f32x4* xd = reinterpret_cast<f32x4*>(dX + ((long)b * (T + 1) + row) * D);
    const f32x4* gs = reinterpret_cast<const f32x4*>(dxc + ((long)b * R + min(u, k + 1)) * D);
    f32x4 v[EMAXV];
#pragma unroll
    for (int q = 0; q < EMAXV; ++q)
        if (q * 64 + lane < nvec) v[q] = gs[q * 64 + lane];
    if (u > k) {
        const float Sb = S[b];
        const float w = Sb > 0.f ? g[(long)b * T + (row - 1)] / Sb : 0.f;
        if (w == 0.f) return;                              // the forward added nothing of this row to r: its gradient passes unchanged
        const f32x4* ds = reinterpret_cast<const f32x4*>(dyc + ((long)b * R + (k + 1)) * D);
        f32x4 d[EMAXV], o[EMAXV];
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) { d[q] = ds[q * 64 + lane]; o[q] = xd[q * 64 + lane]; }
#pragma unroll
        for (int q = 0; q < EMAXV; ++q)
            if (q * 64 + lane < nvec) {
                const f32x4 e = v[q] - d[q];
                v[q] = f32x4{fmaf(w, e[0], o[q][0]), fmaf(w, e[1], o[q][1]), fmaf(w, e[2], o[q][2]), fmaf(w, e[3], o[q][3])};
            }
    }
#pragma unroll
    for (int q = 0; q < EMAXV; ++q)
        if (q * 64 + lane < nvec) xd[q * 64 + lane] = v[q];
}

bool evo_args_ok(int B, int T, int k, int D) {
    if (B <= 0 || B > 65535 || T < 2 || T > EMAXT || k < 1 || k > T - 1) return false;
    return D >= 4 && D <= 256 * EMAXV && (D & 3) == 0;
}

}  // namespace

extern "C" {

// kept_prev NULL: g_out [B,T] = mean over heads of cls_row [B,H,1+T]'s token columns (g_in unused).  Otherwise g_out = g_in with the
// entries at kept_prev [B,k] evolved by cls_row [B,H,k+2].  -> g_out, kept [B,k], dropped [B,T-k] = d2s_select_topk(g_out, k).
int d2s_evo_select(const float* g_in, const long long* kept_prev, const float* cls_row, float* g_out, long long* kept, long long* dropped,
                   int B, int H, int T, int k, float tau, hipStream_t stream) {
    if (!cls_row || !g_out || !kept || !dropped || (kept_prev && !g_in)) return D2S_ERR_ARG;
    if (B <= 0 || B > 65535 || H <= 0 || T < 2 || T > EMAXT || k < 1 || k > T - 1 || !(tau >= 0.f && tau <= 1.f)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(evo_select_kernel, dim3(B), dim3(256), (size_t)2 * T * sizeof(float), stream, g_in, kept_prev, cls_row, g_out, kept,
                       dropped, H, T, k, tau);
    return d2s_check_launch();
}

// yc, xc [B,k+2,D], kept [B,k], dropped [B,T-k] -> X [B,1+T,D] updated in place
int d2s_evo_scatter_fwd(const float* yc, const float* xc, const long long* kept, const long long* dropped, float* X, int B, int T, int k,
                        int D, hipStream_t stream) {
    if (!evo_args_ok(B, T, k, D) || !yc || !xc || !kept || !dropped || !X) return D2S_ERR_ARG;
    const long units = (long)B * (T + 1);
    hipLaunchKernelGGL(evo_scatter_fwd_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, stream, yc, xc, kept, dropped, X, T, k, D,
                       units);
    return d2s_check_launch();
}

// dX [B,1+T,D] (the gradient of the written-back X), kept, dropped -> dyc [B,k+2,D], every element written
int d2s_evo_scatter_bwd(const float* dX, const long long* kept, const long long* dropped, float* dyc, int B, int T, int k, int D,
                        hipStream_t stream) {
    if (!evo_args_ok(B, T, k, D) || !dX || !kept || !dropped || !dyc) return D2S_ERR_ARG;
    const int nchunk = (D + 255) >> 8;
    const int delta_blocks = B * nchunk;
    const long copy_rows = (long)B * (k + 1);
    hipLaunchKernelGGL(evo_scatter_bwd_kernel, dim3((unsigned)(delta_blocks + (copy_rows + 3) / 4)), dim3(256),
                       (size_t)(T - k) * sizeof(int), stream, dX, kept, dropped, dyc, T, k, D, nchunk, delta_blocks, copy_rows);
    return d2s_check_launch();
}

// dxc, dyc [B,k+2,D] (dyc as d2s_evo_scatter_bwd wrote it), g [B,T], S [B] (d2s_gather_fuse_fwd's), kept, dropped -> dX [B,1+T,D] in place
int d2s_evo_gather_bwd(const float* dxc, const float* dyc, const float* g, const float* S, const long long* kept, const long long* dropped,
                       float* dX, int B, int T, int k, int D, hipStream_t stream) {
    if (!evo_args_ok(B, T, k, D) || !dxc || !dyc || !g || !S || !kept || !dropped || !dX) return D2S_ERR_ARG;
    const long units = (long)B * (T + 1);
    hipLaunchKernelGGL(evo_gather_bwd_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, stream, dxc, dyc, g, S, kept, dropped, dX, T,
                       k, D, units);
    return d2s_check_launch();
}

}  // extern "C"
