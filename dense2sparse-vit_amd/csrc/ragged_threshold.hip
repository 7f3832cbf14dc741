// Training the dynamic keep ratio on the ragged packed batch (--patch-score-threshold --ragged-train): what a
// threshold stage on a packed batch [total, D] with cu_seqlens [B+1] (image b owns rows cu[b] .. cu[b+1]-1, row cu[b] is its CLS token)
// adds to the kernels of ragged.hip and ragged_train.hip once it has to be differentiated and to carry a loss.
//   half_mean_concat_varlen_bwd_kernel (+ _vec)   the backward of half_mean_concat_varlen_kernel (ragged.hip)
//   ragged_mask_loss_kernel<BWD>                  the mask loss of a packed stage: per image, KL(q || softmax(scores)) or the squared
//                                                 difference, q the teacher target gathered at the surviving tokens and renormalised
//   ragged_teacher_rows_kernel                    the teacher's token of every packed row and the row weights of the token distillation
// Latency / HBM work, no atomics, no memset: every output element is written exactly once.
#include "d2s_common.h"
#include "d2s_hip_ragged_threshold.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// Backward of the split / token-mean / concat on a packed batch.  The forward gave every row of a segment (CLS included) the mean over the
// segment's T non-CLS rows in the second half of the columns, so a non-CLS row's gradient there is (1 / T) * the sum of g_out[., c] over
// ALL rows of the segment, the CLS row's is 0 (it is not part of the mean); the first half is a copy.  T = 0: zeros.  Wave w of a
// workgroup sums rows w, w+4, ... and the four partial sums are combined as (0+1)+(2+3).
// grid: (column chunks over the two halves, B) - the forward's
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_mean_concat_varlen_bwd_kernel(const float* __restrict__ g_out, const int* __restrict__ cu,
                                                                          float* __restrict__ g_x, int C) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = C >> 1;
    const int chunks = (half + 63) >> 6;
    const bool second = (int)blockIdx.x >= chunks;
    const int c = (second ? half : 0) + ((int)blockIdx.x - (second ? chunks : 0)) * 64 + lane;
    const bool ok = c < (second ? C : half);
    const int r0 = cu[blockIdx.y], n = cu[blockIdx.y + 1] - r0;      // rows of the segment, CLS included
    if (n <= 0) return;
    const int T = n - 1;
    const long base = (long)r0 * C + c;
    if (!second) {
        if (ok)
            for (int t = wave; t < n; t += 4) g_x[base + (long)t * C] = g_out[base + (long)t * C];
        return;
    }
    float s = 0.f;
    if (ok)
        for (int t = wave; t < n; t += 4) s += g_out[base + (long)t * C];
    red[wave][lane] = s;
    __syncthreads();
    const float g = T > 0 ? ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)T : 0.f;
    if (ok)
        for (int t = wave; t < n; t += 4) g_x[base + (long)t * C] = t == 0 ? 0.f : g;
}

// 16-byte form (C a multiple of 8): a lane owns 4 consecutive columns, as in half_mean_concat_varlen_vec_kernel
__global__ __launch_bounds__(256) void half_mean_concat_varlen_bwd_vec_kernel(const float* __restrict__ g_out, const int* __restrict__ cu,
                                                                              float* __restrict__ g_x, int C) {
    __shared__ f32x4 red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = C >> 1;
    const int chunks = (half + 255) >> 8;
    const bool second = (int)blockIdx.x >= chunks;
    const int c = (second ? half : 0) + ((int)blockIdx.x - (second ? chunks : 0)) * 256 + lane * 4;
    const bool ok = c < (second ? C : half);
    const int r0 = cu[blockIdx.y], n = cu[blockIdx.y + 1] - r0;
    if (n <= 0) return;
    const int T = n - 1;
    const long base = (long)r0 * C + c;
    if (!second) {
        if (ok)
#pragma unroll 4
            for (int t = wave; t < n; t += 4)
                *reinterpret_cast<f32x4*>(g_x + base + (long)t * C) = *reinterpret_cast<const f32x4*>(g_out + base + (long)t * C);
        return;
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (ok)
#pragma unroll 8
        for (int t = wave; t < n; t += 4) s += *reinterpret_cast<const f32x4*>(g_out + base + (long)t * C);
    red[wave][lane] = s;
    __syncthreads();
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (T > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = ((red[0][lane][j] + red[1][lane][j]) + (red[2][lane][j] + red[3][lane][j])) / (float)T;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (ok)
#pragma unroll 4
        for (int t = wave; t < n; t += 4) *reinterpret_cast<f32x4*>(g_x + base + (long)t * C) = t == 0 ? zero : g;
}

// ---------------------------------------------------------------------------------------------------------
// Mask loss of a packed stage.  One workgroup per image; its T non-CLS rows r (T clamped to [0, N] and to the buffer) have scores s_r and
// original patch ids j_r = row_src[r] - 1.  q_r = target[b, j_r] / sum_r target[b, j_r] (0 when the sum is 0 or the id is outside
// [0, N)): the teacher target gathered at the survivors and renormalised, d2s_gather_renorm's recursion.
//   kl  (mode 1)  loss_rows[b] = sum_r q_r (log q_r - log_softmax(s)_r), a zero q_r contributing nothing;  d/ds_r = p_r * sum(q) - q_r
//   mse (mode 3)  loss_rows[b] = sum_r (s_r - q_r)^2;                                                      d/ds_r = 2 (s_r - q_r)
// BWD writes dscores = scale * d/ds over the image's rows, exactly 0 at the CLS row; the forward writes loss_rows[b] (0 for T = 0).
// The maximum, the sums and their combine order are softmax_rows_kernel's: per-thread strided partials, the wave butterfly, then
// (0+1)+(2+3); p = exp(s - max) * (1 / sum).  LDS: [N] scores -> exponentials, [N] q.
// ---------------------------------------------------------------------------------------------------------
enum RaggedLossMode : int { RAGGED_LOSS_KL = 1, RAGGED_LOSS_MSE = 3 };      // d2s_kl_rows' KL_PROB_TARGET / MSE_TARGET

__device__ __forceinline__ float block_sum4(float v, float* red, float* bc, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) *bc = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return *bc;
}

template <bool BWD>
__global__ __launch_bounds__(256) void ragged_mask_loss_kernel(const float* __restrict__ scores, const float* __restrict__ target,
                                                               const int* __restrict__ cu, const int* __restrict__ row_src,
                                                               float* __restrict__ out, int total, int N, int mode, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* ss = sh;
    float* qs = sh + N;
    __shared__ float red[4];
    __shared__ float bc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = min(max(cu[b], 0), total);
    int T = cu[b + 1] - r0 - 1;
    T = min(min(T, N), total - r0 - 1);              // never past the LDS arrays or the buffers
    if (T < 0) T = 0;
    if (BWD && tid == 0 && r0 < total) out[r0] = 0.f;                // the CLS row carries no score
    if (T == 0) {
        if (!BWD && tid == 0) out[b] = 0.f;
        return;
    }
    const float* sr = scores + r0 + 1;
    const int* ids = row_src + r0 + 1;
    const float* tb = target + (long)b * N;
    // ---- gather and renormalise the target
    float part = 0.f;
    for (int t = tid; t < T; t += 256) {
        const int id = ids[t] - 1;
        const float g = (id >= 0 && id < N) ? tb[id] : 0.f;
        ss[t] = sr[t];
        qs[t] = g;
        part += g;
    }
    const float qsum = block_sum4(part, red, &bc, tid);
    for (int t = tid; t < T; t += 256) qs[t] = qsum > 0.f ? qs[t] / qsum : 0.f;      // the same thread wrote qs[t]
    if (mode == RAGGED_LOSS_MSE) {
        if (BWD) {
            for (int t = tid; t < T; t += 256) out[r0 + 1 + t] = scale * (2.f * (ss[t] - qs[t]));
        } else {
            float l = 0.f;
            for (int t = tid; t < T; t += 256) {
                const float d = ss[t] - qs[t];
                l += d * d;
            }
            l = block_sum4(l, red, &bc, tid);
            if (tid == 0) out[b] = l;
        }
        return;
    }
    // ---- softmax statistics over the T scores
    float m = -INFINITY;
    for (int t = tid; t < T; t += 256) m = fmaxf(m, ss[t]);
    m = wave_max(m);
    __syncthreads();
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) bc = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    m = bc;
    float sum = 0.f;
    for (int t = tid; t < T; t += 256) {
        const float e = expf(ss[t] - m);
        if (BWD) ss[t] = e;
        sum += e;
    }
    sum = block_sum4(sum, red, &bc, tid);
    if (BWD) {
        const float inv = 1.0f / sum;
        const float qtot = qsum > 0.f ? 1.f : 0.f;                   // sum_r q_r: 1, or 0 when the image's target vanished
        for (int t = tid; t < T; t += 256) out[r0 + 1 + t] = scale * (ss[t] * inv * qtot - qs[t]);
    } else {
        const float lse = m + logf(sum);
        float l = 0.f;
        for (int t = tid; t < T; t += 256) {
            const float q = qs[t];
            if (q > 0.f) l += q * (logf(q) - (ss[t] - lse));
        }
        l = block_sum4(l, red, &bc, tid);
        if (tid == 0) out[b] = l;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Teacher rows and row weights of the token distillation on a packed batch: packed row r of image b takes teacher token
// token_t[b, row_src[r] - 1, :] and the weight 1 / (total - B); a CLS row (or an id outside [0, N)) takes zeros and the weight 0.
// grid: (B, 4): image b writes the rows from its CLS row up to the next image's (the first image from row 0, the last one up to `total`,
// both clamped to [0, total]) - together every row, once - and the four workgroups of an image interleave over them, one wave per row.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ragged_teacher_rows_kernel(const float* __restrict__ token_t, long image_stride,
                                                                  const int* __restrict__ cu, const int* __restrict__ row_src,
                                                                  float* __restrict__ out, float* __restrict__ w, int B, int total, int N,
                                                                  int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int c0 = min(max(cu[b], 0), total);
    const int r0 = b == 0 ? 0 : c0;
    const int r1 = b == B - 1 ? total : min(max(cu[b + 1], r0), total);
    const int nv = D >> 2;
    const float wt = total > B ? 1.0f / (float)(total - B) : 0.f;
    const float* tb = token_t + (long)b * image_stride;
    for (int r = r0 + (int)blockIdx.y * 4 + wave; r < r1; r += 4 * (int)gridDim.y) {
        const int id = row_src[r] - 1;
        const bool live = r != c0 && id >= 0 && id < N;
        f32x4* d4 = reinterpret_cast<f32x4*>(out + (long)r * D);
        if (live) {
            const f32x4* s4 = reinterpret_cast<const f32x4*>(tb + (long)id * D);
            for (int c = lane; c < nv; c += 64) d4[c] = s4[c];
        } else {
            for (int c = lane; c < nv; c += 64) d4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (lane == 0) w[r] = live ? wt : 0.f;
    }
}

}  // namespace

extern "C" {

// g_out [total, C], cu_seqlens [B+1] -> g_x [total, C]
int d2s_half_mean_concat_varlen_bwd(const float* g_out, const int* cu_seqlens, float* g_x, int B, int C, hipStream_t stream) {
    if (!g_out || !cu_seqlens || !g_x || B <= 0 || C <= 0 || (C & 1)) return D2S_ERR_ARG;
    const bool vec = (C % 8 == 0) && ((reinterpret_cast<uintptr_t>(g_out) | reinterpret_cast<uintptr_t>(g_x)) & 15) == 0;
    if (vec) {
        const int chunks = ((C >> 1) + 255) >> 8;
        hipLaunchKernelGGL(half_mean_concat_varlen_bwd_vec_kernel, dim3(2 * chunks, B), dim3(256), 0, stream, g_out, cu_seqlens, g_x, C);
        return d2s_check_launch();
    }
    const int chunks = ((C >> 1) + 63) >> 6;
    hipLaunchKernelGGL(half_mean_concat_varlen_bwd_kernel, dim3(2 * chunks, B), dim3(256), 0, stream, g_out, cu_seqlens, g_x, C);
    return d2s_check_launch();
}

// scores [total], target [B, N], row_src [total] -> loss_rows [B].  mode 1: kl_div, 3: mse.  N <= 8192.
int d2s_ragged_mask_loss_fwd(const float* scores, const float* target, const int* cu_seqlens, const int* row_src, float* loss_rows, int B,
                             int total, int N, int mode, hipStream_t stream) {
    if (!scores || !target || !cu_seqlens || !row_src || !loss_rows || B <= 0 || total <= 0 || N <= 0 || N > 8192) return D2S_ERR_ARG;
    if (mode != RAGGED_LOSS_KL && mode != RAGGED_LOSS_MSE) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_mask_loss_kernel<false>, dim3(B), dim3(256), (size_t)2 * N * sizeof(float), stream, scores, target,
                       cu_seqlens, row_src, loss_rows, total, N, mode, 1.0f);
    return d2s_check_launch();
}

// the same inputs -> dscores [total] = scale * d loss_rows[b] / d scores over every image's rows, 0 at the CLS rows
int d2s_ragged_mask_loss_bwd(const float* scores, const float* target, const int* cu_seqlens, const int* row_src, float* dscores, int B,
                             int total, int N, int mode, float scale, hipStream_t stream) {
    if (!scores || !target || !cu_seqlens || !row_src || !dscores || B <= 0 || total <= 0 || N <= 0 || N > 8192) return D2S_ERR_ARG;
    if (mode != RAGGED_LOSS_KL && mode != RAGGED_LOSS_MSE) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_mask_loss_kernel<true>, dim3(B), dim3(256), (size_t)2 * N * sizeof(float), stream, scores, target,
                       cu_seqlens, row_src, dscores, total, N, mode, scale);
    return d2s_check_launch();
}

// token_t: B images of N rows of D floats, image b at token_t + b * image_stride (rows dense) -> out [total, D], w [total]
int d2s_ragged_teacher_rows(const float* token_t, long image_stride, const int* cu_seqlens, const int* row_src, float* out, float* w, int B,
                            int total, int N, int D, hipStream_t stream) {
    if (!token_t || !cu_seqlens || !row_src || !out || !w || B <= 0 || total <= 0 || N <= 0 || D <= 0 || (D & 3) || image_stride < 0 ||
        (image_stride & 3))
        return D2S_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(token_t) | reinterpret_cast<uintptr_t>(out)) & 15) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_teacher_rows_kernel, dim3(B, 4), dim3(256), 0, stream, token_t, image_stride, cu_seqlens, row_src, out, w, B,
                       total, N, D);
    return d2s_check_launch();
}

}  // extern "C"
