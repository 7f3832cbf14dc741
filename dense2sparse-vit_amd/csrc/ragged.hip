// Ragged inference through every threshold stage (--ragged-cascade): what a pruning stage after the first needs on
// a batch that is already packed [total, D] with cu_seqlens [B+1] (image b owns rows cu[b] .. cu[b+1]-1, row cu[b] is its CLS token):
// the predictor's split / token-mean / concat per segment, softmax + threshold selection over segments of different length, and the
// re-pack of the kept rows.  The reference's second stage cannot run (vit_models/dynamic_vit.py:945-946); these kernels restate, per
// segment, what half_mean_concat_kernel (select.hip), softmax_rows_kernel (select.hip), select_threshold_kernel and ragged_pack_kernel
// (threshold.hip) do per image of a dense batch, with the same arithmetic in the same order: on equal lengths they give the same bits.
// Latency / HBM work, no atomics, every output element written exactly once.
#include "d2s_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// split / token-mean / concat on a packed batch (dynamic_vit.py:540-544).  For every row r of segment b: out[r, c] = x[r, c] for
// c < C/2 and the mean of x[., c] over the segment's non-CLS rows for c >= C/2 (the CLS row is left out of the mean and receives it
// like every other row; a segment without a non-CLS row gets a mean of 0).  Wave w of a workgroup sums the non-CLS tokens w, w+4, ...
// and the four partial sums are combined as (0+1)+(2+3): half_mean_concat_kernel's order.
// grid: (column chunks over the two halves, B)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_mean_concat_varlen_kernel(const float* __restrict__ x, const int* __restrict__ cu,
                                                                      float* __restrict__ out, int C) {
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
            for (int t = wave; t < n; t += 4) out[base + (long)t * C] = x[base + (long)t * C];
        return;
    }
    float s = 0.f;
    if (ok)
        for (int t = wave; t < T; t += 4) s += x[base + (long)(t + 1) * C];
    red[wave][lane] = s;
    __syncthreads();
    const float mean = T > 0 ? ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)T : 0.f;
    if (ok)
        for (int t = wave; t < n; t += 4) out[base + (long)t * C] = mean;
}

// 16-byte form (C a multiple of 8): a lane owns 4 consecutive columns, as in half_mean_concat_vec_kernel
__global__ __launch_bounds__(256) void half_mean_concat_varlen_vec_kernel(const float* __restrict__ x, const int* __restrict__ cu,
                                                                          float* __restrict__ out, int C) {
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
                *reinterpret_cast<f32x4*>(out + base + (long)t * C) = *reinterpret_cast<const f32x4*>(x + base + (long)t * C);
        return;
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (ok)
#pragma unroll 8
        for (int t = wave; t < T; t += 4) s += *reinterpret_cast<const f32x4*>(x + base + (long)(t + 1) * C);
    red[wave][lane] = s;
    __syncthreads();
    f32x4 mean = {0.f, 0.f, 0.f, 0.f};
    if (T > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mean[j] = ((red[0][lane][j] + red[1][lane][j]) + (red[2][lane][j] + red[3][lane][j])) / (float)T;
    }
    if (ok)
#pragma unroll 4
        for (int t = wave; t < n; t += 4) *reinterpret_cast<f32x4*>(out + base + (long)t * C) = mean;
}

// ---------------------------------------------------------------------------------------------------------
// softmax + threshold selection over the non-CLS rows of every segment.  One workgroup per image.
// softmax: exp(s - max) * (1 / sum) with the thread mapping and combine order of softmax_rows_kernel; selection: the stable ascending
// rank, the SEQUENTIAL fp32 running sum in sorted order and the compare of select_threshold_kernel.
// keep [total]: 1 at the CLS row, 0/1 elsewhere; counts[b]: kept non-CLS rows; probs [total] (optional): the keep probabilities, 0 at
// the CLS row; dense_mask [B, N]: 1 at row_src[r] - 1 of every kept non-CLS row r, 0 elsewhere - built in LDS and written once in full.
// LDS: [N] probabilities -> dense flags, [N] sorted values -> running sums, [N] ranks.  A segment never has more than N non-CLS rows.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ragged_select_threshold_kernel(const float* __restrict__ scores, const int* __restrict__ cu,
                                                                      const int* __restrict__ row_src, float threshold, int N,
                                                                      float* __restrict__ probs, float* __restrict__ keep,
                                                                      int* __restrict__ counts, float* __restrict__ dense_mask) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* ps = sh;
    float* srt = sh + N;
    int* rank = reinterpret_cast<int*>(sh + 2 * N);
    int* flag = reinterpret_cast<int*>(sh);          // reuses ps once the probabilities are no longer read
    __shared__ float red[4];
    __shared__ float bc;
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = cu[b];
    int T = cu[b + 1] - r0 - 1;
    T = T < 0 ? 0 : (T > N ? N : T);                 // never past the LDS arrays
    const float* sr = scores + r0 + 1;
    // ---- softmax over the T non-CLS scores
    float m = -INFINITY;
    for (int t = tid; t < T; t += 256) m = fmaxf(m, sr[t]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) bc = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    m = bc;
    float sum = 0.f;
    for (int t = tid; t < T; t += 256) {
        const float e = expf(sr[t] - m);
        ps[t] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) bc = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    __syncthreads();
    const float inv = bc;
    for (int t = tid; t < T; t += 256) ps[t] = ps[t] * inv;
    __syncthreads();
    // ---- stable ascending rank, sequential running sum
    for (int i = tid; i < T; i += 256) {
        const float v = ps[i];
        int cnt = 0;
        for (int j = 0; j < T; ++j) {
            const float u = ps[j];
            cnt += (u < v) || (u == v && j < i);
        }
        rank[i] = cnt;
        srt[cnt] = v;
        if (probs) probs[r0 + 1 + i] = v;
    }
    __syncthreads();
    if (tid == 0) {
        float run = 0.f;
        for (int r = 0; r < T; ++r) {
            run += srt[r];
            srt[r] = run;
        }
    }
    for (int t = tid; t < N; t += 256) flag[t] = 0;  // ps is dead from here on
    __syncthreads();
    int kept = 0;
    for (int i = tid; i < T; i += 256) {
        const int f = srt[rank[i]] > threshold;
        keep[r0 + 1 + i] = f ? 1.f : 0.f;
        if (f) {
            const int id = row_src[r0 + 1 + i] - 1;
            if (id >= 0 && id < N) flag[id] = 1;
        }
        kept += f;
    }
    if (tid == 0) {
        keep[r0] = 1.f;                              // the CLS token is always kept
        if (probs) probs[r0] = 0.f;
    }
    kept = wave_sum_i(kept);
    if (lane == 0) wave_tot[wave] = kept;
    __syncthreads();
    if (tid == 0) counts[b] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    for (int t = tid; t < N; t += 256) dense_mask[(long)b * N + t] = flag[t] ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------------------
// re-pack: segment b of the old packed batch contributes its CLS row and the rows whose keep flag is non-zero, in order, to
// out[cu_new[b] .. cu_new[b+1]).  One workgroup per image, 256 old rows at a time: positions from ballot prefix sums (no atomics),
// then one wave per output row copies it with 16-byte accesses.  row_src_new carries row_src_old (the ORIGINAL token index) along.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ragged_repack_kernel(const float* __restrict__ x, const float* __restrict__ keep,
                                                            const int* __restrict__ cu_old, const int* __restrict__ cu_new,
                                                            const int* __restrict__ row_src_old, float* __restrict__ out,
                                                            int* __restrict__ row_src_new, int D) {
    __shared__ int src[256];           // old row (relative to the segment) of the rows this chunk keeps, in order
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = cu_old[b], n = cu_old[b + 1] - r0;
    const int o0 = cu_new[b], cnt = cu_new[b + 1] - o0;     // == the number of kept rows when cu_new was built from these flags
    const int nv = D >> 2;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        const int f = (i < n) ? (i == 0 || keep[r0 + i] != 0.f) : 0;
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_tot[w];
        if (f) src[woff + before] = i;
        const int here = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
        for (int j = wave; j < here && base + j < cnt; j += 4) {
            const int s = src[j];
            const f32x4* s4 = reinterpret_cast<const f32x4*>(x + (long)(r0 + s) * D);
            f32x4* d4 = reinterpret_cast<f32x4*>(out + (long)(o0 + base + j) * D);
            for (int c = lane; c < nv; c += 64) d4[c] = s4[c];
            if (lane == 0) row_src_new[o0 + base + j] = row_src_old[r0 + s];
        }
        base += here;
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// x [total, C], cu_seqlens [B+1] -> out [total, C]
int d2s_half_mean_concat_varlen(const float* x, const int* cu_seqlens, float* out, int B, int C, hipStream_t stream) {
    if (!x || !cu_seqlens || !out || B <= 0 || C <= 0 || (C & 1)) return D2S_ERR_ARG;
    const bool vec = (C % 8 == 0) && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec) {
        const int chunks = ((C >> 1) + 255) >> 8;
        hipLaunchKernelGGL(half_mean_concat_varlen_vec_kernel, dim3(2 * chunks, B), dim3(256), 0, stream, x, cu_seqlens, out, C);
        return d2s_check_launch();
    }
    const int chunks = ((C >> 1) + 63) >> 6;
    hipLaunchKernelGGL(half_mean_concat_varlen_kernel, dim3(2 * chunks, B), dim3(256), 0, stream, x, cu_seqlens, out, C);
    return d2s_check_launch();
}

// scores [total] (one per packed row; the CLS rows' entries are ignored), row_src [total] = original token index of every row
// (patch id + 1, 0 for CLS) -> probs [total] (may be null), keep [total], counts [B], dense_mask [B, N].  N <= 8192.
int d2s_ragged_select_threshold(const float* scores, const int* cu_seqlens, const int* row_src, float threshold, int N, float* probs,
                                float* keep, int* counts, float* dense_mask, int B, hipStream_t stream) {
    if (!scores || !cu_seqlens || !row_src || !keep || !counts || !dense_mask || B <= 0 || N <= 0 || N > 8192) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_select_threshold_kernel, dim3(B), dim3(256), (size_t)3 * N * sizeof(float), stream, scores, cu_seqlens,
                       row_src, threshold, N, probs, keep, counts, dense_mask);
    return d2s_check_launch();
}

// x [total, D], keep [total], cu_new from d2s_ragged_offsets(counts, B, 1) -> out [cu_new[B], D], row_src_new [cu_new[B]]
int d2s_ragged_repack(const float* x, const float* keep, const int* cu_old, const int* cu_new, const int* row_src_old, float* out,
                      int* row_src_new, int B, int D, hipStream_t stream) {
    if (!x || !keep || !cu_old || !cu_new || !row_src_old || !out || !row_src_new || B <= 0 || D <= 0 || (D & 3)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_repack_kernel, dim3(B), dim3(256), 0, stream, x, keep, cu_old, cu_new, row_src_old, out, row_src_new, D);
    return d2s_check_launch();
}

}  // extern "C"
