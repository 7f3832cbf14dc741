// Training through a ragged packed batch (--method ats --ats-train; DESIGN.md section 24, "Training through the stages"): the two row
// moves a differentiable ragged trunk adds to the block sequence.  (Its attention backward is the VARLEN form of the two kernels in
// attention_f32.hip, d2s_attn_varlen_bwd_f32.)
//   ragged_repack_bwd_kernel   the backward of ragged_repack_kernel (ragged.hip): a kept row of the old packed batch takes the gradient
//                              of the row it became, a dropped row takes zeros
//   ragged_cls_scatter_kernel  the backward of the head's gather of the CLS rows (d2s_gather_rows_i32 with cu_seqlens as the index)
// Latency / HBM work, no atomics, no memset: every output row is written exactly once, 16 bytes per lane.
#include "d2s_common.h"
#include "d2s_hip_ragged_train.h"

namespace {

// One workgroup per image, 256 old rows at a time.  The kept rows' positions in the new segment come from the ballot prefix sums of
// ragged_repack_kernel (same flags, same order), then one wave per OLD row copies the matching new row or writes zeros.  A position
// at or past the new segment's length (cu_new not built from these flags) reads nothing and writes zeros.
__global__ __launch_bounds__(256) void ragged_repack_bwd_kernel(const float* __restrict__ g_new, const float* __restrict__ keep,
                                                                const int* __restrict__ cu_old, const int* __restrict__ cu_new,
                                                                float* __restrict__ g_old, int D) {
    __shared__ int pos[256];           // new row (relative to the new segment) of every old row of this chunk, -1: dropped
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = cu_old[b], n = cu_old[b + 1] - r0;
    const int o0 = cu_new[b], cnt = cu_new[b + 1] - o0;
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
        const int p = base + woff + before;
        pos[tid] = (f && p < cnt) ? p : -1;
        const int here = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
        const int rows = min(256, n - c0);
        for (int j = wave; j < rows; j += 4) {
            const int s = pos[j];
            f32x4* d4 = reinterpret_cast<f32x4*>(g_old + (long)(r0 + c0 + j) * D);
            if (s >= 0) {
                const f32x4* s4 = reinterpret_cast<const f32x4*>(g_new + (long)(o0 + s) * D);
                for (int c = lane; c < nv; c += 64) d4[c] = s4[c];
            } else {
                for (int c = lane; c < nv; c += 64) d4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        base += here;
        __syncthreads();
    }
}

// One workgroup per image: image b writes the rows from its CLS row up to the next image's (the first image from row 0, the last one up
// to `total`, both clamped to [0, total]), its CLS row from g_cls[b] and zeros elsewhere - together every row of g, once.
__global__ __launch_bounds__(256) void ragged_cls_scatter_kernel(const float* __restrict__ g_cls, const int* __restrict__ cu,
                                                                 float* __restrict__ g, int B, int total, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int c0 = min(max(cu[b], 0), total);
    const int r0 = b == 0 ? 0 : c0;
    const int r1 = b == B - 1 ? total : min(max(cu[b + 1], r0), total);
    const int nv = D >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(g_cls + (long)b * D);
    for (int r = r0 + wave; r < r1; r += 4) {
        f32x4* d4 = reinterpret_cast<f32x4*>(g + (long)r * D);
        if (r == c0) {
            for (int c = lane; c < nv; c += 64) d4[c] = s4[c];
        } else {
            for (int c = lane; c < nv; c += 64) d4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

}  // namespace

extern "C" {

// g_new [cu_new[B], D], keep [cu_old[B]], cu_old / cu_new as d2s_ragged_repack took them -> g_old [cu_old[B], D]
int d2s_ragged_repack_bwd(const float* g_new, const float* keep, const int* cu_old, const int* cu_new, float* g_old, int B, int D,
                          hipStream_t stream) {
    if (!g_new || !keep || !cu_old || !cu_new || !g_old || B <= 0 || D <= 0 || (D & 3)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_repack_bwd_kernel, dim3(B), dim3(256), 0, stream, g_new, keep, cu_old, cu_new, g_old, D);
    return d2s_check_launch();
}

// g_cls [B, D], cu_seqlens [B+1] -> g [total, D]
int d2s_ragged_cls_scatter(const float* g_cls, const int* cu_seqlens, float* g, int B, int total, int D, hipStream_t stream) {
    if (!g_cls || !cu_seqlens || !g || B <= 0 || total <= 0 || D <= 0 || (D & 3)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_cls_scatter_kernel, dim3(B), dim3(256), 0, stream, g_cls, cu_seqlens, g, B, total, D);
    return d2s_check_launch();
}

}  // extern "C"
