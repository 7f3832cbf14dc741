// Training ATS and A-ViT in the bf16 arithmetic mode (train_bf16=True / --ats-train-bf16, --avit-bf16; DESIGN.md sections 24 and 25): the
// two backward row moves at the points where rows leave the ragged packed batch.  Both produce the gradient of the rows that ENTERED, in
// fp32 and - the same values rounded once, to nearest even - in bf16, which the gradient GEMMs of the bf16 data path read.
//   ragged_repack_bwd_bf16out_kernel      d2s_ragged_repack_bwd (ragged_train.hip) with the bf16 form stored in the same pass
//   avit_halt_repack_bwd_bf16out_kernel   the whole backward of an A-ViT block boundary: d2s_ragged_repack_bwd, then d2s_avit_halt_bwd
//                                         (avit.hip), then the cast - one launch, every row read once and written once in each form
// Geometry of both: image x row-chunk slot.  The plain kernels run one workgroup per image (128 workgroups for 25 000 rows at the benchmark
// batch, half the CUs idle); here workgroup (b, s) owns the 64-row chunks s, s + SLOTS, ... of image b and recounts the kept rows in front
// of each of them from `keep` (4 bytes per row against D * 6 bytes moved per row), so no workgroup waits for another and a DeiT image
// (197 rows) is spread over 4 workgroups.  A slot without a chunk ends at once.
// Latency / HBM work, no atomics, no memset: every output element is written exactly once, 16 bytes (fp32) and 8 bytes (bf16) per lane.
#include "d2s_common.h"
#include "d2s_hip_ragged_stage_bf16.h"

namespace {

constexpr int CHUNK = 64;   // rows per chunk: one ballot of wave 0 places them
constexpr int SLOTS = 8;    // gridDim.y

typedef __bf16 bf16x4s __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_both(float* __restrict__ o, __bf16* __restrict__ o16, long row, int D, int c, f32x4 v) {
    reinterpret_cast<f32x4*>(o + row * D)[c] = v;
    bf16x4s hv;
#pragma unroll
    for (int j = 0; j < 4; ++j) hv[j] = (__bf16)v[j];
    reinterpret_cast<bf16x4s*>(o16 + row * D)[c] = hv;
}

// The kept flag of old row i of an image, as ragged_repack_kernel reads it: the CLS row is always kept.
__device__ __forceinline__ int kept_flag(const float* __restrict__ keep, int r0, int i) { return i == 0 || keep[r0 + i] != 0.f; }

// The new position (relative to the new segment) of the CHUNK old rows from c0 on, -1 for a dropped row or a position at or past cnt.
// `base` holds the kept rows in front of old row `counted` and is moved up to the end of this chunk.  Called by all 256 threads.
__device__ __forceinline__ void place_chunk(const float* __restrict__ keep, int r0, int n, int cnt, int c0, int& counted, int& base,
                                            int* pos, int* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int part = 0;
    for (int i = counted + tid; i < c0; i += 256) part += kept_flag(keep, r0, i);
    part = wave_sum_i(part);
    if (lane == 0) wtot[wave] = part;
    __syncthreads();
    base += (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    if (wave == 0) {
        const int i = c0 + lane;
        const int f = i < n ? kept_flag(keep, r0, i) : 0;
        const unsigned long long bal = __ballot(f);
        const int p = base + __popcll(bal & ((1ull << lane) - 1ull));
        pos[lane] = (f && p < cnt) ? p : -1;
        if (lane == 0) wtot[4] = __popcll(bal);
    }
    __syncthreads();
    base += wtot[4];
    counted = min(c0 + CHUNK, n);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid (B, SLOTS).  Both segments are clamped to their buffers: the old one to [0, cu_old[B]], the new one to [0, cu_new[B]].
__global__ __launch_bounds__(256) void ragged_repack_bwd_bf16out_kernel(const float* __restrict__ g_new, const float* __restrict__ keep,
                                                                        const int* __restrict__ cu_old, const int* __restrict__ cu_new,
                                                                        float* __restrict__ g_old, __bf16* __restrict__ g_old16, int B,
                                                                        int D) {
    __shared__ int pos[CHUNK];
    __shared__ int wtot[5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int tot_old = max(cu_old[B], 0), tot_new = max(cu_new[B], 0);
    const int r0 = clampi(cu_old[b], 0, tot_old), n = clampi(cu_old[b + 1], r0, tot_old) - r0;
    const int o0 = clampi(cu_new[b], 0, tot_new), cnt = clampi(cu_new[b + 1], o0, tot_new) - o0;
    const int nv = D >> 2;
    int counted = 0, base = 0;
    for (int c0 = blockIdx.y * CHUNK; c0 < n; c0 += SLOTS * CHUNK) {
        place_chunk(keep, r0, n, cnt, c0, counted, base, pos, wtot);
        const int rows = min(CHUNK, n - c0);
        for (int j = wave; j < rows; j += 4) {
            const int s = pos[j];
            const long row = (long)(r0 + c0 + j);
            if (s >= 0) {
                const f32x4* s4 = reinterpret_cast<const f32x4*>(g_new + (long)(o0 + s) * D);
                for (int c = lane; c < nv; c += 64) store_both(g_old, g_old16, row, D, c, s4[c]);
            } else {
                for (int c = lane; c < nv; c += 64) store_both(g_old, g_old16, row, D, c, f32x4{0.f, 0.f, 0.f, 0.f});
            }
        }
        __syncthreads();
    }
}

// grid (B, SLOTS).  Image b owns rows [r0, r0 + n) of the batch that entered the halting step, clamped to [0, total) as in
// avit_halt_bwd_kernel; what arrived (g_new, null: nothing - the last layer) sits on the rows its re-pack kept.  Per element the
// expressions are avit_halt_bwd_kernel's, in its order, on the value ragged_repack_bwd_kernel would have stored:
//   a finished image (halt_layer[b, 0] < layer): what arrived, or zeros
//   row i >= 1 of a live image: what arrived (or zeros), column 0 plus the halting score's term
//   its CLS row: what arrived (or zeros) plus w[b] * dacc[b], column 0 plus the CLS score's term
// The two dot products of the CLS term are summed by the workgroup that owns chunk 0, in avit_halt_bwd_kernel's order.
__global__ __launch_bounds__(256) void avit_halt_repack_bwd_bf16out_kernel(
    const float* __restrict__ g_new, const float* __restrict__ keep, const int* __restrict__ cu_new, const float* __restrict__ h,
    const int* __restrict__ cu, const int* __restrict__ row_src, const int* __restrict__ nh, const float* __restrict__ w,
    const float* __restrict__ dacc, const float* __restrict__ ycls, const float* __restrict__ ysave, const float* __restrict__ gsc,
    float* __restrict__ g, __bf16* __restrict__ g16, int B, int N, int D, int total, int layer, int L, float gamma) {
    __shared__ int pos[CHUNK];
    __shared__ int wtot[5];
    __shared__ float redf[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int fresh = g_new == nullptr;
    const int r0 = min(max(cu[b], 0), total);
    const int n = min(max(cu[b + 1], r0), total) - r0;
    int o0 = 0, cnt = 0;
    if (!fresh) {
        const int tot_new = max(cu_new[B], 0);
        o0 = clampi(cu_new[b], 0, tot_new);
        cnt = clampi(cu_new[b + 1], o0, tot_new) - o0;
    }
    const long s0 = (long)b * N;
    const long d0 = (long)b * D;
    const int nv = D >> 2;
    const int n0 = n > 0 ? nh[s0] : 0;
    const bool dead = n0 < layer;                    // finished in an earlier layer: a dead row, nothing of the loss depends on it
    const float gbar = gsc[layer - 1], gp = gsc[L];
    int counted = 0, base = 0;
    for (int c0 = blockIdx.y * CHUNK; c0 < n; c0 += SLOTS * CHUNK) {
        if (!fresh) {
            place_chunk(keep, r0, n, cnt, c0, counted, base, pos, wtot);
        }
        float add0 = 0.f, wv = 0.f;
        if (c0 == 0 && !dead) {                      // uniform over the workgroup
            float a = 0.f, e = 0.f;
            for (int col = tid; col < D; col += 256) {
                const float da = dacc[d0 + col];
                a += da * ycls[d0 + col];
                e += da * ysave[d0 + col];
            }
            a = wave_sum(a);
            e = wave_sum(e);
            if (lane == 0) {
                redf[0][wave] = a;
                redf[1][wave] = e;
            }
            __syncthreads();
            const float s_l = (redf[0][0] + redf[0][1]) + (redf[0][2] + redf[0][3]);
            const float s_n = (redf[1][0] + redf[1][1]) + (redf[1][2] + redf[1][3]);
            const float gh0 = (n0 > layer ? (s_l - s_n) - gp : 0.f) + gbar;
            const float h0 = h[r0];
            add0 = gh0 * gamma * (h0 * (1.0f - h0));
            wv = w[b];
        }
        const int rows = min(CHUNK, n - c0);
        for (int j = wave; j < rows; j += 4) {
            const int i = c0 + j;
            const long r = (long)r0 + i;
            const int s = fresh ? -1 : pos[j];
            const f32x4* s4 = reinterpret_cast<const f32x4*>(g_new + (long)(o0 + max(s, 0)) * D);
            float add = 0.f;
            if (!dead && i > 0) {
                const int t = row_src[r];
                if (t > 0 && t < N) {
                    const float gh = (nh[s0 + t] > layer ? -gp : 0.f) + gbar;
                    const float hv = h[r];
                    add = gh * gamma * (hv * (1.0f - hv));
                }
            }
            for (int c = lane; c < nv; c += 64) {
                f32x4 v = s >= 0 ? s4[c] : f32x4{0.f, 0.f, 0.f, 0.f};
                if (!dead) {
                    if (i > 0) {
                        if (c == 0) v[0] = v[0] + add;
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float u = v[q] + wv * dacc[d0 + 4 * c + q];
                            if (c == 0 && q == 0) u += add0;
                            v[q] = u;
                        }
                    }
                }
                store_both(g, g16, r, D, c, v);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// d2s_ragged_repack_bwd that also writes the bf16 form of every row: g_new [cu_new[B], D], keep [cu_old[B]] -> g_old [cu_old[B], D] fp32,
// that entry's bits, and g_old_bf16 [cu_old[B], D], the same values rounded once.
int d2s_ragged_repack_bwd_bf16out(const float* g_new, const float* keep, const int* cu_old, const int* cu_new, float* g_old,
                                  void* g_old_bf16, int B, int D, hipStream_t stream) {
    if (!g_new || !keep || !cu_old || !cu_new || !g_old || !g_old_bf16 || B <= 0 || D <= 0 || (D & 3)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ragged_repack_bwd_bf16out_kernel, dim3(B, SLOTS), dim3(256), 0, stream, g_new, keep, cu_old, cu_new, g_old,
                       static_cast<__bf16*>(g_old_bf16), B, D);
    return d2s_check_launch();
}

// The backward of an A-ViT block boundary in one launch: d2s_ragged_repack_bwd (g_new, keep, cu_new: all three or none - none is the
// last layer, d2s_avit_halt_bwd's fresh = 1), then d2s_avit_halt_bwd, written in fp32 (g_old, those entries' bits) and in bf16.
int d2s_avit_halt_repack_bwd_bf16out(const float* g_new, const float* keep, const int* cu_new, const float* h, const int* cu_seqlens,
                                     const int* row_src, const int* halt_layer, const float* w, const float* dacc, const float* ycls,
                                     const float* ysave, const float* gsc, float* g_old, void* g_old_bf16, int B, int N, int D, int total,
                                     int layer, int L, float gamma, hipStream_t stream) {
    if (!h || !cu_seqlens || !row_src || !halt_layer || !w || !dacc || !ycls || !ysave || !gsc || !g_old || !g_old_bf16) return D2S_ERR_ARG;
    if ((g_new != nullptr) != (keep != nullptr) || (g_new != nullptr) != (cu_new != nullptr)) return D2S_ERR_ARG;
    if (B <= 0 || N <= 0 || D <= 0 || (D & 3) || total <= 0 || layer < 1 || L < layer || L > 64) return D2S_ERR_ARG;
    hipLaunchKernelGGL(avit_halt_repack_bwd_bf16out_kernel, dim3(B, SLOTS), dim3(256), 0, stream, g_new, keep, cu_new, h, cu_seqlens,
                       row_src, halt_layer, w, dacc, ycls, ysave, gsc, g_old, static_cast<__bf16*>(g_old_bf16), B, N, D, total, layer, L,
                       gamma);
    return d2s_check_launch();
}

}  // extern "C"
