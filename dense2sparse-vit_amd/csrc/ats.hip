// Adaptive Token Sampling at inference (ATS, Fayyaz et al. 2022; DESIGN.md section 24 - the build's own definition, the reference has
// no ATS): a stage inside a block, between the attention half and the MLP half, that keeps a different number of tokens for every image.
// It acts on a ragged packed batch (image b owns rows cu[b] .. cu[b+1]-1, row cu[b] is its CLS token) and reads what the block already
// made: the CLS softmax row of the varlen attention, [H, total], and the block's own qkv, fp32 or bf16.
//
//   score      a_j = sum_h A[h, CLS, j];  v_j = ||V_j||_2 over the H * 64 concatenated head values;  w_j = a_j v_j, tot = sum_j w_j,
//              s_j = w_j / tot;  tot not > 0 or not finite: s_j = 1 / T for every j
//   selection  (on the emitted fp32 scores)  stable ascending rank (equal values lowest index first); c_i = the running sum in that
//              order, summed SEQUENTIALLY in fp32 (select_threshold_kernel's reason: the order decides a token whose running sum lands
//              within rounding of a threshold);  for k = 0 .. K-1: u_k = (float)(2k+1) / (float)(2K) correctly rounded, t_k = u_k *
//              c_{T-1}, i_k = the first position with c_i >= t_k;  kept = the SET of picked tokens (1 .. min(K, T) of them) and CLS
//
// One workgroup per image.  No atomics, no memset, no scratch, nothing read back by the host; every output element is written exactly
// once, so results are bit-identical run to run.  A bf16 qkv is widened to fp32 at the load (exact) and every lane sums the same eight
// columns in the same order for either element type: d2s_ats_select on a bf16 qkv is d2s_ats_select on its fp32 copy bit for bit.
#include "d2s_common.h"
#include "d2s_hip_ats.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int DH = 64;
constexpr int NT = 1024;              // threads of the workgroup: 16 waves share the row norms of one image
constexpr int NW = NT / 64;
constexpr int RB = 4;                 // rows a wave has in flight (8 spill: 1024 threads leave a lane 128 registers)
constexpr int ATS_MAX_N = 2049;       // rows of one image, CLS included
constexpr int ATS_MAX_PATCHES = 8192; // N of dense_mask (d2s_ragged_select_threshold's limit)
constexpr int ATS_MAX_K = 1 << 22;    // 2K + 1 stays an exact fp32 integer
// dynamic LDS: (max(max_n - 1, N) + 3 (max_n - 1)) floats, at the limits 32 KiB + 24 KiB = 56 KiB: under the 64 KiB a kernel gets unasked

// eight consecutive V values of one row, widened to fp32
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
    } else {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void ats_select_kernel(const float* __restrict__ cls_row, const T* __restrict__ qkv,
                                                        const int* __restrict__ cu, const int* __restrict__ row_src, int K, int N, int H,
                                                        int total, int M, int L, float* __restrict__ score, float* __restrict__ keep,
                                                        int* __restrict__ counts, float* __restrict__ dense_mask) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* ps = sh;                                          // [L] w_j -> s_j; dead after the ranks, then the dense flags
    float* srt = sh + L;                                     // [M] sorted scores -> running sums
    int* rank = reinterpret_cast<int*>(sh + L + M);          // [M]
    int* sel = rank + M;                                     // [M] 1 at every picked position of the sorted order
    int* flag = reinterpret_cast<int*>(sh);                  // [N] dense_mask of this image
    __shared__ float red[NW];
    __shared__ float bc;
    __shared__ int wave_tot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = cu[b];
    const int rows = cu[b + 1] - r0;
    const bool sane = r0 >= 0 && r0 < total && rows > 0;     // offsets that are no offsets: the image writes its count and mask row only
    int Tn = sane ? rows - 1 : 0;
    Tn = min(Tn, min(M, total - r0 - 1));                    // never past the LDS arrays or the packed batch
    Tn = max(Tn, 0);
    const int HD = H * DH;
    const long ld = 3L * HD;
    // ---- w_j = a_j * ||V_j||: one wave per row, a lane owns eight consecutive columns of every 512.  A wave takes RB rows at a time and
    // issues all their loads before the first sum, so it waits for HBM once per RB rows (a row past the end repeats the last one, unused)
    for (int j0 = wave * RB; j0 < Tn; j0 += NW * RB) {
        long r[RB];
        float ss[RB], a[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            r[q] = (long)r0 + 1 + min(j0 + q, Tn - 1);
            ss[q] = 0.f;
            a[q] = 0.f;
        }
        for (int c = lane * 8; c < HD; c += 512) {
            float v[RB][8];
#pragma unroll
            for (int q = 0; q < RB; ++q) load8(qkv + r[q] * ld + 2L * HD + c, v[q]);
#pragma unroll
            for (int q = 0; q < RB; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) ss[q] = fmaf(v[q][e], v[q][e], ss[q]);
        }
        for (int h = lane; h < H; h += 64) {
            float u[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) u[q] = cls_row[(long)h * total + r[q]];
#pragma unroll
            for (int q = 0; q < RB; ++q) a[q] += u[q];
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {                       // independent butterflies: their latencies overlap
            ss[q] = wave_sum(ss[q]);
            a[q] = wave_sum(a[q]);
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < RB; ++q)
                if (j0 + q < Tn) ps[j0 + q] = a[q] * sqrtf(ss[q]);
        }
    }
    __syncthreads();
    // ---- tot and the scores
    float s = 0.f;
    for (int j = tid; j < Tn; j += NT) s += ps[j];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += red[w];
        bc = tot;
    }
    __syncthreads();
    const float tot = bc;
    const bool ok = tot > 0.f && tot < INFINITY;             // false for a NaN as well
    const float uni = 1.0f / (float)max(Tn, 1);
    for (int j = tid; j < Tn; j += NT) ps[j] = ok ? __fdiv_rn(ps[j], tot) : uni;
    __syncthreads();
    // ---- stable ascending rank by counting
    for (int i = tid; i < Tn; i += NT) {
        const float v = ps[i];
        int cnt = 0;
        for (int j = 0; j < Tn; ++j) {                       // every lane reads the same address: an LDS broadcast (16-byte reads measured slower)
            const float u = ps[j];
            cnt += (u < v) || (u == v && j < i);
        }
        cnt = min(cnt, Tn - 1);                              // a NaN cannot reach here; the clamp keeps the LDS write in bounds regardless
        rank[i] = cnt;
        srt[cnt] = v;
        sel[i] = 0;
        score[r0 + 1 + i] = v;
    }
    __syncthreads();
    // ---- the running sum, sequentially, by one lane; the others clear the dense flags meanwhile (ps is dead)
    if (tid == 0) {                                          // eight independent LDS reads at a time, then the adds in order
        float run = 0.f;
        int r = 0;
        for (; r + 8 <= Tn; r += 8) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = srt[r + e];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                run += v[e];
                srt[r + e] = run;
            }
        }
        for (; r < Tn; ++r) {
            run += srt[r];
            srt[r] = run;
        }
    }
    if (dense_mask)
        for (int t = tid; t < N; t += NT) flag[t] = 0;
    __syncthreads();
    // ---- the K searches, in parallel: the first position whose running sum reaches t_k (the sums never decrease: the scores are >= 0)
    if (Tn > 0) {
        const float last = srt[Tn - 1];
        const float den = (float)(2 * K);
        for (int k = tid; k < K; k += NT) {
            const float t = __fdiv_rn((float)(2 * k + 1), den) * last;
            int lo = 0, hi = Tn - 1;                         // the last position always qualifies
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (srt[mid] >= t) hi = mid; else lo = mid + 1;
            }
            sel[lo] = 1;                                     // several k may pick one position: they all write the same value
        }
    }
    __syncthreads();
    // ---- flags in token order, counted by ballots
    int kept = 0;
    for (int c0 = 0; c0 < Tn; c0 += NT) {
        const int i = c0 + tid;
        const int f = (i < Tn) ? sel[rank[i]] : 0;
        if (i < Tn) {
            keep[r0 + 1 + i] = f ? 1.f : 0.f;
            if (f && dense_mask) {
                const int id = row_src[r0 + 1 + i] - 1;
                if (id >= 0 && id < N) flag[id] = 1;
            }
        }
        kept += __popcll(__ballot(f));
    }
    if (lane == 0) wave_tot[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) c += wave_tot[w];
        counts[b] = c;
        if (sane) {
            keep[r0] = 1.f;                                  // the CLS token is always kept
            score[r0] = 0.f;
        }
    }
    if (dense_mask)
        for (int t = tid; t < N; t += NT) dense_mask[(long)b * N + t] = flag[t] ? 1.f : 0.f;
}

template <typename T>
int launch(const float* cls_row, const T* qkv, const int* cu, const int* row_src, int K, int N, int B, int H, int total, int max_n,
           float* score, float* keep, int* counts, float* dense_mask, hipStream_t stream) {
    const int M = max_n - 1;
    const int L = (dense_mask && N > M) ? N : M;
    hipLaunchKernelGGL(ats_select_kernel<T>, dim3(B), dim3(NT), ((size_t)L + 3 * (size_t)M) * sizeof(float), stream, cls_row, qkv, cu, row_src,
                       K, N, H, total, M, L, score, keep, counts, dense_mask);
    return d2s_check_launch();
}

}  // namespace

extern "C" {

int d2s_ats_select(const float* cls_row, const void* qkv, int qkv_is_bf16, const int* cu_seqlens, const int* row_src, int K, int N, int B,
                   int H, int total, int max_n, float* score, float* keep, int* counts, float* dense_mask, hipStream_t stream) {
    if (!cls_row || !qkv || !cu_seqlens || !row_src || !score || !keep || !counts || B <= 0 || H <= 0 || K <= 0 || K > ATS_MAX_K ||
        total <= 0 || max_n < 1 || max_n > ATS_MAX_N || (dense_mask && (N <= 0 || N > ATS_MAX_PATCHES)))
        return D2S_ERR_ARG;
    if (qkv_is_bf16)
        return launch(cls_row, static_cast<const __bf16*>(qkv), cu_seqlens, row_src, K, N, B, H, total, max_n, score, keep, counts, dense_mask,
                      stream);
    return launch(cls_row, static_cast<const float*>(qkv), cu_seqlens, row_src, K, N, B, H, total, max_n, score, keep, counts, dense_mask,
                  stream);
}

}  // extern "C"
