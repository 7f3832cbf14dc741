// Token selection by the student's own CLS attention (attn_selection; DESIGN.md section 21 - the build's own definition, the reference
// names the branch at vit_models/dynamic_vit.py:265 and never connects it).  One launch per pruning stage replaces the score predictor,
// the softmax over its scores and the hard top-k:
//
//   w[b,t]     = max_h  cls_row[b,h,lead+t]                  (reduce 0, the teacher target's rule, losses.py:76-79)
//              = (sum_h cls_row[b,h,lead+t]) / H             (reduce 1, mean_heads; h ascending)
//   probs[b,t] = w[b,t] / sum_t w[b,t]
//   kept / dropped = the hard top-k of probs as d2s_select_topk orders it (value descending, equal values lowest index first, both
//                    lists ascending) - ranked on the emitted fp32 probs, so d2s_select_topk(probs, k) gives the same ids bit for bit.
//
// One workgroup per image: the head reduction reads H rows with loads coalesced along t, the row sum is a wave butterfly then
// (r0 + r1) + (r2 + r3) (teacher_target_kernel's order), ranking is by counting over the probabilities staged in LDS, compaction by wave
// ballots.  No atomics, no memset, no scratch, nothing read back by the host: deterministic and legal inside a captured step.
#include "d2s_common.h"

namespace {

__global__ __launch_bounds__(256) void select_cls_attn_kernel(const float* __restrict__ cls_row, int H, int n, int lead, int T, int k,
                                                              int reduce, float* __restrict__ probs, long long* __restrict__ kept,
                                                              long long* __restrict__ dropped) {
    extern __shared__ __attribute__((aligned(16))) float sh[];  // [T] w, then probs; [T] keep flags (as int)
    float* ps = sh;
    int* flag = reinterpret_cast<int*>(sh + T);
    __shared__ float red[4];
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* ab = cls_row + (long)blockIdx.x * H * n + lead;
    float part = 0.f;
    for (int t = tid; t < T; t += 256) {
        float w;
        if (reduce) {
            float s = 0.f;
            for (int h = 0; h < H; ++h) s += ab[(long)h * n + t];
            w = s / (float)H;
        } else {
            w = -INFINITY;
            for (int h = 0; h < H; ++h) w = fmaxf(w, ab[(long)h * n + t]);
        }
        ps[t] = w;
        part += w;
    }
    part = wave_sum(part);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    float* pr = probs + (long)blockIdx.x * T;
    for (int t = tid; t < T; t += 256) {       // a thread renormalises the entries it wrote itself
        const float p = ps[t] / tot;
        ps[t] = p;
        pr[t] = p;
    }
    if (k == 0 && !dropped) return;            // uniform: probabilities only
    __syncthreads();
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
    long long* ko = kept + (long)blockIdx.x * k;
    long long* dr = dropped ? dropped + (long)blockIdx.x * (T - k) : nullptr;
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
            else if (dr && i - pos < T - k) dr[i - pos] = i;
        }
        base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// cls_row [B,H,n] fp32 (the attention forward's CLS softmax row); token t of image b is column lead + t, 0 <= t < T, lead + T <= n.
// reduce: 0 max over heads, 1 mean.  -> probs [B,T] (always written), kept [B,k] / dropped [B,T-k] int64 ascending (dropped may be null).
int d2s_select_cls_attn(const float* cls_row, int B, int H, int n, int lead, int T, int k, int reduce, float* probs, long long* kept,
                        long long* dropped, hipStream_t stream) {
    if (!cls_row || !probs || (!kept && k > 0) || B <= 0 || H <= 0 || n <= 0 || lead < 0 || T <= 0 || T > 16384 ||
        (long)lead + T > n || k < 0 || k > T || (reduce != 0 && reduce != 1))
        return D2S_ERR_ARG;
    // 2 T floats of dynamic LDS: 128 KiB at T = 16384, above the runtime's default per-kernel limit; the CU has 160 KiB
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&select_cls_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  2 * 16384 * (int)sizeof(float));
        attr_set = true;
    }
    hipLaunchKernelGGL(select_cls_attn_kernel, dim3(B), dim3(256), (size_t)2 * T * sizeof(float), stream, cls_row, H, n, lead, T, k,
                       reduce, probs, kept, (T - k) > 0 ? dropped : nullptr);
    return d2s_check_launch();
}

}  // extern "C"
