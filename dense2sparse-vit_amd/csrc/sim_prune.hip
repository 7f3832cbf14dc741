// Similarity stage after attention ranking (--sim-prune R; DESIGN.md section 30 - the build's own definition, Zero-TPrune's similarity
// stage restated for this selector): an attention-selecting stage first takes c = k + r candidates by importance (d2s_select_cls_attn,
// unchanged) and then prunes the r candidates that resemble a MORE important candidate most, so the k survivors are not near-duplicates.
//
//   metric     m_t = (sum_h K[b,t,h,:]) / H  (h ascending), divided by its L2 norm - tome.hip's metric with tome.hip's rule for a zero
//              row: 0/0 = NaN, every comparison with its scores is false, so it is never a partner and as a source its best is -inf
//   partition  the candidates ordered by probs descending, equal values lowest id first: the c_b = c - c/2 most important are group B,
//              the c_a = c/2 least important group A; both kept as lists in ascending token id
//   match      score[a][b] = sum_d m_a[d] m_b[d] on the fp32 matrix pipe (32 x 32 tiles over D = 64, one summation order for every pair);
//              best[a] = max_b score, partner[a] = the lowest token id attaining it (the lowest id of B where no comparison succeeded)
//   prune      the r members of A with the largest best, d2s_select_topk's rule (value descending, equal values lowest id first)
//   lists      kept [B, c - r] = the candidates without the pruned ones, dropped [B, T - c + r] = every other token, both int64 ascending;
//              pruned / partner / sim [B, r] in ascending pruned id
//
// Two launches per call, no host synchronisation between them:
//   match   grid (32-row tile of A, image): every workgroup redoes the partition of its image (counting over the candidates'
//           probabilities staged in LDS, compaction by wave ballots - a few microseconds, cheaper than a third launch), then a wave owns
//           32-column tiles of B; the running best stays in registers (squeeze_match_kernel's scheme).  (best, partner) of the c_a rows go
//           to the head of the image's kept list, which has room for them (8 c_a <= 8 (c - r) bytes because r <= c/2) and is only
//           written for good by the launch after.
//   select  one workgroup per image: the same partition, (best, partner) read back into LDS BEFORE anything is written, ranking by
//           counting, every list compacted by wave ballots.
// No atomics, no memset, no scratch, nothing read back by the host: deterministic and legal inside a captured step.
#include "d2s_common.h"
#include "d2s_hip_sim_prune.h"
#include <limits.h>

namespace {

constexpr int SP_DH = 64;         // width of the metric: the head dimension
constexpr int SP_MAXT = 1024;     // longest scored sequence: static LDS below
constexpr int SP_TILE = 32;       // A rows per workgroup and B rows per wave step of the match (one 32x32x2 MFMA tile)

// ---------------------------------------------------------------------------------------------------------
// metric.  16 lanes per token row, lane e holding columns 4 e .. 4 e + 3: every head's K row is read as one 256-byte line, 16 bytes per
// lane.  The squared norm is a 4-term fma chain per lane then a butterfly over the row's 16 lanes (commutative additions: all 16 lanes
// get the same bits), so equal K rows give equal metric bits wherever they sit.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_metric_kernel(const float* __restrict__ qkv, long rows, int H, float* __restrict__ metric) {
    const int e = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool ok = row < rows;
    const long ld = 3L * H * SP_DH;
    const f32x4* kp = reinterpret_cast<const f32x4*>(qkv + (ok ? row : 0) * ld + (long)H * SP_DH) + e;      // K of head 0
    f32x4 m = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; ++h) {
        const f32x4 v = kp[h * (SP_DH / 4)];
        m[0] += v[0]; m[1] += v[1]; m[2] += v[2]; m[3] += v[3];
    }
    const float fh = (float)H;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = m[j] / fh;
        ss = fmaf(m[j], m[j], ss);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float nrm = sqrtf(ss);
    if (ok) reinterpret_cast<f32x4*>(metric + row * SP_DH)[e] = f32x4{m[0] / nrm, m[1] / nrm, m[2] / nrm, m[3] / nrm};
}

// (s, j) beats (bs, bj): a larger score, or the same score at a lower position
__device__ __forceinline__ bool beats(float s, int j, float bs, int bj) { return s > bs || (s == bs && j < bj); }

// Block-wide stable compaction over i in [0, N): emit(i, f, pos) with f = flag(i) and pos = the number of set flags below i.
template <typename Flag, typename Emit>
__device__ __forceinline__ void block_compact(int N, int* wave_tot, Flag flag, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int i = c0 + tid;
        const int f = (i < N) ? flag(i) : 0;
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_tot[w];
        if (i < N) emit(i, f, base + woff + before);
        base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
}

struct Partition {
    float pc[SP_MAXT];       // probability of candidate j
    int cid[SP_MAXT];        // token id of candidate j, clamped into [0, T)
    int in_b[SP_MAXT];       // candidate j belongs to group B
    int a_pos[SP_MAXT / 2];  // candidate positions of group A, ascending
    int b_pos[SP_MAXT];      // candidate positions of group B, ascending
    int wave_tot[4];
};

// The importance-guided partition of one image, by the whole workgroup.  cand is trusted to be d2s_select_cls_attn's list (ascending
// ids, so a lower position is a lower id), but never to index outside the image.  Ends synchronised.
__device__ __forceinline__ void partition(Partition& s, const float* __restrict__ pr, const long long* __restrict__ cd, int T, int c) {
    const int tid = threadIdx.x, c_a = c >> 1, c_b = c - c_a;
    for (int j = tid; j < c; j += 256) {
        const long long id = cd[j];
        const int t = id < 0 ? 0 : (id >= T ? T - 1 : (int)id);
        s.cid[j] = t;
        s.pc[j] = pr[t];
    }
    __syncthreads();
    for (int j = tid; j < c; j += 256) {
        const float v = s.pc[j];
        int cnt = 0;
        for (int i = 0; i < c; ++i) {
            const float u = s.pc[i];
            cnt += (u > v) || (u == v && i < j);
        }
        s.in_b[j] = cnt < c_b;
    }
    __syncthreads();
    block_compact(c, s.wave_tot, [&](int j) { return s.in_b[j]; },
                  [&](int j, int f, int pos) {
                      if (f) { if (pos < c_b) s.b_pos[pos] = j; }
                      else if (j - pos < c_a) s.a_pos[j - pos] = j;
                  });
}

// ---------------------------------------------------------------------------------------------------------
// match.  Lane l of a wave holds row (l & 31) of the A tile and of the current B tile, columns 8 c + 4 (l >> 5) .. + 3 of chunk c: MFMA q
// of a chunk multiplies columns 8 c + q and 8 c + 4 + q, so every dot runs over the 64 columns in one fixed order whatever its position.
// A row past the end of a list reads scored token 0 instead (in bounds) and is masked out afterwards.  Each lane keeps the running best
// of its 16 accumulator rows over its column (ascending B tiles, strict >: the lowest position stays); one butterfly over the 32 columns
// and one LDS step over the 4 waves finish it.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim_match_kernel(const float* __restrict__ metric, const float* __restrict__ probs,
                                                        const long long* __restrict__ cand, int n, int lead, int T, int c, int r,
                                                        long long* __restrict__ kept) {
    __shared__ Partition s;
    __shared__ float wc[4][SP_TILE];
    __shared__ int wj[4][SP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * SP_TILE;
    const int c_a = c >> 1, c_b = c - c_a;
    partition(s, probs + (long)b * T, cand + (long)b * c, T, c);
    const float* mb = metric + ((long)b * n + lead) * SP_DH;      // metric row of scored token 0
    const bool aok = i0 + l31 < c_a;
    const f32x4* ap = reinterpret_cast<const f32x4*>(mb + (long)(aok ? s.cid[s.a_pos[i0 + l31]] : 0) * SP_DH) + half;
    f32x4 a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = ap[2 * q];
    float bestc[16];
    int bestj[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { bestc[q] = -INFINITY; bestj[q] = INT_MAX; }
    for (int j0 = wave * SP_TILE; j0 < c_b; j0 += 4 * SP_TILE) {
        const int j = j0 + l31;
        const bool bok = j < c_b;
        const f32x4* bp = reinterpret_cast<const f32x4*>(mb + (long)(bok ? s.cid[s.b_pos[j]] : 0) * SP_DH) + half;
        f32x4 bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) bv[q] = bp[2 * q];
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma32(a[q][u], bv[q][u], acc);
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (bok && acc[q] > bestc[q]) { bestc[q] = acc[q]; bestj[q] = j; }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float oc = __shfl_xor(bestc[q], o, 64);
            const int oj = __shfl_xor(bestj[q], o, 64);
            if (beats(oc, oj, bestc[q], bestj[q])) { bestc[q] = oc; bestj[q] = oj; }
        }
        if (l31 == 0) { wc[wave][mfma32_row(q, half)] = bestc[q]; wj[wave][mfma32_row(q, half)] = bestj[q]; }
    }
    __syncthreads();
    if (tid < SP_TILE && i0 + tid < c_a) {
        float v = wc[0][tid];
        int j = wj[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (beats(wc[w][tid], wj[w][tid], v, j)) { v = wc[w][tid]; j = wj[w][tid]; }
        if (j == INT_MAX) j = 0;      // no comparison succeeded (a NaN row): best stays -inf, the partner is B's lowest id
        // the image's kept list as the call's workspace: c_a floats, then c_a ints
        float* wbest = reinterpret_cast<float*>(kept + (long)b * (c - r));
        int* wpart = reinterpret_cast<int*>(wbest + c_a);
        wbest[i0 + tid] = v;
        wpart[i0 + tid] = s.cid[s.b_pos[j]];
    }
}

// ---------------------------------------------------------------------------------------------------------
// select.  One workgroup per image; with r == 0 nothing was matched, kept is cand and dropped its complement.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim_select_kernel(const float* __restrict__ probs, const long long* __restrict__ cand, int T, int c,
                                                         int r, long long* __restrict__ kept, long long* __restrict__ dropped,
                                                         long long* __restrict__ pruned, long long* __restrict__ partner,
                                                         float* __restrict__ sim) {
    __shared__ Partition s;
    __shared__ float best[SP_MAXT / 2];
    __shared__ int part[SP_MAXT / 2];
    __shared__ int prune_a[SP_MAXT / 2];      // A row p is pruned
    __shared__ int gone[SP_MAXT];             // candidate j is pruned
    __shared__ int keep_t[SP_MAXT];           // token t is kept
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c_a = c >> 1, k = c - r, m = T - k;
    partition(s, probs + (long)b * T, cand + (long)b * c, T, c);
    long long* ko = kept + (long)b * k;
    if (r > 0) {
        const float* wbest = reinterpret_cast<const float*>(ko);
        const int* wpart = reinterpret_cast<const int*>(wbest + c_a);
        for (int p = tid; p < c_a; p += 256) { best[p] = wbest[p]; part[p] = wpart[p]; }
    }
    for (int j = tid; j < c; j += 256) gone[j] = 0;
    for (int t = tid; t < T; t += 256) keep_t[t] = 0;
    __syncthreads();      // the workspace is in LDS: kept may be written from here on
    if (r > 0) {
        for (int p = tid; p < c_a; p += 256) {
            const float v = best[p];
            int cnt = 0;
            for (int i = 0; i < c_a; ++i) {
                const float u = best[i];
                cnt += (u > v) || (u == v && i < p);
            }
            prune_a[p] = cnt < r;
            if (cnt < r) gone[s.a_pos[p]] = 1;
        }
        __syncthreads();
        long long* po = pruned + (long)b * r;
        long long* pa = partner + (long)b * r;
        float* so = sim + (long)b * r;
        block_compact(c_a, s.wave_tot, [&](int p) { return prune_a[p]; },
                      [&](int p, int f, int pos) {
                          if (f && pos < r) { po[pos] = s.cid[s.a_pos[p]]; pa[pos] = part[p]; so[pos] = best[p]; }
                      });
    }
    block_compact(c, s.wave_tot, [&](int j) { return !gone[j]; },
                  [&](int j, int f, int pos) {
                      if (f && pos < k) { ko[pos] = s.cid[j]; keep_t[s.cid[j]] = 1; }
                  });      // ends synchronised: keep_t is complete
    if (m > 0) {
        long long* dr = dropped + (long)b * m;
        block_compact(T, s.wave_tot, [&](int t) { return !keep_t[t]; },
                      [&](int t, int f, int pos) { if (f && pos < m) dr[pos] = t; });
    }
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

// qkv [B * n, 3, H, 64] fp32 -> metric [B, n, 64]
int d2s_key_metric_f32(const float* qkv, int B, int n, int H, float* metric, hipStream_t stream) {
    if (!qkv || !metric || B <= 0 || n <= 0 || H <= 0) return D2S_ERR_ARG;
    const long rows = (long)B * n;
    if ((rows + 15) / 16 > INT_MAX) return D2S_ERR_ARG;
    if (overlaps(qkv, (size_t)rows * 3 * H * SP_DH * sizeof(float), metric, (size_t)rows * SP_DH * sizeof(float))) return D2S_ERR_ARG;
    hipLaunchKernelGGL(key_metric_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, stream, qkv, rows, H, metric);
    return d2s_check_launch();
}

// metric [B, n, 64], probs [B, T], cand [B, c] int64 ascending -> kept [B, c - r], dropped [B, T - c + r], pruned / partner [B, r] int64,
// sim [B, r]
int d2s_sim_prune_f32(const float* metric, const float* probs, const long long* cand, int B, int n, int lead, int T, int c, int r,
                      long long* kept, long long* dropped, long long* pruned, long long* partner, float* sim, hipStream_t stream) {
    if (!metric || !probs || !cand || !kept || B <= 0 || B > 65535 || n <= 0 || lead < 0) return D2S_ERR_ARG;
    if (c < 1 || c > T || T > SP_MAXT || (long)lead + T > n || r < 0 || r > c / 2) return D2S_ERR_ARG;
    const int k = c - r, m = T - k;
    if ((m > 0 && !dropped) || (r > 0 && (!pruned || !partner || !sim))) return D2S_ERR_ARG;
    const void* in[3] = {metric, probs, cand};
    const size_t in_bytes[3] = {(size_t)B * n * SP_DH * sizeof(float), (size_t)B * T * sizeof(float), (size_t)B * c * sizeof(long long)};
    const void* out[5] = {kept, dropped, pruned, partner, sim};
    const size_t out_bytes[5] = {(size_t)B * k * sizeof(long long), (size_t)B * m * sizeof(long long), (size_t)B * r * sizeof(long long),
                                 (size_t)B * r * sizeof(long long), (size_t)B * r * sizeof(float)};
    for (int o = 0; o < 5; ++o)
        for (int i = 0; i < 3; ++i)
            if (overlaps(out[o], out_bytes[o], in[i], in_bytes[i])) return D2S_ERR_ARG;
    if (r > 0)
        hipLaunchKernelGGL(sim_match_kernel, dim3((c / 2 + SP_TILE - 1) / SP_TILE, B), dim3(256), 0, stream, metric, probs, cand, n, lead, T,
                           c, r, kept);
    hipLaunchKernelGGL(sim_select_kernel, dim3(B), dim3(256), 0, stream, probs, cand, T, c, r, kept, dropped, pruned, partner, sim);
    return d2s_check_launch();
}

}  // extern "C"
