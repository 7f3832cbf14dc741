// LTP in the bf16 arithmetic mode ("In the bf16 arithmetic mode"): the attention a token RECEIVES, rebuilt from the
// operands the bf16 attention kernels multiply.
//   ltp_score_bf16_kernel       per head, s_h[j] = sum_i w_i P[h, i, j] (w = 1, or the policy's m_i), as per-head partials in the workspace
//   ltp_score_bf16_fold_kernel  score[j] = (sum_h s_h[j]) / (H * sum_i w_i), heads in ascending order, scaled once
// On the bf16 data path qkv exists in bf16 only and the log-sum-exp (and cinv) was written by the bf16 attention forward from the
// bf16-rounded operands q and bf16(fp32(k) * scale); the fp32 score kernel (ltp.hip) reads fp32 qkv and cannot serve.  This kernel is the
// key-stationary loop of the bf16 attention backward's dK/dV pass (attn_bwd_dkv_bf16_kernel, attention_bf16.hip) with everything but P
// stripped, as ltp.hip's is the fp32 pass stripped: a wave keeps 32 keys as four bf16x8 fragments, scaled before the bf16 rounding, the
// image's query rows stream through one 32-row LDS tile (the next tile travels through registers meanwhile), S = Q K^T runs on
// v_mfma_f32_32x32x16_bf16 (the lane owns ONE key and 16 of the tile's 32 query rows) and P = 2^(fma(S, log2 e, -lse log2 e)) is the
// backward's expression on the backward's operands: the backward's bits.  The lane's column sum needs no atomics: 16 rows per tile in
// register order, tiles in ascending order, then the two half-waves are added once (as the DPOL instantiation sums dpolicy).
// The helpers are copies of attention_bf16.hip's (an anonymous namespace there), so that file compiles exactly as it did.
// Grid: key tile x (image, head), per-head partials plus a fold - ltp.hip's, for ltp.hip's reasons.
// No atomics, no memset, fixed summation orders: two launches on equal inputs give the same bits.
#include "d2s_common.h"
#include "d2s_hip_ltp_bf16.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int DH = 64;
constexpr int KP = 72;   // Q tile row pitch in bf16 (144 B: conflict-free 16-byte fragment reads)

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// thread -> (row = tid / 8 of the 32-row tile, 8 consecutive d).  qkv is bf16 here, so the tile's rows travel as they are: the round trip
// through fp32 that stage_rows / put_rows make at scale 1 is the identity on bf16 values.
__device__ __forceinline__ bf16x8 stage_rows(const __bf16* __restrict__ base, long ld, int row0, int n, int tid) {
    const long row = min(row0 + (tid >> 3), n - 1);          // clamped: rows past the image are masked by lse = +inf
    return *reinterpret_cast<const bf16x8*>(base + row * ld + (tid & 7) * 8);
}
__device__ __forceinline__ void put_rows(__bf16* __restrict__ S, int tid, const bf16x8& v) {      // [row][d], pitch KP
    *reinterpret_cast<bf16x8*>(&S[(tid >> 3) * KP + (tid & 7) * 8]) = v;
}
// this lane's own row, d = 16 kk + 8 half + j, scaled in fp32 and rounded to bf16 once
__device__ __forceinline__ void row_frags(const __bf16* __restrict__ base, long ld, int row, int n, int half, float scale, bf16x8 (&f)[4]) {
    const __bf16* p = base + (long)min(row, n - 1) * ld + 8 * half;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(p + 16 * kk);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[kk][j] = (__bf16)((float)v[j] * scale);
    }
}
// acc[rows of the LDS tile][this lane's own row] = tile (LDS [row][d]) x this lane's fragments
__device__ __forceinline__ f32x16 mma_rows(const __bf16* __restrict__ S, const bf16x8 (&f)[4], int l31, int half) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 tf = *reinterpret_cast<const bf16x8*>(&S[l31 * KP + 16 * kk + 8 * half]);
        acc = mfma_bf16(tf, f[kk], acc);
    }
    return acc;
}

// Image b's rows: dense, rows b * n .. ; VARLEN, cu[b] .. cu[b + 1] clamped to [0, total) and the length to [0, max_n], as VarlenSeg
// does in attention_bf16.hip - a bad cu_seqlens is never dereferenced outside the buffers.  Both kernels use this one function, so
// they agree on every segment.
template <bool VARLEN>
__device__ __forceinline__ int ltp_rows(const int* __restrict__ cu, int total, int b, int n, int& row_base) {
    if constexpr (VARLEN) {
        const int r0 = min(max(cu[b], 0), total), r1 = min(max(cu[b + 1], r0), total);
        row_base = r0;
        return min(r1 - r0, n);
    } else {
        row_base = b * n;
        return n;
    }
}

struct LtpScoreBf16Args {
    const __bf16* qkv; const float* lse; const float* policy; const float* cinv; const int* cu;
    float* part; float* score;
    int n, H, total; float scale;
};

// part: [B, H, n] (dense) or [H, total] (VARLEN) - the layout of lse.  POLICY: the summand is (P~_ij mk_ij + cinv_i) m_i with
// P~_ij = exp(S_ij - lse_i), mk_ij = policy_j off the diagonal and 1 on it - the probabilities d2s_attn_policy_fwd_bf16 defines and its
// backward feeds to dV - and m_i = policy_i the query's weight.  With an all-ones policy and cinv = 0 every extra operation is a
// multiplication by 1 or an addition of 0: the plain form's bits.
template <bool POLICY, bool VARLEN>
__global__ __launch_bounds__(256, 4) void ltp_score_bf16_kernel(LtpScoreBf16Args a) {
    static_assert(!(POLICY && VARLEN), "the ragged form has no policy");
    __shared__ __attribute__((aligned(16))) __bf16 Qs[32 * KP];
    __shared__ float lse_s[32];
    __shared__ float ci_s[POLICY ? 32 : 1], m_s[POLICY ? 32 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all key tiles of one head on one XCD (they stream the same Q panel)
    const int H = a.H;
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    int row_base;
    const int n = ltp_rows<VARLEN>(a.cu, a.total, b, a.n, row_base);
    if (bx * 128 >= n) return;                          // block-uniform, before any barrier: this image has no keys in this tile
    const long stat0 = VARLEN ? (long)h * a.total + row_base : ((long)b * H + h) * n;
    const __bf16* qb = a.qkv + (long)row_base * ld + h * DH;
    const __bf16* kb = qb + (long)H * DH;
    const float* lse_b = a.lse + stat0;
    const float* ci_b = POLICY ? a.cinv + stat0 : nullptr;
    const float* polb = POLICY ? a.policy + (long)b * n : nullptr;
    const int k0 = bx * 128 + wave * 32;
    const bool active = k0 < n, kok = k0 + l31 < n;
    constexpr float L2E = 1.44269504088896340736f;

    bf16x8 kf[4];
    row_frags(kb, ld, k0 + l31, n, half, a.scale, kf);      // scaled keys, as the backward scales them
    float pol_key = 0.f;                                    // POLICY: this lane's key's policy
    if constexpr (POLICY) pol_key = kok ? polb[k0 + l31] : 0.f;

    const int ntiles = (n + 31) / 32;
    bf16x8 qr;
    float lr = 0.f, cir = 0.f, mr = 0.f;
    float col = 0.f;
    auto fetch = [&](int row0) {
        qr = stage_rows(qb, ld, row0, n, tid);
        if (tid < 32) {
            const int qi = row0 + tid, qc = min(qi, n - 1);
            const float l0 = lse_b[qc];
            lr = qi < n ? l0 * L2E : INFINITY;      // queries past the image: p = 2^(s log2 e - inf) = 0
            if constexpr (POLICY) {
                const float c0 = ci_b[qc], m0 = polb[qc];
                cir = qi < n ? c0 : 0.f;            // ... and they carry cinv = 0 and weight 0
                mr = qi < n ? m0 : 0.f;
            }
        }
    };
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        put_rows(Qs, tid, qr);
        if (tid < 32) { lse_s[tid] = lr; if (POLICY) { ci_s[tid] = cir; m_s[tid] = mr; } }
        __syncthreads();
        if (t + 1 < ntiles) fetch((t + 1) * 32);       // the next tile's rows travel through registers while this tile is multiplied
        if (!active) continue;
        const f32x16 s = mma_rows(Qs, kf, l31, half);  // S[query = row(r, half)][key = l31], scaled
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = mfma32_row(r, half);
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_s[qi]));      // P~, the backward's expression
            if constexpr (POLICY) {
                const bool diag = t * 32 == k0 && qi == l31;      // a wave's 32 keys start at a multiple of 32: one query tile holds the diagonal
                p *= diag ? 1.f : pol_key;
                p = (p + ci_s[qi]) * m_s[qi];
            }
            col += p;
        }
    }
    if (!active) return;
    col += __shfl_xor(col, 32, 64);      // the other half-wave's 16 rows of every tile (commutative: both halves hold the same bits)
    if (half == 0 && kok) a.part[stat0 + k0 + l31] = col;
}

// score[row_base + j] = (sum_h part_h[j]) / (H * den), h ascending; den = the image's rows (plain, VARLEN) or the sum of its policy
// (lane-strided partials, wave butterfly, waves as (0+1)+(2+3)): the fp32 fold's order and meaning.  One workgroup per image.
template <bool POLICY, bool VARLEN>
__global__ __launch_bounds__(256) void ltp_score_bf16_fold_kernel(LtpScoreBf16Args a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, H = a.H;
    int row_base;
    const int n = ltp_rows<VARLEN>(a.cu, a.total, b, a.n, row_base);
    if (n <= 0) return;
    float den = (float)n;
    if constexpr (POLICY) {
        float v = 0.f;
        for (int i = tid; i < n; i += 256) v += a.policy[(long)b * n + i];
        v = wave_sum(v);
        if (lane == 0) red[wave] = v;
        __syncthreads();
        den = (red[0] + red[1]) + (red[2] + red[3]);
    }
    const float div = (float)H * den;
    for (int j = tid; j < n; j += 256) {
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += a.part[(VARLEN ? (long)h * a.total + row_base : ((long)b * H + h) * n) + j];
        a.score[(long)row_base + j] = s / div;
    }
}

template <bool POLICY, bool VARLEN>
int ltp_score_bf16_launch(const LtpScoreBf16Args& a, int B, hipStream_t stream) {
    hipLaunchKernelGGL((ltp_score_bf16_kernel<POLICY, VARLEN>), dim3((a.n + 127) / 128, B * a.H), dim3(256), 0, stream, a);
    hipLaunchKernelGGL((ltp_score_bf16_fold_kernel<POLICY, VARLEN>), dim3(B), dim3(256), 0, stream, a);
    return d2s_check_launch();
}

}  // namespace

extern "C" {

size_t d2s_ltp_score_bf16_workspace_bytes(long rows, int H) {
    if (rows <= 0 || H <= 0) return 0;
    return (size_t)rows * (size_t)H * sizeof(float);
}

int d2s_ltp_score_bf16(const void* qkv, const float* lse, const float* policy, const float* cinv, const int* cu_seqlens, float* score,
                       void* workspace, size_t workspace_bytes, int B, int n, int total, int H, float scale, hipStream_t stream) {
    if (!qkv || !lse || !score || !workspace || B <= 0 || n <= 0 || n > 8192 || total <= 0 || H <= 0) return D2S_ERR_ARG;
    if ((policy != nullptr) != (cinv != nullptr) || (policy && cu_seqlens)) return D2S_ERR_ARG;
    if (!cu_seqlens && (long)B * n != (long)total) return D2S_ERR_ARG;
    if (workspace_bytes < d2s_ltp_score_bf16_workspace_bytes(total, H)) return D2S_ERR_ARG;
    const LtpScoreBf16Args a{static_cast<const __bf16*>(qkv), lse, policy, cinv, cu_seqlens, static_cast<float*>(workspace), score, n, H, total,
                             scale};
    if (cu_seqlens) return ltp_score_bf16_launch<false, true>(a, B, stream);
    if (policy) return ltp_score_bf16_launch<true, false>(a, B, stream);
    return ltp_score_bf16_launch<false, false>(a, B, stream);
}

}  // extern "C"
