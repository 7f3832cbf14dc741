// LTP baseline (learned per-block token thresholds; DESIGN.md section 27 - the build's own definition): the kernels.
//   ltp_score_kernel          the attention a token RECEIVES: per head, the column sums of the softmax P the block's attention computed,
//                             s_h[j] = sum_i w_i P[h, i, j] (w = 1, or the policy's m_i), as per-head partials in the workspace
//   ltp_score_fold_kernel     score[j] = (sum_h s_h[j]) / (H * sum_i w_i), heads in ascending order, scaled once
//   ltp_select_kernel         keep = CLS or (score >= theta) on the ragged packed batch, counts for the re-pack
//   ltp_soft_mask_fwd_kernel  M = sigmoid((score - theta) / tau), m_out = m_in * M, per-image sums of M (the regulariser)
//   ltp_soft_mask_bwd_kernel  gM, gm_in and the per-image partials of dtheta; ltp_dtheta_fold_kernel sums them in image order
// The score kernel is the key-stationary loop of the fp32 attention backward's dK/dV pass (attention_f32.hip) with everything but P
// stripped: a wave keeps 32 keys in registers while the query tiles of the image stream through LDS, S = Q K^T runs on the f32-input
// MFMA (natural orientation: the lane owns ONE key and 16 of the tile's 32 query rows), P is recomputed from the saved log-sum-exp by
// the backward's own expression - so the probabilities are the backward's bits - and the lane's column sum needs no atomics: 16 rows per
// tile in register order, tiles in ascending order, then the two half-waves are added once.  The helpers are copies of that file's, so
// that its kernels compile exactly as they did.
// Grid: key tile x (image, head), as the backward's - per-head partials plus a fold rather than a head loop inside the workgroup: at
// n = 197 an image has two 128-key tiles, and B * 2 workgroups would leave most of the 256 CUs idle at small B, while the partials cost
// H * rows floats of traffic, nothing next to the qkv rows each workgroup streams.
// fp32 only, no atomics, fixed summation orders: two launches on equal inputs give the same bits.
#include "d2s_common.h"
#include "d2s_hip_ltp.h"

namespace {

constexpr int DH = 64;
constexpr int PITCH = 68;  // floats; 16-B aligned rows, conflict-free ds_read_b128 for 16 distinct rows

// operand fragment of one token row for lane (row, half): r[t] = base[row][8t + 4half .. +3] * scale
__device__ __forceinline__ void load_rows_regs(const float* __restrict__ base, long ld, int row, int nrows, int half, float scale,
                                               f32x4 (&r)[8]) {
    if (row < nrows) {
        const float* p = base + (long)row * ld + 4 * half;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            r[t] = *reinterpret_cast<const f32x4*>(p + 8 * t);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[t][j] *= scale;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) r[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// cooperative load of a 32-row x 64-float tile (rows row0.., zero-filled beyond nrows) by 256 threads: 2 float4 each
__device__ __forceinline__ void tile_load(const float* __restrict__ base, long ld, int row0, int nrows, int tid, f32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256, row = row0 + (f >> 4), d4 = (f & 15) * 4;
        r[i] = row < nrows ? *reinterpret_cast<const f32x4*>(base + (long)row * ld + d4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
__device__ __forceinline__ void tile_store(float* __restrict__ S, int tid, const f32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256;
        *reinterpret_cast<f32x4*>(&S[(f >> 4) * PITCH + (f & 15) * 4]) = r[i];
    }
}

// acc[r] += sum_d X[rowlane][d] * Yreg[d]  : A operand from an LDS tile (row = lane&31), B operand from registers
__device__ __forceinline__ void mma_lds_reg(const float* __restrict__ S, int l31, int half, const f32x4 (&y)[8], f32x16& acc) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&S[l31 * PITCH + 8 * t + 4 * half]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(a[j], y[t][j], acc);
    }
}

// Image b's rows: dense, rows b * n .. ; VARLEN, cu[b] .. cu[b + 1] clamped to [0, total) and the length to [0, max_n] - a bad
// cu_seqlens is never dereferenced outside the buffers.  Both kernels of the score use this one function, so they agree on every segment.
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

struct LtpScoreArgs {
    const float* qkv; const float* lse; const float* policy; const float* cinv; const int* cu;
    float* part; float* score;
    int n, H, total; float scale;
};

// part: [B, H, n] (dense) or [H, total] (VARLEN) - the layout of lse.  POLICY: P_ij = exp(S_ij - lse_i) mk_ij + cinv_i with mk_ij =
// policy_j off the diagonal and 1 on it, exactly the probabilities d2s_attn_policy_fwd_f32 defines (and its backward feeds to dV); the
// query row i enters with weight policy_i.  With an all-ones policy and cinv = 0 every extra operation is a multiplication by 1 or an
// addition of 0: the plain form's bits.
template <bool POLICY, bool VARLEN>
__global__ __launch_bounds__(256, 3) void ltp_score_kernel(LtpScoreArgs a) {
    static_assert(!(POLICY && VARLEN), "the ragged form has no policy");
    __shared__ __attribute__((aligned(16))) float Qs[32 * PITCH];
    __shared__ float lse_s[32], ci_s[32], m_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all key tiles of one head on one XCD (they stream the same Q panel)
    const int H = a.H;
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    int row_base;
    const int n = ltp_rows<VARLEN>(a.cu, a.total, b, a.n, row_base);
    if (bx * 128 >= n) return;                          // block-uniform: this image has no keys in this tile
    const long stat0 = VARLEN ? (long)h * a.total + row_base : ((long)b * H + h) * n;
    const float* qb = a.qkv + (long)row_base * ld + h * DH;
    const float* kb = qb + (long)H * DH;
    const float* lse_b = a.lse + stat0;
    const float* ci_b = POLICY ? a.cinv + stat0 : nullptr;
    const float* polb = POLICY ? a.policy + (long)b * n : nullptr;
    const int k0 = bx * 128 + wave * 32;
    const bool active = k0 < n;

    f32x4 kreg[8];
    load_rows_regs(kb, ld, k0 + l31, n, half, a.scale, kreg);  // scaled keys, as the backward scales them
    const float pol_key = (POLICY && k0 + l31 < n) ? polb[k0 + l31] : 0.f;   // this lane's key

    const int ntiles = (n + 31) / 32;
    f32x4 qr[2];
    float lr = 0.f, cir = 0.f, mr = 0.f;
    float col = 0.f;
    tile_load(qb, ld, 0, n, tid, qr);
    if (tid < 32) {
        lr = tid < n ? lse_b[tid] : INFINITY;
        if (POLICY) { cir = tid < n ? ci_b[tid] : 0.f; mr = tid < n ? polb[tid] : 0.f; }
    }
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        tile_store(Qs, tid, qr);
        if (tid < 32) { lse_s[tid] = lr; if (POLICY) { ci_s[tid] = cir; m_s[tid] = mr; } }
        __syncthreads();
        if (t + 1 < ntiles) {       // the next tile's rows travel through registers while this tile is multiplied
            tile_load(qb, ld, (t + 1) * 32, n, tid, qr);
            if (tid < 32) {
                const int qi = (t + 1) * 32 + tid;
                lr = qi < n ? lse_b[qi] : INFINITY;
                if (POLICY) { cir = qi < n ? ci_b[qi] : 0.f; mr = qi < n ? polb[qi] : 0.f; }
            }
        }
        if (!active) continue;
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        mma_lds_reg(Qs, l31, half, kreg, s);   // S[query = row(r,half)][key = l31], scaled
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = mfma32_row(r, half);
            float p = __expf(s[r] - lse_s[qi]);  // rows beyond n carry lse = +inf -> p = 0
            if (POLICY) {
                p *= (t * 32 + qi == k0 + l31) ? 1.f : pol_key;
                p = (p + ci_s[qi]) * m_s[qi];    // rows beyond n carry cinv = 0 and weight 0
            }
            col += p;
        }
    }
    if (!active) return;
    col += __shfl_xor(col, 32, 64);      // the other half-wave's 16 rows of every tile (commutative: both halves hold the same bits)
    if (half == 0 && k0 + l31 < n) a.part[stat0 + k0 + l31] = col;
}

// score[row_base + j] = (sum_h part_h[j]) / (H * den), h ascending; den = the image's rows (plain, VARLEN) or the sum of its policy
// (lane-strided partials, wave butterfly, waves as (0+1)+(2+3)).  One workgroup per image.
template <bool POLICY, bool VARLEN>
__global__ __launch_bounds__(256) void ltp_score_fold_kernel(LtpScoreArgs a) {
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
int ltp_score_launch(const LtpScoreArgs& a, int B, hipStream_t stream) {
    hipLaunchKernelGGL((ltp_score_kernel<POLICY, VARLEN>), dim3((a.n + 127) / 128, B * a.H), dim3(256), 0, stream, a);
    hipLaunchKernelGGL((ltp_score_fold_kernel<POLICY, VARLEN>), dim3(B), dim3(256), 0, stream, a);
    return d2s_check_launch();
}

__device__ __forceinline__ float ltp_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// sum over the workgroup's 256 threads in a fixed order: wave butterfly, waves as (0+1)+(2+3); every thread gets the result
__device__ __forceinline__ float ltp_block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per image of the packed batch (segment clamped to [0, total)): keep = 1 at the CLS row (the segment's first) and where
// score >= theta[0] (fp32 against fp32; a NaN score is dropped), counts[b] = kept rows without CLS.  dense [B, T] (optional): 1 at
// row_src[r] - 1 of every kept non-CLS row, 0 elsewhere; a row whose row_src is outside [1, T] is left out of it.
__global__ __launch_bounds__(256) void ltp_select_kernel(const float* __restrict__ score, const int* __restrict__ cu,
                                                         const int* __restrict__ row_src, const float* __restrict__ theta,
                                                         float* __restrict__ keep, int* __restrict__ counts, float* __restrict__ dense,
                                                         int T, int total) {
    __shared__ int redi[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = min(max(cu[b], 0), total);
    const int n = min(max(cu[b + 1], r0), total) - r0;
    const float th = theta[0];
    if (dense) {
        for (int t = tid; t < T; t += 256) dense[(long)b * T + t] = 0.f;
        __syncthreads();                 // the flags below land on the zeros (same workgroup, barrier in between)
    }
    int kept = 0;
    if (tid == 0 && n > 0) keep[r0] = 1.f;
    for (int i = 1 + tid; i < n; i += 256) {
        const int r = r0 + i;
        const bool k = score[r] >= th;
        keep[r] = k ? 1.f : 0.f;
        kept += k ? 1 : 0;
        if (dense && k) {
            const int t = row_src[r];
            if (t >= 1 && t <= T) dense[(long)b * T + t - 1] = 1.f;
        }
    }
    kept = wave_sum_i(kept);
    if (lane == 0) redi[wave] = kept;
    __syncthreads();
    if (tid == 0) counts[b] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
}

// Dense [B, N], token 0 = CLS.  M = sigmoid((score - theta) * inv_tau) at the patches and 1 at CLS, m_out = m_in * M (m_in null: ones),
// msum[b] = sum of M over the image's patches (lane-strided partials, then ltp_block_sum).
__global__ __launch_bounds__(256) void ltp_soft_mask_fwd_kernel(const float* __restrict__ score, const float* __restrict__ m_in,
                                                                const float* __restrict__ theta, float* __restrict__ M,
                                                                float* __restrict__ m_out, float* __restrict__ msum, int N,
                                                                float inv_tau) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long o = (long)blockIdx.x * N;
    const float th = theta[0];
    float acc = 0.f;
    for (int t = tid; t < N; t += 256) {
        float mv = 1.f;
        if (t > 0) {
            mv = ltp_sigmoid((score[o + t] - th) * inv_tau);
            acc += mv;
        }
        M[o + t] = mv;
        m_out[o + t] = (m_in ? m_in[o + t] : 1.f) * mv;
    }
    acc = ltp_block_sum(acc, red);
    if (tid == 0) msum[blockIdx.x] = acc;
}

// g_out: the gradient of m_out.  gM = g_out * m_in + greg[b] at the patches (greg [B] or null: the gradient of msum, the regulariser's
// share lambda / (S B T) times what arrives at the loss - device values, never read on the host) and 0 at CLS; gm_in = (accumulate ?
// gm_in : 0) + g_out * M; dpart[b] = sum over the image's patches of gM * M * (1 - M).  gm_in may be null (the first stage: m_in is
// the constant 1).
__global__ __launch_bounds__(256) void ltp_soft_mask_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ M,
                                                                const float* __restrict__ m_in, const float* __restrict__ greg,
                                                                float* __restrict__ gM, float* __restrict__ gm_in,
                                                                float* __restrict__ dpart, int N, int accumulate) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long o = (long)blockIdx.x * N;
    const float gr = greg ? greg[blockIdx.x] : 0.f;
    float acc = 0.f;
    for (int t = tid; t < N; t += 256) {
        const float g = g_out[o + t], mv = M[o + t];
        float gm = 0.f;
        if (t > 0) {
            gm = g * (m_in ? m_in[o + t] : 1.f) + gr;
            acc += gm * (mv * (1.0f - mv));
        }
        gM[o + t] = gm;
        if (gm_in) gm_in[o + t] = (accumulate ? gm_in[o + t] : 0.f) + g * mv;
    }
    acc = ltp_block_sum(acc, red);
    if (tid == 0) dpart[blockIdx.x] = acc;
}

// dtheta[0] = (accumulate ? dtheta[0] : 0) - inv_tau * sum_b dpart[b]: one wave, lane-strided over the images, then the butterfly
__global__ __launch_bounds__(64) void ltp_dtheta_fold_kernel(const float* __restrict__ dpart, float* __restrict__ dtheta, int B,
                                                             float inv_tau, int accumulate) {
    float v = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) v += dpart[b];
    v = wave_sum(v);
    if (threadIdx.x == 0) dtheta[0] = (accumulate ? dtheta[0] : 0.f) - inv_tau * v;
}

}  // namespace

extern "C" {

size_t d2s_ltp_score_workspace_bytes(long rows, int H) {
    if (rows <= 0 || H <= 0) return 0;
    return (size_t)rows * (size_t)H * sizeof(float);
}

int d2s_ltp_score_f32(const float* qkv, const float* lse, const float* policy, const float* cinv, const int* cu_seqlens, float* score,
                      void* workspace, size_t workspace_bytes, int B, int n, int total, int H, float scale, hipStream_t stream) {
    if (!qkv || !lse || !score || B <= 0 || n <= 0 || n > 8192 || total <= 0 || H <= 0) return D2S_ERR_ARG;
    if ((policy != nullptr) != (cinv != nullptr) || (policy && cu_seqlens)) return D2S_ERR_ARG;
    if (!cu_seqlens && (long)B * n != (long)total) return D2S_ERR_ARG;
    if (!workspace || workspace_bytes < d2s_ltp_score_workspace_bytes(total, H)) return D2S_ERR_WORKSPACE;
    const LtpScoreArgs a{qkv, lse, policy, cinv, cu_seqlens, static_cast<float*>(workspace), score, n, H, total, scale};
    if (cu_seqlens) return ltp_score_launch<false, true>(a, B, stream);
    if (policy) return ltp_score_launch<true, false>(a, B, stream);
    return ltp_score_launch<false, false>(a, B, stream);
}

int d2s_ltp_select(const float* score, const int* cu_seqlens, const int* row_src, const float* theta, float* keep, int* counts,
                   float* dense_mask, int B, int T, int total, hipStream_t stream) {
    if (!score || !cu_seqlens || !theta || !keep || !counts || B <= 0 || total <= 0) return D2S_ERR_ARG;
    if (dense_mask && (!row_src || T <= 0)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ltp_select_kernel, dim3(B), dim3(256), 0, stream, score, cu_seqlens, row_src, theta, keep, counts, dense_mask, T, total);
    return d2s_check_launch();
}

int d2s_ltp_soft_mask_fwd(const float* score, const float* m_in, const float* theta, float* M, float* m_out, float* msum, int B, int N,
                          float inv_tau, hipStream_t stream) {
    if (!score || !theta || !M || !m_out || !msum || B <= 0 || N < 2 || !(inv_tau > 0.f)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ltp_soft_mask_fwd_kernel, dim3(B), dim3(256), 0, stream, score, m_in, theta, M, m_out, msum, N, inv_tau);
    return d2s_check_launch();
}

int d2s_ltp_soft_mask_bwd(const float* g_out, const float* M, const float* m_in, const float* greg, float* gM, float* gm_in,
                          float* dtheta, float* dpart_ws, int B, int N, float inv_tau, int accumulate_gm, int accumulate_dtheta,
                          hipStream_t stream) {
    if (!g_out || !M || !gM || !dtheta || !dpart_ws || B <= 0 || N < 2 || !(inv_tau > 0.f)) return D2S_ERR_ARG;
    if ((accumulate_gm != 0 && accumulate_gm != 1) || (accumulate_dtheta != 0 && accumulate_dtheta != 1)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ltp_soft_mask_bwd_kernel, dim3(B), dim3(256), 0, stream, g_out, M, m_in, greg, gM, gm_in, dpart_ws, N,
                       accumulate_gm);
    hipLaunchKernelGGL(ltp_dtheta_fold_kernel, dim3(1), dim3(64), 0, stream, dpart_ws, dtheta, B, inv_tau, accumulate_dtheta);
    return d2s_check_launch();
}

}  // extern "C"
