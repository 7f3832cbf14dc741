// Attention on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16), head dim 64: forward and backward of the bf16 arithmetic mode
// (d2s_set_gemm_mode(2); BASELINE config 5's regime).  Same contracts as d2s_attn_fwd_f32 / d2s_attn_bwd_f32 - fp32 qkv in, fp32 out /
// log-sum-exp / CLS softmax row / dqkv out - so either backward can run from either forward's outputs.  Q, K, V are
// rounded to bf16 on their way into registers / LDS, the scores, the softmax and both accumulations are fp32.
//
// Orientation (no cross-lane traffic for P, no shuffles for the rescale): S^T = K Q^T as in the fp32 kernel - a lane owns ONE query
// (column) and 16 of the tile's 32 keys - and then O^T = V^T P^T, so the P registers (packed to bf16) are directly the B operand and
// the output accumulator's column is again the lane's own query: the running-maximum rescale and the final 1/l are lane-local.
// The 32x32x16 MFMA wants 8 CONSECUTIVE reduction indices per lane half; the accumulator hands a lane keys {0-3, 8-11} (half 0) /
// {4-7, 12-15} (half 1) of each 16-key block.  A reduction may be walked in any order, so V^T is stored in LDS with its keys permuted
// to that order (pos(key)) and both operands agree.
//
// POLICY (the 32-key-tile forward, dQ and dK/dV; the 64-key-tile forward has no policy form): Attention.softmax_with_policy
// (vit_models/dynamic_vit.py:195-214) fused into the same passes, the math of the fp32 POLICY kernels (attention_f32.hip) in this file's
// orientation:  mk_ij = (i == j) ? 1 : policy[b, j] (real-valued, 0/1 is not assumed; column 0 is the CLS key);
//     e_ij = 2^(s log2 e - m log2 e) mk_ij with the running maximum m over ALL real keys, masked ones included; l_i = sum_j e_ij; the bf16 P
//     that the MFMA multiplies is the masked e;  O_i = (acc_i + (eps/n) vsum) * 1 / (l_i + eps), vsum[d] = the column sum over the n keys of
//     the bf16-rounded V, folded out of the V tiles on their way to LDS (per thread in ascending key order, then 32 partials in ascending
//     order: no atomics);  lse_i = m_i + log(l_i + eps), cinv_i = (eps/n) / (l_i + eps);  CLS row (e_0j mk_0j + eps/n) / (l_0 + eps).
//     With an all-ones policy and eps = 0 every factor is 1 and every addend 0: the bits of the plain kernel.
//   backward:  P~_ij = exp(S_ij - lse_i);  dS_ij = P~_ij mk_ij (dP_ij - delta_i);  dV uses P~_ij mk_ij + cinv_i;
//     DPOL: dpolicy[b, j] = sum_h sum_{i != j} P~_ij (dP_ij - delta_i) - the key-owning lane walks the queries in ascending tile order into
//     [B, H, n] partials, an ordered fold over the heads follows, column 0 = 0; a masked key keeps its non-zero dpolicy, nothing is skipped.
//     As in the fp32 kernels the O(eps) gradient through the row maximum (which the reference's autograd carries because it does not
//     detach the max) is left out: it is <= eps = 1e-6 relative.
//
// VARLEN (the 32-key-tile forward, dQ and dK/dV; no policy): a ragged packed batch, inference with a dynamic keep ratio
// (vit_models/dynamic_vit.py:935-949) and, with VLSE and the two backward kernels, training on it in the bf16 mode (DESIGN.md section
// 10.3).  Image b owns rows cu[b] .. cu[b+1] of qkv [total, 3, H, 64], of out [total, H*64] and of its bf16
// copy; n = cu[b+1] - cu[b] is per image and the kernel's n argument is the bound that sized the grid.  A block whose first query lies past
// its image returns before any barrier (block-uniform).  The CLS softmax row goes to cls_row[h * total + cu[b] + j]; no log-sum-exp is
// written unless VLSE asks for it: lse[h * total + cu[b] + i] = m + log(l) then, the layout of d2s_attn_varlen_fwd_lse_f32.  With
// cu = [0, n, 2n, ...] every block does the dense kernel's arithmetic in the dense kernel's order: the same bits.  In the backward kernels
// lse and delta are read at that place, the 128-row tiles count from the image's own row 0, a workgroup whose tile starts at or past its
// image's n returns before any barrier, and the segment is clamped to [0, total), its length to [0, max_n] (VarlenSeg): the rows of an
// image are the bits of the dense backward on that image alone.
//
// KEYW (the 32-key-tile forward, dQ and dK/dV; no policy, no ragged form): attention whose keys carry weights, token merging on the bf16
// data path, at inference and in training.  out_i = sum_j w_j exp(S_ij) v_j / sum_j w_j exp(S_ij), w = key_w [B, n] >= 1: the
// tile's 32 weights travel through pol_s as a policy does, e_ij = 2^(s log2 e - m log2 e) * w_j (one more fp32 rounding) feeds both the
// row sum and the bf16 P; no diagonal exception.  The running maximum stays the one over the raw scores (w >= 1 keeps e w >= e), so
// lse_i = m_i + log(l_i) is the log of the weighted denominator, d2s_attn_keyw_fwd_f32's definition.  The weights travel in `policy`.
// With unit weights the multiply is by 1.0: the bits of the plain kernel.
//   backward:  P_ij = w_j exp(S_ij - lse_i) with that lse (one more fp32 rounding, before P meets dP - delta or the bf16 packing), then the
//     plain rule dV = P^T dO, dS = P (dP - delta), dQ = scale dS K, dK = scale dS^T Q; the weights get no gradient.  The dQ kernel stages the
//     tile's weights in pol_s as the forward does, the dK/dV kernel keeps its lane's key's weight in one register.  32-key tiles only.
#include "d2s_common.h"
#include "d2s_hip_ext.h"
#include "d2s_hip_ragged_bf16.h"
#include "d2s_hip_tome_train_bf16.h"
#include <cstdlib>
#include <type_traits>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int DH = 64;
constexpr int KP = 72;   // K tile row pitch in bf16 (144 B: conflict-free 16-byte fragment reads)
constexpr int VP = 40;   // V^T tile row pitch in bf16 (80 B)

__device__ __forceinline__ int key_pos(int key) {   // position of a key inside its 16-key block in the MFMA's reduction order
    const int b = key & 15;
    return (key & ~15) | (b < 4 ? b : b < 8 ? b + 4 : b < 12 ? b - 4 : b);
}

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// 8 consecutive values of a q / k / v row as fp32, from the fp32 qkv tensor or from its bf16 form (the qkv GEMM's c_bf16: the same
// values this kernel would round to itself, so both inputs give identical results)
__device__ __forceinline__ void load8(const float* __restrict__ p, f32x4 (&r)[2]) {
    r[0] = *reinterpret_cast<const f32x4*>(p);
    r[1] = *reinterpret_cast<const f32x4*>(p + 4);
}
__device__ __forceinline__ void load8(const __bf16* __restrict__ p, f32x4 (&r)[2]) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[0][j] = (float)v[j]; r[1][j] = (float)v[4 + j]; }
}

// mk of the 16 keys a lane holds in accumulator order (registers 4g .. 4g+3 = tile rows 8g + 4 half + 0..3) from the tile's policy in LDS.
// A wave's 32 queries start at a multiple of 32, so the diagonal i == j lies in one key tile only (diag_tile, wave-uniform), at row l31.
__device__ __forceinline__ void tile_policy(const float* __restrict__ pol_s, int half, int l31, bool diag_tile, f32x4 (&pg)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) pg[g] = *reinterpret_cast<const f32x4*>(&pol_s[8 * g + 4 * half]);
    if (diag_tile) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (mfma32_row(r, half) == l31) pg[r >> 2][r & 3] = 1.f;
    }
}

// policy: POLICY's keep policy or KEYW's key weights, [B, n]; cinv, eps: POLICY; cu, total: VARLEN.  The other instantiations read none of them.
// cinv carries no __restrict__: with it the POLICY instantiations spill 6 SGPRs instead of 2.
template <typename QT, bool POLICY = false, bool VARLEN = false, bool KEYW = false, bool VLSE = false>
__global__ __launch_bounds__(256, 3) void attn_fwd_bf16_kernel(const QT* __restrict__ qkv, float* __restrict__ out,
                                                               __bf16* __restrict__ out16, float* __restrict__ lse, float* __restrict__ cls_row, int n, int H,
                                                               float scale, const float* __restrict__ policy, float* cinv, float eps,
                                                               const int* __restrict__ cu, int total) {
    __shared__ __attribute__((aligned(16))) __bf16 Ks[32 * KP];      // [key][d]
    __shared__ __attribute__((aligned(16))) __bf16 Vt[DH * VP];      // [d][pos(key)]
    __shared__ __attribute__((aligned(16))) float pol_s[(POLICY || KEYW) ? 32 : 1];  // the tile's policy (KEYW: its key weights)
    __shared__ __attribute__((aligned(16))) float vred[POLICY ? 32 * DH : 1];        // [staging key row][d] partial column sums of V
    __shared__ float vsum_s[POLICY ? DH : 1];                                        // (eps/n) * column sums of V
    extern __shared__ __attribute__((aligned(16))) float cls_s[];    // [n] raw scaled scores of query 0 (block 0 only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    static_assert(!(POLICY && VARLEN), "the ragged form has no policy");
    static_assert(!(KEYW && (POLICY || VARLEN)), "key weights combine with neither the policy nor the ragged form");
    static_assert(!VLSE || VARLEN, "VLSE: the ragged form that keeps its log-sum-exp for the backward");
    long tok0 = (long)b * n;                       // first token row of the image
    [[maybe_unused]] long cls0 = 0;                // VARLEN: start of the image's CLS softmax row inside cls_row [H, total]
    if constexpr (VARLEN) {
        const int row_base = cu[b];
        n = cu[b + 1] - row_base;
        if (bx * 128 >= n) return;                 // block-uniform, before any barrier: this image has no queries in this tile
        tok0 = row_base;
        cls0 = (long)h * total + row_base;
    }
    const QT* qb = qkv + tok0 * ld + h * DH;
    const QT* kb = qb + (long)H * DH;
    const QT* vb = kb + (long)H * DH;
    const int q0 = bx * 128 + wave * 32;
    const bool active = q0 < n;
    const bool want_cls = cls_row != nullptr && bx == 0 && wave == 0;
    const float* polb = nullptr;
    if constexpr (POLICY || KEYW) polb = policy + (long)b * n;

    // B operand of S^T = K Q^T: this lane's query, d = 16 kk + 8 half + j, scaled, as bf16 (scale = 2^-3 for 64-wide heads: the product
    // is exact, so fp32 and bf16 qkv inputs round to the same operand).  The softmax is evaluated as 2^(s log2 e - m log2 e): one FMA and
    // one v_exp_f32 per element - the kernel is bound by its softmax VALU work (~150 vector instructions beside 8 MFMAs per 32-key tile
    // before round 3), not by the MFMAs
    const float qscale = scale;
    constexpr float L2E = 1.44269504088896340736f;
    bf16x8 qf[4];
    {
        const int qi = min(q0 + l31, n - 1);
        const QT* p = qb + (long)qi * ld + 8 * half;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            f32x4 ac[2];
            load8(p + 16 * kk, ac);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qf[kk][j] = (__bf16)(ac[0][j] * qscale); qf[kk][4 + j] = (__bf16)(ac[1][j] * qscale); }
        }
    }

    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // staging: thread -> (key = tid / 8, 8 consecutive d); rows past the sequence are clamped (their scores are masked below)
    const int skey = tid >> 3, sd8 = (tid & 7) * 8;
    const int ntiles = (n + 31) / 32;
    f32x4 kr[2], vr[2];
    float pr = 0.f;                              // POLICY: policy of key t * 32 + (tid & 31); KEYW: its weight
    f32x4 vacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};      // POLICY: this thread's 8 columns of V summed over its key rows
    auto fetch = [&](int t) {
        const long row = min(t * 32 + skey, n - 1);
        load8(kb + row * ld + sd8, kr);
        load8(vb + row * ld + sd8, vr);
        if constexpr (POLICY || KEYW) { const int kj = t * 32 + (tid & 31); const float p0 = polb[min(kj, n - 1)]; pr = kj < n ? p0 : 0.f; }
    };
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        {
            bf16x8 kv;
#pragma unroll
            for (int j = 0; j < 4; ++j) { kv[j] = (__bf16)kr[0][j]; kv[4 + j] = (__bf16)kr[1][j]; }
            *reinterpret_cast<bf16x8*>(&Ks[skey * KP + sd8]) = kv;
            const int pos = key_pos(skey);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Vt[(sd8 + j) * VP + pos] = (__bf16)vr[0][j];
                Vt[(sd8 + 4 + j) * VP + pos] = (__bf16)vr[1][j];
            }
            if constexpr (KEYW) {
                if (tid < 32) pol_s[tid] = pr;
            }
            if (POLICY) {
                if (tid < 32) pol_s[tid] = pr;
                if (t * 32 + skey < n) {         // rows past the sequence are clamped copies of the last key: not summed
#pragma unroll
                    for (int j = 0; j < 4; ++j) { vacc[0][j] += (float)(__bf16)vr[0][j]; vacc[1][j] += (float)(__bf16)vr[1][j]; }
                }
            }
        }
        __syncthreads();
        fetch(min(t + 1, ntiles - 1));
        if (!active) continue;

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[l31 * KP + 16 * kk + 8 * half]);
            s = mfma_bf16(kf, qf[kk], s);      // s[r] = S^T[key = row(r, half)][query = l31]
        }
        const int kv0 = t * 32;
        if (kv0 + 32 > n) {          // only the last tile can hold keys past the sequence (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kv0 + mfma32_row(r, half) >= n) s[r] = -INFINITY;
        }
        float mt = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
        if (want_cls && l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kv0 + mfma32_row(r, half);
                if (key < n) cls_s[key] = s[r];
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float m2 = m_new * L2E;
        float rs = 0.f;
        f32x4 pg[4];
        if (POLICY) tile_policy(pol_s, half, l31, kv0 == q0, pg);
        if constexpr (KEYW) {      // the 16 key weights in accumulator order; a key weighs the same for every query, its own included
#pragma unroll
            for (int g = 0; g < 4; ++g) pg[g] = *reinterpret_cast<const f32x4*>(&pol_s[8 * g + 4 * half]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -m2));
            if (POLICY) s[r] *= pg[r >> 2][r & 3];      // keys past the sequence: e = 0 already
            if constexpr (KEYW) s[r] *= pg[r >> 2][r & 3];      // w >= 1 (e w >= e): the running maximum stays the one over the raw scores
            rs += s[r];
        }
        rs += __shfl_xor(rs, 32, 64);
        // O^T columns are this lane's own query: the rescale is lane-local - and after the first tiles the running maximum rarely
        // moves, so the 32 multiplies are skipped whenever no query of the wave needs them (exact: alpha == 1 for every lane then)
        if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * L2E);
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
        }
        l_run += rs;
        m_run = m_new;
        // B operand of O^T = V^T P^T: registers r = 8 kk .. 8 kk + 7 are reduction indices 8 half .. 8 half + 7 of 16-key block kk
        bf16x8 pf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[kk][j] = (__bf16)s[8 * kk + j];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&Vt[(32 * dt + l31) * VP + 16 * kk + 8 * half]);
                o[dt] = mfma_bf16(vf, pf[kk], o[dt]);      // o[dt][r] = O^T[d = 32 dt + row(r, half)][query = l31]
            }
    }
    float c = 0.f;
    if constexpr (POLICY) {      // fold the 32 staging rows' partial column sums -> vsum_s[64] = (eps/n) * sum_key V[key][d]
        c = eps / (float)n;
        *reinterpret_cast<f32x4*>(&vred[skey * DH + sd8]) = vacc[0];
        *reinterpret_cast<f32x4*>(&vred[skey * DH + sd8 + 4]) = vacc[1];
        __syncthreads();
        if (tid < DH) {
            float tsum = 0.f;
#pragma unroll
            for (int g = 0; g < 32; ++g) tsum += vred[g * DH + tid];
            vsum_s[tid] = tsum * c;
        }
        __syncthreads();
    }
    if (!active) return;
    const bool qok = q0 + l31 < n;
    const float inv_l = 1.0f / (POLICY ? l_run + eps : l_run);
    if (qok) {
        const long po = (tok0 + q0 + l31) * H * DH + h * DH;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {      // registers 4g .. 4g+3 hold d = 32 dt + 8 g + 4 half + 0..3
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = POLICY ? (o[dt][4 * g + j] + vsum_s[32 * dt + 8 * g + 4 * half + j]) * inv_l : o[dt][4 * g + j] * inv_l;
                if (out) *reinterpret_cast<f32x4*>(out + po + 32 * dt + 8 * g + 4 * half) = v;
                if (out16) {      // bf16 copy for the projection GEMM of the bf16 mode (its a_bf16)
                    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
                    bf16x4_t hv;
#pragma unroll
                    for (int j = 0; j < 4; ++j) hv[j] = (__bf16)v[j];
                    *reinterpret_cast<bf16x4_t*>(out16 + po + 32 * dt + 8 * g + 4 * half) = hv;
                }
            }
        if constexpr (!VARLEN) {
            if (half == 0) {
                lse[((long)b * H + h) * n + q0 + l31] = m_run + logf(POLICY ? l_run + eps : l_run);
                if (POLICY) cinv[((long)b * H + h) * n + q0 + l31] = c * inv_l;
            }
        }
        if constexpr (VLSE) {
            if (half == 0) lse[cls0 + q0 + l31] = m_run + logf(l_run);      // [H, total]: the image's rows start where its CLS row does
        }
    }
    if (want_cls) {
        const float m0 = __shfl(m_run, 0, 64), il0 = __shfl(inv_l, 0, 64);
        float* cr = cls_row + (VARLEN ? cls0 : ((long)b * H + h) * n);
        for (int j = lane; j < n; j += 64) {
            float e = expf(cls_s[j] - m0);
            if (POLICY) e = e * (j == 0 ? 1.f : polb[j]) + c;
            cr[j] = e * il0;
        }
    }
}

// ---- forward, 64-key tiles, V row-major with transposed reads (round 3) ---------------------------------------------------------------
// Same orientation and outputs as attn_fwd_bf16_kernel; what changes is the tile machinery around the softmax:
//   * 64 keys per tile: half the barriers, row maxima / sums / the rescale test once per 64 keys;
//   * V goes to LDS row-major [key][d] with two ds_write_b128 per thread (like K) instead of 16 scalar ds_write_b16 into a transposed image;
//     the A operand of O^T = V^T P^T (one d row, 8 consecutive keys per lane) is fetched with ds_read_b64_tr_b16, the hardware's transposing
//     read: per 16-lane group it reads a 4-key x 16-d block and hands lane i column i.  The accumulator hands a lane the keys {0-3, 8-11}
//     (half 0) / {4-7, 12-15} (half 1) of a 16-key block as reduction slots 0-7, i.e. exactly two 4-key blocks - no key permutation is
//     needed any more.  Row pitch 96 bf16 (48 dwords): the 4 rows x 2 groups of a half-wave's read start on banks 0, 8, ..., 56.
constexpr int KP2 = 72;   // K tile row pitch (bf16)
constexpr int VP2 = 96;   // V tile row pitch (bf16): 192 B = 48 dwords (conflict-free transposed reads)
typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 tr_frag(const __bf16* __restrict__ base, int off0, int off1) {      // two 4-key blocks -> 8 reduction slots
    const bf16x4v a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4v*)(base + off0));
    const bf16x4v b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4v*)(base + off1));
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[j] = a[j]; r[4 + j] = b[j]; }
    return r;
}

template <typename QT>
__global__ __launch_bounds__(256, 3) void attn_fwd_bf16_kernel64(const QT* __restrict__ qkv, float* __restrict__ out,
                                                                 __bf16* __restrict__ out16, float* __restrict__ lse, float* __restrict__ cls_row, int n, int H,
                                                                 float scale) {
    __shared__ __attribute__((aligned(16))) __bf16 Ks[64 * KP2];      // [key][d]
    __shared__ __attribute__((aligned(16))) __bf16 Vs[64 * VP2];      // [key][d]
    extern __shared__ __attribute__((aligned(16))) float cls_s[];     // [n] raw scaled scores of query 0 (block 0 only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    const QT* qb = qkv + (long)b * n * ld + h * DH;
    const QT* kb = qb + (long)H * DH;
    const QT* vb = kb + (long)H * DH;
    const int q0 = bx * 128 + wave * 32;
    const bool active = q0 < n;
    const bool want_cls = cls_row != nullptr && bx == 0 && wave == 0;
    constexpr float L2E = 1.44269504088896340736f;

    bf16x8 qf[4];
    {
        const int qi = min(q0 + l31, n - 1);
        const QT* p = qb + (long)qi * ld + 8 * half;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            f32x4 ac[2];
            load8(p + 16 * kk, ac);
#pragma unroll
            for (int j = 0; j < 4; ++j) { qf[kk][j] = (__bf16)(ac[0][j] * scale); qf[kk][4 + j] = (__bf16)(ac[1][j] * scale); }
        }
    }
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // staging: thread -> (key = tid / 4 of the 64-key tile, 16 consecutive d); rows past the sequence are clamped (masked below)
    const int skey = tid >> 2, sd16 = (tid & 3) * 16;
    const int ntiles = (n + 63) / 64;
    f32x4 kr[4], vr[4];
    auto fetch = [&](int t) {
        const long row = min(t * 64 + skey, n - 1);
        f32x4 a[2];
        load8(kb + row * ld + sd16, a); kr[0] = a[0]; kr[1] = a[1];
        load8(kb + row * ld + sd16 + 8, a); kr[2] = a[0]; kr[3] = a[1];
        load8(vb + row * ld + sd16, a); vr[0] = a[0]; vr[1] = a[1];
        load8(vb + row * ld + sd16 + 8, a); vr[2] = a[0]; vr[3] = a[1];
    };
    // transposed-read addressing: lane j = 4 q + p of a 16-lane group supplies row q (a key), columns 4 p .. 4 p + 3 (d) of the block
    const int tj = l31 & 15, tq = tj >> 2, tp = tj & 3;
    const int v_lane = (4 * half + tq) * VP2 + 16 * (l31 >> 4) + 4 * tp;      // + 32 dt (d block) + (16 kk [+ 8]) * VP2 (key block)
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        {
            bf16x8 h0, h1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h0[j] = (__bf16)kr[0][j]; h0[4 + j] = (__bf16)kr[1][j]; h1[j] = (__bf16)kr[2][j]; h1[4 + j] = (__bf16)kr[3][j]; }
            *reinterpret_cast<bf16x8*>(&Ks[skey * KP2 + sd16]) = h0;
            *reinterpret_cast<bf16x8*>(&Ks[skey * KP2 + sd16 + 8]) = h1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h0[j] = (__bf16)vr[0][j]; h0[4 + j] = (__bf16)vr[1][j]; h1[j] = (__bf16)vr[2][j]; h1[4 + j] = (__bf16)vr[3][j]; }
            *reinterpret_cast<bf16x8*>(&Vs[skey * VP2 + sd16]) = h0;
            *reinterpret_cast<bf16x8*>(&Vs[skey * VP2 + sd16 + 8]) = h1;
        }
        __syncthreads();
        fetch(min(t + 1, ntiles - 1));
        if (!active) continue;

        f32x16 s[2];
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb2][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(32 * kb2 + l31) * KP2 + 16 * kk + 8 * half]);
                s[kb2] = mfma_bf16(kf, qf[kk], s[kb2]);      // s[kb2][r] = S^T[key = 32 kb2 + row(r, half)][query = l31]
            }
        }
        const int kv0 = t * 64;
        if (kv0 + 64 > n) {          // only the last tile can hold keys past the sequence (wave-uniform)
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kv0 + 32 * kb2 + mfma32_row(r, half) >= n) s[kb2][r] = -INFINITY;
        }
        float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, fmaxf(s[0][r], s[1][r]));
        if (want_cls && l31 == 0) {
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kv0 + 32 * kb2 + mfma32_row(r, half);
                    if (key < n) cls_s[key] = s[kb2][r];
                }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float m2 = m_new * L2E;
        float rs = 0.f;
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kb2][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb2][r], L2E, -m2));
                rs += s[kb2][r];
            }
        rs += __shfl_xor(rs, 32, 64);
        if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * L2E);
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
        }
        l_run += rs;
        m_run = m_new;
        // B operand of O^T = V^T P^T: registers 8 q .. 8 q + 7 of s[kb2] are the reduction slots of 16-key block kk = 2 kb2 + q
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (__bf16)s[kk >> 1][8 * (kk & 1) + j];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const int base = v_lane + 32 * dt + 16 * kk * VP2;
                const bf16x8 vf = tr_frag(Vs, base, base + 8 * VP2);
                o[dt] = mfma_bf16(vf, pf, o[dt]);      // o[dt][r] = O^T[d = 32 dt + row(r, half)][query = l31]
            }
        }
    }
    if (!active) return;
    const bool qok = q0 + l31 < n;
    const float inv_l = 1.0f / l_run;
    if (qok) {
        const long po = ((long)b * n + q0 + l31) * H * DH + h * DH;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = o[dt][4 * g + j] * inv_l;
                if (out) *reinterpret_cast<f32x4*>(out + po + 32 * dt + 8 * g + 4 * half) = v;
                if (out16) {
                    bf16x4v hv;
#pragma unroll
                    for (int j = 0; j < 4; ++j) hv[j] = (__bf16)v[j];
                    *reinterpret_cast<bf16x4v*>(out16 + po + 32 * dt + 8 * g + 4 * half) = hv;
                }
            }
        if (half == 0) lse[((long)b * H + h) * n + q0 + l31] = m_run + logf(l_run);
    }
    if (want_cls) {
        const float m0 = __shfl(m_run, 0, 64), il0 = __shfl(inv_l, 0, 64);
        float* cr = cls_row + ((long)b * H + h) * n;
        for (int j = lane; j < n; j += 64) cr[j] = expf(cls_s[j] - m0) * il0;
    }
}

// staging helpers shared by the backward kernels: thread -> (row = tid / 8 of the 32-row tile, 8 consecutive d)
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ base, long ld, int row0, int n, int tid, f32x4 (&r)[2]) {
    const long row = min(row0 + (tid >> 3), n - 1);          // clamped: consumers mask by index / by lse = +inf
    load8(base + row * ld + (tid & 7) * 8, r);
}
__device__ __forceinline__ void put_rows(__bf16* __restrict__ S, int tid, const f32x4 (&r)[2], float scale) {      // [row][d], pitch KP
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = (__bf16)(r[0][j] * scale); v[4 + j] = (__bf16)(r[1][j] * scale); }
    *reinterpret_cast<bf16x8*>(&S[(tid >> 3) * KP + (tid & 7) * 8]) = v;
}
__device__ __forceinline__ void put_rows_t(__bf16* __restrict__ St, int tid, const f32x4 (&r)[2]) {                // [d][pos(row)], pitch VP
    const int pos = key_pos(tid >> 3), d8 = (tid & 7) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        St[(d8 + j) * VP + pos] = (__bf16)r[0][j];
        St[(d8 + 4 + j) * VP + pos] = (__bf16)r[1][j];
    }
}
template <typename T>
__device__ __forceinline__ void row_frags(const T* __restrict__ base, long ld, int row, int n, int half, float scale, bf16x8 (&f)[4]) {
    const T* p = base + (long)min(row, n - 1) * ld + 8 * half;       // this lane's own row, d = 16 kk + 8 half + j
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        f32x4 ac[2];
        load8(p + 16 * kk, ac);
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[kk][j] = (__bf16)(ac[0][j] * scale); f[kk][4 + j] = (__bf16)(ac[1][j] * scale); }
    }
}
__device__ __forceinline__ void pack2(const f32x16& s, bf16x8 (&pf)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[kk][j] = (__bf16)s[8 * kk + j];
}
// acc^T[dt] += T^T-tile (LDS [d][pos]) x packed registers: the O^T = V^T P^T step of the forward, reused by every backward product
__device__ __forceinline__ void mma_t(const __bf16* __restrict__ St, const bf16x8 (&pf)[2], int l31, int half, f32x16 (&acc)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 tf = *reinterpret_cast<const bf16x8*>(&St[(32 * dt + l31) * VP + 16 * kk + 8 * half]);
            acc[dt] = mfma_bf16(tf, pf[kk], acc[dt]);
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
// acc^T -> one row of 64 d (at element offset `off` of p, and of the optional bf16 copy p16)
__device__ __forceinline__ void store_t(const f32x16 (&acc)[2], float* __restrict__ p, __bf16* __restrict__ p16, long off, int half, float mul) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[dt][4 * g + j] * mul;
            if (p) *reinterpret_cast<f32x4*>(p + off + 32 * dt + 8 * g + 4 * half) = v;
            if (p16) {
                typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
                bf16x4_t hv;
#pragma unroll
                for (int j = 0; j < 4; ++j) hv[j] = (__bf16)v[j];
                *reinterpret_cast<bf16x4_t*>(p16 + off + 32 * dt + 8 * g + 4 * half) = hv;
            }
        }
}

// VARLEN in the two backward kernels: image b owns rows cu[b] .. cu[b+1] of qkv / dout / dqkv, `n` arrives as max_n.  The segment is clamped
// to [0, total) and its length to [0, max_n]: no cu value is dereferenced outside the buffers.  The ragged form has no policy, so the
// segment travels in the place of the kernels' last (policy) argument: the dense and POLICY instantiations keep the argument list, the
// argument layout and with them the instructions they had (one more argument, even an empty one, moves the hidden grid-size words and
// re-schedules the DPOL dK/dV).
struct VarlenSeg { const int* cu; int total; };
__device__ __forceinline__ int varlen_rows(VarlenSeg v, int b, int max_n, int& row_base) {
    const int r0 = min(max(v.cu[b], 0), v.total), r1 = min(max(v.cu[b + 1], r0), v.total);
    row_base = r0;
    return min(r1 - r0, max_n);
}

// ---- backward, dQ: a lane owns one query; loop over key tiles (S^T, dP^T, dS^T lane-local, dQ^T = K^T dS^T) ------------------------
// ONE_KEY (both backward kernels): an image of one key - a CLS-only image of a ragged batch, or the dense entry at n = 1 - has the constant
// softmax row 1, so dS = 0 and dQ = dK = 0 exactly.  The tile loop leaves (rb(dO) - dO) . v there (dP multiplies the bf16-rounded dO, delta
// the unrounded one: one bf16 rounding of dO); with the flag the exact zeros are written instead.  The ragged launch sets it and the dense
// launch picks the flagged instantiation at n = 1 only, so an image's rows stay the bits of the dense backward on that image alone and
// every instantiation that runs at n > 1 keeps its code.  The POLICY kernels do not take it.
// `tail` is the policy (const float*; read by the POLICY instantiations only; no __restrict__: with it the one on fp32 qkv re-schedules) or,
// VARLEN, the segment table.  KEYW: the key weights [B, n] travel in `tail` as a policy does.
template <typename QT, bool POLICY = false, bool VARLEN = false, bool ONE_KEY = false, bool KEYW = false>
__global__ __launch_bounds__(256, 3) void attn_bwd_dq_bf16_kernel(const QT* __restrict__ qkv, const float* __restrict__ dout,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  float* __restrict__ dqkv, __bf16* __restrict__ dqkv16, int n, int H, float scale,
                                                                  std::conditional_t<VARLEN, VarlenSeg, const float*> tail) {
    static_assert(!(POLICY && (VARLEN || ONE_KEY)), "the ragged form has no policy, the policy kernels no one-key form");
    static_assert(!(KEYW && (POLICY || VARLEN || ONE_KEY)), "key weights combine with neither the policy, the ragged nor the one-key form");
    __shared__ __attribute__((aligned(16))) __bf16 Ks[32 * KP];
    __shared__ __attribute__((aligned(16))) __bf16 Vs[32 * KP];
    __shared__ __attribute__((aligned(16))) __bf16 Kt[DH * VP];
    __shared__ __attribute__((aligned(16))) float pol_s[(POLICY || KEYW) ? 32 : 1];      // the tile's policy (KEYW: its key weights)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    [[maybe_unused]] int row_base = 0;             // VARLEN: the image's first row of the packed batch
    [[maybe_unused]] long stat0v = 0;              // VARLEN: the image's first lse / delta entry of [H, total]
    if constexpr (VARLEN) {
        n = varlen_rows(tail, b, n, row_base);
        if (bx * 128 >= n) return;                 // block-uniform, before any barrier: this image has no queries in this tile
        stat0v = (long)h * tail.total + row_base;
    }
    // the dense offsets stay spelled where they are used: the dense instantiations keep their address arithmetic
    const QT* qb = qkv + (VARLEN ? (long)row_base : (long)b * n) * ld + h * DH;
    const QT* kb = qb + (long)H * DH;
    const QT* vb = kb + (long)H * DH;
    const float* dob = dout + (VARLEN ? (long)row_base : (long)b * n) * ldo + h * DH;
    const int q0 = bx * 128 + wave * 32;
    const bool active = q0 < n, qok = q0 + l31 < n;
    bf16x8 qf[4], dof[4];
    row_frags(qb, ld, q0 + l31, n, half, scale, qf);
    constexpr float L2E = 1.44269504088896340736f;      // p = 2^(s log2 e - lse log2 e): one FMA and one v_exp_f32 per element
    row_frags(dob, ldo, q0 + l31, n, half, 1.0f, dof);
    const float lse_i = qok ? lse[(VARLEN ? stat0v : ((long)b * H + h) * n) + q0 + l31] * 1.44269504088896340736f : INFINITY;
    const float dl_i = qok ? delta[(VARLEN ? stat0v : ((long)b * H + h) * n) + q0 + l31] : 0.f;
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    const int ntiles = (n + 31) / 32;
    f32x4 kr[2], vr[2];
    const float* polb = nullptr;
    float pr = 0.f;                              // POLICY: policy of the staged tile's key tid & 31; KEYW: its weight
    auto fetch_pol = [&](int row0) {
        const int kj = row0 + (tid & 31);
        const float p0 = polb[min(kj, n - 1)];
        pr = kj < n ? p0 : 0.f;
    };
    if constexpr (POLICY || KEYW) {
        polb = tail + (long)b * n;
        fetch_pol(0);
    }
    stage_rows(kb, ld, 0, n, tid, kr);
    stage_rows(vb, ld, 0, n, tid, vr);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        put_rows(Ks, tid, kr, 1.0f);
        put_rows(Vs, tid, vr, 1.0f);
        put_rows_t(Kt, tid, kr);
        if ((POLICY || KEYW) && tid < 32) pol_s[tid] = pr;
        __syncthreads();
        const int tn = min(t + 1, ntiles - 1) * 32;
        stage_rows(kb, ld, tn, n, tid, kr);
        stage_rows(vb, ld, tn, n, tid, vr);
        if (POLICY || KEYW) fetch_pol(tn);
        if (!active) continue;
        f32x16 s = mma_rows(Ks, qf, l31, half);        // scaled scores^T [key][query]
        const f32x16 dp = mma_rows(Vs, dof, l31, half);  // dP^T[key][query] = sum_d V[key][d] dO[query][d]
        const int kv0 = t * 32;
        if constexpr (POLICY) {                        // dS^T = P~^T mk (dP^T - delta)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 pg = *reinterpret_cast<const f32x4*>(&pol_s[8 * g + 4 * half]);
                if (kv0 == q0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (8 * g + 4 * half + j == l31) pg[j] = 1.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * g + j;
                    s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_i)) * pg[j] * (dp[r] - dl_i);
                }
            }
        } else if constexpr (KEYW) {                   // dS^T = (P~^T w) (dP^T - delta): a key weighs the same for every query, no diagonal exception
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 pg = *reinterpret_cast<const f32x4*>(&pol_s[8 * g + 4 * half]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * g + j;
                    s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_i)) * pg[j] * (dp[r] - dl_i);
                }
            }
        } else
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_i)) * (dp[r] - dl_i);      // dS^T = P^T (dP^T - delta)
        if (kv0 + 32 > n) {          // keys past the sequence exist in the last tile only (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kv0 + mfma32_row(r, half) >= n) s[r] = 0.f;
        }
        bf16x8 pf[2];
        pack2(s, pf);
        mma_t(Kt, pf, l31, half, dq);                    // dQ^T[d][query] += sum_key K[key][d] dS^T[key][query]
    }
    if constexpr (ONE_KEY) {
        if (n == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
        }
    }
    if (active && qok) store_t(dq, dqkv, dqkv16, ((VARLEN ? (long)row_base : (long)b * n) + q0 + l31) * ld + h * DH, half, scale);
}

// ---- backward, dK / dV: a lane owns one key; loop over query tiles ------------------------------------------------------------------
// The policy arguments, read by the POLICY / DPOL instantiations only (dpol_part [B, H, n]: DPOL).  One struct: as three plain arguments the
// DPOL instantiations load them in other groups, and the backward with dpolicy measured 0.3 us slower (118.8 -> 119.1 us at B 128, H 6, n 197).
// VARLEN: the segment table takes the struct's place, as in the dQ kernel.  KEYW: the key weights [B, n] travel in `policy`.
struct AttnPolBwd { const float* policy; const float* cinv; float* dpol_part; };
template <typename QT, bool POLICY = false, bool DPOL = false, bool VARLEN = false, bool ONE_KEY = false, bool KEYW = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_bf16_kernel(const QT* __restrict__ qkv, const float* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   float* __restrict__ dqkv, __bf16* __restrict__ dqkv16, int n, int H, float scale,
                                                                   std::conditional_t<VARLEN, VarlenSeg, AttnPolBwd> pol) {
    static_assert(!DPOL || POLICY, "the policy's gradient needs a policy");
    static_assert(!(POLICY && (VARLEN || ONE_KEY)), "the ragged form has no policy, the policy kernels no one-key form");
    static_assert(!(KEYW && (POLICY || DPOL || VARLEN || ONE_KEY)), "key weights combine with neither the policy, the ragged nor the one-key form");
    __shared__ __attribute__((aligned(16))) __bf16 Qs[32 * KP];
    __shared__ __attribute__((aligned(16))) __bf16 Ds[32 * KP];
    __shared__ __attribute__((aligned(16))) __bf16 Qt[DH * VP];
    __shared__ __attribute__((aligned(16))) __bf16 Dt[DH * VP];
    __shared__ float lse_s[32], dl_s[32];
    __shared__ float ci_s[POLICY ? 32 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    [[maybe_unused]] int row_base = 0;             // VARLEN: the image's first row of the packed batch
    [[maybe_unused]] long stat0v = 0;              // VARLEN: the image's first lse / delta entry of [H, total]
    if constexpr (VARLEN) {
        n = varlen_rows(pol, b, n, row_base);      // `pol` is the segment table here
        if (bx * 128 >= n) return;                 // block-uniform, before any barrier: this image has no keys in this tile
        stat0v = (long)h * pol.total + row_base;
    }
    const QT* qb = qkv + (VARLEN ? (long)row_base : (long)b * n) * ld + h * DH;
    const QT* kb = qb + (long)H * DH;
    const QT* vb = kb + (long)H * DH;
    const float* dob = dout + (VARLEN ? (long)row_base : (long)b * n) * ldo + h * DH;
    const float* lse_b = lse + (VARLEN ? stat0v : ((long)b * H + h) * n);
    const float* dl_b = delta + (VARLEN ? stat0v : ((long)b * H + h) * n);
    const int k0 = bx * 128 + wave * 32;
    const bool active = k0 < n, kok = k0 + l31 < n;
    bf16x8 kf[4], vf[4];
    row_frags(kb, ld, k0 + l31, n, half, scale, kf);     // scaled copy: only the scores use it
    constexpr float L2E = 1.44269504088896340736f;
    row_frags(vb, ld, k0 + l31, n, half, 1.0f, vf);
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
    const int ntiles = (n + 31) / 32;
    f32x4 qr[2], dr[2];
    float lr, dlr;
    const float* ci_b = nullptr;
    float pol_key = 0.f, cir = 0.f, dpol_acc = 0.f;      // POLICY: this lane's key's policy, the staged query's cinv; DPOL: the column sum
    if constexpr (POLICY) {
        ci_b = pol.cinv + ((long)b * H + h) * n;
        pol_key = kok ? pol.policy[(long)b * n + k0 + l31] : 0.f;
    }
    [[maybe_unused]] float w_key = 0.f;                   // KEYW: this lane's key's weight
    if constexpr (KEYW) w_key = kok ? pol.policy[(long)b * n + k0 + l31] : 0.f;
    auto fetch = [&](int row0) {
        stage_rows(qb, ld, row0, n, tid, qr);
        stage_rows(dob, ldo, row0, n, tid, dr);
        const int qi = row0 + (tid & 31), qc = min(qi, n - 1);
        const float l0 = lse_b[qc], d0 = dl_b[qc];
        lr = qi < n ? l0 * L2E : INFINITY;      // queries past the sequence: p = 2^(s log2 e - inf) = 0
        dlr = qi < n ? d0 : 0.f;
        if constexpr (POLICY) { const float c0 = ci_b[qc]; cir = qi < n ? c0 : 0.f; }
    };
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        put_rows(Qs, tid, qr, 1.0f);
        put_rows(Ds, tid, dr, 1.0f);
        put_rows_t(Qt, tid, qr);
        put_rows_t(Dt, tid, dr);
        if (tid < 32) { lse_s[tid] = lr; dl_s[tid] = dlr; if (POLICY) ci_s[tid] = cir; }
        __syncthreads();
        fetch(min(t + 1, ntiles - 1) * 32);
        if (!active) continue;
        f32x16 s = mma_rows(Qs, kf, l31, half);          // S[query = row(r, half)][key = l31], scaled
        f32x16 dp = mma_rows(Ds, vf, l31, half);         // dP[query][key] = sum_d dO[query][d] V[key][d]
        if constexpr (POLICY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = mfma32_row(r, half);
                const bool diag = t * 32 == k0 && qi == l31;      // a wave's 32 keys start at a multiple of 32: one query tile holds the diagonal
                float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_s[qi]));      // P~; queries past the sequence: 0
                const float g = dp[r] - dl_s[qi];
                if (DPOL) dpol_acc += diag ? 0.f : p * g;      // dL/dmk_ij, before the mask multiplies it
                p *= diag ? 1.f : pol_key;
                s[r] = p + ci_s[qi];                           // dV sees the eps/n term of every key, masked or not
                dp[r] = p * g;
            }
        } else
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = mfma32_row(r, half);
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], L2E, -lse_s[qi]));
            if constexpr (KEYW) p *= w_key;              // before p feeds dV and dS
            s[r] = p;
            dp[r] = p * (dp[r] - dl_s[qi]);
        }
        bf16x8 pf[2], dsf[2];
        pack2(s, pf);
        pack2(dp, dsf);
        mma_t(Dt, pf, l31, half, dv);                    // dV^T[d][key] += sum_query dO[query][d] P[query][key]
        mma_t(Qt, dsf, l31, half, dk);                   // dK^T[d][key] += sum_query Q[query][d] dS[query][key]
    }
    if constexpr (DPOL) {
        if (active) {
            dpol_acc += __shfl_xor(dpol_acc, 32, 64);      // the other half-wave's 16 rows of every tile (commutative: both halves hold the same bits)
            if (half == 0 && kok) pol.dpol_part[((long)b * H + h) * n + k0 + l31] = dpol_acc;
        }
    }
    if constexpr (ONE_KEY) {      // as in the dQ kernel; dV = P^T dO is untouched
        if (n == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; }
        }
    }
    if (active && kok) {
        const long row = ((VARLEN ? (long)row_base : (long)b * n) + k0 + l31) * ld + h * DH;
        store_t(dk, dqkv, dqkv16, row + (long)H * DH, half, scale);
        store_t(dv, dqkv, dqkv16, row + 2L * H * DH, half, 1.0f);
    }
}

// dpolicy[b, j] = sum_h part[b, h, j], h ascending; column 0 (the CLS key, constant 1 in every policy) gets 0
__global__ __launch_bounds__(256) void attn_dpol_fold_bf16_kernel(const float* __restrict__ part, float* __restrict__ dpolicy, int B, int n, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * n) return;
    const long b = i / n, j = i - b * n;
    float s = 0.f;
    if (j > 0)
        for (int h = 0; h < H; ++h) s += part[(b * H + h) * n + j];
    dpolicy[i] = s;
}

}  // namespace

// D2S_ATTN_BF16_T64 [1]: 1 = the 64-key-tile forward with transposed V reads for long sequences (n >= 384, or where 64-key tiles pad no more
// than 32-key tiles), 2 = always, 0 = never (the 32-key-tile kernel).  Same-call A/B: n = 577 182.4 -> 179.3 us, config 5 +0.9 %; n = 197 36.8 ->
// 39.4 us (256 instead of 224 padded keys), hence the rule.
static bool attn_t64(int n) {
    static const int mode = [] { const char* e = getenv("D2S_ATTN_BF16_T64"); return e ? atoi(e) : 1; }();
    return mode >= 2 || (mode == 1 && (n >= 384 || (n + 63) / 64 * 64 == (n + 31) / 32 * 32));
}

// (qkv, qkv_is_bf16) of the C ABI -> f(qkv as const float* or as const __bf16*): every kernel is instantiated for both
template <typename F>
static int with_qkv_type(const void* qkv, int qkv_is_bf16, F f) {
    return qkv_is_bf16 ? f(static_cast<const __bf16*>(qkv)) : f(static_cast<const float*>(qkv));
}

// forward launch of the 32-key-tile kernel; n bounds the longest image: it sizes the grid and, when the CLS softmax row is wanted, its LDS
template <bool POLICY, bool VARLEN, bool KEYW, bool VLSE = false, typename QT>
static int attn_fwd_bf16_launch(const QT* qkv, float* out, void* out_bf16, float* lse, float* cls_row, int B, int n, int H, float scale,
                                hipStream_t stream, const float* policy = nullptr, float* cinv = nullptr, float eps = 0.f,
                                const int* cu = nullptr, int total = 0) {
    hipLaunchKernelGGL((attn_fwd_bf16_kernel<QT, POLICY, VARLEN, KEYW, VLSE>), dim3((n + 127) / 128, B * H), dim3(256),
                       cls_row ? (size_t)n * sizeof(float) : 0, stream, qkv, out, static_cast<__bf16*>(out_bf16), lse, cls_row, n, H, scale, policy,
                       cinv, eps, cu, total);
    return d2s_check_launch();
}

// the dense forward: 64-key tiles where attn_t64 says so
template <typename QT>
static int attn_fwd_bf16_dense(const QT* qkv, float* out, void* out_bf16, float* lse, float* cls_row, int B, int n, int H, float scale,
                               hipStream_t stream) {
    if (!attn_t64(n)) return attn_fwd_bf16_launch<false, false, false>(qkv, out, out_bf16, lse, cls_row, B, n, H, scale, stream);
    hipLaunchKernelGGL(attn_fwd_bf16_kernel64<QT>, dim3((n + 127) / 128, B * H), dim3(256), cls_row ? (size_t)n * sizeof(float) : 0, stream, qkv,
                       out, static_cast<__bf16*>(out_bf16), lse, cls_row, n, H, scale);
    return d2s_check_launch();
}

// backward launches: delta, dQ, dK/dV (with the policy's column sums when dpolicy is asked for) and then the fold over the heads
template <bool POLICY, typename QT>
static int attn_bwd_bf16_launch(const QT* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* dqkv_bf16,
                                float* delta_ws, int B, int n, int H, float scale, hipStream_t stream, const float* policy = nullptr,
                                const float* cinv = nullptr, float* dpolicy = nullptr, float* dpol_ws = nullptr) {
    const int rc = d2s_attn_delta(out, dout, delta_ws, B, n, H, stream);
    if (rc != D2S_OK) return rc;
    dim3 grid((n + 127) / 128, B * H), block(256);
    __bf16* dqkv16 = static_cast<__bf16*>(dqkv_bf16);
    if constexpr (!POLICY) {
        if (n == 1) {      // one key: the instantiations that write the exact zeros of dQ and dK (ONE_KEY)
            hipLaunchKernelGGL((attn_bwd_dq_bf16_kernel<QT, false, false, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, n, H,
                               scale, policy);
            hipLaunchKernelGGL((attn_bwd_dkv_bf16_kernel<QT, false, false, false, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16,
                               n, H, scale, AttnPolBwd{nullptr, nullptr, nullptr});
            return d2s_check_launch();
        }
    }
    hipLaunchKernelGGL((attn_bwd_dq_bf16_kernel<QT, POLICY>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, n, H, scale, policy);
    if (POLICY && dpolicy) {
        hipLaunchKernelGGL((attn_bwd_dkv_bf16_kernel<QT, POLICY, POLICY>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, n, H, scale,
                           AttnPolBwd{policy, cinv, dpol_ws});
        hipLaunchKernelGGL(attn_dpol_fold_bf16_kernel, dim3((unsigned)(((long)B * n + 255) / 256)), dim3(256), 0, stream, dpol_ws, dpolicy, B, n, H);
    } else {
        hipLaunchKernelGGL((attn_bwd_dkv_bf16_kernel<QT, POLICY, false>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, n, H, scale,
                           AttnPolBwd{policy, cinv, nullptr});
    }
    return d2s_check_launch();
}

// Backward of the same mode (same contract as d2s_attn_bwd_f32): dqkv [B,n,3,H,64] fully written; delta_ws: [B,H,n] floats of scratch.
template <typename QT>
static int attn_bwd_bf16_impl(const QT* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* dqkv_bf16,
                              float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !out || !dout || !lse || (!dqkv && !dqkv_bf16) || !delta_ws || B <= 0 || n <= 0 || H <= 0) return D2S_ERR_ARG;
    return attn_bwd_bf16_launch<false>(qkv, out, dout, lse, dqkv, dqkv_bf16, delta_ws, B, n, H, scale, stream);
}

// the ragged backward: d2s_attn_delta over the packed rows (the dense [B, H, n] layout with B = 1, n = total), then the VARLEN dQ and dK/dV;
// max_n sizes the grid as in the forward
template <typename QT>
static int attn_varlen_bwd_bf16_launch(const QT* qkv, const int* cu, const float* out, const float* dout, const float* lse, float* dqkv,
                                       void* dqkv_bf16, float* delta_ws, int B, int total, int max_n, int H, float scale, hipStream_t stream) {
    const int rc = d2s_attn_delta(out, dout, delta_ws, 1, total, H, stream);
    if (rc != D2S_OK) return rc;
    dim3 grid((max_n + 127) / 128, B * H), block(256);
    __bf16* dqkv16 = static_cast<__bf16*>(dqkv_bf16);
    const VarlenSeg seg{cu, total};
    hipLaunchKernelGGL((attn_bwd_dq_bf16_kernel<QT, false, true, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, max_n, H, scale,
                       seg);
    hipLaunchKernelGGL((attn_bwd_dkv_bf16_kernel<QT, false, false, true, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, max_n, H,
                       scale, seg);
    return d2s_check_launch();
}

// the key-weighted backward: the dense backward's three launches with the KEYW dQ and dK/dV
template <typename QT>
static int attn_keyw_bwd_bf16_launch(const QT* qkv, const float* key_w, const float* out, const float* dout, const float* lse, float* dqkv,
                                     void* dqkv_bf16, float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    const int rc = d2s_attn_delta(out, dout, delta_ws, B, n, H, stream);
    if (rc != D2S_OK) return rc;
    dim3 grid((n + 127) / 128, B * H), block(256);
    __bf16* dqkv16 = static_cast<__bf16*>(dqkv_bf16);
    hipLaunchKernelGGL((attn_bwd_dq_bf16_kernel<QT, false, false, false, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, dqkv16, n, H,
                       scale, key_w);
    hipLaunchKernelGGL((attn_bwd_dkv_bf16_kernel<QT, false, false, false, false, true>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv,
                       dqkv16, n, H, scale, AttnPolBwd{key_w, nullptr, nullptr});
    return d2s_check_launch();
}

extern "C" {

// Same contract as d2s_attn_fwd_f32; Q, K, V rounded to bf16 for the two matrix products (bf16 arithmetic mode).
int d2s_attn_fwd_bf16(const float* qkv, float* out, float* lse, float* cls_row, int B, int n, int H, float scale,
                      hipStream_t stream) {
    if (!qkv || !out || !lse || B <= 0 || n <= 0 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return attn_fwd_bf16_dense(qkv, out, nullptr, lse, cls_row, B, n, H, scale, stream);
}

// The same forward on the bf16 data path: qkv may be given in bf16 (qkv_is_bf16 != 0: the c_bf16 of the qkv GEMM, same [B,n,3,H,64]
// layout - the values this kernel would round to itself, so the results are identical), and a dense [B, n, H*64] bf16 copy of the
// output is written for the projection GEMM (its a_bf16); out may be NULL in forward-only passes that consume the bf16 form alone.
int d2s_attn_fwd_bf16_bf16out(const void* qkv, int qkv_is_bf16, float* out, void* out_bf16, float* lse, float* cls_row, int B, int n, int H,
                              float scale, hipStream_t stream) {
    if (!qkv || !out_bf16 || !lse || B <= 0 || n <= 0 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) { return attn_fwd_bf16_dense(q, out, out_bf16, lse, cls_row, B, n, H, scale, stream); });
}

int d2s_attn_bwd_bf16(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta_ws, int B, int n,
                      int H, float scale, hipStream_t stream) {
    return attn_bwd_bf16_impl(qkv, out, dout, lse, dqkv, nullptr, delta_ws, B, n, H, scale, stream);
}
// ... on the bf16 data path: qkv optionally in bf16 (as in the forward), and a bf16 copy of dqkv (same [B,n,3,H,64] layout): the a_bf16
// of the qkv Linear's input-gradient GEMM and the dy_bf16 of its weight gradient; dqkv may be NULL when only that form is consumed
int d2s_attn_bwd_bf16_bf16out(const void* qkv, int qkv_is_bf16, const float* out, const float* dout, const float* lse, float* dqkv,
                              void* dqkv_bf16, float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    if (!dqkv_bf16) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16,
                         [&](auto q) { return attn_bwd_bf16_impl(q, out, dout, lse, dqkv, dqkv_bf16, delta_ws, B, n, H, scale, stream); });
}

// Policy attention (d2s_attn_policy_fwd_f32's contract and outputs) on the bf16 matrix cores and the bf16 data path: qkv fp32 or bf16 as in
// d2s_attn_fwd_bf16_bf16out, out (fp32) and / or out_bf16 written - at least one; the backward needs out.  Always the 32-key-tile kernel.
// With an all-ones policy and eps = 0 the outputs are the bits of d2s_attn_fwd_bf16_bf16out where that entry uses the same kernel.
int d2s_attn_policy_fwd_bf16(const void* qkv, int qkv_is_bf16, const float* policy, float* out, void* out_bf16, float* lse, float* cinv,
                             float* cls_row, int B, int n, int H, float scale, float eps, hipStream_t stream) {
    if (!qkv || !policy || (!out && !out_bf16) || !lse || !cinv || B <= 0 || n <= 0 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_fwd_bf16_launch<true, false, false>(q, out, out_bf16, lse, cls_row, B, n, H, scale, stream, policy, cinv, eps);
    });
}

// Ragged packed batch on the bf16 matrix cores and the bf16 data path (d2s_attn_varlen_fwd_f32's contract; inference with a dynamic keep
// ratio): qkv [total,3,H,64] fp32 or bf16 as in d2s_attn_fwd_bf16_bf16out, image b = rows cu_seqlens[b] .. cu_seqlens[b+1]; out (fp32)
// [total,H*64] and / or out_bf16 written - at least one; cls_row (optional) [H,total]: softmax row of each image's first (CLS) token.
// max_n bounds the longest image (sizes the grid and the CLS row's LDS; any upper bound works).  Always the 32-key-tile kernel: one launch
// serves images of different lengths.  Forward only, no log-sum-exp.  With equal lengths the outputs are the bits of
// d2s_attn_fwd_bf16_bf16out where that entry uses the same kernel.
int d2s_attn_varlen_fwd_bf16(const void* qkv, int qkv_is_bf16, const int* cu_seqlens, float* out, void* out_bf16, float* cls_row, int B,
                             int total, int max_n, int H, float scale, hipStream_t stream) {
    if (!qkv || !cu_seqlens || (!out && !out_bf16) || B <= 0 || total <= 0 || max_n <= 0 || max_n > 8192 || H <= 0) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_fwd_bf16_launch<false, true, false>(q, out, out_bf16, nullptr, cls_row, B, max_n, H, scale, stream, nullptr, nullptr, 0.f,
                                                        cu_seqlens, total);
    });
}

// d2s_attn_varlen_fwd_bf16 that also keeps lse [H, total] (row cu_seqlens[b] + i of head h at h * total + cu_seqlens[b] + i, the layout of
// d2s_attn_varlen_fwd_lse_f32) for d2s_attn_varlen_bwd_bf16: an instantiation of its own beside the inference one, the same launch geometry,
// out / out_bf16 / cls_row bit for bit that entry's.
int d2s_attn_varlen_fwd_lse_bf16(const void* qkv, int qkv_is_bf16, const int* cu_seqlens, float* out, void* out_bf16, float* lse, float* cls_row,
                                 int B, int total, int max_n, int H, float scale, hipStream_t stream) {
    if (!qkv || !cu_seqlens || (!out && !out_bf16) || !lse || B <= 0 || total <= 0 || max_n <= 0 || max_n > 8192 || H <= 0) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_fwd_bf16_launch<false, true, false, true>(q, out, out_bf16, lse, cls_row, B, max_n, H, scale, stream, nullptr, nullptr, 0.f,
                                                              cu_seqlens, total);
    });
}

// Its backward (out, lse as that call wrote them; dout [total, H*64]): dqkv [total, 3, H, 64] and / or dqkv_bf16 written - at least one; fully
// when cu_seqlens covers [0, total), every element once, no atomics; delta_ws: [H, total] floats of scratch.  The dense backward's three
// launches with every image's rows and statistics taken from cu_seqlens: each image's rows are bit for bit d2s_attn_bwd_bf16_bf16out's on
// that image alone, in both forms.  64-bit offsets: no panel limit.
int d2s_attn_varlen_bwd_bf16(const void* qkv, int qkv_is_bf16, const int* cu_seqlens, const float* out, const float* dout, const float* lse,
                             float* dqkv, void* dqkv_bf16, float* delta_ws, int B, int total, int max_n, int H, float scale, hipStream_t stream) {
    if (!qkv || !cu_seqlens || !out || !dout || !lse || (!dqkv && !dqkv_bf16) || !delta_ws || B <= 0 || total <= 0 || max_n <= 0 ||
        max_n > 8192 || H <= 0)
        return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_varlen_bwd_bf16_launch(q, cu_seqlens, out, dout, lse, dqkv, dqkv_bf16, delta_ws, B, total, max_n, H, scale, stream);
    });
}

// Backward of d2s_attn_policy_fwd_bf16 (lse, cinv as that call wrote them; out its fp32 output): dqkv and / or dqkv_bf16 fully written -
// at least one.  dpolicy (optional) [B, n]: the gradient of the policy, column 0 = 0; it needs dpol_ws, [B, H, n] floats of scratch.  dqkv does not depend on
// whether dpolicy is asked for; no atomics, two launches are bit-identical.  The kernels address with 64-bit offsets: no panel limit.
int d2s_attn_policy_bwd_bf16(const void* qkv, int qkv_is_bf16, const float* policy, const float* out, const float* dout, const float* lse,
                             const float* cinv, float* dqkv, void* dqkv_bf16, float* delta_ws, float* dpolicy, float* dpol_ws, int B, int n, int H,
                             float scale, hipStream_t stream) {
    if (!qkv || !policy || !out || !dout || !lse || !cinv || (!dqkv && !dqkv_bf16) || !delta_ws || (dpolicy && !dpol_ws) || B <= 0 || n <= 0 ||
        H <= 0)
        return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_bwd_bf16_launch<true>(q, out, dout, lse, dqkv, dqkv_bf16, delta_ws, B, n, H, scale, stream, policy, cinv, dpolicy, dpol_ws);
    });
}

// Key-weighted attention (d2s_attn_keyw_fwd_f32's definition; token merging at inference) on the bf16 matrix cores and the bf16 data path:
// qkv fp32 or bf16 as in d2s_attn_fwd_bf16_bf16out, key_w [B, n] fp32 (>= 1), out (fp32) and / or out_bf16 written - at least one; lse
// [B, H, n] = log of the weighted denominator.  No CLS row.  Always the 32-key-tile kernel, d2s_attn_policy_fwd_bf16's grid.  With unit
// weights the outputs are the bits of d2s_attn_fwd_bf16_bf16out where that entry uses the same kernel.  2 <= n <= 8192.
int d2s_attn_keyw_fwd_bf16(const void* qkv, int qkv_is_bf16, const float* key_w, float* out, void* out_bf16, float* lse, int B, int n, int H,
                           float scale, hipStream_t stream) {
    if (!qkv || !key_w || (!out && !out_bf16) || !lse || B <= 0 || n < 2 || n > 8192 || H <= 0) return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_fwd_bf16_launch<false, false, true>(q, out, out_bf16, lse, nullptr, B, n, H, scale, stream, key_w);
    });
}

// Backward of d2s_attn_keyw_fwd_bf16 (out its fp32 output, lse as it wrote it - the log of the weighted denominator; dout [B, n, H*64]):
// dqkv (fp32) and / or dqkv_bf16, both [B, n, 3, H, 64], at least one, fully written; delta_ws: [B, H, n] floats of scratch.  The three
// launches of d2s_attn_bwd_bf16_bf16out with P_ij = w_j exp(S_ij - lse_i); the weights get no gradient.  With unit weights and the plain
// forward's out and lse: that entry's bits.  No atomics, two launches are bit-identical.  2 <= n <= 8192.
int d2s_attn_keyw_bwd_bf16(const void* qkv, int qkv_is_bf16, const float* key_w, const float* out, const float* dout, const float* lse,
                           float* dqkv, void* dqkv_bf16, float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !key_w || !out || !dout || !lse || (!dqkv && !dqkv_bf16) || !delta_ws || B <= 0 || n < 2 || n > 8192 || H <= 0)
        return D2S_ERR_ARG;
    return with_qkv_type(qkv, qkv_is_bf16, [&](auto q) {
        return attn_keyw_bwd_bf16_launch(q, key_w, out, dout, lse, dqkv, dqkv_bf16, delta_ws, B, n, H, scale, stream);
    });
}

}  // extern "C"
