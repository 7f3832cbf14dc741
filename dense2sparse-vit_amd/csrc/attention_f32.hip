// Fused multi-head attention, fp32 on the f32-input MFMA (32x32x2), head dim 64 (every model on the path).
// Replaces Attention.forward's q@k^T -> softmax -> @v (vit_models/dynamic_vit.py:218-229) without materialising
// the [B,H,n,n] matrix, emits the CLS row of the softmax that the reference returns (:234) and that the teacher's
// rows feed into MaskLoss (losses.py:76-79), and provides the backward (dq, dk, dv) by recomputation from the
// saved log-sum-exp.
//
// qkv is the raw output of the qkv Linear: [B, n, 3, H, 64] (row stride 3*H*64); out / dout are [B, n, H*64].
//
// Orientation trick (no cross-lane traffic for P): forward and dQ compute S^T = K Q^T, so a lane owns ONE query
// (column) and 16 of the tile's 32 keys (rows) in its accumulator registers - the row softmax is an in-lane
// reduction plus one exchange between the half-waves, and the accumulator registers are, as they stand, the
// A operand of the following P V (resp. dS K) product.  dK/dV use the natural orientation S = Q K^T for the same
// reason (their sums run over queries).
//
// MFMA maps (d2s_common.h): lane l holds A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]; C reg r: row (r&3)+8(r>>2)+4(l>>5),
// col l&31.  The 64-long d reduction is walked as 32 steps; step s = 4t+j uses d = 8t + 4*half + j, so each lane
// fetches its operand as 8 float4 (t = 0..7).
#include "d2s_common.h"
#include "d2s_hip_ragged_train.h"

namespace {

#ifdef D2S_ATTN_STAMPS   // diagnostic build only (tools/attn_stamps.py): per-workgroup phase stamps in shader cycles + 100 MHz wall ticks
__device__ unsigned long long g_attn_stamps[16 * 8192];
#define ASTAMP(i) if (threadIdx.x == 0) { const int L_ = blockIdx.y * gridDim.x + blockIdx.x; if (L_ < 8192) g_attn_stamps[16 * L_ + (i)] = __builtin_amdgcn_s_memtime(); }
#define ASTAMPR(i) if (threadIdx.x == 0) { const int L_ = blockIdx.y * gridDim.x + blockIdx.x; if (L_ < 8192) g_attn_stamps[16 * L_ + (i)] = __builtin_amdgcn_s_memrealtime(); }
#else
#define ASTAMP(i)
#define ASTAMPR(i)
#endif

constexpr int DH = 64;
constexpr int PITCH = 68;  // floats; 16-B aligned rows, conflict-free ds_read_b128 for 16 distinct rows

__device__ __forceinline__ void load_rows_regs(const float* __restrict__ base, long ld, int row, int nrows, int half,
                                               float scale, f32x4 (&r)[8]) {
    // operand fragment of one token row for lane (row, half): r[t] = base[row][8t + 4half .. +3] * scale
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
// out[dt] += X^T-style product: A operand = accumulator-layout registers p[r], B operand = LDS tile row mfma32_row(r,half)
// `groups` (wave-uniform, 1..4): only tile rows < 8 * groups carry non-zero p (the last, partial tile of a sequence): registers
// 4g..4g+3 cover rows [8g, 8g + 8), so whole groups of MFMAs whose A operand is exactly zero are skipped (bit-identical result).
__device__ __forceinline__ void mma_reg_lds(const f32x16& p, const float* __restrict__ S, int l31, int half, f32x16 (&o)[2],
                                            int groups = 4) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g < groups) {
#pragma unroll
            for (int r = 4 * g; r < 4 * g + 4; ++r) {
                const float* row = &S[mfma32_row(r, half) * PITCH];
                o[0] = mfma32(p[r], row[l31], o[0]);
                o[1] = mfma32(p[r], row[32 + l31], o[1]);
            }
        }
    }
}

// Transposed form of the same product: o[dt][r] = O^T[d = 32 dt + row(r, half)][query = l31].  The LDS tile row supplies the A operand
// and the accumulator-layout registers the B operand, so the output COLUMN is the lane's own query: the running-maximum rescale and the
// final 1 / l of the forward are lane-local (no cross-lane broadcast of alpha).
__device__ __forceinline__ void mma_lds_reg_t(const f32x16& p, const float* __restrict__ S, int l31, int half, f32x16 (&o)[2],
                                              int groups = 4) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g < groups) {
#pragma unroll
            for (int r = 4 * g; r < 4 * g + 4; ++r) {
                const float* row = &S[mfma32_row(r, half) * PITCH];
                o[0] = mfma32(row[l31], p[r], o[0]);
                o[1] = mfma32(row[32 + l31], p[r], o[1]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
// POLICY: Attention.softmax_with_policy (vit_models/dynamic_vit.py:195-214) fused into the same pass:
//     mk_ij = policy[b,j] or (i == j);  e_ij = exp(S_ij - max_j S_ij) * mk_ij;  P_ij = (e_ij + eps/n) / (sum_j e_ij + eps)
// The running maximum is taken over ALL keys (masked ones included, as the reference does), masked keys add nothing to l or O, and the
// eps terms enter once at the end: O_i = (sum_j e_ij v_j + (eps/n) sum_j v_j) / (l_i + eps).  Saved for the backward: lse_i = m_i +
// log(l_i + eps) (so that e_ij / (l_i + eps) = exp(S_ij - lse_i) mk_ij) and cinv_i = (eps/n) / (l_i + eps).
// VARLEN: ragged packed batch (inference with a dynamic keep ratio, :935-949): image b owns rows cu[b] .. cu[b+1] of qkv / out, its
// lse / CLS row live at [h * total + cu[b] + i].
struct AttnFwdArgs {
    const float* qkv; float* out; float* lse; float* cls_row;
    const float* policy; float* cinv; const int* cu;
    int n, H; float scale, eps; int total;
};

// KEYW: per-key weights (token merging, tome.hip / DESIGN.md section 22: key j stands for key_w[b,j] patches).  softmax_j(S_ij + log w_j) is
// computed as e_ij w_j / sum_j e_ij w_j with e_ij = exp(S_ij - max_j S_ij): the weight multiplies the exponential, the running maximum stays
// the one over the raw scores (1 <= w <= n).  The weights travel in a.policy and are staged in pol_s; lse_i = m_i + log(sum_j e_ij w_j).
template <bool POLICY, bool VARLEN, bool KEYW = false>
__global__ __launch_bounds__(256, 3) void attn_fwd_kernel(AttnFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float Ks[32 * PITCH];
    __shared__ __attribute__((aligned(16))) float Vs[32 * PITCH];
    __shared__ float pol_s[32];
    __shared__ __attribute__((aligned(16))) float vred[POLICY ? 16 * 64 : 4];
    __shared__ float vsum_s[64];
    extern __shared__ __attribute__((aligned(16))) float cls_s[];  // [n] raw scaled scores of query 0 (block 0 only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int H = a.H;
    ASTAMP(0); ASTAMPR(8);
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH;
    const int row_base = VARLEN ? a.cu[b] : 0;
    const int n = VARLEN ? a.cu[b + 1] - row_base : a.n;
    if (VARLEN && bx * 128 >= n) return;                // block-uniform: this image has no queries in this tile
    const long tok0 = VARLEN ? (long)row_base : (long)b * n;       // first token row of the image
    const float* qb = a.qkv + tok0 * ld + h * DH;
    const float* kb = qb + (long)H * DH;
    const float* vb = kb + (long)H * DH;
    const float* polb = (POLICY || KEYW) ? a.policy + (long)b * n : nullptr;
    const float scale = a.scale;
    const int q0 = bx * 128 + wave * 32;
    const bool active = q0 < n;
    const bool want_cls = a.cls_row != nullptr && bx == 0 && wave == 0;
    const int qi = q0 + l31;

    f32x4 qreg[8];
    load_rows_regs(qb, ld, qi, n, half, scale, qreg);

    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 vacc = {0.f, 0.f, 0.f, 0.f};

    const int ntiles = (n + 31) / 32;
    f32x4 kr[2], vr[2];
    float pr = 0.f;
    tile_load(kb, ld, 0, n, tid, kr);
    tile_load(vb, ld, 0, n, tid, vr);
    if ((POLICY || KEYW) && tid < 32) pr = tid < n ? polb[tid] : 0.f;
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        tile_store(Ks, tid, kr);
        tile_store(Vs, tid, vr);
        if (KEYW && tid < 32) pol_s[tid] = pr;
        if (POLICY) {
            if (tid < 32) pol_s[tid] = pr;
            vacc += vr[0];      // column sums of V over every key (rows beyond n were loaded as zeros)
            vacc += vr[1];
        }
        __syncthreads();
        if (t == 0) { ASTAMP(1); }
        if (t == 1) { ASTAMP(2); }
        if (t == 2) { ASTAMP(3); }
        if (t + 1 < ntiles) {
            tile_load(kb, ld, (t + 1) * 32, n, tid, kr);
            tile_load(vb, ld, (t + 1) * 32, n, tid, vr);
            if ((POLICY || KEYW) && tid < 32) { const int kj = (t + 1) * 32 + tid; pr = kj < n ? polb[kj] : 0.f; }
        }
        if (!active) continue;
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        mma_lds_reg(Ks, l31, half, qreg, s);  // s[r] = S^T[key = row(r,half)][query = l31], already scaled
        const int kv0 = t * 32;
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (kv0 + mfma32_row(r, half) >= n) s[r] = -INFINITY;
            mt = fmaxf(mt, s[r]);
        }
        if (want_cls && l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kv0 + mfma32_row(r, half);
                if (key < n) cls_s[key] = s[r];
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __expf(s[r] - m_new);
            if (POLICY) {
                const int kr_ = mfma32_row(r, half);
                s[r] *= (kv0 + kr_ == qi) ? 1.f : pol_s[kr_];
            }
            if (KEYW) s[r] *= pol_s[mfma32_row(r, half)];
            rs += s[r];
        }
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        // O is kept transposed (O^T[d][query]): its column is this lane's own query, so the rescale is lane-local
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[0][r] *= alpha;
            o[1][r] *= alpha;
        }
        mma_lds_reg_t(s, Vs, l31, half, o, min(4, (n - kv0 + 7) >> 3));
    }
    ASTAMP(4);
    const float c = POLICY ? a.eps / (float)n : 0.f;
    if (POLICY) {   // fold the 16 per-thread partial column sums of every column quad (threads with equal tid & 15) -> vsum_s[64]
        *reinterpret_cast<f32x4*>(&vred[(tid >> 4) * 64 + (tid & 15) * 4]) = vacc;
        __syncthreads();
        if (tid < 64) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) t += vred[g * 64 + tid];
            vsum_s[tid] = t * c;
        }
        __syncthreads();
    }
    if (!active) return;
    const float inv_l = 1.0f / (POLICY ? l_run + a.eps : l_run);
    if (qi < n) {      // registers 4g .. 4g+3 of o[dt] hold d = 32 dt + 8 g + 4 half + 0..3 of this lane's query
        float* p = a.out + (tok0 + qi) * H * DH + h * DH;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float num = o[dt][4 * g + j];
                    if (POLICY) num += vsum_s[32 * dt + 8 * g + 4 * half + j];
                    v[j] = num * inv_l;
                }
                *reinterpret_cast<f32x4*>(p + 32 * dt + 8 * g + 4 * half) = v;
            }
    }
    const long stat0 = VARLEN ? (long)h * a.total + row_base : ((long)b * H + h) * n;
    if (half == 0 && qi < n) {
        if (a.lse) a.lse[stat0 + qi] = m_run + logf(POLICY ? l_run + a.eps : l_run);
        if (POLICY && a.cinv) a.cinv[stat0 + qi] = c * inv_l;
    }
    if (want_cls) {
        const float m0 = __shfl(m_run, 0, 64), il0 = __shfl(inv_l, 0, 64);
        float* cr = a.cls_row + stat0;
        // cls_s was written by lanes 0 and 32 of this wave only; same-wave LDS accesses are ordered
        for (int j = lane; j < n; j += 64) {
            float e = expf(cls_s[j] - m0);
            if (POLICY) e = e * (j == 0 ? 1.f : polb[j]) + c;
            cr[j] = e * il0;
        }
    }
    ASTAMP(5); ASTAMPR(9);
}

// delta[b,h,i] = sum_d dout[b,i,h,d] * out[b,i,h,d]
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                         float* __restrict__ delta, long rows, int n, int H) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long b = row / n, i = row - b * n;
    for (int h = 0; h < H; ++h) {
        const long e = row * H * DH + h * DH + lane;
        const float s = wave_sum(out[e] * dout[e]);
        if (lane == 0) delta[(b * H + h) * n + i] = s;
    }
}

// the tile fetch of the DPOL dK/dV and the VARLEN dQ instantiations: 32-bit element offsets from the (wave-uniform) panel bases - a head's
// panel spans n * ld < 2^32 elements (checked by the entries) - so that the loop-invariant per-thread addresses cost one register each, not two
__device__ __forceinline__ void tile_load_u32(const float* __restrict__ base, unsigned ld, int row0, int nrows, int tid, f32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = tid + i * 256, row = row0 + (f >> 4);
        const unsigned off = (unsigned)row * ld + (unsigned)((f & 15) * 4);
        r[i] = row < nrows ? *reinterpret_cast<const f32x4*>(base + off) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// VARLEN in the two backward kernels (training through a ragged packed batch): image b owns rows cu[b] .. cu[b+1] of
// qkv / dout / dqkv, its lse / delta live at [h * total + cu[b] + i] (what attn_fwd_kernel<false, true> writes), `n` arrives as max_n.
// The segment is clamped to [0, total) and its length to [0, max_n]: a bad cu is never dereferenced outside the buffers.  The dense
// instantiations are handed VarlenSeg{} and never read it.
struct VarlenSeg { const int* cu; int total; };
__device__ __forceinline__ int varlen_rows(VarlenSeg v, int b, int max_n, int& row_base) {
    const int r0 = min(max(v.cu[b], 0), v.total), r1 = min(max(v.cu[b + 1], r0), v.total);
    row_base = r0;
    return min(r1 - r0, max_n);
}

// ---------------------------------------------------------------------------------------------------------
// backward, dQ: one wave per 32 queries, loops over key tiles (same orientation as forward)
// ---------------------------------------------------------------------------------------------------------
// POLICY: dS_ij = exp(S_ij - lse_i) mk_ij (dP_ij - delta_i) with lse_i = m_i + log(l_i + eps); the eps/n term of P does not depend on
// S.  (The O(eps) gradient through the row maximum, which the reference's autograd carries because it does not detach the max, is
// left out: it is <= eps = 1e-6 relative.)
// KEYW (backward of attn_fwd_kernel<false, false, true>, training through token merging): P_ij = w_j exp(S_ij - lse_i) with lse_i = m_i +
// log sum_j e_ij w_j as that forward wrote it; the weights travel in `policy`, are staged per key tile in pol_s as the forward does, and
// multiply the exponential - every key, the diagonal included.  They are counts and get no gradient.
// VARLEN: the same tiles on image b's rows of a packed batch; a workgroup whose 128-row tile starts at or past the image's n returns
// before its first barrier (block-uniform).
template <bool POLICY, bool KEYW = false, bool VARLEN = false>
__global__ __launch_bounds__(256, 3) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ dqkv, int n, int H, float scale,
                                                          const float* __restrict__ policy, VarlenSeg varlen) {
    static_assert(!(KEYW && POLICY), "key weights travel in the policy's argument");
    static_assert(!(VARLEN && (POLICY || KEYW)), "the ragged form has neither a policy nor key weights");
    __shared__ __attribute__((aligned(16))) float Ks[32 * PITCH];
    __shared__ __attribute__((aligned(16))) float Vs[32 * PITCH];
    __shared__ float pol_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    int row_base = 0;
    if constexpr (VARLEN) {
        n = varlen_rows(varlen, b, n, row_base);
        if (bx * 128 >= n) return;                      // block-uniform: this image has no queries in this tile
    }
    // the dense offsets stay spelled where they are used, as they were: hoisting them into one tok0 / stat0 reorders the dense
    // instantiations' scalar address arithmetic (same results, other instructions)
    const long stat0v = VARLEN ? (long)h * varlen.total + row_base : 0;        // the image's first lse / delta entry
    const float* qb = qkv + (VARLEN ? (long)row_base : (long)b * n) * ld + h * DH;
    const float* kb = qb + (long)H * DH;
    const float* vb = kb + (long)H * DH;
    const float* dob = dout + (VARLEN ? (long)row_base : (long)b * n) * ldo + h * DH;
    const int q0 = bx * 128 + wave * 32;
    const bool active = q0 < n;

    f32x4 qreg[8], doreg[8];
    load_rows_regs(qb, ld, q0 + l31, n, half, scale, qreg);
    load_rows_regs(dob, ldo, q0 + l31, n, half, 1.0f, doreg);
    const bool qok = q0 + l31 < n;
    const float lse_i = qok ? lse[(VARLEN ? stat0v : ((long)b * H + h) * n) + q0 + l31] : INFINITY;
    const float dl_i = qok ? delta[(VARLEN ? stat0v : ((long)b * H + h) * n) + q0 + l31] : 0.f;

    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }

    const int ntiles = (n + 31) / 32;
    f32x4 kr[2], vr[2];
    float pr = 0.f;
    const float* polb = (POLICY || KEYW) ? policy + (long)b * n : nullptr;
    // VARLEN: 32-bit element offsets for the tile fetches, as in the DPOL instantiation (an image's panel spans max_n * ld < 2^32 elements,
    // checked by the entry) - the registers that frees keep this instantiation out of scratch, where the dense one spills 16 bytes
    if (VARLEN) {
        tile_load_u32(kb, (unsigned)ld, 0, n, tid, kr);
        tile_load_u32(vb, (unsigned)ld, 0, n, tid, vr);
    } else {
        tile_load(kb, ld, 0, n, tid, kr);
        tile_load(vb, ld, 0, n, tid, vr);
    }
    if ((POLICY || KEYW) && tid < 32) pr = tid < n ? polb[tid] : 0.f;
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        tile_store(Ks, tid, kr);
        tile_store(Vs, tid, vr);
        if ((POLICY || KEYW) && tid < 32) pol_s[tid] = pr;
        __syncthreads();
        if (t + 1 < ntiles) {
            if (VARLEN) {
                tile_load_u32(kb, (unsigned)ld, (t + 1) * 32, n, tid, kr);
                tile_load_u32(vb, (unsigned)ld, (t + 1) * 32, n, tid, vr);
            } else {
                tile_load(kb, ld, (t + 1) * 32, n, tid, kr);
                tile_load(vb, ld, (t + 1) * 32, n, tid, vr);
            }
            if ((POLICY || KEYW) && tid < 32) { const int kj = (t + 1) * 32 + tid; pr = kj < n ? polb[kj] : 0.f; }
        }
        if (!active) continue;
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        mma_lds_reg(Ks, l31, half, qreg, s);    // scaled scores^T
        mma_lds_reg(Vs, l31, half, doreg, dp);  // dP^T[key][query] = sum_d V[key][d] dO[query][d]
        const int kv0 = t * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr_ = mfma32_row(r, half);
            float p = (kv0 + kr_ < n) ? __expf(s[r] - lse_i) : 0.f;
            if (POLICY) p *= (kv0 + kr_ == q0 + l31) ? 1.f : pol_s[kr_];
            if (KEYW) p *= pol_s[kr_];
            s[r] = p * (dp[r] - dl_i);          // dS^T
        }
        mma_reg_lds(s, Ks, l31, half, dq, min(4, (n - kv0 + 7) >> 3));      // dQ[query][d] += sum_key dS^T[key][query] K[key][d]
    }
    if (!active) return;
    float* dqb = dqkv + (VARLEN ? (long)row_base : (long)b * n) * ld + h * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qi = q0 + mfma32_row(r, half);
        if (qi < n) {
            float* p = dqb + (long)qi * ld;
            p[l31] = dq[0][r] * scale;
            p[32 + l31] = dq[1][r] * scale;
        }
    }
}

__device__ __forceinline__ void dkv_fetch_next(const float* __restrict__ qb, const float* __restrict__ dob, const float* __restrict__ lse_b,
                                               const float* __restrict__ dl_b, const float* __restrict__ ci_b, unsigned ld, unsigned ldo,
                                               int t1, int n, int tid, f32x4 (&qr)[2], f32x4 (&dr)[2], float& lr, float& dlr, float& cir) {
    tile_load_u32(qb, ld, t1 * 32, n, tid, qr);
    tile_load_u32(dob, ldo, t1 * 32, n, tid, dr);
    if (tid < 32) {
        const unsigned qi = (unsigned)(t1 * 32 + tid);
        lr = qi < (unsigned)n ? lse_b[qi] : INFINITY;
        dlr = qi < (unsigned)n ? dl_b[qi] : 0.f;
        cir = qi < (unsigned)n ? ci_b[qi] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward, dK / dV: one wave per 32 keys, loops over query tiles (natural orientation S = Q K^T)
// ---------------------------------------------------------------------------------------------------------
// POLICY: P_ij = exp(S_ij - lse_i) mk_ij + cinv_i feeds dV (the eps/n term reaches every key, masked or not); dS as in the dQ kernel.
// DPOL: the gradient of the policy itself, for the DynamicViT baseline whose predictor learns through the mask of this softmax only.  With
// m_ij = p_j + (1 - p_j) [i == j]:  dL/dm_ij = exp(S_ij - lse_i) (dP_ij - delta_i) - the product below BEFORE the mask multiplies it - and
// dpolicy[b, j] = sum_h sum_{i != j} dL/dm_ij.  The lane owns key j and walks every query, so its column sum needs no atomics: 16 rows per
// tile in register order, tiles in ascending order, then the two half-waves (rows 4 half + ...) are added once.  Each wave of a workgroup
// owns 32 keys of its own, so nothing is reduced across waves.  A masked key (p_j = 0) has dS = 0 but a non-zero column sum (that is the
// straight-through estimator's signal) and the policy is real-valued here: nothing is skipped and 0/1 is not assumed.
// dpol_part [B, H, n]: per-head partials, folded over h in ascending order by attn_dpol_fold_kernel (no __restrict__ on it: with it this
// instantiation re-schedules).
// KEYW (backward of the key-weighted forward): P_ij = w_j exp(S_ij - lse_i), the weights in `policy` as in the dQ kernel.  The lane owns
// key j, so w_j is one register loaded once (pol_key's slot) and multiplies p before it feeds dV and dS; no diagonal exception.
// VARLEN: as in the dQ kernel.
template <bool POLICY, bool DPOL = false, bool KEYW = false, bool VARLEN = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           float* __restrict__ dqkv, int n, int H, float scale,
                                                           const float* __restrict__ policy, const float* __restrict__ cinv,
                                                           float* dpol_part, VarlenSeg varlen) {
    static_assert(!DPOL || POLICY, "the policy's gradient needs a policy");
    static_assert(!(KEYW && POLICY), "key weights travel in the policy's argument");
    static_assert(!(VARLEN && (POLICY || DPOL || KEYW)), "the ragged form has neither a policy nor key weights");
    __shared__ __attribute__((aligned(16))) float Qs[32 * PITCH];
    __shared__ __attribute__((aligned(16))) float Ds[32 * PITCH];
    __shared__ float lse_s[32], dl_s[32], ci_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    int bx, by;
    xcd_remap_2d(bx, by);      // all blocks of one head on one XCD (shared K / V / Q / dO panels stay in its L2)
    const int b = by / H, h = by % H;
    const long ld = 3L * H * DH, ldo = (long)H * DH;
    int row_base = 0;
    if constexpr (VARLEN) {
        n = varlen_rows(varlen, b, n, row_base);
        if (bx * 128 >= n) return;                      // block-uniform: this image has no keys in this tile
    }
    const long tok0 = VARLEN ? (long)row_base : (long)b * n;       // first token row of the image
    const long stat0 = VARLEN ? (long)h * varlen.total + row_base : ((long)b * H + h) * n;
    const float* qb = qkv + tok0 * ld + h * DH;
    const float* kb = qb + (long)H * DH;
    const float* vb = kb + (long)H * DH;
    const float* dob = dout + tok0 * ldo + h * DH;
    const float* lse_b = lse + stat0;
    const float* dl_b = delta + stat0;
    const int k0 = bx * 128 + wave * 32;
    const bool active = k0 < n;

    f32x4 kreg[8], vreg[8];
    load_rows_regs(kb, ld, k0 + l31, n, half, scale, kreg);  // scaled copy, used for the scores only
    load_rows_regs(vb, ld, k0 + l31, n, half, 1.0f, vreg);

    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }

    const int ntiles = (n + 31) / 32;
    f32x4 qr[2], dr[2];
    float lr = 0.f, dlr = 0.f, cir = 0.f;
    float dpol_acc = 0.f;
    const float* ci_b = POLICY ? cinv + ((long)b * H + h) * n : nullptr;
    const float pol_key = ((POLICY || KEYW) && k0 + l31 < n) ? policy[(long)b * n + k0 + l31] : 0.f;   // this lane's key
    tile_load(qb, ld, 0, n, tid, qr);
    tile_load(dob, ldo, 0, n, tid, dr);
    if (tid < 32) { lr = tid < n ? lse_b[tid] : INFINITY; dlr = tid < n ? dl_b[tid] : 0.f; if (POLICY) cir = tid < n ? ci_b[tid] : 0.f; }
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        tile_store(Qs, tid, qr);
        tile_store(Ds, tid, dr);
        if (tid < 32) { lse_s[tid] = lr; dl_s[tid] = dlr; if (POLICY) ci_s[tid] = cir; }
        __syncthreads();
        // the next tile's rows travel through registers while this tile is multiplied; DPOL has no registers to spare for that (one more
        // accumulator at 2 waves per SIMD) and fetches them after the products instead (dkv_fetch_next), the CU's other workgroup covering the wait
        if (!DPOL && t + 1 < ntiles) {
            tile_load(qb, ld, (t + 1) * 32, n, tid, qr);
            tile_load(dob, ldo, (t + 1) * 32, n, tid, dr);
            if (tid < 32) {
                const int qi = (t + 1) * 32 + tid;
                lr = qi < n ? lse_b[qi] : INFINITY;
                dlr = qi < n ? dl_b[qi] : 0.f;
                if (POLICY) cir = qi < n ? ci_b[qi] : 0.f;
            }
        }
        if (DPOL && !active && t + 1 < ntiles) dkv_fetch_next(qb, dob, lse_b, dl_b, ci_b, (unsigned)ld, (unsigned)ldo, t + 1, n, tid, qr, dr, lr, dlr, cir);
        if (!active) continue;
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        mma_lds_reg(Qs, l31, half, kreg, s);   // S[query = row(r,half)][key = l31], scaled
        mma_lds_reg(Ds, l31, half, vreg, dp);  // dP[query][key] = sum_d dO[query][d] V[key][d]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = mfma32_row(r, half);
            float p = __expf(s[r] - lse_s[qi]);  // rows beyond n carry lse = +inf -> p = 0
            if (DPOL) {      // w = dL/dm_ij; rows beyond n carry p = 0
                const bool diag = t * 32 + qi == k0 + l31;
                const float g = dp[r] - dl_s[qi];
                dpol_acc += diag ? 0.f : p * g;
                p *= diag ? 1.f : pol_key;
                s[r] = p + ci_s[qi];
                dp[r] = p * g;                             // the bits of the plain POLICY instantiation
                continue;
            }
            if (POLICY) p *= (t * 32 + qi == k0 + l31) ? 1.f : pol_key;
            if (KEYW) p *= pol_key;
            s[r] = POLICY ? p + ci_s[qi] : p;
            dp[r] = p * (dp[r] - dl_s[qi]);
        }
        const int qgroups = min(4, (n - t * 32 + 7) >> 3);          // query rows of this tile that exist
        mma_reg_lds(s, Ds, l31, half, dv, qgroups);     // dV[key][d] += sum_query P[query][key] dO[query][d]
        mma_reg_lds(dp, Qs, l31, half, dk, qgroups);    // dK[key][d] += sum_query dS[query][key] Q[query][d]
        if (DPOL && t + 1 < ntiles) dkv_fetch_next(qb, dob, lse_b, dl_b, ci_b, (unsigned)ld, (unsigned)ldo, t + 1, n, tid, qr, dr, lr, dlr, cir);
    }
    if (!active) return;
    // DPOL: the epilogue's lane coordinates are derived afresh from an opaque copy of the thread id, so that the loop does not carry them
    int l31e = l31, halfe = half, k0e = k0;
    if constexpr (DPOL) {
        int t2 = (int)threadIdx.x;
        asm volatile("" : "+v"(t2));
        l31e = t2 & 31; halfe = (t2 >> 5) & 1; k0e = bx * 128 + (t2 >> 6) * 32;
        dpol_acc += __shfl_xor(dpol_acc, 32, 64);      // the other half-wave's 16 rows of every tile (commutative: both halves hold the same bits)
        if (halfe == 0 && k0e + l31e < n) dpol_part[((long)b * H + h) * n + k0e + l31e] = dpol_acc;
    }
    float* dkb = dqkv + tok0 * ld + (long)H * DH + h * DH;
    float* dvb = dkb + (long)H * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ki = k0e + mfma32_row(r, halfe);
        if (ki < n) {
            float* pk = dkb + (long)ki * ld;
            float* pv = dvb + (long)ki * ld;
            pk[l31e] = dk[0][r] * scale;
            pk[32 + l31e] = dk[1][r] * scale;
            pv[l31e] = dv[0][r];
            pv[32 + l31e] = dv[1][r];
        }
    }
}

// dpolicy[b, j] = sum_h part[b, h, j], h ascending; column 0 (the CLS key, constant 1 in every policy) gets 0
__global__ __launch_bounds__(256) void attn_dpol_fold_kernel(const float* __restrict__ part, float* __restrict__ dpolicy, int B, int n, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * n) return;
    const long b = i / n, j = i - b * n;
    float s = 0.f;
    if (j > 0)
        for (int h = 0; h < H; ++h) s += part[(b * H + h) * n + j];
    dpolicy[i] = s;
}

}  // namespace

#ifdef D2S_ATTN_STAMPS
extern "C" int d2s_debug_read_attn_stamps(unsigned long long* host_out, int n_wg) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_attn_stamps), (size_t)n_wg * 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

// forward launch; n_max bounds the longest image: it sizes the grid and, when the CLS softmax row is wanted, that row's dynamic LDS
template <bool POLICY, bool VARLEN, bool KEYW = false>
static int attn_fwd_launch(const AttnFwdArgs& a, int B, int n_max, hipStream_t stream) {
    hipLaunchKernelGGL((attn_fwd_kernel<POLICY, VARLEN, KEYW>), dim3((n_max + 127) / 128, B * a.H), dim3(256),
                       a.cls_row ? (size_t)n_max * sizeof(float) : 0, stream, a);
    return d2s_check_launch();
}

// backward launches: delta, dQ, dK/dV and (DPOL) the fold of the policy's gradient over the heads.  `policy` carries the key weights with
// KEYW; with VARLEN n is max_n and delta_ws is [H, total]: the dense kernel's [B, H, n] layout with B = 1, n = total
template <bool POLICY, bool DPOL = false, bool KEYW = false, bool VARLEN = false>
static int attn_bwd_launch(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta_ws, int B, int n,
                           int H, float scale, hipStream_t stream, const float* policy = nullptr, const float* cinv = nullptr,
                           float* dpolicy = nullptr, float* dpol_ws = nullptr, VarlenSeg seg = VarlenSeg{nullptr, 0}) {
    const long rows = VARLEN ? (long)seg.total : (long)B * n;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, out, dout, delta_ws, rows,
                       VARLEN ? seg.total : n, H);
    dim3 grid((n + 127) / 128, B * H), block(256);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<POLICY, KEYW, VARLEN>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, n, H, scale, policy, seg);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<POLICY, DPOL, KEYW, VARLEN>), grid, block, 0, stream, qkv, dout, lse, delta_ws, dqkv, n, H, scale,
                       policy, cinv, dpol_ws, seg);
    if (DPOL)
        hipLaunchKernelGGL(attn_dpol_fold_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, dpol_ws, dpolicy, B, n, H);
    return d2s_check_launch();
}

// the two ragged forward entries: one instantiation, one launch geometry; lse is null for the entry that keeps none
static int attn_varlen_fwd(const float* qkv, const int* cu_seqlens, float* out, float* lse, float* cls_row, int B, int total, int max_n, int H,
                           float scale, hipStream_t stream) {
    if (!qkv || !cu_seqlens || !out || B <= 0 || total <= 0 || max_n <= 0 || max_n > 8192 || H <= 0) return D2S_ERR_ARG;
    return attn_fwd_launch<false, true>(AttnFwdArgs{qkv, out, lse, cls_row, nullptr, nullptr, cu_seqlens, 0, H, scale, 0.f, total}, B, max_n, stream);
}

extern "C" {

// qkv [B,n,3,H,64] -> out [B,n,H*64], lse [B,H,n]; cls_row [B,H,n] (softmax row of query 0) if non-null.
int d2s_attn_fwd_f32(const float* qkv, float* out, float* lse, float* cls_row, int B, int n, int H, float scale,
                     hipStream_t stream) {
    if (!qkv || !out || !lse || B <= 0 || n <= 0 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return attn_fwd_launch<false, false>(AttnFwdArgs{qkv, out, lse, cls_row, nullptr, nullptr, nullptr, n, H, scale, 0.f, 0}, B, n, stream);
}

// Attention with the keep policy of the dynamic-keep-ratio training path fused in (vit_models/dynamic_vit.py:195-214,216-236 with
// policy != None): policy [B,n] (1 = kept; entry 0 is the CLS token).  lse [B,H,n] = m + log(l + eps), cinv [B,H,n] = (eps/n)/(l + eps)
// are what the backward needs.
int d2s_attn_policy_fwd_f32(const float* qkv, const float* policy, float* out, float* lse, float* cinv, float* cls_row, int B, int n,
                            int H, float scale, float eps, hipStream_t stream) {
    if (!qkv || !policy || !out || !lse || !cinv || B <= 0 || n <= 0 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return attn_fwd_launch<true, false>(AttnFwdArgs{qkv, out, lse, cls_row, policy, cinv, nullptr, n, H, scale, eps, 0}, B, n, stream);
}

// Ragged packed batch (inference with a dynamic keep ratio, vit_models/dynamic_vit.py:935-949): qkv [total,3,H,64], image b = rows
// cu_seqlens[b] .. cu_seqlens[b+1]; out [total,H*64]; cls_row (optional) [H,total]: softmax row of each image's first (CLS) token.
// max_n bounds the longest image (sizes the grid; any upper bound works).  Forward only.
int d2s_attn_varlen_fwd_f32(const float* qkv, const int* cu_seqlens, float* out, float* cls_row, int B, int total, int max_n, int H,
                            float scale, hipStream_t stream) {
    return attn_varlen_fwd(qkv, cu_seqlens, out, nullptr, cls_row, B, total, max_n, H, scale, stream);
}

// d2s_attn_varlen_fwd_f32 that also keeps lse [H, total] (lse of row cu[b] + i of head h at h * total + cu[b] + i) for
// d2s_attn_varlen_bwd_f32: the same instantiation and launch geometry, out / cls_row bit for bit that entry's.
int d2s_attn_varlen_fwd_lse_f32(const float* qkv, const int* cu_seqlens, float* out, float* lse, float* cls_row, int B, int total, int max_n,
                                int H, float scale, hipStream_t stream) {
    if (!lse) return D2S_ERR_ARG;
    return attn_varlen_fwd(qkv, cu_seqlens, out, lse, cls_row, B, total, max_n, H, scale, stream);
}

// Backward of d2s_attn_varlen_fwd_lse_f32 (out, lse as that call wrote them): dqkv [total, 3*H*64] is fully written when cu_seqlens covers
// [0, total), every element once, no atomics; delta_ws: [H, total] floats of scratch.  d2s_attn_bwd_f32's three launches with the image's
// rows taken from cu_seqlens: each image's rows are bit for bit d2s_attn_bwd_f32's on that image alone.
int d2s_attn_varlen_bwd_f32(const float* qkv, const int* cu_seqlens, const float* out, const float* dout, const float* lse, float* dqkv,
                            float* delta_ws, int B, int total, int max_n, int H, float scale, hipStream_t stream) {
    if (!qkv || !cu_seqlens || !out || !dout || !lse || !dqkv || !delta_ws || B <= 0 || total <= 0 || max_n <= 0 || max_n > 8192 || H <= 0)
        return D2S_ERR_ARG;
    if ((long)max_n * 3 * H * 64 >= (1L << 32)) return D2S_ERR_ARG;      // tile_load_u32: one image's qkv panel must fit 32-bit element offsets
    return attn_bwd_launch<false, false, false, true>(qkv, out, dout, lse, dqkv, delta_ws, B, max_n, H, scale, stream, nullptr, nullptr, nullptr,
                                                      nullptr, VarlenSeg{cu_seqlens, total});
}

// Attention whose keys carry weights (token merging at inference): key_w [B,n], key j of image b counts key_w[b,j]
// times in every softmax row - out_i = sum_j w_j exp(S_ij) v_j / sum_j w_j exp(S_ij); lse [B,H,n] (nullable) = log of that denominator.
// With every weight 1.0 the output is bit for bit d2s_attn_fwd_f32's.  Its backward is d2s_attn_keyw_bwd_f32.
int d2s_attn_keyw_fwd_f32(const float* qkv, const float* key_w, float* out, float* lse, int B, int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !key_w || !out || B <= 0 || n < 2 || H <= 0 || n > 8192) return D2S_ERR_ARG;      // a merged sequence keeps CLS and a token
    return attn_fwd_launch<false, false, true>(AttnFwdArgs{qkv, out, lse, nullptr, key_w, nullptr, nullptr, n, H, scale, 0.f, 0}, B, n, stream);
}

// delta[b,h,i] = sum_d dout[b,i,h,d] * out[b,i,h,d]: the row term of the softmax backward, shared by the fp32 and bf16 backward kernels
int d2s_attn_delta(const float* out, const float* dout, float* delta, int B, int n, int H, hipStream_t stream) {
    if (!out || !dout || !delta || B <= 0 || n <= 0 || H <= 0) return D2S_ERR_ARG;
    const long rows = (long)B * n;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, out, dout, delta, rows, n, H);
    return d2s_check_launch();
}

// dqkv [B,n,3,H,64] is fully written.  delta_ws: [B,H,n] floats of scratch.
int d2s_attn_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* delta_ws, int B,
                     int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !out || !dout || !lse || !dqkv || !delta_ws || B <= 0 || n <= 0 || H <= 0) return D2S_ERR_ARG;
    return attn_bwd_launch<false>(qkv, out, dout, lse, dqkv, delta_ws, B, n, H, scale, stream);
}

// Backward of d2s_attn_keyw_fwd_f32 (training through token merging): lse as that call wrote it, P_ij = w_j
// exp(S_ij - lse_i), dV = P^T dO, dS = P * (dP - delta).  The weights are counts and get no gradient.  d2s_attn_bwd_f32's launches and
// geometry, the forward entry's limits; dqkv is fully written, and with every weight 1.0 it is bit for bit d2s_attn_bwd_f32's.
int d2s_attn_keyw_bwd_f32(const float* qkv, const float* key_w, const float* out, const float* dout, const float* lse, float* dqkv,
                          float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !key_w || !out || !dout || !lse || !dqkv || !delta_ws || B <= 0 || n < 2 || H <= 0 || n > 8192) return D2S_ERR_ARG;
    return attn_bwd_launch<false, false, true>(qkv, out, dout, lse, dqkv, delta_ws, B, n, H, scale, stream, key_w);
}

// Backward of d2s_attn_policy_fwd_f32 (lse, cinv as that call wrote them).
int d2s_attn_policy_bwd_f32(const float* qkv, const float* policy, const float* out, const float* dout, const float* lse,
                            const float* cinv, float* dqkv, float* delta_ws, int B, int n, int H, float scale, hipStream_t stream) {
    if (!qkv || !policy || !out || !dout || !lse || !cinv || !dqkv || !delta_ws || B <= 0 || n <= 0 || H <= 0) return D2S_ERR_ARG;
    return attn_bwd_launch<true>(qkv, out, dout, lse, dqkv, delta_ws, B, n, H, scale, stream, policy, cinv);
}

// d2s_attn_policy_bwd_f32 plus the gradient of the policy: dpolicy [B, n] is fully written (column 0 = 0), dpol_ws: [B, H, n] floats of
// scratch.  dqkv is bit for bit what d2s_attn_policy_bwd_f32 writes; no atomics, so two launches are bit-identical.
int d2s_attn_policy_bwd_dpol_f32(const float* qkv, const float* policy, const float* out, const float* dout, const float* lse,
                                 const float* cinv, float* dqkv, float* delta_ws, float* dpolicy, float* dpol_ws, int B, int n, int H,
                                 float scale, hipStream_t stream) {
    if (!qkv || !policy || !out || !dout || !lse || !cinv || !dqkv || !delta_ws || !dpolicy || !dpol_ws || B <= 0 || n <= 0 || H <= 0)
        return D2S_ERR_ARG;
    if ((long)n * 3 * H * 64 >= (1L << 32)) return D2S_ERR_ARG;      // tile_load_u32: one image's qkv panel must fit 32-bit element offsets
    return attn_bwd_launch<true, true>(qkv, out, dout, lse, dqkv, delta_ws, B, n, H, scale, stream, policy, cinv, dpolicy, dpol_ws);
}

}  // extern "C"
