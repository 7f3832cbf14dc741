// Token Merging at inference (ToMe, Bolya et al. 2023; DESIGN.md section 22 - the build's own definition, the reference has no ToMe):
// every block removes r tokens by merging them into their most similar partner instead of dropping them.
//
//   metric     m_t = (sum_h K[b,t,h,:]) / H  (h ascending), divided by its L2 norm  (a zero row is NOT special-cased: 0/0 = NaN, every
//              comparison with its scores is false, so as an A row it gets node_max = -inf / node_idx = 0 and as a B row it is never chosen)
//   sets       A = even token indices (CLS = A row 0), T_a = ceil(n/2);  B = odd indices, T_b = floor(n/2)
//   match      score[i][j] = sum_d m_a(i)[d] m_b(j)[d], one fma chain d = 0..63 for every pair;  node_max[i] = max_j score, node_idx[i] =
//              the lowest j attaining it;  CLS: node_max = -inf, node_idx = 0 and never a source
//   sources    the r A rows with the largest node_max, d2s_select_topk's rule (value descending, equal values lowest index first)
//   plan       unm_idx [B, T_a - r] ascending (CLS first), src_idx [B, r] ascending, dst_idx [B, r] = node_idx[src_idx]; all set-relative
//   merge      output rows: the unmerged A rows in unm_idx order, then every B row in order.  B row j with sources becomes
//              (s_j x_j + sum s_src x_src) / (s_j + sum s_src), sources in ascending src_idx order after the row itself; size_out is the
//              denominator.  A row without sources (unmerged A, untouched B) is copied bit for bit.
//
//   backward   (training through the merge; the plan and the sizes are constants, the match reads K under no gradient)  the merge is linear
//              in x, so every INPUT row's gradient is one output row's, scaled: a merged row (a source, or a B row with sources) gets
//              (size_t / size_out_row) dy_row, every other row its output row's gradient bit for bit.  On the bf16 data path
//              (d2s_tome_merge_bwd_bf16out) the same pass also stores every row in bf16, the fp32 value rounded once, for the GEMMs
//              that read the gradient behind the merge.
//
// No atomics, no memset, no scratch, nothing read back by the host: deterministic and legal inside a captured step.
//
// The match also reads a bf16 qkv (the qkv GEMM's c_bf16 on the bf16 data path): the kernel is a template on the element type, the bf16
// load converts each value to fp32 (exact) and everything after the load is the same fp32 code in the same order, so
// d2s_tome_match_bf16(q16) is d2s_tome_match(float(q16)) bit for bit.
#include "d2s_common.h"
#include "d2s_hip_ext.h"
#include "d2s_hip_tome_train_bf16.h"
#include <type_traits>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int DH = 64;
constexpr int MPITCH = 68;        // floats per staged B row: 16-B aligned, a wave's 64 row writes spread over 16 bank slots instead of one
constexpr int TOME_MAX_N = 896;   // (448 * 68 + 3 * 448) floats = 124.3 KiB of dynamic LDS (attnsel.hip runs with 128 KiB)

// normalised metric of one token, computed by ONE thread in a fixed order (so equal K rows give equal bits wherever they sit)
// (from a bf16 row: 8 values per 16-byte access, each widened to fp32 - exact - and added in the same order, h ascending, d in place)
template <typename T>
__device__ __forceinline__ void metric_row(const T* __restrict__ krow, int H, float (&m)[DH]) {
#pragma unroll
    for (int d = 0; d < DH; ++d) m[d] = 0.f;
    for (int h = 0; h < H; ++h) {
        if constexpr (sizeof(T) == 4) {
            const f32x4* p = reinterpret_cast<const f32x4*>(krow + h * DH);
#pragma unroll
            for (int q = 0; q < DH / 4; ++q) {
                const f32x4 v = p[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) m[4 * q + j] += v[j];
            }
        } else {
            const bf16x8* p = reinterpret_cast<const bf16x8*>(krow + h * DH);
#pragma unroll
            for (int q = 0; q < DH / 8; ++q) {
                const bf16x8 v = p[q];
#pragma unroll
                for (int j = 0; j < 8; ++j) m[8 * q + j] += (float)v[j];
            }
        }
    }
    const float fh = (float)H;
    float ss = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        m[d] = m[d] / fh;
        ss = fmaf(m[d], m[d], ss);
    }
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int d = 0; d < DH; ++d) m[d] = m[d] / nrm;
}

template <typename T>
__global__ __launch_bounds__(256) void tome_match_kernel(const T* __restrict__ qkv, int n, int H, int r, float* __restrict__ node_max,
                                                         int* __restrict__ node_idx, int* __restrict__ unm_idx, int* __restrict__ src_idx,
                                                         int* __restrict__ dst_idx) {
    extern __shared__ __attribute__((aligned(16))) float sh[];   // [T_b][MPITCH] metric of set B, [T_a] node_max, [T_a] node_idx, [T_a] source flags
    __shared__ int wave_tot[4];
    const int Ta = (n + 1) >> 1, Tb = n >> 1;
    float* mb = sh;
    float* vmax = sh + Tb * MPITCH;
    int* vidx = reinterpret_cast<int*>(vmax + Ta);
    int* flag = vidx + Ta;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long ld = 3L * H * DH;
    const T* kb = qkv + (long)blockIdx.x * n * ld + (long)H * DH;     // K of token 0, head 0
    float a[DH];
    for (int j = tid; j < Tb; j += 256) {
        metric_row(kb + (long)(2 * j + 1) * ld, H, a);
#pragma unroll
        for (int q = 0; q < DH / 4; ++q) *reinterpret_cast<f32x4*>(&mb[j * MPITCH + 4 * q]) = f32x4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
    }
    __syncthreads();
    float* nm = node_max + (long)blockIdx.x * Ta;
    int* ni = node_idx + (long)blockIdx.x * Ta;
    for (int i = tid; i < Ta; i += 256) {      // the A row stays in registers; every lane reads the same B row: an LDS broadcast
        float best = -INFINITY;
        int arg = 0;
        if (i > 0) {
            metric_row(kb + (long)(2 * i) * ld, H, a);
            for (int j = 0; j < Tb; ++j) {
                const float* row = &mb[j * MPITCH];
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < DH / 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s = fmaf(a[4 * q + e], v[e], s);
                }
                if (s > best) { best = s; arg = j; }
            }
        }
        vmax[i] = best;
        vidx[i] = arg;
        nm[i] = best;
        ni[i] = arg;
    }
    __syncthreads();
    // rank by counting among the non-CLS rows; CLS (row 0) is never a source, whatever the values
    for (int i = tid; i < Ta; i += 256) {
        int f = 0;
        if (r > 0 && i > 0) {
            const float v = vmax[i];
            int cnt = 0;
            for (int j = 1; j < Ta; ++j) {
                const float u = vmax[j];
                cnt += (u > v) || (u == v && j < i);
            }
            f = cnt < r;
        }
        flag[i] = f;
    }
    __syncthreads();
    int* um = unm_idx + (long)blockIdx.x * (Ta - r);
    int* so = src_idx + (long)blockIdx.x * r;
    int* ds = dst_idx + (long)blockIdx.x * r;
    int base = 0;  // number of sources among indices below the current 256-chunk
    for (int c0 = 0; c0 < Ta; c0 += 256) {
        const int i = c0 + tid;
        const int f = (i < Ta) ? flag[i] : 0;
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wave_tot[w];
        const int pos = base + woff + before;
        if (i < Ta) {
            if (f) { if (pos < r) { so[pos] = i; ds[pos] = vidx[i]; } }
            else if (i - pos < Ta - r) um[i - pos] = i;
        }
        base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
}

// one wave per output row, 16-byte accesses; a destination row finds its sources by scanning dst_idx with ballots, in ascending order
__global__ __launch_bounds__(256) void tome_merge_kernel(const float* __restrict__ x, const float* __restrict__ size,
                                                         const int* __restrict__ unm_idx, const int* __restrict__ src_idx,
                                                         const int* __restrict__ dst_idx, long rows_out, int n, int D, int r,
                                                         float* __restrict__ x_out, float* __restrict__ size_out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_out) return;          // wave-uniform
    const int Ta = (n + 1) >> 1, no = n - r, na = Ta - r;
    const long b = row / no;
    const int o = (int)(row - b * no);
    const float* xb = x + b * n * (long)D;
    const float* sb = size ? size + b * n : nullptr;
    const int* srcs = src_idx + b * r;
    const int* dsts = dst_idx + b * r;
    const int D4 = D >> 2;
    f32x4* yo = reinterpret_cast<f32x4*>(x_out + row * D);
    int t, j = -1;                        // t: the input token this output row starts from
    if (o < na) {
        const int u = unm_idx[b * na + o];
        t = 2 * min(max(u, 0), Ta - 1);   // a plan is trusted to be a plan, but never to index outside the image
    } else {
        j = o - na;
        t = 2 * j + 1;
    }
    const float s0 = sb ? sb[t] : 1.f;
    const f32x4* x0 = reinterpret_cast<const f32x4*>(xb + (long)t * D);
    float den = s0;
    const int trips = (D4 + 63) >> 6;     // wave-uniform: the ballots below need the whole wave in every trip
    for (int k = 0; k < trips; ++k) {
        const int c = k * 64 + lane;
        const bool live = c < D4;
        const f32x4 v0 = live ? x0[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 acc = v0 * s0;
        float d = s0;
        bool found = false;
        if (j >= 0) {
            for (int p0 = 0; p0 < r; p0 += 64) {
                const int p = p0 + lane;
                unsigned long long bal = __ballot(p < r && dsts[p] == j);
                while (bal) {
                    const int bit = __ffsll((long long)bal) - 1;
                    bal &= bal - 1;
                    const int st = 2 * min(max(srcs[p0 + bit], 0), Ta - 1);
                    const float ss = sb ? sb[st] : 1.f;
                    if (live) {
                        const f32x4 vs = reinterpret_cast<const f32x4*>(xb + (long)st * D)[c];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = fmaf(ss, vs[e], acc[e]);
                    }
                    d += ss;
                    found = true;
                }
            }
        }
        if (live) yo[c] = found ? acc / d : v0;     // a row nothing merges into is copied bit for bit
        den = d;
    }
    if (lane == 0) size_out[row] = den;
}

// position of `key` in the ascending list v[0..len) or -1; every lane of the wave searches for the same key and gets the same answer
__device__ __forceinline__ int find_ascending(const int* __restrict__ v, int len, int key) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < len && v[lo] == key) ? lo : -1;
}

// backward of tome_merge_kernel: one wave per INPUT row, 16-byte accesses, every dx row written exactly once.  The row's case is
// wave-uniform: a B row (odd token) scans dst_idx with ballots as the forward does, an A row (even token) looks itself up in src_idx and
// then in unm_idx (both ascending: binary search).  An A row in neither list (not a plan) gets zeros; every index taken from the plan
// is checked against the image before it is used.
// BF16OUT: the row is written a second time in bf16 (dx16: the fp32 value rounded once), for the GEMMs of the bf16 data path that read the
// gradient behind the merge; the pair of pointers takes the place of the last argument, the plain instantiation keeps its argument list.
struct MergeDx { float* dx; __bf16* dx16; };
typedef __bf16 bf16x4m __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void put4(MergeDx o, long row, int D, int c, const f32x4& v) {
    reinterpret_cast<f32x4*>(o.dx + row * D)[c] = v;
    bf16x4m hv;
#pragma unroll
    for (int j = 0; j < 4; ++j) hv[j] = (__bf16)v[j];
    reinterpret_cast<bf16x4m*>(o.dx16 + row * D)[c] = hv;
}
template <bool BF16OUT = false>
__global__ __launch_bounds__(256) void tome_merge_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ size,
                                                             const float* __restrict__ size_out, const int* __restrict__ unm_idx,
                                                             const int* __restrict__ src_idx, const int* __restrict__ dst_idx, long rows_in,
                                                             int n, int D, int r, std::conditional_t<BF16OUT, MergeDx, float* __restrict__> dx) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= rows_in) return;           // wave-uniform
    const int Ta = (n + 1) >> 1, Tb = n >> 1, no = n - r, na = Ta - r;
    const long b = row / n;
    const int t = (int)(row - b * n);
    const int* srcs = src_idx + b * r;
    const int* dsts = dst_idx + b * r;
    int o = -1;                           // the output row this input row's gradient comes from (-1: none)
    bool scaled = false;
    if (t & 1) {
        const int j = t >> 1;
        o = na + j;
        for (int p0 = 0; p0 < r; p0 += 64) {
            const int p = p0 + lane;
            if (__ballot(p < r && dsts[p] == j)) { scaled = true; break; }
        }
    } else {
        const int i = t >> 1;
        const int p = r > 0 ? find_ascending(srcs, r, i) : -1;
        if (p >= 0) {
            const int d = dsts[p];
            if (d >= 0 && d < Tb) { o = na + d; scaled = true; }
        } else {
            o = find_ascending(unm_idx + b * na, na, i);      // a position in [0, na) or -1
        }
    }
    const int D4 = D >> 2;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BF16OUT) {      // spelled apart: the plain instantiation keeps its statements and with them its instructions
        if (o < 0) {
            for (int c = lane; c < D4; c += 64) put4(dx, row, D, c, zero);
            return;
        }
        const f32x4* g = reinterpret_cast<const f32x4*>(dy + (b * no + o) * (long)D);
        if (!scaled) {
            for (int c = lane; c < D4; c += 64) put4(dx, row, D, c, g[c]);      // a copied row: no multiply, the bits of dy
            return;
        }
        const float w = (size ? size[b * n + t] : 1.f) / size_out[b * no + o];
        for (int c = lane; c < D4; c += 64) put4(dx, row, D, c, g[c] * w);
    } else {
        f32x4* xo = reinterpret_cast<f32x4*>(dx + row * D);
        if (o < 0) {
            for (int c = lane; c < D4; c += 64) xo[c] = zero;
            return;
        }
        const f32x4* g = reinterpret_cast<const f32x4*>(dy + (b * no + o) * (long)D);
        if (!scaled) {
            for (int c = lane; c < D4; c += 64) xo[c] = g[c];
            return;
        }
        const float w = (size ? size[b * n + t] : 1.f) / size_out[b * no + o];
        for (int c = lane; c < D4; c += 64) xo[c] = g[c] * w;
    }
}

}  // namespace

extern "C" {

// qkv [B,n,3,H,64] fp32 as the qkv GEMM writes it (K is read in place) -> node_max [B,T_a] fp32, node_idx [B,T_a], unm_idx [B,T_a-r],
// src_idx [B,r], dst_idx [B,r] int32, T_a = ceil(n/2).  2 <= n <= 896, H >= 1, 0 <= r <= (n-1)/2 (the caller clips r).
int d2s_tome_match(const float* qkv, int B, int n, int H, int r, float* node_max, int* node_idx, int* unm_idx, int* src_idx, int* dst_idx,
                   hipStream_t stream) {
    if (!qkv || !node_max || !node_idx || !unm_idx || B <= 0 || n < 2 || n > TOME_MAX_N || H <= 0 || r < 0 || r > (n - 1) / 2 ||
        (r > 0 && (!src_idx || !dst_idx)))
        return D2S_ERR_ARG;
    const int Ta = (n + 1) / 2, Tb = n / 2;
    static bool attr_set = false;       // n = 577 stages 80 KiB, above the runtime's default per-kernel limit of dynamic LDS (64 KiB)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tome_match_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (TOME_MAX_N / 2) * (MPITCH + 3) * (int)sizeof(float));
        attr_set = true;
    }
    hipLaunchKernelGGL(tome_match_kernel<float>, dim3(B), dim3(256), ((size_t)Tb * MPITCH + 3 * (size_t)Ta) * sizeof(float), stream, qkv, n, H, r,
                       node_max, node_idx, unm_idx, src_idx, dst_idx);
    return d2s_check_launch();
}

// The same match on a bf16 qkv [B,n,3,H,64] (the qkv GEMM's c_bf16 on the bf16 data path): d2s_tome_match on the widened tensor, bit for
// bit in all five outputs.  Its limits and refusals.  The raised dynamic-LDS limit is a property of the kernel function: this
// instantiation sets its own on its first call.
int d2s_tome_match_bf16(const void* qkv_bf16, int B, int n, int H, int r, float* node_max, int* node_idx, int* unm_idx, int* src_idx,
                        int* dst_idx, hipStream_t stream) {
    if (!qkv_bf16 || !node_max || !node_idx || !unm_idx || B <= 0 || n < 2 || n > TOME_MAX_N || H <= 0 || r < 0 || r > (n - 1) / 2 ||
        (r > 0 && (!src_idx || !dst_idx)))
        return D2S_ERR_ARG;
    const int Ta = (n + 1) / 2, Tb = n / 2;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tome_match_kernel<__bf16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (TOME_MAX_N / 2) * (MPITCH + 3) * (int)sizeof(float));
        attr_set = true;
    }
    hipLaunchKernelGGL(tome_match_kernel<__bf16>, dim3(B), dim3(256), ((size_t)Tb * MPITCH + 3 * (size_t)Ta) * sizeof(float), stream,
                       static_cast<const __bf16*>(qkv_bf16), n, H, r, node_max, node_idx, unm_idx, src_idx, dst_idx);
    return d2s_check_launch();
}

// x [B,n,D] fp32, size [B,n] fp32 or null (all ones), the plan of d2s_tome_match -> x_out [B,n-r,D], size_out [B,n-r].  D % 4 == 0.
int d2s_tome_merge(const float* x, const float* size, const int* unm_idx, const int* src_idx, const int* dst_idx, int B, int n, int D, int r,
                   float* x_out, float* size_out, hipStream_t stream) {
    if (!x || !unm_idx || !x_out || !size_out || B <= 0 || n < 2 || n > TOME_MAX_N || D <= 0 || (D & 3) || r < 0 || r > (n - 1) / 2 ||
        (r > 0 && (!src_idx || !dst_idx)))
        return D2S_ERR_ARG;
    const long rows = (long)B * (n - r);
    if ((rows + 3) / 4 > 0x7fffffffL) return D2S_ERR_ARG;
    hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, size, unm_idx, src_idx, dst_idx, rows, n,
                       D, r, x_out, size_out);
    return d2s_check_launch();
}

// Backward of d2s_tome_merge in x: dy [B,n-r,D], size [B,n] or null (all ones), size_out [B,n-r] as the forward wrote it, the forward's
// plan -> dx [B,n,D], every row written once (r = 0: the identity copy).  The sizes and the plan get no gradient.  d2s_tome_merge's limits.
int d2s_tome_merge_bwd(const float* dy, const float* size, const float* size_out, const int* unm_idx, const int* src_idx, const int* dst_idx,
                       int B, int n, int D, int r, float* dx, hipStream_t stream) {
    if (!dy || !size_out || !unm_idx || !dx || B <= 0 || n < 2 || n > TOME_MAX_N || D <= 0 || (D & 3) || r < 0 || r > (n - 1) / 2 ||
        (r > 0 && (!src_idx || !dst_idx)))
        return D2S_ERR_ARG;
    const long rows = (long)B * n;
    if ((rows + 3) / 4 > 0x7fffffffL) return D2S_ERR_ARG;
    hipLaunchKernelGGL(tome_merge_bwd_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, dy, size, size_out, unm_idx, src_idx,
                       dst_idx, rows, n, D, r, dx);
    return d2s_check_launch();
}

// d2s_tome_merge_bwd that also writes the bf16 form of every row (the bf16 data path behind a merge): dx [B,n,D] fp32 - that entry's bits -
// and dx_bf16 [B,n,D], the same values rounded once.  One pass, every row of both outputs written exactly once, no atomics; r = 0 is the
// copy plus its rounding.  d2s_tome_merge_bwd's limits and refusals, plus a null dx_bf16.
int d2s_tome_merge_bwd_bf16out(const float* dy, const float* size, const float* size_out, const int* unm_idx, const int* src_idx,
                               const int* dst_idx, int B, int n, int D, int r, float* dx, void* dx_bf16, hipStream_t stream) {
    if (!dy || !size_out || !unm_idx || !dx || !dx_bf16 || B <= 0 || n < 2 || n > TOME_MAX_N || D <= 0 || (D & 3) || r < 0 ||
        r > (n - 1) / 2 || (r > 0 && (!src_idx || !dst_idx)))
        return D2S_ERR_ARG;
    const long rows = (long)B * n;
    if ((rows + 3) / 4 > 0x7fffffffL) return D2S_ERR_ARG;
    hipLaunchKernelGGL(tome_merge_bwd_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, dy, size, size_out, unm_idx, src_idx,
                       dst_idx, rows, n, D, r, MergeDx{dx, static_cast<__bf16*>(dx_bf16)});
    return d2s_check_launch();
}

}  // extern "C"
