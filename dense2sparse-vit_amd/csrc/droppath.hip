// Stochastic depth (DropPath, vit_models/deit.py:69-77): per-sample Bernoulli(keep) draws for both residual branches of every block,
// as ONE table per step, and the row scaling that the backward pass (and the stand-alone module) applies.
//
// The forward never runs a kernel of its own: the proj and fc2 GEMMs scale their branch by the table row in their epilogue
// (gemm_common.h, EPI_BIAS_RESID_ROWSCALE).  The backward scales the gradient entering a branch once, into the block's scratch
// (8 bytes per element and branch), and the scaled copy feeds that branch's weight-gradient and input-gradient GEMMs.
#include "d2s_common.h"

namespace {

// table[r][b] = floor(keep_r + u(seed, r, b)) / keep_r with keep_r = 1 - rates[r]: 0 or 1 / keep_r.  One thread per entry; the draw is
// Philox4x32-10 with key = seed and counter = (b, r, 0, 0), so an entry depends on (seed, rates[r], r, b) only - not on R, B or the launch.
__global__ __launch_bounds__(256) void drop_path_scales_kernel(const float* __restrict__ rates, float* __restrict__ table, int R, int B,
                                                               unsigned long long seed) {
    const int b = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (b >= B) return;
    const float rate = rates[r];
    float s = 1.0f;
    if (rate > 0.f) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)r, 0u, 0u};
        uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
        for (int i = 0; i < 10; ++i) philox_round(c, k);
        const float keep = 1.0f - rate;
        const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);       // [0, 1)
        s = fminf(floorf(keep + u), 1.0f) / keep;                        // keep + u can round up to 2 when keep is 1 ulp below 1
    }
    table[(long)r * B + b] = s;
}

// out[m][:] = rowscale[m / rows_per_group] * g[m][:]: a wave per row, 16-byte accesses, the scale loaded once per row
__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ g, const float* __restrict__ rowscale,
                                                         float* __restrict__ out, long M, int D, int rows_per_group) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const float s = rowscale[m / rows_per_group];
    const f32x4* src = reinterpret_cast<const f32x4*>(g + m * D);
    f32x4* dst = reinterpret_cast<f32x4*>(out + m * D);
    for (int i = lane; i < D / 4; i += 64) {
        f32x4 v = src[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= s;
        dst[i] = v;
    }
}

// the same for a feature count or a base address that rules the 16-byte form out: a thread per element
__global__ __launch_bounds__(256) void scale_rows_scalar_kernel(const float* __restrict__ g, const float* __restrict__ rowscale,
                                                                float* __restrict__ out, long total, long group_elems) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = g[i] * rowscale[i / group_elems];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

// table [R][B] fp32 from rates [R] (device, 0 <= rate < 1) and a seed; row 2i is block i's attention branch, row 2i + 1 its MLP branch.
// A row whose rate is 0 holds exactly 1.0f.
int d2s_drop_path_scales(const float* rates, float* table, int R, int B, unsigned long long seed, hipStream_t stream) {
    if (!rates || !table || R <= 0 || B <= 0 || R > 65535) return D2S_ERR_ARG;
    hipLaunchKernelGGL(drop_path_scales_kernel, dim3((B + 255) / 256, R), dim3(256), 0, stream, rates, table, R, B, seed);
    return d2s_check_launch();
}

// out [M][D] = rowscale[m / rows_per_group] * g [M][D] (dense rows; out may alias g).  rowscale holds ceil(M / rows_per_group) floats.
int d2s_scale_rows(const float* g, const float* rowscale, float* out, long M, int D, int rows_per_group, hipStream_t stream) {
    if (!g || !rowscale || !out || M <= 0 || D <= 0 || rows_per_group <= 0) return D2S_ERR_ARG;
    if (D % 4 == 0 && al16(g) && al16(out)) {
        const long blocks = (M + 3) / 4;
        if (blocks > 0x7fffffffL) return D2S_ERR_ARG;
        hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, rowscale, out, M, D, rows_per_group);
    } else {
        const long total = M * D, blocks = (total + 255) / 256;
        if (blocks > 0x7fffffffL) return D2S_ERR_ARG;
        hipLaunchKernelGGL(scale_rows_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, rowscale, out, total,
                           (long)rows_per_group * D);
    }
    return d2s_check_launch();
}

// DropPath.forward on a [B, inner] tensor with the draws given: out[b][:] = s[b] * x[b][:] (its own backward with the gradient as x).
// Runs as d2s_scale_rows over [B * inner / d][d] with d the largest power of two <= 1024 that divides inner.
int d2s_drop_path_fwd(const float* x, const float* s, float* out, int B, long inner, hipStream_t stream) {
    if (!x || !s || !out || B <= 0 || inner <= 0) return D2S_ERR_ARG;
    long d = 1;
    while (d < 1024 && inner % (d * 2) == 0) d *= 2;
    if (inner / d > 0x7fffffffL) return D2S_ERR_ARG;
    return d2s_scale_rows(x, s, out, (long)B * (inner / d), (int)d, (int)(inner / d), stream);
}

}  // extern "C"
