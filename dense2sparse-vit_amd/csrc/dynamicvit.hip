// Decision and predictor kernels of the DynamicViT baseline (vit_models/default_dynamic_vit.py): Gumbel noise, the 2-way LogSoftmax +
// hard Gumbel keep decision with its straight-through backward (:321, :454), and the policy-weighted pooling of the predictor (:327-329).
// The LayerNorm, the four Linears and the GELUs around them are the library's existing LayerNorm / GEMM launches.
#include "d2s_common.h"

namespace {

// 32 random bits -> Gumbel(0, 1): g = -log(E), E = -log(u) ~ Exp(1), torch's own construction of F.gumbel_softmax's noise.  u takes the
// top 23 bits: (k + 0.5) 2^-23 with k < 2^23 is exact in fp32 (k + 0.5 needs 24 significant bits), so u lies in [2^-24, 1 - 2^-24],
// strictly inside (0, 1), and g in [-2.82, 16.64] is always finite.  (A 24-bit k would round 16777215.5 to 2^24: u = 1, E = 0, g = +inf.)
__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}

__global__ __launch_bounds__(256) void gumbel_from_bits_kernel(const uint32_t* __restrict__ bits, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gumbel_from_bits(bits[i]);
}

__global__ __launch_bounds__(256) void gumbel_noise_kernel(float* __restrict__ out, long n, unsigned long long seed) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;      // one Philox block = 4 outputs
    if (q * 4 >= n) return;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)((unsigned long long)q >> 32), 0u, 0u};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; ++r) philox_round(c, k);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q * 4 + j < n) out[q * 4 + j] = gumbel_from_bits(c[j]);
}

// z [M,2] raw logits -> logp = log_softmax(z); with a = logp_0 + g_0, c = logp_1 + g_1 (tau = 1):
// y0 = softmax(a, c)_0, hard = (a >= c) (argmax: the first index wins a tie), decision = hard * prev.
__global__ __launch_bounds__(256) void gumbel_keep_fwd_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                              const float* __restrict__ prev, float* __restrict__ logp,
                                                              float* __restrict__ y0, float* __restrict__ hard,
                                                              float* __restrict__ decision, long M) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float z0 = z[2 * i], z1 = z[2 * i + 1];
    const float m = fmaxf(z0, z1);
    const float lse = logf(expf(z0 - m) + expf(z1 - m));
    const float l0 = (z0 - m) - lse, l1 = (z1 - m) - lse;
    const float a = l0 + g[2 * i], c = l1 + g[2 * i + 1];
    const float mm = fmaxf(a, c);
    const float e0 = expf(a - mm), e1 = expf(c - mm);
    const float h = a >= c ? 1.f : 0.f;
    logp[2 * i] = l0;
    logp[2 * i + 1] = l1;
    y0[i] = e0 / (e0 + e1);
    hard[i] = h;
    decision[i] = h * prev[i];
}

// straight-through (F.gumbel_softmax(hard=True)): dlogp_0 = gd * prev * y0 (1 - y0), dlogp_1 = -dlogp_0, dprev = gd * hard.
// LogSoftmax backward: dz_k = dlogp_k - softmax_k * (dlogp_0 + dlogp_1), and that sum is exactly 0: dz = dlogp.
__global__ __launch_bounds__(256) void gumbel_keep_bwd_kernel(const float* __restrict__ gd, const float* __restrict__ prev,
                                                              const float* __restrict__ y0, const float* __restrict__ hard,
                                                              float* __restrict__ dz, float* __restrict__ dprev, long M) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float y = y0[i], gi = gd[i];
    const float d0 = gi * prev[i] * (y * (1.f - y));
    dz[2 * i] = d0;
    dz[2 * i + 1] = -d0;
    dprev[i] = gi * hard[i];
}

// Column sums over the tokens of image b for 64 columns of the upper half: wave w walks rows w, w + 4, ..., lane = column; the four
// partials meet in LDS and are added in wave order.  WEIGHTED: sum_j x[b, j, C/2 + c] p[b, j] and sum_j p[b, j].
template <bool WEIGHTED>
__device__ __forceinline__ float upper_colsum(const float* __restrict__ xb, const float* __restrict__ pb, int N, int C, int col, bool ok,
                                              float (&red)[4][64], float (&pred)[4], float& psum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc = 0.f, pacc = 0.f;
    for (int j = wave; j < N; j += 4) {
        const float p = WEIGHTED ? pb[j] : 1.f;
        if (ok) acc += xb[(long)j * C + C / 2 + col] * p;
        pacc += p;
    }
    red[wave][lane] = acc;
    if (lane == 0) pred[wave] = pacc;
    __syncthreads();
    psum = ((pred[0] + pred[1]) + pred[2]) + pred[3];
    return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// x [B,N,C], p [B,N] -> out [B,N,C]: out[:, :, :C/2] = x[:, :, :C/2]; out[b, j, C/2 + c] = glob[b, c] = sum_j x[b,j,C/2+c] p_j / sum_j p_j.
// grid (ceil(C/2 / 64), B).  psum [B] and glob [B, C/2] are kept for the backward.
__global__ __launch_bounds__(256) void policy_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ p, float* __restrict__ out,
                                                              float* __restrict__ psum_out, float* __restrict__ glob, int N, int C) {
    __shared__ float red[4][64];
    __shared__ float pred[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, half = C / 2;
    const int col = blockIdx.x * 64 + lane;
    const bool ok = col < half;
    const float* xb = x + (long)b * N * C;
    float psum;
    const float s = upper_colsum<true>(xb, p + (long)b * N, N, C, col, ok, red, pred, psum);
    const float gl = s / psum;
    if (!ok) return;
    if (wave == 0) {
        glob[(long)b * half + col] = gl;
        if (blockIdx.x == 0 && lane == 0) psum_out[b] = psum;
    }
    float* ob = out + (long)b * N * C;
    for (int j = wave; j < N; j += 4) {
        ob[(long)j * C + col] = xb[(long)j * C + col];
        ob[(long)j * C + half + col] = gl;
    }
}

// G[b, c] = sum_j gout[b, j, C/2 + c]
__global__ __launch_bounds__(256) void policy_pool_gsum_kernel(const float* __restrict__ gout, float* __restrict__ G, int N, int C) {
    __shared__ float red[4][64];
    __shared__ float pred[4];
    const int lane = threadIdx.x & 63, b = blockIdx.y, half = C / 2;
    const int col = blockIdx.x * 64 + lane;
    const bool ok = col < half;
    float unused;
    const float s = upper_colsum<false>(gout + (long)b * N * C, nullptr, N, C, col, ok, red, pred, unused);
    if (ok && threadIdx.x < 64) G[(long)b * half + col] = s;
}

// one wave per token row (b, j): dx[:C/2] = gout[:C/2]; dx[C/2 + c] = G_c p_j / psum; dp_j = (G . x_j - G . glob) / psum
__global__ __launch_bounds__(256) void policy_pool_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ x, const float* __restrict__ p,
                                                              const float* __restrict__ psum, const float* __restrict__ glob,
                                                              const float* __restrict__ G, float* __restrict__ dx, float* __restrict__ dp,
                                                              long rows, int N, int C) {
    const int lane = threadIdx.x & 63, half = C / 2;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long b = row / N;
    const float ps = psum[b], w = p[row] / ps;
    const float* Gb = G + b * half;
    const float* gb = glob + b * half;
    const float* xr = x + row * C;
    const float* gr = gout + row * C;
    float* dr = dx + row * C;
    float dot_x = 0.f, dot_g = 0.f;
    for (int c = lane; c < half; c += 64) {
        const float g = Gb[c];
        dot_x += g * xr[half + c];
        dot_g += g * gb[c];
        dr[c] = gr[c];
        dr[half + c] = g * w;
    }
    dot_x = wave_sum(dot_x);
    dot_g = wave_sum(dot_g);
    if (lane == 0) dp[row] = (dot_x - dot_g) / ps;
}

// Ratio term of the DynamicViT objective, one wave per image: diff[b] = mean_j d[b, j] - rho, loss_row[b] = diff[b]^2.  Lane l adds columns
// l, l + 64, ... in ascending order, then the wave's fixed butterfly: two launches give the same bits.
__global__ __launch_bounds__(256) void ratio_rows_fwd_kernel(const float* __restrict__ d, float rho, float* __restrict__ loss_row,
                                                             float* __restrict__ diff, int B, int N) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* db = d + (long)b * N;
    float acc = 0.f;
    for (int j = lane; j < N; j += 64) acc += db[j];
    acc = wave_sum(acc);
    if (lane == 0) {
        const float df = acc / (float)N - rho;
        diff[b] = df;
        loss_row[b] = df * df;
    }
}

// grad[b, j] = g[0] * scale * 2 diff[b] / N   (scale: the weight over stages and batch the caller folded in)
__global__ __launch_bounds__(256) void ratio_rows_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ g, float scale,
                                                             float* __restrict__ grad, long rows, int N) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    grad[i] = g[0] * scale * (2.f * diff[i / N] / (float)N);
}

}  // namespace

extern "C" {

// d [B,N] keep decisions -> loss_row [B] = (mean_j d - rho)^2, diff [B] = mean_j d - rho (kept for the backward)
int d2s_ratio_rows_fwd(const float* d, float rho, float* loss_row, float* diff, int B, int N, hipStream_t stream) {
    if (!d || !loss_row || !diff || B <= 0 || N <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(ratio_rows_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, d, rho, loss_row, diff, B, N);
    return d2s_check_launch();
}

// diff [B], g: device scalar (gradient of the summed loss) -> grad [B,N] = g * scale * 2 diff[b] / N
int d2s_ratio_rows_bwd(const float* diff, const float* g, float scale, float* grad, int B, int N, hipStream_t stream) {
    if (!diff || !g || !grad || B <= 0 || N <= 0) return D2S_ERR_ARG;
    const long rows = (long)B * N;
    hipLaunchKernelGGL(ratio_rows_bwd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, diff, g, scale, grad, rows, N);
    return d2s_check_launch();
}

// out[0..n) = Gumbel(0, 1) numbers of the stream `seed`
int d2s_gumbel_noise(float* out, long n, unsigned long long seed, hipStream_t stream) {
    if (!out || n <= 0) return D2S_ERR_ARG;
    const long blocks = ((n + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(gumbel_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, out, n, seed);
    return d2s_check_launch();
}

// out[i] = the Gumbel number d2s_gumbel_noise makes of the 32 random bits bits[i] (the conversion alone, for tests of its range)
int d2s_gumbel_from_bits(const unsigned* bits, float* out, long n, hipStream_t stream) {
    if (!bits || !out || n <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gumbel_from_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, bits, out, n);
    return d2s_check_launch();
}

// z, g [M,2], prev [M] -> logp [M,2], y0, hard, decision [M]
int d2s_gumbel_keep_fwd(const float* z, const float* g, const float* prev, float* logp, float* y0, float* hard, float* decision, long M,
                        hipStream_t stream) {
    if (!z || !g || !prev || !logp || !y0 || !hard || !decision || M <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gumbel_keep_fwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, z, g, prev, logp, y0, hard, decision, M);
    return d2s_check_launch();
}

// gd (gradient of decision), prev, y0, hard [M] -> dz [M,2] (gradient of the RAW logits), dprev [M]
int d2s_gumbel_keep_bwd(const float* gd, const float* prev, const float* y0, const float* hard, float* dz, float* dprev, long M,
                        hipStream_t stream) {
    if (!gd || !prev || !y0 || !hard || !dz || !dprev || M <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(gumbel_keep_bwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, gd, prev, y0, hard, dz, dprev, M);
    return d2s_check_launch();
}

// x [B,N,C] (C even), p [B,N] -> out [B,N,C], psum [B], glob [B,C/2]
int d2s_policy_pool_fwd(const float* x, const float* p, float* out, float* psum, float* glob, int B, int N, int C, hipStream_t stream) {
    if (!x || !p || !out || !psum || !glob || B <= 0 || N <= 0 || C <= 0 || (C & 1)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(policy_pool_fwd_kernel, dim3((C / 2 + 63) / 64, B), dim3(256), 0, stream, x, p, out, psum, glob, N, C);
    return d2s_check_launch();
}

// gout [B,N,C] -> dx [B,N,C], dp [B,N]; gsum_ws: [B, C/2] floats of scratch
int d2s_policy_pool_bwd(const float* gout, const float* x, const float* p, const float* psum, const float* glob, float* dx, float* dp,
                        float* gsum_ws, int B, int N, int C, hipStream_t stream) {
    if (!gout || !x || !p || !psum || !glob || !dx || !dp || !gsum_ws || B <= 0 || N <= 0 || C <= 0 || (C & 1)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(policy_pool_gsum_kernel, dim3((C / 2 + 63) / 64, B), dim3(256), 0, stream, gout, gsum_ws, N, C);
    const long rows = (long)B * N;
    hipLaunchKernelGGL(policy_pool_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, gout, x, p, psum, glob, gsum_ws, dx, dp,
                       rows, N, C);
    return d2s_check_launch();
}

}  // extern "C"
