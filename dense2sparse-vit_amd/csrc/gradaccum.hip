// Gradient accumulation and global-norm clipping over the flat gradient arena (d2s.engine.TrainStep accum_steps= / clip_grad=).
//
//   grad_accumulate : acc = g | acc = fl(acc + g) | g = fl(acc + g)   - the window's fp32 sum in arrival order, element by element
//   grad_sumsq      : per-chunk sum of squares of the combined gradient, one fixed tree per chunk
//   grad_clip_fold  : ordered fold of the per-chunk partials in double -> {total_norm, coef} of torch.nn.utils.clip_grad_norm_
//
// All three walk the arena in the 1024-element chunks of the fused AdamW (csrc/loss.hip: one workgroup of 256 threads per chunk, one
// f32x4 per thread) and read the same per-chunk descriptor: a chunk that is not `active` - a frozen tensor, or one that is in no
// parameter group - is not read and not written.  No atomics, every order is fixed: two launches on the same input are bit-identical.
#include "d2s_common.h"

namespace {

constexpr int CH = 1024;
struct ChunkDesc { float lr, wd; int active; int pad; };      // csrc/loss.hip

// MODE 0: dst = src (8 B / element); 1: dst = fl(dst + src) (12 B); 2: src-side result, g = fl(acc + g) (12 B).
template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ g,
                                                              const ChunkDesc* __restrict__ desc) {
    if (!desc[blockIdx.x].active) return;
    const long base = (long)blockIdx.x * CH + threadIdx.x * 4;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + base);
    if constexpr (MODE == 0) {
        *reinterpret_cast<f32x4*>(acc + base) = gv;
    } else {
        const f32x4 av = *reinterpret_cast<const f32x4*>(acc + base);
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = av[j] + gv[j];
        *reinterpret_cast<f32x4*>((MODE == 1 ? acc : g) + base) = r;
    }
}

// partials[c] = sum of g^2 over chunk c (0 for a chunk that is not active, so the fold needs no descriptor).
// The fp32 tree of one chunk, after one rounding per square (or none where the compiler contracts square and add into an FMA):
//   2 levels inside the thread     (x0^2 + x1^2) + (x2^2 + x3^2)
//   6 levels across the wave       xor butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits)
//   2 levels across the 4 waves    (w0 + w1) + (w2 + w3)
// Reduction depth L = 10 additions on any path from a square to the chunk's partial; everything after it is double.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const ChunkDesc* __restrict__ desc,
                                                         float* __restrict__ partials) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    if (!desc[blockIdx.x].active) {
        if (tid == 0) partials[blockIdx.x] = 0.f;
        return;
    }
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + (long)blockIdx.x * CH + tid * 4);
    float s = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  Thread t folds partials[t], partials[t + 256], ... in ascending order in double, then the 256 sums are folded by a
// fixed binary tree in LDS.  total_norm = fl(scale * sqrt(sum)) (double until the final rounding); coef = min(1, max_norm /
// (total_norm + 1e-6)) in fp32, as clip_grad_norm_ forms it from its fp32 norm (a NaN norm gives a NaN coefficient, as there).
__global__ __launch_bounds__(256) void grad_clip_fold_kernel(const float* __restrict__ partials, int n_chunks, float scale,
                                                             float max_norm, float* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int c = tid; c < n_chunks; c += 256) s += (double)partials[c];
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)((double)scale * sqrt(red[0]));
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;
    }
}

}  // namespace

extern "C" {

int d2s_grad_accumulate(float* acc, float* g, const void* chunk_desc, int n_chunks, int mode, hipStream_t stream) {
    if (!acc || !g || !chunk_desc || n_chunks <= 0 || mode < 0 || mode > 2) return D2S_ERR_ARG;
    const size_t span = (size_t)n_chunks * CH;      // both pointers are __restrict__ in the kernel: the two arenas must not overlap
    if ((acc <= g && g < acc + span) || (g <= acc && acc < g + span)) return D2S_ERR_ARG;
    const ChunkDesc* d = static_cast<const ChunkDesc*>(chunk_desc);
    if (mode == 0) hipLaunchKernelGGL(grad_accumulate_kernel<0>, dim3(n_chunks), dim3(256), 0, stream, acc, g, d);
    else if (mode == 1) hipLaunchKernelGGL(grad_accumulate_kernel<1>, dim3(n_chunks), dim3(256), 0, stream, acc, g, d);
    else hipLaunchKernelGGL(grad_accumulate_kernel<2>, dim3(n_chunks), dim3(256), 0, stream, acc, g, d);
    return d2s_check_launch();
}

int d2s_grad_clip_coef(const float* g, const void* chunk_desc, int n_chunks, float scale, float max_norm, float* partials, float* out,
                       hipStream_t stream) {
    if (!g || !chunk_desc || n_chunks <= 0 || !partials || !out || !(scale > 0.f) || !(max_norm > 0.f)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(256), 0, stream, g, static_cast<const ChunkDesc*>(chunk_desc), partials);
    hipLaunchKernelGGL(grad_clip_fold_kernel, dim3(1), dim3(256), 0, stream, partials, n_chunks, scale, max_norm, out);
    return d2s_check_launch();
}

}  // extern "C"
