// Training / validation input pipeline on the GPU (the reference's build_data_sets.py:8-34 transforms + timm Mixup, train.py:29-31):
// crop + resize (bit-exact with Pillow's 8-bit two-pass resampler), horizontal flip, ToTensor + Normalize, RandomErasing and
// Mixup / CutMix, on a batch of variable-size RGB uint8 HWC images packed into one flat buffer.
//
// Pillow's resampler (libImaging/Resample.c, 8 bits per channel), restated:
//   coefficients per output index xx, in double:  scale = in / out, fs = max(scale, 1), support = filter_support * fs,
//     center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in) - xmin,
//     w_t = filter((t + xmin - center + 0.5) * (1 / fs)), normalised by their sum, then (int)(w * 2^22 +- 0.5) (sign of w);
//   horizontal pass first (only the source rows the vertical pass reads), into uint8, then the vertical pass; each pass starts its
//   integer accumulator at 1 << 21 and ends with clamp(acc >> 22, 0, 255).
// torchvision crops before it resizes, so the filter clamps at the crop edge: the crop is resampled with in0 = 0, in1 = size.
//
// No contraction anywhere in this file (the Makefile also builds it with -ffp-contract=off): the coefficients must round like
// Pillow's, and the Mixup blend is fl(x * a) + fl(x' * b) as two separate torch ops compute it.
#pragma clang fp contract(off)
#include "d2s_common.h"

namespace {

// Descriptor: D2S_AUG_DESC int32 per sample (float fields stored as their bit patterns).  Written by d2s/data.py (pack_batch).
enum {
    A_OFF_LO = 0, A_OFF_HI, A_H, A_W,            // byte offset of the HWC image in the pixel buffer, source height / width
    A_CI, A_CJ, A_CH, A_CW,                      // crop box (top, left, height, width) in source pixels
    A_GH, A_GW, A_WY, A_WX,                      // resize grid (height, width); top-left of the S x S window computed from it
    A_FILTER, A_FLIP,                            // 0 bilinear, 1 bicubic; horizontal flip of the window
    A_YFIRST, A_YN, A_ROWOFF,                    // crop rows [yfirst, yfirst + yn) the vertical pass reads; their first row in the scratch
    A_EMODE, A_ECOUNT,                           // erase mode (0 off, 1 const, 2 rand, 3 pixel), number of boxes
    A_MIX,                                       // 0 none, 1 mixup, 2 cutmix
    A_PIXA, A_PIXB, A_LABA, A_LABB,              // float: out = x * pixa + x' * pixb;  label = y * laba + y' * labb
    A_CY0, A_CY1, A_CX0, A_CX1,                  // cutmix box [y0, y1) x [x0, x1)
    A_LABEL,                                     // class index
    A_BOXES = 32                                 // erase boxes: (top, left, h, w) x D2S_AUG_MAX_ERASE
};
constexpr int MAX_ERASE = 8;
constexpr int DESC = A_BOXES + 4 * MAX_ERASE;     // 64
constexpr int PREC = 22;                          // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr int HROWS = 8;                          // source rows staged per horizontal-pass workgroup (at most)
constexpr int VROWS = 8;                          // output rows per vertical-pass workgroup
constexpr int LDS_MAX = 160 * 1024;

__device__ __forceinline__ float fbits(int v) { return __int_as_float(v); }

__device__ __forceinline__ double filter_eval(int f, double x) {
    if (f == 0) {                                 // bilinear (triangle), support 1
        if (x < 0.0) x = -x;
        if (x < 1.0) return 1.0 - x;
        return 0.0;
    }
    const double a = -0.5;                        // bicubic, support 2
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for one output index: fixed-point taps into k[0, cnt), returns xmin.
__device__ int pillow_coeffs(int f, int in_size, int out_size, int xx, int* k, int& cnt) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (f == 0 ? 1.0 : 2.0) * fs;
    const double ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int t = 0; t < xmax; ++t) ww += filter_eval(f, (t + xmin - center + 0.5) * ss);
    for (int t = 0; t < xmax; ++t) {
        double w = filter_eval(f, (t + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[t] = w < 0 ? (int)(-0.5 + w * (1 << PREC)) : (int)(0.5 + w * (1 << PREC));
    }
    cnt = xmax;
    return xmin;
}

__device__ __forceinline__ int clip8(int acc) {
    acc >>= PREC;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// ---- pass 1: horizontal resample of crop rows [yfirst, yfirst + yn), window columns only, into uint8 scratch [rows, S, 3] --------
// grid (bands, B); LDS: S * kmax coefficients, S xmin, S counts, then `rows` staged source row segments of `rowbytes` each.
__global__ __launch_bounds__(256) void augment_hpass_kernel(const uint8_t* __restrict__ pix, long pix_chunks, const int* __restrict__ desc,
                                                            int S, int kmax, int rows, int rowbytes, uint8_t* __restrict__ inter) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int* d = desc + (long)blockIdx.y * DESC;
    const int yn = d[A_YN];
    const int r0 = (int)blockIdx.x * rows;
    if (r0 >= yn) return;                                   // uniform per workgroup
    const int nr = min(rows, yn - r0);
    int* kk = reinterpret_cast<int*>(lds);
    int* kxmin = kk + S * kmax;
    int* kcnt = kxmin + S;
    unsigned char* rowbuf = reinterpret_cast<unsigned char*>(kcnt + S);
    rowbuf += (16 - (reinterpret_cast<uintptr_t>(rowbuf) & 15)) & 15;
    const int W = d[A_W], cw = d[A_CW], f = d[A_FILTER], gw = d[A_GW], wx = d[A_WX];
    const long off = (long)(((unsigned long)(unsigned)d[A_OFF_HI] << 32) | (unsigned)d[A_OFF_LO]);
    for (int x = threadIdx.x; x < S; x += blockDim.x) {
        int cnt;
        kxmin[x] = pillow_coeffs(f, cw, gw, wx + x, kk + x * kmax, cnt);
        kcnt[x] = cnt;
    }
    // stage the row segments with 16-byte loads from their enclosing aligned chunks (the buffer is a whole number of chunks)
    const int row_src0 = d[A_CI] + d[A_YFIRST] + r0;
    const int nchunk_row = rowbytes >> 4;
    for (int q = threadIdx.x; q < nr * nchunk_row; q += blockDim.x) {
        const int r = q / nchunk_row, c = q - r * nchunk_row;
        const long s0 = off + ((long)(row_src0 + r) * W + d[A_CJ]) * 3;
        const long e0 = s0 + (long)cw * 3;
        const long g = (s0 >> 4) + c;
        if (g * 16 < e0 && g < pix_chunks)
            *reinterpret_cast<uint4*>(rowbuf + r * rowbytes + c * 16) = reinterpret_cast<const uint4*>(pix)[g];
    }
    __syncthreads();
    const long rowoff = d[A_ROWOFF] + r0;
    for (int p = threadIdx.x; p < nr * S; p += blockDim.x) {
        const int r = p / S, x = p - r * S;
        const long s0 = off + ((long)(row_src0 + r) * W + d[A_CJ]) * 3;
        const unsigned char* src = rowbuf + r * rowbytes + (int)(s0 & 15) + kxmin[x] * 3;
        const int* k = kk + x * kmax;
        const int cnt = kcnt[x];
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
            a0 += (int)src[3 * t] * w;
            a1 += (int)src[3 * t + 1] * w;
            a2 += (int)src[3 * t + 2] * w;
        }
        uint8_t* o = inter + ((rowoff + r) * S + x) * 3;
        o[0] = (uint8_t)clip8(a0);
        o[1] = (uint8_t)clip8(a1);
        o[2] = (uint8_t)clip8(a2);
    }
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// N(0, 1) keyed by (seed, sample, channel, y, x): splitmix64 of the key, Box-Muller in double, rounded to fp32.
// tests/augment_ref.py::erase_normal restates it.
__device__ float keyed_normal(unsigned long long seed, int sample, int c, int y, int x) {
    const unsigned long long key = ((unsigned long long)sample << 40) | ((unsigned long long)c << 32) |
                                   ((unsigned long long)(y & 0xFFFF) << 16) | (unsigned long long)(x & 0xFFFF);
    const unsigned long long h1 = mix64(seed ^ mix64(key));
    const unsigned long long h2 = mix64(h1);
    const double u1 = (double)((h1 >> 11) + 1) * 0x1.0p-53;
    const double u2 = (double)(h2 >> 11) * 0x1.0p-53;
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// One sample's uint8 pixel at output (y, x): vertical resample of the scratch, flip.
__device__ __forceinline__ void vresample_pixel(const int* __restrict__ d, const uint8_t* __restrict__ inter, const int* kv, int ymin, int cnt,
                                                int S, int x, int u[3]) {
    const int xc = d[A_FLIP] ? S - 1 - x : x;
    const int yn = d[A_YN];
    const uint8_t* base = inter + ((long)d[A_ROWOFF] * S + xc) * 3;
    const int* k = kv;
    int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < cnt; ++t) {
        int r = ymin - d[A_YFIRST] + t;
        r = r < 0 ? 0 : (r >= yn ? yn - 1 : r);              // never outside the sample's rows (host and device agree on them)
        const uint8_t* q = base + (long)r * S * 3;
        const int w = k[t];
        a0 += (int)q[0] * w;
        a1 += (int)q[1] * w;
        a2 += (int)q[2] * w;
    }
    u[0] = clip8(a0);
    u[1] = clip8(a1);
    u[2] = clip8(a2);
}

// ToTensor + Normalize and erasing of one sample's uint8 pixel at output (y, x).
__device__ __forceinline__ void finish_pixel(const int* __restrict__ d, const int u[3], int sample, int y, int x, unsigned long long seed,
                                             float v[3]) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)u[c] / 255.f - mean[c]) / stdv[c];
    const int mode = d[A_EMODE], n = d[A_ECOUNT];
    if (mode) {
        int hit = -1;
        for (int e = 0; e < n; ++e) {                        // later boxes overwrite earlier ones, as in timm's loop
            const int* b = d + A_BOXES + 4 * e;
            if (y >= b[0] && y < b[0] + b[2] && x >= b[1] && x < b[1] + b[3]) hit = e;
        }
        if (hit >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c] = mode == 1 ? 0.f : (mode == 2 ? keyed_normal(seed, sample, c, 0xFFFF - hit, 0xFFFF) : keyed_normal(seed, sample, c, y, x));
        }
    }
}

// One sample's value at output (y, x) for the 3 channels: the two steps above, fused.
__device__ __forceinline__ void sample_pixel(const int* __restrict__ d, const uint8_t* __restrict__ inter, const int* kv, int kmax,
                                             int ymin, int cnt, int sample, int S, int y, int x, unsigned long long seed, float v[3]) {
    int u[3];
    vresample_pixel(d, inter, kv, ymin, cnt, S, x, u);
    finish_pixel(d, u, sample, y, x, seed, v);
}

__device__ __forceinline__ void mix_out(const int* __restrict__ d, const float vi[3], const float vj[3], int y, int x, float o[3]) {
    const int m = d[A_MIX];
    if (m == 1) {
        const float a = fbits(d[A_PIXA]), b = fbits(d[A_PIXB]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p = vi[c] * a, q = vj[c] * b;
            o[c] = p + q;
        }
    } else if (m == 2 && y >= d[A_CY0] && y < d[A_CY1] && x >= d[A_CX0] && x < d[A_CX1]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = vj[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = vi[c];
    }
}

// ---- pass 2: vertical resample + epilogue for the pair (i, B-1-i), VROWS output rows per workgroup -------------------------------
// grid (ceil(S / VROWS), ceil(B / 2)); LDS: per sample of the pair VROWS * kmax coefficients, VROWS ymin, VROWS counts.
__global__ __launch_bounds__(256) void augment_vpass_kernel(const uint8_t* __restrict__ inter, const int* __restrict__ desc, int B, int S,
                                                            int kmax, unsigned long long seed, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int i = blockIdx.y, j = B - 1 - i;
    const int y0 = blockIdx.x * VROWS;
    const int ny = min(VROWS, S - y0);
    const int* di = desc + (long)i * DESC;
    const int* dj = desc + (long)j * DESC;
    int* kk = reinterpret_cast<int*>(lds);                    // [2][VROWS][kmax]
    int* kmin = kk + 2 * VROWS * kmax;                        // [2][VROWS]
    int* kcnt = kmin + 2 * VROWS;
    for (int q = threadIdx.x; q < 2 * ny; q += blockDim.x) {
        const int s = q / ny, r = q - s * ny;
        const int* d = s ? dj : di;
        int cnt;
        kmin[s * VROWS + r] = pillow_coeffs(d[A_FILTER], d[A_CH], d[A_GH], d[A_WY] + y0 + r, kk + (s * VROWS + r) * kmax, cnt);
        kcnt[s * VROWS + r] = cnt;
    }
    __syncthreads();
    const long plane = (long)S * S;
    for (int p = threadIdx.x; p < ny * S; p += blockDim.x) {
        const int r = p / S, x = p - r * S, y = y0 + r;
        float vi[3], vj[3], o[3];
        sample_pixel(di, inter, kk + r * kmax, kmax, kmin[r], kcnt[r], i, S, y, x, seed, vi);
        if (j != i) {
            sample_pixel(dj, inter, kk + (VROWS + r) * kmax, kmax, kmin[VROWS + r], kcnt[VROWS + r], j, S, y, x, seed, vj);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) vj[c] = vi[c];
        }
        const long pos = (long)y * S + x;
        mix_out(di, vi, vj, y, x, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((long)i * 3 + c) * plane + pos] = o[c];
        if (j != i) {
            mix_out(dj, vj, vi, y, x, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[((long)j * 3 + c) * plane + pos] = o[c];
        }
    }
}

// ---- the same in two passes around the op kernel of csrc/randaug.hip (RandAugment / ColorJitter work on the uint8 image) ------------------
// pass 2a: vertical resample + flip into uint8 [B, S, S, 3].  grid (ceil(S / VROWS), B); LDS: VROWS * kmax coefficients, ymin, counts.
__global__ __launch_bounds__(256) void augment_vpass_u8_kernel(const uint8_t* __restrict__ inter, const int* __restrict__ desc, int S, int kmax,
                                                               uint8_t* __restrict__ img) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int i = blockIdx.y;
    const int y0 = blockIdx.x * VROWS;
    const int ny = min(VROWS, S - y0);
    const int* d = desc + (long)i * DESC;
    int* kk = reinterpret_cast<int*>(lds);                    // [VROWS][kmax]
    int* kmin = kk + VROWS * kmax;
    int* kcnt = kmin + VROWS;
    for (int r = threadIdx.x; r < ny; r += blockDim.x) {
        int cnt;
        kmin[r] = pillow_coeffs(d[A_FILTER], d[A_CH], d[A_GH], d[A_WY] + y0 + r, kk + r * kmax, cnt);
        kcnt[r] = cnt;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < ny * S; p += blockDim.x) {
        const int r = p / S, x = p - r * S;
        int u[3];
        vresample_pixel(d, inter, kk + r * kmax, kmin[r], kcnt[r], S, x, u);
        uint8_t* o = img + (((long)i * S + y0 + r) * S + x) * 3;
        o[0] = (uint8_t)u[0];
        o[1] = (uint8_t)u[1];
        o[2] = (uint8_t)u[2];
    }
}

// pass 2b: ToTensor + Normalize, erasing and the mix for the pair (i, B-1-i) from uint8 [B, S, S, 3].  grid (ceil(S / VROWS), ceil(B / 2)).
__global__ __launch_bounds__(256) void augment_finish_kernel(const uint8_t* __restrict__ img, const int* __restrict__ desc, int B, int S,
                                                             unsigned long long seed, float* __restrict__ out) {
    const int i = blockIdx.y, j = B - 1 - i;
    const int y0 = blockIdx.x * VROWS;
    const int ny = min(VROWS, S - y0);
    const int* di = desc + (long)i * DESC;
    const int* dj = desc + (long)j * DESC;
    const long plane = (long)S * S;
    for (int p = threadIdx.x; p < ny * S; p += blockDim.x) {
        const int r = p / S, x = p - r * S, y = y0 + r;
        const long pos = (long)y * S + x;
        const uint8_t* qi = img + ((long)i * plane + pos) * 3;
        const uint8_t* qj = img + ((long)j * plane + pos) * 3;
        const int ui[3] = {qi[0], qi[1], qi[2]}, uj[3] = {qj[0], qj[1], qj[2]};
        float vi[3], vj[3], o[3];
        finish_pixel(di, ui, i, y, x, seed, vi);
        if (j != i) {
            finish_pixel(dj, uj, j, y, x, seed, vj);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) vj[c] = vi[c];
        }
        mix_out(di, vi, vj, y, x, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((long)i * 3 + c) * plane + pos] = o[c];
        if (j != i) {
            mix_out(dj, vj, vi, y, x, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[((long)j * 3 + c) * plane + pos] = o[c];
        }
    }
}

// ---- soft labels (timm mixup_target): label[i] = one_hot(t_i) * laba_i + one_hot(t_{B-1-i}) * labb_i, one_hot in {off, on} -----------
__global__ __launch_bounds__(256) void augment_labels_kernel(const int* __restrict__ desc, int B, int C, float on, float off,
                                                             float* __restrict__ out) {
    const int i = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int* di = desc + (long)i * DESC;
    const int ti = di[A_LABEL], tj = desc[(long)(B - 1 - i) * DESC + A_LABEL];
    const float y1 = c == ti ? on : off, y2 = c == tj ? on : off;
    const float p = y1 * fbits(di[A_LABA]), q = y2 * fbits(di[A_LABB]);
    out[(long)i * C + c] = p + q;
}

}  // namespace

extern "C" {

int d2s_augment_desc_ints(void) { return DESC; }

// Dynamic LDS of the horizontal pass for one staged row count, and the row count used for a batch (as many as fit, at most HROWS).
static size_t hpass_lds(int S, int kmax, int rows, int rowbytes) { return (size_t)S * (kmax + 2) * 4 + 16 + (size_t)rows * rowbytes; }
static int hpass_rows(int S, int kmax, int rowbytes) {
    int rows = HROWS;
    while (rows > 1 && hpass_lds(S, kmax, rows, rowbytes) > (size_t)LDS_MAX / 2) --rows;     // two workgroups per CU when it can
    return hpass_lds(S, kmax, rows, rowbytes) <= (size_t)LDS_MAX ? rows : 0;
}

/* pix: packed uint8 HWC images, pix_bytes a multiple of 16; desc: [B, DESC] int32 (device).  Host-side maxima over the batch:
 * max_rows = max yn, kmax_h / kmax_v = max 2 * ceil(support) + 1 of the horizontal / vertical filters, rowbytes = max staged row
 * segment bytes (crop width * 3 + 32, a multiple of 16).  inter: scratch of sum(yn) * S * 3 bytes.  out: [B, 3, S, S] fp32. */
int d2s_augment_images(const uint8_t* pix, long pix_bytes, const int* desc, int B, int S, int max_rows, int kmax_h, int kmax_v,
                       int rowbytes, unsigned long long seed, uint8_t* inter, float* out, hipStream_t stream) {
    if (!pix || !desc || !inter || !out || B <= 0 || S <= 0 || S > 4096 || max_rows <= 0 || kmax_h <= 0 || kmax_v <= 0 ||
        rowbytes < 32 || (rowbytes & 15) || (pix_bytes & 15) || pix_bytes <= 0)
        return D2S_ERR_ARG;
    const int rows = hpass_rows(S, kmax_h, rowbytes);
    const size_t vlds = (size_t)2 * VROWS * (kmax_v + 2) * 4;
    if (rows == 0 || vlds > (size_t)LDS_MAX) return D2S_ERR_ARG;           // a crop more than ~40x the output size
    const size_t hlds = hpass_lds(S, kmax_h, rows, rowbytes);
    hipLaunchKernelGGL(augment_hpass_kernel, dim3((unsigned)((max_rows + rows - 1) / rows), (unsigned)B), dim3(256), hlds, stream, pix,
                       pix_bytes >> 4, desc, S, kmax_h, rows, rowbytes, inter);
    int rc = d2s_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(augment_vpass_kernel, dim3((unsigned)((S + VROWS - 1) / VROWS), (unsigned)((B + 1) / 2)), dim3(256), vlds, stream,
                       inter, desc, B, S, kmax_v, seed, out);
    return d2s_check_launch();
}

size_t d2s_augment_ops_scratch_bytes(int B, int S) { return 3 * d2s_randaug_scratch_bytes(B, S); }

/* d2s_augment_images with an op table (csrc/randaug.hip) applied to the uint8 image between the flip and ToTensor: the fused second pass
 * becomes vertical pass + flip -> uint8, the op kernel, Normalize + erase + mix.  images: d2s_augment_ops_scratch_bytes(B, S) bytes of
 * scratch (three uint8 [B, S, S, 3] images), 16-byte aligned.  With an empty list for every image the output equals d2s_augment_images'. */
int d2s_augment_images_ops(const uint8_t* pix, long pix_bytes, const int* desc, const int* table, int B, int S, int max_rows, int kmax_h,
                           int kmax_v, int rowbytes, unsigned long long seed, uint8_t* inter, uint8_t* images, float* out,
                           hipStream_t stream) {
    if (!pix || !desc || !table || !inter || !images || !out || B <= 0 || S <= 0 || S > 4096 || max_rows <= 0 || kmax_h <= 0 || kmax_v <= 0 ||
        rowbytes < 32 || (rowbytes & 15) || (pix_bytes & 15) || pix_bytes <= 0)
        return D2S_ERR_ARG;
    const int rows = hpass_rows(S, kmax_h, rowbytes);
    const size_t vlds = (size_t)VROWS * (kmax_v + 2) * 4;
    if (rows == 0 || vlds > (size_t)LDS_MAX) return D2S_ERR_ARG;
    const size_t one = d2s_randaug_scratch_bytes(B, S);
    const size_t hlds = hpass_lds(S, kmax_h, rows, rowbytes);
    hipLaunchKernelGGL(augment_hpass_kernel, dim3((unsigned)((max_rows + rows - 1) / rows), (unsigned)B), dim3(256), hlds, stream, pix,
                       pix_bytes >> 4, desc, S, kmax_h, rows, rowbytes, inter);
    int rc = d2s_check_launch();
    if (rc) return rc;
    const unsigned bands = (unsigned)((S + VROWS - 1) / VROWS);
    hipLaunchKernelGGL(augment_vpass_u8_kernel, dim3(bands, (unsigned)B), dim3(256), vlds, stream, inter, desc, S, kmax_v, images);
    rc = d2s_check_launch();
    if (rc) return rc;
    rc = d2s_randaug_apply(images, table, B, S, images + one, images + 2 * one, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(augment_finish_kernel, dim3(bands, (unsigned)((B + 1) / 2)), dim3(256), 0, stream, images + 2 * one, desc, B, S, seed,
                       out);
    return d2s_check_launch();
}

/* out: [B, C] fp32 soft labels (timm mixup_target with on = 1 - s + s / C, off = s / C rounded by the caller as torch.full does). */
int d2s_augment_labels(const int* desc, int B, int C, float on, float off, float* out, hipStream_t stream) {
    if (!desc || !out || B <= 0 || C <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(augment_labels_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)B), dim3(256), 0, stream, desc, B, C, on, off, out);
    return d2s_check_launch();
}

}  // extern "C"
