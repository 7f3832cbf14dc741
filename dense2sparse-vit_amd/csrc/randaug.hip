// RandAugment / ColorJitter on the GPU (timm's auto_augment.py "increasing" ops and ImageEnhance-based ColorJitter), bit-exact with
// Pillow on uint8 RGB HWC images.  The host (d2s/data.py) draws every random quantity and writes, per image, a list of at most
// RA_MAX_OPS ops; this kernel applies an image's list in order.  tests/randaug_ref.py restates every op in numpy.
//
// One workgroup per image; the ops of an image are sequential (a workgroup barrier between them), images are independent.  Every op
// reads one buffer and writes another (the geometric ops and SMOOTH read neighbours, so nothing runs in place): op 0 reads `in`, the
// last op writes `out`, and the ops in between alternate between `out` and one scratch image, so that any image size works with one
// code path (a 224 x 224 x 3 image is 147 KiB and stays in L2 between two ops of its workgroup; 384 x 384 x 3 is 432 KiB).  LDS holds
// only the three 256-bin histograms, their prefix sums and the three 256-entry tables.
//
// Pillow's arithmetic, restated:
//   affine    libImaging/Geometry.c: xin = a0 (x + .5) + a1 (y + .5) + a2 (double), fill when outside [0, W) x [0, H); then -.5, floor,
//             neighbours clamped to the image; bilinear a + (b - a) d truncated; bicubic p1 + d (p2 + d (p3 + d p4)) clipped, truncated
//   enhance   libImaging/Blend.c: fp32 d + f (x - d), truncated when 0 <= f <= 1, clipped first otherwise; degenerates: 0 (Brightness),
//             L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Color), int(mean(L) + 0.5) (Contrast), ImageFilter.SMOOTH (Sharpness)
//   LUT ops   PIL/ImageOps.py autocontrast (cutoff 0), equalize, posterize, solarize, invert; timm's solarize_add
// No contraction anywhere (the Makefile also builds this file with -ffp-contract=off).  The only atomics are integer LDS atomics
// (histogram counts, min / max bin, the luma sum): integer sums do not depend on the order.
#pragma clang fp contract(off)
#include "d2s_common.h"

namespace {

enum { OP_NONE = 0, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_AFFINE, OP_COLOR, OP_CONTRAST,
       OP_BRIGHTNESS, OP_SHARPNESS, OP_COUNT };
// Op table entry: RA_OP_INTS int32.  Written by d2s/data.py (pack_ops).
enum { E_CODE = 0, E_RESAMPLE, E_IARG, E_FARG, E_MATRIX };      // E_FARG: a float's bits; E_MATRIX: six doubles (int pairs, 8-byte aligned)
constexpr int RA_MAX_OPS = 8;
constexpr int RA_OP_INTS = 16;
constexpr int THREADS = 1024;
constexpr int FILL_R = 124, FILL_G = 116, FILL_B = 104;          // round(255 * ImageNet mean)

struct Lds {
    unsigned hist[3][256];
    unsigned pre[3][256];        // exclusive prefix sums of the histogram (equalize)
    unsigned char lut[3][256];
    int lo[3], hi[3];
    unsigned lsum;
};

__device__ __forceinline__ unsigned byte_of(const unsigned* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

// 48 bytes = 16 whole pixels = three 16-byte accesses: the unit of every pointwise pass when the image is a multiple of it (and its
// base therefore 16-byte aligned; the entry point checks the buffers).  Other sizes go pixel by pixel.
__device__ __forceinline__ void load48(const uint8_t* p, unsigned w[12]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint4 v = q[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
}

// dst pixel = f(src pixel) for every pixel; f(const unsigned in[3], unsigned out[3]).
template <class F>
__device__ __forceinline__ void pointwise(const uint8_t* src, uint8_t* dst, int npix, bool vec, F f) {
    if (vec) {
        for (int g = threadIdx.x; g < npix / 16; g += THREADS) {
            unsigned w[12], o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            load48(src + (size_t)g * 48, w);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const unsigned in[3] = {byte_of(w, 3 * p), byte_of(w, 3 * p + 1), byte_of(w, 3 * p + 2)};
                unsigned out[3];
                f(in, out);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[(3 * p + c) >> 2] |= out[c] << (((3 * p + c) & 3) * 8);
            }
            uint4* q = reinterpret_cast<uint4*>(dst + (size_t)g * 48);
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
        }
    } else {
        for (int p = threadIdx.x; p < npix; p += THREADS) {
            const unsigned in[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
            unsigned out[3];
            f(in, out);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[3 * p + c] = (uint8_t)out[c];
        }
    }
}

// f(const unsigned in[3]) for every pixel (the histogram and the luma sum).
template <class F>
__device__ __forceinline__ void foreach_pixel(const uint8_t* src, int npix, bool vec, F f) {
    if (vec) {
        for (int g = threadIdx.x; g < npix / 16; g += THREADS) {
            unsigned w[12];
            load48(src + (size_t)g * 48, w);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                const unsigned in[3] = {byte_of(w, 3 * p), byte_of(w, 3 * p + 1), byte_of(w, 3 * p + 2)};
                f(in);
            }
        }
    } else {
        for (int p = threadIdx.x; p < npix; p += THREADS) {
            const unsigned in[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
            f(in);
        }
    }
}

__device__ __forceinline__ unsigned luma(const unsigned in[3]) { return (19595u * in[0] + 38470u * in[1] + 7471u * in[2] + 0x8000u) >> 16; }

// Image.blend(degenerate, image, f) for one channel.
__device__ __forceinline__ unsigned blend(unsigned d, unsigned x, float f, bool inside) {
    float t = (float)(int)d + f * (float)((int)x - (int)d);
    if (!inside) t = t <= 0.f ? 0.f : (t >= 255.f ? 255.f : t);
    return (unsigned)(int)t;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ void affine_op(const uint8_t* src, uint8_t* dst, int S, const double* m, int resample) {
    const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5];
    for (int p = threadIdx.x; p < S * S; p += THREADS) {
        const int y = p / S, x = p - y * S;
        double xin = (a0 * (x + 0.5) + a1 * (y + 0.5)) + a2;
        double yin = (a3 * (x + 0.5) + a4 * (y + 0.5)) + a5;
        uint8_t* o = dst + 3 * p;
        if (xin < 0.0 || xin >= (double)S || yin < 0.0 || yin >= (double)S) {
            o[0] = FILL_R; o[1] = FILL_G; o[2] = FILL_B;
            continue;
        }
        xin -= 0.5;
        yin -= 0.5;
        const int x0 = (int)floor(xin), y0 = (int)floor(yin);
        const double dx = xin - x0, dy = yin - y0;
        if (resample == 0) {
            const int xa = clampi(x0, S - 1) * 3, xb = clampi(x0 + 1, S - 1) * 3;
            const uint8_t* r0 = src + (size_t)clampi(y0, S - 1) * S * 3;
            const uint8_t* r1 = src + (size_t)clampi(y0 + 1, S - 1) * S * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p00 = r0[xa + c], p01 = r0[xb + c], p10 = r1[xa + c], p11 = r1[xb + c];
                const double v1 = p00 + (p01 - p00) * dx;
                const double v2 = p10 + (p11 - p10) * dx;
                o[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
            }
        } else {
            int xs[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) xs[t] = clampi(x0 - 1 + t, S - 1) * 3;
            double col[3][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint8_t* row = src + (size_t)clampi(y0 - 1 + r, S - 1) * S * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double v1 = row[xs[0] + c], v2 = row[xs[1] + c], v3 = row[xs[2] + c], v4 = row[xs[3] + c];
                    const double p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
                    col[c][r] = v2 + dx * (p2 + dx * (p3 + dx * p4));
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v1 = col[c][0], v2 = col[c][1], v3 = col[c][2], v4 = col[c][3];
                const double p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
                const double v = v2 + dy * (p2 + dy * (p3 + dy * p4));
                o[c] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (uint8_t)(int)v);
            }
        }
    }
}

// Sharpness: blend(SMOOTH(image), image, f); SMOOTH copies the 1-pixel border, where the blend of a pixel with itself is the pixel.
__device__ void sharpness_op(const uint8_t* src, uint8_t* dst, int S, float f) {
    const bool inside = f >= 0.f && f <= 1.f;
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    for (int p = threadIdx.x; p < S * S; p += THREADS) {
        const int y = p / S, x = p - y * S;
        const uint8_t* q = src + 3 * p;
        uint8_t* o = dst + 3 * p;
        if (y == 0 || x == 0 || y == S - 1 || x == S - 1) {
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
            continue;
        }
        const int rs = S * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float ss = 0.5f;                                      // libImaging/Filter.c: offset + 0.5, then the rows y + 1, y, y - 1
            ss += ((float)q[rs - 3 + c] * k1 + (float)q[rs + c] * k1) + (float)q[rs + 3 + c] * k1;
            ss += ((float)q[-3 + c] * k1 + (float)q[c] * k5) + (float)q[3 + c] * k1;
            ss += ((float)q[-rs - 3 + c] * k1 + (float)q[-rs + c] * k1) + (float)q[-rs + 3 + c] * k1;
            const unsigned d = ss <= 0.f ? 0u : (ss >= 255.f ? 255u : (unsigned)(int)ss);
            o[c] = (uint8_t)blend(d, q[c], f, inside);
        }
    }
}

// The three 256-entry tables of a LUT op into L.lut (histogram ops read `src` first).
__device__ __forceinline__ void build_lut(Lds& L, const uint8_t* src, int npix, bool vec, int code, int iarg) {
    const int t = threadIdx.x;
    if (code == OP_AUTOCONTRAST || code == OP_EQUALIZE) {
        if (t < 768) (&L.hist[0][0])[t] = 0;
        if (t < 3) { L.lo[t] = 256; L.hi[t] = -1; }
        __syncthreads();
        foreach_pixel(src, npix, vec, [&](const unsigned in[3]) {
            atomicAdd(&L.hist[0][in[0]], 1u);
            atomicAdd(&L.hist[1][in[1]], 1u);
            atomicAdd(&L.hist[2][in[2]], 1u);
        });
        __syncthreads();
        if (t < 768 && (&L.hist[0][0])[t]) {
            atomicMin(&L.lo[t >> 8], t & 255);
            atomicMax(&L.hi[t >> 8], t & 255);
        }
        if (code == OP_EQUALIZE && t < 3) {
            unsigned n = 0;
            for (int i = 0; i < 256; ++i) {
                L.pre[t][i] = n;
                n += L.hist[t][i];
            }
        }
        __syncthreads();
    }
    if (t < 768) {
        const int c = t >> 8, i = t & 255;
        int v = i;
        if (code == OP_AUTOCONTRAST) {
            const int lo = L.lo[c], hi = L.hi[c];
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double offset = (double)(-lo) * scale;
                v = clampi((int)((double)i * scale + offset), 255);
            }
        } else if (code == OP_EQUALIZE) {
            const int lo = L.lo[c], hi = L.hi[c];              // more than one non-empty bin <=> lo < hi; sum(histogram) = npix
            const unsigned step = hi > lo ? ((unsigned)npix - L.hist[c][hi]) / 255u : 0u;
            if (step) v = (int)min(255u, (step / 2 + L.pre[c][i]) / step);
        } else if (code == OP_INVERT) {
            v = 255 - i;
        } else if (code == OP_POSTERIZE) {
            v = i & ~((1 << (8 - iarg)) - 1);
        } else if (code == OP_SOLARIZE) {
            v = i < iarg ? i : 255 - i;
        } else {                                               // OP_SOLARIZE_ADD (threshold 128)
            v = i < 128 ? min(255, i + iarg) : i;
        }
        L.lut[c][i] = (unsigned char)v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void randaug_kernel(const uint8_t* in, const int* __restrict__ table, int S, uint8_t* scratch,
                                                          uint8_t* out) {
    __shared__ Lds L;
    const int b = blockIdx.x;
    const int npix = S * S;
    const size_t nbytes = (size_t)npix * 3;
    const bool vec = npix % 16 == 0;
    const int* ops = table + (size_t)b * RA_MAX_OPS * RA_OP_INTS;
    int nops = 0;
    while (nops < RA_MAX_OPS && ops[nops * RA_OP_INTS + E_CODE] != OP_NONE) ++nops;
    const uint8_t* src = in + b * nbytes;
    uint8_t* const bufs[2] = {out + b * nbytes, scratch + b * nbytes};
    if (nops == 0) {
        pointwise(src, bufs[0], npix, vec, [](const unsigned i[3], unsigned o[3]) { o[0] = i[0]; o[1] = i[1]; o[2] = i[2]; });
        return;
    }
    for (int k = 0; k < nops; ++k) {
        const int* e = ops + k * RA_OP_INTS;
        const int code = e[E_CODE], iarg = e[E_IARG];
        const float f = __int_as_float(e[E_FARG]);
        const bool inside = f >= 0.f && f <= 1.f;
        uint8_t* dst = bufs[(nops - 1 - k) & 1];
        if (code <= OP_SOLARIZE_ADD) {
            build_lut(L, src, npix, vec, code, iarg);
            pointwise(src, dst, npix, vec, [&](const unsigned i[3], unsigned o[3]) {
                o[0] = L.lut[0][i[0]]; o[1] = L.lut[1][i[1]]; o[2] = L.lut[2][i[2]];
            });
        } else if (code == OP_AFFINE) {
            affine_op(src, dst, S, reinterpret_cast<const double*>(e + E_MATRIX), e[E_RESAMPLE]);
        } else if (code == OP_COLOR) {
            pointwise(src, dst, npix, vec, [&](const unsigned i[3], unsigned o[3]) {
                const unsigned d = luma(i);
                o[0] = blend(d, i[0], f, inside); o[1] = blend(d, i[1], f, inside); o[2] = blend(d, i[2], f, inside);
            });
        } else if (code == OP_CONTRAST) {
            if (threadIdx.x == 0) L.lsum = 0;
            __syncthreads();
            unsigned part = 0;                                    // at most 255 * 4096^2 < 2^32 over the whole image
            foreach_pixel(src, npix, vec, [&](const unsigned i[3]) { part += luma(i); });
            atomicAdd(&L.lsum, part);
            __syncthreads();
            const unsigned d = (unsigned)(int)((double)L.lsum / (double)npix + 0.5);
            pointwise(src, dst, npix, vec, [&](const unsigned i[3], unsigned o[3]) {
                o[0] = blend(d, i[0], f, inside); o[1] = blend(d, i[1], f, inside); o[2] = blend(d, i[2], f, inside);
            });
        } else if (code == OP_BRIGHTNESS) {
            pointwise(src, dst, npix, vec, [&](const unsigned i[3], unsigned o[3]) {
                o[0] = blend(0, i[0], f, inside); o[1] = blend(0, i[1], f, inside); o[2] = blend(0, i[2], f, inside);
            });
        } else {
            sharpness_op(src, dst, S, f);
        }
        __syncthreads();                                          // this op's stores before the next op's loads (same workgroup)
        src = dst;
    }
}

// Any table content is memory-safe: a code outside the enum runs as one of the ops, LUT indices are bytes, neighbour indices are clamped.
}  // namespace

extern "C" {

int d2s_randaug_max_ops(void) { return RA_MAX_OPS; }
int d2s_randaug_op_ints(void) { return RA_OP_INTS; }
size_t d2s_randaug_scratch_bytes(int B, int S) {
    if (B <= 0 || S <= 0 || S > 4096) return 0;
    return ((size_t)B * S * S * 3 + 15) / 16 * 16;
}

/* in, out: [B, S, S, 3] uint8 (distinct buffers, 16-byte aligned); table: [B, RA_MAX_OPS, RA_OP_INTS] int32 (device), an image's list
 * ends at the first entry with code 0; scratch: d2s_randaug_scratch_bytes(B, S) bytes, 16-byte aligned.  An empty list copies. */
int d2s_randaug_apply(const uint8_t* in, const int* table, int B, int S, uint8_t* scratch, uint8_t* out, hipStream_t stream) {
    if (!in || !table || !scratch || !out || B <= 0 || S <= 0 || S > 4096 || in == out || in == scratch || out == scratch ||
        ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)table & 7))
        return D2S_ERR_ARG;
    hipLaunchKernelGGL(randaug_kernel, dim3((unsigned)B), dim3(THREADS), 0, stream, in, table, S, scratch, out);
    return d2s_check_launch();
}

}  // extern "C"
