// A-ViT baseline (--method avit; DESIGN.md section 25 - the build's own definition): per-token adaptive depth on the ragged packed batch.
// Every block ends with a halting step; the tokens that halted leave the batch before the next block (d2s_ragged_repack).
//   avit_halt_kernel         the halting step of block `layer` (1-based): h = sigmoid(gamma * y[row, 0] - beta) for every live row, the
//                            dense per-token state [B, N] (cumulative score c, remainder R, halting layer nh; reached through row_src),
//                            the CLS weight w[b] and acc[b] += w[b] * y_cls, keep / counts for the re-pack, the per-image partial sums of
//                            the two penalty terms
//   avit_halt_bwd_kernel     its backward, added to the gradient that arrives through the re-pack (or written in full: fresh)
//   avit_penalty_fwd_kernel  ponder mean and distribution prior from the per-layer, per-image partials
//   avit_penalty_bwd_kernel  their gradient as one factor per layer (and one for the ponder term) that avit_halt_bwd_kernel applies
// One workgroup per image; the CLS row of an image decides first (thread 0), the other rows follow it.  Latency work: a row costs one
// load of its channel 0.  No atomics; every sum has a fixed order (lane-strided partials, wave butterfly, waves as (0+1)+(2+3); the
// penalty kernels sum sequentially), so two launches give the same bits.
#include "d2s_common.h"
#include "d2s_hip_avit.h"

namespace {

__device__ __forceinline__ float avit_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// Image b owns rows [r0, r0 + n) of the packed batch, clamped to [0, total); row r0 is its CLS token (token index 0).  An image whose
// CLS token has halted in an earlier layer (nh[b, 0] != 0) is finished: its CLS row is a dead row - weight 0, no state touched, nothing
// added to the partials - and any other row it still has is dropped.
// part [B, 3]: sum of h over the image's live rows, the number of live rows, sum of (layer + R) over the rows that halt here.
__global__ __launch_bounds__(256) void avit_halt_kernel(const float* __restrict__ y, const int* __restrict__ cu,
                                                        const int* __restrict__ row_src, float* __restrict__ c, float* __restrict__ R,
                                                        int* __restrict__ nh, float* __restrict__ h, float* __restrict__ w,
                                                        float* __restrict__ acc, float* __restrict__ ycls, float* __restrict__ ysave,
                                                        float* __restrict__ keep, int* __restrict__ counts, float* __restrict__ part,
                                                        int N, int D, int total, int layer, int last, float gamma, float beta, float thr) {
    __shared__ float redf[2][4];
    __shared__ int redi[2][4];
    __shared__ float bw;
    __shared__ int bflag[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = min(max(cu[b], 0), total);
    const int n = min(max(cu[b + 1], r0), total) - r0;
    const long s0 = (long)b * N;
    float sh = 0.f, srho = 0.f;
    int nlive = 0, kept = 0;
    if (tid == 0) {
        int dead = 1, halt = 0;
        float wv = 0.f;
        if (n > 0) {
            float hv = 0.f;
            if (nh[s0] == 0) {
                dead = 0;
                hv = avit_sigmoid(gamma * y[(long)r0 * D] - beta);
                const float c0 = c[s0], c1 = c0 + hv;
                halt = last || c1 > thr;
                c[s0] = c1;
                wv = hv;
                if (halt) {
                    wv = 1.0f - c0;
                    nh[s0] = layer;
                    R[s0] = wv;
                    srho = (float)layer + wv;
                }
                sh = hv;
                nlive = 1;
            }
            if (h) h[r0] = hv;
            keep[r0] = 1.f;                          // the CLS row is always kept, as d2s_ragged_repack requires
        }
        w[b] = wv;
        bw = wv;
        bflag[0] = dead;
        bflag[1] = halt;
    }
    __syncthreads();
    const int dead = bflag[0], cls_halt = bflag[1];
    const float wv = bw;
    for (int i = 1 + tid; i < n; i += 256) {
        const int r = r0 + i;
        const int t = row_src[r];
        float hv = 0.f, k = 0.f;
        if (!dead && t > 0 && t < N) {
            hv = avit_sigmoid(gamma * y[(long)r * D] - beta);
            const float c0 = c[s0 + t], c1 = c0 + hv;
            c[s0 + t] = c1;
            if (cls_halt || last || c1 > thr) {
                const float rem = 1.0f - c0;
                nh[s0 + t] = layer;
                R[s0 + t] = rem;
                srho += (float)layer + rem;
            } else {
                k = 1.f;
                ++kept;
            }
            sh += hv;
            ++nlive;
        }
        if (h) h[r] = hv;
        keep[r] = k;
    }
    sh = wave_sum(sh);
    srho = wave_sum(srho);
    nlive = wave_sum_i(nlive);
    kept = wave_sum_i(kept);
    if (lane == 0) {
        redf[0][wave] = sh;
        redf[1][wave] = srho;
        redi[0][wave] = nlive;
        redi[1][wave] = kept;
    }
    __syncthreads();
    if (tid == 0) {
        part[(long)b * 3 + 0] = (redf[0][0] + redf[0][1]) + (redf[0][2] + redf[0][3]);
        part[(long)b * 3 + 1] = (float)((redi[0][0] + redi[0][1]) + (redi[0][2] + redi[0][3]));
        part[(long)b * 3 + 2] = (redf[1][0] + redf[1][1]) + (redf[1][2] + redf[1][3]);
        counts[b] = (redi[1][0] + redi[1][1]) + (redi[1][2] + redi[1][3]);
    }
    const long d0 = (long)b * D;
    for (int col = tid; col < D; col += 256) {
        const float yc = n > 0 ? y[(long)r0 * D + col] : 0.f;
        if (ycls) ycls[d0 + col] = yc;
        if (!dead) {
            acc[d0 + col] += wv * yc;
            if (cls_halt && ysave) ysave[d0 + col] = yc;
        }
    }
}

// g [total, D]: the gradient of the rows that entered the halting step.  fresh = 0: it holds what arrived through the re-pack and
// the step's own terms are added; fresh = 1: nothing arrived (the last layer) and every element of the image's rows is written.
// nh / R-derived w, ycls (this layer's CLS rows), ysave (the CLS row of every image at its halting layer) are the finished forward's;
// gsc [L + 1]: avit_penalty_bwd_kernel's factors.
__global__ __launch_bounds__(256) void avit_halt_bwd_kernel(float* __restrict__ g, const float* __restrict__ h, const int* __restrict__ cu,
                                                            const int* __restrict__ row_src, const int* __restrict__ nh,
                                                            const float* __restrict__ w, const float* __restrict__ dacc,
                                                            const float* __restrict__ ycls, const float* __restrict__ ysave,
                                                            const float* __restrict__ gsc, int N, int D, int total, int layer, int L,
                                                            int fresh, float gamma) {
    __shared__ float redf[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r0 = min(max(cu[b], 0), total);
    const int n = min(max(cu[b + 1], r0), total) - r0;
    if (n <= 0) return;
    const long s0 = (long)b * N;
    const int n0 = nh[s0];
    const bool dead = n0 < layer;                    // finished in an earlier layer: a dead row, nothing of the loss depends on it
    if (fresh) {
        // a live image: the CLS row and column 0 of every row are written below
        for (int i = (dead ? 0 : 1) + wave; i < n; i += 4)
            for (int col = (dead ? 0 : 1) + lane; col < D; col += 64) g[(long)(r0 + i) * D + col] = 0.f;
    }
    if (dead) return;
    const long d0 = (long)b * D;
    float a = 0.f, e = 0.f;
    for (int col = tid; col < D; col += 256) {
        const float da = dacc[d0 + col];
        a += da * ycls[d0 + col];
        e += da * ysave[d0 + col];
    }
    a = wave_sum(a);
    e = wave_sum(e);
    if (lane == 0) {
        redf[0][wave] = a;
        redf[1][wave] = e;
    }
    __syncthreads();
    const float s_l = (redf[0][0] + redf[0][1]) + (redf[0][2] + redf[0][3]);
    const float s_n = (redf[1][0] + redf[1][1]) + (redf[1][2] + redf[1][3]);
    const float gbar = gsc[layer - 1], gp = gsc[L];
    for (int i = 1 + tid; i < n; i += 256) {
        const long r = r0 + i;
        const int t = row_src[r];
        float add = 0.f;
        if (t > 0 && t < N) {
            const float gh = (nh[s0 + t] > layer ? -gp : 0.f) + gbar;
            const float hv = h[r];
            add = gh * gamma * (hv * (1.0f - hv));
        }
        g[r * D] = (fresh ? 0.f : g[r * D]) + add;
    }
    const float gh0 = (n0 > layer ? (s_l - s_n) - gp : 0.f) + gbar;
    const float h0 = h[r0];
    const float add0 = gh0 * gamma * (h0 * (1.0f - h0));
    const float wv = w[b];
    for (int col = tid; col < D; col += 256) {
        float v = (fresh ? 0.f : g[(long)r0 * D + col]) + wv * dacc[d0 + col];
        if (col == 0) v += add0;
        g[(long)r0 * D + col] = v;
    }
}

// part [L, B, 3] as avit_halt_kernel wrote them, tgt [L] the normalised target distribution -> out[0] = mean over the B * N tokens of
// (n + R), out[1] = P = sum_l tgt_l (log tgt_l - log p_l) / L with p = clamp(Hbar / sum Hbar, 0.01, 0.99); hbar [L], cnt [L] (live rows of
// the layer) for the backward.  Lane l sums its layer over the images in order; lane 0 finishes sequentially.  L <= 64.
__global__ __launch_bounds__(64) void avit_penalty_fwd_kernel(const float* __restrict__ part, const float* __restrict__ tgt,
                                                              float* __restrict__ out, float* __restrict__ hbar, float* __restrict__ cnt,
                                                              int L, int B, float inv_bn) {
    __shared__ float hb[64], rho[64];
    const int l = threadIdx.x;
    if (l < L) {
        float sh = 0.f, nl = 0.f, sr = 0.f;
        for (int b = 0; b < B; ++b) {
            const float* p = part + ((long)l * B + b) * 3;
            sh += p[0];
            nl += p[1];
            sr += p[2];
        }
        const float v = nl > 0.f ? sh / nl : 0.f;
        hb[l] = v;
        rho[l] = sr;
        hbar[l] = v;
        cnt[l] = nl;
    }
    __syncthreads();
    if (l == 0) {
        float S = 0.f, r = 0.f, P = 0.f;
        for (int j = 0; j < L; ++j) {
            S += hb[j];
            r += rho[j];
        }
        for (int j = 0; j < L; ++j) {
            const float q = S > 0.f ? hb[j] / S : 0.f;
            const float p = fminf(fmaxf(q, 0.01f), 0.99f);
            const float t = tgt[j];
            if (t > 0.f) P += t * (logf(t) - logf(p));
        }
        out[0] = r * inv_bn;
        out[1] = P / (float)L;
    }
}

// gsc[k] = dprior * dP/dHbar_k / cnt_k for k < L (0 for a layer without a live row), gsc[L] = dponder / (B * N).
// dP/dHbar_k = a_k / S - (sum_l a_l Hbar_l) / S^2 with a_l = -tgt_l / (L p_l) where 0.01 <= Hbar_l / S <= 0.99 and 0 elsewhere.
__global__ __launch_bounds__(64) void avit_penalty_bwd_kernel(const float* __restrict__ hbar, const float* __restrict__ cnt,
                                                              const float* __restrict__ tgt, const float* __restrict__ dponder,
                                                              const float* __restrict__ dprior, float* __restrict__ gsc, int L,
                                                              float inv_bn) {
    __shared__ float al[64];
    __shared__ float bc[2];
    const int l = threadIdx.x;
    if (l == 0) {
        float S = 0.f;
        for (int j = 0; j < L; ++j) S += hbar[j];
        float A = 0.f;
        for (int j = 0; j < L; ++j) {
            const float q = S > 0.f ? hbar[j] / S : 0.f;
            const float a = (q >= 0.01f && q <= 0.99f) ? -tgt[j] / ((float)L * q) : 0.f;
            al[j] = a;
            A += a * hbar[j];
        }
        bc[0] = S;
        bc[1] = A;
        gsc[L] = dponder[0] * inv_bn;
    }
    __syncthreads();
    if (l < L) {
        const float S = bc[0], A = bc[1];
        const float n = cnt[l];
        gsc[l] = (S > 0.f && n > 0.f) ? dprior[0] * (al[l] / S - A / (S * S)) / n : 0.f;
    }
}

}  // namespace

extern "C" {

int d2s_avit_halt(const float* y, const int* cu_seqlens, const int* row_src, float* c, float* R, int* halt_layer, float* h, float* w,
                  float* acc, float* ycls, float* ysave, float* keep, int* counts, float* part, int B, int N, int D, int total, int layer,
                  int last, float gamma, float beta, float threshold, hipStream_t stream) {
    if (!y || !cu_seqlens || !row_src || !c || !R || !halt_layer || !w || !acc || !keep || !counts || !part) return D2S_ERR_ARG;
    if (B <= 0 || N <= 0 || D <= 0 || total <= 0 || layer < 1 || (last != 0 && last != 1)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(avit_halt_kernel, dim3(B), dim3(256), 0, stream, y, cu_seqlens, row_src, c, R, halt_layer, h, w, acc, ycls, ysave,
                       keep, counts, part, N, D, total, layer, last, gamma, beta, threshold);
    return d2s_check_launch();
}

int d2s_avit_halt_bwd(float* g, const float* h, const int* cu_seqlens, const int* row_src, const int* halt_layer, const float* w,
                      const float* dacc, const float* ycls, const float* ysave, const float* gsc, int B, int N, int D, int total, int layer,
                      int L, int fresh, float gamma, hipStream_t stream) {
    if (!g || !h || !cu_seqlens || !row_src || !halt_layer || !w || !dacc || !ycls || !ysave || !gsc) return D2S_ERR_ARG;
    if (B <= 0 || N <= 0 || D <= 0 || total <= 0 || layer < 1 || L < layer || L > 64 || (fresh != 0 && fresh != 1)) return D2S_ERR_ARG;
    hipLaunchKernelGGL(avit_halt_bwd_kernel, dim3(B), dim3(256), 0, stream, g, h, cu_seqlens, row_src, halt_layer, w, dacc, ycls, ysave, gsc,
                       N, D, total, layer, L, fresh, gamma);
    return d2s_check_launch();
}

int d2s_avit_penalty_fwd(const float* part, const float* tgt, float* out, float* hbar, float* cnt, int L, int B, int N,
                         hipStream_t stream) {
    if (!part || !tgt || !out || !hbar || !cnt || L < 1 || L > 64 || B <= 0 || N <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(avit_penalty_fwd_kernel, dim3(1), dim3(64), 0, stream, part, tgt, out, hbar, cnt, L, B,
                       1.0f / ((float)B * (float)N));
    return d2s_check_launch();
}

int d2s_avit_penalty_bwd(const float* hbar, const float* cnt, const float* tgt, const float* dponder, const float* dprior, float* gsc,
                         int L, int B, int N, hipStream_t stream) {
    if (!hbar || !cnt || !tgt || !dponder || !dprior || !gsc || L < 1 || L > 64 || B <= 0 || N <= 0) return D2S_ERR_ARG;
    hipLaunchKernelGGL(avit_penalty_bwd_kernel, dim3(1), dim3(64), 0, stream, hbar, cnt, tgt, dponder, dprior, gsc, L,
                       1.0f / ((float)B * (float)N));
    return d2s_check_launch();
}

}  // extern "C"
