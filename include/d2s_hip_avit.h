/* d2s_hip_avit.h - the entries of libd2s_hip.so for the A-ViT baseline: per-token adaptive depth on the ragged packed batch
 * (--method avit).
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h, d2s_hip_squeeze.h, d2s_hip_ats.h, d2s_hip_ragged_train.h and
 * d2s_hip_ragged_threshold.h are closed as well; these entries follow the same style (one `int d2s_...(` declaration at the start of a
 * line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the caller, 0 on success or D2S_ERR_* (< 0), nothing
 * throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * The batch is ragged and packed: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, the first of them its CLS token;
 * row_src [total] is the original token index of every row (0 at CLS, 1 .. N-1 at the patches).  Inside the kernels a segment is clamped
 * to [0, total) and a row whose row_src is outside [1, N) is skipped, so nothing is dereferenced outside the buffers.  The per-token
 * state is dense, [B, N]: c the cumulative halting score, R the remainder, halt_layer the layer a token halted at (0: still live); a run
 * starts from all three cleared.  An image whose CLS token has halted is finished: from then on its CLS row is a dead row (weight 0, no
 * state touched, no part in any sum).  fp32 only, no atomics, fixed summation orders: two launches on equal inputs give the same bits.
 */
#ifndef D2S_HIP_AVIT_H
#define D2S_HIP_AVIT_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The halting step of block `layer` (1-based; last != 0: every live token halts here) on y [total, D], the residual stream after the
 * block.  For every live row: h = sigmoid(gamma * y[row, 0] - beta), c += h; the row halts when c > threshold (strict, fp32; the caller
 * passes 1 - eps), when `last`, or when its image's CLS row halts in this launch; a halting row gets halt_layer = layer and R = 1 - (c
 * before this layer).  Written: h [total] (0 at a dead or skipped row; optional), w [B] (h of the CLS row, R if it halts here, 0 for a
 * finished image), acc [B, D] += w[b] * y[CLS row], ycls [B, D] = the CLS rows (optional), ysave [B, D] = the CLS row of every image that
 * finishes here (other images untouched; optional), keep [total] (1 at every CLS row and at every row that goes on, 0 elsewhere) and
 * counts [B] (rows that go on, CLS not counted) as d2s_ragged_offsets / d2s_ragged_repack take them, part [B, 3] = per image {sum of h
 * over its live rows, number of live rows, sum of (layer + R) over the rows that halt here}.  One workgroup per image.
 * D2S_ERR_ARG before any launch: a null pointer other than h, ycls, ysave; B, N, D, total <= 0; layer < 1; last not 0 or 1. */
int d2s_avit_halt(const float* y, const int* cu_seqlens, const int* row_src, float* c, float* R, int* halt_layer, float* h, float* w,
                  float* acc, float* ycls, float* ysave, float* keep, int* counts, float* part, int B, int N, int D, int total, int layer,
                  int last, float gamma, float beta, float threshold, d2s_stream_t stream);

/* Backward of d2s_avit_halt for block `layer` of L, after the whole forward: halt_layer [B, N] is the finished forward's, h, w, ycls are
 * this layer's, ysave [B, D] holds every image's CLS row at its halting layer, dacc [B, D] is the gradient of acc, gsc [L + 1] comes from
 * d2s_avit_penalty_bwd.  For a row live at `layer`, with t its token, n its halting layer and n0 its image's CLS halting layer:
 *   g_h = [layer < n] * ([t = 0] * (<dacc_b, ycls_b> - <dacc_b, ysave_b>) - gsc[L]) + gsc[layer - 1]
 *   g[row, 0] += g_h * gamma * h (1 - h);  g[CLS row, :] += w[b] * dacc_b
 * fresh = 0: g [total, D] holds the gradient that arrived through the re-pack and is updated in place; fresh = 1: nothing arrived (the
 * last layer) and every element of g is written (zeros where nothing is added; cu_seqlens must cover [0, total)).  The rows of a
 * finished image receive nothing.  One workgroup per image.
 * D2S_ERR_ARG before any launch: a null pointer; B, N, D, total <= 0; layer < 1; L < layer; L > 64; fresh not 0 or 1. */
int d2s_avit_halt_bwd(float* g, const float* h, const int* cu_seqlens, const int* row_src, const int* halt_layer, const float* w,
                      const float* dacc, const float* ycls, const float* ysave, const float* gsc, int B, int N, int D, int total, int layer,
                      int L, int fresh, float gamma, d2s_stream_t stream);

/* The two penalty terms from part [L, B, 3] (layer l - 1 at part + (l - 1) * B * 3) and tgt [L], the target distribution over the layers:
 * out[0] = mean over the B * N tokens of (halting layer + remainder); out[1] = P = sum_l tgt_l (log tgt_l - log p_l) / L with
 * Hbar_l = (sum of h over the rows live at l) / (their number) - 0 for a layer without a live row - and p = clamp(Hbar / sum Hbar, 0.01,
 * 0.99).  hbar [L] and cnt [L] (live rows per layer) are kept for the backward.  One wave; sums in index order.
 * D2S_ERR_ARG before any launch: a null pointer; L < 1; L > 64; B, N <= 0. */
int d2s_avit_penalty_fwd(const float* part, const float* tgt, float* out, float* hbar, float* cnt, int L, int B, int N,
                         d2s_stream_t stream);

/* Backward of d2s_avit_penalty_fwd as the per-layer factors d2s_avit_halt_bwd applies: dponder [1] and dprior [1] are the gradients of
 * out[0] and out[1] (device scalars) -> gsc [L + 1]: gsc[k] = dprior * dP/dHbar_k / cnt_k (0 for a layer without a live row; the
 * clamp passes no gradient outside its range), gsc[L] = dponder / (B * N).
 * D2S_ERR_ARG before any launch: a null pointer; L < 1; L > 64; B, N <= 0. */
int d2s_avit_penalty_bwd(const float* hbar, const float* cnt, const float* tgt, const float* dponder, const float* dprior, float* gsc,
                         int L, int B, int N, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_AVIT_H */
