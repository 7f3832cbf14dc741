/* d2s_hip_evo.h - the entries of libd2s_hip.so for the Evo-ViT baseline: slow-fast token update (--method evo).
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h, d2s_hip_squeeze.h, d2s_hip_ats.h, d2s_hip_ragged_train.h,
 * d2s_hip_ragged_threshold.h and d2s_hip_avit.h are closed as well; these entries follow the same style (one `int d2s_...(` declaration at
 * the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the caller, 0 on success or
 * D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * X [B, 1+T, D] is the full token tensor (CLS first), g [B, T] the global score of the T patch tokens, kept [B, k] / dropped [B, T-k] the
 * ascending int64 id lists of a slow-fast block (together a partition of 0 .. T-1; a row whose id is outside [0, T) is skipped, nothing
 * is dereferenced for it), xc / yc [B, k+2, D] the block's input [CLS | kept | representative row] (d2s_gather_fuse_fwd with t = 0) and
 * its output.  Common limits: 1 <= B <= 65535, 2 <= T <= 4095, 1 <= k <= T-1, D % 4 == 0, D <= 1024.  fp32 only, no atomics, fixed
 * summation orders, nothing read back by the host: two launches on equal inputs give the same bits, and every launch may be captured.
 */
#ifndef D2S_HIP_EVO_H
#define D2S_HIP_EVO_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Score evolution and re-selection, one workgroup per image.  kept_prev NULL (the start; g_in is not read and may be NULL):
 * g_out[b,t] = (sum_h cls_row[b,h,1+t]) / H with cls_row [B, H, 1+T], h ascending.  Otherwise cls_row is [B, H, k+2], the row of a
 * slow-fast block that ran on kept_prev [B, k]: g_out = g_in except g_out[b, kept_prev_i] = fma(tau, (sum_h cls_row[b,h,1+i]) / H,
 * (1 - tau) * g_in[b, kept_prev_i]).  Then kept [B, k] / dropped [B, T-k] = the hard top-k of g_out exactly as d2s_select_topk(g_out, k)
 * emits it (value descending, equal values lowest index first, both lists ascending).  g_out may be g_in.
 * D2S_ERR_ARG before any launch: cls_row, g_out, kept or dropped null; kept_prev given without g_in; B, T, k outside the common limits;
 * H <= 0; tau outside [0, 1]. */
int d2s_evo_select(const float* g_in, const long long* kept_prev, const float* cls_row, float* g_out, long long* kept, long long* dropped,
                   int B, int H, int T, int k, float tau, d2s_stream_t stream);

/* The write-back of a slow-fast block, in place on X: X[b,0] = yc[b,0]; X[b,1+kept_i] = yc[b,1+i]; X[b,1+dropped_j] += d with
 * d = yc[b,k+1] - xc[b,k+1], per element one subtraction then one addition (the fast update).  Every row of X has one writer.
 * D2S_ERR_ARG before any launch: a null pointer; B, T, k, D outside the common limits. */
int d2s_evo_scatter_fwd(const float* yc, const float* xc, const long long* kept, const long long* dropped, float* X, int B, int T, int k,
                        int D, d2s_stream_t stream);

/* Backward of d2s_evo_scatter_fwd in yc: dX [B, 1+T, D] is the gradient of the written-back X -> dyc [B, k+2, D], every element written:
 * dyc[b,0] = dX[b,0]; dyc[b,1+i] = dX[b,1+kept_i]; dyc[b,k+1] = delta_b = sum_j dX[b,1+dropped_j], the dropped list cut into four
 * contiguous quarters, each summed in ascending j, the four partial rows added as (0 + 1) + (2 + 3).  (The gradient in X is dX itself
 * at the dropped rows and nothing at the replaced ones; the term -delta onto xc[b,k+1] is applied by d2s_evo_gather_bwd.)
 * D2S_ERR_ARG before any launch: a null pointer; B, T, k, D outside the common limits. */
int d2s_evo_scatter_bwd(const float* dX, const long long* kept, const long long* dropped, float* dyc, int B, int T, int k, int D,
                        d2s_stream_t stream);

/* Backward of the gather [CLS | kept | r] together with the fast update's -r term, in place on dX (on entry the gradient of the
 * written-back X, on return the gradient of X before the block): dX[b,0] = dxc[b,0]; dX[b,1+kept_i] = dxc[b,1+i];
 * dX[b,1+dropped_j] = fma(w_j, dxc[b,k+1] - dyc[b,k+1], dX[b,1+dropped_j]) with w_j = g[b,dropped_j] / S[b] as d2s_gather_fuse_fwd formed
 * it (0 when S[b] <= 0; a zero weight leaves the row as it is).  dxc is the block's input gradient, dyc what d2s_evo_scatter_bwd wrote.
 * D2S_ERR_ARG before any launch: a null pointer; B, T, k, D outside the common limits. */
int d2s_evo_gather_bwd(const float* dxc, const float* dyc, const float* g, const float* S, const long long* kept, const long long* dropped,
                       float* dX, int B, int T, int k, int D, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_EVO_H */
