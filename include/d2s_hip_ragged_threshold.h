/* d2s_hip_ragged_threshold.h - the entries of libd2s_hip.so for training the dynamic keep ratio on the ragged packed batch
 * (--patch-score-threshold --ragged-train).
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h, d2s_hip_squeeze.h, d2s_hip_ats.h and d2s_hip_ragged_train.h are closed as well;
 * these entries follow the same style (one `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's
 * conventions: device pointers owned by the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on
 * `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * The batch is ragged and packed, as in d2s_hip_ragged_train.h: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, the first
 * of them its CLS token; row_src [total] is the ORIGINAL token index of every row (patch id + 1, 0 for CLS); an image of one row (CLS only)
 * is valid.  fp32 only.  No entry uses atomics or needs its output cleared: every output element is written exactly once when cu_seqlens
 * covers [0, total).
 */
#ifndef D2S_HIP_RAGGED_THRESHOLD_H
#define D2S_HIP_RAGGED_THRESHOLD_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of d2s_half_mean_concat_varlen: g_out [total, C] -> g_x [total, C].  Columns c < C/2: a copy.  Columns c >= C/2: a non-CLS row
 * of image b takes (1 / T_b) * the sum of g_out[., c] over ALL rows of the image (the CLS row received the mean too), its CLS row takes 0
 * (it is no part of the mean); T_b = 0: zeros.  The forward's grid and its two forms (16-byte accesses when C is a multiple of 8 and both
 * pointers are 16-byte aligned); wave w sums rows w, w+4, ..., the four partial sums are combined as (0+1)+(2+3).  Like the forward it
 * takes no `total`: cu_seqlens must lie inside the buffers.
 * D2S_ERR_ARG before any launch: a null pointer; B, C <= 0; C odd. */
int d2s_half_mean_concat_varlen_bwd(const float* g_out, const int* cu_seqlens, float* g_x, int B, int C, d2s_stream_t stream);

/* Mask loss of a packed threshold stage: scores [total] (one per packed row, the CLS rows' entries are ignored), target [B, N] (the
 * teacher target of d2s_teacher_target) -> loss_rows [B].  For image b over its non-CLS rows r: q_r = target[b, row_src[r] - 1] / the sum
 * of those entries (d2s_gather_renorm's recursion; 0 when the sum is 0).  mode 1 (kl_div): sum_r q_r (log q_r - log_softmax(scores)_r), a
 * zero q_r contributing nothing; mode 3 (mse): sum_r (scores_r - q_r)^2.  An image without a non-CLS row gives 0.  One workgroup per
 * image, 2 N floats of LDS; the maximum, the sums and their combine order are those of d2s_softmax_rows.  A segment is clamped to
 * [0, total) and to N rows.
 * D2S_ERR_ARG before any launch: a null pointer; B, total, N <= 0; N > 8192; a mode other than 1 and 3. */
int d2s_ragged_mask_loss_fwd(const float* scores, const float* target, const int* cu_seqlens, const int* row_src, float* loss_rows, int B,
                             int total, int N, int mode, d2s_stream_t stream);

/* Its gradient: dscores [total] = scale * d loss_rows[b] / d scores - mode 1: scale * (p_r - q_r) with p = softmax over the image's non-CLS
 * scores (p_r * sum(q) - q_r, should the image's target have vanished); mode 3: scale * 2 (scores_r - q_r); exactly 0 at every CLS row.
 * D2S_ERR_ARG before any launch: as d2s_ragged_mask_loss_fwd. */
int d2s_ragged_mask_loss_bwd(const float* scores, const float* target, const int* cu_seqlens, const int* row_src, float* dscores, int B,
                             int total, int N, int mode, float scale, d2s_stream_t stream);

/* Teacher rows and row weights of the token distillation on a packed batch: token_t holds B images of N rows of D floats, image b at
 * token_t + b * image_stride (floats; N * D for a contiguous [B, N, D], (N + 1) * D for the token view of a [B, N + 1, D] tensor)
 * -> out [total, D], row r of image b = token_t[b, row_src[r] - 1, :], and w [total] = 1 / (total - B); a CLS row takes zeros and the
 * weight 0.  d2s_kl_rows then runs over out with contiguous maps and w as its row_weight.  Image b writes the rows from its CLS row up to
 * the next image's (the first from row 0, the last up to total), clamped to [0, total].
 * D2S_ERR_ARG before any launch: a null pointer; B, total, N, D <= 0; D or image_stride not a multiple of 4; image_stride < 0; token_t or
 * out not 16-byte aligned. */
int d2s_ragged_teacher_rows(const float* token_t, long image_stride, const int* cu_seqlens, const int* row_src, float* out, float* w, int B,
                            int total, int N, int D, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_RAGGED_THRESHOLD_H */
