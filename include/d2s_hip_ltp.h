/* d2s_hip_ltp.h - the entries of libd2s_hip.so for the LTP baseline: learned per-block token thresholds on the attention a token
 * receives.
 *
 * d2s_hip.h is the frozen core of the C ABI and the older d2s_hip_*.h headers are closed as well; these entries follow the same style
 * (one `int d2s_...(` or `size_t d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device
 * pointers owned by the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * fp32 only, no atomics, fixed summation orders: two launches on equal inputs give the same bits.  Every argument error is reported
 * before any launch, and a segment of a packed batch is clamped to [0, total) inside the kernels, so nothing is dereferenced outside the
 * buffers whatever cu_seqlens holds.
 */
#ifndef D2S_HIP_LTP_H
#define D2S_HIP_LTP_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace d2s_ltp_score_f32 needs for `rows` token rows (B * n, or total) and H heads: the per-head partial column sums.
 * 0 for rows <= 0 or H <= 0.  No stream, nothing launched. */
size_t d2s_ltp_score_workspace_bytes(long rows, int H);

/* The attention every token RECEIVES in one block, from that block's qkv [rows, 3, H, 64] and the log-sum-exp its attention forward
 * wrote: score[j] = sum_h sum_i w_i P[h, i, j] / (H sum_i w_i) per image, P recomputed as the attention backward recomputes it.  Each
 * image's scores sum to 1.  Three forms, chosen by the pointers:
 *   plain   policy, cinv, cu_seqlens null: B images of n rows, total = B * n, lse [B, H, n] (d2s_attn_fwd_f32), P = exp(S - lse), w = 1;
 *   policy  policy [B, n] and cinv [B, H, n] given, cu_seqlens null: lse, cinv as d2s_attn_policy_fwd_f32 wrote them for this policy,
 *           P_ij = exp(S_ij - lse_i) mk_ij + cinv_i with mk_ij = policy_j off the diagonal and 1 on it, w_i = policy_i (eps is inside
 *           lse and cinv); with an all-ones policy and eps = 0 the result is bit for bit the plain form's;
 *   varlen  cu_seqlens [B + 1] given, policy and cinv null: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, lse
 *           [H, total] (d2s_attn_varlen_fwd_lse_f32), n is max_n, any upper bound of the longest image; on equal lengths the result is
 *           bit for bit the plain form's.  Rows no segment covers are left untouched.
 * score [rows] is written at every row, the CLS entry with its true value.  Two launches: key tile x (image, head) workgroups on the
 * f32-input matrix pipe writing per-head partials into the workspace, then one workgroup per image that folds the heads in ascending
 * order and scales once.
 * D2S_ERR_ARG before any launch: qkv, lse or score null; B, n, total, H <= 0; n > 8192; one of policy / cinv without the other; a policy
 * together with cu_seqlens; total != B * n without cu_seqlens.  D2S_ERR_WORKSPACE: workspace null or smaller than
 * d2s_ltp_score_workspace_bytes(total, H). */
int d2s_ltp_score_f32(const float* qkv, const float* lse, const float* policy, const float* cinv, const int* cu_seqlens, float* score,
                      void* workspace, size_t workspace_bytes, int B, int n, int total, int H, float scale, d2s_stream_t stream);

/* The hard decision of a stage on the packed batch: keep [total] = 1 at every image's first (CLS) row and where score >= theta[0] - the
 * fp32 score against the fp32 parameter, read from device memory - and 0 elsewhere (a NaN score is dropped); counts [B] = kept rows per
 * image, CLS not counted: the form d2s_ragged_offsets / d2s_ragged_repack take.  dense_mask [B, T] (optional; needs row_src [total], the
 * original token index of every row): 1 at row_src - 1 of every kept non-CLS row, 0 elsewhere.  One workgroup per image.
 * D2S_ERR_ARG before any launch: score, cu_seqlens, theta, keep or counts null; B, total <= 0; dense_mask without row_src or with T <= 0. */
int d2s_ltp_select(const float* score, const int* cu_seqlens, const int* row_src, const float* theta, float* keep, int* counts,
                   float* dense_mask, int B, int T, int total, d2s_stream_t stream);

/* The soft mask of a stage on the dense batch, score and m_in [B, N] (token 0 = CLS; m_in null: all ones): M = sigmoid((score -
 * theta[0]) * inv_tau) at the patches and 1 at CLS, m_out = m_in * M, msum [B] = each image's sum of M over its patches (the
 * regulariser's numerator).  One workgroup per image.
 * D2S_ERR_ARG before any launch: score, theta, M, m_out or msum null; B <= 0; N < 2; inv_tau not > 0. */
int d2s_ltp_soft_mask_fwd(const float* score, const float* m_in, const float* theta, float* M, float* m_out, float* msum, int B, int N,
                          float inv_tau, d2s_stream_t stream);

/* Backward of d2s_ltp_soft_mask_fwd; the score carries no gradient.  g_out [B, N] is the gradient of m_out, greg [B] (optional)
 * the gradient of msum - the regulariser's share per mask entry, lambda / (S B T) times what arrives at the loss, as device values.
 * gM = g_out * m_in + greg[b] at the patches and 0 at CLS; gm_in (optional) = g_out * M, added to what it holds when accumulate_gm;
 * dtheta[0] = -inv_tau * sum over all patches of gM M (1 - M), added to what it holds when accumulate_dtheta.  The sum runs per image
 * in dpart_ws [B] and then over the images in one wave, both in a fixed order.
 * D2S_ERR_ARG before any launch: g_out, M, gM, dtheta or dpart_ws null; B <= 0; N < 2; inv_tau not > 0; a flag not 0 or 1. */
int d2s_ltp_soft_mask_bwd(const float* g_out, const float* M, const float* m_in, const float* greg, float* gM, float* gm_in,
                          float* dtheta, float* dpart_ws, int B, int N, float inv_tau, int accumulate_gm, int accumulate_dtheta,
                          d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_LTP_H */
