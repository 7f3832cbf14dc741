/* d2s_hip_ltp_bf16.h - the entries of libd2s_hip.so for the LTP baseline in the bf16 arithmetic mode: the attention a token receives,
 * rebuilt on the bf16 matrix cores from the operands the bf16 attention kernels multiply ("In the bf16 arithmetic
 * mode").
 *
 * d2s_hip.h is the frozen core of the C ABI and the older d2s_hip_*.h headers are closed as well, and so is this one at its two entries;
 * they follow the same style (one `int d2s_...(` or `size_t d2s_...(` declaration at the start of a line, one comment per entry) and
 * d2s_hip.h's conventions: device pointers owned by the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work
 * enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * No atomics, no memset, fixed summation orders: two launches on equal inputs give the same bits.  Every argument error is D2S_ERR_ARG
 * and is reported before any launch, and a segment of a packed batch is clamped to [0, total) inside the kernels, so nothing is
 * dereferenced outside the buffers whatever cu_seqlens holds.
 */
#ifndef D2S_HIP_LTP_BF16_H
#define D2S_HIP_LTP_BF16_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace d2s_ltp_score_bf16 needs for `rows` token rows (B * n, or total) and H heads: the per-head partial column sums.
 * 0 for rows <= 0 or H <= 0.  No stream, nothing launched. */
size_t d2s_ltp_score_bf16_workspace_bytes(long rows, int H);

/* d2s_ltp_score_f32's quantity on the bf16 data path: qkv is bf16 [rows, 3, H, 64] (the qkv GEMM's bf16 output) and lse (and cinv) is
 * what the bf16 attention forward wrote from it.  score[j] = sum_h sum_i w_i P[h, i, j] / (H sum_i w_i) per image, fp32, with P
 * recomputed as the bf16 attention backward recomputes it: S = q . bf16(fp32(k) * scale) on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation, P~ = 2^(fma(S, log2 e, -lse log2 e)).  Each image's scores sum to 1.  Three forms, chosen by the pointers:
 *   plain   policy, cinv, cu_seqlens null: B images of n rows, total = B * n, lse [B, H, n] (d2s_attn_fwd_bf16_bf16out), P = P~, w = 1;
 *   policy  policy [B, n] and cinv [B, H, n] given, cu_seqlens null: lse, cinv as d2s_attn_policy_fwd_bf16 wrote them for this policy,
 *           P_ij = P~_ij mk_ij + cinv_i with mk_ij = policy_j off the diagonal and 1 on it, w_i = policy_i (eps is inside lse and cinv);
 *           with an all-ones policy and eps = 0 the result is bit for bit the plain form's;
 *   varlen  cu_seqlens [B + 1] given, policy and cinv null: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, lse
 *           [H, total] (d2s_attn_varlen_fwd_lse_bf16), n is max_n, any upper bound of the longest image; on equal lengths the result is
 *           bit for bit the plain form's, and every image's rows are the bits of the plain form on that image alone.  Rows no segment
 *           covers are left untouched.
 * score [rows] is written once at every row, the CLS entry with its true value.  Two launches: key tile x (image, head) workgroups
 * writing per-head partials into the workspace, then one workgroup per image that folds the heads in ascending order and divides once.
 * D2S_ERR_ARG before any launch: qkv, lse, score or workspace null; B, n, total, H <= 0; n > 8192 (the bf16 varlen attention's limit);
 * workspace_bytes < d2s_ltp_score_bf16_workspace_bytes(total, H); one of policy / cinv without the other; a policy together with
 * cu_seqlens; total != B * n without cu_seqlens. */
int d2s_ltp_score_bf16(const void* qkv, const float* lse, const float* policy, const float* cinv, const int* cu_seqlens, float* score,
                       void* workspace, size_t workspace_bytes, int B, int n, int total, int H, float scale, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_LTP_BF16_H */
