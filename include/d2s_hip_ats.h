/* d2s_hip_ats.h - the entry of libd2s_hip.so for adaptive token sampling at inference (--method ats).
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h and d2s_hip_squeeze.h are closed as well; this entry follows the same style (one
 * `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the
 * caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists it under this file's name in its one table, d2s.lib.ABI.
 *
 * The batch is ragged and packed, as for d2s_ragged_select_threshold: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, the
 * first of them its CLS token, at most max_n rows per image; row_src [total] is the ORIGINAL token index of every row (patch id + 1, 0 at
 * CLS).  Limits: max_n <= 2049, N <= 8192, K <= 4194304.
 */
#ifndef D2S_HIP_ATS_H
#define D2S_HIP_ATS_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One ATS stage's scores and selection, one workgroup per image, for the T non-CLS rows j of the image:
 * a_j = sum_h cls_row[h * total + r_j] (cls_row [H, total]: the CLS softmax row of d2s_attn_varlen_fwd*), v_j = ||V_j||_2 over the H * 64
 * values at column 2 * H * 64 of qkv [total, 3 * H * 64] (fp32, or bf16 with qkv_is_bf16 != 0: widened at the load, the same bits as on the
 * fp32 copy), w_j = a_j v_j, score_j = w_j / sum_j w_j, or 1 / T for every j when that sum is not > 0 or not finite.
 * Selection on the emitted fp32 scores: stable ascending order (equal values lowest index first), c_i = the running sum in that order summed
 * sequentially in fp32, and for k = 0 .. K-1 the first position with c_i >= ((float)(2k+1) / (float)(2K)) * c_{T-1} is picked (division
 * correctly rounded, one multiply); the SET of picked tokens, 1 .. min(K, T) of them, is kept, and CLS always.
 * Outputs, d2s_ragged_select_threshold's: score [total] (0 at CLS rows), keep [total] 0/1 (1 at CLS rows), counts [B] kept non-CLS rows,
 * dense_mask [B, N] (may be null; then N is not read) = 1 at row_src - 1 of every kept row.  An image with T = 0 writes counts = 0, its CLS
 * entries and a zero mask row.  No atomics, nothing read by the host, every element written once.
 * D2S_ERR_ARG before any launch: a null pointer other than dense_mask; B, H, K <= 0; total <= 0; max_n < 1; a limit above exceeded. */
int d2s_ats_select(const float* cls_row, const void* qkv, int qkv_is_bf16, const int* cu_seqlens, const int* row_src, int K, int N, int B,
                   int H, int total, int max_n, float* score, float* keep, int* counts, float* dense_mask, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_ATS_H */
