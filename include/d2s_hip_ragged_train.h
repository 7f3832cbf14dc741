/* d2s_hip_ragged_train.h - the entries of libd2s_hip.so for training through a ragged packed batch (--method ats --ats-train; DESIGN.md
 * section 24, "Training through the stages").
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h, d2s_hip_squeeze.h and d2s_hip_ats.h are closed as well; these entries follow the
 * same style (one `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers
 * owned by the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * The batch is ragged and packed, as for d2s_attn_varlen_fwd_f32: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, the
 * first of them its CLS token, at most max_n rows per image (max_n sizes the grid: any upper bound up to 8192 works); an image of one row
 * (CLS only) is valid.  fp32 only.  No entry uses atomics or needs its output cleared: every output element is written exactly once.
 */
#ifndef D2S_HIP_RAGGED_TRAIN_H
#define D2S_HIP_RAGGED_TRAIN_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d2s_attn_varlen_fwd_f32 that also keeps the log-sum-exp of every softmax row for the backward: qkv [total, 3, H, 64] -> out [total, H*64],
 * lse [H, total] (row cu_seqlens[b] + i of head h at h * total + cu_seqlens[b] + i), cls_row [H, total] (optional).  The same kernel and
 * launch geometry: out and cls_row are bit for bit that entry's.
 * D2S_ERR_ARG before any launch: a null pointer other than cls_row; B, total, max_n, H <= 0; max_n > 8192. */
int d2s_attn_varlen_fwd_lse_f32(const float* qkv, const int* cu_seqlens, float* out, float* lse, float* cls_row, int B, int total, int max_n,
                                int H, float scale, d2s_stream_t stream);

/* Backward of d2s_attn_varlen_fwd_lse_f32 (out, lse as that call wrote them; dout [total, H*64]): dqkv [total, 3, H, 64] is fully written
 * when cu_seqlens covers [0, total).  delta_ws: [H, total] floats of scratch.  d2s_attn_bwd_f32's three launches, the dQ and dK/dV kernels
 * with every image's rows and statistics taken from cu_seqlens and its 128-row tiles counted from the image's own row 0: the rows of an
 * image are bit for bit what d2s_attn_bwd_f32 writes for that image alone.  Inside the kernels a segment is clamped to [0, total) and its
 * length to [0, max_n], so no cu_seqlens is dereferenced outside the buffers (rows past max_n of an image are then left unwritten).
 * D2S_ERR_ARG before any launch: a null pointer; B, total, max_n, H <= 0; max_n > 8192 (the forward entry's refusals); max_n * 3 * H * 64
 * >= 2^32 (H above 2730 at max_n = 8192: the dQ kernel addresses an image's rows with 32-bit element offsets). */
int d2s_attn_varlen_bwd_f32(const float* qkv, const int* cu_seqlens, const float* out, const float* dout, const float* lse, float* dqkv,
                            float* delta_ws, int B, int total, int max_n, int H, float scale, d2s_stream_t stream);

/* Backward of d2s_ragged_repack: g_new [cu_new[B], D] -> g_old [cu_old[B], D]; row cu_old[b] + i of g_old is the row of g_new that old
 * row became when i == 0 or keep[cu_old[b] + i] != 0 (the kept rows of an image keep their order), zeros otherwise.  keep, cu_old and
 * cu_new are the forward's.  One workgroup per image.
 * D2S_ERR_ARG before any launch: a null pointer; B, D <= 0; D not a multiple of 4. */
int d2s_ragged_repack_bwd(const float* g_new, const float* keep, const int* cu_old, const int* cu_new, float* g_old, int B, int D,
                          d2s_stream_t stream);

/* Backward of the head's gather of the CLS rows (d2s_gather_rows_i32 with cu_seqlens as the index): g_cls [B, D] -> g [total, D], row
 * cu_seqlens[b] = g_cls[b], every other row zeros.  One workgroup per image.
 * D2S_ERR_ARG before any launch: a null pointer; B, total, D <= 0; D not a multiple of 4. */
int d2s_ragged_cls_scatter(const float* g_cls, const int* cu_seqlens, float* g, int B, int total, int D, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_RAGGED_TRAIN_H */
