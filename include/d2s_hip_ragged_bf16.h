/* d2s_hip_ragged_bf16.h - the entries of libd2s_hip.so for training through a ragged packed batch in the bf16 arithmetic mode
 * (--ragged-train --ragged-bf16): varlen attention with its log-sum-exp, and its backward, on the bf16 matrix cores.
 *
 * d2s_hip.h is the frozen core of the C ABI and every later header is closed as well; these entries follow the same style (one
 * `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the
 * caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * The batch is ragged and packed, as for d2s_attn_varlen_fwd_bf16: image b owns rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of `total`, the
 * first of them its CLS token, at most max_n rows per image (max_n sizes the grid: any upper bound up to 8192 works); an image of one row
 * (CLS only) is valid.  qkv is fp32 or (qkv_is_bf16 != 0) bf16, the c_bf16 of the qkv GEMM: both give identical results.  Neither entry
 * uses atomics or needs its output cleared: every output element is written exactly once, two launches are bit-identical.
 */
#ifndef D2S_HIP_RAGGED_BF16_H
#define D2S_HIP_RAGGED_BF16_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d2s_attn_varlen_fwd_bf16 that also keeps the log-sum-exp of every softmax row for the backward: qkv [total, 3, H, 64] -> out (fp32)
 * [total, H*64] and / or out_bf16, at least one; lse [H, total] (row cu_seqlens[b] + i of head h at h * total + cu_seqlens[b] + i, the
 * layout of d2s_attn_varlen_fwd_lse_f32) = m + log(l); cls_row [H, total] (optional).  The 32-key-tile kernel and that entry's launch
 * geometry: out, out_bf16 and cls_row are bit for bit that entry's.
 * D2S_ERR_ARG before any launch: a null qkv, cu_seqlens or lse; out and out_bf16 both null; B, total, max_n, H <= 0; max_n > 8192. */
int d2s_attn_varlen_fwd_lse_bf16(const void* qkv, int qkv_is_bf16, const int* cu_seqlens, float* out, void* out_bf16, float* lse, float* cls_row,
                                 int B, int total, int max_n, int H, float scale, d2s_stream_t stream);

/* Backward of d2s_attn_varlen_fwd_lse_bf16 (out its fp32 output, lse as that call wrote them; dout [total, H*64]): dqkv (fp32) and / or
 * dqkv_bf16, both [total, 3, H, 64], at least one; fully written when cu_seqlens covers [0, total).  delta_ws: [H, total] floats of scratch.
 * d2s_attn_bwd_bf16_bf16out's three launches, the dQ and dK/dV kernels with every image's rows and statistics taken from cu_seqlens and
 * its 128-row tiles counted from the image's own row 0: the rows of an image are bit for bit what d2s_attn_bwd_bf16_bf16out writes for
 * that image alone (B = 1, n = its length), in both forms; an image of one row gets dQ = dK = 0 exactly (one key: the softmax row is
 * constant), as that entry writes at n = 1.  Inside the kernels a segment is clamped to [0, total) and its length to
 * [0, max_n], so no cu_seqlens is dereferenced outside the buffers (rows past max_n of an image are then left unwritten).  64-bit
 * offsets: no panel limit.
 * D2S_ERR_ARG before any launch: a null pointer other than one of dqkv / dqkv_bf16; both of those null; B, total, max_n, H <= 0;
 * max_n > 8192. */
int d2s_attn_varlen_bwd_bf16(const void* qkv, int qkv_is_bf16, const int* cu_seqlens, const float* out, const float* dout, const float* lse,
                             float* dqkv, void* dqkv_bf16, float* delta_ws, int B, int total, int max_n, int H, float scale, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_RAGGED_BF16_H */
