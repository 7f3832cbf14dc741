/* d2s_hip_tome_train_bf16.h - the entries of libd2s_hip.so for training through token merging in the bf16 arithmetic mode
 * (train_bf16=True / --tome-train-bf16): the key-weighted attention backward on the bf16 matrix cores and the merge
 * backward that also writes the bf16 form of the gradient it produces.
 *
 * d2s_hip.h is the frozen core of the C ABI and every later header is closed as well; these entries follow the same style (one
 * `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the
 * caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * Neither entry uses atomics or needs its output cleared: every output element is written exactly once, two launches are bit-identical.
 */
#ifndef D2S_HIP_TOME_TRAIN_BF16_H
#define D2S_HIP_TOME_TRAIN_BF16_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of d2s_attn_keyw_fwd_bf16 (d2s_hip_ext.h): qkv [B, n, 3, H, 64] fp32 or (qkv_is_bf16 != 0) bf16, the c_bf16 of the qkv GEMM -
 * both give identical results; key_w [B, n] fp32 (>= 1); out that entry's fp32 output, lse [B, H, n] as it wrote it (the log of the
 * weighted denominator); dout [B, n, H*64].  dqkv (fp32) and / or dqkv_bf16, both [B, n, 3, H, 64], at least one, fully written, the bf16
 * form the fp32 one rounded once.  delta_ws: [B, H, n] floats of scratch.  The three launches of d2s_attn_bwd_bf16_bf16out (delta, dQ,
 * dK/dV; 32-key tiles) with P_ij = w_j exp(S_ij - lse_i) and then the plain rule: dV = P^T dO, dS = P (dP - delta), dQ = scale dS K,
 * dK = scale dS^T Q.  The weights get no gradient.  With every weight 1.0 and the plain forward's out and lse the outputs are the bits of
 * d2s_attn_bwd_bf16_bf16out.
 * D2S_ERR_ARG before any launch: a null pointer other than one of dqkv / dqkv_bf16; both of those null; B <= 0 or H <= 0; n < 2 or
 * n > 8192. */
int d2s_attn_keyw_bwd_bf16(const void* qkv, int qkv_is_bf16, const float* key_w, const float* out, const float* dout, const float* lse,
                           float* dqkv, void* dqkv_bf16, float* delta_ws, int B, int n, int H, float scale, d2s_stream_t stream);

/* d2s_tome_merge_bwd that also writes the bf16 form of every row: dy [B, n-r, D], size [B, n] or null (all ones), size_out [B, n-r] as the
 * forward wrote it, the forward's plan -> dx [B, n, D] fp32, bit for bit d2s_tome_merge_bwd's, and dx_bf16 [B, n, D], the same values
 * rounded once.  One pass; an even row that the plan names nowhere gets zeros in both forms; r = 0 is the copy plus its rounding.
 * D2S_ERR_ARG before any launch: d2s_tome_merge_bwd's cases (a null dy, size_out, unm_idx or dx; B <= 0; n < 2 or n > 896; D <= 0 or
 * D % 4 != 0; r < 0 or r > (n-1)/2; r > 0 with a null src_idx or dst_idx) and a null dx_bf16. */
int d2s_tome_merge_bwd_bf16out(const float* dy, const float* size, const float* size_out, const int* unm_idx, const int* src_idx,
                               const int* dst_idx, int B, int n, int D, int r, float* dx, void* dx_bf16, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_TOME_TRAIN_BF16_H */
