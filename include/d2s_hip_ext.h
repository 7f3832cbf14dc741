/* d2s_hip_ext.h - entries of libd2s_hip.so added after d2s_hip.h was frozen.
 *
 * d2s_hip.h is the frozen core of the C ABI: its list of entries no longer changes.  This file holds the two entries that followed it and is
 * closed as well (a later feature brings a header of its own: d2s_hip_squeeze.h); they are declared in the same style
 * (one `int d2s_...(` declaration at the start of a line, one comment per entry) and under d2s_hip.h's conventions: device pointers owned
 * by the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 */
#ifndef D2S_HIP_EXT_H
#define D2S_HIP_EXT_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Token Merging at inference on the bf16 data path ------------------------------------------------------ */

/* d2s_attn_keyw_fwd_f32's attention (key j counts key_w[b,j] times in every softmax row: out_i = sum_j w_j exp(S_ij) v_j / sum_j w_j
 * exp(S_ij), w = key_w [B,n] fp32, >= 1) on the bf16 matrix cores: qkv [B,n,3,H,64] fp32 or bf16 (qkv_is_bf16 != 0: the qkv GEMM's c_bf16;
 * both give the same bits), out [B,n,H*64] fp32 and / or out_bf16 (the projection GEMM's a_bf16) written - at least one; lse [B,H,n] =
 * log of the weighted denominator.  No CLS row.  Always the 32-key-tile kernel on d2s_attn_policy_fwd_bf16's grid; all weights 1.0: bit
 * for bit d2s_attn_fwd_bf16_bf16out where that entry runs the same kernel.  Forward only.  D2S_ERR_ARG before any launch for a null qkv,
 * key_w or lse, both outputs null, B <= 0, H <= 0, n < 2 or n > 8192. */
int d2s_attn_keyw_fwd_bf16(const void* qkv, int qkv_is_bf16, const float* key_w, float* out /* nullable */, void* out_bf16 /* nullable */,
                           float* lse, int B, int n, int H, float scale, d2s_stream_t stream);

/* d2s_tome_match on a bf16 qkv [B,n,3,H,64] (the qkv GEMM's c_bf16, K read in place): every value is widened to fp32 (exact) and the
 * fp32 match runs unchanged, so all five outputs are bit for bit d2s_tome_match's on the widened tensor.  Its outputs, its limits
 * (2 <= n <= 896, H >= 1, 0 <= r <= (n-1)/2, src_idx / dst_idx required iff r > 0) and its refusals. */
int d2s_tome_match_bf16(const void* qkv_bf16, int B, int n, int H, int r, float* node_max, int* node_idx, int* unm_idx, int* src_idx,
                        int* dst_idx, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_EXT_H */
