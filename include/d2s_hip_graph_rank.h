/* d2s_hip_graph_rank.h - the entry of libd2s_hip.so for graph ranking: token selection by a weighted PageRank over a block's attention
 * graph (--graph-rank T).
 *
 * d2s_hip.h is the frozen core of the C ABI and the older d2s_hip_*.h headers are closed as well; this entry follows the same style
 * (one `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by
 * the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists it under this file's name in its one table, d2s.lib.ABI.
 *
 * fp32 only, no atomics, no memset, fixed summation orders: two calls on equal inputs give the same bits.  Every argument error is
 * reported before any launch.
 */
#ifndef D2S_HIP_GRAPH_RANK_H
#define D2S_HIP_GRAPH_RANK_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `iters` steps of the unnormalised PageRank iteration over the attention graph of one block, per image and head, from that block's
 * qkv [B * n, 3, H, 64] and the log-sum-exp [B, H, n] its attention forward wrote (d2s_attn_fwd_f32):
 *   P_ij = exp(scale q_i . k_j - lse_i), recomputed as the attention backward recomputes it; every one of the n rows is a node;
 *   s^0 = w0 [B, H, n], or 1 / n everywhere when w0 is null;  s^{t+1}_j = sum_i s^t_i P_ij;  rank [B, H, n] = s^iters.
 * No damping and no renormalisation: the rows of P sum to 1, so every (image, head) keeps the mass of its start vector.  iters = 1
 * with w0 null is the mean attention a token receives, per head.
 * One launch per step: key tile of 128 x (image, head) workgroups on the f32-input matrix pipe, each step reading the vector the step
 * before wrote.  The steps ping-pong between ws [B, H, n] and rank so that the last one writes rank for either parity of iters; ws may
 * be null when iters == 1, and holds s^{iters - 1} afterwards otherwise.  w0 is only read.
 * D2S_ERR_ARG before any launch, rank and ws untouched: qkv, lse or rank null; ws null with iters >= 2; B <= 0; H <= 0; n < 1 or
 * n > 8192; iters < 1 or iters > 1024; w0 the same pointer as rank or ws. */
int d2s_graph_rank_f32(const float* qkv, const float* lse, const float* w0, float* rank, float* ws, int B, int n, int H, float scale,
                       int iters, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_GRAPH_RANK_H */
