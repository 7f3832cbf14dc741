/* d2s_hip_sim_prune.h - the entries of libd2s_hip.so for the similarity stage of an attention-selecting student: among the candidates
 * the importance ranking chose, prune those that resemble a more important candidate most (--sim-prune R).
 *
 * d2s_hip.h is the frozen core of the C ABI and the older d2s_hip_*.h headers are closed as well; these entries follow the same style
 * (one `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by
 * the caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * fp32 only, no atomics, no memset, fixed summation orders: two calls on equal inputs give the same bits.  Every argument error is
 * reported before any launch.
 */
#ifndef D2S_HIP_SIM_PRUNE_H
#define D2S_HIP_SIM_PRUNE_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The key metric of every token of a block, from that block's qkv [B * n, 3, H, 64]: metric [B, n, 64], row t = the mean of token t's
 * keys over the heads (h ascending), divided by its L2 norm - d2s_tome_match's metric, with its rule for a zero row (0 / 0 = NaN, not
 * special-cased).  Only the K third of qkv is read, 16 bytes per lane; one launch.
 * D2S_ERR_ARG before the launch, metric untouched: qkv or metric null; B, n or H <= 0; metric overlapping qkv. */
int d2s_key_metric_f32(const float* qkv, int B, int n, int H, float* metric, d2s_stream_t stream);

/* The similarity stage on one importance ranking.  metric [B, n, 64] as above; scored token t of image b is row lead + t, 0 <= t < T;
 * probs [B, T] and cand [B, c] (int64, ascending) as d2s_select_cls_attn wrote them for c candidates.
 *   The candidates are ordered by probs descending, equal values lowest id first; the c_b = c - c / 2 most important are group B, the
 *   c_a = c / 2 least important group A.  score[a][b] = sum_d metric_a[d] metric_b[d], one summation order for every pair (fp32 matrix
 *   pipe); best[a] = max_b score, partner[a] = the lowest id attaining it (B's lowest id when no comparison succeeded: a NaN row, best
 *   = -inf).  The r members of A with the largest best are pruned, equal values lowest id first (d2s_select_topk's rule).
 *   kept [B, c - r] = the candidates without the pruned ones, dropped [B, T - c + r] = every other scored token, both int64 ascending;
 *   pruned [B, r], partner [B, r] (int64 token ids) and sim [B, r] (= best) in ascending pruned id.
 * r == 0 copies cand to kept; pruned, partner and sim may then be null, as dropped may when T - c + r == 0.
 * Two launches (the match over (32-row tile of A, image), then one workgroup per image), no host synchronisation between them; between
 * the two, the head of every image's kept list holds that image's (best, partner) pairs.
 * D2S_ERR_ARG before any launch, outputs untouched: a null pointer where a list is not empty; B <= 0 or B > 65535; lead < 0;
 * not 1 <= c <= T <= 1024; lead + T > n; not 0 <= r <= c / 2; an output overlapping metric, probs or cand. */
int d2s_sim_prune_f32(const float* metric, const float* probs, const long long* cand, int B, int n, int lead, int T, int c, int r,
                      long long* kept, long long* dropped, long long* pruned, long long* partner, float* sim, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_SIM_PRUNE_H */
