/* d2s_hip_squeeze.h - the entries of libd2s_hip.so for pruning and squeezing (--squeeze-dropped).
 *
 * d2s_hip.h is the frozen core of the C ABI and d2s_hip_ext.h is closed as well; these entries follow the same style (one `int d2s_...(`
 * declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the caller, 0 on
 * success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * Common to the three: x [B,n,D] fp32 is one stage's input, [CLS | T scored tokens] with n = T + 1; kept [B,k] and dropped [B,m], m = T - k,
 * are the selector's int64 stage-relative ids; a plan is dst [B,m] int32 (a POSITION in kept, not a token id) and sim [B,m] fp32.
 * D2S_ERR_ARG before any launch for B <= 0 or B > 65535, n < 2 or n > 4096, k < 1 or k > T, D not a multiple of 64 or above 1024, and
 * for a null pointer (dropped, dst and sim may be null when m == 0: they are empty).  An id outside [0, T) or a dst outside [0, k)
 * contributes nothing and is never dereferenced.  Fixed-order sums: results are bit-identical run to run.
 */
#ifndef D2S_HIP_SQUEEZE_H
#define D2S_HIP_SQUEEZE_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The plan: with r_t = 1 / ||x[b,1+t]||_2 (0 for a zero norm), c_ij = <x[b,1+dropped_i], x[b,1+kept_j]> r_dropped_i r_kept_j, all fp32:
 * sim[b,i] = max_j c_ij and dst[b,i] = the lowest j that attains it.  Bit-identical kept rows give bit-identical c_ij, so a duplicate
 * resolves to the lower position.  Grid (32 dropped rows, image); the m x k matrix is never written.  dst = -1, sim = 0 for a dropped id
 * outside [0, T) or when no kept id is valid.  m == 0: returns 0 without a launch. */
int d2s_squeeze_match(const float* x, const long long* kept, const long long* dropped, int B, int n, int k, int D, int* dst, float* sim,
                      d2s_stream_t stream);

/* The stage's output y [B,k+1,D] and Z [B,k] in one launch: y[b,0] = x[b,0]; with w_i = expf(sim[b,i]) and E = expf(1.0f),
 * Z[b,j] = E + sum_{i: dst[b,i] = j} w_i and y[b,1+j] = (E x[b,1+kept_j] + sum_i w_i x[b,1+dropped_i]) / Z[b,j], the row itself first, then
 * the sources in ascending i.  A kept row without a source is copied bit for bit (Z = E); m == 0 gives d2s_gather_pack_fwd's bits. */
int d2s_gather_squeeze_fwd(const float* x, const long long* kept, const long long* dropped, const int* dst, const float* sim, int B, int n,
                           int k, int D, float* y, float* Z, d2s_stream_t stream);

/* The backward in x with the plan held constant, g [B,k+1,D] -> dx [B,n,D], every row written exactly once by the one launch (no memset,
 * no atomics): dx[b,0] = g[b,0]; a kept token gets (E / Z_j) g[b,1+j], or g[b,1+j] bit for bit when it had no source (Z_j == E); a dropped
 * token gets (w_i / Z_dst) g[b,1+dst_i]; a token in neither list gets zeros.  Z is the forward's. */
int d2s_gather_squeeze_bwd(const float* g, const long long* kept, const long long* dropped, const int* dst, const float* sim,
                           const float* Z, int B, int n, int k, int D, float* dx, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_SQUEEZE_H */
