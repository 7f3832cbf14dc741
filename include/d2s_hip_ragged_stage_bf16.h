/* d2s_hip_ragged_stage_bf16.h - the entries of libd2s_hip.so for training ATS and A-ViT in the bf16 arithmetic mode (train_bf16=True /
 * --ats-train-bf16, --avit-bf16; DESIGN.md sections 24 and 25): the two backward row moves at the points where rows leave the ragged
 * packed batch, each writing the gradient of the rows that entered in fp32 and, rounded once to nearest even, in bf16.
 *
 * d2s_hip.h is the frozen core of the C ABI and every later header is closed as well; these entries follow the same style (one
 * `int d2s_...(` declaration at the start of a line, one comment per entry) and d2s_hip.h's conventions: device pointers owned by the
 * caller, 0 on success or D2S_ERR_* (< 0), nothing throws, nothing allocates, work enqueued on `stream`.  The Python binding
 * lists them under this file's name in its one table, d2s.lib.ABI.
 *
 * Neither entry uses atomics or needs its output cleared: every output element is written exactly once, two launches are bit-identical.
 * Neither needs scratch.  Every segment is clamped to its buffer, so no offset value makes a kernel touch memory outside it.
 */
#ifndef D2S_HIP_RAGGED_STAGE_BF16_H
#define D2S_HIP_RAGGED_STAGE_BF16_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d2s_ragged_repack_bwd (d2s_hip_ragged_train.h) that also writes the bf16 form of every row: g_new [cu_new[B], D], keep [cu_old[B]],
 * cu_old / cu_new [B + 1] as d2s_ragged_repack took them -> g_old [cu_old[B], D] fp32, bit for bit that entry's, and g_old_bf16
 * [cu_old[B], D], the same values rounded once.  One pass: a kept row (the first row of an image always is) takes the row it became, a
 * dropped row and a kept position at or past the new segment's length take zeros, in both forms.  The old segments are clamped to
 * [0, cu_old[B]], the new ones to [0, cu_new[B]].
 * D2S_ERR_ARG before any launch, outputs untouched: a null pointer; B <= 0; D <= 0 or D % 4 != 0. */
int d2s_ragged_repack_bwd_bf16out(const float* g_new, const float* keep, const int* cu_old, const int* cu_new, float* g_old,
                                  void* g_old_bf16, int B, int D, d2s_stream_t stream);

/* The whole backward of an A-ViT block boundary (d2s_hip_avit.h) in one launch: the gradient g_new [cu_new[B], D] of the rows that went
 * on arrives through the re-pack (keep [total], cu_new [B + 1]; all three null: nothing arrived - the last layer, d2s_avit_halt_bwd's
 * fresh = 1), the halting step's own terms are added, and the gradient of the rows that entered the step is written as g_old [total, D]
 * fp32 - bit for bit d2s_ragged_repack_bwd followed by d2s_avit_halt_bwd - and as g_old_bf16 [total, D], the same values rounded once.
 * h, cu_seqlens, row_src, halt_layer, w, dacc, ycls, ysave, gsc, N, layer, L, gamma: as d2s_avit_halt_bwd takes them.
 * D2S_ERR_ARG before any launch, outputs untouched: d2s_avit_halt_bwd's cases (a null h, cu_seqlens, row_src, halt_layer, w, dacc, ycls,
 * ysave or gsc; B, N, D or total <= 0; layer < 1; L < layer or L > 64), a null g_old or g_old_bf16, D % 4 != 0, and g_new, keep and
 * cu_new given only in part. */
int d2s_avit_halt_repack_bwd_bf16out(const float* g_new, const float* keep, const int* cu_new, const float* h, const int* cu_seqlens,
                                     const int* row_src, const int* halt_layer, const float* w, const float* dacc, const float* ycls,
                                     const float* ysave, const float* gsc, float* g_old, void* g_old_bf16, int B, int N, int D, int total,
                                     int layer, int L, float gamma, d2s_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_RAGGED_STAGE_BF16_H */
