/* d2s_hip_gemm_plan.h - the plan query of the exact fp32 GEMM (csrc/gemm_f32.hip).
 *
 * d2s_hip.h is the frozen core of the C ABI, d2s_hip_ext.h, d2s_hip_squeeze.h, d2s_hip_ats.h, d2s_hip_ragged_train.h,
 * d2s_hip_ragged_threshold.h, d2s_hip_avit.h and d2s_hip_evo.h are closed as well; this entry follows the same style (one declaration at the
 * start of a line, one comment per entry).  It is host arithmetic only: nothing is launched, nothing allocated, no stream is taken.
 * The Python binding
 * lists it under this file's name in its one table, d2s.lib.ABI.
 *
 * Two argument rules of d2s_gemm_f32 that d2s_hip.h does not spell out, both D2S_ERR_ARG before any launch, in every mode:
 *   - layouts 0 / 1 (NT / NN) with accumulate != 0 and an epilogue other than 0 or 8: accumulation IS epilogue 8 (C += A op(B)); it does
 *     not combine with a bias, residual or activation epilogue;
 *   - remap_rows_per_img > 0 with an epilogue other than 7: the output row remap m -> m + (m / rows_per_img + 1) * skip belongs to the
 *     patch embedding's row-add store, no other epilogue applies it.
 */
#ifndef D2S_HIP_GEMM_PLAN_H
#define D2S_HIP_GEMM_PLAN_H

#include "d2s_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What d2s_gemm_f32(layout, ..., M, N, K, ..., mode) launches - for layout 2 also d2s_linear_wgrad_f32 with M = n_out, N = n_in,
 * K = tokens: tile_m | tile_n << 16 | k_slices << 32.  tile_m x tile_n is the workgroup's output tile (128x128, 128x64, 64x128 or
 * 64x64; the weight gradient always 128x128), k_slices the z extent of the grid, i.e. the slice count after the reduction share of a
 * slice was rounded up to whole 16-deep K-steps; with k_slices > 1 the call needs the workspace d2s_gemm_f32_workspace_bytes names and
 * ends in the ordered slab combine.  The launch, the workspace query and this query read tile and slices from one helper.
 * Returns 0 for invalid arguments (layout outside 0..2, mode outside 0..2, M, N or K <= 0) and for the calls csrc/gemm_split.hip runs:
 * layouts 0 / 1 in modes 1 / 2, layout 2 in mode 2 (layout 2 in mode 1 stays on the exact kernel and is answered). */
size_t d2s_gemm_f32_plan(int layout, int M, int N, int K, int mode);

#ifdef __cplusplus
}
#endif

#endif /* D2S_HIP_GEMM_PLAN_H */
