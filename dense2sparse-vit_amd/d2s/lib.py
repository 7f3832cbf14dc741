"""ctypes binding of lib/libd2s_hip.so, the C ABI that the headers under include/ declare: one table, ABI, with one key per header.

There is no fallback: if the shared object is missing or a symbol cannot be resolved this raises, and every op
raises on a non-zero return code.  Tensors are passed as raw device pointers; the caller keeps them alive and all
work is enqueued on torch's current HIP stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("D2S_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libd2s_hip.so")   # override: diagnostic builds

P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t

# header under include/ -> {entry: (restype, [argtypes])}, headers and entries in the order they were added.  An int-returning entry
# launches: load() appends its trailing d2s_stream_t and call() passes the current stream.  Every other entry is a query without a
# stream, reached through query(): a size_t or long result, or an int one whose argtypes are None (it takes no argument at all).
ABI = {
    "d2s_hip.h": {  # the core
        "d2s_gemm_f32_workspace_bytes": (Z, [I, I, I, I, I]),
        "d2s_gemm_f32": (I, [I, P, L, P, L, P, L, I, I, I, I, P, P, L, P, I, I, I, I, I, P, Z]),
        "d2s_gemm_f32_bf16io": (I, [I, P, L, P, L, P, L, I, I, I, I, P, P, L, P, P, P, P, P, Z]),
        "d2s_convert_bf16": (I, [P, P, L]),
        "d2s_linear_wgrad_workspace_bytes": (Z, [I, I, I, I]),
        "d2s_linear_wgrad_f32": (I, [P, L, P, L, P, L, P, I, I, I, I, I, P, Z]),
        "d2s_linear_wgrad_f32_bf16x": (I, [P, P, L, P, L, P, L, P, I, I, I, I, P, Z]),
        "d2s_batchnorm_workspace_bytes": (Z, [L, I]),
        "d2s_batchnorm_fwd": (I, [P, P, P, P, P, P, P, P, L, I, F, F, I, P, Z]),
        "d2s_batchnorm_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I, L, I, P, Z]),
        "d2s_transpose_f32": (I, [P, P, I, I]),
        "d2s_transpose_batched_f32": (I, [P, P, P, I]),
        "d2s_colsum_workspace_bytes": (Z, [I, I]),
        "d2s_colsum_f32": (I, [P, L, I, I, P, I, P, Z]),
        "d2s_layernorm_fwd": (I, [P, L, L, L, L, P, P, P, P, P, L, I, F]),
        "d2s_layernorm_fwd_bf16out": (I, [P, L, L, L, L, P, P, P, P, P, P, L, I, F]),
        "d2s_layernorm_bwd_workspace_bytes": (Z, [L, I]),
        "d2s_layernorm_bwd": (I, [P, L, L, L, L, P, P, P, P, P, P, P, P, I, I, L, I, P, Z]),
        "d2s_layernorm_bwd_bf16out": (I, [P, L, L, L, L, P, P, P, P, P, P, P, P, P, I, I, L, I, P, Z]),
        "d2s_softmax_rows": (I, [P, P, I, I]),
        "d2s_select_topk": (I, [P, I, I, I, P, P]),
        "d2s_gather_pack_fwd": (I, [P, P, P, I, I, I, I]),
        "d2s_scatter_unpack_bwd": (I, [P, P, P, I, I, I, I]),
        "d2s_gather_fuse_fwd": (I, [P, P, P, P, P, P, I, I, I, I, I]),
        "d2s_gather_fuse_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I]),
        "d2s_select_cls_attn": (I, [P, I, I, I, I, I, I, I, P, P, P]),
        "d2s_tome_match": (I, [P, I, I, I, I, P, P, P, P, P]),
        "d2s_tome_merge": (I, [P, P, P, P, P, I, I, I, I, P, P]),
        "d2s_tome_merge_bwd": (I, [P, P, P, P, P, P, I, I, I, I, P]),
        "d2s_half_mean_concat": (I, [P, P, P, I, I, I]),
        "d2s_im2col_patch": (I, [P, P, I, I, I, I, I]),
        "d2s_fill_cls": (I, [P, P, P, I, I, I]),
        "d2s_batch_sum": (I, [P, P, I, L, L, I]),
        "d2s_copy_rows": (I, [P, L, L, L, L, P, L, L, L, L, L, I, I]),
        "d2s_assemble_tokens": (I, [P, P, P, P, I, I, I]),
        "d2s_softmax_policy_fwd": (I, [P, P, P, I, I, I, F]),
        "d2s_softmax_policy_bwd": (I, [P, P, P, P, I, I, I, F]),
        "d2s_unfold_fwd": (I, [P, L, L, L, L, P, I, I, I, I, I, I, I]),
        "d2s_unfold_bwd": (I, [P, P, L, L, L, L, I, I, I, I, I, I, I]),
        "d2s_performer_workspace_bytes": (Z, [I, I]),
        "d2s_performer_attn_fwd": (I, [P, P, P, P, P, P, P, P, I, I, F, P, Z]),
        "d2s_performer_attn_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, F, P, Z]),
        "d2s_attn_fwd_f32": (I, [P, P, P, P, I, I, I, F]),
        "d2s_attn_fwd_bf16": (I, [P, P, P, P, I, I, I, F]),
        "d2s_attn_fwd_bf16_bf16out": (I, [P, I, P, P, P, P, I, I, I, F]),
        "d2s_attn_bwd_f32": (I, [P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_bwd_bf16": (I, [P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_bwd_bf16_bf16out": (I, [P, I, P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_delta": (I, [P, P, P, I, I, I]),
        "d2s_teacher_target": (I, [P, P, I, I, I, I]),
        "d2s_gather_renorm": (I, [P, P, P, I, I, I, I]),
        "d2s_kl_rows": (I, [P, L, L, L, L, P, L, L, L, L, P, P, P, P, L, I, I, P]),
        "d2s_select_threshold": (I, [P, I, I, F, P, L, I, P]),
        "d2s_gather_rows_i32": (I, [P, P, P, I, I]),
        "d2s_ragged_offsets": (I, [P, I, I, P]),
        "d2s_ragged_pack": (I, [P, P, P, P, P, I, I, I]),
        "d2s_half_mean_concat_varlen": (I, [P, P, P, I, I]),
        "d2s_ragged_select_threshold": (I, [P, P, P, F, I, P, P, P, P, I]),
        "d2s_ragged_repack": (I, [P, P, P, P, P, P, P, I, I]),
        "d2s_mask_row_weights": (I, [P, L, P]),
        "d2s_dense_mask_agreement": (I, [P, P, I, I, P]),
        "d2s_patch_keep_mask": (I, [P, I, I, I, P]),
        "d2s_compose_ids": (I, [P, I, P, I, P, I]),
        "d2s_attn_policy_fwd_f32": (I, [P, P, P, P, P, P, I, I, I, F, F]),
        "d2s_attn_policy_bwd_f32": (I, [P, P, P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_policy_bwd_dpol_f32": (I, [P, P, P, P, P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_policy_fwd_bf16": (I, [P, I, P, P, P, P, P, P, I, I, I, F, F]),
        "d2s_attn_policy_bwd_bf16": (I, [P, I, P, P, P, P, P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_keyw_fwd_f32": (I, [P, P, P, P, I, I, I, F]),
        "d2s_attn_keyw_bwd_f32": (I, [P, P, P, P, P, P, P, I, I, I, F]),
        "d2s_attn_varlen_fwd_f32": (I, [P, P, P, P, I, I, I, I, F]),
        "d2s_attn_varlen_fwd_bf16": (I, [P, I, P, P, P, P, I, I, I, I, F]),
        "d2s_sum_scalar": (I, [P, L, F, P]),
        "d2s_scale_by_scalar": (I, [P, P, F, P, L]),
        "d2s_mask_agreement": (I, [P, P, I, I, I, P]),
        "d2s_act_grad": (I, [P, P, P, L, I]),
        "d2s_normal_noise": (I, [P, L, ctypes.c_ulonglong]),
        "d2s_perturbed_topk_workspace_bytes": (Z, [I, I, I]),
        "d2s_perturbed_topk_fwd": (I, [P, P, P, I, I, I, I, F, P, Z]),
        "d2s_perturbed_topk_bwd": (I, [P, P, P, P, I, I, I, I, F]),
        "d2s_soft_gather_fwd": (I, [P, P, P, I, I, I, I]),
        "d2s_soft_gather_bwd_x": (I, [P, P, P, I, I, I, I]),
        "d2s_soft_gather_bwd_ind": (I, [P, P, P, I, I, I, I]),
        "d2s_softmax_rows_bwd": (I, [P, P, P, I, I]),
        "d2s_block_saved_floats": (L, [I, I, I, I, I, I]),
        "d2s_block_bwd_scratch_floats": (L, [I, I, I, I, I]),
        "d2s_block_workspace_bytes": (Z, [I, I, I, I, I]),
        "d2s_block_wgrad_workspace_bytes": (Z, [I, I, I, I, I]),
        "d2s_block_fwd_f32": (I, [P, P, I, I, I, I, I, F, F, P, P, P, I, I, P, Z]),
        "d2s_block_bwd_f32": (I, [P, P, P, P, P, I, I, I, I, I, F, P, P, P, I, P, Z, P, Z, P]),
        "d2s_drop_path_scales": (I, [P, P, I, I, ctypes.c_ulonglong]),
        "d2s_gemm_f32_rowscale": (I, [I, P, L, P, L, P, L, I, I, I, P, P, L, P, I, I, P, P, P, P, Z]),
        "d2s_scale_rows": (I, [P, P, P, L, I, I]),
        "d2s_drop_path_fwd": (I, [P, P, P, I, L]),
        "d2s_block_bwd_dp_scratch_floats": (L, [I, I, I, I, I]),
        "d2s_block_fwd_f32_dp": (I, [P, P, P, P, I, I, I, I, I, F, F, P, P, P, I, I, P, Z]),
        "d2s_block_bwd_f32_dp": (I, [P, P, P, P, P, P, P, I, I, I, I, I, F, P, P, P, I, P, Z, P, Z, P]),
        "d2s_adamw_chunk_elems": (I, None),
        "d2s_adamw_step": (I, [P, P, P, P, P, I, F, F, F, I, F, P]),
        "d2s_adamw_step_ema": (I, [P, P, P, P, P, I, F, F, F, I, F, P, P, F]),
        "d2s_adamw_step_clip": (I, [P, P, P, P, P, I, F, F, F, I, F, P, P, F, P]),
        "d2s_grad_accumulate": (I, [P, P, P, I, I]),
        "d2s_grad_clip_coef": (I, [P, P, I, F, F, P, P]),
        "d2s_augment_desc_ints": (I, None),
        "d2s_augment_images": (I, [P, L, P, I, I, I, I, I, I, ctypes.c_ulonglong, P, P]),
        "d2s_augment_labels": (I, [P, I, I, F, F, P]),
        "d2s_randaug_max_ops": (I, None),
        "d2s_randaug_op_ints": (I, None),
        "d2s_randaug_scratch_bytes": (Z, [I, I]),
        "d2s_randaug_apply": (I, [P, P, I, I, P, P]),
        "d2s_augment_ops_scratch_bytes": (Z, [I, I]),
        "d2s_augment_images_ops": (I, [P, L, P, P, I, I, I, I, I, I, ctypes.c_ulonglong, P, P, P]),
        "d2s_gumbel_noise": (I, [P, L, ctypes.c_ulonglong]),
        "d2s_gumbel_from_bits": (I, [P, P, L]),
        "d2s_gumbel_keep_fwd": (I, [P, P, P, P, P, P, P, L]),
        "d2s_gumbel_keep_bwd": (I, [P, P, P, P, P, P, L]),
        "d2s_policy_pool_fwd": (I, [P, P, P, P, P, I, I, I]),
        "d2s_policy_pool_bwd": (I, [P, P, P, P, P, P, P, P, I, I, I]),
        "d2s_ratio_rows_fwd": (I, [P, F, P, P, I, I]),
        "d2s_ratio_rows_bwd": (I, [P, P, F, P, I, I]),
    },
    "d2s_hip_ext.h": {  # token merging on the bf16 data path
        "d2s_attn_keyw_fwd_bf16": (I, [P, I, P, P, P, P, I, I, I, F]),
        "d2s_tome_match_bf16": (I, [P, I, I, I, I, P, P, P, P, P]),
    },
    "d2s_hip_squeeze.h": {  # pruning and squeezing, DESIGN.md section 23
        "d2s_squeeze_match": (I, [P, P, P, I, I, I, I, P, P]),
        "d2s_gather_squeeze_fwd": (I, [P, P, P, P, P, I, I, I, I, P, P]),
        "d2s_gather_squeeze_bwd": (I, [P, P, P, P, P, P, I, I, I, I, P]),
    },
    "d2s_hip_ats.h": {  # adaptive token sampling at inference, DESIGN.md section 24
        "d2s_ats_select": (I, [P, P, I, P, P, I, I, I, I, I, I, P, P, P, P]),
    },
    "d2s_hip_ragged_train.h": {  # training through a ragged packed batch, DESIGN.md section 24
        "d2s_attn_varlen_fwd_lse_f32": (I, [P, P, P, P, P, I, I, I, I, F]),
        "d2s_attn_varlen_bwd_f32": (I, [P, P, P, P, P, P, P, I, I, I, I, F]),
        "d2s_ragged_repack_bwd": (I, [P, P, P, P, P, I, I]),
        "d2s_ragged_cls_scatter": (I, [P, P, P, I, I, I]),
    },
    "d2s_hip_ragged_threshold.h": {  # training the dynamic keep ratio on the ragged batch, DESIGN.md section 10.2
        "d2s_half_mean_concat_varlen_bwd": (I, [P, P, P, I, I]),
        "d2s_ragged_mask_loss_fwd": (I, [P, P, P, P, P, I, I, I, I]),
        "d2s_ragged_mask_loss_bwd": (I, [P, P, P, P, P, I, I, I, I, F]),
        "d2s_ragged_teacher_rows": (I, [P, L, P, P, P, P, I, I, I, I]),
    },
    "d2s_hip_avit.h": {  # the A-ViT baseline: per-token adaptive depth on the ragged batch, DESIGN.md section 25
        "d2s_avit_halt": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, F, F]),
        "d2s_avit_halt_bwd": (I, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, F]),
        "d2s_avit_penalty_fwd": (I, [P, P, P, P, P, I, I, I]),
        "d2s_avit_penalty_bwd": (I, [P, P, P, P, P, P, I, I, I]),
    },
    "d2s_hip_evo.h": {  # the Evo-ViT baseline: slow-fast token update, DESIGN.md section 26
        "d2s_evo_select": (I, [P, P, P, P, P, P, I, I, I, I, F]),
        "d2s_evo_scatter_fwd": (I, [P, P, P, P, P, I, I, I, I]),
        "d2s_evo_scatter_bwd": (I, [P, P, P, P, I, I, I, I]),
        "d2s_evo_gather_bwd": (I, [P, P, P, P, P, P, P, I, I, I, I]),
    },
    "d2s_hip_gemm_plan.h": {  # which tile and how many K slices the exact fp32 GEMM runs, DESIGN.md section 7
        "d2s_gemm_f32_plan": (Z, [I, I, I, I, I]),
    },
    "d2s_hip_ragged_bf16.h": {  # training on the ragged batch in the bf16 arithmetic mode, DESIGN.md section 10.3
        "d2s_attn_varlen_fwd_lse_bf16": (I, [P, I, P, P, P, P, P, I, I, I, I, F]),
        "d2s_attn_varlen_bwd_bf16": (I, [P, I, P, P, P, P, P, P, P, I, I, I, I, F]),
    },
    "d2s_hip_ltp.h": {  # the LTP baseline: learned per-block token thresholds, DESIGN.md section 27
        "d2s_ltp_score_workspace_bytes": (Z, [L, I]),
        "d2s_ltp_score_f32": (I, [P, P, P, P, P, P, P, Z, I, I, I, I, F]),
        "d2s_ltp_select": (I, [P, P, P, P, P, P, P, I, I, I]),
        "d2s_ltp_soft_mask_fwd": (I, [P, P, P, P, P, P, I, I, F]),
        "d2s_ltp_soft_mask_bwd": (I, [P, P, P, P, P, P, P, P, I, I, F, I, I]),
    },
    "d2s_hip_tome_train_bf16.h": {  # training through token merging in the bf16 arithmetic mode, DESIGN.md section 22
        "d2s_attn_keyw_bwd_bf16": (I, [P, I, P, P, P, P, P, P, P, I, I, I, F]),
        "d2s_tome_merge_bwd_bf16out": (I, [P, P, P, P, P, P, I, I, I, I, P, P]),
    },
    "d2s_hip_ragged_stage_bf16.h": {  # training ATS and A-ViT in the bf16 arithmetic mode, DESIGN.md sections 24 and 25
        "d2s_ragged_repack_bwd_bf16out": (I, [P, P, P, P, P, P, I, I]),
        "d2s_avit_halt_repack_bwd_bf16out": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, F]),
    },
    "d2s_hip_ltp_bf16.h": {  # the LTP score on the bf16 data path, DESIGN.md section 27
        "d2s_ltp_score_bf16_workspace_bytes": (Z, [L, I]),
        "d2s_ltp_score_bf16": (I, [P, P, P, P, P, P, P, Z, I, I, I, I, F]),
    },
    "d2s_hip_graph_rank.h": {  # token selection by PageRank over the block's attention, DESIGN.md section 29
        "d2s_graph_rank_f32": (I, [P, P, P, P, P, I, I, I, F, I]),
    },
    "d2s_hip_sim_prune.h": {  # the similarity stage after attention ranking, DESIGN.md section 30
        "d2s_key_metric_f32": (I, [P, I, I, I, P]),
        "d2s_sim_prune_f32": (I, [P, P, P, I, I, I, I, I, I, P, P, P, P, P]),
    },
}

_lib = None


class D2SError(RuntimeError):
    pass


def load():
    """Load the library once; raises D2SError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise D2SError(f"{LIB_PATH} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or `make -C dense2sparse-vit_amd/csrc`). The d2s path has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for entries in ABI.values():
        for name, (res, args) in entries.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = [] if args is None else list(args) + ([P] if res is I else [])
    _lib = lib
    return lib


def symbols(header=None):
    """The sorted entry names of one header (its file name under include/), or of all of them."""
    return sorted(ABI[header]) if header is not None else sorted(name for entries in ABI.values() for name in entries)


def signature(name):
    """(restype, argtypes) of an entry as the table holds it: without the stream that load() appends."""
    for entries in ABI.values():
        if name in entries:
            return entries[name]
    raise KeyError(name)


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise D2SError("d2s ops need device tensors (no CPU fallback)")
    return t.data_ptr()


# The host side of a step is ~430 C-ABI calls; at small per-GPU batches (BASELINE config 3: 32 images) and in the bf16 arithmetic mode the
# step is bound by how fast Python can issue them (measured: 12.8 ms of enqueue per 12.8 ms step at B = 32), so the per-call overhead
# matters: the raw handle of torch's current stream comes from the C-level getter (0.3 us; torch.cuda.current_stream().cuda_stream builds
# a Stream object: 8 us), and the bound ctypes functions are looked up once.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)
_fns = {}


def stream():
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _fn(name):
    f = _fns.get(name)
    if f is None:
        f = _fns[name] = getattr(load(), name)
    return f


def call(name, *args):
    """Invoke an int-returning entry point on the current stream; raise on error code."""
    rc = _fn(name)(*args, stream())
    if rc != 0:
        raise D2SError(f"{name} failed with code {rc}")


def query(name, *args):
    return _fn(name)(*args)
