"""ctypes binding of libidb_kernels.so (the C ABI declared in include/idb_kernels.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C faceposegenerator_amd/csrc``.
There is no fallback: if the shared object is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# IDB_LIB selects another build of the same ABI (measurement tools: the profiling library libidb_kernels_prof.so, `make prof`)
LIB_PATH = os.environ.get("IDB_LIB") or os.path.join(_HERE, "libidb_kernels.so")

IDB_BF16, IDB_F16, IDB_F32 = 0, 1, 2
IDB_MAX_SRC = 4
IDB_PLMS_SLOTS = 4
IDB_PLMS_KEEP, IDB_PLMS_SAVE, IDB_PLMS_RESTORE = 0, 1, 2
IDB_HEAD_COSFACE, IDB_HEAD_ARCFACE, IDB_HEAD_ADAFACE = 0, 1, 2
IDB_HEAD_SGD_WS_BYTES = 8192
IDB_SGD_CLIP_WS_BYTES = 65536
IDB_SGD_CLIP_MAX_TENSORS = 8
IDB_ATTN_BWD_KEY_BLOCK, IDB_ATTN_BWD_SLICE, IDB_ATTN_BWD_FULL_GRID = 128, 32, 128
IDB_LORA_MAX_RANK, IDB_LORA_GRAD_CHUNK_ROWS, IDB_LORA_GRAD_MAX_CHUNKS = 16, 32, 256
IDB_ADAMW_TABLE_MAX = 1024
IDB_PAIR_DIST2, IDB_PAIR_KNN, IDB_PAIR_PRDC, IDB_PAIR_NEAREST, IDB_PAIR_POLY = 0, 1, 2, 3, 4
# the selected points of idb_verif_roc, in the order of its points / ints outputs
IDB_VERIF_POINTS = ("eer_t2", "eer_t1", "fmr0", "fmr1000", "fmr100", "fmr20", "fmr10", "fnmr0", "fnmr100", "fnmr1000", "youden", "mcc", "first")

# every symbol include/idb_kernels.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "idb_version", "idb_launch_count", "idb_last_error", "idb_device_check",
    "idb_gemm_workspace_bytes", "idb_gemm_plan", "idb_gemm_row_stats_tiles", "idb_gemm_folds_layernorm", "idb_gemm_fuses_groupnorm", "idb_gemm_emits_gn_partials", "idb_gemm",
    "idb_pack_conv_weight", "idb_pack_matrix", "idb_tiled_weight_bytes", "idb_tile_weight", "idb_lora_merge", "idb_lora_merge_scaled", "idb_pack_matrix_scaled", "idb_ln_fold_vectors",
    "idb_groupnorm_workspace_bytes", "idb_groupnorm", "idb_groupnorm_plan", "idb_layernorm", "idb_groupnorm_stats",
    "idb_attention", "idb_attention_plan", "idb_embed_tokens", "idb_softmax_rows",
    "idb_timestep_sinusoid", "idb_linear_f32", "idb_conv_in",
    "idb_cfg_ddpm_step", "idb_cfg_plms_step", "idb_postprocess",
    "idb_nhwc_to_nchw_f32", "idb_f32_nhwc_to_nchw", "idb_cast_f32", "idb_vae_sample", "idb_warp_affine_u8",
    "idb_crop_resize_area_u8", "idb_conv2d_f32", "idb_maxpool2d_f32", "idb_softmax_pairs_f32", "idb_nms_mask",
    "idb_quantize_fp8", "idb_pack_weight_fp8", "idb_gemm_fp8", "idb_groupnorm_fp8",
    "idb_arcface_stem", "idb_arcface_head_workspace_bytes", "idb_arcface_head",
    "idb_resize_aa_u8", "idb_pose_stem", "idb_pose_head",
    "idb_resize_bicubic_aa_u8", "idb_vit_patchify", "idb_vit_tokens", "idb_vit_head",
    "idb_pair_workspace_bytes", "idb_pair_dist2", "idb_pair_knn_radii", "idb_pair_prdc_counts", "idb_pair_nearest", "idb_pair_poly_sums",
    "idb_verif_cos_scores", "idb_verif_workspace_bytes", "idb_verif_roc",
    "idb_frb_pair_dist", "idb_frb_workspace_bytes", "idb_frb_fold_counts",
    "idb_resize_linear_u8", "idb_fiqa_tail",
    "idb_diffuse_targets", "idb_objective_workspace_bytes", "idb_objective_mse_x0", "idb_crop_resize_bilinear_f32", "idb_crop_resize_area_f32",
    "idb_identity_losses",
    "idb_randaug",
    "idb_head_pack", "idb_head_workspace_bytes", "idb_head_loss", "idb_head_logits",
    "idb_head_grad_workspace_bytes", "idb_head_loss_grad", "idb_head_sgd_step",
    "idb_tail_workspace_bytes", "idb_tail_forward", "idb_tail_backward", "idb_sgd_clip_step",
    "idb_blk_conv_workspace_bytes", "idb_blk_conv_forward", "idb_blk_conv_dgrad", "idb_blk_conv_wgrad",
    "idb_blk_bn_workspace_bytes", "idb_blk_bn_forward", "idb_blk_bn_backward", "idb_blk_affine", "idb_blk_pack_images",
    "idb_sgd_clip_table_workspace_bytes", "idb_sgd_clip_step_table",
    "idb_attention_fwd_train", "idb_attention_bwd_workspace_bytes", "idb_attention_bwd_plan", "idb_attention_bwd",
    "idb_lora_grad_workspace_bytes", "idb_lora_grad",
    "idb_layernorm_bwd", "idb_geglu_fwd", "idb_geglu_bwd", "idb_adamw_clip_table_workspace_bytes", "idb_adamw_clip_step_table",
    "idb_groupnorm_bwd_workspace_bytes", "idb_groupnorm_bwd_plan", "idb_groupnorm_bwd",
]


class GemmSrc(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("channels", C.c_int32), ("taps", C.c_int32),
                ("in_h", C.c_int32), ("in_w", C.c_int32), ("upsample", C.c_int32)]


class GemmDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("batch", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("stride", C.c_int32), ("n", C.c_int32), ("nsrc", C.c_int32),
                ("src", GemmSrc * IDB_MAX_SRC),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("sample_bias", C.c_void_p),
                ("sample_bias_ld", C.c_int32), ("residual", C.c_void_p), ("geglu", C.c_int32),
                ("out", C.c_void_p), ("out_dtype", C.c_int32), ("out_ld", C.c_int32),
                ("split_k", C.c_int32), ("tile", C.c_int32), ("out_scale", C.c_float), ("flags", C.c_int32), ("act", C.c_int32),
                ("counters", C.c_void_p), ("counters_len", C.c_int32), ("gn_partials", C.c_void_p), ("gn_groups", C.c_int32),
                ("row_stats_out", C.c_void_p), ("ln_stats", C.c_void_p), ("ln_tiles", C.c_int32), ("ln_u", C.c_void_p),
                ("ln_v", C.c_void_p), ("ln_eps", C.c_float), ("pad_mode", C.c_int32), ("w_layout", C.c_int32),
                ("w_groups", C.c_int32), ("w_group_rows", C.c_int32), ("w_group_stride", C.c_int64),
                ("gn_in_partials", C.c_void_p), ("gn_in_chunks", C.c_int32), ("gn_in_groups", C.c_int32), ("gn_in_nsrc", C.c_int32),
                ("gn_in_silu", C.c_int32), ("gn_in_eps", C.c_float), ("gn_in_gamma", C.c_void_p), ("gn_in_beta", C.c_void_p),
                ("act_slope", C.c_void_p), ("out2", C.c_void_p), ("out2_scale", C.c_void_p), ("out2_shift", C.c_void_p)]


class GemmFp8Desc(C.Structure):
    _fields_ = [("out_dtype", C.c_int32), ("batch", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("stride", C.c_int32),
                ("n", C.c_int32), ("x", C.c_void_p), ("channels", C.c_int32), ("taps", C.c_int32), ("in_h", C.c_int32),
                ("in_w", C.c_int32), ("upsample", C.c_int32), ("x_scale", C.c_float), ("w", C.c_void_p), ("w_scale", C.c_void_p),
                ("bias", C.c_void_p), ("sample_bias", C.c_void_p), ("sample_bias_ld", C.c_int32), ("residual", C.c_void_p),
                ("out", C.c_void_p), ("out_ld", C.c_int32), ("gn_partials", C.c_void_p), ("gn_groups", C.c_int32)]


class HeadDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("b", C.c_int32), ("d", C.c_int32), ("c", C.c_int32),
                ("s", C.c_double), ("m", C.c_double), ("h", C.c_double), ("t_alpha", C.c_double),
                ("emb", C.c_void_p), ("norms", C.c_void_p), ("label", C.c_void_p), ("kernel", C.c_void_p),
                ("wn", C.c_void_p), ("col_norm", C.c_void_p), ("ada_state", C.c_void_p)]


class TailDesc(C.Structure):
    _fields_ = [("b", C.c_int32), ("ch", C.c_int32), ("hw", C.c_int32), ("n", C.c_int32), ("x_dtype", C.c_int32), ("training", C.c_int32),
                ("p", C.c_double), ("eps2", C.c_double), ("eps1", C.c_double), ("momentum", C.c_double),
                ("x", C.c_void_p), ("keep", C.c_void_p), ("bn2_weight", C.c_void_p), ("bn2_bias", C.c_void_p), ("bn2_mean", C.c_void_p),
                ("bn2_var", C.c_void_p), ("fc_weight", C.c_void_p), ("fc_bias", C.c_void_p), ("feat_weight", C.c_void_p),
                ("feat_bias", C.c_void_p), ("feat_mean", C.c_void_p), ("feat_var", C.c_void_p)]


class BlkConvDesc(C.Structure):
    _fields_ = [("b", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("x", C.c_void_p), ("affine", C.c_void_p), ("slope", C.c_void_p), ("weight", C.c_void_p)]


class IdbError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared object (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise IdbError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"or `make -C faceposegenerator_amd/csrc` (there is no CPU fallback)")
    # torch ships its own libamdhip64 under the same soname: loaded after torch, the library binds to torch's HIP runtime; loaded
    # before it, the process maps two HIP (and HSA) runtimes and the one initialised second finds no device
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    sig = {
        "idb_version": (C.c_int, []),
        "idb_launch_count": (C.c_uint64, []),
        "idb_last_error": (C.c_char_p, []),
        "idb_device_check": (C.c_int, [C.c_int]),
        "idb_gemm_workspace_bytes": (sz, [C.POINTER(GemmDesc)]),
        "idb_gemm_plan": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "idb_gemm": (C.c_int, [C.POINTER(GemmDesc), vp, sz, vp]),
        "idb_gemm_row_stats_tiles": (i32, [C.POINTER(GemmDesc)]),
        "idb_gemm_folds_layernorm": (i32, [C.POINTER(GemmDesc)]),
        "idb_gemm_fuses_groupnorm": (i32, [C.POINTER(GemmDesc)]),
        "idb_gemm_emits_gn_partials": (i32, [C.POINTER(GemmDesc), i32]),
        "idb_lora_merge_scaled": (C.c_int, [vp, vp, vp, vp, i64, i64, i32, f32, vp, i32, vp]),
        "idb_pack_conv_weight": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "idb_pack_matrix": (C.c_int, [vp, vp, i64, i64, i32, i32, vp]),
        "idb_pack_matrix_scaled": (C.c_int, [vp, vp, i64, i64, i32, vp, i32, vp]),
        "idb_ln_fold_vectors": (C.c_int, [vp, vp, vp, i32, f32, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]),
        "idb_tiled_weight_bytes": (sz, [i64, i64]),
        "idb_tile_weight": (C.c_int, [vp, vp, i64, i64, i32, vp]),
        "idb_lora_merge": (C.c_int, [vp, vp, vp, vp, i64, i64, i32, f32, i32, vp]),
        "idb_groupnorm_workspace_bytes": (sz, [i32, i32, i32]),
        "idb_groupnorm": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, f32, vp, vp, i32, vp, i32, vp, sz, vp, i32, vp, i32, vp]),
        "idb_groupnorm_plan": (C.c_int, [i32] * 7 + [C.POINTER(i32)] * 7),
        "idb_layernorm": (C.c_int, [vp, vp, i64, i32, f32, vp, vp, i32, vp]),
        "idb_groupnorm_stats": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, vp, sz, C.POINTER(i32), i32, vp]),
        "idb_attention": (C.c_int, [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, f32, i32, i32, vp]),
        "idb_attention_plan": (C.c_int, [i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "idb_embed_tokens": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "idb_softmax_rows": (C.c_int, [vp, i64, i32, i32, vp]),
        "idb_timestep_sinusoid": (C.c_int, [vp, vp, i32, i32, vp]),
        "idb_linear_f32": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "idb_conv_in": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, i32, vp]),
        "idb_cfg_ddpm_step": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        "idb_cfg_plms_step": (C.c_int, [vp, vp, vp, vp, vp] + [i32] * 11 + [vp]),
        "idb_postprocess": (C.c_int, [vp, vp, vp, i64, vp]),
        "idb_nhwc_to_nchw_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "idb_f32_nhwc_to_nchw": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "idb_cast_f32": (C.c_int, [vp, vp, i64, i32, vp]),
        "idb_vae_sample": (C.c_int, [vp, vp, f32, vp, vp, vp, i32, i32, i32, vp]),
        "idb_warp_affine_u8": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp]),
        "idb_crop_resize_area_u8": (C.c_int, [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, f32, f32, vp]),
        "idb_conv2d_f32": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        "idb_maxpool2d_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "idb_softmax_pairs_f32": (C.c_int, [vp, vp, i32, i32, vp]),
        "idb_nms_mask": (C.c_int, [vp, vp, i32, C.c_float, i32, i32, vp, vp]),
        "idb_quantize_fp8": (C.c_int, [vp, vp, i64, f32, i32, vp]),
        "idb_pack_weight_fp8": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "idb_gemm_fp8": (C.c_int, [C.POINTER(GemmFp8Desc), vp]),
        "idb_groupnorm_fp8": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, f32, vp, vp, i32, vp, f32, i32, vp, sz, vp, i32, vp]),
        "idb_arcface_stem": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
        "idb_arcface_head_workspace_bytes": (sz, [i32, i32, i32]),
        "idb_arcface_head": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "idb_resize_aa_u8": (C.c_int, [vp, i32, i32, i32, i32, vp, vp]),
        "idb_pose_stem": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
        "idb_pose_head": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp]),
        "idb_resize_bicubic_aa_u8": (C.c_int, [vp, i32, i32, i32, vp, vp]),
        "idb_vit_patchify": (C.c_int, [vp, i32, i32, vp, i32, vp]),
        "idb_vit_tokens": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "idb_vit_head": (C.c_int, [vp, i64, i32, i32, vp, vp, f32, vp, i32, vp]),
        "idb_pair_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "idb_pair_dist2": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
        "idb_pair_knn_radii": (C.c_int, [vp, i32, i32, vp, i32, vp, vp, sz, vp]),
        "idb_pair_prdc_counts": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "idb_pair_nearest": (C.c_int, [vp, i32, vp, i32, i32, vp, i32, vp, vp, vp, sz, vp]),
        "idb_pair_poly_sums": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, i32, i32, f32, f32, vp, vp, sz, vp]),
        "idb_verif_cos_scores": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp]),
        "idb_verif_workspace_bytes": (sz, [i32, i32]),
        "idb_verif_roc": (C.c_int, [vp, i32, vp, i32, vp, vp, vp, vp, sz, vp]),
        "idb_frb_pair_dist": (C.c_int, [vp, vp, i32, i32, vp, vp, vp]),
        "idb_frb_workspace_bytes": (sz, [i32, i32, i32]),
        "idb_frb_fold_counts": (C.c_int, [vp, vp, i32, vp, i32, vp, i32, vp, vp, sz, vp]),
        "idb_resize_linear_u8": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        "idb_fiqa_tail": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "idb_diffuse_targets": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
        "idb_objective_workspace_bytes": (sz, [i32, i64]),
        "idb_objective_mse_x0": (C.c_int, [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
        "idb_crop_resize_bilinear_f32": (C.c_int, [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, vp]),
        "idb_crop_resize_area_f32": (C.c_int, [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, f32, f32, vp]),
        "idb_identity_losses": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "idb_randaug": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]),
        "idb_head_pack": (C.c_int, [vp, i32, i32, vp, vp, vp, vp]),
        "idb_head_workspace_bytes": (sz, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "idb_head_loss": (C.c_int, [C.POINTER(HeadDesc), vp, vp, vp, vp, vp, sz, vp]),
        "idb_head_logits": (C.c_int, [C.POINTER(HeadDesc), vp, vp, vp, sz, vp]),
        "idb_head_grad_workspace_bytes": (sz, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "idb_head_loss_grad": (C.c_int, [C.POINTER(HeadDesc), vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "idb_head_sgd_step": (C.c_int, [vp, vp, vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double, i32, vp, vp, vp, vp, vp, sz,
                                        vp]),
        "idb_tail_workspace_bytes": (sz, [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "idb_tail_forward": (C.c_int, [C.POINTER(TailDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "idb_tail_backward": (C.c_int, [C.POINTER(TailDesc)] + [vp] * 8 + [i32] + [vp] * 7 + [sz, vp]),
        "idb_sgd_clip_step": (C.c_int, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)] + [C.c_double] * 4 + [i32, vp, vp, sz,
                                        vp]),
        "idb_blk_conv_workspace_bytes": (sz, [i32] * 7 + [C.POINTER(i32), C.POINTER(i32)]),
        "idb_blk_conv_forward": (C.c_int, [C.POINTER(BlkConvDesc), vp, vp]),
        "idb_blk_conv_dgrad": (C.c_int, [C.POINTER(BlkConvDesc), vp, vp, vp]),
        "idb_blk_conv_wgrad": (C.c_int, [C.POINTER(BlkConvDesc), vp, vp, vp, sz, vp]),
        "idb_blk_bn_workspace_bytes": (sz, [i64, i32, C.POINTER(i32)]),
        "idb_blk_bn_forward": (C.c_int, [vp, i64, i32, i32, C.c_double, C.c_double] + [vp] * 8 + [sz, vp]),
        "idb_blk_bn_backward": (C.c_int, [vp, vp, i64, i32] + [vp] * 10 + [sz, vp]),
        "idb_blk_affine": (C.c_int, [vp] * 5 + [i64, i32, vp, vp]),
        "idb_blk_pack_images": (C.c_int, [vp, i32, i32, i32, vp, vp]),
        "idb_sgd_clip_table_workspace_bytes": (sz, [i32]),
        "idb_sgd_clip_step_table": (C.c_int, [i32, vp, vp, vp, vp] + [C.c_double] * 4 + [i32, vp, vp, sz, vp]),
        "idb_attention_fwd_train": (C.c_int, [vp, i32, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, vp]),
        "idb_attention_bwd_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "idb_attention_bwd_plan": (C.c_int, [i32, i32, i32, i32] + [C.POINTER(i32)] * 4),
        "idb_attention_bwd": (C.c_int, [vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, i32, vp, sz, i32, i32, i32, i32, i32, f32,
                                        i32, vp]),
        "idb_lora_grad_workspace_bytes": (sz, [i64, i32, i32, i32]),
        "idb_lora_grad": (C.c_int, [vp, i32, vp, i32, vp, vp, vp, vp, i64, i32, i32, i32, f32, vp, sz, i32, vp]),
        "idb_layernorm_bwd": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, f32, i32, vp]),
        "idb_geglu_fwd": (C.c_int, [vp, i32, vp, i64, i32, i32, vp]),
        "idb_geglu_bwd": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, vp]),
        "idb_adamw_clip_table_workspace_bytes": (sz, [i32]),
        "idb_adamw_clip_step_table": (C.c_int, [i32, vp, vp, vp, vp, vp] + [C.c_double] * 7 + [i64, vp, vp, vp, sz, vp]),
        "idb_groupnorm_bwd_workspace_bytes": (sz, [i32, i32, i32]),
        "idb_groupnorm_bwd_plan": (C.c_int, [i32] * 5 + [C.POINTER(i32)] * 5),
        "idb_groupnorm_bwd": (C.c_int, [vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, f32, i32, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().idb_last_error()
        raise IdbError(f"{what or 'idb call'} failed (status {rc}): {msg.decode() if msg else ''}")


# descriptor fields gemm_desc takes by name (everything but the positional ones)
_DESC_FIELDS = frozenset(name for name, _ in GemmDesc._fields_) - {"dtype", "batch", "out_h", "out_w", "n", "nsrc", "src", "w"}


def gemm_desc(dtype: int, srcs, w_ptr, n: int, batch: int, oh: int, ow: int, **fields) -> GemmDesc:
    """The one place the package fills an idb_gemm_desc.  srcs: [(ptr, channels, taps, in_h, in_w[, upsample])]; every other
    field of the descriptor by name (stride defaults to 1, out_dtype to dtype, out_ld to n; pointers as addresses or None)."""
    unknown = set(fields) - _DESC_FIELDS
    if unknown:
        raise TypeError(f"gemm_desc: unknown idb_gemm_desc field(s) {sorted(unknown)}")
    if len(srcs) > IDB_MAX_SRC:
        raise ValueError(f"gemm_desc: {len(srcs)} sources, idb_gemm takes at most {IDB_MAX_SRC}")
    d = GemmDesc()
    d.dtype, d.batch, d.out_h, d.out_w, d.stride, d.n, d.nsrc = dtype, batch, oh, ow, 1, n, len(srcs)
    for s, (ptr, ch, taps, ih, iw, *up) in zip(d.src, srcs):
        s.ptr, s.channels, s.taps, s.in_h, s.in_w, s.upsample = ptr, ch, taps, ih, iw, (up[0] if up else 0)
    d.w, d.out_dtype, d.out_ld = w_ptr, dtype, n
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def run_gemm(lib, d: GemmDesc, workspace_fn, stream) -> int:
    """idb_gemm on `d`: workspace_fn(nbytes) -> a device uint8 tensor of at least nbytes, asked only when the plan needs one.
    Returns idb_gemm's status unchecked (the engine handles IDB_EUNSUPPORTED of a grouped launch itself)."""
    need = lib.idb_gemm_workspace_bytes(C.byref(d))
    ws = workspace_fn(need).data_ptr() if need > 0 else None
    return lib.idb_gemm(C.byref(d), ws, need, stream)
