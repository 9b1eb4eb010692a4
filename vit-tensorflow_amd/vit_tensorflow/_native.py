"""ctypes binding of libvitx.so (include/vitx.h).  No compute happens in Python: every tensor op of
the hot path is a HIP kernel behind the C ABI.  There is deliberately NO CPU fallback -- if the
library is missing or no GPU is visible, calls fail loudly."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITX_LIB", os.path.join(_HERE, "..", "lib", "libvitx.so"))

VARIANT_VIT, VARIANT_DEEPVIT, VARIANT_CAIT, VARIANT_PATCH_MERGER = 0, 1, 2, 3
POOL_CLS, POOL_MEAN = 0, 1
COMPUTE_FP32, COMPUTE_BF16, COMPUTE_BF16X3 = 0, 1, 2
OK, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_STATE, ERR_COMM = 0, -1, -2, -3, -4, -5


class VitxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libvitx error {code}: {msg}")
        self.code = code
        self.message = msg


class _ConfigFlags(C.Structure):
    _fields_ = [("cct_block", C.c_int32), ("nest_block", C.c_int32), ("global_k", C.c_int32),
                ("conv_proj_kernel", C.c_int16), ("conv_proj_stride", C.c_int16)]


class _ConfigTail(C.Union):
    """The last four words of vitx_config.  include/vitx.h carved cct_block, nest_block and global_k out of the first three reserved words and
    conv_proj_kernel / conv_proj_stride (two halves) out of the last; `reserved` keeps its four-word view here (reserved[0] is cct_block,
    reserved[1] nest_block, reserved[2] global_k, reserved[3] the two conv_proj halves), so code that zeroes or inspects it by that name sees
    the layout it always saw.  The struct has no spare word left."""
    _anonymous_ = ("_flags",)
    _fields_ = [("reserved", C.c_int32 * 4), ("_flags", _ConfigFlags)]


class Config(C.Structure):
    _anonymous_ = ("_tail",)
    _fields_ = [
        ("variant", C.c_int32),
        ("image_h", C.c_int32), ("image_w", C.c_int32),
        ("patch_h", C.c_int32), ("patch_w", C.c_int32),
        ("channels", C.c_int32),
        ("num_classes", C.c_int32), ("dim", C.c_int32), ("depth", C.c_int32), ("cls_depth", C.c_int32),
        ("heads", C.c_int32), ("dim_head", C.c_int32), ("mlp_dim", C.c_int32),
        ("pool", C.c_int32),
        ("dropout", C.c_float), ("emb_dropout", C.c_float), ("layer_dropout", C.c_float),
        ("ln_eps", C.c_float),
        ("compute", C.c_int32),
        ("max_batch", C.c_int32),
        ("device_id", C.c_int32),
        ("num_parallel_branches", C.c_int32),
        ("patch_merge_layer", C.c_int32), ("patch_merge_num_tokens", C.c_int32),
        ("small_dataset", C.c_int32),
        ("_tail", _ConfigTail),
    ]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


MIM_MAE, MIM_SIMMIM, MIM_MPP = 0, 1, 2


class MimConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("decoder_dim", C.c_int32), ("decoder_depth", C.c_int32), ("decoder_heads", C.c_int32), ("decoder_dim_head", C.c_int32),
        ("literal_loss", C.c_int32),
        ("masking_ratio", C.c_double),
        ("output_channel_bits", C.c_int32), ("max_pixel_val", C.c_float), ("has_norm", C.c_int32),
        ("norm_mean", C.c_float * 4), ("norm_std", C.c_float * 4),
        ("reserved", C.c_int32 * 5),
    ]


class DistillConfig(C.Structure):
    _fields_ = [("temperature", C.c_float), ("alpha", C.c_float), ("hard", C.c_int32), ("literal_loss", C.c_int32), ("reserved", C.c_int32 * 8)]


class CCTConfig(C.Structure):
    _fields_ = [
        ("img_height", C.c_int32), ("img_width", C.c_int32),
        ("n_input_channels", C.c_int32), ("embedding_dim", C.c_int32), ("n_conv_layers", C.c_int32), ("kernel_size", C.c_int32),
        ("stride", C.c_int32), ("pooling_kernel_size", C.c_int32), ("pooling_stride", C.c_int32),
        ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("dim_feedforward", C.c_int32), ("num_classes", C.c_int32),
        ("positional_embedding", C.c_int32), ("in_planes", C.c_int32),
        ("ln_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32), ("conv_chunk", C.c_int32),
        ("reserved", C.c_int32 * 8),
    ]


CCT_POS = {"learnable": 0, "sine": 1, "none": 2}


class NesTConfig(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("num_classes", C.c_int32), ("dim", C.c_int32), ("heads", C.c_int32),
        ("num_hierarchies", C.c_int32), ("block_repeats", C.c_int32 * 8), ("mlp_mult", C.c_int32),
        ("ln_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32), ("conv_chunk", C.c_int32),
        ("small_attn", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class TwinsConfig(C.Structure):
    _fields_ = [
        ("image_h", C.c_int32), ("image_w", C.c_int32), ("num_classes", C.c_int32),
        ("emb_dim", C.c_int32 * 4), ("patch_size", C.c_int32 * 4), ("local_patch_size", C.c_int32 * 4), ("global_k", C.c_int32 * 4),
        ("depth", C.c_int32 * 4), ("peg_kernel_size", C.c_int32),
        ("ln_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32),
        ("fused_global_attn", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class CvTConfig(C.Structure):
    _fields_ = [
        ("image_h", C.c_int32), ("image_w", C.c_int32), ("num_classes", C.c_int32),
        ("emb_dim", C.c_int32 * 3), ("emb_kernel", C.c_int32 * 3), ("emb_stride", C.c_int32 * 3), ("proj_kernel", C.c_int32 * 3),
        ("kv_proj_stride", C.c_int32 * 3), ("heads", C.c_int32 * 3), ("depth", C.c_int32 * 3), ("mlp_mult", C.c_int32 * 3),
        ("ln_eps", C.c_float), ("bn_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32),
        ("fused_attn", C.c_int32), ("reserved", C.c_int32 * 8),
    ]


CF_MAX_SCALES = 8


class CrossFormerConfig(C.Structure):
    _fields_ = [
        ("image_h", C.c_int32), ("image_w", C.c_int32), ("num_classes", C.c_int32),
        ("dim", C.c_int32 * 4), ("depth", C.c_int32 * 4), ("global_window_size", C.c_int32 * 4), ("local_window_size", C.c_int32 * 4),
        ("n_kernels", C.c_int32 * 4), ("kernel_sizes", (C.c_int32 * CF_MAX_SCALES) * 4), ("strides", C.c_int32 * 4),
        ("ln_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32),
        ("window_attn", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class RegionViTConfig(C.Structure):
    _fields_ = [
        ("image_h", C.c_int32), ("image_w", C.c_int32), ("num_classes", C.c_int32),
        ("dim", C.c_int32 * 4), ("depth", C.c_int32 * 4), ("window_size", C.c_int32), ("local_patch_size", C.c_int32),
        ("tokenize_local_3_conv", C.c_int32), ("use_peg", C.c_int32),
        ("ln_eps", C.c_float), ("compute", C.c_int32), ("max_batch", C.c_int32), ("device_id", C.c_int32),
        ("window_attn", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class CrossViTConfig(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("num_classes", C.c_int32), ("sm_dim", C.c_int32), ("lg_dim", C.c_int32),
        ("sm_patch_size", C.c_int32), ("sm_enc_depth", C.c_int32), ("sm_enc_heads", C.c_int32), ("sm_enc_mlp_dim", C.c_int32),
        ("sm_enc_dim_head", C.c_int32),
        ("lg_patch_size", C.c_int32), ("lg_enc_depth", C.c_int32), ("lg_enc_heads", C.c_int32), ("lg_enc_mlp_dim", C.c_int32),
        ("lg_enc_dim_head", C.c_int32),
        ("cross_attn_depth", C.c_int32), ("cross_attn_heads", C.c_int32), ("cross_attn_dim_head", C.c_int32), ("depth", C.c_int32),
        ("dropout", C.c_float), ("emb_dropout", C.c_float),
        ("ln_eps", C.c_float),
        ("compute", C.c_int32),
        ("max_batch", C.c_int32),
        ("device_id", C.c_int32),
        ("reserved", C.c_int32 * 8),
    ]


PIT_MAX_STAGES = 8


class PiTConfig(C.Structure):
    _fields_ = [
        ("image_h", C.c_int32), ("image_w", C.c_int32), ("image_size", C.c_int32), ("patch_size", C.c_int32), ("num_classes", C.c_int32),
        ("dim", C.c_int32), ("n_stages", C.c_int32), ("depth", C.c_int32 * PIT_MAX_STAGES), ("heads", C.c_int32 * PIT_MAX_STAGES),
        ("mlp_dim", C.c_int32), ("dim_head", C.c_int32), ("pool_stages", C.c_int32),
        ("ln_eps", C.c_float),
        ("compute", C.c_int32),
        ("max_batch", C.c_int32),
        ("device_id", C.c_int32),
        ("long_attn", C.c_int32),
        ("reserved", C.c_int32 * 8),
    ]


GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)

# every symbol include/vitx.h declares: (name, restype, argtypes)
_P = C.POINTER
SYMBOLS: List[Tuple[str, object, list]] = [
    ("vitx_version", C.c_char_p, []),
    ("vitx_last_error", C.c_char_p, []),
    ("vitx_param_table_size", C.c_int32, [_P(Config), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_param_table_entry", C.c_int32, [_P(Config), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_create", C.c_int32, [_P(Config), _P(C.c_void_p)]),
    ("vitx_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_get_config", C.c_int32, [C.c_void_p, _P(Config)]),
    ("vitx_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_bind_arenas", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_set_patch_input", C.c_int32, [C.c_void_p, C.c_int32]),
    ("vitx_set_long_attn", C.c_int32, [C.c_void_p, C.c_int32]),
    ("vitx_distill_backward_input", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_forward_patches", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_forward_patches_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_get_opt_state", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_set_opt_state", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("vitx_transformer_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_transformer_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_patch_unfold", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_embed_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_embed_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_spt_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_spt_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_patch_dense_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_head_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_head_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_head_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_head_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_embed_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_embed_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_extract_patches_shape", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    ("vitx_extract_patches", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_extract_patches_backward", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_extract_patches_dev", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("vitx_extract_patches_backward_dev", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("vitx_ce_loss_grad_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    ("vitx_adamw_step", C.c_int32, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    ("vitx_sgd_step", C.c_int32, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    ("vitx_set_stream", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("vitx_sync", C.c_int32, [C.c_void_p]),
    ("vitx_graph_capture_begin", C.c_int32, [C.c_void_p]),
    ("vitx_graph_capture_end", C.c_int32, [C.c_void_p, _P(C.c_void_p)]),
    ("vitx_graph_launch", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("vitx_graph_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_set_grad_ready_callback", C.c_int32, [C.c_void_p, GRAD_READY_FN, C.c_void_p]),
    ("vitx_comm_unique_id", C.c_int32, [C.c_void_p]),
    ("vitx_comm_init", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_comm_overlap", C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32]),
    ("vitx_comm_stats", C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("vitx_comm_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_debug_switches", C.c_int32, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("vitx_allreduce_grads", C.c_int32, [C.c_void_p]),
    ("vitx_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_workspace_bytes", C.c_int32, [C.c_void_p, _P(C.c_int64)]),
    ("vitx_debug_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_bench_gemm", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_float), _P(C.c_float)]),
    ("vitx_check_gemm", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_float)]),
    ("vitx_mim_create", C.c_int32, [C.c_void_p, _P(MimConfig), _P(C.c_void_p)]),
    ("vitx_mim_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_mim_decoder", C.c_void_p, [C.c_void_p]),
    ("vitx_mim_param_table_size", C.c_int32, [C.c_void_p, _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_mim_param_table_entry", C.c_int32, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_mim_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_mim_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_mim_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_mim_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_mim_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_mim_num_masked", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    ("vitx_mim_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_mim_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_mim_backward", C.c_int32, [C.c_void_p]),
    ("vitx_mim_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_forward_distill", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_backward_distill", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_distill_create", C.c_int32, [C.c_void_p, _P(DistillConfig), _P(C.c_void_p)]),
    ("vitx_distill_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_distill_param_table_size", C.c_int32, [C.c_void_p, _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_distill_param_table_entry", C.c_int32, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_distill_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_distill_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_distill_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_distill_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_float, C.c_float, C.c_void_p]),
    ("vitx_distill_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_float, C.c_float, C.c_void_p]),
    ("vitx_distill_backward", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("vitx_distill_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_crossvit_param_table_size", C.c_int32, [_P(CrossViTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_crossvit_param_table_entry", C.c_int32, [_P(CrossViTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_crossvit_create", C.c_int32, [_P(CrossViTConfig), _P(C.c_void_p)]),
    ("vitx_crossvit_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_crossvit_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossvit_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossvit_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossvit_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_crossvit_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_crossvit_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_crossvit_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_crossvit_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]),
    ("vitx_crossvit_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_crossvit_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_crossvit_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_cct_param_table_size", C.c_int32, [_P(CCTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_cct_param_table_entry", C.c_int32, [_P(CCTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_cct_sequence_length", C.c_int32, [_P(CCTConfig), _P(C.c_int32)]),
    ("vitx_cct_create", C.c_int32, [_P(CCTConfig), _P(C.c_void_p)]),
    ("vitx_cct_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_cct_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cct_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cct_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cct_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_cct_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_cct_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_cct_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_cct_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_cct_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_cct_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_cct_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_cct_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_cct_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_nest_param_table_size", C.c_int32, [_P(NesTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_nest_param_table_entry", C.c_int32, [_P(NesTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_nest_create", C.c_int32, [_P(NesTConfig), _P(C.c_void_p)]),
    ("vitx_nest_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_nest_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_nest_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_nest_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_nest_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_nest_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_nest_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_nest_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_nest_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_nest_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_nest_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_nest_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_nest_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_nest_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_twins_param_table_size", C.c_int32, [_P(TwinsConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_twins_param_table_entry", C.c_int32, [_P(TwinsConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_twins_create", C.c_int32, [_P(TwinsConfig), _P(C.c_void_p)]),
    ("vitx_twins_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_twins_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_twins_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_twins_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_twins_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_twins_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_twins_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_twins_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_twins_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_twins_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_twins_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_twins_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_twins_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_twins_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_cvt_param_table_size", C.c_int32, [_P(CvTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_cvt_param_table_entry", C.c_int32, [_P(CvTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_cvt_create", C.c_int32, [_P(CvTConfig), _P(C.c_void_p)]),
    ("vitx_cvt_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_cvt_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cvt_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cvt_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_cvt_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_cvt_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_cvt_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_cvt_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_cvt_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_cvt_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_cvt_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_cvt_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_cvt_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_cvt_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_crossformer_param_table_size", C.c_int32, [_P(CrossFormerConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_crossformer_param_table_entry", C.c_int32,
     [_P(CrossFormerConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_crossformer_create", C.c_int32, [_P(CrossFormerConfig), _P(C.c_void_p)]),
    ("vitx_crossformer_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_crossformer_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossformer_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossformer_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_crossformer_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_crossformer_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_crossformer_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_crossformer_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_crossformer_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_crossformer_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_crossformer_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_crossformer_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_crossformer_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_crossformer_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_crossformer_partition", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 6),
    ("vitx_crossformer_window_attn", C.c_int32, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_float, C.c_int32] + [C.c_void_p] * 3),
    ("vitx_regionvit_param_table_size", C.c_int32, [_P(RegionViTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_regionvit_param_table_entry", C.c_int32,
     [_P(RegionViTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_regionvit_create", C.c_int32, [_P(RegionViTConfig), _P(C.c_void_p)]),
    ("vitx_regionvit_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_regionvit_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_regionvit_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_regionvit_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_regionvit_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_regionvit_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_regionvit_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_regionvit_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_regionvit_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_regionvit_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_regionvit_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_regionvit_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_regionvit_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_regionvit_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("vitx_regionvit_attn", C.c_int32, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_float, C.c_int32] + [C.c_void_p] * 4),
    ("vitx_regionvit_partition", C.c_int32, [C.c_void_p] * 4 + [C.c_int32] * 7),
    ("vitx_pit_param_table_size", C.c_int32, [_P(PiTConfig), _P(C.c_int64), _P(C.c_int64)]),
    ("vitx_pit_param_table_entry", C.c_int32, [_P(PiTConfig), C.c_int64, C.c_char_p, C.c_int32, _P(C.c_int64), _P(C.c_int32), _P(C.c_int64)]),
    ("vitx_pit_create", C.c_int32, [_P(PiTConfig), _P(C.c_void_p)]),
    ("vitx_pit_destroy", C.c_int32, [C.c_void_p]),
    ("vitx_pit_set_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_pit_get_params", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_pit_get_grads", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("vitx_pit_params_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_pit_grads_dev", C.c_int32, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
    ("vitx_pit_params_changed", C.c_int32, [C.c_void_p]),
    ("vitx_pit_set_long_attn", C.c_int32, [C.c_void_p, C.c_int32]),
    ("vitx_pit_forward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_pit_forward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("vitx_pit_backward", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_pit_backward_dev", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("vitx_pit_pool_forward", C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("vitx_pit_pool_backward", C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("vitx_pit_profile_begin", C.c_int32, [C.c_void_p]),
    ("vitx_pit_profile_end", C.c_int32, [C.c_void_p, _P(KernelStat), C.c_int32, _P(C.c_int32)]),
    ("vitx_pit_read", C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
]

_lib = None


def lib():
    """Load libvitx.so once.  Raises (never falls back) when the HIP library has not been built."""
    global _lib
    if _lib is None:
        path = os.path.abspath(LIB_PATH)
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `python vit-tensorflow_amd/build.py` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        l = C.CDLL(path, mode=C.RTLD_LOCAL)
        for name, res, args in SYMBOLS:
            fn = getattr(l, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> None:
    if rc != OK:
        raise VitxError(rc, lib().vitx_last_error().decode("utf-8", "replace"))


def table_of(prefix: str, arg):
    """([(name, shape, offset)], elements) from `<prefix>_param_table_size / _entry`; arg: what they take first (a config by reference, or a handle)."""
    l = lib()
    size_fn, entry_fn = getattr(l, prefix + "_param_table_size"), getattr(l, prefix + "_param_table_entry")
    nt, ne = C.c_int64(), C.c_int64()
    check(size_fn(arg, C.byref(nt), C.byref(ne)))
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    rank, off = C.c_int32(), C.c_int64()
    for i in range(nt.value):
        check(entry_fn(arg, i, name, 256, shape, C.byref(rank), C.byref(off)))
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(rank.value)), int(off.value)))
    return out, int(ne.value)


def param_table(cfg: Config):
    """[(name, shape, offset)] from the C library (host-only call; no GPU needed)."""
    return table_of("vitx", C.byref(cfg))


def crossvit_param_table(cfg: CrossViTConfig):
    """[(name, shape, offset)] of CrossViT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_crossvit", C.byref(cfg))


def cct_param_table(cfg: CCTConfig):
    """[(name, shape, offset)] of CCT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_cct", C.byref(cfg))


def nest_param_table(cfg: NesTConfig):
    """[(name, shape, offset)] of NesT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_nest", C.byref(cfg))


def twins_param_table(cfg: TwinsConfig):
    """[(name, shape, offset)] of TwinsSVT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_twins", C.byref(cfg))


def cvt_param_table(cfg: CvTConfig):
    """[(name, shape, offset)] of CvT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_cvt", C.byref(cfg))


def crossformer_param_table(cfg: CrossFormerConfig):
    """[(name, shape, offset)] of CrossFormer's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_crossformer", C.byref(cfg))


def regionvit_param_table(cfg: RegionViTConfig):
    """[(name, shape, offset)] of RegionViT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_regionvit", C.byref(cfg))


def pit_param_table(cfg: PiTConfig):
    """[(name, shape, offset)] of PiT's variables from the C library (host-only call; no GPU needed)."""
    return table_of("vitx_pit", C.byref(cfg))


def mim_param_table(handle, prefix="vitx_mim"):
    """[(name, shape, offset)] of a wrapper object's own parameters (prefix 'vitx_mim': MAE / SimMIM, 'vitx_distill': DistillWrapper)."""
    return table_of(prefix, handle)


def debug_switches():
    """[(name, class, state, doc)] for every VITX_* environment variable the library reads (csrc/env.hip): class "tuning" (same results),
    "path" (another validated code path) or "diag" (may corrupt results; ignored by the release library)."""
    need = C.c_int64()
    check(lib().vitx_debug_switches(None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib().vitx_debug_switches(buf, need.value, None))
    return [tuple(line.split("\t", 3)) for line in buf.value.decode().splitlines()]


def cct_sequence_length(cfg: CCTConfig) -> int:
    n = C.c_int32()
    check(lib().vitx_cct_sequence_length(C.byref(cfg), C.byref(n)))
    return int(n.value)
