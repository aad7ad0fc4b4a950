"""ctypes binding of librn_hip.so (C ABI: include/rn_hip.h).

PyTorch-ROCm tensors are only the device-memory / stream / autograd carrier: every call
below hands raw device pointers and the current HIP stream to a hand-written gfx950
kernel.  There is no CPU or eager-PyTorch fallback -- a missing library, or a tensor that is
not a contiguous fp32 device tensor, raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RN_LIB_PATH") or os.path.join(_HERE, "librn_hip.so")   # (RN_LIB_PATH: A/B measurements of two builds on one box)

MAX_SEG = 16
ACT = {None: 0, "none": 0, "linear": 0, "relu": 1, "elu": 2, "relu6": 3, "sigmoid": 4}
LOSS_MODE = {"bce_dice": 0, "focal": 1}
OPT = {"momentum": 0, "rmsprop": 1, "adam": 2}
OPT_BLOCK = 1024
LR_MAX_BOUNDARIES = 8    # RN_LR_MAX_BOUNDARIES
LOSS_STATS_HEADER = 8
OPT_F_NORM, OPT_F_LRDEV, OPT_F_EMA, OPT_F_CLIP, OPT_F_ACCUM, OPT_F_GATE = 1, 2, 4, 8, 16, 32    # enum rn_opt_feature
CTL_F_ACCUM, CTL_F_GUARD, CTL_F_LR, CTL_F_EMA = 1, 2, 4, 8                                      # enum rn_ctl_feature
API_VERSION = 427     # RN_API_VERSION of include/rn_hip.h these bindings were written against


class RnError(RuntimeError):
    pass


class LrSchedule(C.Structure):
    """rn_lr_schedule (a field of StepControl); built by train.LRSchedule.struct()."""
    _fields_ = [("kind", C.c_int32), ("n_boundaries", C.c_int32), ("base_lr", C.c_double), ("warmup_factor", C.c_double),
                ("final_factor", C.c_double), ("decay_factor", C.c_double), ("warmup_steps", C.c_int64), ("total_steps", C.c_int64),
                ("boundaries", C.c_int64 * LR_MAX_BOUNDARIES)]


class StepControl(C.Structure):
    """rn_step_control (passed by pointer, read before rn_step_control_eval returns): the fields of a clear feature stay 0 / None."""
    _fields_ = [("features", C.c_uint32), ("optimizer_kind", C.c_int32),
                ("accumulate_steps", C.c_int32), ("micro_dev", C.c_void_p), ("accum_dev", C.c_void_p),                          # ACCUM
                ("norm_sq", C.c_void_p), ("gate_dev", C.c_void_p), ("skipped_dev", C.c_void_p),                                 # GUARD
                ("schedule", LrSchedule), ("step_dev", C.c_void_p), ("lr_dev", C.c_void_p),                                     # LR
                ("ema_decay", C.c_double), ("ema_warmup", C.c_int32), ("ema_updates_dev", C.c_void_p), ("ema_dev", C.c_void_p)]  # EMA


class OptUpdate(C.Structure):
    """rn_opt_update (passed by pointer, read before rn_optimizer_update returns): the fields of a clear feature stay 0 / None."""
    _fields_ = [("kind", C.c_int32), ("features", C.c_uint32), ("w", C.c_void_p), ("grad", C.c_void_p), ("state1", C.c_void_p),
                ("state2", C.c_void_p), ("wd_per_block", C.c_void_p), ("count", C.c_int64), ("lr", C.c_float), ("grad_scale", C.c_float),
                ("step", C.c_int64), ("advance_counter", C.c_void_p), ("advance_by", C.c_uint64),
                ("partial", C.c_void_p), ("lr_dev", C.c_void_p), ("ema", C.c_void_p), ("ema_dev", C.c_void_p),       # NORM, LRDEV, EMA
                ("clip_norm", C.c_float), ("norm_sq", C.c_void_p),                                                   # CLIP
                ("acc", C.c_void_p), ("inv_accum", C.c_float), ("accum_dev", C.c_void_p), ("gate_dev", C.c_void_p)]  # ACCUM, GATE


class ConvSeg(C.Structure):
    _fields_ = [("x", C.c_void_p), ("wgt", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p),
                ("dy", C.c_void_p), ("dx", C.c_void_p),
                ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cout", C.c_int32),
                ("x_ld", C.c_int32), ("x_coff", C.c_int32), ("wgt_bytes", C.c_int64)]


class AssignLevel(C.Structure):
    _fields_ = [("anchor_sizes", C.c_void_p), ("grid_h", C.c_int32), ("grid_w", C.c_int32), ("cls_out", C.c_void_p),
                ("reg_out", C.c_void_p), ("trainable_out", C.c_void_p), ("argmax_out", C.c_void_p)]


class ConvGeom(C.Structure):
    _fields_ = [("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("cin", C.c_int32),
                ("groups", C.c_int32)]


class WinoGn(C.Structure):
    _fields_ = [("in_rows", C.c_void_p), ("in_gamma", C.c_void_p), ("in_beta", C.c_void_p), ("in_groups", C.c_int32),
                ("in_act", C.c_int32), ("in_eps", C.c_float), ("out_rows", C.c_void_p), ("out_groups", C.c_int32),
                ("u_ready", C.c_void_p), ("urot_ready", C.c_int32)]


class WinoGnBwd(C.Structure):
    _fields_ = [("in_rows", C.c_void_p), ("in_gamma", C.c_void_p), ("in_beta", C.c_void_p), ("in_groups", C.c_int32),
                ("in_act", C.c_int32), ("in_eps", C.c_float), ("in_g_rows_group", C.c_void_p), ("in_g_rows_chan", C.c_void_p),
                ("out_rows", C.c_void_p), ("out_g_rows_group", C.c_void_p), ("out_gamma", C.c_void_p),
                ("out_groups", C.c_int32), ("out_eps", C.c_float), ("defer_wgrad", C.c_int32)]


class WinoGnPlanCall(C.Structure):
    """rn_wino_gn_plan_call"""
    _fields_ = [("in_chunked", C.c_int32), ("out_chunked", C.c_int32), ("in_w", C.c_int32), ("out_w", C.c_int32),
                ("in_slabs", C.c_int32), ("out_slabs", C.c_int32), ("stride_w", C.c_int32), ("in_staged", C.c_int32),
                ("out_staged", C.c_int32)]


class WinoGnPlan(C.Structure):
    """rn_wino_gn_plan: the kernels one folded Winograd layer launches (rn_conv3x3_winograd_gn_plan, host only)"""
    _fields_ = [("fwd", WinoGnPlanCall), ("bwd", WinoGnPlanCall), ("tiles", C.c_int32), ("chunks", C.c_int32),
                ("partial_chunk", C.c_int32), ("u_frag", C.c_int32)]


class ConvPlanCall(C.Structure):
    """rn_conv_plan_call: the kernels one convolution call launches"""
    _fields_ = [("path", C.c_int32), ("cfg", C.c_int32), ("load", C.c_int32), ("nsplit", C.c_int32), ("ksplit", C.c_int32),
                ("blocks", C.c_int32), ("grouped", C.c_int32), ("batched", C.c_int32), ("phases", C.c_int32),
                ("phases_no_taps", C.c_int32), ("windows", C.c_int32), ("direct", C.c_int32), ("reduce", C.c_int32),
                ("m_tile", C.c_int32), ("n_piece", C.c_int32), ("patch_bytes", C.c_int64), ("rows_per_sample", C.c_int32),
                ("reserved_", C.c_int32)]


class ConvPlan(C.Structure):
    """rn_conv_plan: what rn_conv2d_fwd / _fwd_stats / _dgrad / _wgrad / _bwd launch (rn_conv2d_plan, host only)"""
    _fields_ = [("call", ConvPlanCall), ("dgrad", ConvPlanCall), ("wgrad", ConvPlanCall), ("unmerged", C.c_int32), ("reserved_", C.c_int32)]


# enum rn_conv_op / rn_conv_path / rn_conv_load / rn_conv_reduce / rn_conv_unmerged
CONV_OPS = {"fwd": 0, "fwd_stats": 1, "dgrad": 2, "wgrad": 3, "bwd": 4}
CONV_PATHS = {0: None, 1: "direct_grouped", 2: "stem", 3: "x3_1x1", 4: "x3_patch", 5: "fp32", 6: "merged_bwd"}
CONV_LOADS = {0: "scalar", 1: "vec4", 2: "vec4_tap"}
CONV_REDUCES = {0: None, 1: "launched", 2: "deferred"}
CONV_UNMERGED = {0: None, 1: "switch", 2: "x3_1x1", 3: "direct_grouped", 4: "x3_patch", 5: "shape"}


class ReduceDesc(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("count", C.c_int32), ("nrows", C.c_uint16), ("accumulate", C.c_uint16)]


class ReduceList(C.Structure):
    """rn_reduce_list: deferred row reductions recorded by the gradient entry points, owned by the caller (host memory)."""
    _fields_ = [("desc", C.POINTER(ReduceDesc)), ("capacity", C.c_int32), ("count", C.c_int32)]

    @classmethod
    def make(cls, capacity=1024):
        arr = (ReduceDesc * capacity)()
        lst = cls(C.cast(arr, C.POINTER(ReduceDesc)), capacity, 0)
        lst._keep = arr
        return lst


class AddSeg(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("out", C.c_void_p), ("count", C.c_int64)]


class GnSeg(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("residual", C.c_void_p), ("dy", C.c_void_p),
                ("dx", C.c_void_p), ("dresidual", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("n", C.c_int32), ("hw", C.c_int32), ("x_ld", C.c_int32), ("dx_ld", C.c_int32), ("dx_accumulate", C.c_int32)]


class GnParams(C.Structure):
    _fields_ = [("c", C.c_int32), ("groups", C.c_int32), ("act", C.c_int32), ("act_after_residual", C.c_int32),
                ("in_f16", C.c_int32), ("out_f16", C.c_int32), ("eps", C.c_float),
                ("drop_rate", C.c_float), ("drop_seed", C.c_uint64), ("drop_seed_dev", C.c_void_p), ("sync", C.c_void_p),
                ("stat_rows", C.c_void_p)]


class GnPlan(C.Structure):
    """rn_gn_plan: the kernels one rn_group_norm_fwd / rn_group_norm_bwd call launches (rn_group_norm_plan, host only)"""
    _fields_ = [("path", C.c_int32), ("slice_wc", C.c_int32), ("slice_r", C.c_int32), ("slice_blocks", C.c_int32),
                ("coop_r", C.c_int32), ("coop_ppc", C.c_int32), ("coop_blocks", C.c_int32),
                ("rows_sw", C.c_int32), ("rows_per_group", C.c_int32), ("rows_apply_r", C.c_int32), ("rows_apply_blocks", C.c_int32),
                ("rows_per_sample", C.c_int32 * 16), ("stats_kernel", C.c_int32), ("finalize_kernel", C.c_int32),
                ("apply_kernel", C.c_int32), ("apply_blocks", C.c_int32), ("param_grad", C.c_int32),
                ("param_grad_deferred", C.c_int32), ("total_chunks", C.c_int32)]


# enum rn_gn_path / rn_gn_kernel / rn_gn_param_grad
GN_PATHS = {1: "producer_rows", 2: "slice", 3: "grid_resident", 4: "narrow_slice", 5: "rows", 6: "three_kernels"}
GN_KERNELS = {0: None, 1: "gn_partial_kernel", 2: "gn_partial_f16x8_kernel", 3: "gn_finalize_kernel",
              4: "gn_finalize_cols_segs_kernel", 5: "gn_apply_kernel", 6: "gn_apply_f16x8_kernel"}
GN_PARAM_GRADS = {0: None, 1: "finalize_blocks", 2: "gn_param_grad_kernel", 3: "rn_reduce_rows"}


class GnRows(C.Structure):
    """rn_gn_rows: partial (sum, sum of squares) rows a conv / depthwise forward wrote for the GroupNorm that follows"""
    _fields_ = [("rows", C.c_void_p), ("rows_per_sample", C.c_int32), ("per_group", C.c_int32), ("groups", C.c_int32)]


class GnResidualNorm(C.Structure):
    _fields_ = [("mean", C.c_void_p), ("rstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("groups", C.c_int)]


class F16Fold(C.Structure):
    """rn_f16_fold"""
    _fields_ = [("in_mean", C.c_void_p), ("in_rstd", C.c_void_p), ("in_gamma", C.c_void_p), ("in_beta", C.c_void_p),
                ("in_groups", C.c_int32), ("in_act", C.c_int32), ("partial", C.c_void_p),
                ("seg_chunk_start", C.c_void_p), ("total_chunks", C.c_int32)]


class F16Plan(C.Structure):
    """rn_f16_plan: the kernel one rn_conv2d_fwd_f16 / rn_conv2d_fwd_f16_fold call launches (rn_conv2d_f16_plan, host only)"""
    _fields_ = [("kernel", C.c_int32), ("cfg", C.c_int32), ("vec", C.c_int32), ("tap_uniform", C.c_int32), ("fold", C.c_int32),
                ("stats", C.c_int32), ("pipe", C.c_int32), ("epilogue", C.c_int32), ("a_nt", C.c_int32), ("frag_copy", C.c_int32),
                ("blocks", C.c_int32), ("k_tiles", C.c_int32), ("rows_per_sample", C.c_int32), ("multi_stats", C.c_int32),
                ("tiles_per_sample", C.c_int32 * MAX_SEG)]


# enum rn_f16_kernel / rn_f16_epilogue
F16_KERNELS = {0: None, 1: "igemm", 2: "sg"}
F16_EPILOGUES = {0: "staged", 1: "scalar_f16", 2: "scalar_f32"}


class DwF16(C.Structure):
    """rn_dw_f16: one fp16 depthwise 3 x 3 call (rn_depthwise_fwd_f16)"""
    _fields_ = [("x", C.c_void_p), ("wgt", C.c_void_p), ("y", C.c_void_p),
                ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32),
                ("in_mean", C.c_void_p), ("in_rstd", C.c_void_p), ("in_gamma", C.c_void_p), ("in_beta", C.c_void_p),
                ("in_groups", C.c_int32), ("in_act", C.c_int32), ("partial", C.c_void_p)]


class DwF16Plan(C.Structure):
    """rn_dw_f16_plan: what rn_depthwise_fwd_f16 launches for a descriptor (rn_depthwise_f16_plan, host only)"""
    _fields_ = [(name, C.c_int32) for name in (
        "oh", "ow", "pad_t", "pad_l", "kernel", "pixels_per_thread", "pixel_lanes", "rows_per_thread", "strips_per_sample",
        "strips_per_chunk", "pixels_per_chunk", "rows_per_sample", "blocks", "fold", "stats")]


DW_F16_KERNELS = {0: None, 1: "s1", 2: "s2"}       # enum rn_dw_f16_kernel


class DenseF16Plan(C.Structure):
    """rn_dense_f16_plan: what rn_dense_f16_put / _finalize / _norm launch for a shape (rn_dense_f16_plan, host only)"""
    _fields_ = [(name, C.c_int32) for name in (
        "op", "vec", "chunk", "rows", "octets_per_block", "lanes", "grid_x", "grid_y", "grid_z", "threads")]


DENSE_F16_OPS = {"put": 1, "finalize": 2, "norm": 3}       # enum rn_dense_f16_op


class MbRows(C.Structure):
    """rn_mb_rows"""
    _fields_ = [("rows", C.c_void_p), ("rows_per_sample", C.c_int32), ("width", C.c_int32), ("bn", C.c_int32)]


class MbNorm(C.Structure):
    """rn_mb_norm: one GroupNorm (+ activation + dropout) block, applied by the kernels on either side of it"""
    _fields_ = [("y", C.c_void_p), ("stat", MbRows), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("c", C.c_int32), ("groups", C.c_int32), ("act", C.c_int32), ("eps", C.c_float),
                ("drop_rate", C.c_float), ("drop_seed", C.c_uint64), ("drop_seed_dev", C.c_void_p)]


class MbDy(C.Structure):
    """rn_mb_dy"""
    _fields_ = [("dy", C.c_void_p), ("norm", C.POINTER(MbNorm)), ("g", C.c_void_p), ("g_plain", C.c_int32), ("grows", MbRows)]


class MbGout(C.Structure):
    """rn_mb_gout"""
    _fields_ = [("out", C.c_void_p), ("add1", C.c_void_p), ("add2", C.c_void_p), ("norm", C.POINTER(MbNorm)),
                ("store_plain", C.c_int32), ("grows", MbRows), ("planes", C.c_void_p)]


class LossSeg(C.Structure):
    _fields_ = [("cls_logit", C.c_void_p), ("cls_label", C.c_void_p), ("reg_pred", C.c_void_p),
                ("reg_label", C.c_void_p), ("trainable", C.c_void_p), ("d_cls_logit", C.c_void_p),
                ("d_reg_pred", C.c_void_p), ("rows", C.c_int64)]


# enum rn_loss_term; the names are those of losses.parse_class_loss and of the w_ / s_ fields below
LOSS_TERM = {"bce": 1, "balanced_bce": 2, "dice": 4, "jaccard": 8, "fixed_iou": 16, "focal": 32}


class LossTerms(C.Structure):
    """rn_loss_terms (passed by pointer, read before the call returns): weight and smooth of a clear term stay 0."""
    _fields_ = [("terms", C.c_uint32), ("w_bce", C.c_float), ("w_balanced_bce", C.c_float), ("w_dice", C.c_float),
                ("w_jaccard", C.c_float), ("w_fixed_iou", C.c_float), ("w_focal", C.c_float),
                ("s_dice", C.c_float), ("s_jaccard", C.c_float), ("s_fixed_iou", C.c_float)]


# enum rn_regr_term; the names are those of losses.parse_regr_loss and of the w_ fields below
REGR_TERM = {"huber": 1, "iou": 2, "giou": 4}
REGR_STATS_FLOATS = 8    # RN_REGR_STATS_FLOATS


class RegrTerms(C.Structure):
    """rn_regr_terms (passed by pointer, read before the call returns): weight and delta of a clear term stay 0."""
    _fields_ = [("terms", C.c_uint32), ("w_huber", C.c_float), ("w_iou", C.c_float), ("w_giou", C.c_float),
                ("delta_huber", C.c_float)]


class MetricsSeg(C.Structure):
    """rn_metrics_seg: one pyramid level of rn_train_metrics_pass"""
    _fields_ = [("cls_logit", C.c_void_p), ("cls_label", C.c_void_p), ("reg_pred", C.c_void_p), ("reg_label", C.c_void_p),
                ("trainable", C.c_void_p), ("anchor_sizes", C.c_void_p),
                ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("anchors", C.c_int32)]


TRAIN_METRICS_STATE_BYTES = 96   # RN_TRAIN_METRICS_STATE_BYTES
TRAIN_METRICS_MAX_WORKSPACE_BYTES = 65600   # RN_TRAIN_METRICS_MAX_WORKSPACE_BYTES


class DetLevel(C.Structure):
    _fields_ = [("prob", C.c_void_p), ("boxes", C.c_void_p), ("rows_per_image", C.c_int64),
                ("regression", C.c_void_p), ("anchor_sizes", C.c_void_p),
                ("grid_h", C.c_int32), ("grid_w", C.c_int32), ("num_anchors", C.c_int32),
                ("prob_f16", C.c_int32), ("regression_f16", C.c_int32), ("prob_is_logit", C.c_int32)]


class DetParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("num_classes", C.c_int32), ("max_per_class", C.c_int32),
                ("score_threshold", C.c_float), ("iou_threshold", C.c_float), ("max_candidates", C.c_int64)]


class DetPlan(C.Structure):
    """rn_det_plan: the kernels one rn_detect / rn_boxes_decode / rn_nms_classwise call launches (rn_detect_plan, host only)"""
    _fields_ = [("scan", C.c_int32), ("scan_half", C.c_int32), ("scan_logit", C.c_int32), ("scan_q", C.c_int32),
                ("scan_lds_per_wave", C.c_int32), ("scan_grid", C.c_int32), ("offsets_blocks", C.c_int32),
                ("emit_mode", C.c_int32), ("emit_grid", C.c_int32), ("emit_lds_bytes", C.c_int32),
                ("segments", C.c_int32), ("nseg", C.c_int32), ("workspace_bytes", C.c_uint64)]


# enum rn_det_scan / rn_det_emit / rn_det_segments
DET_SCANS = {0: None, 1: "T", 2: "T_PLAIN", 3: "Q", 4: "LDS", 5: "GENERIC"}
DET_EMITS = {0: None, 1: "HIST", 2: "STRIDED"}
DET_SEGMENTS = {1: "LDS_SCATTER", 2: "GLOBAL_SCATTER"}


class DwPlan(C.Structure):
    """rn_dw_plan: the kernels the rn_depthwise_* calls of one shape launch (rn_depthwise_plan, host only)"""
    _fields_ = [("oh", C.c_int32), ("ow", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32),
                ("fwd_kernel", C.c_int32), ("fwd_blocks", C.c_int32), ("dgrad_kernel", C.c_int32), ("dgrad_blocks", C.c_int32),
                ("wgrad_ok", C.c_int32), ("wgrad_chunks", C.c_int32), ("wgrad_ppc", C.c_int32), ("bwd_blocks", C.c_int32),
                ("stats_r", C.c_int32), ("stats_ppc", C.c_int32), ("stats_rows_per_sample", C.c_int32), ("stats_blocks", C.c_int32),
                ("wgrad_workspace_bytes", C.c_uint64)]


# enum rn_dw_fwd / rn_dw_dgrad
DW_FWDS = {0: None, 1: "k3", 2: "generic"}
DW_DGRADS = {0: None, 1: "k3_parity", 2: "k3", 3: "generic"}


_lib = None

# every symbol include/rn_hip.h declares (tests/test_abi.py checks the .so exports them all)
SYMBOLS = [
    "rn_version", "rn_last_error", "rn_same_pad",
    "rn_conv2d_fwd_workspace", "rn_conv2d_dgrad_workspace",
    "rn_zero", "rn_conv2d_fwd", "rn_conv2d_stats_rows", "rn_conv2d_fwd_stats", "rn_conv2d_dropout_rows", "rn_conv2d_fwd_dropout", "rn_depthwise_stats_rows", "rn_depthwise_fwd_stats", "rn_group_norm_rows_ok",
    "rn_conv2d_dgrad", "rn_conv2d_wgrad_workspace", "rn_conv2d_wgrad", "rn_conv2d_bwd",
    "rn_conv2d_bias_grad_workspace", "rn_conv2d_bias_grad", "rn_conv2d_plan", "rn_gemm_batched_plan", "rn_conv3x3_winograd_workspace", "rn_conv3x3_winograd",
    "rn_conv3x3_winograd_wgrad_workspace", "rn_conv3x3_winograd_wgrad", "rn_conv3x3_winograd_keep_bytes",
    "rn_conv3x3_winograd_bwd_workspace", "rn_conv3x3_winograd_bwd", "rn_flush_reductions", "rn_gemm_batched",
    "rn_winograd_bwd_products_workspace", "rn_winograd_bwd_products", "rn_wino_gn_rows", "rn_conv3x3_winograd_gn", "rn_conv3x3_winograd_gn_bwd", "rn_conv3x3_winograd_gn_bwd_wgrad", "rn_conv3x3_winograd_gn_plan", "rn_reduce_rows", "rn_resize_bilinear_normalize", "rn_resize_pair_u8",
    "rn_resize_pair_u8_augment_workspace", "rn_resize_pair_u8_augment",
    "rn_resize_pair_u8_batch", "rn_resize_pair_u8_augment_batch_workspace", "rn_resize_pair_u8_augment_batch",
    "rn_depthwise_fwd", "rn_depthwise_dgrad", "rn_depthwise_wgrad_workspace", "rn_depthwise_wgrad", "rn_depthwise_bwd", "rn_depthwise_plan",
    "rn_group_norm_sync_bytes", "rn_group_norm_workspace", "rn_group_norm_fwd", "rn_group_norm_bwd", "rn_group_norm_plan",
    "rn_act_fwd", "rn_act_bwd", "rn_upsample_add_fwd", "rn_upsample_add_bwd_top",
    "rn_pack_weights_f16", "rn_pack_weights_f16_bytes", "rn_cast_f32_to_f16", "rn_pad_cast_rgb_f16", "rn_conv2d_fwd_f16", "rn_conv2d_f16_fold_rows", "rn_conv2d_fwd_f16_fold", "rn_group_norm_finalize", "rn_group_norm_apply_f16", "rn_group_norm_apply_res_f16", "rn_maxpool_fwd_f16", "rn_maxpool_gn_fwd_f16", "rn_upsample_add_fwd_f16",
    "rn_act_fwd_f16", "rn_flip_width", "rn_dropout", "rn_dropout_strided", "rn_maxpool_fwd", "rn_maxpool_bwd", "rn_maxpool_bwd_arg", "rn_avgpool_fwd", "rn_avgpool_bwd",
    "rn_loss_workspace", "rn_loss_fwd", "rn_loss_bwd",
    "rn_loss_terms_stats_floats", "rn_loss_terms_workspace", "rn_loss_terms_fwd", "rn_loss_terms_bwd",
    "rn_regr_terms_workspace", "rn_regr_terms_fwd", "rn_regr_terms_bwd",
    "rn_iou", "rn_anchor_assign", "rn_anchor_assign_levels", "rn_anchor_assign_levels_pair", "rn_decode_boxes", "rn_detect_workspace", "rn_detect",
    "rn_boxes_decode", "rn_nms_classwise_workspace", "rn_nms_classwise", "rn_detect_plan",
    "rn_optimizer_workspace", "rn_grad_norm_l2reg", "rn_optimizer_update", "rn_counter_add", "rn_add_segs",
    "rn_mb_rows_max", "rn_mb_compact_rows_layout", "rn_mb_compact_rows", "rn_mb_pointwise_rows", "rn_mb_pointwise_fwd", "rn_mb_depthwise_rows", "rn_mb_depthwise_fwd", "rn_mb_apply",
    "rn_set_product_mode", "rn_get_product_mode",
    "rn_set_x3_bfrag", "rn_get_x3_bfrag", "rn_x3_bfrag_ok", "rn_x3_bfrag_bytes", "rn_x3_pack_bfrag", "rn_gemm_batched_bfrag", "rn_conv3x3_winograd_gn_u_bytes", "rn_conv3x3_winograd_gn_weights",
    "rn_conv2d_f16_stats_tiles", "rn_group_norm_fwd_f16_tiles", "rn_conv2d_f16_plan", "rn_conv2d_f16_pipe_available",
    "rn_mb_pointwise_bwd_rows", "rn_mb_pointwise_bwd_workspace", "rn_mb_pointwise_bwd",
    "rn_mb_depthwise_bwd_rows", "rn_mb_depthwise_bwd_workspace", "rn_mb_depthwise_bwd", "rn_set_mb_dw_taps", "rn_get_mb_dw_taps",
    "rn_debug_collective_standin", "rn_optimizer_norm_pairs", "rn_norm_reg_finalize",
    "rn_step_control_eval", "rn_grad_norm_partial",
    "rn_train_metrics_workspace", "rn_train_metrics_pass", "rn_train_metrics_fold", "rn_train_metrics_reset",
    "rn_depthwise_f16_rows", "rn_depthwise_fwd_f16", "rn_depthwise_f16_plan",
    "rn_avgpool_gn_fwd_f16", "rn_dense_f16_rows", "rn_dense_f16_put", "rn_dense_f16_finalize", "rn_dense_f16_norm", "rn_dense_f16_plan",
]


def lib():
    """Load librn_hip.so (built by `make -C retinanet-tensorflow_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RnError("librn_hip.so not found at %s: build it with "
                          "`make -C retinanet-tensorflow_amd/csrc` (there is no fallback path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        if not hasattr(L, "rn_version") or L.rn_version() != API_VERSION:
            raise RnError("%s reports ABI version %s, these bindings need %d: rebuild it (make -C retinanet-tensorflow_amd/csrc)"
                          % (LIB_PATH, L.rn_version() if hasattr(L, "rn_version") else "none", API_VERSION))
        L.rn_last_error.restype = C.c_char_p
        L.rn_group_norm_sync_bytes.argtypes = []
        for name in ("rn_conv2d_wgrad_workspace", "rn_depthwise_wgrad_workspace", "rn_group_norm_workspace", "rn_group_norm_sync_bytes",
                     "rn_loss_workspace", "rn_detect_workspace", "rn_optimizer_workspace",
                     "rn_conv2d_bias_grad_workspace", "rn_nms_classwise_workspace", "rn_conv3x3_winograd_workspace", "rn_conv2d_fwd_workspace",
                     "rn_conv2d_dgrad_workspace",
                     "rn_conv3x3_winograd_wgrad_workspace", "rn_conv3x3_winograd_bwd_workspace", "rn_wino_gn_rows",
                     "rn_winograd_bwd_products_workspace", "rn_conv2d_stats_rows", "rn_depthwise_stats_rows", "rn_conv2d_dropout_rows",
                     "rn_x3_bfrag_bytes", "rn_conv3x3_winograd_gn_u_bytes"):
            getattr(L, name).restype = C.c_size_t
        L.rn_optimizer_workspace.argtypes = [C.c_int64]
        L.rn_depthwise_fwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_depthwise_dgrad.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_depthwise_bwd.argtypes = [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_depthwise_wgrad_workspace.argtypes = [C.c_int] * 6
        L.rn_depthwise_plan.argtypes = [C.c_int] * 7 + [C.POINTER(DwPlan)]
        L.rn_depthwise_wgrad.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_conv2d_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_conv2d_dgrad.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_zero.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.rn_optimizer_norm_pairs.argtypes = [C.c_int64]
        L.rn_optimizer_norm_pairs.restype = C.c_int64
        L.rn_optimizer_update.argtypes = [C.POINTER(OptUpdate), C.c_void_p]
        L.rn_norm_reg_finalize.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.rn_step_control_eval.argtypes = [C.POINTER(StepControl), C.c_void_p]
        L.rn_grad_norm_partial.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
        L.rn_debug_collective_standin.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]
        L.rn_conv2d_stats_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.rn_conv2d_fwd_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_conv2d_dropout_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rn_conv2d_fwd_dropout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_depthwise_stats_rows.argtypes = [C.c_int] * 7 + [C.c_void_p]
        L.rn_group_norm_rows_ok.argtypes = [C.c_int] * 4
        L.rn_depthwise_fwd_stats.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
        L.rn_conv2d_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.POINTER(ConvPlan)]
        L.rn_gemm_batched_plan.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.POINTER(ConvPlan)]
        L.rn_conv2d_fwd_workspace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv2d_dgrad_workspace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv2d_bwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_conv2d_wgrad_workspace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv2d_wgrad.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_conv2d_bias_grad_workspace.argtypes = [C.c_int]
        L.rn_conv3x3_winograd_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.rn_resize_bilinear_normalize.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p,
                                                                                                         C.c_void_p]
        L.rn_resize_pair_u8.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        L.rn_resize_pair_u8_augment_workspace.argtypes = [C.c_int, C.c_int]
        L.rn_resize_pair_u8_augment_workspace.restype = C.c_size_t
        L.rn_resize_pair_u8_augment.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_resize_pair_u8_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.rn_resize_pair_u8_augment_batch_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
        L.rn_resize_pair_u8_augment_batch_workspace.restype = C.c_size_t
        L.rn_resize_pair_u8_augment_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_gemm_batched.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]
        L.rn_flush_reductions.argtypes = [C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_wgrad_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.rn_conv3x3_winograd_wgrad.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_bwd_workspace.argtypes = [C.c_void_p] + [C.c_int] * 6
        L.rn_conv3x3_winograd_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_keep_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_wino_gn_rows.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rn_winograd_bwd_products_workspace.argtypes = [C.c_int] * 4
        L.rn_winograd_bwd_products.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int] * 3 + \
                                              [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_x3_bfrag_ok.argtypes = [C.c_int] * 3
        L.rn_conv2d_f16_stats_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "rn_conv2d_f16_plan"):    # (added without an ABI bump, like the entries below: a library from before it still loads)
            L.rn_conv2d_f16_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(F16Plan)]
            L.rn_conv2d_f16_pipe_available.argtypes = []
        L.rn_group_norm_fwd_f16_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_gn_u_bytes.argtypes = [C.c_int] * 3
        L.rn_conv3x3_winograd_gn_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_x3_bfrag_bytes.argtypes = [C.c_int] * 3
        L.rn_x3_pack_bfrag.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
        L.rn_gemm_batched_bfrag.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]
        L.rn_set_x3_bfrag.argtypes = [C.c_int]
        L.rn_set_mb_dw_taps.argtypes = [C.c_int]
        L.rn_conv3x3_winograd_gn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_gn_bwd_wgrad.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                       C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv3x3_winograd_gn_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_conv3x3_winograd_gn_plan.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(WinoGnPlan)]
        L.rn_group_norm_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(GnPlan)]
        L.rn_reduce_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rn_conv2d_bias_grad.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p]
        L.rn_group_norm_workspace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_group_norm_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
        L.rn_group_norm_bwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_act_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.rn_act_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.rn_upsample_add_fwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_upsample_add_bwd_top.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_pack_weights_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.rn_pack_weights_f16_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.rn_pack_weights_f16_bytes.restype = C.c_size_t
        L.rn_cast_f32_to_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.rn_pad_cast_rgb_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.rn_conv2d_fwd_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv2d_f16_fold_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_conv2d_fwd_f16_fold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_depthwise_f16_rows.argtypes = [C.c_int] * 5
        L.rn_depthwise_fwd_f16.argtypes = [C.POINTER(DwF16), C.c_void_p]
        L.rn_depthwise_f16_plan.argtypes = [C.POINTER(DwF16), C.POINTER(DwF16Plan)]
        L.rn_group_norm_finalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_group_norm_apply_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rn_group_norm_apply_res_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rn_maxpool_fwd_f16.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_maxpool_gn_fwd_f16.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p]
        L.rn_avgpool_gn_fwd_f16.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p]
        L.rn_dense_f16_rows.argtypes = [C.c_int]
        L.rn_dense_f16_put.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]
        L.rn_dense_f16_finalize.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_dense_f16_norm.argtypes = [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.rn_dense_f16_plan.argtypes = [C.c_int] * 7 + [C.POINTER(DenseF16Plan)]
        L.rn_upsample_add_fwd_f16.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_act_fwd_f16.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.rn_flip_width.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.rn_dropout_strided.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 5 + [C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]
        L.rn_dropout.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p]
        L.rn_maxpool_fwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_maxpool_bwd_arg.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_maxpool_bwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_avgpool_fwd.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_avgpool_bwd.argtypes = [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p]
        L.rn_loss_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.rn_loss_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p]
        L.rn_loss_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
        L.rn_loss_terms_stats_floats.restype = C.c_size_t
        L.rn_loss_terms_stats_floats.argtypes = [C.c_int]
        L.rn_loss_terms_workspace.restype = C.c_size_t
        L.rn_loss_terms_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LossTerms)]
        L.rn_loss_terms_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LossTerms), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_loss_terms_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(LossTerms), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        L.rn_regr_terms_workspace.restype = C.c_size_t
        L.rn_regr_terms_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RegrTerms)]
        L.rn_regr_terms_fwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(RegrTerms), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]
        L.rn_regr_terms_bwd.argtypes = [C.c_void_p, C.c_int, C.POINTER(RegrTerms), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_iou.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rn_anchor_assign.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 4 + \
                                      [C.c_void_p] * 4 + [C.c_void_p]
        L.rn_anchor_assign_levels.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p]
        L.rn_anchor_assign_levels_pair.argtypes = L.rn_anchor_assign_levels.argtypes
        L.rn_decode_boxes.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]
        L.rn_detect_workspace.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_detect.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 6 + [C.c_void_p, C.c_size_t,
                                                                                     C.c_void_p]
        L.rn_boxes_decode.argtypes = L.rn_detect.argtypes
        L.rn_nms_classwise_workspace.argtypes = [C.c_void_p]
        L.rn_detect_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(DetPlan)]
        L.rn_nms_classwise.argtypes = [C.c_void_p] * 5 + [C.c_void_p] + [C.c_void_p] * 6 + [C.c_void_p, C.c_size_t,
                                                                                        C.c_void_p]
        L.rn_grad_norm_l2reg.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                                             C.c_size_t, C.c_void_p]
        L.rn_counter_add.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.rn_add_segs.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for name in ("rn_mb_pointwise_rows", "rn_mb_depthwise_rows", "rn_mb_pointwise_bwd_rows", "rn_mb_pointwise_bwd_workspace",
                     "rn_mb_depthwise_bwd_rows", "rn_mb_depthwise_bwd_workspace"):
            getattr(L, name).restype = C.c_size_t
        L.rn_mb_compact_rows_layout.restype = C.c_size_t
        L.rn_mb_compact_rows_layout.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.rn_mb_compact_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rn_mb_pointwise_rows.argtypes = [C.c_int] * 5 + [C.c_void_p]
        L.rn_mb_pointwise_fwd.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_mb_depthwise_rows.argtypes = [C.c_int] * 6 + [C.c_void_p]
        L.rn_mb_depthwise_fwd.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]
        L.rn_mb_apply.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p]
        L.rn_mb_pointwise_bwd_rows.argtypes = [C.c_int] * 5 + [C.c_void_p]
        L.rn_mb_pointwise_bwd_workspace.argtypes = [C.c_int] * 4
        L.rn_mb_pointwise_bwd.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rn_mb_depthwise_bwd_rows.argtypes = [C.c_int] * 6 + [C.c_void_p]
        L.rn_mb_depthwise_bwd_workspace.argtypes = [C.c_int] * 5
        L.rn_mb_depthwise_bwd.argtypes = [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        # (the entries were added without an ABI bump -- no existing entry or struct changed -- so a library of the same version
        # from before them loads for A/B measurements; metrics.TrainMetrics raises if they are missing)
        if hasattr(L, "rn_train_metrics_pass"):
            L.rn_train_metrics_workspace.restype = C.c_size_t
            L.rn_train_metrics_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.rn_train_metrics_pass.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
            L.rn_train_metrics_fold.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.rn_train_metrics_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.rn_same_pad.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.rn_same_pad.restype = None
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise RnError("%s failed (status %d): %s" % (what, status, lib().rn_last_error().decode()))


def same_pad(n, k, s):
    """TF SAME rule -> (out, pad_before); host-side mirror of rn_same_pad."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def ptr(t):
    """Raw device pointer of a contiguous fp32/u8/int tensor on the GPU (or None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RnError("rn_hip kernels need device tensors (got a CPU tensor): there is no CPU fallback")
    if not t.is_contiguous():
        raise RnError("rn_hip kernels need contiguous tensors")
    return t.data_ptr()


def f32(t):
    if t.dtype != torch.float32:
        raise RnError("this rn_hip kernel is fp32 (got %s)" % t.dtype)
    return ptr(t)


def f16(t):
    if t.dtype != torch.float16:
        raise RnError("this rn_hip kernel takes fp16 storage (got %s)" % t.dtype)
    return ptr(t)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# one scratch arena per device, reused by every op (ops are stream-ordered); grown on demand
_workspaces = {}
WORKSPACE_MIN_BYTES = 256 << 20


SIDE_STREAMS = set()   # raw handles of streams that run concurrently with the main one
_side_streams = {}


_sync_words = {}


def sync_counters(device):
    """The zeroed region (rn_group_norm_sync_bytes()) per (device, current stream) for rn_gn_params.sync: counters and
    exchange rows of the grid-resident GroupNorm path.  Word 2 is set if a wait ever timed out."""
    # one region per stream HANDLE (two grid-resident kernels that run concurrently on different streams must not share
    # tags / exchange rows).  Nothing may be allocated (and zero-filled) inside a graph capture: a capturing stream without
    # a region of its own takes the region of key 0 -- the one the warm-up pass before the capture sized -- which it shares
    # with nobody while the capture (and later the replay, on the stream that replays it) is the only user.
    # Keys: a registered side stream has its own region (it runs concurrently with the main one); EVERY other stream -- the
    # default stream, a warm-up stream, the capture stream: whichever is "the main stream" at the moment, never two at once --
    # shares the region of key 0.  (A side stream never donates its region to key 0, and warm-up streams made for a
    # re-capture do not leak a region each.)
    h = stream().value or 0
    capturing = torch.cuda.is_current_stream_capturing() if device.type == 'cuda' else False
    key = (device.type, device.index, h if h in SIDE_STREAMS else 0)
    if key[2] == 0:
        _hand_over(key, h, device)
    t = _sync_words.get(key)
    if t is None:
        if capturing:
            raise RnError("the grid-resident GroupNorm's exchange region must exist before graph capture (run the step once eagerly)")
        t = torch.zeros(lib().rn_group_norm_sync_bytes() // 4, dtype=torch.int32, device=device)
        _sync_words[key] = t
    return t


_region_owner = {}     # region key -> raw handle of the stream that used the shared "main stream" region last


def _hand_over(key, h, device):
    """The regions of key 0 are shared by every stream that is not a registered side stream, on the understanding that only one
    of them runs these kernels at a time.  Enforced here instead of assumed: when a DIFFERENT stream asks for the region, it is
    made to wait for everything the previous user has queued (an event recorded on that stream now), so two such streams --
    say an evaluation stream beside the training stream -- serialise on the region instead of sharing barrier words.  Inside a
    graph capture nothing can be recorded on an outside stream: the capture's owner (train.Trainer) orders it behind the warm-up
    stream itself."""
    last = _region_owner.get(key)
    if last is not None and last != h and device.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
        try:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.ExternalStream(last, device=device) if last else torch.cuda.default_stream(device))
            torch.cuda.current_stream(device).wait_event(ev)
        except RuntimeError:
            pass                # (the previous stream no longer exists: nothing left to wait for)
    if device.type != 'cuda' or not torch.cuda.is_current_stream_capturing():
        # (a capture stream is not an owner anyone can wait for later: it may be gone by then, and nothing could be recorded on
        # it from outside anyway -- the previous REAL owner stays on record)
        _region_owner[key] = h


def barrier_timeouts():
    """Number of (device, stream) exchange regions of the grid-resident GroupNorm whose error word is set (should always be 0)."""
    return sum(int(t[2].item()) for t in {id(t): t for t in _sync_words.values()}.values())


def reset_barrier_timeouts():
    """Clear the error words (after the caller has dealt with a reported timeout, e.g. by switching the path off)."""
    for t in {id(t): t for t in _sync_words.values()}.values():
        t[2] = 0


def side_stream(device, index=0):
    """A stream (per device and index) for work that may overlap the main stream; it gets its own workspace."""
    key = (device.type, device.index, index)
    st = _side_streams.get(key)
    if st is None:
        lo, hi = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, 'priority_range') else (0, 0)
        st = torch.cuda.Stream(device=device, priority=int(os.environ.get('RN_SIDE_PRIO', lo)))  # lowest priority
        _side_streams[key] = st
        SIDE_STREAMS.add(st.cuda_stream)
    return st


def join_side_streams(device, skip=()):
    """Make the current stream wait for everything queued on this device's side streams (except the indices in `skip`)."""
    cur = torch.cuda.current_stream(device)
    for (t, i, idx), st in _side_streams.items():
        if t == device.type and i == device.index and idx not in skip:
            cur.wait_stream(st)


def workspace(nbytes, device):
    # one arena for the main stream (whichever stream that currently is: default, warm-up or graph-capture
    # stream) and one per registered side stream: ops on a side stream run concurrently with the main one
    h = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    key = (device.type, device.index, h if h in SIDE_STREAMS else 0)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RnError("workspace must be sized before graph capture (need %d bytes)" % nbytes)
        size = max(int(nbytes), WORKSPACE_MIN_BYTES)
        ws = torch.empty(size, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws
