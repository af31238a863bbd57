"""ctypes binding of libbd_hip.so (C ABI declared in include/bd_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, a RuntimeError is
raised (never a silent PyTorch/CPU substitute).
"""
import ctypes as C
import os

import torch  # noqa: F401  -- must be imported first so libbd_hip.so binds to torch's HIP runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbd_hip.so")

i32, i64, f32, f64, vp, sz = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_size_t


class PoisonQsampleDesc(C.Structure):
    _fields_ = [("B", i32), ("C", i32), ("H", i32), ("W", i32),
                ("images_f32", vp), ("images_u8", vp), ("is_poison", vp), ("trigger", vp), ("target_img", vp),
                ("noise", vp), ("timesteps", vp), ("alphas", vp), ("alphas_cumprod", vp), ("vmin", f32),
                ("x_noisy", vp), ("ld_noisy", i64), ("target", vp), ("ld_target", i64),
                ("R_out", vp), ("x0_out", vp), ("mask_out", vp), ("image_out", vp), ("row_index", vp), ("flip", vp)]


class QsampleDesc(C.Structure):
    _fields_ = [("B", i32), ("C", i32), ("H", i32), ("W", i32), ("x0", vp), ("R", vp), ("noise", vp),
                ("timesteps", vp), ("alphas", vp), ("alphas_cumprod", vp),
                ("x_noisy", vp), ("ld_noisy", i64), ("target", vp), ("ld_target", i64)]


class PoisonQsampleCorrDesc(C.Structure):
    _fields_ = PoisonQsampleDesc._fields_ + [("corr", vp)]


class QsampleCorrDesc(C.Structure):
    _fields_ = QsampleDesc._fields_ + [("corr", vp)]


class DdpmStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("noise", vp), ("prev_sample", vp),
                ("pred_original", vp), ("alphas_cumprod", vp), ("t", i32), ("prev_t", i32), ("variance_type", i32),
                ("clip_sample", i32), ("clip_sample_range", f32), ("clip_defense", i32), ("clip_defense_range", f32),
                ("x0_quantile", vp), ("image_elems", i64), ("sample_max_value", f32)]


class DdimStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("noise", vp), ("prev_sample", vp),
                ("pred_original", vp), ("alphas_cumprod", vp), ("t", i32), ("prev_t", i32),
                ("final_alpha_cumprod", f32), ("eta", f32), ("clip_sample", i32), ("clip_sample_range", f32),
                ("x0_quantile", vp), ("image_elems", i64), ("sample_max_value", f32)]


class AbsQuantileDesc(C.Structure):
    _fields_ = [("B", i32), ("m", i64), ("x", vp), ("model_output", vp), ("alphas_cumprod", vp), ("n_alphas", i32), ("t", i32),
                ("q", f32), ("out", vp), ("workspace", vp), ("workspace_bytes", sz)]


AQ_REGISTERS, AQ_STREAM = 0, 1


class AbsQuantilePlanInfo(C.Structure):
    """bd_abs_quantile_plan_info; path is enum bd_abs_quantile_path"""
    _fields_ = [("path", i32), ("workgroups", i32), ("threads", i32), ("values_per_thread", i32), ("passes", i32), ("switch_m", i64),
                ("workspace_bytes", sz)]


REPAINT_UNDO_MAX = 8


class RepaintStepDesc(C.Structure):
    _fields_ = [("N", i32), ("C", i32), ("H", i32), ("W", i32), ("stride", i64 * 4), ("model_output", vp), ("sample", vp), ("noise", vp),
                ("prev_sample", vp), ("pred_original", vp), ("original_image", vp), ("orig_stride", i64 * 4), ("mask", vp),
                ("mask_stride", i64 * 4), ("shift", vp), ("shift_stride", i64 * 4), ("alphas_cumprod", vp), ("n_alphas", i32),
                ("t", i32), ("prev_t", i32), ("final_alpha_cumprod", f32), ("eta", f32), ("clip_sample", i32), ("clip_sample_range", f32)]


class RepaintUndoDesc(C.Structure):
    _fields_ = [("N", i32), ("C", i32), ("H", i32), ("W", i32), ("stride", i64 * 4), ("sample", vp), ("out", vp), ("shift", vp),
                ("shift_stride", i64 * 4), ("betas", vp), ("n_betas", i32), ("t", i32), ("k", i32)]


class DpmStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("m1", vp), ("m2", vp), ("m0_out", vp), ("prev_out", vp),
                ("convert", i32), ("alpha_s", f32), ("sigma_s", f32), ("x0_clip", i32), ("x0_range", f32),
                ("cx", f32), ("c0", f32), ("c1", f32), ("c2", f32), ("clip", i32), ("clip_range", f32)]


class UnipcStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("last_sample", vp), ("h1", vp), ("h2", vp), ("h3", vp),
                ("m0_out", vp), ("corrected_out", vp), ("prev_out", vp),
                ("convert", i32), ("alpha_s", f32), ("sigma_s", f32), ("x0_clip", i32), ("x0_range", f32),
                ("kl", f32), ("k0", f32), ("k1", f32), ("k2", f32), ("k3", f32), ("px", f32), ("p0", f32), ("p1", f32), ("p2", f32),
                ("clip", i32), ("clip_range", f32)]


class DeisStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("m1", vp), ("m2", vp), ("m0_out", vp), ("prev_out", vp),
                ("alpha_s", f32), ("sigma_s", f32), ("x0_clip", i32), ("x0_range", f32), ("cx", f32), ("c0", f32),
                ("alpha_t", f32), ("k0", f32), ("k1", f32), ("k2", f32), ("clip", i32), ("clip_range", f32)]


class SigmaStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("base", vp), ("h1", vp), ("h2", vp), ("h3", vp),
                ("x0_out", vp), ("d_out", vp), ("prev_out", vp), ("scaled_out", vp), ("sigma_in", f32), ("average", i32),
                ("c0", f32), ("c1", f32), ("c2", f32), ("c3", f32), ("in_div", f32), ("clip", i32), ("clip_range", f32)]


class SigmaNoiseStepDesc(C.Structure):
    _fields_ = [("n", i64), ("model_output", vp), ("sample", vp), ("noise", vp), ("base", vp), ("x0_out", vp), ("prev_out", vp),
                ("scaled_out", vp), ("sigma_in", f32), ("dt", f32), ("churn", i32), ("s_noise", f32), ("churn_mul", f32),
                ("up", i32), ("sigma_up", f32), ("in_div", f32), ("clip", i32), ("clip_range", f32)]


class GnFwdDesc(C.Structure):
    _fields_ = [("B", i32), ("HW", i32), ("C", i32), ("G", i32), ("eps", f32), ("silu", i32),
                ("x", vp), ("ldx", i64), ("gamma", vp), ("beta", vp), ("y", vp), ("ldy", i64),
                ("mean", vp), ("rstd", vp), ("workspace", vp), ("workspace_bytes", sz),
                ("y_split", vp), ("ldys", i64), ("stats", vp), ("stats_splits", i32)]


class GnBwdDesc(C.Structure):
    _fields_ = [("B", i32), ("HW", i32), ("C", i32), ("G", i32), ("silu", i32),
                ("x", vp), ("ldx", i64), ("gamma", vp), ("beta", vp), ("mean", vp), ("rstd", vp),
                ("dy", vp), ("lddy", i64), ("dx", vp), ("lddx", i64), ("accumulate_dx", i32),
                ("dgamma", vp), ("dbeta", vp), ("workspace", vp), ("workspace_bytes", sz),
                ("dx_colsum", vp), ("ld_colsum", i64), ("dx_split", vp), ("lddxs", i64),
                ("dx_add", vp), ("ld_add", i64), ("param_partials", vp), ("dx_split_c0", i32), ("dx_split_c1", i32)]


class GnParamItem(C.Structure):
    _fields_ = [("partials", vp), ("C", i32), ("dgamma", vp), ("dbeta", vp)]


class GnPlanInfo(C.Structure):
    _fields_ = [("resident", i32), ("nt", i32), ("cb", i32), ("q", i32), ("R", i32), ("E", i32), ("emax", i32),
                ("S", i32), ("threads", i32), ("r", i32), ("per", i32), ("workspace_bytes", sz)]


class Operand(C.Structure):
    _fields_ = [("kind", i32), ("kc", i32), ("p", vp), ("ld", i64), ("bs_outer", i64), ("bs_inner", i64),
                ("C", i32), ("Hs", i32), ("Ws", i32), ("Ho", i32), ("Wo", i32), ("stride", i32),
                ("pad_t", i32), ("pad_l", i32), ("ups", i32), ("split", vp)]


class IgemmDesc(C.Structure):
    _fields_ = [("A", Operand), ("B", Operand), ("M", i32), ("N", i32), ("K", i32),
                ("batch_outer", i32), ("batch_inner", i32),
                ("C", vp), ("ldc", i64), ("c_bs_outer", i64), ("c_bs_inner", i64),
                ("alpha", f32), ("out_scale", f32), ("bias", vp),
                ("rowbias", vp), ("ld_rowbias", i64), ("rows_per_group", i32),
                ("residual", vp), ("ldr", i64), ("accumulate", i32), ("ksplit", i32),
                ("workspace", vp), ("workspace_bytes", sz), ("tile", i32), ("mode", i32),
                ("a_colsum", vp)]


class IgemmPlanInfo(C.Structure):
    _fields_ = [("cls", i32), ("fast", i32), ("a_vec", i32), ("b_vec", i32), ("tile", i32), ("threads", i32), ("depth", i32),
                ("ksplit", i32), ("chunks_per_split", i32), ("reduce", i32), ("workspace_bytes", sz), ("colsum_offset", sz)]


class ConvFwdDesc(C.Structure):
    _fields_ = [("B", i32), ("Hs", i32), ("Ws", i32), ("Cin", i32), ("Cout", i32), ("stride", i32),
                ("pad_t", i32), ("pad_l", i32), ("ups", i32), ("Ho", i32), ("Wo", i32),
                ("x", vp), ("ldx", i64), ("w", vp), ("bias", vp), ("rowbias", vp), ("ld_rowbias", i64),
                ("residual", vp), ("ldr", i64), ("out_scale", f32), ("y", vp), ("ldy", i64),
                ("workspace", vp), ("workspace_bytes", sz), ("mode", i32), ("w_split", vp)]


class ConvDgradDesc(C.Structure):
    _fields_ = [("B", i32), ("Hs", i32), ("Ws", i32), ("Cin", i32), ("Cout", i32), ("stride", i32),
                ("pad_t", i32), ("pad_l", i32), ("ups", i32), ("Ho", i32), ("Wo", i32),
                ("dy", vp), ("lddy", i64), ("w", vp), ("dx", vp), ("lddx", i64), ("accumulate", i32),
                ("workspace", vp), ("workspace_bytes", sz), ("mode", i32), ("w_split", vp)]


class ConvWgradDesc(C.Structure):
    _fields_ = [("B", i32), ("Hs", i32), ("Ws", i32), ("Cin", i32), ("Cout", i32), ("stride", i32),
                ("pad_t", i32), ("pad_l", i32), ("ups", i32), ("Ho", i32), ("Wo", i32),
                ("x", vp), ("ldx", i64), ("dy", vp), ("lddy", i64), ("dw", vp),
                ("workspace", vp), ("workspace_bytes", sz), ("mode", i32), ("db", vp)]


class ThinPlanInfo(C.Structure):
    """bd_conv3x3_thin_plan_info; path is enum bd_thin_path, prof_class a C string or None"""
    _fields_ = [("path", i32), ("J", i32), ("loops", i32), ("pix_per_block", i32), ("grid_x", i32), ("grid_y", i32),
                ("partial_rows", i32), ("workspace_bytes", sz), ("prof_class", C.c_char_p)]


class ConvPsDesc(C.Structure):
    _fields_ = [("B", i32), ("H", i32), ("W", i32), ("K", i32), ("N", i32), ("direction", i32),
                ("x_split", vp), ("ldx", i64), ("w_split", vp), ("bias", vp), ("rowbias", vp), ("ld_rowbias", i64),
                ("residual", vp), ("ldr", i64), ("out_scale", f32), ("y", vp), ("ldy", i64), ("accumulate", i32),
                ("workspace", vp), ("workspace_bytes", sz), ("gn_part", vp), ("gn_groups", i32), ("mode", i32)]


class ConvPsWgradDesc(C.Structure):
    _fields_ = [("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32), ("x_split", vp), ("ldx", i64),
                ("dy_split", vp), ("lddy", i64), ("dw", vp), ("db", vp), ("workspace", vp), ("workspace_bytes", sz),
                ("mode", i32)]


PS_256, PS_256_SHARED_TAP, PS_128 = 0, 1, 2                    # enum bd_ps_kernel
PS_WGRAD, PS_WGRAD_SHARED_TAP, PS_WGRAD_PHASE = 0, 1, 2        # enum bd_ps_wgrad_kernel


class ConvPsPlanInfo(C.Structure):
    """bd_conv3x3_ps_plan_info; kernel is enum bd_ps_kernel, prof_class a C string"""
    _fields_ = [("kernel", i32), ("tiles_m", i32), ("tiles_n", i32), ("ksplit", i32), ("chunks_per_split", i32), ("stages", i32),
                ("reduce", i32), ("grid", i32), ("gn_splits", i32), ("workspace_bytes", sz), ("prof_class", C.c_char_p)]


class ConvPsWgradPlanInfo(C.Structure):
    """bd_conv3x3_ps_wgrad_plan_info; kernel is enum bd_ps_wgrad_kernel, prof_class a C string"""
    _fields_ = [("kernel", i32), ("ntaps", i32), ("tiles_m", i32), ("tiles_n", i32), ("slots", i32), ("ksplit", i32),
                ("chunks_per_split", i32), ("reduce", i32), ("grid", i32), ("bias_rows", i32), ("slab_floats", sz),
                ("workspace_bytes", sz), ("de_offset", sz), ("prof_class", C.c_char_p)]


class UpsampleConvDesc(C.Structure):
    _fields_ = [("B", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32), ("x_split", vp), ("ldx", i64), ("dy_split", vp),
                ("lddy", i64), ("e_split", vp), ("et_split", vp), ("bias", vp), ("y", vp), ("ldy", i64), ("dx", vp), ("lddx", i64),
                ("accumulate", i32), ("dw", vp), ("db", vp), ("workspace", vp), ("workspace_bytes", sz), ("mode", i32)]


class ConvS2DgradDesc(C.Structure):
    _fields_ = [("B", i32), ("Ho", i32), ("Wo", i32), ("Cin", i32), ("Cout", i32), ("pad", i32), ("dy_split", vp), ("lddy", i64),
                ("wT_split", vp), ("dx", vp), ("lddx", i64), ("accumulate", i32), ("mode", i32)]


class GemmSpDesc(C.Structure):
    _fields_ = [("M", i32), ("N", i32), ("K", i32), ("batch", i32), ("a", vp), ("lda", i64), ("a_bs", i64), ("a_kmajor", i32),
                ("b", vp), ("ldb", i64), ("b_bs", i64), ("b_kmajor", i32), ("c", vp), ("ldc", i64), ("c_bs", i64),
                ("c_split", vp), ("ldcs", i64), ("cs_bs", i64), ("bias", vp), ("residual", vp), ("ldr", i64), ("r_bs", i64),
                ("alpha", f32), ("out_scale", f32), ("accumulate", i32), ("a_colsum", vp), ("workspace", vp), ("workspace_bytes", sz),
                ("mode", i32)]


class GemmSpPlanInfo(C.Structure):
    """bd_gemm_sp_plan_info; form is 2 * a_kmajor + b_kmajor, prof_class a C string"""
    _fields_ = [("form", i32), ("tiles_m", i32), ("tiles_n", i32), ("batch", i32), ("ksplit", i32), ("chunks_per_split", i32),
                ("reduce", i32), ("colsum_reduce", i32), ("grid", i64), ("workspace_bytes", sz), ("colsum_offset", sz),
                ("prof_class", C.c_char_p)]


class AttnSpDesc(C.Structure):
    _fields_ = [("B", i32), ("heads", i32), ("N", i32), ("dh", i32), ("qkv_split", vp), ("ld", i64), ("scale", f32), ("o_split", vp),
                ("ldo", i64), ("pt_split", vp), ("do_split", vp), ("lddo", i64), ("dst_split", vp), ("dqkv_split", vp), ("lddqkv", i64),
                ("mode", i32)]


class Conv2dDesc(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("w", vp), ("bias", vp), ("y", vp), ("ldy", i64), ("B", i32), ("H", i32), ("W", i32), ("Cin", i32),
                ("Cout", i32), ("KH", i32), ("KW", i32), ("stride_h", i32), ("stride_w", i32), ("pad_h", i32), ("pad_w", i32), ("relu", i32),
                ("w_kc", i32)]


LOSS_MAX_GROUPS = 4


class LossGroupsDesc(C.Structure):
    _fields_ = [("n_groups", i32), ("group_rows", i64 * LOSS_MAX_GROUPS), ("group_weight", f32 * LOSS_MAX_GROUPS)]


class ImagePairDesc(C.Structure):
    _fields_ = [("N", i32), ("C", i32), ("H", i32), ("W", i32), ("preds", vp), ("p_stride", i64 * 4), ("target", vp), ("t_stride", i64 * 4)]


class CrossPlanInfo(C.Structure):
    _fields_ = [("strips", i32), ("col_tiles", i32), ("csplit", i32), ("tiles_per_split", i32), ("csplit_cap", i32)]


class VbTermsDesc(C.Structure):
    _fields_ = [("N", i32), ("C", i32), ("H", i32), ("W", i32), ("x0", vp), ("x0_stride", i64 * 4), ("x_t", vp), ("xt_stride", i64 * 4),
                ("eps", vp), ("eps_stride", i64 * 4), ("t", vp), ("t_host", vp), ("alphas_cumprod", vp), ("T", i32),
                ("term_add", vp), ("term_mul", vp), ("inv_sigma_dec", f32), ("clip_denoised", i32), ("bits", vp), ("x0_mse", vp)]


class VbTermsShiftDesc(C.Structure):
    _fields_ = VbTermsDesc._fields_ + [("r", vp), ("r_stride", i64 * 4), ("term_shift", vp)]


class UnetConfig(C.Structure):
    _fields_ = [("sample_size", i32), ("in_channels", i32), ("out_channels", i32), ("num_blocks", i32),
                ("block_out_channels", i32 * 8), ("down_attn", i32 * 8), ("up_attn", i32 * 8),
                ("layers_per_block", i32), ("downsample_padding", i32), ("flip_sin_to_cos", i32),
                ("freq_shift", f32), ("norm_eps", f32), ("norm_num_groups", i32), ("attention_head_dim", i32),
                ("mid_block_scale_factor", f32), ("compute_mode", i32)]


# name -> (restype, argtypes).  Every symbol declared in include/bd_hip.h must appear here
# (tests/test_abi.py cross-checks the header against this table and the built library).
SIGNATURES = {
    "bd_last_error": (C.c_char_p, []),
    "bd_version": (i32, []),
    "bd_poison_qsample": (i32, [C.POINTER(PoisonQsampleDesc), vp]),
    "bd_qsample": (i32, [C.POINTER(QsampleDesc), vp]),
    "bd_poison_qsample_corr": (i32, [C.POINTER(PoisonQsampleCorrDesc), vp]),
    "bd_qsample_corr": (i32, [C.POINTER(QsampleCorrDesc), vp]),
    "bd_nchw_to_nhwc": (i32, [vp, vp, i32, i32, i32, i32, i64, vp]),
    "bd_nhwc_to_nchw": (i32, [vp, i64, vp, i32, i32, i32, i32, vp]),
    "bd_ddpm_step": (i32, [C.POINTER(DdpmStepDesc), vp]),
    "bd_ddim_step": (i32, [C.POINTER(DdimStepDesc), vp]),
    "bd_abs_quantile_workspace_bytes": (sz, [i32, i64]),
    "bd_abs_quantile": (i32, [C.POINTER(AbsQuantileDesc), vp]),
    "bd_abs_quantile_plan": (i32, [i32, i64, C.POINTER(AbsQuantilePlanInfo)]),
    "bd_to_image": (i32, [vp, i32, i64, i32, i32, i32, i32, vp, vp, vp]),
    "bd_timestep_embedding": (i32, [vp, i32, i32, i32, i32, f32, vp, vp]),
    "bd_gn_workspace_bytes": (sz, [i32, i32]),
    "bd_gn_fwd_takes_stats": (i32, [i32, i32, i32, i32]),
    "bd_gn_fwd": (i32, [C.POINTER(GnFwdDesc), vp]),
    "bd_gn_bwd": (i32, [C.POINTER(GnBwdDesc), vp]),
    "bd_lincomb": (i32, [i32, C.POINTER(vp), C.POINTER(f32), i64, i32, f32, vp, vp]),
    "bd_dpm_step": (i32, [C.POINTER(DpmStepDesc), vp]),
    "bd_unipc_step": (i32, [C.POINTER(UnipcStepDesc), vp]),
    "bd_deis_step": (i32, [C.POINTER(DeisStepDesc), vp]),
    "bd_sigma_step": (i32, [C.POINTER(SigmaStepDesc), vp]),
    "bd_sigma_noise_step": (i32, [C.POINTER(SigmaNoiseStepDesc), vp]),
    "bd_scale_input": (i32, [vp, i64, f32, f32, vp, vp]),
    "bd_timestep_embedding_f32": (i32, [vp, i32, i32, i32, i32, f32, vp, vp]),
    "bd_unet_forward_tf": (i32, [vp, i32, i32, vp, vp, i64, vp, i32, vp, i64, vp, sz, vp]),
    "bd_repaint_step": (i32, [C.POINTER(RepaintStepDesc), vp]),
    "bd_repaint_undo": (i32, [C.POINTER(RepaintUndoDesc), C.POINTER(vp), vp]),
    "bd_anp_apply": (i32, [vp, i64, vp, vp, vp, i32, i64, vp, vp]),
    "bd_anp_grad": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, vp, vp]),
    "bd_ssim_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "bd_ssim": (i32, [vp, vp, i32, i32, i32, i32, i64, i64, i64, i64, f32, vp, vp, sz, vp]),
    "bd_pairwise_sqdist_workspace_bytes": (sz, [i32, i32]),
    "bd_pairwise_sqdist": (i32, [vp, i64, i32, i32, vp, i64, vp, sz, vp]),
    "bd_total_variation": (i32, [vp, i32, i32, i32, i32, i64, i64, i64, i64, vp, vp]),
    "bd_cross_plan": (i32, [i32, i32, i32, C.POINTER(CrossPlanInfo)]),
    "bd_knn_sqradius_workspace_bytes": (sz, [i32, i32, i32]),
    "bd_knn_sqradius": (i32, [vp, i64, i32, i32, i32, vp, vp, sz, vp]),
    "bd_cross_ksmallest_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "bd_cross_ksmallest": (i32, [vp, i64, i32, vp, i64, i32, i32, i32, i64, vp, vp, sz, vp]),
    "bd_cross_count_min_workspace_bytes": (sz, [i32, i32, i32]),
    "bd_cross_count_min": (i32, [vp, i64, i32, vp, i64, i32, i32, vp, vp, vp, vp, sz, vp]),
    "bd_poly3_rowsum_workspace_bytes": (sz, [i32, i32, i32]),
    "bd_poly3_rowsum": (i32, [vp, i64, i32, vp, i64, i32, i32, i32, vp, vp, sz, vp]),
    "bd_image_loss_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "bd_image_loss": (i32, [C.POINTER(ImagePairDesc), i32, vp, vp, sz, vp]),
    "bd_ssim_images_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "bd_ssim_images": (i32, [C.POINTER(ImagePairDesc), f32, vp, vp, sz, vp]),
    "bd_vb_terms_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "bd_vb_terms": (i32, [C.POINTER(VbTermsDesc), vp, sz, vp]),
    "bd_vb_terms_shift": (i32, [C.POINTER(VbTermsShiftDesc), vp, sz, vp]),
    "bd_conv2d_nhwc": (i32, [C.POINTER(Conv2dDesc), vp]),
    "bd_pool2d_nhwc": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "bd_resize_bilinear_nhwc": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, i32, f32, f32, vp]),
    "bd_global_avgpool_nhwc": (i32, [vp, i64, vp, i32, i32, i32, vp]),
    "bd_gn_bwd_defers": (i32, [i32, i32, i32, i32]),
    "bd_gn_bwd_params": (i32, [C.POINTER(GnParamItem), i32, i32, vp]),
    "bd_gn_plan": (i32, [i32, i32, i32, i32, i32, C.POINTER(GnPlanInfo)]),
    "bd_igemm_workspace_bytes": (sz, [C.POINTER(IgemmDesc)]),
    "bd_igemm_plan": (i32, [C.POINTER(IgemmDesc), C.POINTER(IgemmPlanInfo)]),
    "bd_igemm": (i32, [C.POINTER(IgemmDesc), vp]),
    "bd_split_bf16": (i32, [vp, i64, vp, vp]),
    "bd_split_rows": (i32, [vp, i64, i64, i32, vp, i64, vp]),
    "bd_split_wt": (i32, [vp, i32, i32, vp, vp]),
    "bd_split_rows_ups2": (i32, [vp, i64, i32, i32, i32, i32, vp, i64, vp]),
    "bd_conv3x3_ps": (i32, [C.POINTER(ConvPsDesc), vp]),
    "bd_conv3x3_ps_workspace_bytes": (sz, [C.POINTER(ConvPsDesc)]),
    "bd_conv3x3_ps_gn_splits": (i32, [i32, i32, i32, i32, i32, i32]),
    "bd_conv3x3_ps_plan": (i32, [C.POINTER(ConvPsDesc), C.POINTER(ConvPsPlanInfo)]),
    "bd_upsample_weights": (i32, [vp, i32, i32, vp, vp, vp]),
    "bd_upsample_conv_fwd": (i32, [C.POINTER(UpsampleConvDesc), vp]),
    "bd_upsample_conv_dgrad": (i32, [C.POINTER(UpsampleConvDesc), vp]),
    "bd_upsample_conv_wgrad": (i32, [C.POINTER(UpsampleConvDesc), vp]),
    "bd_upsample_conv_wgrad_workspace_bytes": (sz, [C.POINTER(UpsampleConvDesc)]),
    "bd_upsample_conv_dgrad_workspace_bytes": (sz, [C.POINTER(UpsampleConvDesc)]),
    "bd_upsample_conv_wgrad_plan": (i32, [C.POINTER(UpsampleConvDesc), C.POINTER(ConvPsWgradPlanInfo)]),
    "bd_upsample_conv_dgrad_tap_groups": (i32, [C.POINTER(UpsampleConvDesc)]),
    "bd_conv3x3_s2_dgrad_ps": (i32, [C.POINTER(ConvS2DgradDesc), vp]),
    "bd_gemm_sp_workspace_bytes": (sz, [C.POINTER(GemmSpDesc)]),
    "bd_gemm_sp": (i32, [C.POINTER(GemmSpDesc), vp]),
    "bd_gemm_sp_plan": (i32, [C.POINTER(GemmSpDesc), C.POINTER(GemmSpPlanInfo)]),
    "bd_attn_sp_supported": (i32, [i32, i32]),
    "bd_attn_sp_fwd": (i32, [C.POINTER(AttnSpDesc), vp]),
    "bd_attn_sp_bwd": (i32, [C.POINTER(AttnSpDesc), vp]),
    "bd_conv3x3_ps_wgrad": (i32, [C.POINTER(ConvPsWgradDesc), vp]),
    "bd_conv3x3_ps_wgrad_workspace_bytes": (sz, [C.POINTER(ConvPsWgradDesc)]),
    "bd_conv3x3_ps_wgrad_plan": (i32, [C.POINTER(ConvPsWgradDesc), C.POINTER(ConvPsWgradPlanInfo)]),
    "bd_conv3x3_fwd": (i32, [C.POINTER(ConvFwdDesc), vp]),
    "bd_conv3x3_dgrad": (i32, [C.POINTER(ConvDgradDesc), vp]),
    "bd_conv3x3_wgrad": (i32, [C.POINTER(ConvWgradDesc), vp]),
    "bd_conv3x3_workspace_bytes": (sz, [i32] * 8),
    "bd_conv3x3_fwd_plan": (i32, [C.POINTER(ConvFwdDesc), C.POINTER(ThinPlanInfo)]),
    "bd_conv3x3_dgrad_plan": (i32, [C.POINTER(ConvDgradDesc), C.POINTER(ThinPlanInfo)]),
    "bd_conv3x3_wgrad_plan": (i32, [C.POINTER(ConvWgradDesc), C.POINTER(ThinPlanInfo)]),
    "bd_colsum": (i32, [vp, i64, i64, i32, i64, vp, i64, i32, vp]),
    "bd_sum2x2": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, i32, vp]),
    "bd_add": (i32, [vp, i64, vp, i64, i64, i32, f32, i32, vp]),
    "bd_softmax_fwd": (i32, [vp, vp, i64, i32, vp]),
    "bd_softmax_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "bd_silu_fwd": (i32, [vp, vp, i64, vp]),
    "bd_silu_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "bd_reduce_workspace_bytes": (sz, []),
    "bd_loss_fwd_bwd": (i32, [vp, i64, vp, i64, i64, i32, i32, f32, vp, vp, i64, vp, vp]),
    "bd_loss_groups_workspace_bytes": (sz, [i32]),
    "bd_loss_groups_fwd_bwd": (i32, [vp, i64, vp, i64, i64, i32, i32, f32, C.POINTER(LossGroupsDesc), vp, vp, i64, vp, sz, vp]),
    "bd_sumsq": (i32, [vp, i64, vp, vp, vp]),
    "bd_adam_clip": (i32, [vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, f64, i32, vp, vp]),
    "bd_prof_enable": (i32, [i32]),
    "bd_prof_enabled": (i32, []),
    "bd_prof_reset": (i32, []),
    "bd_prof_num_classes": (i32, []),
    "bd_prof_get": (i32, [i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f64)]),
    "bd_mfma_probe": (i32, [i32, i32, i32, C.POINTER(f64), vp]),
    "bd_axpy": (i32, [vp, vp, i64, f32, i32, vp]),
    "bd_adam_clip_dev": (i32, [vp, vp, vp, vp, i64, vp, f64, vp, f64, f64, f64, vp, vp]),
    "bd_adam_clip_ema": (i32, [vp, vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, f64, i32, f32, vp, vp]),
    "bd_adam_clip_ema_dev": (i32, [vp, vp, vp, vp, vp, i64, vp, f64, vp, f64, f64, f64, vp, vp]),
    "bd_ema_update": (i32, [vp, vp, i64, f32, vp]),
    "bd_unet_create": (i32, [C.POINTER(UnetConfig), C.POINTER(vp)]),
    "bd_unet_destroy": (None, [vp]),
    "bd_unet_set_compute_mode": (i32, [vp, i32]),
    "bd_unet_set_deferred_join": (i32, [vp, i32]),
    "bd_unet_stream_wait_aux": (i32, [vp, vp]),
    "bd_unet_num_params": (i64, [vp]),
    "bd_unet_num_tensors": (i32, [vp]),
    "bd_unet_param_info": (i32, [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32), i64 * 4, C.POINTER(i32)]),
    "bd_unet_workspace_bytes": (sz, [vp, i32, i32]),
    "bd_unet_forward": (i32, [vp, i32, i32, vp, vp, i64, vp, i32, vp, i64, vp, sz, vp]),
    "bd_unet_backward": (i32, [vp, i32, vp, vp, i64, vp, i64, vp, vp, sz, vp]),
    "bd_unet_backward_input": (i32, [vp, i32, vp, vp, i64, vp, i64, vp, vp, i64, vp, sz, vp]),
    "bd_unet_num_segments": (i32, [vp]),
    "bd_unet_set_aux_stream": (i32, [vp, i32]),
    "bd_unet_set_static_weights": (i32, [vp, i32]),
    "bd_unet_reset_static_cache": (i32, [vp]),
    "bd_tune_set": (i32, [C.c_char_p, i32]),
    "bd_unet_segment_range": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64)]),
    "bd_unet_segment_num_ranges": (i32, [vp, i32]),
    "bd_unet_segment_range_k": (i32, [vp, i32, i32, C.POINTER(i64), C.POINTER(i64)]),
    "bd_unet_backward_segment": (i32, [vp, i32, i32, vp, vp, i64, vp, i64, vp, vp, sz, vp, C.POINTER(i64), C.POINTER(i64)]),
}

_lib = None


def load():
    """Load libbd_hip.so (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m baddiffusion_amd.build` (hipcc, gfx950). "
            "There is no CPU / PyTorch fallback for the hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what=""):
    if status != 0:
        msg = load().bd_last_error()
        raise RuntimeError(f"libbd_hip {what} failed ({status}): {msg.decode() if msg else ''}")


def ptr(t):
    """data_ptr of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream():
    """hipStream_t of torch's current stream, as void*."""
    return torch.cuda.current_stream().cuda_stream
