"""ctypes binding of libnefnet_hip.so (declared in include/nefnet_hip.h).

There is no CPU fallback: if the shared library is missing or fails to load, importing any compute
entry point raises.  Build it with `python -m electrocardio_panorama_amd.csrc.build`.
"""
import ctypes as C
import os

import torch  # noqa: F401  (first: the library must bind to the HIP runtime PyTorch-ROCm has already loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnefnet_hip.so")

NEF_OK = 0
_ERR = {-1: "NEF_E_SHAPE", -2: "NEF_E_NULL", -3: "NEF_E_WORKSPACE", -4: "NEF_E_UNSUPPORTED"}

p = C.c_void_p
i32 = C.c_int
i64 = C.c_int64
f32 = C.c_float
sz = C.c_size_t


class ConvArgs(C.Structure):
    """Mirror of `nef_conv_args` (include/nefnet_hip.h)."""
    _fields_ = [
        ("x", p), ("wp", p), ("y", p), ("bias", p), ("in_scale", p), ("res", p), ("gate", p), ("mask", p),
        ("x_bs", i64), ("x_gs", i64), ("y_bs", i64), ("y_gs", i64), ("sc_bs", i64), ("sc_gs", i64),
        ("res_bs", i64), ("res_gs", i64), ("gate_bs", i64), ("gate_gs", i64),
        ("B", i32), ("T", i32), ("G", i32), ("Cin_g", i32), ("Cout_g", i32), ("K", i32),
        ("relu", i32), ("gate_scale", f32), ("drop_scale", f32), ("drop_p", f32), ("rng_seed", C.c_uint64),
        ("pro_a", p), ("pro_b", p), ("pro_mode", i32), ("pro_Bp", i32), ("rng_seed_dev", p), ("wino", i32),
        ("stats", p),
        ("bnb_x", p), ("bnb_mean", p), ("bnb_invstd", p), ("bnb_a", p), ("bnb_b", p), ("bnb_slots", p), ("bnb_Bp", i32),
        ("bnb_up", i32), ("x_scale", f32), ("reserved0", i32), ("x_amax", p), ("x_amax_next", p), ("x_clamped", p),
        ("res_scale", p), ("rs_bs", i64), ("rs_gs", i64), ("gate_rowscale", p), ("gr_bs", i64), ("gr_gs", i64),
        ("stats_mode", i32), ("reserved1", i32),
    ]


class BwwArgs(C.Structure):
    """Mirror of `nef_bww_args` (include/nefnet_hip.h)."""
    _fields_ = [
        ("x", p), ("gy", p), ("gw", p), ("ws", p), ("in_scale", p), ("pro_a", p), ("pro_b", p),
        ("x_amax", p), ("gy_amax", p), ("x_amax_next", p), ("gy_amax_next", p), ("clamped", p), ("ws_bytes", sz),
        ("x_bs", i64), ("x_gs", i64), ("gy_bs", i64), ("gy_gs", i64), ("sc_bs", i64), ("sc_gs", i64),
        ("B", i32), ("T", i32), ("G", i32), ("Cin_g", i32), ("Cout_g", i32), ("K", i32),
        ("pro_mode", i32), ("pro_Bp", i32), ("form", i32), ("x_scale", f32), ("gy_scale", f32), ("reserved0", i32),
    ]


class BnBwdArgs(C.Structure):
    """Mirror of `nef_bn_bwd_args` (include/nefnet_hip.h)."""
    _fields_ = [
        ("g", p), ("gout", p), ("out", p), ("wout", p), ("x", p), ("mean", p), ("invstd", p), ("a", p), ("b", p),
        ("gx", p), ("ggamma", p), ("gbeta", p), ("gx_chan_sum", p), ("slots", p), ("ws", p), ("ws_bytes", sz),
        ("P", i32), ("Bp", i32), ("C", i32), ("L", i32), ("nslot", i32), ("form", i32), ("phase_major", i32), ("reserved0", i32),
    ]


class UpdateArgs(C.Structure):
    """Mirror of `nef_update_args` (include/nefnet_hip.h)."""
    _fields_ = [
        ("p", p), ("g", p), ("buf", p), ("m", p), ("v", p), ("step", p), ("skip_if_positive", p), ("skipped", p), ("lr_dev", p),
        ("run_end", p), ("run_mul", p), ("n", i64), ("beta1", C.c_double), ("beta2", C.c_double),
        ("lr", f32), ("gscale", f32), ("mu", f32), ("eps", f32), ("weight_decay", f32),
        ("rule", i32), ("nesterov", i32), ("n_runs", i32),
    ]


class EmaArgs(C.Structure):
    """Mirror of `nef_ema_args` (include/nefnet_hip.h)."""
    _fields_ = [("ema", p), ("n_averaged", p), ("decay", C.c_double), ("warmup", i32), ("reserved0", i32)]


class TrustArgs(C.Structure):
    """Mirror of `nef_trust_args` (include/nefnet_hip.h)."""
    _fields_ = [("seg_end", p), ("seg_wd_mul", p), ("seg_adapt", p), ("ratio", p), ("stats", p), ("taint", p), ("ws", p),
                ("ws_bytes", sz), ("trust_coef", f32), ("trust_eps", f32), ("n_segs", i32), ("reserved0", i32)]


class LrSchedArgs(C.Structure):
    """Mirror of `nef_lr_sched_args` (include/nefnet_hip.h)."""
    _fields_ = [("t", p), ("base_dev", p), ("lr_out", p), ("skip_if_positive", p), ("flag", p), ("warmup_updates", i64),
                ("total_updates", i64), ("base", C.c_double), ("warmup_start", C.c_double), ("lr_floor", C.c_double),
                ("poly_power", C.c_double), ("shape", i32), ("advance", i32)]


class LossSsimArgs(C.Structure):
    """Mirror of `nef_loss_ssim_args` (include/nefnet_hip.h)."""
    _fields_ = [("pred", p), ("target", p), ("noise", p), ("rois", p), ("losses", p), ("ws", p), ("ws_bytes", sz), ("gscale", p),
                ("g_pred", p), ("B", i32), ("L", i32), ("factor", f32), ("reserved0", i32)]


class LossSegArgs(C.Structure):
    """Mirror of `nef_loss_seg_args` (include/nefnet_hip.h)."""
    _fields_ = [("pred", p), ("target", p), ("noise", p), ("rois", p), ("losses", p), ("g_pred", p), ("ws", p), ("ws_bytes", sz),
                ("B", i32), ("L", i32), ("reg_l2", i32), ("f2", f32), ("w", f32 * 7), ("reserved0", i32)]


class LossSlopeArgs(C.Structure):
    """Mirror of `nef_loss_slope_args` (include/nefnet_hip.h)."""
    _fields_ = [("pred", p), ("target", p), ("noise", p), ("rois", p), ("losses", p), ("ws", p), ("ws_bytes", sz), ("gscale", p),
                ("g_pred", p), ("B", i32), ("L", i32), ("factor", f32), ("l2", i32), ("slot", i32), ("reserved0", i32)]


class LossCorrArgs(C.Structure):
    """Mirror of `nef_loss_corr_args` (include/nefnet_hip.h)."""
    _fields_ = [("pred", p), ("target", p), ("noise", p), ("rois", p), ("losses", p), ("ws", p), ("ws_bytes", sz), ("gscale", p),
                ("g_pred", p), ("eps", C.c_double), ("B", i32), ("L", i32), ("factor", f32), ("slot", i32)]


class LocateScoreArgs(C.Structure):
    """Mirror of `nef_locate_score_args` (include/nefnet_hip.h)."""
    _fields_ = [("pred", p), ("obs", p), ("rois", p), ("scores", p), ("pred_bs", i64), ("pred_as", i64), ("obs_bs", i64), ("obs_rs", i64),
                ("sc_bs", i64), ("sc_rs", i64), ("col_off", i64), ("eps", C.c_double),
                ("B", i32), ("A", i32), ("R", i32), ("L", i32), ("mode", i32), ("group", i32)]


class LocateBestArgs(C.Structure):
    """Mirror of `nef_locate_best_args` (include/nefnet_hip.h)."""
    _fields_ = [("scores", p), ("cands", p), ("best_score", p), ("best_theta", p), ("best_index", p), ("sc_bs", i64), ("sc_rs", i64),
                ("index_base", i64), ("B", i32), ("R", i32), ("A", i32), ("per_pair", i32), ("init", i32), ("keep_index", i32)]


class LocateCandsArgs(C.Structure):
    """Mirror of `nef_locate_cands_args` (include/nefnet_hip.h)."""
    _fields_ = [("best_theta", p), ("best_index", p), ("cands", p), ("s1", f32), ("s2", f32), ("ph1", f32), ("ph2", f32),
                ("B", i32), ("R", i32), ("radius", i32), ("reserved0", i32)]


class AugmentArgs(C.Structure):
    """Mirror of `nef_augment_args` (include/nefnet_hip.h)."""
    _fields_ = [("x", p), ("rois", p), ("y", p), ("seed_dev", p), ("seed", C.c_uint64),
                ("wander_amp", C.c_double), ("wander_lo", C.c_double), ("wander_hi", C.c_double), ("hum_amp", C.c_double),
                ("hum_hz", C.c_double), ("sample_rate", C.c_double), ("noise_std", f32), ("lead_drop", f32),
                ("B", i32), ("V", i32), ("L", i32), ("R", i32), ("crop", i32), ("reserved0", i32)]


class LeadMaskMixFwdArgs(C.Structure):
    """Mirror of `nef_lead_mask_mix_fwd_args` (include/nefnet_hip.h)."""
    _fields_ = [("z1", p), ("z2r", p), ("mask", p), ("q", p), ("choice_dev", p), ("latent", p), ("D", p), ("picks", p),
                ("B", i32), ("V", i32), ("T", i32), ("c1", i32), ("c2", i32), ("reserved0", i32)]


class LeadMaskMixBwdArgs(C.Structure):
    """Mirror of `nef_lead_mask_mix_bwd_args` (include/nefnet_hip.h)."""
    _fields_ = [("gD", p), ("latent", p), ("z1", p), ("z2r", p), ("q", p), ("mask", p), ("choice_dev", p), ("gz1", p), ("gz2r", p),
                ("gq", p), ("B", i32), ("V", i32), ("T", i32), ("c1", i32), ("c2", i32), ("relu_z1", i32), ("up", i32), ("reserved0", i32)]


class AugmentMaskArgs(C.Structure):
    """Mirror of `nef_augment_mask_args` (include/nefnet_hip.h)."""
    _fields_ = [("mask", p), ("seed_dev", p), ("seed", C.c_uint64), ("lead_drop", f32), ("B", i32), ("V", i32), ("reserved0", i32)]


class NoiseRowArgs(C.Structure):
    """Mirror of `nef_noise_row_args` (include/nefnet_hip.h)."""
    _fields_ = [("target", p), ("rois", p), ("out", p), ("sigma", p), ("seed_dev", p), ("seed", C.c_uint64), ("Rw", i32), ("L", i32)]


class WarpArgs(C.Structure):
    """Mirror of `nef_warp_args` (include/nefnet_hip.h)."""
    _fields_ = [("data", p), ("target", p), ("rest", p), ("rois", p), ("data_out", p), ("target_out", p), ("rest_out", p),
                ("rois_out", p), ("seed", C.c_uint64), ("index0", i64), ("amp", C.c_double * 6),
                ("jitter", i32), ("B", i32), ("V", i32), ("R", i32), ("L", i32), ("reserved0", i32)]


class BeatBatchArgs(C.Structure):
    """Mirror of `nef_beat_batch_args` (include/nefnet_hip.h)."""
    _fields_ = [("signal", p), ("plan", p), ("data", p), ("target_view", p), ("rest_view", p), ("signal_elems", i64),
                ("B", i32), ("V", i32), ("R", i32), ("dtype", i32)]


class BeatRangeArgs(C.Structure):
    """Mirror of `nef_beat_range_args` (include/nefnet_hip.h)."""
    _fields_ = [("signal", p), ("plan", p), ("range", p), ("signal_elems", i64), ("B", i32), ("V", i32), ("R", i32), ("dtype", i32)]


class BeatStitchArgs(C.Structure):
    """Mirror of `nef_beat_stitch_args` (include/nefnet_hip.h)."""
    _fields_ = [("views", p), ("range", p), ("table", p), ("out", p), ("view_bs", i64), ("view_as", i64), ("out_elems", i64),
                ("Bt", i32), ("A", i32), ("fill", i32), ("reserved0", i32)]


class RecordingStatsArgs(C.Structure):
    """Mirror of `nef_recording_stats_args` (include/nefnet_hip.h)."""
    _fields_ = [("out", p), ("signal", p), ("beat_table", p), ("rec_table", p), ("out_offsets", p), ("score_leads", p), ("stats", p),
                ("out_elems", i64), ("signal_elems", i64), ("Bt", i32), ("N", i32), ("A", i32), ("fill", i32), ("dtype", i32),
                ("reserved0", i32)]


class MarkEnvelopeArgs(C.Structure):
    """Mirror of `nef_mark_envelope_args` (include/nefnet_hip.h)."""
    _fields_ = [("signal", p), ("table", p), ("env", p), ("signal_elems", i64), ("env_elems", i64), ("max_len", i64), ("N", i32), ("D", i32),
                ("H", i32), ("lead_bits", i32), ("dtype", i32), ("reserved0", i32)]


class MarkPeaksArgs(C.Structure):
    """Mirror of `nef_mark_peaks_args` (include/nefnet_hip.h)."""
    _fields_ = [("env", p), ("table", p), ("peaks", p), ("count", p), ("level", p), ("env_elems", i64), ("max_len", i64),
                ("frac", C.c_double), ("N", i32), ("seg", i32), ("r", i32), ("max_peaks", i32)]


class ResampleArgs(C.Structure):
    """Mirror of `nef_resample_args` (include/nefnet_hip.h)."""
    _fields_ = [("src", p), ("table", p), ("dst", p), ("taps", p), ("first", p), ("src_elems", i64), ("dst_elems", i64),
                ("max_out_len", i64), ("N", i32), ("max_rows", i32), ("up", i32), ("down", i32), ("K", i32), ("dtype", i32)]


class SlidingMedianArgs(C.Structure):
    """Mirror of `nef_sliding_median_args` (include/nefnet_hip.h)."""
    _fields_ = [("src", p), ("table", p), ("dst", p), ("minuend", p), ("src_elems", i64), ("dst_elems", i64), ("minuend_elems", i64),
                ("max_len", i64), ("N", i32), ("max_rows", i32), ("h", i32), ("dtype", i32), ("minuend_dtype", i32), ("reserved0", i32)]


class PackDesc(C.Structure):
    """Mirror of `nef_pack_desc` (include/nefnet_hip.h)."""
    _fields_ = [("w", p), ("wp", p), ("G", i32), ("Cog", i32), ("Cig", i32), ("K", i32), ("transpose_flip", i32),
                ("wino", i32), ("src_mode", i32), ("src_Cr", i32)]


# name -> (restype, argtypes); every symbol include/nefnet_hip.h declares
SIGNATURES = {
    "nef_abi_version": (i32, []),
    "nef_debug_spin_us": (i32, [f32, i32, p]),
    "nef_stem_fwd": (i32, [p, p, p, i32, i32, i32, p]),
    "nef_stem_bwd_ws_bytes": (sz, [i32]),
    "nef_stem_bwd_weight": (i32, [p, p, p, p, p, sz, i32, i32, i32, p]),
    "nef_stem_bwd_weight_live": (i32, [p, p, p, p, p, sz, i32, i32, i32, p, p]),
    "nef_pack_weights": (i32, [C.POINTER(PackDesc), i32, p]),
    "nef_pack_bytes": (sz, [C.POINTER(PackDesc)]),
    "nef_live_extent": (i32, [p, p, i32, i32, i32, p]),
    "nef_conv_fwd": (i32, [C.POINTER(ConvArgs), p]),
    "nef_conv_fwd_live": (i32, [C.POINTER(ConvArgs), p, i32, p]),
    "nef_conv_fwd_live_res": (i32, [C.POINTER(ConvArgs), p, i32, i32, p]),
    "nef_conv_args_bytes": (sz, []),
    "nef_conv_bwd_weight_ws_bytes": (sz, [C.POINTER(BwwArgs)]),
    "nef_conv_bwd_weight": (i32, [C.POINTER(BwwArgs), p]),
    "nef_conv_bwd_weight_live": (i32, [C.POINTER(BwwArgs), p, i32, p]),
    "nef_bww_args_bytes": (sz, []),
    "nef_h2_tail_census_ws_bytes": (sz, [i32, i32, i32]),
    "nef_h2_tail_census": (i32, [p, i64, i64, i32, i32, i32, i32, p, i64, i64, p, p, i32, i32, p, f32, f32, p, sz, p, p, p, p]),
    "nef_bwd_weight_clamp_ends": (i32, [p, p, i64, i64, p, i32, i32, i32, i32, i32, p]),
    "nef_chan_sum_ws_bytes": (sz, [i32]),
    "nef_chan_sum": (i32, [p, p, p, sz, i32, i32, i32, p]),
    "nef_convt2_fwd": (i32, [p, p, p, p, i32, i32, i32, i32, i32, p]),
    "nef_convt2_bwd_data": (i32, [p, p, p, i32, i32, i32, i32, i32, p]),
    "nef_group_transpose": (i32, [p, p, i32, i32, i32, p]),
    "nef_convt2_interleave": (i32, [p, p, p, i32, i32, i32, p]),
    "nef_convt2_deinterleave": (i32, [p, p, i32, i32, i32, p]),
    "nef_convt2_bwd_weight_ws_bytes": (sz, [i32, i32, i32]),
    "nef_convt2_bwd_weight": (i32, [p, p, p, p, p, sz, i32, i32, i32, i32, i32, p]),
    "nef_theta_mlp_fwd": (i32, [p, p, p, p, i32, i32, p]),
    "nef_theta_mlp_bwd": (i32, [p, p, p, p, i32, i32, p]),
    "nef_theta_encode": (i32, [p, p, i32, p]),
    "nef_chscale_fwd": (i32, [p, p, i64, p, i32, i32, i32, p]),
    "nef_chscale_bwd": (i32, [p, p, p, i64, p, p, i32, i32, i32, i32, p]),
    "nef_gate": (i32, [p, p, p, f32, i64, p]),
    "nef_add": (i32, [p, p, p, i64, p]),
    "nef_roi_align_fwd": (i32, [p, p, p, i32, i32, i32, i32, i32, p]),
    "nef_roi_align_bwd": (i32, [p, p, p, i32, i32, i32, i32, i32, p]),
    "nef_window_crop": (i32, [p, i64, i64, p, i32, i32, i32, i32, i32, i32, p]),
    "nef_window_scatter": (i32, [p, p, i64, i64, i32, i32, i32, i32, i32, i32, p]),
    "nef_roi_unpool_fwd": (i32, [p, p, p, p, i32, i32, i32, p]),
    "nef_roi_unpool_bwd": (i32, [p, p, p, i32, i32, i32, p]),
    "nef_roi_segment_table": (i32, [p, p, p, i32, p]),
    "nef_lead_mean": (i32, [p, p, p, i32, i32, i32, p]),
    "nef_mix_fwd": (i32, [p, p, p, p, p, i32, i32, i32, i32, i32, p, p]),
    "nef_mix_bwd": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, i32, i32, p, i32, i32, i32, p]),
    "nef_mix_fwd_shared": (i32, [p, p, p, p, p, i32, i32, i32, i32, i32, p, p]),
    "nef_lead_mean_mix_shared": (i32, [p, p, p, p, p, i32, i32, i32, i32, i32, p, p]),
    "nef_lead_mean_mix_unpool": (i32, [p, p, p, p, p, p, p, i32, i32, i32, i32, i32, p, p]),
    "nef_mix_bwd_unpool": (i32, [p, p, p, p, p, p, p, p, p, i32, i32, i32, i32, i32, p, i32, p]),
    "nef_mix_bwd_unpool_rs": (i32, [p, p, p, p, p, p, p, p, p, p, p, sz, p, i32, i32, i32, i32, i32, p, i32, p]),
    "nef_mix_bwd_unpool_rs_ws_bytes": (sz, [i32, i32]),
    "nef_pass_combine_fwd": (i32, [p, p, p, i32, i32, i32, p]),
    "nef_pass_combine_bwd": (i32, [p, p, i32, i32, i32, p]),
    "nef_pass_combine_stats_ws_bytes": (sz, [i32, i32]),
    "nef_pass_combine_fwd_stats": (i32, [p, p, p, p, p, p, p, p, p, p, p, p, sz, i32, i32, i32, f32, f32, p, p]),
    "nef_upsample2_fwd": (i32, [p, p, i64, i32, p]),
    "nef_upsample2_bwd": (i32, [p, p, i64, i32, p]),
    "nef_bn_ws_bytes": (sz, [i32, i32]),
    "nef_bn_train_stats": (i32, [p, p, p, p, p, p, p, p, p, p, sz, i32, i32, i32, i32, f32, f32, p, p]),
    "nef_conv_stats_slots": (i32, [i32, i32]),
    "nef_bn_stats_from_slots": (i32, [p, i32, p, p, p, p, p, p, p, p, p, sz, i32, i32, i32, i32, f32, f32, p, p]),
    "nef_bn_eval_affine": (i32, [p, p, p, p, p, p, i32, f32, p]),
    "nef_fold_bn": (i32, [p, p, p, p, p, p, i32, i32, p]),
    "nef_affine_relu_fwd": (i32, [p, p, p, p, i32, i32, i32, i32, p]),
    "nef_bn_bwd_ws_bytes": (sz, [C.POINTER(BnBwdArgs)]),
    "nef_bn_relu_bwd": (i32, [C.POINTER(BnBwdArgs), p]),
    "nef_bn_bwd_args_bytes": (sz, []),
    "nef_bn_relu_bwd_outconv_w": (i32, [C.POINTER(BnBwdArgs), p, p, p, sz, p]),
    "nef_bn_relu_bwd_outconv_w_ws_bytes": (sz, [C.POINTER(BnBwdArgs)]),
    "nef_outconv_fwd": (i32, [p, p, p, i32, p, p, p, i32, i32, i32, p]),
    "nef_outconv_bwd_weight": (i32, [p, p, p, p, p, i32, p, p, p, sz, i32, i32, i32, p]),
    "nef_outconv_bwd_data": (i32, [p, p, p, p, i32, i32, i32, p]),
    "nef_outconv_bwd_weight_ws_bytes": (sz, [i32]),
    "nef_loss_ws_bytes": (sz, []),
    "nef_loss_fwd": (i32, [p, p, p, p, p, p, sz, i64, f32, f32, f32, i32, i32, p]),
    "nef_loss_bwd": (i32, [p, p, p, p, p, p, p, p, i64, f32, f32, f32, i32, i32, p]),
    "nef_loss_noise_fwd": (i32, [p, p, p, p, p, p, p, sz, i64, f32, f32, f32, i32, i32, p]),
    "nef_loss_noise_bwd": (i32, [p, p, p, p, p, p, p, p, p, i64, f32, f32, f32, i32, i32, p]),
    "nef_loss_ssim_fwd": (i32, [C.POINTER(LossSsimArgs), p]),
    "nef_loss_ssim_bwd": (i32, [C.POINTER(LossSsimArgs), p]),
    "nef_loss_ssim_ws_bytes": (sz, [i32, i32]),
    "nef_loss_ssim_args_bytes": (sz, []),
    "nef_loss_seg_fwd": (i32, [C.POINTER(LossSegArgs), p]),
    "nef_loss_seg_bwd": (i32, [C.POINTER(LossSegArgs), p]),
    "nef_loss_seg_ws_bytes": (sz, [i32, i32]),
    "nef_loss_seg_args_bytes": (sz, []),
    "nef_loss_slope_fwd": (i32, [C.POINTER(LossSlopeArgs), p]),
    "nef_loss_slope_bwd": (i32, [C.POINTER(LossSlopeArgs), p]),
    "nef_loss_slope_ws_bytes": (sz, [i32, i32]),
    "nef_loss_slope_args_bytes": (sz, []),
    "nef_loss_corr_fwd": (i32, [C.POINTER(LossCorrArgs), p]),
    "nef_loss_corr_bwd": (i32, [C.POINTER(LossCorrArgs), p]),
    "nef_loss_corr_ws_bytes": (sz, [i32, i32]),
    "nef_loss_corr_args_bytes": (sz, []),
    "nef_locate_score": (i32, [C.POINTER(LocateScoreArgs), p]),
    "nef_locate_score_args_bytes": (sz, []),
    "nef_locate_best": (i32, [C.POINTER(LocateBestArgs), p]),
    "nef_locate_best_args_bytes": (sz, []),
    "nef_locate_cands": (i32, [C.POINTER(LocateCandsArgs), p]),
    "nef_locate_cands_args_bytes": (sz, []),
    "nef_augment": (i32, [C.POINTER(AugmentArgs), p]),
    "nef_augment_args_bytes": (sz, []),
    "nef_lead_mask_mix_fwd": (i32, [C.POINTER(LeadMaskMixFwdArgs), p]),
    "nef_lead_mask_mix_fwd_args_bytes": (sz, []),
    "nef_lead_mask_mix_bwd": (i32, [C.POINTER(LeadMaskMixBwdArgs), p]),
    "nef_lead_mask_mix_bwd_args_bytes": (sz, []),
    "nef_augment_mask": (i32, [C.POINTER(AugmentMaskArgs), p]),
    "nef_augment_mask_args_bytes": (sz, []),
    "nef_noise_row": (i32, [C.POINTER(NoiseRowArgs), p]),
    "nef_noise_row_args_bytes": (sz, []),
    "nef_warp": (i32, [C.POINTER(WarpArgs), p]),
    "nef_warp_args_bytes": (sz, []),
    "nef_beat_batch": (i32, [C.POINTER(BeatBatchArgs), p]),
    "nef_beat_batch_args_bytes": (sz, []),
    "nef_beat_range": (i32, [C.POINTER(BeatRangeArgs), p]),
    "nef_beat_range_args_bytes": (sz, []),
    "nef_beat_stitch": (i32, [C.POINTER(BeatStitchArgs), p]),
    "nef_beat_stitch_args_bytes": (sz, []),
    "nef_recording_stats": (i32, [C.POINTER(RecordingStatsArgs), p]),
    "nef_recording_stats_args_bytes": (sz, []),
    "nef_mark_envelope": (i32, [C.POINTER(MarkEnvelopeArgs), p]),
    "nef_mark_envelope_args_bytes": (sz, []),
    "nef_mark_peaks": (i32, [C.POINTER(MarkPeaksArgs), p]),
    "nef_mark_peaks_args_bytes": (sz, []),
    "nef_resample": (i32, [C.POINTER(ResampleArgs), p]),
    "nef_resample_args_bytes": (sz, []),
    "nef_sliding_median": (i32, [C.POINTER(SlidingMedianArgs), p]),
    "nef_sliding_median_args_bytes": (sz, []),
    "nef_sgd_momentum": (i32, [p, p, p, i64, f32, f32, f32, i32, p, p, p, p]),
    "nef_adam": (i32, [p, p, p, p, i64, f32, C.c_double, C.c_double, f32, f32, f32, p, p, p, p, p]),
    "nef_update": (i32, [C.POINTER(UpdateArgs), p]),
    "nef_update_args_bytes": (sz, []),
    "nef_update_ema": (i32, [C.POINTER(UpdateArgs), C.POINTER(EmaArgs), p]),
    "nef_ema_args_bytes": (sz, []),
    "nef_update_trust": (i32, [C.POINTER(UpdateArgs), C.POINTER(TrustArgs), C.POINTER(EmaArgs), p]),
    "nef_update_trust_ws_bytes": (sz, [i64, i32]),
    "nef_trust_args_bytes": (sz, []),
    "nef_lr_sched": (i32, [C.POINTER(LrSchedArgs), p]),
    "nef_lr_sched_args_bytes": (sz, []),
    "nef_grad_clip_ws_bytes": (sz, []),
    "nef_grad_clip": (i32, [p, i64, f32, f32, p, p, p, sz, p]),
    "nef_h2_taint": (i32, [p, p, p, p]),
    "nef_amax_roll": (i32, [p, p, i32, f32, f32, i32, p]),
    "nef_step_words": (i32, [p, p, i32, i32, i64, p]),
    "nef_flatten": (i32, [C.POINTER(p), C.POINTER(i64), i32, p, p]),
    "nef_flatten_acc": (i32, [C.POINTER(p), C.POINTER(i64), i32, p, i32, p, p]),
    "nef_copy_many": (i32, [C.POINTER(p), C.POINTER(p), C.POINTER(i64), i32, i32, p]),
    "nef_regroup_halves": (i32, [p, p, i32, i32, i32, i32, p]),
    "nef_slots_to_rows": (i32, [p, i32, p, i32, i32, p]),
    "nef_poly_weights": (i32, [p, p, i32, i32, i32, p]),
    "nef_poly_fwd_edge": (i32, [p, p, p, i32, i32, i32, i32, i32, p, p, i32, p, i32, p, p]),
    "nef_poly_wgrad_fold_ws_bytes": (sz, [i32, i32, i32, i32]),
    "nef_poly_wgrad_fold": (i32, [p, p, p, p, p, sz, i32, i32, i32, i32, i32, p]),
    "nef_poly_bwd_edge": (i32, [p, p, p, i32, i32, i32, i32, i32, p, p, p, p, p, i32, p, i32, i32, p]),
    "nef_view_metrics": (i32, [p, p, p, p, p, i32, i32, i32, p]),
    "nef_view_seg_metrics": (i32, [p, p, p, p, p, i32, i32, i32, p]),
    "nef_view_slope_metrics": (i32, [p, p, p, p, p, i32, i32, i32, p]),
    "nef_view_corr_metrics": (i32, [p, p, p, p, p, i32, i32, i32, p]),
    "nef_pano_h_from_f32": (i32, [p, p, i32, i32, i32, p]),
    "nef_pano_h_pack_weight": (i32, [p, p, i32, i32, p]),
    "nef_pano_h_conv": (i32, [p, p, p, p, p, i32, i32, i32, i32, i32, i32, i32, i64, i64, p]),
    "nef_pano_h_conv_pair": (i32, [p, p, p, p, p, p, p, i32, i32, i32, i32, i64, i64, p]),
    "nef_pano_h_conv_outconv": (i32, [p, p, p, p, p, p, i32, i32, i32, i64, i64, p]),
    "nef_pano_h_conv_tail": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, i64, i64, p]),
    "nef_pano_h_outconv": (i32, [p, p, p, p, i32, i32, i32, i64, i64, p]),
}

_lib = None


class NefLibraryError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle with typed entry points."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NefLibraryError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m electrocardio_panorama_amd.csrc.build`.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:         # a stale .so whose ABI number did not move (additions keep it): the missing symbol tells
            raise NefLibraryError(f"{LIB_PATH} does not export {name}: it is older than this binding; rebuild with "
                                  "`python -m electrocardio_panorama_amd.csrc.build`") from None
        fn.restype = res
        fn.argtypes = args
    # a stale .so next to a newer binding (or the reverse)
    for name, size, mirror in (("nef_conv_args", lib.nef_conv_args_bytes(), ConvArgs),
                               ("nef_bww_args", lib.nef_bww_args_bytes(), BwwArgs),
                               ("nef_bn_bwd_args", lib.nef_bn_bwd_args_bytes(), BnBwdArgs),
                               ("nef_update_args", lib.nef_update_args_bytes(), UpdateArgs),
                               ("nef_ema_args", lib.nef_ema_args_bytes(), EmaArgs),
                               ("nef_trust_args", lib.nef_trust_args_bytes(), TrustArgs),
                               ("nef_lr_sched_args", lib.nef_lr_sched_args_bytes(), LrSchedArgs),
                               ("nef_loss_ssim_args", lib.nef_loss_ssim_args_bytes(), LossSsimArgs),
                               ("nef_loss_seg_args", lib.nef_loss_seg_args_bytes(), LossSegArgs),
                               ("nef_loss_slope_args", lib.nef_loss_slope_args_bytes(), LossSlopeArgs),
                               ("nef_loss_corr_args", lib.nef_loss_corr_args_bytes(), LossCorrArgs),
                               ("nef_locate_score_args", lib.nef_locate_score_args_bytes(), LocateScoreArgs),
                               ("nef_locate_best_args", lib.nef_locate_best_args_bytes(), LocateBestArgs),
                               ("nef_locate_cands_args", lib.nef_locate_cands_args_bytes(), LocateCandsArgs),
                               ("nef_augment_args", lib.nef_augment_args_bytes(), AugmentArgs),
                               ("nef_lead_mask_mix_fwd_args", lib.nef_lead_mask_mix_fwd_args_bytes(), LeadMaskMixFwdArgs),
                               ("nef_lead_mask_mix_bwd_args", lib.nef_lead_mask_mix_bwd_args_bytes(), LeadMaskMixBwdArgs),
                               ("nef_augment_mask_args", lib.nef_augment_mask_args_bytes(), AugmentMaskArgs),
                               ("nef_noise_row_args", lib.nef_noise_row_args_bytes(), NoiseRowArgs),
                               ("nef_warp_args", lib.nef_warp_args_bytes(), WarpArgs),
                               ("nef_beat_batch_args", lib.nef_beat_batch_args_bytes(), BeatBatchArgs),
                               ("nef_beat_range_args", lib.nef_beat_range_args_bytes(), BeatRangeArgs),
                               ("nef_beat_stitch_args", lib.nef_beat_stitch_args_bytes(), BeatStitchArgs),
                               ("nef_recording_stats_args", lib.nef_recording_stats_args_bytes(), RecordingStatsArgs),
                               ("nef_mark_envelope_args", lib.nef_mark_envelope_args_bytes(), MarkEnvelopeArgs),
                               ("nef_mark_peaks_args", lib.nef_mark_peaks_args_bytes(), MarkPeaksArgs),
                               ("nef_resample_args", lib.nef_resample_args_bytes(), ResampleArgs),
                               ("nef_sliding_median_args", lib.nef_sliding_median_args_bytes(), SlidingMedianArgs)):
        if size != C.sizeof(mirror):
            raise NefLibraryError(f"{LIB_PATH}: {name} is {size} bytes, the binding mirrors {C.sizeof(mirror)}; rebuild with "
                                  "`python -m electrocardio_panorama_amd.csrc.build`")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc == NEF_OK:
        return
    if rc < 0:
        raise NefLibraryError(f"{what}: {_ERR.get(rc, rc)}")
    raise NefLibraryError(f"{what}: hipError_t {rc}")
