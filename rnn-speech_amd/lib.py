"""ctypes binding of libamdspeech.so (the C ABI in include/amdspeech.h).

There is NO CPU fallback: if the shared library is missing or a call fails the
import / call raises.  The library is built in-tree by build.py (hipcc, gfx950).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMDSPEECH_LIB") or os.path.join(HERE, "libamdspeech.so")   # env: dev override only


class AmdSpeechError(RuntimeError):
    pass


class DataflowTimeout(AmdSpeechError):
    """amdspeech_lstm_status returned AMDSPEECH_ETIMEOUT: a whole-sequence launch gave up waiting.  The mini-batch's results are
    invalid; it can be repeated on the launch-per-diagonal kernels.  Any OTHER error of that call is a device fault."""


ETIMEOUT = -4                     # include/amdspeech.h
ECALLBACK = -100                  # ops.ctc_beam_search_fused: the status its trampoline returns when `step` raised


class LstmDesc(C.Structure):
    _fields_ = [("T", C.c_int), ("B", C.c_int), ("H", C.c_int), ("L", C.c_int),
                ("keep_in", C.c_float), ("keep_out", C.c_float), ("seed", C.c_uint64),
                ("precision", C.c_int), ("flags", C.c_int)]


class CtcHead(C.Structure):          # amdspeech_ctc_head (include/amdspeech.h): the CTC head fused into the whole-sequence LSTM kernels
    _fields_ = [("w_out", C.c_void_p), ("b_out", C.c_void_p), ("logits", C.c_void_p), ("dense_labels", C.c_void_p),
                ("loss", C.c_void_p), ("dlogits", C.c_void_p), ("ctc_ws", C.c_void_p), ("C", C.c_int), ("U", C.c_int)]


class LstmPlanInfo(C.Structure):     # amdspeech_lstm_plan_info (include/amdspeech.h): the kernel path of a descriptor, read-only
    _fields_ = [(n, C.c_int) for n in ("fwd_path", "bwd_path", "nmt", "kb", "mv", "wpx", "uw", "fwd_mt", "pair", "bf16p", "bf16p_reserved",
                                       "xw_parts", "nfw", "w_pieces", "dz0_inkernel", "flow2_q")]


class LstmBidirPlanInfo(C.Structure):     # amdspeech_lstm_bidir_plan_info (include/amdspeech.h): the recurrence launches of a layer-wise bidirectional call, read-only
    _fields_ = [(n, C.c_int) for n in ("path", "cus", "fwd_kpw", "fwd_waves", "fwd_groups", "fwd_wgs", "fwd_lds", "bwd_kpw", "bwd_waves",
                                       "bwd_groups", "bwd_wgs", "bwd_lds")]


class CtcPlanInfo(C.Structure):     # amdspeech_ctc_plan_info (include/amdspeech.h): the recursion kernel of a CTC shape, read-only
    _fields_ = [(n, C.c_int) for n in ("kernel", "threads", "rmax", "smax")]


class GemmPlanInfo(C.Structure):     # amdspeech_gemm_plan_info (include/amdspeech.h): the kernel and launch geometry of one product, read-only
    _fields_ = [(n, C.c_int) for n in ("family", "variant", "splits", "k_chunk", "atomic", "zero_fill", "grid", "tiles_m", "tiles_n", "map",
                                       "bm", "bn", "col_slices", "a_vec", "b_vec")]


class FrontendPlanInfo(C.Structure):     # amdspeech_frontend_plan_info (include/amdspeech.h): the kernels and launch geometry of a front-end call, read-only
    _fields_ = [(n, C.c_int) for n in ("frames_kernel", "maxq", "n_dft", "frame_len", "hop", "n_bins", "bin_tiles", "kp", "lds_bytes", "t_full",
                                       "tiles_per_utt", "n_items", "workgroups", "dct_kernel", "dct_col_tiles", "meta_by_copy")]


class FrameStackPlanInfo(C.Structure):     # amdspeech_frame_stack_plan_info (include/amdspeech.h): the launch geometry of a frame-stacking call, read-only
    _fields_ = [(n, C.c_int) for n in ("t_out", "d_out", "vec", "workgroups", "meta_by_copy")]


class SpecAugmentDesc(C.Structure):     # amdspeech_spec_augment_desc (include/amdspeech.h): the masking policy and the seed of one call
    _fields_ = [(n, C.c_int) for n in ("period", "freq_masks", "freq_width", "time_masks", "time_width", "time_permille")] + \
               [("seed", C.c_uint64)]


class SpecAugmentPlanInfo(C.Structure):     # amdspeech_spec_augment_plan_info (include/amdspeech.h): the launch geometry of a masking call, read-only
    _fields_ = [(n, C.c_int) for n in ("vec", "lanes", "items_per_workgroup", "workgroups", "reps")]


class FeatureNormDesc(C.Structure):     # amdspeech_feature_norm_desc (include/amdspeech.h): the mode and the variance handling of one call
    _fields_ = [("mode", C.c_int), ("norm_vars", C.c_int), ("var_floor", C.c_double)]


class FeatureNormPlanInfo(C.Structure):     # amdspeech_feature_norm_plan_info (include/amdspeech.h): the launch geometry of a normalisation call, read-only
    _fields_ = [(n, C.c_int) for n in ("vec", "split", "workgroups", "lds_bytes", "meta_by_copy", "workspace_bytes")]


class LookaheadPlanInfo(C.Structure):     # amdspeech_lookahead_plan_info (include/amdspeech.h): the launch geometry of the lookahead-convolution calls, read-only
    _fields_ = [(n, C.c_int) for n in ("vec", "unroll", "col_blocks", "t_chunk", "chunks", "workgroups", "lds_bytes", "dw_partials", "dw_terms",
                                       "reduce_slices", "reduce_terms", "reduce_workgroups")]


class Conv2dPlanInfo(C.Structure):     # amdspeech_conv2d_plan_info (include/amdspeech.h): the launch geometry of the front convolution's calls, read-only
    _fields_ = [(n, C.c_int) for n in ("t_out", "f_out", "k", "k_pad", "tile_t", "tile_f", "vec", "fwd_workgroups", "fwd_lds_bytes",
                                       "weights_resident", "k_chunk", "k_rows", "k_groups", "dw_partials", "bwd_workgroups", "bwd_lds_bytes",
                                       "dw_terms", "reduce_slices", "reduce_terms", "reduce_workgroups")]


class VadPlanInfo(C.Structure):     # amdspeech_vad_plan_info (include/amdspeech.h): the launch geometry of the voice-activity calls, read-only
    _fields_ = [(n, C.c_int) for n in ("load_vec", "frames_per_tile", "tiles_per_row", "workgroups", "threads", "f_max", "select_passes",
                                       "row_workgroups", "row_threads", "meta_by_copy")]


class ResampleRowsPlanInfo(C.Structure):     # amdspeech_resample_rows_plan_info (include/amdspeech.h): the launch geometry of a per-row resampling call, read-only
    _fields_ = [(n, C.c_int) for n in ("tile", "tiles_per_row", "workgroups", "span_max", "table_chunk", "lds_bytes", "any_copy", "meta_launches")]


class ReverbRowsPlanInfo(C.Structure):     # amdspeech_reverb_rows_plan_info (include/amdspeech.h): the launch geometry of a reverberation call, read-only
    _fields_ = [(n, C.c_int) for n in ("tile", "tiles_per_row", "workgroups", "taps", "span_max", "k_chunk", "k_chunks", "lds_bytes", "copy_rows",
                                       "meta_launches")]


class NoiseMixRowsPlanInfo(C.Structure):     # amdspeech_noise_mix_rows_plan_info (include/amdspeech.h): the launch geometry of a noise-mixing call, read-only
    _fields_ = [(n, C.c_int) for n in ("tile", "tiles_per_row", "workgroups", "lds_bytes", "copy_rows", "meta_launches")]


class XentPlanInfo(C.Structure):     # amdspeech_xent_plan_info (include/amdspeech.h): the row kernel and launch geometry of a cross-entropy call, read-only
    _fields_ = [(n, C.c_int) for n in ("kernel", "values_per_lane", "threads", "rows_per_workgroup", "grid", "c_min", "c_max", "loss_threads",
                                       "loss_grid")]


class LmStepPlanInfo(C.Structure):     # amdspeech_lm_step_plan_info (include/amdspeech.h): the instantiation and launch geometry of a language-model step, read-only
    _fields_ = [(n, C.c_int) for n in ("kernel", "row_tile", "threads", "launches", "n_min", "n_max", "col_tiles", "row_tiles", "lds_bytes",
                                       "out_row_tile", "out_row_tiles", "v_max")]


class BlankSkipPlanInfo(C.Structure):     # amdspeech_ctc_blank_skip_plan_info (include/amdspeech.h): the kernels and launch geometry of a blank-skipping call, read-only
    _fields_ = [(n, C.c_int) for n in ("kernel", "words_per_lane", "vec", "c_min", "c_max", "rows_threads", "rows_per_workgroup", "rows_grid",
                                       "t_chunk", "chunks", "scan_threads", "scan_grid", "gather_threads", "gather_grid", "launches",
                                       "workspace_bytes")]


class RnntPlanInfo(C.Structure):     # amdspeech_rnnt_plan_info (include/amdspeech.h): the instantiations and launch geometry of the transducer calls, read-only
    _fields_ = [(n, C.c_int) for n in ("threads", "col_tiles", "c_min", "c_max", "j_min", "j_max", "fwd_t_tile", "fwd_u_tile", "fwd_k_chunk",
                                       "fwd_t_tiles", "fwd_u_tiles", "fwd_grid", "fwd_lds_bytes", "rows_per_workgroup", "rows_grid",
                                       "rec_kernel", "rec_threads", "rec_states", "u_min", "u_max", "rec_grid", "rec_lds_bytes", "bwd_t_tile",
                                       "bwd_u_tile", "bwd_k_slice", "bwd_k_slices", "bwd_t_chunk", "bwd_t_chunks", "bwd_items", "bwd_grid",
                                       "bwd_lds_bytes", "dg_terms", "dw_terms", "reduce_dg_grid", "reduce_dw_grid", "launches_fwd",
                                       "launches_loss", "launches_bwd")]


# amdspeech_lm_step_fn (include/amdspeech.h): (user, n, parent, token, dest, logq) -> status, called on the thread that called the decoder
LM_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float))

GEMM_FAMILIES = ("skinny_n", "skinny_k", "skinny_tn", "tn_direct", "kc_direct", "lds", "bf3", "bf16p")      # AMDSPEECH_GEMM_* (include/amdspeech.h)
GEMM_MAP_LINEAR, GEMM_MAP_XCD, GEMM_MAP_XCD_BLOCKS, GEMM_MAP_KC_BAND = range(4)      # AMDSPEECH_GEMM_MAP_*
GEMM_GROUP_MAX = 10                                                                 # AMDSPEECH_GEMM_GROUP_MAX
CTC_KERNELS = ("wave", "shift", "pair", "edge")      # AMDSPEECH_CTC_KERNEL_* (include/amdspeech.h)
LSTM_PATHS = ("flow", "big1", "big", "hoist", "diag", "diag_bf3")      # AMDSPEECH_LSTM_PATH_* (include/amdspeech.h)
XENT_KERNELS = ("wave", "block")      # AMDSPEECH_XENT_KERNEL_* (include/amdspeech.h)
BLANK_SKIP_KERNELS = ("wave", "block")      # AMDSPEECH_BLANK_SKIP_KERNEL_* (include/amdspeech.h)
RNNT_REC_KERNELS = ("wave", "block1", "block4", "block10")      # AMDSPEECH_RNNT_REC_* (include/amdspeech.h)
LM_STEP_KERNELS = ("mfma16",)      # AMDSPEECH_LM_STEP_KERNEL_* (include/amdspeech.h)
FEATURE_NORM_MODES = ("none", "utterance", "global")      # AMDSPEECH_FEATURE_NORM_* (include/amdspeech.h)
LSTM_ARMED, LSTM_ARM_NEXT, LSTM_SAME_WS, LSTM_PER_DIAGONAL, LSTM_INJECT_TIMEOUT = 1, 2, 4, 8, 16      # amdspeech_lstm_desc.flags (include/amdspeech.h)


COMM_ID_BYTES = 128
WS_Z0, WS_ZTOP, WS_DZTOP, WS_DZ0, WS_HFINAL, WS_CFINAL, WS_GATES = range(7)
BIDIR_WS_Z0, BIDIR_WS_YTOP_FW, BIDIR_WS_YTOP_BW, BIDIR_WS_DYTOP_FW, BIDIR_WS_DYTOP_BW, BIDIR_WS_DZ0, BIDIR_WS_HFINAL, BIDIR_WS_CFINAL = range(8)

_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_L = C.c_long
_SZ = C.c_size_t

# name -> (restype, argtypes); must list EVERY symbol include/amdspeech.h declares.
PROTOTYPES = {
    "amdspeech_version": (_I, []),
    "amdspeech_last_error": (C.c_char_p, []),
    "amdspeech_device_cu_count": (_I, []),
    "amdspeech_linear_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I]),
    "amdspeech_linear_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I]),
    "amdspeech_gemm_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
    "amdspeech_gemm_bf16x3": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
    "amdspeech_gemm_bf16": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
    "amdspeech_gemm_plan": (_I, [_I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, C.POINTER(GemmPlanInfo)]),
    "amdspeech_gemm_f32_tn_group": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
    "amdspeech_colsum_accumulate": (_I, [_P, _P, _I, _I, _I, _P]),
    "amdspeech_gemm_bf16_packed_scratch_bytes": (_SZ, [_I, _I, _I, _I, _I, _I, _I]),
    "amdspeech_gemm_bf16_packed": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _SZ]),
    "amdspeech_gemm_bf16_packed_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, C.POINTER(GemmPlanInfo)]),
    "amdspeech_bf16_copy": (_I, [_P, _P, C.c_long, C.c_long, _I, _I, _P, C.c_long, _P, _P]),
    "amdspeech_bf16_transpose": (_I, [_P, _P, C.c_long, _I, _P, C.c_long]),
    "amdspeech_batchnorm_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F]),
    "amdspeech_batchnorm_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I]),
    "amdspeech_batchnorm_sum": (_I, [_P, _P, _P, _I, _P, _I, _I, _I]),
    "amdspeech_batchnorm_apply": (_I, [_P, _P, _P, _P, _I, _F, _P, _P, _P, _I, _I, _I]),
    "amdspeech_batchnorm_bwd_sums": (_I, [_P, _P, _P, _P, _I, _I, _I]),
    "amdspeech_batchnorm_bwd_apply": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _I, _I]),
    "amdspeech_lstm_workspace_bytes": (_SZ, [C.POINTER(LstmDesc)]),
    "amdspeech_lstm_ws_ptr": (_P, [C.POINTER(LstmDesc), _P, _I]),
    "amdspeech_lstm_fwd": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _L, _P, _L, _P, _P, _P]),
    "amdspeech_lstm_status": (_I, [C.POINTER(LstmDesc), _P]),
    "amdspeech_lstm_workspace_release": (_I, [_P, _P]),
    "amdspeech_lstm_beside_forward": (_I, [_P, _P]),
    "amdspeech_lstm_beside_tail": (_I, [_P, _P]),
    "amdspeech_lstm_bwd": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _L, _P, _P, _L, _P]),
    "amdspeech_lstm_ctc_fusable": (_I, [C.POINTER(LstmDesc), _I, _I]),
    "amdspeech_lstm_pair_fusable": (_I, [C.POINTER(LstmDesc)]),
    "amdspeech_lstm_fwd_pair": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _P, C.POINTER(LstmDesc), _P, _P, _P, _L, _L, _P, _P, _P]),
    "amdspeech_lstm_bwd_pair": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _P, _P, C.POINTER(LstmDesc), _P, _P, _P, _P, _L, _L, _P]),
    "amdspeech_lstm_fwd_ctc": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _L, _P, _L, _P, _P, _P, C.POINTER(CtcHead)]),
    "amdspeech_lstm_bwd_ctc": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _L, _P, _P, _L, _P, C.POINTER(CtcHead)]),
    "amdspeech_lstm_dropout_multipliers": (_I, [_P, C.POINTER(LstmDesc), _I, _I, _P]),
    "amdspeech_lstm_plan": (_I, [C.POINTER(LstmDesc), _I, _I, C.POINTER(LstmPlanInfo)]),
    "amdspeech_lstm_plan_xw_halves": (_I, [C.POINTER(LstmDesc), _I, _I]),
    "amdspeech_lstm_plan_xw_ksteps": (_I, [C.POINTER(LstmDesc), _I, _I]),
    "amdspeech_lstm_bidir_workspace_bytes": (_SZ, [C.POINTER(LstmDesc)]),
    "amdspeech_lstm_bidir_ws_ptr": (_P, [C.POINTER(LstmDesc), _P, _I]),
    "amdspeech_lstm_bidir_layer_stride": (_L, [C.POINTER(LstmDesc)]),
    "amdspeech_lstm_bidir_path": (_I, [C.POINTER(LstmDesc)]),
    "amdspeech_lstm_bidir_plan": (_I, [C.POINTER(LstmDesc), C.POINTER(LstmBidirPlanInfo)]),
    "amdspeech_lstm_bidir_fwd": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _P, _P, _P, _P]),
    "amdspeech_lstm_bidir_bwd": (_I, [_P, C.POINTER(LstmDesc), _P, _P, _P, _P, _P]),
    "amdspeech_lstm_bidir_status": (_I, [C.POINTER(LstmDesc), _P]),
    "amdspeech_lstm_bidir_dropout_multipliers": (_I, [_P, C.POINTER(LstmDesc), _I, _I, _I, _P]),
    "amdspeech_ctc_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "amdspeech_ctc_plan": (_I, [_I, _I, _I, _I, C.POINTER(CtcPlanInfo)]),
    "amdspeech_ctc_loss_fwd_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_ctc_loss_fwd_bwd_staged": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I]),
    "amdspeech_ctc_align_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "amdspeech_ctc_align_plan": (_I, [_I, _I, _I, _I, C.POINTER(CtcPlanInfo)]),
    "amdspeech_ctc_align": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "amdspeech_ctc_greedy_decode": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "amdspeech_merge_repeated": (_I, [_P, _P, _P, _I, _I, _I]),
    "amdspeech_edit_distance": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "amdspeech_ctc_beam_search_host": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_ctc_beam_search_host_mt": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I]),
    "amdspeech_ctc_beam_search_host_nbest": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I]),
    "amdspeech_edit_distance_host": (_I, [_P, _P, _I, _P, _P, _I, _I, _P]),
    "amdspeech_crc32c": (C.c_uint32, [_P, _SZ, C.c_uint32]),
    "amdspeech_resample_workspace_bytes": (_SZ, [C.c_int]),
    "amdspeech_resample_num_samples": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "amdspeech_resample": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "amdspeech_resample_rows_num_samples": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "amdspeech_resample_rows_workspace_bytes": (_SZ, [C.c_int]),
    "amdspeech_resample_rows": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "amdspeech_resample_rows_plan": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(ResampleRowsPlanInfo)]),
    "amdspeech_speed_perturb_draw": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.c_int]),
    "amdspeech_reverb_rows_workspace_bytes": (_SZ, [_I]),
    "amdspeech_reverb_rows": (_I, [_P, _P, C.POINTER(_I), _I, _I, _P, C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I), _P, _P]),
    "amdspeech_reverb_rows_plan": (_I, [C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I),
                                        C.POINTER(ReverbRowsPlanInfo)]),
    "amdspeech_row_sumsq_workspace_bytes": (_SZ, [_I]),
    "amdspeech_row_sumsq": (_I, [_P, _P, C.POINTER(_I), _I, _I, _P, _P]),
    "amdspeech_noise_mix_rows_workspace_bytes": (_SZ, [_I]),
    "amdspeech_noise_mix_rows": (_I, [_P, _P, C.POINTER(_I), _I, _I, _P, C.POINTER(_I), _P, _I, _I, _P, C.POINTER(_I), C.POINTER(_I),
                                      C.POINTER(_I), _P, _P]),
    "amdspeech_noise_mix_rows_plan": (_I, [C.POINTER(_I), _I, _I, C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I),
                                           C.POINTER(NoiseMixRowsPlanInfo)]),
    "amdspeech_augment_draw": (_I, [C.c_uint64, C.c_uint64, _I, _I, _I, _I, C.POINTER(_I), _I, _I, C.POINTER(_I)]),
    "amdspeech_audio_probe": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long)]),
    "amdspeech_audio_decode": (C.c_int, [C.c_char_p, _P, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int), C.c_int]),
    "amdspeech_optim_workspace_bytes": (_SZ, [_L]),
    "amdspeech_clip_adam": (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _P, _P]),
    "amdspeech_frontend_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "amdspeech_frontend_num_frames": (_I, [_I, _I, _I]),
    "amdspeech_frontend_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(FrontendPlanInfo)]),
    "amdspeech_frontend_mfcc": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_frontend_fbank": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_frame_stack_num_frames": (_I, [_I, _I]),
    "amdspeech_frame_stack": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "amdspeech_frame_stack_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(FrameStackPlanInfo)]),
    "amdspeech_spec_augment": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(SpecAugmentDesc)]),
    "amdspeech_spec_augment_spans": (_I, [C.POINTER(SpecAugmentDesc), _I, _I, C.POINTER(C.c_int)]),
    "amdspeech_spec_augment_plan": (_I, [_I, _I, _I, C.POINTER(SpecAugmentDesc), C.POINTER(SpecAugmentPlanInfo)]),
    "amdspeech_feature_norm_plan": (_I, [_I, _I, _I, _I, C.POINTER(FeatureNormPlanInfo)]),
    "amdspeech_feature_moments": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "amdspeech_feature_norm": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(FeatureNormDesc), _P, _P]),
    "amdspeech_lookahead_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "amdspeech_lookahead_bwd_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "amdspeech_lookahead_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_lookahead_plan": (_I, [_I, _I, _I, _I, C.POINTER(LookaheadPlanInfo)]),
    "amdspeech_conv2d_fwd": (_I, [_P, _P, _P, _P, _P] + [_I] * 9 + [_P, _P]),
    "amdspeech_conv2d_bwd_workspace_bytes": (_SZ, [_I] * 9),
    "amdspeech_conv2d_bwd": (_I, [_P, _P, _P, _P, _P] + [_I] * 9 + [_P, _P, _P]),
    "amdspeech_conv2d_plan": (_I, [_I] * 9 + [C.POINTER(Conv2dPlanInfo)]),
    "amdspeech_vad_num_frames": (_I, [_I, _I]),
    "amdspeech_vad_workspace_bytes": (_SZ, [_I, _I, _I]),
    "amdspeech_vad_plan": (_I, [_I, _I, _I, C.POINTER(VadPlanInfo)]),
    "amdspeech_vad_energy": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P]),
    "amdspeech_vad_flags": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _I, _I, _P, _P, _P]),
    "amdspeech_gather_spans": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _I, _P, _I]),
    "amdspeech_profile_enable": (_I, [_I]),
    "amdspeech_profile_get": (_I, [_I, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "amdspeech_profile_get_flops": (_I, [_I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "amdspeech_comm_available": (_I, []),
    "amdspeech_comm_unique_id": (_I, [_P]),
    "amdspeech_comm_init": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "amdspeech_comm_destroy": (_I, [_P]),
    "amdspeech_comm_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.c_char_p, _I]),
    "amdspeech_allreduce_sum_f32": (_I, [_P, _P, _P, _L]),
    "amdspeech_broadcast_f32": (_I, [_P, _P, _P, _L, _I]),
    "amdspeech_reverse_sequences": (_I, [_P, _P, _P, _P, _I, _I, _I, _I]),
    "amdspeech_axpy": (_I, [_P, _F, _P, _P, _L]),
    "amdspeech_fill": (_I, [_P, _P, _F, _L]),
    "amdspeech_embed_fwd": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_embed_bwd_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "amdspeech_embed_bwd": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "amdspeech_xent_workspace_bytes": (_SZ, [_I, _I, _I]),
    "amdspeech_xent_plan": (_I, [_I, _I, _I, C.POINTER(XentPlanInfo)]),
    "amdspeech_xent_fwd_bwd": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _F, _P, _P, _P, _P]),
    "amdspeech_lm_step": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P, _L, _P, _P, _P]),
    "amdspeech_lm_step_plan": (_I, [_I, _I, _I, _I, C.POINTER(LmStepPlanInfo)]),
    "amdspeech_lm_step_pool_bytes": (_SZ, [_I, _I, _I]),
    "amdspeech_ctc_beam_search_fused_slots": (_I, [_I, _I]),
    "amdspeech_ctc_beam_search_host_fused": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _F, _F, LM_STEP_FN, _P, _P, _P, _P, _P, _I]),
    "amdspeech_ctc_blank_skip_workspace_bytes": (_SZ, [_I, _I, _I]),
    "amdspeech_ctc_blank_skip_plan": (_I, [_I, _I, _I, C.POINTER(BlankSkipPlanInfo)]),
    "amdspeech_ctc_blank_skip": (_I, [_P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    "amdspeech_rnnt_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(RnntPlanInfo)]),
    "amdspeech_rnnt_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "amdspeech_rnnt_targets": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "amdspeech_rnnt_joint_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "amdspeech_rnnt_loss_fwd_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "amdspeech_rnnt_joint_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "amdspeech_rnnt_greedy_step": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "amdspeech_lm_step_state": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P, _L]),
}

_lib = None


def load():
    """Load the library (once).  Raises AmdSpeechError when it is absent --
    the product path never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmdSpeechError(
            "libamdspeech.so not found at %s -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().amdspeech_last_error().decode("utf-8", "replace")
        raise (DataflowTimeout if rc == ETIMEOUT else AmdSpeechError)("%s failed (%d): %s" % (what or "amdspeech call", rc, msg))
