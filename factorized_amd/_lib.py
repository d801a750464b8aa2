"""ctypes binding of libmfm_hip.so (the C ABI declared in include/mfm_hip.h).

The HIP library is the product: there is NO CPU fallback.  Importing this module
without the built library raises immediately with the build instruction.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MFM_LIB_PATH: another build of the same library -- instrumented debug builds, scripts/seq_step_timeline.py)
LIB_PATH = os.environ.get("MFM_LIB_PATH") or os.path.join(_HERE, "libmfm_hip.so")

MFM_KLEF_NPARAM = 78
MFM_LOSS_SLOTS = 8
MFM_MAX_SEQ = 6
ABI_VERSION = 5
MFM_ERR_UNSUPPORTED = -3
# slots of mfm_plan_latent_form's out[16] (include/mfm_hip.h): the kernel form the latent stack takes at the plan's sizes --
# row or staged kernels, floats of the LDS weight panel (0: weights read from L2), rows per workgroup of the staged backward /
# forward, MFMA or quad products, workgroups per row of the row kernels, tabulated or searched bias gradients, stages, whether
# the early-fusion fc1 has a stage of its own, floats per row record, largest K / N of a layer, work items of the widest stage
# forward / backward, biases of all layers together
LATENT_FORM_SLOTS = ("row_path", "wpanel", "rows_per_wg", "rows_fwd", "mfma", "nch", "bias_tab", "nstages", "split0",
                     "rec_size", "max_k", "max_n", "items_fwd", "items_bwd", "n_bias")
# slots of mfm_plan_seq_form's out[4]: 1 = step-by-step path (0: weight-resident recurrence kernels), the widest resident h,
# 1 = a resident fp32 recurrence on the MFMA kernels (0: the VALU kernels, or one of the other two families)
SEQ_FORM_SLOTS = ("stepwise", "max_resident_h", "mfma")


class MfmError(RuntimeError):
    pass


class MfmUnsupported(MfmError):
    """an entry answered MFM_ERR_UNSUPPORTED (sizes its kernels do not cover) and enqueued nothing: the caller takes another path"""


class GemmDesc(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("c2", C.c_void_p),
                ("bias", C.c_void_p), ("bias2", C.c_void_p),
                ("a_sz", C.c_int64), ("a_sm", C.c_int64), ("a_sk", C.c_int64),
                ("b_sz", C.c_int64), ("b_sk", C.c_int64), ("b_sn", C.c_int64),
                ("c_sz", C.c_int64), ("ldc", C.c_int64), ("bias_sz", C.c_int64),
                ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("n_valid", C.c_int32),
                ("batch", C.c_int32), ("split_k", C.c_int32), ("accumulate", C.c_int32),
                ("alpha", C.c_float), ("a_bf16", C.c_int32), ("c_bf16", C.c_int32), ("reserved_", C.c_int32 * 2)]


class SeqDesc(C.Structure):
    _fields_ = [("gates", C.c_void_p), ("hs", C.c_void_p), ("cs", C.c_void_p),
                ("w_hh", C.c_void_p), ("w_ih", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p),
                ("h_init", C.c_void_p), ("ld_init", C.c_int64),
                ("dh_ext", C.c_void_p), ("ld_dh", C.c_int64),
                ("d_h_init", C.c_void_p), ("ld_dinit", C.c_int64),
                ("h", C.c_int32), ("is_dec", C.c_int32), ("dc_ext", C.c_void_p), ("w_pack", C.c_void_p),
                ("store_bf16", C.c_int32), ("bf16_dot", C.c_int32), ("h_last", C.c_void_p)]


class MemDesc(C.Structure):
    _fields_ = [("a1", C.c_void_p), ("a2", C.c_void_p), ("chat", C.c_void_p),
                ("w1m", C.c_void_p), ("w2m", C.c_void_p), ("w1b", C.c_void_p), ("b1b", C.c_void_p),
                ("w2b", C.c_void_p), ("b2b", C.c_void_p),
                ("gam1", C.c_void_p), ("gam2", C.c_void_p), ("mems", C.c_void_p), ("mem_out", C.c_void_p),
                ("dmem_out", C.c_void_p), ("du1", C.c_void_p), ("du2", C.c_void_p), ("dchat", C.c_void_p),
                ("T", C.c_int32), ("B", C.c_int32), ("M", C.c_int32), ("H1", C.c_int32), ("H2", C.c_int32),
                ("train", C.c_int32), ("p1", C.c_float), ("p2", C.c_float), ("seed", C.c_uint64),
                ("seed_dev", C.c_void_p), ("ld_wm", C.c_int64), ("dchat_pre_tanh", C.c_int32), ("reserved_", C.c_int32)]


class AdamSpan(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("step", C.c_int32), ("reserved", C.c_int32)]


MFM_ADAM_MAX_SPANS = 8


class SgdSpan(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("lr", C.c_float), ("weight_decay", C.c_float),
                ("momentum", C.c_float), ("dampening", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


MFM_SGD_MAX_SPANS = 112
MFM_SGD_NESTEROV, MFM_SGD_MAXIMIZE, MFM_SGD_FIRST = 1, 2, 4


class AdamExtSpan(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("step", C.c_int32), ("flags", C.c_int32), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("reserved", C.c_int32)]


MFM_ADAMX_MAX_SPANS = 88
MFM_ADAMX_MAXIMIZE, MFM_ADAMX_AMSGRAD, MFM_ADAMX_DECOUPLED = 1, 2, 4


class ClipSpan(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64)]


class DecFc1Item(C.Structure):
    _fields_ = [("hs", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("x", C.c_void_p),
                ("xhat", C.c_void_p), ("dxhat", C.c_void_p), ("dhs", C.c_void_p), ("loss", C.c_void_p),
                ("ldx", C.c_int64), ("d", C.c_int32), ("h", C.c_int32), ("Hp", C.c_int32),
                ("inv_count", C.c_float), ("grad_scale", C.c_float), ("pad_", C.c_int32)]


MFM_CLIP_MAX_SPANS = 112
MFM_NORM_L2, MFM_NORM_INF, MFM_NORM_L1 = 0, 1, 2
MFM_AVG_SWA, MFM_AVG_EMA = 0, 1
MFM_KEEP_MIN, MFM_KEEP_MAX = 0, 1
# MfmKeepBestState as int32 words: best_value (a float), calls, best_call, taken, ticket, 3 reserved
MFM_KEEP_STATE_WORDS = 8
MFM_PLATEAU_MAX_GROUPS = 16
MFM_PLATEAU_MIN, MFM_PLATEAU_MAX = 0, 1
MFM_PLATEAU_REL, MFM_PLATEAU_ABS = 0, 1
# MfmPlateauState as int32 words: best (a double: words 0-1), num_bad_epochs, cooldown_counter, last_epoch, reduced, reductions,
# 1 reserved
MFM_PLATEAU_STATE_WORDS = 8


class PlateauGroups(C.Structure):
    _fields_ = [("lr", C.c_void_p * MFM_PLATEAU_MAX_GROUPS), ("min_lr", C.c_double * MFM_PLATEAU_MAX_GROUPS)]


class LossWeights(C.Structure):
    _fields_ = [("disc", C.c_float), ("gen_l", C.c_float), ("gen_a", C.c_float), ("gen_v", C.c_float), ("reg", C.c_float),
                ("write_disc_loss", C.c_int32)]


class PlanConfig(C.Structure):
    _fields_ = [("d_l", C.c_int32), ("d_a", C.c_int32), ("d_v", C.c_int32),
                ("zl", C.c_int32), ("za", C.c_int32), ("zv", C.c_int32), ("zy", C.c_int32),
                ("fl", C.c_int32), ("fa", C.c_int32), ("fv", C.c_int32), ("fy", C.c_int32),
                ("output_dim", C.c_int32), ("loss_kind", C.c_int32),
                ("T", C.c_int32), ("B", C.c_int32),
                ("lda_xl", C.c_float), ("lda_xa", C.c_float), ("lda_xv", C.c_float), ("lda_reg", C.c_float),
                ("drop_zy", C.c_float), ("drop_zl", C.c_float), ("drop_za", C.c_float),
                ("drop_zv", C.c_float), ("drop_y", C.c_float),
                ("reg_scale", C.c_float), ("precision", C.c_int32),
                ("variant", C.c_int32), ("hl", C.c_int32), ("ha", C.c_int32), ("hv", C.c_int32), ("mem_dim", C.c_int32),
                ("nn1", C.c_int32), ("nn2", C.c_int32), ("g1", C.c_int32), ("g2", C.c_int32),
                ("drop_nn1", C.c_float), ("drop_nn2", C.c_float), ("drop_g1", C.c_float), ("drop_g2", C.c_float)]


_SIGS = {
    "mfm_abi_version": (C.c_int, []),
    "mfm_last_error": (C.c_char_p, []),
    "mfm_device_cus": (C.c_int, []),
    "mfm_gemm_grouped_f32": (C.c_int, [C.POINTER(GemmDesc), C.c_int, C.c_void_p]),
    "mfm_gemm_grouped_bf16": (C.c_int, [C.POINTER(GemmDesc), C.c_int, C.c_void_p]),
    "mfm_lstm_pack_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "mfm_lstm_pack_bf16": (C.c_int, [C.POINTER(SeqDesc), C.c_int, C.c_void_p]),
    "mfm_lstm_seq_fwd_bf16": (C.c_int, [C.POINTER(SeqDesc), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mfm_lstm_seq_bwd_bf16": (C.c_int, [C.POINTER(SeqDesc), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mfm_lstm_seq_fwd": (C.c_int, [C.POINTER(SeqDesc), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mfm_lstm_seq_bwd": (C.c_int, [C.POINTER(SeqDesc), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mfm_dw_bf16_lstm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_dw_f32_lstm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_mmd_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_mfn_mem_fwd": (C.c_int, [C.POINTER(MemDesc), C.c_void_p]),
    "mfm_mfn_mem_bwd": (C.c_int, [C.POINTER(MemDesc), C.c_void_p]),
    "mfm_mse_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float,
                                  C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_adam_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "mfm_adam_flat_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamSpan), C.c_int32,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "mfm_adam_flat_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                        C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "mfm_adam_flat_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "mfm_adam_flat_spans_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamSpan), C.c_int32,
                                              C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "mfm_sgd_flat_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SgdSpan), C.c_int32, C.c_float, C.c_void_p]),
    "mfm_sgd_flat_spans_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SgdSpan), C.c_int32, C.c_float,
                                             C.c_void_p, C.c_void_p]),
    "mfm_adam_ext_flat_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdamExtSpan),
                                          C.c_int32, C.c_float, C.c_void_p]),
    "mfm_adam_ext_flat_spans_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(AdamExtSpan), C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "mfm_clip_workspace_floats": (C.c_int64, []),
    "mfm_clip_grad_norm_flat_spans": (C.c_int, [C.c_void_p, C.POINTER(ClipSpan), C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_clip_grad_value_flat_spans": (C.c_int, [C.c_void_p, C.POINTER(ClipSpan), C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "mfm_dec_fc1_f32": (C.c_int, [C.POINTER(DecFc1Item), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mfm_avg_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "mfm_keep_best_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_void_p]),
    "mfm_plateau_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(PlateauGroups), C.c_int32, C.c_int32, C.c_int32,
                                   C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mfm_dataset_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int64, C.c_void_p]),
    "mfm_predict_klef_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int64]),
    "mfm_predict_klef": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_void_p]),
    "mfm_encode_klef_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "mfm_encode_klef": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int64,
                                  C.c_void_p]),
    "mfm_encode_mfn_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_encode_mfn_tile_rows": (C.c_int, [C.c_int64, C.c_int64]),
    "mfm_encode_mfn": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_void_p), C.c_int64, C.c_void_p]),
    "mfm_decode_factors_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "mfm_decode_factors": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_void_p]),
    "mfm_objective_klef_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_objective_klef": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p,
                                     C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_objective_mfn_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_objective_mfn_tile_rows": (C.c_int, [C.c_int64, C.c_int64]),
    "mfm_objective_mfn": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p,
                                    C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "mfm_predict_zeros_klef_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_predict_zeros_klef": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_predict_zeros_mfn_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_predict_zeros_mfn_tile_rows": (C.c_int, [C.c_int64, C.c_int64]),
    "mfm_predict_zeros_mfn": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_predict_mfn_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_predict_mfn_tile_rows": (C.c_int, [C.c_int64, C.c_int64]),
    "mfm_predict_mfn": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_influence_factors_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_influence_factors": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_impute_missing_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int64]),
    "mfm_impute_missing_tile_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "mfm_impute_missing": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p), C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_void_p]),
    "mfm_predict_missing_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                                         C.c_int64]),
    "mfm_predict_missing_tile_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "mfm_predict_missing": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p]),
    "mfm_predict_ablation_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                                          C.c_int64]),
    "mfm_predict_ablation_tile_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "mfm_predict_ablation": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_void_p]),
    "mfm_train_ablation_d_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_train_ablation_d_mask_offset": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int64]),
    "mfm_train_ablation_d_tile_rows": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "mfm_train_ablation_d": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                       C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_predict_ablation_mfn_workspace_floats": (C.c_int64, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                                              C.c_int32, C.c_int64]),
    "mfm_predict_ablation_mfn_tile_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "mfm_predict_ablation_mfn": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p]),
    "mfm_p2p_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "mfm_p2p_handle_bytes": (C.c_int, []),
    "mfm_p2p_export": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mfm_p2p_connect": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mfm_p2p_local_base": (C.c_void_p, [C.c_void_p]),
    "mfm_p2p_connect_bases": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mfm_p2p_allreduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mfm_p2p_allreduce_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_void_p]),
    "mfm_p2p_allreduce_adam_guarded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                                 C.c_int64, C.c_void_p]),
    "mfm_p2p_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mfm_p2p_wait_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "mfm_p2p_destroy": (None, [C.c_void_p]),
    "mfm_plan_num_params": (C.c_int, [C.c_int32]),
    "mfm_plan_set_gauss": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mfm_plan_create": (C.c_int, [C.POINTER(PlanConfig), C.POINTER(C.c_int64), C.c_int64,
                                  C.POINTER(C.c_void_p)]),
    "mfm_plan_destroy": (None, [C.c_void_p]),
    "mfm_plan_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "mfm_plan_init_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mfm_plan_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "mfm_plan_backward_ext": (C.c_int, [C.c_void_p] * 11),
    "mfm_plan_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_backward_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LossWeights),
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_out_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mfm_plan_host_status": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32))]),
    "mfm_plan_grad_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_train_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_float,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_train_step_staged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(AdamSpan),
                                             C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "mfm_plan_set_option_str": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "mfm_plan_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "mfm_plan_state_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mfm_plan_clear_status": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfm_plan_latent_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mfm_plan_seq_layout": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "mfm_plan_latent_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mfm_plan_seq_form": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "mfm_plan_mfn_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mfm_plan_flops_per_step": (C.c_double, [C.c_void_p]),
    "mfm_plan_bytes_per_step": (C.c_double, [C.c_void_p]),
    "mfm_plan_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "mfm_plan_set_timing_every": (C.c_int, [C.c_void_p, C.c_int]),
    "mfm_plan_num_kernels": (C.c_int, []),
    "mfm_plan_kernel_name": (C.c_char_p, [C.c_int]),
    "mfm_plan_collect_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mfm_timing_bracket_overhead_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mfm_plan_kernel_flops": (C.c_double, [C.c_void_p, C.c_int]),
}

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MfmError(
                "factorized_amd: %s is missing. Build the gfx950 HIP library first:\n"
                "    python -c 'import __graft_entry__ as g; g.build()'   (or factorized_amd/csrc/build.sh)\n"
                "There is no CPU fallback for this package." % LIB_PATH)
        # torch first: its ROCm runtime (libamdhip64) must be the one this process initialises -- a process that loads this
        # library before torch ends up with two HIP runtimes and "no ROCm-capable device" in the second one
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)   # AttributeError if the ABI and the binding drift apart
            fn.restype = res
            fn.argtypes = args
        if L.mfm_abi_version() != ABI_VERSION:
            raise MfmError("libmfm_hip.so ABI version %d, binding expects %d" % (L.mfm_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().mfm_last_error()
        raise MfmError("%s failed (%d): %s" % (what or "libmfm_hip call", rc,
                                               msg.decode() if msg else "?"))


def exported_names():
    return list(_SIGS)
