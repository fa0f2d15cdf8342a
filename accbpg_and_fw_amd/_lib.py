"""ctypes binding of libaccbpg_hip.so (C-ABI: include/accbpg_hip.h).

There is no CPU fallback: if the shared library is missing or a device tensor is
required and absent, the call raises.  Error codes are mapped to the exception
types the reference raises in the same situations (accbpg/functions.py:44-50,
233-234, 251-252, 269-270, 340).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ACCBPG_HIP_LIB: development builds of the same library, e.g. the experiment of DESIGN.md section 4)
LIB_PATH = os.environ.get("ACCBPG_HIP_LIB") or os.path.join(_HERE, "lib", "libaccbpg_hip.so")

OK, ERR_ASSERT, ERR_NOT_PD, ERR_HIP, ERR_ARG = 0, 1, 2, 3, 4

_lib = None


class FwProbe(C.Structure):
    _fields_ = [("i", C.c_int64), ("j", C.c_int64), ("w_i", C.c_double), ("w_j", C.c_double),
                ("x_j", C.c_double), ("logdet_H", C.c_double), ("q_prev", C.c_double)]


class FwDivProbe(C.Structure):
    """The record of accbpg_fw_div_probe_step (accbpg_fw_div_probe)."""
    _fields_ = [("i", C.c_int64), ("w_i", C.c_double), ("x_i", C.c_double), ("sum_w", C.c_double),
                ("sum_w2", C.c_double), ("slope", C.c_double), ("div", C.c_double), ("min_x", C.c_double),
                ("sum_u2", C.c_double)]


class FwStep(C.Structure):
    """One record of accbpg_fw_run: the probe record, the update the device applied, and what became of the step."""
    _fields_ = [("i", C.c_int64), ("j", C.c_int64), ("w_i", C.c_double), ("w_j", C.c_double), ("x_j", C.c_double),
                ("q_prev", C.c_double), ("p", C.c_int64), ("xscale", C.c_double), ("xadd", C.c_double),
                ("hcoef", C.c_double), ("hdiv", C.c_double), ("kind", C.c_int32), ("status", C.c_int32)]


class FwDivParams(C.Structure):
    """accbpg_fw_div_params: the run parameters and the host's exact book at the start of an accbpg_fw_div_run call."""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("k0", C.c_int64), ("L", C.c_double),
                ("gamma", C.c_double), ("ls_ratio", C.c_double), ("epsilon", C.c_double), ("ld", C.c_double),
                ("q", C.c_double), ("F_prev", C.c_double)]


class FwDivStep(C.Structure):
    """One record of accbpg_fw_div_run (accbpg_fw_div_step): the probe record, the step the device predicted with its
    own book behind it, and what became of it."""
    _fields_ = [("probe", FwDivProbe), ("L", C.c_double), ("a", C.c_double), ("hcoef", C.c_double),
                ("hdiv", C.c_double), ("ld1", C.c_double), ("q1", C.c_double), ("f1", C.c_double),
                ("trials", C.c_int32), ("status", C.c_int32), ("reason", C.c_int32), ("reserved", C.c_int32)]


class TrialOut(C.Structure):
    """accbpg_trial_out: what a clean accbpg_dopt_burg_trial returns."""
    _fields_ = [("fy", C.c_double), ("lin", C.c_double), ("dxy", C.c_double), ("dzz", C.c_double), ("fx", C.c_double),
                ("fk", C.c_double), ("prox_info", C.c_int32 * 2), ("fk_answered", C.c_int32), ("reserved", C.c_int32)]


TRIAL_REPLAY = 5            # ACCBPG_TRIAL_REPLAY
FW_RUN_MAX = 1024           # ACCBPG_FW_RUN_MAX
FW_APPLIED, FW_STOPPED, FW_BAD_PIVOT, FW_NOT_RUN = 0, 1, 2, 3      # accbpg_fw_step.status
FW_DIV_TRIALS_MAX = 64      # ACCBPG_FW_DIV_TRIALS_MAX
FW_DIV_LINESEARCH, FW_DIV_FIXED_L, FW_DIV_CLASSICAL = 0, 1, 2      # accbpg_fw_div_params.mode
FW_DIV_APPLIED, FW_DIV_STOPPED, FW_DIV_HANDED_BACK, FW_DIV_NOT_RUN = 0, 1, 2, 3    # accbpg_fw_div_step.status
(FW_DIV_HB_NONE, FW_DIV_HB_BUDGET, FW_DIV_HB_L_INF, FW_DIV_HB_SLOPE, FW_DIV_HB_MIN_X, FW_DIV_HB_PIVOT, FW_DIV_HB_CAP,
 FW_DIV_HB_ARITH) = range(8)                                        # accbpg_fw_div_step.reason
(FW_DIV_RP_END, FW_DIV_RP_STOP, FW_DIV_RP_DEVICE_HB, FW_DIV_RP_HOST_HB, FW_DIV_RP_DISAGREE,
 FW_DIV_RP_PIVOT) = range(6)                                        # accbpg_fw_div_replay: *verdict_out

_P = C.c_void_p
_SIGS = {
    "accbpg_abi_version": (C.c_int, []),
    "accbpg_last_error": (C.c_char_p, []),
    "accbpg_dopt_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, C.POINTER(_P), C.c_int]),
    "accbpg_dopt_destroy": (C.c_int, [_P]),
    "accbpg_dopt_set_stream": (C.c_int, [_P, _P]),
    "accbpg_dopt_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_dopt_func_grad_begin": (C.c_int, [_P, _P, C.c_int, _P]),
    "accbpg_dopt_func_grad_end": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "accbpg_dopt_eval_gap_ms": (C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    "accbpg_dopt_burg_trial": (C.c_int, [_P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P,
                                         C.POINTER(TrialOut)]),
    "accbpg_dopt_value_reuse": (C.c_int, [_P, C.c_int]),
    "accbpg_dopt_value_reuse_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "accbpg_dopt_value_recorded": (C.c_int, [_P, _P]),
    "accbpg_dopt_value_peer": (C.c_int, [_P, _P]),
    "accbpg_dopt_gram": (C.c_int, [_P, _P, _P]),
    "accbpg_dopt_factor": (C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    "accbpg_dopt_grad": (C.c_int, [_P, _P]),
    "accbpg_tri_pack": (C.c_int, [_P, C.c_int64, _P, _P]),
    "accbpg_tri_unpack": (C.c_int, [_P, C.c_int64, _P, _P]),
    "accbpg_vec_count_bad": (C.c_int, [_P, C.c_int64, _P, _P]),
    "accbpg_dopt_shard_bounds": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "accbpg_shard_unique_id": (C.c_int, [_P]),
    "accbpg_dopt_shard_create": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, _P, C.POINTER(_P)]),
    "accbpg_dopt_shard_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_dopt_shard_destroy": (C.c_int, [_P]),
    "accbpg_debug_shard_pad": (C.c_int, [_P, C.c_int64]),
    "accbpg_dopt_gram_lincomb": (C.c_int, [_P, C.c_double, _P, C.c_double, _P, _P]),
    "accbpg_dopt_eval_gram": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_dopt_batch_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int64, C.c_int64, C.c_int64, _P, C.POINTER(_P)]),
    "accbpg_dopt_batch_destroy": (C.c_int, [_P]),
    "accbpg_dopt_batch_set_stream": (C.c_int, [_P, _P]),
    "accbpg_dopt_batch_size": (C.c_int, [_P]),
    "accbpg_dopt_batch_is_fused": (C.c_int, [_P]),
    "accbpg_dopt_batch_chunk": (C.c_int, [_P]),
    "accbpg_dopt_batch_instance": (_P, [_P, C.c_int]),
    "accbpg_dopt_batch_func_grad": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), _P,
                                              C.c_int64, C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_func_grad_begin": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int), C.c_int, _P, C.c_int64]),
    "accbpg_dopt_batch_func_grad_end": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_burg_simplex_div_prox": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), C.c_double, _P,
                                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_burg_simplex_avg_prox": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double),
                                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _P, _P,
                                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_ls_terms": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_axpby": (C.c_int, [_P, C.POINTER(C.c_double), _P, C.POINTER(C.c_double), _P, C.c_int64,
                                          C.POINTER(C.c_int), _P]),
    "accbpg_vec_workspace_doubles": (C.c_int64, [C.c_int64]),
    "accbpg_burg_simplex_div_prox": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int64, _P, _P,
                                               C.POINTER(C.c_int), _P]),
    "accbpg_burg_divergence": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_ls_terms": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_vec_axpby": (C.c_int, [C.c_double, _P, C.c_double, _P, C.c_int64, _P, _P]),
    "accbpg_vec_dot_diff": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_vec_min_sum": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_vec_div_scalar": (C.c_int, [_P, C.c_double, C.c_int64, _P, _P]),
    "accbpg_vec_vertex": (C.c_int, [C.c_int64, C.c_double, C.c_double, C.c_int64, _P, _P]),
    "accbpg_vec_argminmax": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), _P, _P]),
    "accbpg_dopt_vt_times": (C.c_int, [_P, _P, _P]),
    "accbpg_dopt_get_column": (C.c_int, [_P, C.c_int64, _P]),
    "accbpg_dopt_kyinit": (C.c_int, [_P, _P, C.POINTER(C.c_int64), _P]),
    "accbpg_fw_init": (C.c_int, [_P, _P, C.POINTER(C.c_double)]),
    "accbpg_fw_probe_step": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(FwProbe)]),
    "accbpg_fw_logdet_flush": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "accbpg_fw_logdet_ring": (C.c_int, [_P, C.c_int, C.c_int]),
    "accbpg_fw_logdet_pending": (C.c_int, [_P]),
    "accbpg_fw_update": (C.c_int, [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double]),
    "accbpg_fw_get_state": (C.c_int, [_P, _P, _P, _P]),
    "accbpg_fw_div_probe_step": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(FwDivProbe)]),
    "accbpg_fw_div_apply": (C.c_int, [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "accbpg_fw_logdet_snapshot": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "accbpg_fw_run": (C.c_int, [_P, C.c_int, C.c_double, C.c_int, C.POINTER(FwStep), C.POINTER(C.c_int)]),
    "accbpg_fw_div_run": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(FwDivParams), C.c_int, C.POINTER(FwDivStep),
                                    C.POINTER(C.c_int)]),
    "accbpg_fw_set_state": (C.c_int, [_P, _P, _P, _P]),
    "accbpg_dopt_batch_fw_init": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_fw_probe": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(FwProbe)]),
    "accbpg_dopt_batch_fw_update": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "accbpg_dopt_batch_fw_div_probe": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(FwDivProbe)]),
    "accbpg_dopt_batch_fw_div_apply": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                                 C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "accbpg_dopt_batch_fw_run": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(FwStep), C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_fw_div_run": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(FwDivParams), C.c_int,
                                               C.POINTER(C.c_int), C.POINTER(FwDivStep), C.POINTER(C.c_int)]),
    "accbpg_fw_div_replay": (C.c_int, [C.POINTER(FwDivParams), C.c_int64, C.c_int64, C.c_double, C.c_double,
                                       C.POINTER(FwDivStep), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(FwDivParams), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "accbpg_dopt_batch_kyinit": (C.c_int, [_P, _P, C.POINTER(C.c_int64), _P]),
    "accbpg_poisson_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.POINTER(_P)]),
    "accbpg_poisson_destroy": (C.c_int, [_P]),
    "accbpg_poisson_set_stream": (C.c_int, [_P, _P]),
    "accbpg_poisson_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_poisson_get_ax": (C.c_int, [_P, _P]),
    "accbpg_kldiv_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.POINTER(_P)]),
    "accbpg_kldiv_destroy": (C.c_int, [_P]),
    "accbpg_kldiv_set_stream": (C.c_int, [_P, _P]),
    "accbpg_kldiv_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_kldiv_get_ax": (C.c_int, [_P, _P]),
    "accbpg_svm_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.POINTER(_P)]),
    "accbpg_svm_destroy": (C.c_int, [_P]),
    "accbpg_svm_set_stream": (C.c_int, [_P, _P]),
    "accbpg_svm_func_grad": (C.c_int, [_P, _P, C.c_double, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_svm_get_ax": (C.c_int, [_P, _P]),
    "accbpg_logistic_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.POINTER(_P)]),
    "accbpg_logistic_destroy": (C.c_int, [_P]),
    "accbpg_logistic_set_stream": (C.c_int, [_P, _P]),
    "accbpg_logistic_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_logistic_get": (C.c_int, [_P, C.c_int, _P]),
    "accbpg_logistic_line_begin": (C.c_int, [_P, _P]),
    "accbpg_logistic_line_value": (C.c_int, [_P, C.c_double, C.POINTER(C.c_double)]),
    "accbpg_logistic_line_accept": (C.c_int, [_P, C.c_double]),
    "accbpg_logistic_func_grad_carried": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_fw_direction": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_double, C.c_double, C.c_int64, _P, _P,
                                      C.POINTER(C.c_double), C.POINTER(C.c_int64), _P, _P]),
    "accbpg_l2l1linf_prox": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_double, C.c_int64, _P, _P]),
    "accbpg_l1_norm": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_sq_ls_terms": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_shannon_div_prox": (C.c_int, [C.c_int, _P, _P, C.c_double, C.c_double, C.c_int64, _P, _P, _P]),
    "accbpg_shannon_ls_terms": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_double, C.POINTER(C.c_double), _P, _P]),
    "accbpg_shannon_divergence": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.POINTER(C.c_double), _P, _P]),
    "accbpg_symnmf_create": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_double, _P, C.POINTER(_P)]),
    "accbpg_symnmf_destroy": (C.c_int, [_P]),
    "accbpg_symnmf_set_stream": (C.c_int, [_P, _P]),
    "accbpg_symnmf_func_grad": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_symnmf_plan": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "accbpg_quartic_prox_stage": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int64, _P,
                                            C.POINTER(C.c_double), _P, _P]),
    "accbpg_quartic_ls_terms": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_lmo_l2_ball": (C.c_int, [_P, C.c_int, _P, C.c_double, C.c_double, C.c_double, C.c_int64, _P,
                                     C.POINTER(C.c_double), _P, _P]),
    "accbpg_lmo_linf_ball": (C.c_int, [_P, C.c_int, _P, C.c_double, C.c_double, C.c_int64, _P, _P]),
    "accbpg_burg_reg_div_prox": (C.c_int, [C.c_int, _P, _P, C.c_double, C.c_double, C.c_int64, _P, _P]),
    "accbpg_vec_dot": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_double), _P, _P]),
    "accbpg_combine_ls_terms": (C.c_int, [C.c_int, C.c_double, _P, C.c_double, _P, C.c_double, _P, _P, C.c_int64, _P,
                                          C.POINTER(C.c_double), _P, _P]),
    "accbpg_burg_simplex_prox_acc": (C.c_int, [_P, C.c_double, _P, C.c_double, C.c_double, C.c_int64, _P, _P, _P,
                                               C.POINTER(C.c_int), _P]),
    "accbpg_lmo_l2_ball_pos": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int64, _P, C.POINTER(C.c_double), _P, _P]),
    "accbpg_dopt_profile_enable": (C.c_int, [_P, C.c_int]),
    "accbpg_dopt_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "accbpg_dopt_profile_reset": (C.c_int, [_P]),
    "accbpg_debug_pipe_probe": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_mfma_f64_peak": (C.c_int, [C.c_int, C.POINTER(C.c_double), _P]),
    "accbpg_dopt_factor_in_small_launches": (C.c_int, [_P, C.c_int]),
    "accbpg_debug_chol_variant": (C.c_int, [_P, C.c_int]),
    "accbpg_debug_plan_flags": (C.c_int, [C.c_int]),
    "accbpg_debug_guard_bands": (C.c_int, [C.c_int64]),
    "accbpg_debug_guard_check": (C.c_int, [C.POINTER(C.c_int64)]),
    "accbpg_debug_gemm_loop": (C.c_int, [C.c_int]),
    "accbpg_debug_prox_variant": (C.c_int, [C.c_int]),
    "accbpg_debug_prox_state": (C.c_int, [C.POINTER(C.c_int)]),
    "accbpg_debug_chol_trace": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int64)]),
    "accbpg_debug_gram_variant": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "accbpg_debug_grad_variant": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "accbpg_test_gemm": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int, _P]),
}

EXPORTS = tuple(sorted(_SIGS))


def load():
    """Load the shared library once; raise loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "accbpg_and_fw_amd: %s is missing -- build it with "
            "`make -C accbpg_and_fw_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    msg = load().accbpg_last_error()
    return msg.decode() if msg else ""


def check(rc, what, assert_msg=None):
    """Map a C-ABI status to the reference's exception types."""
    if rc == OK:
        return
    if rc == ERR_ASSERT:
        raise AssertionError(assert_msg or last_error() or what)
    if rc == ERR_NOT_PD:
        raise ValueError("HXHT is singular or not positive definite")   # functions.py:50
    if rc == ERR_ARG:
        raise ValueError("%s: bad argument (%s)" % (what, last_error()))
    raise RuntimeError("%s: HIP error: %s" % (what, last_error()))
