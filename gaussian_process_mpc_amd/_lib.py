"""ctypes binding of libgpmpc_hip.so (C ABI: include/gpmpc.h).

torch is imported first on purpose: its bundled HIP runtime (SONAME libamdhip64.so.7)
must be the one already mapped when the library is dlopen'ed, so that device pointers
and streams handed over from torch tensors belong to the same runtime instance.
"""
import ctypes
import os

import torch  # noqa: F401  (loads the HIP runtime the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPMPC_LIB_PATH: another build of the SAME library (diagnostic builds with in-kernel stamps, A/B runs); never a fallback
LIB_PATH = os.environ.get("GPMPC_LIB_PATH") or os.path.join(_HERE, "csrc", "libgpmpc_hip.so")

MAX_D = 8
MAX_DS = 8
MAX_CONS = 16
MPPI_MAX_SAMPLES = 4096
PARTICLE_COST_MAX_P = 4096
LBFGS_MAX_STARTS = 256
LBFGS_MAX_HISTORY = 16
WANT_GRAD = 1
COV_BUG_COMPAT = 2
DESCRIBE_WANT_COV = 0x100      # gpmpc_moment_match_describe: a call with out_cov
USE_GRAPH = 4
FP32_ACCUM = 8
FP32_ALL = 16
LINPROP_FORM_TILE = 0          # gpmpc_linearised_set_form (include/gpmpc.h, "Linearised propagation")
LINPROP_FORM_STREAM = 1
LINPROP_FORM_AUTO = 2
LINPROP_FORM_DEFAULT = LINPROP_FORM_TILE
LINPROP_STREAM_COLS = 4
LINPROP_AUTO_MAX_B = 32        # measured: profiles/linprop/stream_ab.txt

_ERR = {-1: "bad argument", -2: "device allocation failed", -3: "HIP call / kernel launch failed",
        -4: "workspace too small", -5: "pack not built",
        -6: "current HIP device differs from the device the pack was created on"}


class LibraryMissing(RuntimeError):
    pass


class GpmpcError(RuntimeError):
    pass


class CostParamsC(ctypes.Structure):
    _fields_ = [("gamma", ctypes.c_double),
                ("Q", ctypes.c_double * (MAX_DS * MAX_DS)),
                ("R", ctypes.c_double * (MAX_D * MAX_D)),
                ("R_delta", ctypes.c_double * (MAX_D * MAX_D)),
                ("x_ref", ctypes.c_double * MAX_DS),
                ("u_ref", ctypes.c_double * MAX_D),
                ("last_u", ctypes.c_double * MAX_D),
                ("has_R_delta", ctypes.c_int),
                ("schedule_id", ctypes.c_int)]


class StateConstraintsC(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int),
                ("reserved", ctypes.c_int),
                ("A", ctypes.c_double * (MAX_CONS * MAX_DS)),
                ("b", ctypes.c_double * MAX_CONS),
                ("kappa", ctypes.c_double * MAX_CONS)]


class InputConstraintsC(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int),
                ("reserved", ctypes.c_int),
                ("C", ctypes.c_double * (MAX_CONS * MAX_D)),
                ("d", ctypes.c_double * MAX_CONS),
                ("kappa", ctypes.c_double * MAX_CONS)]


class MppiParamsC(ctypes.Structure):
    _fields_ = [("n_samples", ctypes.c_int),
                ("iterations", ctypes.c_int),
                ("sigma", ctypes.c_double * MAX_D),
                ("sigma_decay", ctypes.c_double),
                ("beta", ctypes.c_double),
                ("seed", ctypes.c_ulonglong),
                ("call_index", ctypes.c_uint),
                ("reserved", ctypes.c_uint),
                ("lb", ctypes.c_double * MAX_D),
                ("ub", ctypes.c_double * MAX_D)]


class LbfgsParamsC(ctypes.Structure):
    _fields_ = [("n_starts", ctypes.c_int),
                ("history", ctypes.c_int),
                ("gtol", ctypes.c_double),
                ("ftol", ctypes.c_double),
                ("c1", ctypes.c_double),
                ("min_step", ctypes.c_double),
                ("lb", ctypes.c_double * MAX_D),
                ("ub", ctypes.c_double * MAX_D)]


class AuglagParamsC(ctypes.Structure):
    _fields_ = [("inner", LbfgsParamsC),
                ("rho0", ctypes.c_double),
                ("growth", ctypes.c_double),
                ("shrink", ctypes.c_double),
                ("rho_max", ctypes.c_double),
                ("lam_max", ctypes.c_double),
                ("feas_tol", ctypes.c_double),
                ("inner_ticks", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class GPModelC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int),
                ("state_dim", ctypes.c_int),
                ("action_dim", ctypes.c_int),
                ("has_nominal", ctypes.c_int),
                ("has_noise", ctypes.c_int),
                ("reserved", ctypes.c_int),
                ("X", ctypes.c_void_p),
                ("beta", ctypes.c_void_p),
                ("Kinv", ctypes.c_void_p),
                ("ld", ctypes.c_size_t),
                ("gp_stride", ctypes.c_size_t),
                ("lambdas", ctypes.c_double * (MAX_DS * MAX_D)),
                ("sigma_f", ctypes.c_double * MAX_DS),
                ("nom_w", ctypes.c_double * (MAX_DS * MAX_D)),
                ("nom_b", ctypes.c_double * MAX_DS),
                ("init_cov", ctypes.c_double * (MAX_DS * MAX_DS)),
                ("action_var", ctypes.c_double * MAX_D),
                ("process_var", ctypes.c_double * MAX_DS)]


_vp, _i, _d, _sz, _u = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_uint
_dp = ctypes.POINTER(ctypes.c_double)
_ull = ctypes.c_ulonglong
_gm, _sc = ctypes.POINTER(GPModelC), ctypes.POINTER(StateConstraintsC)
_ic = ctypes.POINTER(InputConstraintsC)

# name -> (restype, argtypes); every symbol include/gpmpc.h declares
SIGNATURES = {
    "gpmpc_device_count": (_i, []),
    "gpmpc_version": (ctypes.c_char_p, []),
    "gpmpc_last_error": (ctypes.c_char_p, []),
    "gpmpc_pack_create": (_i, [ctypes.POINTER(_vp), _i, _i, _i]),
    "gpmpc_pack_destroy": (_i, [_vp]),
    "gpmpc_pack_resize": (_i, [_vp, _i]),
    "gpmpc_pack_reload_tuning": (_i, [_vp]),
    "gpmpc_pack_graph_captures": (ctypes.c_longlong, [_vp]),
    "gpmpc_pack_callback_captures": (ctypes.c_longlong, [_vp]),
    "gpmpc_store_host": (_i, [_vp, _vp, _sz, _vp]),
    "gpmpc_build_ky": (_i, [_i, _i, _vp, _dp, _d, _d, _vp, _vp, _vp]),
    "gpmpc_pack_build": (_i, [_vp, _vp, _vp, _vp, _dp, _dp, _vp]),
    "gpmpc_pack_build_strided": (_i, [_vp, _vp, _vp, _vp, _sz, _sz, _dp, _dp, _vp]),
    "gpmpc_pack_build_beta": (_i, [_vp, _vp, _vp, _vp, _dp, _dp, _vp]),
    "gpmpc_pack_set_nominal": (_i, [_vp, _dp, _dp, _vp]),
    "gpmpc_pack_get_nominal": (_i, [_vp, _dp, _dp]),
    "gpmpc_pack_set_noise": (_i, [_vp, _dp, _dp, _dp, _vp]),
    "gpmpc_pack_get_noise": (_i, [_vp, _dp, _dp, _dp]),
    "gpmpc_pack_enable_fullcov": (_i, [_vp, _vp]),
    "gpmpc_pack_dims": (_i, [_vp] + [ctypes.POINTER(_i)] * 4),
    "gpmpc_pack_shared_lambda": (_i, [_vp]),
    "gpmpc_pack_export": (_i, [_vp, _vp, _vp, _vp]),
    "gpmpc_moment_match_workspace_bytes": (_sz, [_vp, _i]),
    "gpmpc_moment_match": (_i, [_vp, _i, _vp, _vp, _u] + [_vp] * 10 + [_vp, _sz, _vp]),
    "gpmpc_moment_match_describe": (_i, [_vp, _i, _u, ctypes.c_char_p, _sz]),
    "gpmpc_cost": (_i, [_i, _i, _i, _i, ctypes.POINTER(CostParamsC), _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_cost_grad": (_i, [_i, _i, _i, _i, ctypes.POINTER(CostParamsC)] + [_vp] * 8),
    "gpmpc_cost_schedule_create": (_i, [_i, _i, _i, ctypes.POINTER(_i)]),
    "gpmpc_cost_schedule_destroy": (_i, [_i]),
    "gpmpc_cost_schedule_set": (_i, [_i, _i, _dp, _dp, _dp, _vp]),
    "gpmpc_cost_schedule_set_dev": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "gpmpc_cost_schedule_get": (_i, [_i] + [ctypes.POINTER(_i)] * 5 + [ctypes.POINTER(_vp)]),
    "gpmpc_rollout_jac_workspace_bytes": (_sz, [_vp, _i, _i]),
    "gpmpc_rollout_jac": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_rollout_vjp": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_rollout_constraints": (_i, [_i, _i, _i, _i, ctypes.POINTER(StateConstraintsC), _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_rollout_constrained_workspace_bytes": (_sz, [_vp, _i, _i, _u]),
    "gpmpc_rollout_constrained": (_i, [_vp, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC), _u,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_mppi_sample": (_i, [_i, _i, _i, ctypes.POINTER(MppiParamsC), _i, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_mppi_update": (_i, [_i, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_mppi_solve_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(MppiParamsC), ctypes.POINTER(StateConstraintsC)]),
    "gpmpc_mppi_solve": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC),
                              ctypes.POINTER(MppiParamsC), _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_lbfgs_state_bytes": (_sz, [_i, _i, _i, _i]),
    "gpmpc_lbfgs_start": (_i, [_i, _i, _i, ctypes.POINTER(LbfgsParamsC), _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_lbfgs_tick": (_i, [_i, _i, ctypes.POINTER(LbfgsParamsC), _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_lbfgs_solve_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(LbfgsParamsC)]),
    "gpmpc_lbfgs_solve": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(LbfgsParamsC), _i, _i, _vp, _sz, _vp]),
    "gpmpc_auglag_state_bytes": (_sz, [_i, _i, _i, _i]),
    "gpmpc_auglag_merit": (_i, [_i, _i, _i, _i] + [_vp] * 9),
    "gpmpc_auglag_outer": (_i, [_i, _i, _i, ctypes.POINTER(AuglagParamsC), _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_auglag_solve_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(StateConstraintsC), ctypes.POINTER(AuglagParamsC)]),
    "gpmpc_auglag_solve": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC),
                                ctypes.POINTER(AuglagParamsC), _i, _i, _vp, _sz, _vp]),
    "gpmpc_rollout_workspace_bytes": (_sz, [_vp, _i, _i, _u]),
    "gpmpc_plan_describe": (_i, [_vp, _i, _i, _u, ctypes.c_char_p, _sz]),
    "gpmpc_pack_autotune": (_i, [_vp, _i, _i, _u, ctypes.c_char_p, _sz]),
    "gpmpc_pack_autotune_clear": (_i, [_vp]),
    "gpmpc_rollout": (_i, [_vp, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), _u, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_objective_gradient": (_i, [_vp, _i, _dp, _dp, ctypes.POINTER(CostParamsC), _u, _dp, _vp]),
    "gpmpc_rollout_fullcov_workspace_bytes": (_sz, [_vp, _i, _i, _u]),
    "gpmpc_rollout_fullcov_describe": (_i, [_vp, _i, _i, _u, ctypes.c_char_p, _sz]),
    "gpmpc_rollout_fullcov": (_i, [_vp, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), _u, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_rollout_fullcov_jac_workspace_bytes": (_sz, [_vp, _i, _i]),
    "gpmpc_rollout_fullcov_jac": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_rollout_fullcov_constrained_workspace_bytes": (_sz, [_vp, _i, _i, _u]),
    "gpmpc_rollout_fullcov_constrained": (_i, [_vp, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC), _u,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_mppi_solve_fullcov_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(MppiParamsC), ctypes.POINTER(StateConstraintsC)]),
    "gpmpc_mppi_solve_fullcov": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC),
                                      ctypes.POINTER(MppiParamsC), _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_lbfgs_solve_fullcov_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(LbfgsParamsC)]),
    "gpmpc_lbfgs_solve_fullcov": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(LbfgsParamsC), _i, _i, _vp, _sz, _vp]),
    "gpmpc_auglag_solve_fullcov_workspace_bytes": (_sz, [_vp, _i, ctypes.POINTER(StateConstraintsC), ctypes.POINTER(AuglagParamsC)]),
    "gpmpc_auglag_solve_fullcov": (_i, [_vp, _i, _vp, _vp, ctypes.POINTER(CostParamsC), ctypes.POINTER(StateConstraintsC),
                                        ctypes.POINTER(AuglagParamsC), _i, _i, _vp, _sz, _vp]),
    "gpmpc_timing_enable": (_i, [_i]),
    "gpmpc_debug_run_list": (_i, [_i, _i, _i, ctypes.POINTER(_i), _i, ctypes.POINTER(_i)]),
    "gpmpc_debug_work_list": (_i, [_i] * 7 + [ctypes.POINTER(_i), _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gpmpc_debug_fcs_tables": (_i, [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gpmpc_debug_xcd_order": (_i, [_i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gpmpc_pair_kernel_time": (_i, [_dp, ctypes.POINTER(ctypes.c_longlong), _i]),
    "gpmpc_pair_kernel_time_class": (_i, [_i, _dp, ctypes.POINTER(ctypes.c_longlong)]),
    "gpmpc_matvec": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "gpmpc_kinv_append_workspace_bytes": (_sz, [_i]),
    "gpmpc_kinv_append": (_i, [_i, _vp, _vp, _d, _vp, _vp, _sz, _vp]),
    "gpmpc_gp_append_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_gp_append": (_i, [_i, _i, _vp, _vp, _dp, _d, _d, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gpmpc_kinv_remove": (_i, [_i, _vp, _sz, _i, _vp, _sz, _vp]),
    "gpmpc_gp_replace_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_gp_replace": (_i, [_i, _i, _i, _vp, _vp, _dp, _d, _d, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gpmpc_predict_workspace_bytes": (_sz, [_i, _i, _i]),
    "gpmpc_predict": (_i, [_i, _i, _vp, _dp, _d, _vp, _vp, _d, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_ml_grad_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_ml_grad": (_i, [_i, _i, _vp, _vp, _vp, _vp, _dp, _d, _d, _vp, _vp, _sz, _vp]),
    "gpmpc_sparse_set_form": (_i, [_i]),
    "gpmpc_sparse_accumulate_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "gpmpc_sparse_accumulate": (_i, [_i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _sz, _dp, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_sparse_finish_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_sparse_finish": (_i, [_i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_sparse_append_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_sparse_append": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _dp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_sparse_remove_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_sparse_remove": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _dp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_sparse_replace_workspace_bytes": (_sz, [_i, _i]),
    "gpmpc_sparse_replace": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _dp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpmpc_gp_posterior_workspace_bytes": (_sz, [_gm, _i, _i]),
    "gpmpc_gp_posterior": (_i, [_gm, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_particle_noise": (_i, [_i, _i, _i, _ull, _u, _vp, _vp]),
    "gpmpc_particle_step_workspace_bytes": (_sz, [_gm, _i, _i, _i]),
    "gpmpc_particle_step": (_i, [_gm, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_particle_stats": (_i, [_i, _i, _i, _i, _vp, _vp, _sc, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_particle_rollout_workspace_bytes": (_sz, [_gm, _i, _i, _i, _i]),
    "gpmpc_particle_rollout": (_i, [_gm, _i, _i, _i, _vp, _vp, _ull, _u, _sc, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_particle_cost": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(CostParamsC), _sc, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_particle_evaluate_workspace_bytes": (_sz, [_gm, _i, _i, _i, _i]),
    "gpmpc_particle_evaluate": (_i, [_gm, _i, _i, _i, _vp, _vp, _ull, _u, ctypes.POINTER(CostParamsC), _sc, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_mppi_solve_particles_workspace_bytes": (_sz, [_gm, _i, _i, ctypes.POINTER(MppiParamsC), _sc]),
    "gpmpc_mppi_solve_particles": (_i, [_gm, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), _sc, ctypes.POINTER(MppiParamsC), _vp, _vp, _vp,
                                        _vp, _sz, _vp]),
    "gpmpc_linearised_set_form": (_i, [_i]),
    "gpmpc_linearised_step_workspace_bytes": (_sz, [_gm, _i, _i, _i]),
    "gpmpc_linearised_step": (_i, [_gm, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _i, _vp, _sz, _vp]),
    "gpmpc_linearised_rollout_workspace_bytes": (_sz, [_gm, _i, _i, _u, _i]),
    "gpmpc_linearised_rollout": (_i, [_gm, _i, _i, _vp, _vp, ctypes.POINTER(CostParamsC), _sc, _u, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp,
                                      _sz, _vp]),
    "gpmpc_mppi_solve_linearised_workspace_bytes": (_sz, [_gm, _i, ctypes.POINTER(MppiParamsC), _sc]),
    "gpmpc_mppi_solve_linearised": (_i, [_gm, _i, _vp, _vp, ctypes.POINTER(CostParamsC), _sc, ctypes.POINTER(MppiParamsC), _vp, _vp, _vp, _vp,
                                         _sz, _vp]),
    "gpmpc_linearised_fc_step_workspace_bytes": (_sz, [_gm, _i, _i, _i]),
    "gpmpc_linearised_fc_step": (_i, [_gm, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _i, _vp, _sz, _vp]),
    "gpmpc_linearised_fc_rollout_workspace_bytes": (_sz, [_gm, _i, _i, _u, _i]),
    "gpmpc_linearised_fc_rollout": (_i, [_gm, _i, _i, _vp, _vp, _vp, _sz, ctypes.POINTER(CostParamsC), _sc, _u, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _i, _vp, _sz, _vp]),
    "gpmpc_linearised_fc_vjp": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_linearised_fc_constraints": (_i, [_i, _i, _i, _i, _sc, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_feedback_input_cost": (_i, [_i, _i, _i, _i, ctypes.POINTER(CostParamsC), _vp, _sz, _vp, _vp, _vp, _vp]),
    "gpmpc_feedback_input_constraints": (_i, [_i, _i, _i, _i, _ic, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_particle_inputs": (_i, [_i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "gpmpc_particle_step_inputs_workspace_bytes": (_sz, [_gm, _i, _i, _i]),
    "gpmpc_particle_step_inputs": (_i, [_gm, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_particle_input_stats": (_i, [_i, _i, _i, _i, _vp, _ic, _vp, _vp, _vp, _vp, _vp]),
    "gpmpc_particle_rollout_feedback_workspace_bytes": (_sz, [_gm, _i, _i, _i, _i, _i]),
    "gpmpc_particle_rollout_feedback": (_i, [_gm, _i, _i, _i, _vp, _vp, _ull, _u, _sc, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _ic, _vp, _vp,
                                             _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "gpmpc_linearised_fc_rollout_inputs_workspace_bytes": (_sz, [_gm, _i, _i, _u, _i, _i, _ic]),
    "gpmpc_linearised_fc_rollout_inputs": (_i, [_gm, _i, _i, _vp, _vp, _vp, _sz, ctypes.POINTER(CostParamsC), _sc, _u, _vp, _vp, _vp, _vp, _vp,
                                                _vp, _vp, _i, _ic, _vp, _vp, _i, _vp, _sz, _vp]),
}

_lib = None


def lib():
    """The loaded library; raises LibraryMissing (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gaussian_process_mpc_amd/csrc`. There is no CPU fallback.")
        h = ctypes.CDLL(LIB_PATH)
        # A/B runs against an OLDER build of the library (GPMPC_LIB_PATH + GPMPC_LIB_ALLOW_MISSING=1, tools/lib_ab.py) may lack
        # entry points added since; the product library must export every declared symbol
        tolerant = bool(os.environ.get("GPMPC_LIB_PATH")) and os.environ.get("GPMPC_LIB_ALLOW_MISSING") == "1"
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(h, name)      # AttributeError if a declared symbol is missing
            except AttributeError:
                if tolerant:
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        detail = lib().gpmpc_last_error().decode() if rc == -3 else ""
        if rc == -1 and ("mppi" in what or "lbfgs" in what or "auglag" in what or "sparse" in what or "particle" in what
                         or "gp_posterior" in what or "linearised" in what or "fullcov_" in what):    # these refusals say which parameter
            detail = lib().gpmpc_last_error().decode()
        if rc == -1 and not detail:        # refusals of a cost schedule say which and why
            why = lib().gpmpc_last_error().decode()
            detail = why if "cost schedule" in why else ""
        if rc == -5:                       # refusals on a pack with a nominal model say why (others leave the text alone)
            why = lib().gpmpc_last_error().decode()
            detail = why if ("nominal model" in why or why.startswith(what + ":")) else ""      # (its own text: never a stale one)
        raise GpmpcError(f"{what} failed: {_ERR.get(rc, rc)} {detail}".strip())


def require_gpu():
    """Device for all numerical work.  Raises if no GPU is visible (no CPU fallback)."""
    lib()
    if not torch.cuda.is_available():
        raise GpmpcError("no HIP device visible: the GP-MPC rollout runs on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr(device=None):
    """Current HIP stream of `device` (default: the current device) as a void*.  The device index is passed explicitly:
    torch.cuda.current_stream() WITHOUT one goes through torch.cuda.is_available() on every call, which costs ~0.1 ms per
    call in a fresh process (measured on the solver-callback path: it doubled the latency of a C1 callback pair)."""
    idx = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
    return ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


def ptr(t):
    """Device pointer of a contiguous float64 CUDA tensor (or NULL for None)."""
    if t is None:
        return ctypes.c_void_p(0)
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return ctypes.c_void_p(t.data_ptr())


def host_doubles(a):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_dp)
