"""MI355X-native hot path of risk-sensitive GP-MPC.

The compute path is the hand-written HIP library ``csrc/libgpmpc_hip.so`` reached
through the C ABI declared in ``include/gpmpc.h``; this package is the host side that
mirrors the reference's Python surface for the path (same class / method names and
argument meaning):

* :class:`GaussianProcessRegression`  (reference ``src/gpr.py``)
* :class:`Dynamics`                   (reference ``src/dynamics.py``)
* :class:`RiskSensitiveMPC`           (reference ``src/mpc.py``)
* :func:`mean_prop_torch`, :func:`variance_prop_torch`, :func:`covariance_prop_torch`
  (reference ``src/tools/uncertainty_prop.py``)

There is no CPU fallback: every numerical entry point raises if the HIP library or a
GPU is missing.
"""
from ._lib import lib, LibraryMissing, GpmpcError, require_gpu          # noqa: F401
from .gpr import GaussianProcessRegression                              # noqa: F401
from .dynamics import Dynamics                                          # noqa: F401
from .mpc import RiskSensitiveMPC                                       # noqa: F401
from .uncertainty_prop import mean_prop_torch, variance_prop_torch, covariance_prop_torch  # noqa: F401
from .simulator import Simulator, PendulumPlant, CartPolePlant          # noqa: F401
from .rollout import GPPack, CostParams, CostSchedule, StateConstraints, InputConstraints, rollout, rollout_constraints, rollout_fullcov, rollout_fullcov_jac, moment_match   # noqa: F401
from .nominal import LinearNominalModel                                 # noqa: F401
from .mppi import mppi_sample, mppi_update, mppi_solve                  # noqa: F401
from .device_lbfgs import lbfgs_start, lbfgs_tick, lbfgs_solve, lbfgs_state_view, lbfgs_state_fields   # noqa: F401
from .device_auglag import auglag_params, auglag_merit, auglag_outer, auglag_solve, auglag_state_view, auglag_state_fields   # noqa: F401
from .sparse import SparseGPState, SparseDynamics, select_inducing      # noqa: F401
from .particles import GPModel, gp_posterior, particle_noise, particle_step, particle_stats, particle_rollout   # noqa: F401
from .particles import particle_inputs, particle_step_inputs, particle_input_stats   # noqa: F401
from .particles import particle_cost, particle_evaluate, mppi_solve_particles   # noqa: F401
from .linearised import linearised_form, linearised_step, linearised_rollout, mppi_solve_linearised   # noqa: F401
from .linearised import linearised_step_full, linearised_fc_vjp, linearised_fc_constraints, packed_dim, lqr_gain, riccati_gain   # noqa: F401
from .linearised import feedback_input_cost, feedback_input_constraints   # noqa: F401

__all__ = ["GaussianProcessRegression", "Dynamics", "RiskSensitiveMPC", "mean_prop_torch",
           "variance_prop_torch", "covariance_prop_torch", "GPPack", "CostParams", "CostSchedule", "StateConstraints", "InputConstraints", "feedback_input_cost", "feedback_input_constraints", "rollout", "rollout_constraints",
           "rollout_fullcov", "rollout_fullcov_jac", "moment_match", "LinearNominalModel", "mppi_sample", "mppi_update", "mppi_solve", "lbfgs_start", "lbfgs_tick", "lbfgs_solve", "lbfgs_state_view", "lbfgs_state_fields",
           "auglag_params", "auglag_merit", "auglag_outer", "auglag_solve", "auglag_state_view", "auglag_state_fields",
           "SparseGPState", "SparseDynamics", "select_inducing",
           "GPModel", "gp_posterior", "particle_noise", "particle_step", "particle_stats", "particle_rollout", "particle_inputs", "particle_step_inputs", "particle_input_stats",
           "particle_cost", "particle_evaluate", "mppi_solve_particles",
           "linearised_form", "linearised_step", "linearised_rollout", "mppi_solve_linearised",
           "linearised_step_full", "linearised_fc_vjp", "linearised_fc_constraints", "packed_dim", "lqr_gain", "riccati_gain",
           "Simulator", "PendulumPlant", "CartPolePlant", "lib", "require_gpu"]
