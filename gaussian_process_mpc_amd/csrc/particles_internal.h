// What particle_cost.hip needs of particles.hip besides the public entries and the model frame (model_frame.h): the model check of every
// particle entry with its noise model, the (B, P) check and the initial draw.  Host only.
#pragma once
#include "gpmpc_internal.h"

// GPMPC_OK, or GPMPC_E_ARG with the text gpmpc_particle_rollout gives for this model (sizes, pointers, hyper-parameters, nominal and noise
// model).  No device work.
int gpmpc_pt_check_model(const char* who, const gpmpc_gp_model* m);
// B, P >= 1 and B P within one array, as gpmpc_particle_step checks them
int gpmpc_pt_check_bp(const char* who, int B, int P);
// out[b P + p] = x0[b] + L eps[p] (k_pt_init), L from the model's init_cov: the step-0 particles of gpmpc_particle_rollout, bit for bit.
// eps dev [P][ds] = gpmpc_particle_noise(P, ds, 0, ...).  The model is taken as checked.
int gpmpc_pt_initial(const gpmpc_gp_model* m, int B, int P, const double* x0, const double* eps, double* out, hipStream_t s);

// Particles under a linear state feedback u^p = v_b + K_t (x^p - mu_b): the launches of linprop_inputs.hip that particles.hip's entries
// (gpmpc_particle_step_inputs, gpmpc_particle_rollout_feedback) enqueue, checked by their callers.
//   inputs     out_u [B P][da] from x_prev [B P][ds], U_t + b u_stride, K_t [da][ds] or null (a copy of v_b), mu_t + b mu_stride
//   assemble   k_pt_assemble with an input per particle: z = (x_prev, U_p + action_sd eps_u); action_sd host [da]
//   stats      gpmpc_particle_input_stats' kernels on inputs [H][B P][da]
int gpmpc_lpi_particle_inputs(int B, int P, int ds, int da, const double* x_prev, const double* U_t, size_t u_stride, const double* K_t,
                              const double* mu_t, size_t mu_stride, double* out_u, hipStream_t s);
int gpmpc_lpi_assemble(int B, int P, int ds, int da, const double* x_prev, const double* U_p, const double* eps, const double* action_sd,
                       double* z, hipStream_t s);
int gpmpc_lpi_input_stats(int B, int P, int H, int da, const double* inputs, const gpmpc_input_constraints* ucons, double* out_umean,
                          double* out_ucov, double* out_uviol, double* out_ujoint, hipStream_t s);
int gpmpc_lpi_check_rows(const char* who, const gpmpc_input_constraints* C);
