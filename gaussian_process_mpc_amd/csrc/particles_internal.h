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
