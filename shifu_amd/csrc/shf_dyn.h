// shf_dyn.h -- joint-space dynamics of a fixed-base articulation as tensors: the mass matrix M(q) and the bias forces
// h(q, qd) behind shf_sim_dynamics (gym.acquire_mass_matrix_tensor / refresh_mass_matrix_tensors).  The kernel lives in
// shf_dyn.hip; shf_api.hip owns ShfSim, checks the call and hands the sim's pieces to shf_dyn_launch.
//
// M(q): the composite-rigid-body matrix, M[i][j] = S_i . (Ic_max(i,j) S_j) for dofs on one chain and 0 otherwise, plus
// ShfModel.armature on the diagonal.  h(q, qd): gravity, Coriolis and centrifugal forces -- the joint torques of one
// recursive Newton-Euler sweep with qdd = 0 and the base accelerating at -gravity * gravity_on.  Both use the step kernels'
// own kinematics and rigid inertias (kinematics / body_inertia of shf_device.h, per-env SHF_T_BODY_MASS_SCALE factors
// included), so that M qdd + h = tau is what the backend's forward dynamics integrates in effort mode for a state inside the
// joint limits and without contact.
// NOT part of M or h: joint damping, the drive gains (kp / kd of the position and velocity modes) and the joint-limit
// penalty.  The step applies them implicitly (they enter its D = S^T IA S + armature + dt (damping + ...)); a controller
// that wants them adds them itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shifu_amd.h"

// One launch for n envs at `group` lanes per env (16, 32 or 64; nb <= group), 256 / group envs per block of 256 threads.
// dof (n, nd, 2) and root (n * actors, 13) are the solver's state; mscale (n, nb) or null; mass (n, nd, nd) and bias (n, nd),
// either may be null.  shf_api.hip launches shf_dyn_kernel(group) with shf_dyn_lds_bytes() of dynamic LDS.
struct ShfDynArgs {
  const ShfModel* model;   // on the device
  int32_t n, actors;
  const float* dof;
  const float* root;
  const float* mscale;
  float gravity[3];
  float* mass;
  float* bias;
};
const void* shf_dyn_kernel(int group);
size_t shf_dyn_lds_bytes(const ShfModel& host_model, int group);
