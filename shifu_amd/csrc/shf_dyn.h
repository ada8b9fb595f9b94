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

// ---- floating base: shf_sim_floating_dynamics (shf_dyn_fb.hip: k_sim_dynamics_fb, the same launch shape) ----------------
// Generalised velocity nu = (v, w, qd): v the world-axes velocity of the root link's origin and w the root's world angular
// velocity (columns 7:10 and 10:13 of the root-state row), qd the nd dof velocities.  Base columns first, linear before
// angular -- the row order [linear; angular] of the fixed-base Jacobian.  This order is the project's own: the reference never
// reads the base columns.
//   jac  (n, nb, 6, nd + 6): body b's rows are [velocity of b's origin; angular velocity of b] = J_b nu in world axes.  Base
//        columns [[I, -[r_b]x], [0, I]] with r_b = p_b - p_root; dof columns as the fixed-base writer forms them, for every
//        moving ancestor (a welded body gets its parent chain's columns at its own origin); body 0's block is [I6 | 0];
//        entries off a body's chain are exact zeros.  One writer per entry.
//   mass (n, nd + 6, nd + 6): the composite-rigid-body matrix in that order.  Base block = the whole robot's composite inertia
//        about the root origin, [[m I, -m [c]x], [m [c]x, I_o]]; coupling rows / columns F_d = Ic S_d (permuted from the kernel's
//        angular-first spatial order); dof block as k_sim_dynamics', armature on the dof diagonal only.  Every off-diagonal
//        value is stored twice from one register: bit-symmetric.
//   bias (n, nd + 6): the generalised forces of one Newton-Euler sweep with nu_dot = 0 -- the CLASSICAL acceleration of the
//        root origin, the root's angular acceleration and qdd all zero, gravity * gravity_on acting.  Rows 0:3 / 3:6: the net
//        force and the moment about the root origin.  The kernel's spatial acceleration of the root is therefore
//        (0, -w x v - g): spatial and classical linear acceleration of a moving reference point differ by w x v.
// With these, M nu_dot + h = (external wrench on the root about its origin, tau) + sum J_c^T f_c.  Left out as above: joint
// damping, drive gains, the joint-limit penalty.
struct ShfDynFbArgs {
  ShfDynArgs d;   // mass (n, nd+6, nd+6), bias (n, nd+6); either may be null
  float* jac;     // (n, nb, 6, nd+6) or null
};
const void* shf_dyn_fb_kernel(int group);
size_t shf_dyn_fb_lds_bytes(const ShfModel& host_model, int group);
