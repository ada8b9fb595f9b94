// shf_dyn.hip -- k_sim_dynamics: mass matrix and bias forces of a fixed-base articulation, one launch for every env
// (definitions and what they leave out: shf_dyn.h).  The floating-base form, k_sim_dynamics_fb, is shf_dyn_fb.hip: a unit of
// its own, so that this one compiles to the machine code it had.
//
// Layout: k_body_state's -- the model staged in LDS, one EnvLds per env, one lane per body, `G` lanes per env, 256 / G envs
// per block.  Per env:
//   1. kinematics + body_inertia: world pose, motion subspace S, velocity v, velocity-product acceleration c, rigid inertia
//      IA and bias force pA = v x* IA v of every body (world axes, about the root's origin);
//   2. outward by level: a_b = a_parent + c_b from a_root = (0, -g)   (qdd = 0), then f_b = IA_b a_b + pA_b;
//   3. inward by level through LDS: composite inertia and force, children added in child_list order (no atomics: the
//      result does not depend on lane timing);
//   4. the lane of dof d's body: F = Ic S_d, h[d] = S_d . f, M[d][d] = S_d . F + armature[d], and for every moving ancestor a
//      M[d][dof[a]] = M[dof[a]][d] = S_a . F (one value stored twice: exactly symmetric).  An ancestor's dof index is below
//      its descendants' (model.py numbers bodies parent first), so lane d owns row d left of the diagonal and column d above
//      it, writes zeros there first and the ancestor entries over them: every entry has one writer.
#include <hip/hip_runtime.h>

#include "shf_device.h"
#include "shf_kernels.h"
#include "shf_dyn.h"

template <int G>
__global__ __launch_bounds__(256) void k_sim_dynamics(ShfDynArgs A) {
  const ShfModel* gm = A.model;
  const int n = A.n, actors = A.actors;
  const float *dof = A.dof, *root = A.root, *mscale = A.mscale;
  const float gx = A.gravity[0], gy = A.gravity[1], gz = A.gravity[2];
  float *mass = A.mass, *bias = A.bias;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const ShfModel* m = stage_model(gm, smem);
  const int epb = 256 / G, es = threadIdx.x / G, l = threadIdx.x % G;
  const int e = blockIdx.x * epb + es;
  if (e >= n) return;
  const int nb = m->nb, nd = m->nd, np = m->np;
  EnvLds L = env_lds_carve(smem + MODEL_WORDS + es * env_lds_words(nb, nd, np), nb, nd, np);
  for (int i = l; i < 2 * nd; i += G) L.dofb[(i >> 1) * DOF_STRIDE + (i & 1)] = dof[(size_t)e * nd * 2 + i];
  for (int i = l; i < 13; i += G) L.root[i] = root[(size_t)e * actors * 13 + i];   // the articulation's own row
  GROUP_SYNC();

  BodyRegs B;
  LaneModel M;
  lane_model_load<DynDims>(m, l, M);
  kinematics<G>(m, L, l, M, B);
  const bool isdyn = M.isdyn, moving = M.moving;
  const int mylevel = M.level(), nl = m->nlevels;
  if (isdyn) body_inertia(M, B, mscale ? mscale + (size_t)e * nb : nullptr, l);

  // the pose slots have served (kinematics ends on a sync): a moving body's slot now carries its S for its descendants
  if (moving) {
    float* o = L.pose + l * POSE_STRIDE;
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = B.S[k];
  }
  // outward: accelerations with qdd = 0
  const float gon = (float)m->gravity_on;
  float a[6] = {0.0f, 0.0f, 0.0f, -(gx * gon), -(gy * gon), -(gz * gon)};
  if (l == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) L.acc[k] = a[k];
  }
  for (int lev = 1; lev <= nl; lev++) {
    GROUP_SYNC();
    if (moving && mylevel == lev) {
      const float* pa = L.acc + M.dynpar() * 6;
#pragma unroll
      for (int i = 0; i < 6; i++) { a[i] = pa[i] + B.c[i]; L.acc[l * 6 + i] = a[i]; }
    }
  }
  if (moving) {
    float f[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float acc = SYMG(B.IA, i, 0) * a[0];
#pragma unroll
      for (int j = 1; j < 6; j++) acc = fmaf(SYMG(B.IA, i, j), a[j], acc);
      f[i] = B.pA[i] + acc;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) B.pA[k] = f[k];
  }
  // inward: composite inertia and force, children in child_list order
  for (int lev = nl; lev >= 1; lev--) {
    if (moving && mylevel == lev) {
      float* o = L.xch + l * XCH_STRIDE;
#pragma unroll
      for (int k = 0; k < 21; k++) o[k] = B.IA[k];
#pragma unroll
      for (int k = 0; k < 6; k++) o[21 + k] = B.pA[k];
    }
    GROUP_SYNC();
    if (moving && mylevel == lev - 1) {
      for (int kk = 0; kk < M.nchild; kk++) {
        const float* o = L.xch + m->child_list[M.child0 + kk] * XCH_STRIDE;
#pragma unroll
        for (int k = 0; k < 21; k++) B.IA[k] += o[k];
#pragma unroll
        for (int k = 0; k < 6; k++) B.pA[k] += o[21 + k];
      }
    }
  }
  GROUP_SYNC();   // (nl = 0: the S slots above)
  if (!moving) return;

  const int d = M.dofi();
  float F[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float acc = SYMG(B.IA, i, 0) * B.S[0];
#pragma unroll
    for (int j = 1; j < 6; j++) acc = fmaf(SYMG(B.IA, i, j), B.S[j], acc);
    F[i] = acc;
  }
  if (bias) {
    float h = B.S[0] * B.pA[0];
#pragma unroll
    for (int k = 1; k < 6; k++) h = fmaf(B.S[k], B.pA[k], h);
    bias[(size_t)e * nd + d] = h;
  }
  if (mass) {
    float* out = mass + (size_t)e * nd * nd;
    for (int j = 0; j < d; j++) { out[d * nd + j] = 0.0f; out[j * nd + d] = 0.0f; }
    float dd = B.S[0] * F[0];
#pragma unroll
    for (int k = 1; k < 6; k++) dd = fmaf(B.S[k], F[k], dd);
    out[d * nd + d] = dd + m->armature[d];
    for (int x = M.dynpar(); x != 0; x = m->dyn[m->parent[x]]) {
      const float* Sa = L.pose + x * POSE_STRIDE;
      float v = Sa[0] * F[0];
#pragma unroll
      for (int k = 1; k < 6; k++) v = fmaf(Sa[k], F[k], v);
      const int ja = m->dof[x];
      out[d * nd + ja] = v;
      out[ja * nd + d] = v;
    }
  }
}

const void* shf_dyn_kernel(int group) {
  switch (group) {
    case 64: return reinterpret_cast<const void*>(&k_sim_dynamics<64>);
    case 32: return reinterpret_cast<const void*>(&k_sim_dynamics<32>);
    default: return reinterpret_cast<const void*>(&k_sim_dynamics<16>);
  }
}
size_t shf_dyn_lds_bytes(const ShfModel& hm, int group) {
  return ((size_t)MODEL_WORDS + (size_t)(256 / group) * env_lds_words(hm.nb, hm.nd, hm.np)) * 4;
}
