// shf_dyn_fb.hip -- k_sim_dynamics_fb: Jacobian, mass matrix and bias forces of a floating-base articulation, one launch for
// every env (conventions: shf_dyn.h).  k_sim_dynamics' layout (shf_dyn.hip) and passes; a translation unit of its own because
// the compiler's code for k_sim_dynamics changes when the two share one.
#include <hip/hip_runtime.h>

#include "shf_device.h"
#include "shf_kernels.h"
#include "shf_dyn.h"

// k_sim_dynamics_fb: the floating-base form (conventions: shf_dyn.h).  The same layout and passes with the root taking part:
//   * the root's six columns are the identity in the kernel's spatial coordinates (angular first, about the root's origin),
//     so its composite inertia IS the base block and a dof's F = Ic S_d the coupling column; FB_SP permutes to the tensors'
//     linear-first order;
//   * outward from a_root = (0, -w x v - g): nu_dot = 0 means a zero CLASSICAL acceleration of the root origin, and the
//     spatial linear acceleration of a moving reference point is the classical one minus w x v; the root's own
//     v x* IA v (body_inertia computes it from the root's twist) enters its force;
//   * inward up to the root (level 0), children in child_list order;
//   * the root's lane writes the 6x6 base block and h[0:6]; the lane of dof d row / column 6 + d as k_sim_dynamics does plus
//     its six coupling entries; body b's lane (welded bodies included) forms its own (6, nd + 6) Jacobian block: every entry
//     has one writer.  The Jacobian needs the kinematics only and is written before the inertia passes, which a launch
//     without mass and bias skips (the values do not depend on which outputs are asked for).
#define FB_SP(i) ((i) < 3 ? (i) + 3 : (i) - 3)
template <int G>
__global__ __launch_bounds__(256) void k_sim_dynamics_fb(ShfDynFbArgs AF) {
  const ShfModel* gm = AF.d.model;
  const int n = AF.d.n, actors = AF.d.actors;
  const float *dof = AF.d.dof, *root = AF.d.root, *mscale = AF.d.mscale;
  const float g3[3] = {AF.d.gravity[0], AF.d.gravity[1], AF.d.gravity[2]};
  float *mass = AF.d.mass, *bias = AF.d.bias, *jac = AF.jac;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const ShfModel* m = stage_model(gm, smem);
  const int epb = 256 / G, es = threadIdx.x / G, l = threadIdx.x % G;
  const int e = blockIdx.x * epb + es;
  if (e >= n) return;
  const int nb = m->nb, nd = m->nd, np = m->np, D = nd + 6;
  EnvLds L = env_lds_carve(smem + MODEL_WORDS + es * env_lds_words(nb, nd, np, nb * D), nb, nd, np);
  for (int i = l; i < 2 * nd; i += G) L.dofb[(i >> 1) * DOF_STRIDE + (i & 1)] = dof[(size_t)e * nd * 2 + i];
  for (int i = l; i < 13; i += G) L.root[i] = root[(size_t)e * actors * 13 + i];   // the articulation's own row
  GROUP_SYNC();

  BodyRegs B;
  LaneModel M;
  lane_model_load<DynDims>(m, l, M);
  kinematics<G>(m, L, l, M, B);
  const bool isdyn = M.isdyn, moving = M.moving;
  const int mylevel = M.level(), nl = m->nlevels;

  // the pose slots have served (kinematics ends on a sync): a moving body's slot now carries its S for its descendants
  if (moving) {
    float* o = L.pose + l * POSE_STRIDE;
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = B.S[k];
  }
  GROUP_SYNC();
  if (jac) {
    // Every body's lane forms its block one row at a time in the env's staging area (L.pt, nb * D words: asked for as the LDS
    // tail), and the group stores that row of all bodies together -- runs of D consecutive words, not one word per lane and
    // 6 * D words apart.  Zeros first, the chain's entries over them, as the mass matrix does; each entry is stored once.
    float* Je = jac + (size_t)e * nb * 6 * D;
    float* st = L.pt + l * D;
    // base columns [[I, -[r]x], [0, I]], r = this body's origin from the root's (0 - r: +0 for the root itself)
    const float r0 = B.p[0], r1 = B.p[1], r2 = B.p[2];
    const float base[6][6] = {{1.0f, 0.0f, 0.0f, 0.0f, r2, 0.0f - r1},
                              {0.0f, 1.0f, 0.0f, 0.0f - r2, 0.0f, r0},
                              {0.0f, 0.0f, 1.0f, r1, 0.0f - r0, 0.0f},
                              {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f},
                              {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f},
                              {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f}};
#pragma unroll
    for (int k = 0; k < 6; k++) {
      if (M.isbody) {
#pragma unroll
        for (int j = 0; j < 6; j++) st[j] = base[k][j];
        for (int d = 0; d < nd; d++) st[6 + d] = 0.0f;
        for (int b = l; b > 0; b = m->parent[b]) {
          const int d = m->dof[b];
          if (d < 0) continue;
          const float* S = L.pose + b * POSE_STRIDE;
          if (k < 3) {
            const float ax[3] = {S[0], S[1], S[2]};
            float t[3];
            cross3(ax, B.p, t);
            st[6 + d] = t[k] + S[3 + k];
          } else {
            st[6 + d] = S[k - 3];
          }
        }
      }
      GROUP_SYNC();
      for (int i = l; i < nb * D; i += G) {
        const int b = i / D;
        Je[(b * 6 + k) * D + (i - b * D)] = L.pt[i];
      }
      GROUP_SYNC();
    }
  }
  if (!mass && !bias) return;

  if (isdyn) body_inertia(M, B, mscale ? mscale + (size_t)e * nb : nullptr, l);
  // outward: accelerations with nu_dot = 0
  const float gon = (float)m->gravity_on;
  float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (l == 0) {
    float wv[3];
    cross3(B.v, B.v + 3, wv);
#pragma unroll
    for (int k = 0; k < 3; k++) a[3 + k] = (0.0f - wv[k]) - g3[k] * gon;
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
  if (isdyn) {
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
  // inward: composite inertia and force up to the root, children in child_list order
  for (int lev = nl; lev >= 1; lev--) {
    if (moving && mylevel == lev) {
      float* o = L.xch + l * XCH_STRIDE;
#pragma unroll
      for (int k = 0; k < 21; k++) o[k] = B.IA[k];
#pragma unroll
      for (int k = 0; k < 6; k++) o[21 + k] = B.pA[k];
    }
    GROUP_SYNC();
    if (isdyn && mylevel == lev - 1) {
      for (int kk = 0; kk < M.nchild; kk++) {
        const float* o = L.xch + m->child_list[M.child0 + kk] * XCH_STRIDE;
#pragma unroll
        for (int k = 0; k < 21; k++) B.IA[k] += o[k];
#pragma unroll
        for (int k = 0; k < 6; k++) B.pA[k] += o[21 + k];
      }
    }
  }
  if (!isdyn) return;

  if (l == 0) {   // the whole robot's composite inertia and net force about the root origin
    if (bias) {
#pragma unroll
      for (int i = 0; i < 6; i++) bias[(size_t)e * D + i] = B.pA[FB_SP(i)];
    }
    if (mass) {
      float* out = mass + (size_t)e * D * D;
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) out[i * D + j] = SYMG(B.IA, FB_SP(i), FB_SP(j));
    }
    return;
  }
  const int d = M.dofi(), r = 6 + d;
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
    bias[(size_t)e * D + r] = h;
  }
  if (mass) {
    float* out = mass + (size_t)e * D * D;
#pragma unroll
    for (int i = 0; i < 6; i++) { const float v = F[FB_SP(i)]; out[i * D + r] = v; out[r * D + i] = v; }
    for (int j = 6; j < r; j++) { out[r * D + j] = 0.0f; out[j * D + r] = 0.0f; }
    float dd = B.S[0] * F[0];
#pragma unroll
    for (int k = 1; k < 6; k++) dd = fmaf(B.S[k], F[k], dd);
    out[r * D + r] = dd + m->armature[d];
    for (int x = M.dynpar(); x != 0; x = m->dyn[m->parent[x]]) {
      const float* Sa = L.pose + x * POSE_STRIDE;
      float v = Sa[0] * F[0];
#pragma unroll
      for (int k = 1; k < 6; k++) v = fmaf(Sa[k], F[k], v);
      const int ja = 6 + m->dof[x];
      out[r * D + ja] = v;
      out[ja * D + r] = v;
    }
  }
}
#undef FB_SP

const void* shf_dyn_fb_kernel(int group) {
  switch (group) {
    case 64: return reinterpret_cast<const void*>(&k_sim_dynamics_fb<64>);
    case 32: return reinterpret_cast<const void*>(&k_sim_dynamics_fb<32>);
    default: return reinterpret_cast<const void*>(&k_sim_dynamics_fb<16>);
  }
}

size_t shf_dyn_fb_lds_bytes(const ShfModel& hm, int group) {   // the tail holds one Jacobian row of every body
  return ((size_t)MODEL_WORDS + (size_t)(256 / group) * env_lds_words(hm.nb, hm.nd, hm.np, hm.nb * (hm.nd + 6))) * 4;
}
