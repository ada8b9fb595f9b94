// shf_cone.h -- the friction-cone ADMM sweep and the effort step the legged controllers share: k_foot_force_qp (shf_qp.hip) and
// k_foot_force_mpc, k_foot_force_efforts (shf_mpc.hip).  Each piece is defined here once; the kernels keep their own linear
// solve (a packed L D L^T per thread there, an explicit inverse per workgroup here) and their own layout of x, z and y.
// tests/cone_ref.py is this text in NumPy, utils/torch_utils.py `_cone_admm` in torch.
//
// The constraint rows of one foot (of one step of the horizon), on its force t = (tx, ty, tz), world axes with z up:
//     A_f = [(0, 0, 1); (-1, 0, mu); (1, 0, mu); (0, -1, mu); (0, 1, mu)],   A_f t = (tz, mu tz - tx, mu tz + tx, mu tz - ty, mu tz + ty),
//     bounds [fz_min, fz_max], [0, inf) x 4 while the foot stands, [0, 0] x 5 while it does not.  A^T A is diagonal: (2, 2, 1 + 4 mu^2).
// ADMM in OSQP form on  minimise 1/2 x^T P x + q^T x,  lo <= A x <= hi,  with K = P + sigma I + rho A^T A, sigma = SIGMA m (m the
// mean diagonal of P over the standing feet's variables), a fixed number of sweeps -- no data-dependent trip count:
//     b = (sigma x - q) + A^T (rho z - y);   xt = K^-1 b  (the kernel's part);   zt = A xt;
//     x = RELAX xt + (1 - RELAX) x;   zr = RELAX zt + (1 - RELAX) z;   z' = clip(zr + y / rho, lo, hi);   y = y + rho (zr - z');   z = z'.
// After the sweeps a foot that does not stand gets +0.0; one that does f_z = clip(x_z, fz_min, fz_max), then f_x, f_y =
// clip(., -mu f_z, mu f_z), so the forces written satisfy every constraint exactly.
// The effort step, from those clamped forces: efforts_d = -sum_f (Jl_f^T f_f)_d over the dof columns (6:) of each foot's linear
// Jacobian rows; + bias[e, 6 + d] when given; the clamp to +-effort_limit[d] last (entries <= 0: no limit), as shf_foot_impedance.
//
// No multiply-add is fused and every sum keeps the association written here (the arithmetic contract of csrc/shf_device.h), so
// the float32 twins follow step by step.  Arrays are passed by reference and indexed by compile-time constants once inlined, so
// nothing lands on the stack.
#pragma once
#include <hip/hip_runtime.h>

namespace cone {

constexpr float RELAX = 1.6f;                    // the over-relaxation of a sweep
constexpr float SIGMA = 1e-6f;                   // sigma over the mean diagonal of P

__device__ __forceinline__ float clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// A_f t
__device__ __forceinline__ void rows(float mu, float tx, float ty, float tz, float (&zt)[5]) {
  const float mz = mu * tz;
  zt[0] = tz; zt[1] = mz - tx; zt[2] = mz + tx; zt[3] = mz - ty; zt[4] = mz + ty;
}

// v = rho z - y
__device__ __forceinline__ void dual(float rho, const float (&z)[5], const float (&y)[5], float (&v)[5]) {
#pragma unroll
  for (int m = 0; m < 5; m++) v[m] = rho * z[m] - y[m];
}

// the components of A_f^T v
__device__ __forceinline__ float at_x(const float (&v)[5]) { return v[2] - v[1]; }
__device__ __forceinline__ float at_y(const float (&v)[5]) { return v[4] - v[3]; }
__device__ __forceinline__ float at_z(float mu, const float (&v)[5]) { return v[0] + mu * (((v[1] + v[2]) + v[3]) + v[4]); }

// the bounds of a foot's rows: [lo0, hi0] on row 0, [0, hic] on rows 1..4
__device__ __forceinline__ void bounds(bool on, float fz_min, float fz_max, float& lo0, float& hi0, float& hic) {
  lo0 = on ? fz_min : 0.0f;
  hi0 = on ? fz_max : 0.0f;
  hic = on ? __builtin_huge_valf() : 0.0f;
}

__device__ __forceinline__ float relax(float xt, float x) { return RELAX * xt + (1.0f - RELAX) * x; }

// zr, z', y over a foot's five rows (irho = 1 / rho)
__device__ __forceinline__ void project(float rho, float irho, const float (&zt)[5], float lo0, float hi0, float hic, float (&z)[5],
                                        float (&y)[5]) {
#pragma unroll
  for (int m = 0; m < 5; m++) {
    const float zr = relax(zt[m], z[m]);
    const float zn = clip(zr + y[m] * irho, m == 0 ? lo0 : 0.0f, m == 0 ? hi0 : hic);
    y[m] = y[m] + rho * (zr - zn);
    z[m] = zn;
  }
}

// component `axis` of the exactly feasible force of a foot whose sweeps ended at (.., v = x_axis, .., xz = x_z)
__device__ __forceinline__ float feasible(bool on, int axis, float v, float xz, float mu, float fz_min, float fz_max) {
  const float fz = clip(xz, fz_min, fz_max);
  const float bnd = mu * fz;
  return on ? (axis == 2 ? fz : clip(v, -bnd, bnd)) : 0.0f;
}

// (Jl_f^T f)_d: J at the foot's block, column 6 (its linear rows' dof columns), D = nd + 6 floats per row
__device__ __forceinline__ float effort_term(const float* J, int D, int d, float fx, float fy, float fz) {
  return (J[d] * fx + J[D + d] * fy) + J[2 * D + d] * fz;
}

// + bias[e, 6 + d], then the clamp
__device__ __forceinline__ float effort_finish(float tau, const float* bias, const float* limit, int e, int D, int d) {
  if (bias) tau += bias[(long long)e * D + 6 + d];
  const float lim = limit ? limit[d] : 0.0f;
  if (lim > 0.0f) tau = tau > lim ? lim : (tau < -lim ? -lim : tau);
  return tau;
}

}  // namespace cone
