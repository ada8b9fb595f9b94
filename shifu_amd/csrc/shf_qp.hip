// shf_qp.hip -- the balance controller's foot-force distribution (LeggedRobot.balance_control): per env, which ground-reaction
// forces the stance feet should produce so that the base gets a wanted wrench without slipping, and the joint efforts that
// produce them.  One launch, one thread per env (as k_osc / k_foot_impedance of shf_glue.hip); a translation unit of its own,
// so that no other kernel's machine code moves.
//
// The problem.  F <= 4 feet, world axes with z up, r_f = p_foot_f - p_root, x = (f_1, .., f_F), G = [[I .. I], [[r_1]x .. [r_F]x]]:
//     minimise  1/2 (G x - w)^T S (G x - w) + 1/2 alpha |x|^2 + 1/2 beta |x - f_prev|^2          (S = diag(weights6))
//     stance foot:  fz_min <= f_z <= fz_max,  |f_x| <= mu f_z,  |f_y| <= mu f_z;        swing foot:  f = 0.
// w is given (n, 6), or formed here from shf_sim_floating_dynamics' M and h (order nu = (v, omega, qd)):
//     a_lin = kp_lin (.) (p* - p) + kd_lin (.) (v* - v),   a_ang = kp_ang (.) orientation_error(q*, q) + kd_ang (.) (omega* - omega),
//     w = M[0:6, 0:6] (a_lin, a_ang) + h[0:6]              (orientation_error as in shf_ik_dls; the coupling M[0:6, 6:] qdd is neglected).
//
// The algorithm: ADMM in OSQP form with a fixed number of sweeps -- no data-dependent trip count, every lane of a wave runs the
// same instructions.  The constraint rows, the sweep around the linear solve, the exact clamp and the effort step are
// csrc/shf_cone.h's, which states them; what is this kernel's own is below.  tests/qp_ref.py `twin` is this text in NumPy,
// operation by operation.
//   1. s_f = 1 for a stance foot, 0 for a swing foot.  Column 3 f + k of G is s_f (e_k, r_f x e_k): a swing foot's columns are
//      zero, so it decouples.  be = beta if f_prev is given, else 0.
//   2. P = G^T S G + (alpha + be) I  (P_ij = sum over c = 0..5 of G_ci S_c G_cj, in that order),
//      q = -G^T (S w) - be s_f f_prev.
//   3. m = (sum of P_ii over the stance feet's variables) / (3 max(#stance, 1))  (1 when nothing stands);
//      rho = sqrt((alpha + be) m),  sigma = 1e-6 m.
//   4. The cone's rows and bounds per foot: a stance foot stands, a swing foot does not.
//   5. K = P + sigma I + rho A^T A = L D L^T once (left-looking, in place, 1 / D kept).
//   6. x = z = y = 0; `iters` of the cone's sweeps with xt = K^-1 b by forward substitution, scaling, backward substitution.
//   7. The forces: the cone's exact clamp of x.
//   8. The efforts: the cone's effort step on those forces.
// Measured convergence (tests/test_foot_force_qp_host.py, DESIGN.md 8h "Balance controller").
//
// Storage: the packed factor (1 / D on its diagonal) and q live in LDS, word k of thread t at [k * 64 + t] as k_osc's arrays (a
// thread touches its own words only: no barrier, no bank conflict); x, z, y and the right-hand side in registers -- the kernel
// is instantiated per foot count so that every index is a compile-time constant and nothing lands on the stack.  No
// multiply-add is fused (the arithmetic contract of csrc/shf_device.h), so the float32 twin follows it step by step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"
#include "shf_cone.h"
#include "shf_quat.h"

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns

namespace {

constexpr int QP_T = 64;                       // threads per block: one wavefront
constexpr int QP_MAX_FEET = 4;
constexpr int qp_words(int nf) { return (3 * nf) * (3 * nf + 1) / 2 + 3 * nf; }
static_assert(QP_T * qp_words(QP_MAX_FEET) * 4 <= 48 * 1024, "the factor and q of a block stay within 48 KiB of LDS");

struct QpArgs {
  const float* j; long long j_env, j_foot;
  const float* root; long long root_env;
  const float* foot; long long foot_env, foot_stride;
  const float* wrench;
  const float* mass; const float* dyn_bias; const float* target; const float* gains;
  const unsigned char* stance;
  const float* mu; float mu_scalar;
  const float* weights; float alpha, beta;
  const float* f_prev;
  float fz_min, fz_max;
  int iters;
  const float* bias; const float* limit;
  int n, nd;
  float* forces; float* efforts;
};

template <int NF>
__global__ void __launch_bounds__(QP_T) k_foot_force_qp(QpArgs A) {
  constexpr int N = 3 * NF, T = QP_T;
  extern __shared__ float qp_lds[];
  const int t = threadIdx.x;
  const int e = blockIdx.x * T + t;
  if (e >= A.n) return;
  float* Lw = qp_lds + t;                        // K = L D L^T: L below the diagonal, 1 / D on it, row-packed lower triangle
  float* qw = Lw + (N * (N + 1) / 2) * T;        // q
#define QP_L(i, j) Lw[((i) * ((i) + 1) / 2 + (j)) * T]
  const float* rp = A.root + (long long)e * A.root_env;
  // the wanted wrench
  float w[6];
  if (A.wrench) {
#pragma unroll
    for (int c = 0; c < 6; c++) w[c] = A.wrench[(long long)e * 6 + c];
  } else {
    const float* tg = A.target + (long long)e * 13;
    const long long D = A.nd + 6;
    const float* Mg = A.mass + (long long)e * D * D;
    float a[6], cc[4], qr[4];
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = A.gains[k] * (tg[k] - rp[k]) + A.gains[3 + k] * (tg[7 + k] - rp[7 + k]);
    cc[0] = -rp[3]; cc[1] = -rp[4]; cc[2] = -rp[5]; cc[3] = rp[6];
    const float tq[4] = {tg[3], tg[4], tg[5], tg[6]};
    shf_quat_mul(tq, cc, qr);
    const float sg = qr[3] > 0.0f ? 1.0f : (qr[3] < 0.0f ? -1.0f : 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) a[3 + k] = A.gains[6 + k] * (qr[k] * sg) + A.gains[9 + k] * (tg[10 + k] - rp[10 + k]);
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float acc = Mg[i * D] * a[0];
#pragma unroll
      for (int k = 1; k < 6; k++) acc = acc + Mg[i * D + k] * a[k];
      w[i] = acc + A.dyn_bias[(long long)e * D + i];
    }
  }
  float mu = A.mu ? A.mu[e] : A.mu_scalar;
  mu = fmaxf(mu, 0.0f);
  const float be = A.f_prev ? A.beta : 0.0f;
  const float ab = A.alpha + be;
  float S[6], sw[6], s[NF];
  bool st[NF];
#pragma unroll
  for (int c = 0; c < 6; c++) { S[c] = A.weights[c]; sw[c] = S[c] * w[c]; }
  // 1. G
  float G[6][N];
#pragma unroll
  for (int c = 0; c < 6; c++)
#pragma unroll
    for (int i = 0; i < N; i++) G[c][i] = 0.0f;
#pragma unroll
  for (int f = 0; f < NF; f++) {
    st[f] = A.stance[(long long)e * NF + f] != 0;
    s[f] = st[f] ? 1.0f : 0.0f;
    const float* pf = A.foot + (long long)e * A.foot_env + (long long)f * A.foot_stride;
    const float x = (pf[0] - rp[0]) * s[f], y = (pf[1] - rp[1]) * s[f], z = (pf[2] - rp[2]) * s[f];
#pragma unroll
    for (int k = 0; k < 3; k++) G[k][3 * f + k] = s[f];
    G[3][3 * f + 1] = -z; G[3][3 * f + 2] = y;
    G[4][3 * f + 0] = z;  G[4][3 * f + 2] = -x;
    G[5][3 * f + 0] = -y; G[5][3 * f + 1] = x;
  }
  // 2. P (into the factor's storage) and q; 3. rho and sigma
  float tr = 0.0f, ns = 0.0f, Pd[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float acc = G[0][i] * S[0] * G[0][j];
#pragma unroll
      for (int c = 1; c < 6; c++) acc = acc + G[c][i] * S[c] * G[c][j];
      if (i == j) { acc = acc + ab; Pd[i] = acc; } else QP_L(i, j) = acc;
    }
    float acc = G[0][i] * sw[0];
#pragma unroll
    for (int c = 1; c < 6; c++) acc = acc + G[c][i] * sw[c];
    float qi = -acc;
    if (A.f_prev) qi = qi - be * (A.f_prev[((long long)e * NF + i / 3) * 3 + i % 3] * s[i / 3]);
    qw[i * T] = qi;
    tr = tr + Pd[i] * s[i / 3];
  }
#pragma unroll
  for (int f = 0; f < NF; f++) ns = ns + s[f];
  float mean = tr / (3.0f * fmaxf(ns, 1.0f));
  mean = ns > 0.0f ? mean : 1.0f;
  const float rho = sqrtf(ab * mean), sigma = cone::SIGMA * mean;
  // 5. K = L D L^T in place
  const float dz = 1.0f + 4.0f * (mu * mu);
  float Dg[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    float d = Pd[j] + (sigma + rho * (j % 3 == 2 ? dz : 2.0f));
#pragma unroll
    for (int k = 0; k < j; k++) { const float v = QP_L(j, k); d = d - (v * v) * Dg[k]; }
    Dg[j] = d;
    const float id = 1.0f / d;
    QP_L(j, j) = id;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      float v = QP_L(i, j);
#pragma unroll
      for (int k = 0; k < j; k++) v = v - (QP_L(i, k) * QP_L(j, k)) * Dg[k];
      QP_L(i, j) = v * id;
    }
  }
  // 6. the sweeps
  float x[N], z[NF][5], y[NF][5], lo0[NF], hi0[NF], hic[NF];
#pragma unroll
  for (int i = 0; i < N; i++) x[i] = 0.0f;
#pragma unroll
  for (int f = 0; f < NF; f++) {
    cone::bounds(st[f], A.fz_min, A.fz_max, lo0[f], hi0[f], hic[f]);
#pragma unroll
    for (int m = 0; m < 5; m++) { z[f][m] = 0.0f; y[f][m] = 0.0f; }
  }
  const float irho = 1.0f / rho;
#pragma nounroll
  for (int it = 0; it < A.iters; it++) {
    float b[N];
#pragma unroll
    for (int f = 0; f < NF; f++) {
      float v[5];
      cone::dual(rho, z[f], y[f], v);
      b[3 * f + 0] = (sigma * x[3 * f + 0] - qw[(3 * f + 0) * T]) + cone::at_x(v);
      b[3 * f + 1] = (sigma * x[3 * f + 1] - qw[(3 * f + 1) * T]) + cone::at_y(v);
      b[3 * f + 2] = (sigma * x[3 * f + 2] - qw[(3 * f + 2) * T]) + cone::at_z(mu, v);
    }
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int k = 0; k < i; k++) b[i] = b[i] - QP_L(i, k) * b[k];
#pragma unroll
    for (int i = 0; i < N; i++) b[i] = b[i] * QP_L(i, i);
#pragma unroll
    for (int i = N - 1; i >= 0; i--)
#pragma unroll
      for (int k = i + 1; k < N; k++) b[i] = b[i] - QP_L(k, i) * b[k];
#pragma unroll
    for (int f = 0; f < NF; f++) {
      float zt[5];
      cone::rows(mu, b[3 * f], b[3 * f + 1], b[3 * f + 2], zt);
#pragma unroll
      for (int k = 0; k < 3; k++) x[3 * f + k] = cone::relax(b[3 * f + k], x[3 * f + k]);
      cone::project(rho, irho, zt, lo0[f], hi0[f], hic[f], z[f], y[f]);
    }
  }
  // 7. the forces, exactly feasible
  float fo[NF][3];
#pragma unroll
  for (int f = 0; f < NF; f++) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fo[f][k] = cone::feasible(st[f], k, x[3 * f + k], x[3 * f + 2], mu, A.fz_min, A.fz_max);
      A.forces[((long long)e * NF + f) * 3 + k] = fo[f][k];
    }
  }
  // 8. the efforts
  const int nd = A.nd, D = A.nd + 6;
  for (int d = 0; d < nd; d++) {
    float tau = 0.0f;
#pragma unroll
    for (int f = 0; f < NF; f++) {
      const float* J = A.j + (long long)e * A.j_env + (long long)f * A.j_foot + 6;   // linear rows, dof columns
      tau = tau - cone::effort_term(J, D, d, fo[f][0], fo[f][1], fo[f][2]);
    }
    A.efforts[(long long)e * nd + d] = cone::effort_finish(tau, A.bias, A.limit, e, D, d);
  }
#undef QP_L
}

}  // namespace

extern "C" int shf_foot_force_qp(const float* j_feet, int64_t j_env_stride, int64_t j_foot_stride, const float* root_pose,
                                 int64_t root_env_stride, const float* foot_pos, int64_t foot_env_stride, int64_t foot_stride,
                                 const float* wrench_or_null, const float* mass_matrix_or_null, const float* dyn_bias_or_null,
                                 const float* base_target_or_null, const float* gains12_or_null, const uint8_t* stance,
                                 const float* mu_or_null, float mu_scalar, const float* weights6, float alpha, float beta,
                                 const float* f_prev_or_null, float fz_min, float fz_max, int32_t iters, const float* bias_or_null,
                                 const float* effort_limit_or_null, int32_t n, int32_t num_feet, int32_t num_dof, float* forces_out,
                                 float* efforts_out, void* stream) {
  if (!j_feet || !root_pose || !foot_pos || !stance || !weights6 || !forces_out || !efforts_out) return shf_set_error("shf_foot_force_qp: null tensor");
  if (!wrench_or_null && (!mass_matrix_or_null || !dyn_bias_or_null || !base_target_or_null || !gains12_or_null))
    return shf_set_error("shf_foot_force_qp: null tensor (without a wrench: mass matrix, bias, base target and gains)");
  if (num_feet < 1 || num_feet > QP_MAX_FEET) return shf_set_error("shf_foot_force_qp: 1 to 4 feet");
  if (num_dof < 1) return shf_set_error("shf_foot_force_qp: at least one dof");
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_foot_force_qp: too many dofs");
  if (!(alpha > 0.0f)) return shf_set_error("shf_foot_force_qp: alpha must be positive");
  if (!(beta >= 0.0f)) return shf_set_error("shf_foot_force_qp: beta must not be negative");
  if (!(fz_min <= fz_max)) return shf_set_error("shf_foot_force_qp: fz_min exceeds fz_max");
  if (!mu_or_null && !(mu_scalar >= 0.0f)) return shf_set_error("shf_foot_force_qp: mu must not be negative");
  if (iters < 1) return shf_set_error("shf_foot_force_qp: iters must be at least 1");
  if (n <= 0) return 0;
  QpArgs A = {j_feet, (long long)j_env_stride, (long long)j_foot_stride, root_pose, (long long)root_env_stride, foot_pos,
              (long long)foot_env_stride, (long long)foot_stride, wrench_or_null, mass_matrix_or_null, dyn_bias_or_null,
              base_target_or_null, gains12_or_null, stance, mu_or_null, mu_scalar, weights6, alpha, beta, f_prev_or_null, fz_min,
              fz_max, (int)iters, bias_or_null, effort_limit_or_null, (int)n, (int)num_dof, forces_out, efforts_out};
  const dim3 grid((n + QP_T - 1) / QP_T), block(QP_T);
  const size_t lds = (size_t)QP_T * qp_words(num_feet) * 4;
  hipStream_t s = (hipStream_t)stream;
  switch (num_feet) {
    case 1: hipLaunchKernelGGL(k_foot_force_qp<1>, grid, block, lds, s, A); break;
    case 2: hipLaunchKernelGGL(k_foot_force_qp<2>, grid, block, lds, s, A); break;
    case 3: hipLaunchKernelGGL(k_foot_force_qp<3>, grid, block, lds, s, A); break;
    default: hipLaunchKernelGGL(k_foot_force_qp<4>, grid, block, lds, s, A); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_foot_force_qp: launch failed");
}
