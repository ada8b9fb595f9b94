// shf_mpc.hip -- the horizon form of the legged controller's stance half (LeggedRobot.locomotion_control(controller="mpc")):
// the convex MPC of Di Carlo et al. (2018) on the base equation shf_foot_force_qp solves for one instant, M6 nu' + h6 = G f,
// rolled over the integer gait schedule.  Three kernels: k_mpc_horizon (one thread per env) lays the schedule, the base
// reference and the footholds out over the horizon; k_foot_force_mpc (one workgroup per env) condenses and solves; and
// k_foot_force_efforts (one thread per env) is the effort step on its own, for the ticks between two solves.  A translation
// unit of its own, so that no other kernel's machine code moves.
//
// The problem, per env.  x = (Theta, p, omega, v), 12 entries, world axes with z up: Theta = (roll, pitch, yaw), the ZYX angles
// of the root quaternion, the yaw unwrapped to within pi of the reference's yaw at step 0; p the root origin; omega, v the
// root's angular and linear velocity.  H steps (1..SHF_MPC_MAX_HORIZON) of delta seconds, F <= 4 feet, unknowns u_{k,f} in R^3
// (variable i = (k F + f) 3 + c, N = 3 F H <= 120).  M6 = M[0:6, 0:6], h6 = h[0:6] of shf_sim_floating_dynamics (order:
// linear, angular), c_{k,f} the contact table:
//     (v', omega')_k = M6^-1 (sum_f c_{k,f} (u_{k,f}; r_{k,f} x u_{k,f}) - h6),   r_{k,f} = pos_{k,f} - (p_root + (p_ref,k - p_ref,0)),
//     Theta_{k+1} = Theta_k + delta Rz(psi_ref,k)^T omega_k,   p_{k+1} = p_k + delta v_k,   (v, omega)_{k+1} = (v, omega)_k + delta (v', omega')_k,
//     minimise  1/2 sum_{k=1..H} (x_k - xref_k)^T diag(weights12) (x_k - xref_k) + 1/2 alpha sum |u_{k,f}|^2,
//     c_{k,f} = 1:  fz_min <= u_z <= fz_max, |u_x| <= mu u_z, |u_y| <= mu u_z;      c_{k,f} = 0:  u_{k,f} = 0.
// What is approximated: M6 and h6 are frozen over the horizon (the legs' motion and the base's rotation do not change them);
// the lever arms r_{k,f} are taken about the reference path, not the predicted one, so that x stays linear in u; Theta' =
// Rz(psi_ref)^T omega holds for small roll and pitch only; and, as in shf_foot_force_qp, the coupling M[0:6, 6:] qdd of the
// dof accelerations is neglected.
//
// k_mpc_horizon.  tests/mpc_ref.py `horizon` is this text in NumPy.  It runs after shf_gait_plan on the same GaitState: the
// stored tick has then ALREADY been advanced, so this tick's clock is tick - 1, and step k of the horizon starts at gait tick
// (tick - 1) + k S (S >= 1 gait ticks per step, delta = S dt).
//   contact (n, H, F) uint8: row 0 is this tick's stance (scheduled and touching: shf_gait_plan's stance_out); row k >= 1 is
//     ((tick - 1) + k S + offset_f) mod P < stance_ticks_f.  Integers only.
//   xref (n, H + 1, 12): row k = (0, 0, yaw + k delta target.omega_z;  target.p.xy + k delta target.v.xy, target.z;  target.omega;
//     target.v) -- the base target rolled forward; row 0 is "now".
//   pos (n, H, F, 3) world: a contact run that includes step 0 keeps foot_pos; a run that starts at step k > 0 gets, for all
//     of its steps, with psi = xref_k.yaw, (cs, sn) = (cos, sin)(psi), (vx, vy, wz) the command and (n_fx, n_fy) the nominal:
//       n_w = (cs n_fx - sn n_fy, sn n_fx + cs n_fy);  hip = xref_k.p.xy + n_w;
//       v_des = ((cs vx - sn vy) - wz n_w.y, (sn vx + cs vy) + wz n_w.x);  g = v_des ((stance_ticks_f dt) / 2);
//       m = sqrt(g_x^2 + g_y^2);  if m > max_step: g = g (max_step / m);  pos = (hip + g, touchdown_z)
//     -- shf_gait_plan's foothold without the velocity feedback, because the prediction rides the reference.  Entries with
//     contact = 0 are +0.0.
//
// k_foot_force_mpc.  tests/mpc_ref.py `twin` is this text in NumPy, operation by operation.  L = weights12 = (L_Theta, L_p,
// L_omega, L_v); k_i, f_i, c_i the step, foot and axis of variable i; "invert" is the in-place Gauss-Jordan sweep without
// pivoting (for k = 0..: p = 1 / a_kk, row = a_k. p, every other row a_i. = a_i. - a_ik row with a_ik = -(a_ik p); a_k. = row
// with a_kk = p), sound for the symmetric positive definite matrices it meets here.
//   1. Minv = invert(M6);  g = -(Minv h6)  (rows 0..2 the linear, 3..5 the angular acceleration without foot forces).
//   2. Free response and tables (one thread): x = x_0; C_0 = S_0 = 0; for s = 0..H-1, psi = xref_s.yaw:
//        Theta = Theta + delta (cos psi omega_x + sin psi omega_y, cos psi omega_y - sin psi omega_x, omega_z);  p = p + delta v;
//        omega = omega + delta g[3:6];  v = v + delta g[0:3]  (after their use);  C_{s+1} = C_s + cos psi,  S_{s+1} = S_s + sin psi;
//        E_{s+1} = x - xref_{s+1}.
//   3. Per variable i, with e_c the axis and r = r_{k,f}:  ang = r x e_c;
//        W_i[r'] = (delta (Minv[r'][c] + ((Minv[r'][3] ang_0 + Minv[r'][4] ang_1) + Minv[r'][5] ang_2))) c_{k,f},  r' = 0..5
//        (what one newton along e_c at step k adds to (v, omega) of the later steps; zero for a foot in the air, so that it
//        decouples);  for s = k + 2..H:  a = C_s - C_{k+1}, b = S_s - S_{k+1},
//        TX_i[s] = a W_i[3] + b W_i[4],  TY_i[s] = a W_i[4] - b W_i[3]   (0 for s <= k + 1).
//      The blocks of B follow in closed form: for s > k, n = s - 1 - k, the column of variable i in the rows of step s is
//        (delta TX_i[s], delta TY_i[s], delta n W_i[5];  delta n W_i[0:3];  W_i[3:6];  W_i[0:3]).
//   4. P = B^T L B + alpha I, q = B^T L E, as sums that never form B.  With m = max(k_i, k_j), S0 = H - m,
//      S2 = sum_{s=m+1..H} (s - 1 - k_i)(s - 1 - k_j) (integers):
//        dv = (W_i[0] L_9 W_j[0] + W_i[1] L_10 W_j[1]) + W_i[2] L_11 W_j[2];  dw likewise on rows 3..5 with L_6..8;
//        dp likewise on rows 0..2 with L_3..5;  dz = W_i[5] L_2 W_j[5];
//        th = sum_{s=m+1..H} ((L_0 TX_i[s]) TX_j[s] + (L_1 TY_i[s]) TY_j[s])   (in that order of s);
//        P_ij = (S0 (dw + dv) + (delta^2 S2) (dp + dz)) + delta^2 th,  + alpha on the diagonal;
//        q_i = sum_{s=k_i+1..H}, n = s - 1 - k_i, of
//              (delta (((L_0 TX_i[s]) E_s[0] + (L_1 TY_i[s]) E_s[1]) + n ((W_i[5] L_2) E_s[2]))
//               + (delta n) (((W_i[0] L_3) E_s[3] + (W_i[1] L_4) E_s[4]) + (W_i[2] L_5) E_s[5]))
//              + ((((W_i[3] L_6) E_s[6] + (W_i[4] L_7) E_s[7]) + (W_i[5] L_8) E_s[8])
//                 + (((W_i[0] L_9) E_s[9] + (W_i[1] L_10) E_s[10]) + (W_i[2] L_11) E_s[11])).
//   5. m = (sum of P_ii over the contact variables, i ascending) / max(their number, 1)  (1 when nothing ever stands);
//      rho = sqrt(alpha m),  sigma = 1e-6 m.
//   6. The cone's rows and bounds (csrc/shf_cone.h, which states them and the sweep) per (k, f): a foot stands where c_{k,f} = 1.
//      Kinv = invert(P + (sigma + rho A^T A) on the diagonal), once.
//   7. x = u_io shifted by warm_shift steps (row min(k + warm_shift, H - 1); 0 without contact), or 0; z = A x; y = 0.
//      `iters` of the cone's sweeps with
//        xt_i = (a_0 + a_1) + (a_2 + a_3),  a_l = sum over j = l, l + 4, .. of Kinv_ij b_j  (four running sums, j ascending).
//   8. Every (k, f): the cone's exact clamp of x.  These go back to u_io; step 0 is forces_out, which therefore satisfies every
//      inequality exactly.
//   9. The efforts: the cone's effort step on forces_out -- the same functions k_foot_force_qp and k_foot_force_efforts call.
//
// The mapping.  An env's system is 120 x 120: too large for a thread's registers, too small for a CU, so a workgroup of one
// wavefront (N <= 64) or two solves one env, thread i owning variable i and row i of P, K and Kinv.  Kinv stays in LDS (57.6
// KB at N = 120; two workgroups per CU), stored so that thread i reads four consecutive columns of its row as one 16-byte
// word and neighbouring threads read neighbouring words (element (i, j) at ((j / 4) N4 + i) 4 + j mod 4: ds_read_b128 without
// bank conflicts), the right-hand side as broadcast 16-byte words.  The explicit inverse is preferred to a triangular
// factor: a sweep is then one matrix-vector product whose 120 terms are independent, where two triangular solves are 240
// dependent steps with a barrier each.  The z and y of a foot's five rows are kept redundantly by its three threads, so a
// sweep needs two barriers (b written / xt written) and no reduction.  No multiply-add is fused (the arithmetic contract of
// csrc/shf_device.h); every per-thread array is indexed by compile-time constants, so nothing lands on the stack.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>

#include "../../include/shifu_amd.h"
#include "shf_cone.h"

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns

namespace {

constexpr int MPC_T = 64;                      // threads per block of the per-env kernels: one wavefront
constexpr int MPC_MAX_FEET = 4;
constexpr int MPC_MAX_H = SHF_MPC_MAX_HORIZON;
constexpr int MPC_MAX_N = 3 * MPC_MAX_FEET * MPC_MAX_H;

// floats of LDS one env's solve takes: Kinv, five vectors (b, pivot row, xt, diagonal, contact flags), W, TX, TY, E, C, S, the forces
constexpr int mpc_lds_floats(int N4, int H) { return N4 * N4 + 5 * N4 + 6 * N4 + 2 * H * N4 + 12 * H + 2 * (H + 1) + 3 * MPC_MAX_FEET; }
static_assert(mpc_lds_floats(MPC_MAX_N, MPC_MAX_H) * 4 <= 80 * 1024, "two envs' solves fit the 160 KiB of a CU");

// ------------------------------------------------------------------------------------------------------ the horizon --
struct HorizonArgs {
  const int* tick; const float* target; const float* yaw;
  int period; int offset[MPC_MAX_FEET]; int stance_ticks[MPC_MAX_FEET];
  const unsigned char* stance;
  const float* foot; long long foot_env, foot_stride;
  const float* command; const float* nominal;
  ShfGaitParams P;
  int H, S, n, nf;
  unsigned char* contact; float* xref; float* pos;
};

__global__ void __launch_bounds__(MPC_T) k_mpc_horizon(HorizonArgs A) {
  const int e = blockIdx.x * MPC_T + threadIdx.x;
  if (e >= A.n) return;
  const int F = A.nf, P = A.period, H = A.H;
  const float* tg = A.target + (long long)e * 13;
  const float yaw0 = A.yaw[e];
  const float dt = A.P.dt;
  const float delta = (float)A.S * dt;
  const float tx = tg[0], ty = tg[1], tz = tg[2], vwx = tg[7], vwy = tg[8], vwz = tg[9], ox = tg[10], oy = tg[11], oz = tg[12];
  const float cvx = A.command[(long long)e * 3], cvy = A.command[(long long)e * 3 + 1], cwz = A.command[(long long)e * 3 + 2];
  for (int k = 0; k <= H; k++) {
    const float kd = (float)k * delta;
    float* xr = A.xref + ((long long)e * (H + 1) + k) * 12;
    xr[0] = 0.0f; xr[1] = 0.0f; xr[2] = yaw0 + kd * oz;
    xr[3] = tx + kd * vwx; xr[4] = ty + kd * vwy; xr[5] = tz;
    xr[6] = ox; xr[7] = oy; xr[8] = oz;
    xr[9] = vwx; xr[10] = vwy; xr[11] = vwz;
  }
  int tm = (A.tick[e] - 1) % P;                  // shf_gait_plan has advanced the stored tick already
  tm = tm < 0 ? tm + P : tm;
#pragma unroll
  for (int f = 0; f < MPC_MAX_FEET; f++) {
    if (f < F) {
      const int st = A.stance_ticks[f], off = A.offset[f];
      const float nfx = A.nominal[3 * f], nfy = A.nominal[3 * f + 1];
      const float* pf = A.foot + (long long)e * A.foot_env + (long long)f * A.foot_stride;
      bool prev = false;
      float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
      for (int k = 0; k < H; k++) {
        const int phi = (tm + (int)(((long long)k * A.S) % P) + off) % P;
        const bool c = k == 0 ? A.stance[(long long)e * F + f] != 0 : phi < st;
        if (c && k == 0) { h0 = pf[0]; h1 = pf[1]; h2 = pf[2]; }
        if (c && k > 0 && !prev) {
          const float kd = (float)k * delta;
          const float psi = yaw0 + kd * oz;
          const float cs = cosf(psi), sn = sinf(psi);
          const float nwx = cs * nfx - sn * nfy, nwy = sn * nfx + cs * nfy;
          const float hx = (tx + kd * vwx) + nwx, hy = (ty + kd * vwy) + nwy;
          const float vdx = (cs * cvx - sn * cvy) - cwz * nwy, vdy = (sn * cvx + cs * cvy) + cwz * nwx;
          const float half = ((float)st * dt) * 0.5f;
          float gx = vdx * half, gy = vdy * half;
          const float m = sqrtf(gx * gx + gy * gy);
          if (m > A.P.max_step) {
            const float q = A.P.max_step / m;
            gx = gx * q; gy = gy * q;
          }
          h0 = hx + gx; h1 = hy + gy; h2 = A.P.touchdown_z;
        }
        const long long o = ((long long)e * H + k) * F + f;
        A.contact[o] = c ? 1 : 0;
        A.pos[o * 3 + 0] = c ? h0 : 0.0f; A.pos[o * 3 + 1] = c ? h1 : 0.0f; A.pos[o * 3 + 2] = c ? h2 : 0.0f;
        prev = c;
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------- the solve --
struct MpcArgs {
  const unsigned char* contact; const float* xref; const float* pos;
  const float* root; long long root_env;
  const float* mass; const float* dyn_bias;
  const float* j; long long j_env, j_foot;
  const float* mu; float mu_scalar;
  const float* weights; float alpha, fz_min, fz_max;
  int iters; float delta;
  const float* bias; const float* limit;
  float* u_io; int warm_shift;
  int n, H, nf, nd;
  float* forces; float* efforts;
};

// the cone's effort step for dof d of env e on forces fo (F x 3, zero where nothing stands).  A function of its own: written out
// inside the kernel the solve measured 0.4 % slower, on the same loops (profiles/r25_legged_core.md)
__device__ __forceinline__ float mpc_effort(const float* j, long long j_env, long long j_foot, const float* bias, const float* limit,
                                            int e, int d, int F, int nd, const float* fo) {
  const int D = nd + 6;
  float tau = 0.0f;
  for (int f = 0; f < F; f++) {
    const float* J = j + (long long)e * j_env + (long long)f * j_foot + 6;   // linear rows, dof columns
    tau = tau - cone::effort_term(J, D, d, fo[3 * f], fo[3 * f + 1], fo[3 * f + 2]);
  }
  return cone::effort_finish(tau, bias, limit, e, D, d);
}

__global__ void __launch_bounds__(2 * MPC_T) k_foot_force_mpc(MpcArgs A) {
  extern __shared__ float4 mpc_lds4[];
  float* lds = (float*)mpc_lds4;
  const int i = threadIdx.x, e = blockIdx.x;
  const int H = A.H, F = A.nf, F3 = 3 * F, N = F3 * H, N4 = (N + 3) & ~3, J4 = N4 >> 2;
  float* Kv = lds;                               // Kinv (P, then K, on the way), element (i, j) at ((j / 4) N4 + i) 4 + j mod 4
  float* bv = Kv + N4 * N4;                      // a sweep's right-hand side
  float* pr = bv + N4;                           // the pivot row of an elimination step
  float* xt = pr + N4;
  float* dg = xt + N4;                           // the diagonal of P
  float* cf = dg + N4;                           // 1.0 for a variable of a foot in contact
  float* Wt = cf + N4;                           // W, row r' at Wt + r' N4
  float* TX = Wt + 6 * N4;                       // TX_i[s] at TX + (s - 1) N4 + i
  float* TY = TX + H * N4;
  float* Ee = TY + H * N4;                       // E_s at Ee + (s - 1) 12
  float* CA = Ee + 12 * H;                       // C_0 .. C_H
  float* CB = CA + (H + 1);                      // S_0 .. S_H
  float* fo = CB + (H + 1);                      // step 0's forces
#define MPC_K(r, c) Kv[((((c) >> 2) * N4 + (r)) << 2) + ((c) & 3)]
  const float* rp = A.root + (long long)e * A.root_env;
  const float* xr = A.xref + (long long)e * (H + 1) * 12;
  const int D = A.nd + 6;
  const float delta = A.delta;
  const float* Lw = A.weights;
  // 1. Minv, g (every thread, in registers)
  float Mi[6][6], g[6];
  {
    const float* Mg = A.mass + (long long)e * D * D;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = 0; c < 6; c++) Mi[r][c] = Mg[r * D + c];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const float p = 1.0f / Mi[k][k];
      float row[6];
#pragma unroll
      for (int c = 0; c < 6; c++) row[c] = Mi[k][c] * p;
#pragma unroll
      for (int r = 0; r < 6; r++) {
        if (r == k) continue;
        const float f = Mi[r][k];
#pragma unroll
        for (int c = 0; c < 6; c++) Mi[r][c] = Mi[r][c] - f * row[c];
        Mi[r][k] = -(f * p);
      }
#pragma unroll
      for (int c = 0; c < 6; c++) Mi[k][c] = row[c];
      Mi[k][k] = p;
    }
    const float* hb = A.dyn_bias + (long long)e * D;
#pragma unroll
    for (int r = 0; r < 6; r++) {
      float acc = Mi[r][0] * hb[0];
#pragma unroll
      for (int c = 1; c < 6; c++) acc = acc + Mi[r][c] * hb[c];
      g[r] = -acc;
    }
  }
  // 2. the free response and the tables of the heading sums
  if (i == 0) {
    const float qx = rp[3], qy = rp[4], qz = rp[5], qw = rp[6];
    const float R20 = 2.0f * (qx * qz - qw * qy), R21 = 2.0f * (qy * qz + qw * qx), R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
    const float R10 = 2.0f * (qx * qy + qw * qz), R00 = 1.0f - 2.0f * (qy * qy + qz * qz);
    float x[12];
    x[0] = atan2f(R21, R22);
    x[1] = asinf(cone::clip(-R20, -1.0f, 1.0f));
    x[2] = atan2f(R10, R00);
    x[2] = x[2] + rintf((xr[2] - x[2]) * 0.15915494309189535f) * 6.283185307179586f;
#pragma unroll
    for (int k = 0; k < 3; k++) { x[3 + k] = rp[k]; x[6 + k] = rp[10 + k]; x[9 + k] = rp[7 + k]; }
    float ca = 0.0f, cb = 0.0f;
    CA[0] = 0.0f; CB[0] = 0.0f;
    for (int s = 0; s < H; s++) {
      const float psi = xr[s * 12 + 2];
      const float cs = cosf(psi), sn = sinf(psi);
      const float t0 = cs * x[6] + sn * x[7], t1 = cs * x[7] - sn * x[6];
      x[0] = x[0] + delta * t0; x[1] = x[1] + delta * t1; x[2] = x[2] + delta * x[8];
#pragma unroll
      for (int k = 0; k < 3; k++) x[3 + k] = x[3 + k] + delta * x[9 + k];
#pragma unroll
      for (int k = 0; k < 3; k++) { x[6 + k] = x[6 + k] + delta * g[3 + k]; x[9 + k] = x[9 + k] + delta * g[k]; }
      ca = ca + cs; cb = cb + sn;
      CA[s + 1] = ca; CB[s + 1] = cb;
#pragma unroll
      for (int r = 0; r < 12; r++) Ee[s * 12 + r] = x[r] - xr[(s + 1) * 12 + r];
    }
  }
  __syncthreads();
  // 3. W, TX, TY of this thread's variable
  const bool var = i < N;
  const int ki = var ? i / F3 : 0;
  const int ri = var ? i - ki * F3 : 0;
  const int fi = ri / 3, ci = ri - 3 * fi;
  bool con = false;
  float W[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (var) {
    const long long o = ((long long)e * H + ki) * F + fi;
    con = A.contact[o] != 0;
    const float s = con ? 1.0f : 0.0f;
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = A.pos[o * 3 + k] - (rp[k] + (xr[ki * 12 + 3 + k] - xr[3 + k]));
    const float a0 = ci == 0 ? 0.0f : (ci == 1 ? -r[2] : r[1]);
    const float a1 = ci == 0 ? r[2] : (ci == 1 ? 0.0f : -r[0]);
    const float a2 = ci == 0 ? -r[1] : (ci == 1 ? r[0] : 0.0f);
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const float mc = ci == 0 ? Mi[q][0] : (ci == 1 ? Mi[q][1] : Mi[q][2]);
      W[q] = (delta * (mc + ((Mi[q][3] * a0 + Mi[q][4] * a1) + Mi[q][5] * a2))) * s;
      Wt[q * N4 + i] = W[q];
    }
    const float c1 = CA[ki + 1], s1 = CB[ki + 1];
    for (int s_ = 1; s_ <= H; s_++) {
      float vx = 0.0f, vy = 0.0f;
      if (s_ > ki + 1) {
        const float a = CA[s_] - c1, b = CB[s_] - s1;
        vx = a * W[3] + b * W[4];
        vy = a * W[4] - b * W[3];
      }
      TX[(s_ - 1) * N4 + i] = vx; TY[(s_ - 1) * N4 + i] = vy;
    }
    cf[i] = s;
  } else if (i < N4) {
#pragma unroll
    for (int q = 0; q < 6; q++) Wt[q * N4 + i] = 0.0f;
    for (int s_ = 0; s_ < H; s_++) { TX[s_ * N4 + i] = 0.0f; TY[s_ * N4 + i] = 0.0f; }
    cf[i] = 0.0f;
  }
  __syncthreads();
  // 4. row i of P, q_i
  const float dd = delta * delta;
  float qi = 0.0f;
  if (var) {
    const float wLv0 = W[0] * Lw[9], wLv1 = W[1] * Lw[10], wLv2 = W[2] * Lw[11];
    const float wLw0 = W[3] * Lw[6], wLw1 = W[4] * Lw[7], wLw2 = W[5] * Lw[8];
    const float wLp0 = W[0] * Lw[3], wLp1 = W[1] * Lw[4], wLp2 = W[2] * Lw[5];
    const float wLz = W[5] * Lw[2];
    const float L0 = Lw[0], L1 = Lw[1];
    for (int kj = 0; kj < H; kj++) {
      const int m = ki > kj ? ki : kj;
      const float S0 = (float)(H - m);
      int s2 = 0;
      for (int s_ = m + 1; s_ <= H; s_++) s2 += (s_ - 1 - ki) * (s_ - 1 - kj);
      const float d2 = dd * (float)s2;
      for (int jj = 0; jj < F3; jj++) {
        const int j = kj * F3 + jj;
        const float w0 = Wt[j], w1 = Wt[N4 + j], w2 = Wt[2 * N4 + j], w3 = Wt[3 * N4 + j], w4 = Wt[4 * N4 + j], w5 = Wt[5 * N4 + j];
        const float dv = (wLv0 * w0 + wLv1 * w1) + wLv2 * w2;
        const float dw = (wLw0 * w3 + wLw1 * w4) + wLw2 * w5;
        const float dp = (wLp0 * w0 + wLp1 * w1) + wLp2 * w2;
        const float dz = wLz * w5;
        float th = 0.0f;
        for (int s_ = m; s_ < H; s_++)
          th = th + ((L0 * TX[s_ * N4 + i]) * TX[s_ * N4 + j] + (L1 * TY[s_ * N4 + i]) * TY[s_ * N4 + j]);
        float acc = (S0 * (dw + dv) + d2 * (dp + dz)) + dd * th;
        if (j == i) { acc = acc + A.alpha; dg[i] = acc; }
        MPC_K(i, j) = acc;
      }
    }
    for (int j = N; j < N4; j++) MPC_K(i, j) = 0.0f;
    for (int s_ = ki + 1; s_ <= H; s_++) {
      const float nn = (float)(s_ - 1 - ki);
      const float* E = Ee + (s_ - 1) * 12;
      const float lx = L0 * TX[(s_ - 1) * N4 + i], ly = L1 * TY[(s_ - 1) * N4 + i];
      const float pa = delta * ((lx * E[0] + ly * E[1]) + nn * (wLz * E[2]));
      const float pb = (delta * nn) * ((wLp0 * E[3] + wLp1 * E[4]) + wLp2 * E[5]);
      const float pc = ((wLw0 * E[6] + wLw1 * E[7]) + wLw2 * E[8]) + ((wLv0 * E[9] + wLv1 * E[10]) + wLv2 * E[11]);
      qi = qi + ((pa + pb) + pc);
    }
  } else if (i < N4) {
    for (int j = 0; j < N4; j++) MPC_K(i, j) = j == i ? 1.0f : 0.0f;   // a padding row: the identity's, inert
    dg[i] = 0.0f;
  }
  __syncthreads();
  // 5. rho, sigma; 6. K on the way to its inverse
  float mu = A.mu ? A.mu[e] : A.mu_scalar;
  mu = fmaxf(mu, 0.0f);
  float tr = 0.0f, nc = 0.0f;
  for (int j = 0; j < N; j++) { tr = tr + dg[j] * cf[j]; nc = nc + cf[j]; }
  float mean = tr / fmaxf(nc, 1.0f);
  mean = nc > 0.0f ? mean : 1.0f;
  const float rho = sqrtf(A.alpha * mean), sigma = cone::SIGMA * mean;
  if (var) MPC_K(i, i) = dg[i] + (sigma + rho * (ci == 2 ? 1.0f + 4.0f * (mu * mu) : 2.0f));
  for (int k = 0; k < N; k++) {
    __syncthreads();
    const float p = 1.0f / MPC_K(k, k);
    float f = 0.0f;
    if (i < N4) { f = MPC_K(i, k); pr[i] = MPC_K(k, i) * p; }
    __syncthreads();
    if (i < N4) {
      const int kq = k >> 2, kr = k & 3;
#pragma unroll 5                                  // several 16-byte reads in flight: one wave per SIMD hides no LDS latency otherwise
      for (int j4 = 0; j4 < J4; j4++) {
        const float4 pv = ((const float4*)pr)[j4];
        float4* ap = (float4*)Kv + (j4 * N4 + i);
        float4 av = *ap;
        if (i == k) {
          av = pv;
        } else {
          av.x = av.x - f * pv.x; av.y = av.y - f * pv.y; av.z = av.z - f * pv.z; av.w = av.w - f * pv.w;
        }
        if (j4 == kq) {
          const float vk = i == k ? p : -(f * p);
          if (kr == 0) av.x = vk; else if (kr == 1) av.y = vk; else if (kr == 2) av.z = vk; else av.w = vk;
        }
        *ap = av;
      }
    }
  }
  // 7. the sweeps
  const int i0 = i - ci;                         // the foot's x component
  float x = 0.0f, z[5], y[5];
  if (A.u_io && var && con) {
    int kk = ki + A.warm_shift;
    kk = kk > H - 1 ? H - 1 : (kk < 0 ? 0 : kk);
    x = A.u_io[(((long long)e * H + kk) * F + fi) * 3 + ci];
  }
  __syncthreads();
  if (i < N4) xt[i] = x;
  __syncthreads();
  {
    cone::rows(mu, var ? xt[i0] : 0.0f, var ? xt[i0 + 1] : 0.0f, var ? xt[i0 + 2] : 0.0f, z);
#pragma unroll
    for (int m = 0; m < 5; m++) y[m] = 0.0f;
  }
  float lo0, hi0, hic;
  cone::bounds(con, A.fz_min, A.fz_max, lo0, hi0, hic);
  const float irho = 1.0f / rho;
#pragma nounroll
  for (int it = 0; it < A.iters; it++) {
    if (i < N4) {
      float bi = 0.0f;
      if (var) {
        float v[5];
        cone::dual(rho, z, y, v);
        const float add = ci == 0 ? cone::at_x(v) : (ci == 1 ? cone::at_y(v) : cone::at_z(mu, v));
        bi = (sigma * x - qi) + add;
      }
      bv[i] = bi;
    }
    __syncthreads();
    float xi = 0.0f;
    if (i < N4) {
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 6                                  // the reads of six steps in flight; the four sums keep their order
      for (int j4 = 0; j4 < J4; j4++) {
        const float4 kv = ((const float4*)Kv)[j4 * N4 + i];
        const float4 b4 = ((const float4*)bv)[j4];
        s0 = s0 + kv.x * b4.x; s1 = s1 + kv.y * b4.y; s2 = s2 + kv.z * b4.z; s3 = s3 + kv.w * b4.w;
      }
      xi = (s0 + s1) + (s2 + s3);
      xt[i] = xi;
    }
    __syncthreads();
    if (var) {
      float zt[5];
      cone::rows(mu, xt[i0], xt[i0 + 1], xt[i0 + 2], zt);
      x = cone::relax(xi, x);
      cone::project(rho, irho, zt, lo0, hi0, hic, z, y);
    }
  }
  // 8. the forces, exactly feasible
  __syncthreads();
  if (i < N4) xt[i] = x;
  __syncthreads();
  if (var) {
    const float u = cone::feasible(con, ci, x, xt[i0 + 2], mu, A.fz_min, A.fz_max);
    if (A.u_io) A.u_io[(long long)e * N + i] = u;
    if (i < F3) { fo[i] = u; A.forces[(long long)e * F3 + i] = u; }
  }
  __syncthreads();
  // 9. the efforts
  if (i < A.nd) A.efforts[(long long)e * A.nd + i] = mpc_effort(A.j, A.j_env, A.j_foot, A.bias, A.limit, e, i, F, A.nd, fo);
#undef MPC_K
}

// ------------------------------------------------------------------------------------------------------ the efforts --
__global__ void __launch_bounds__(MPC_T) k_foot_force_efforts(const float* forces, const unsigned char* stance, const float* j,
                                                               long long j_env, long long j_foot, const float* bias,
                                                               const float* limit, int n, int nf, int nd, float* efforts) {
  const int e = blockIdx.x * MPC_T + threadIdx.x;
  if (e >= n) return;
  float fo[3 * MPC_MAX_FEET];
#pragma unroll
  for (int f = 0; f < MPC_MAX_FEET; f++) {
    const bool on = f < nf && stance[(long long)e * nf + (f < nf ? f : 0)] != 0;
#pragma unroll
    for (int k = 0; k < 3; k++) fo[3 * f + k] = on ? forces[((long long)e * nf + f) * 3 + k] : 0.0f;
  }
  const int D = nd + 6;
  for (int d = 0; d < nd; d++) {
    float tau = 0.0f;
#pragma unroll
    for (int f = 0; f < MPC_MAX_FEET; f++) {
      if (f < nf) {
        const float* J = j + (long long)e * j_env + (long long)f * j_foot + 6;
        tau = tau - cone::effort_term(J, D, d, fo[3 * f], fo[3 * f + 1], fo[3 * f + 2]);
      }
    }
    efforts[(long long)e * nd + d] = cone::effort_finish(tau, bias, limit, e, D, d);
  }
}

// above the default dynamic-LDS limit a kernel has to opt in, once per device (as shf_api.hip's grant_lds: the attribute call
// is not a stream operation and must not recur while the caller's stream is being captured)
int mpc_grant_lds() {
  static std::mutex mu;
  static unsigned long long granted = 0;         // bit d: device d has the limit raised
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  std::lock_guard<std::mutex> lock(mu);
  if (dev < 64 && ((granted >> dev) & 1ull)) return 0;
  if (hipFuncSetAttribute((const void*)k_foot_force_mpc, hipFuncAttributeMaxDynamicSharedMemorySize,
                          mpc_lds_floats(MPC_MAX_N, MPC_MAX_H) * 4) != hipSuccess)
    return 1;
  if (dev < 64) granted |= 1ull << dev;
  return 0;
}

}  // namespace

extern "C" int shf_mpc_horizon(const int32_t* tick, const float* target, const float* yaw, int32_t period_ticks,
                               const int32_t* offset_ticks, const int32_t* stance_ticks, const uint8_t* stance,
                               const float* foot_pos, int64_t foot_env_stride, int64_t foot_stride, const float* command,
                               const float* nominal, ShfGaitParams params, int32_t horizon, int32_t ticks_per_step, int32_t n,
                               int32_t num_feet, uint8_t* contact_out, float* xref_out, float* pos_out, void* stream) {
  if (!tick || !target || !yaw || !offset_ticks || !stance_ticks || !stance || !foot_pos || !command || !nominal || !contact_out ||
      !xref_out || !pos_out)
    return shf_set_error("shf_mpc_horizon: null tensor");
  if (num_feet < 1 || num_feet > MPC_MAX_FEET) return shf_set_error("shf_mpc_horizon: 1 to 4 feet");
  if (horizon < 1 || horizon > MPC_MAX_H) return shf_set_error("shf_mpc_horizon: horizon outside 1..SHF_MPC_MAX_HORIZON");
  if (ticks_per_step < 1) return shf_set_error("shf_mpc_horizon: ticks_per_step must be at least 1");
  if (period_ticks < 1) return shf_set_error("shf_mpc_horizon: period_ticks must be at least 1");
  for (int f = 0; f < num_feet; f++) {
    if (stance_ticks[f] < 1 || stance_ticks[f] > period_ticks) return shf_set_error("shf_mpc_horizon: stance_ticks outside 1..period_ticks");
    if (offset_ticks[f] < 0 || offset_ticks[f] >= period_ticks) return shf_set_error("shf_mpc_horizon: offset_ticks outside 0..period_ticks-1");
  }
  if (!(params.dt > 0.0f)) return shf_set_error("shf_mpc_horizon: dt must be positive");
  if (!(params.max_step >= 0.0f)) return shf_set_error("shf_mpc_horizon: max_step must not be negative");
  if (n <= 0) return 0;
  HorizonArgs A = {};
  A.tick = tick; A.target = target; A.yaw = yaw;
  A.period = (int)period_ticks;
  for (int f = 0; f < MPC_MAX_FEET; f++) {
    A.offset[f] = f < num_feet ? (int)offset_ticks[f] : 0;
    A.stance_ticks[f] = f < num_feet ? (int)stance_ticks[f] : 1;
  }
  A.stance = stance;
  A.foot = foot_pos; A.foot_env = (long long)foot_env_stride; A.foot_stride = (long long)foot_stride;
  A.command = command; A.nominal = nominal; A.P = params;
  A.H = (int)horizon; A.S = (int)ticks_per_step; A.n = (int)n; A.nf = (int)num_feet;
  A.contact = contact_out; A.xref = xref_out; A.pos = pos_out;
  hipLaunchKernelGGL(k_mpc_horizon, dim3((n + MPC_T - 1) / MPC_T), dim3(MPC_T), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_mpc_horizon: launch failed");
}

extern "C" int shf_foot_force_mpc(const uint8_t* contact, const float* xref, const float* pos, const float* root_pose,
                                  int64_t root_env_stride, const float* mass_matrix, const float* dyn_bias, const float* j_feet,
                                  int64_t j_env_stride, int64_t j_foot_stride, const float* mu_or_null, float mu_scalar,
                                  const float* weights12, float alpha, float fz_min, float fz_max, int32_t iters, float step_dt,
                                  const float* bias_or_null, const float* effort_limit_or_null, float* u_io_or_null,
                                  int32_t warm_shift, int32_t n, int32_t horizon, int32_t num_feet, int32_t num_dof,
                                  float* forces_out, float* efforts_out, void* stream) {
  if (!contact || !xref || !pos || !root_pose || !mass_matrix || !dyn_bias || !j_feet || !weights12 || !forces_out || !efforts_out)
    return shf_set_error("shf_foot_force_mpc: null tensor");
  if (num_feet < 1 || num_feet > MPC_MAX_FEET) return shf_set_error("shf_foot_force_mpc: 1 to 4 feet");
  if (horizon < 1 || horizon > MPC_MAX_H) return shf_set_error("shf_foot_force_mpc: horizon outside 1..SHF_MPC_MAX_HORIZON");
  if (num_dof < 1) return shf_set_error("shf_foot_force_mpc: at least one dof");
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_foot_force_mpc: too many dofs");
  if (!(alpha > 0.0f)) return shf_set_error("shf_foot_force_mpc: alpha must be positive");
  if (!(fz_min <= fz_max)) return shf_set_error("shf_foot_force_mpc: fz_min exceeds fz_max");
  if (!mu_or_null && !(mu_scalar >= 0.0f)) return shf_set_error("shf_foot_force_mpc: mu must not be negative");
  if (iters < 1) return shf_set_error("shf_foot_force_mpc: iters must be at least 1");
  if (!(step_dt > 0.0f)) return shf_set_error("shf_foot_force_mpc: step_dt must be positive");
  if (warm_shift < 0) return shf_set_error("shf_foot_force_mpc: warm_shift must not be negative");
  if (n <= 0) return 0;
  MpcArgs A = {contact, xref, pos, root_pose, (long long)root_env_stride, mass_matrix, dyn_bias, j_feet, (long long)j_env_stride,
               (long long)j_foot_stride, mu_or_null, mu_scalar, weights12, alpha, fz_min, fz_max, (int)iters, step_dt, bias_or_null,
               effort_limit_or_null, u_io_or_null, (int)warm_shift, (int)n, (int)horizon, (int)num_feet, (int)num_dof, forces_out,
               efforts_out};
  const int N = 3 * num_feet * horizon, N4 = (N + 3) & ~3;
  const int threads = N4 <= MPC_T ? MPC_T : 2 * MPC_T;       // num_dof <= 32 effort threads fit either way
  const size_t lds = (size_t)mpc_lds_floats(N4, horizon) * 4;
  if (lds > 48 * 1024 && mpc_grant_lds()) return shf_set_error("shf_foot_force_mpc: the LDS limit could not be raised");
  hipLaunchKernelGGL(k_foot_force_mpc, dim3(n), dim3(threads), lds, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_foot_force_mpc: launch failed");
}

extern "C" int shf_foot_force_efforts(const float* forces, const uint8_t* stance, const float* j_feet, int64_t j_env_stride,
                                      int64_t j_foot_stride, const float* bias_or_null, const float* effort_limit_or_null, int32_t n,
                                      int32_t num_feet, int32_t num_dof, float* efforts_out, void* stream) {
  if (!forces || !stance || !j_feet || !efforts_out) return shf_set_error("shf_foot_force_efforts: null tensor");
  if (num_feet < 1 || num_feet > MPC_MAX_FEET) return shf_set_error("shf_foot_force_efforts: 1 to 4 feet");
  if (num_dof < 1) return shf_set_error("shf_foot_force_efforts: at least one dof");
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_foot_force_efforts: too many dofs");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_foot_force_efforts, dim3((n + MPC_T - 1) / MPC_T), dim3(MPC_T), 0, (hipStream_t)stream, forces, stance, j_feet,
                     (long long)j_env_stride, (long long)j_foot_stride, bias_or_null, effort_limit_or_null, (int)n, (int)num_feet,
                     (int)num_dof, efforts_out);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_foot_force_efforts: launch failed");
}
