// shf_gait.hip -- the swing half of the model-based legged controller (LeggedRobot.locomotion_control): per env, which feet
// should stand now, where a lifted foot should land, where it should be on the way, and where the base target has got to.  One
// launch (k_gait_plan), one thread per env, is the gait clock, the foothold planner, the swing trajectory and the base-target
// integrator; a second small kernel (k_leg_effort_mix) adds the swing legs' efforts to the stance efforts of shf_foot_force_qp.
// A translation unit of its own, so that no other kernel's machine code moves.
//
// Time is an integer: one call is one tick.  A gait is period_ticks P and, per foot f, offset_ticks o_f in 0..P-1 and
// stance_ticks S_f in 1..P (S_f = P: the foot always stands).  Nothing in the schedule compares floats, so two number formats
// can never disagree about an event.  World axes, z up; quaternions xyzw; R(q) as in k_foot_impedance.
//
// Per-env state, read and written in place: tick (int32), sched (F uint8: last call's scheduled stance), anchor (F x 3, world),
// target (13 floats: pos, quat, v, omega -- shf_foot_force_qp's base_target row), yaw (the target's heading, never wrapped).
//
// The algorithm.  tests/gait_ref.py `plan` is this text in NumPy, operation by operation.  p, q, v: the root row's position,
// quaternion and linear velocity; x_f: foot f's world position; (n_fx, n_fy): foot f's nominal position in the base frame;
// (vx, vy, wz): the command; c_f: the contact force z of foot f.
//   1. Reset (reset[e] != 0):  tick = 0;  sched_f = 1 and anchor_f = (x_f.xy, touchdown_z - late_depth) for every foot (the
//        foothold under the foot: a foot that hangs in the air at a reset is late, and is pressed down where it is);
//        yaw = atan2(2 (q_x q_y + q_w q_z), 1 - 2 (q_y^2 + q_z^2))  (the base's heading);  target.xy = p.xy.
//   2. Base target.  c = cos(yaw), s = sin(yaw);  v_w = (c vx - s vy, s vx + c vy);  target.xy = target.xy + v_w dt;
//        d = target.xy - p.xy,  r = sqrt(d_x^2 + d_y^2);  if r > leash: target.xy = p.xy + d (leash / r);
//        yaw = yaw + wz dt;  target.quat = (0, 0, sin(yaw / 2), cos(yaw / 2));  target.z = height;
//        target.v = (v_w, 0);  target.omega = (0, 0, wz).
//   3. Schedule, per foot:  phi = ((tick mod P) + o_f) mod P  (tick mod P taken non-negative);  s_f = phi < S_f.
//   4. Foothold, per foot, with R = R(q):  n_w = (R_00 n_fx + R_01 n_fy, R_10 n_fx + R_11 n_fy);  hip = p.xy + n_w;
//        v_des = (v_w.x - wz n_w.y, v_w.y + wz n_w.x);  T_st = S_f dt;
//        g = v_des (T_st / 2) + k_fb (v.xy - v_w);  m = sqrt(g_x^2 + g_y^2);  if m > max_step: g = g (max_step / m);
//        foothold = hip + g.
//   5. Events, per foot.  Lift-off (sched_f == 1, s_f == 0): anchor_f = x_f.
//        Scheduled touchdown (sched_f == 0, s_f == 1): anchor_f = (foothold, touchdown_z - late_depth).
//   6. Foot target y_f in the world.
//        Swing (s_f == 0):  u = (phi - S_f + 1) / (P - S_f)  (integers, one float division),  b = (u u) (3 - 2 u),
//          y.xy = (1 - b) anchor.xy + b foothold,   y.z = ((1 - b) anchor.z + b touchdown_z) + ((4 apex) u) (1 - u)
//          -- the first target lies one tick's motion from the lift-off point, the last one (u = 1) is (foothold, touchdown_z)
//          exactly.
//        Scheduled to stand, not touching (c_f <= contact_threshold):  y = anchor_f  (a late foot keeps pressing down at
//          the planned foothold).
//        Standing and touching (or no contact tensor):  y = x_f.
//        swing_target_f = R^T (y - p)  (rows: sum over k of R_ki (y - p)_k, k = 0, 1, 2 in that order): base frame, what
//          shf_foot_impedance takes.
//   7. Outputs:  stance_f = s_f and (c_f > contact_threshold)  (no contact tensor: s_f);  phase_f = phi / P;
//        sched_f = s_f;  tick = tick + 1.
// No multiply-add is fused (the arithmetic contract of csrc/shf_device.h).  Everything of an env lives in registers: the
// foot loop is unrolled over the four possible feet, so every array index is a compile-time constant.
//
// k_leg_effort_mix, one thread per env:  efforts_out[e, d] = clamp(stance_efforts[e, d] + m swing_efforts[e, d], +-limit[d]),
// m = 1.0 if some foot f with stance[e, f] == 0 has chain[f, d] != 0, else 0.0; limit entries <= 0 (or no limit): no clamp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns

namespace {

constexpr int GAIT_T = 64;                     // threads per block: one wavefront
constexpr int GAIT_MAX_FEET = 4;

struct GaitArgs {
  const float* root; long long root_env;
  const float* foot; long long foot_env, foot_stride;
  const float* contact; long long contact_env, contact_foot;
  const float* command; const float* nominal; const unsigned char* reset;
  int period; int offset[GAIT_MAX_FEET]; int stance_ticks[GAIT_MAX_FEET];
  ShfGaitParams P;
  int* tick; unsigned char* sched; float* anchor; float* target; float* yaw;
  int n, nf;
  unsigned char* stance; float* swing; float* phase;
};

__global__ void __launch_bounds__(GAIT_T) k_gait_plan(GaitArgs A) {
  const int e = blockIdx.x * GAIT_T + threadIdx.x;
  if (e >= A.n) return;
  const int F = A.nf, P = A.period;
  const float* rp = A.root + (long long)e * A.root_env;
  const float px = rp[0], py = rp[1], pz = rp[2];
  const float qx = rp[3], qy = rp[4], qz = rp[5], qw = rp[6];
  const float vx = rp[7], vy = rp[8];
  float* tg = A.target + (long long)e * 13;
  float* an = A.anchor + (long long)e * F * 3;
  unsigned char* sc = A.sched + (long long)e * F;
  float xf[GAIT_MAX_FEET][3], ac[GAIT_MAX_FEET][3];
  bool was[GAIT_MAX_FEET];
#pragma unroll
  for (int f = 0; f < GAIT_MAX_FEET; f++) {
    if (f < F) {
      const float* pf = A.foot + (long long)e * A.foot_env + (long long)f * A.foot_stride;
#pragma unroll
      for (int k = 0; k < 3; k++) { xf[f][k] = pf[k]; ac[f][k] = an[3 * f + k]; }
      was[f] = sc[f] != 0;
    }
  }
  int tick = A.tick[e];
  float yaw = A.yaw[e], tx = tg[0], ty = tg[1];
  // 1. reset
  if (A.reset && A.reset[e]) {
    tick = 0;
#pragma unroll
    for (int f = 0; f < GAIT_MAX_FEET; f++) {
      if (f < F) {
        was[f] = true;
        ac[f][0] = xf[f][0]; ac[f][1] = xf[f][1]; ac[f][2] = A.P.touchdown_z - A.P.late_depth;
      }
    }
    yaw = atan2f(2.0f * (qx * qy + qw * qz), 1.0f - 2.0f * (qy * qy + qz * qz));
    tx = px; ty = py;
  }
  // 2. the base target
  const float cvx = A.command[(long long)e * 3], cvy = A.command[(long long)e * 3 + 1], wz = A.command[(long long)e * 3 + 2];
  const float dt = A.P.dt;
  const float cy = cosf(yaw), sy = sinf(yaw);
  const float vwx = cy * cvx - sy * cvy, vwy = sy * cvx + cy * cvy;
  tx = tx + vwx * dt; ty = ty + vwy * dt;
  {
    const float dx = tx - px, dy = ty - py;
    const float r = sqrtf(dx * dx + dy * dy);
    if (r > A.P.leash) {
      const float k = A.P.leash / r;
      tx = px + dx * k; ty = py + dy * k;
    }
  }
  yaw = yaw + wz * dt;
  const float hy = yaw * 0.5f;
  tg[0] = tx; tg[1] = ty; tg[2] = A.P.height;
  tg[3] = 0.0f; tg[4] = 0.0f; tg[5] = sinf(hy); tg[6] = cosf(hy);
  tg[7] = vwx; tg[8] = vwy; tg[9] = 0.0f;
  tg[10] = 0.0f; tg[11] = 0.0f; tg[12] = wz;
  A.yaw[e] = yaw;
  const float R[9] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qw * qz), 2.0f * (qx * qz + qw * qy),
                      2.0f * (qx * qy + qw * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qw * qx),
                      2.0f * (qx * qz - qw * qy), 2.0f * (qy * qz + qw * qx), 1.0f - 2.0f * (qx * qx + qy * qy)};
  int tm = tick % P;
  tm = tm < 0 ? tm + P : tm;
#pragma unroll
  for (int f = 0; f < GAIT_MAX_FEET; f++) {
    if (f < F) {
      // 3. the schedule
      const int S = A.stance_ticks[f];
      const int phi = (tm + A.offset[f]) % P;
      const bool s = phi < S;
      // 4. the foothold
      const float nfx = A.nominal[3 * f], nfy = A.nominal[3 * f + 1];
      const float nwx = R[0] * nfx + R[1] * nfy, nwy = R[3] * nfx + R[4] * nfy;
      const float hx = px + nwx, hyp = py + nwy;
      const float vdx = vwx - wz * nwy, vdy = vwy + wz * nwx;
      const float half = ((float)S * dt) * 0.5f;
      float gx = vdx * half + A.P.k_fb * (vx - vwx), gy = vdy * half + A.P.k_fb * (vy - vwy);
      const float m = sqrtf(gx * gx + gy * gy);
      if (m > A.P.max_step) {
        const float k = A.P.max_step / m;
        gx = gx * k; gy = gy * k;
      }
      const float fx = hx + gx, fy = hyp + gy;
      // 5. events
      if (was[f] && !s) {
#pragma unroll
        for (int k = 0; k < 3; k++) ac[f][k] = xf[f][k];
      }
      if (!was[f] && s) { ac[f][0] = fx; ac[f][1] = fy; ac[f][2] = A.P.touchdown_z - A.P.late_depth; }
      // 6. the foot's target
      const bool touching = A.contact ? A.contact[(long long)e * A.contact_env + (long long)f * A.contact_foot] > A.P.contact_threshold : true;
      float y0, y1, y2;
      if (!s) {
        const float u = (float)(phi - S + 1) / (float)(P - S);
        const float b = (u * u) * (3.0f - 2.0f * u);
        const float a1 = 1.0f - b;
        y0 = a1 * ac[f][0] + b * fx;
        y1 = a1 * ac[f][1] + b * fy;
        y2 = (a1 * ac[f][2] + b * A.P.touchdown_z) + ((4.0f * A.P.apex) * u) * (1.0f - u);
      } else if (!touching) {
        y0 = ac[f][0]; y1 = ac[f][1]; y2 = ac[f][2];
      } else {
        y0 = xf[f][0]; y1 = xf[f][1]; y2 = xf[f][2];
      }
      const float d0 = y0 - px, d1 = y1 - py, d2 = y2 - pz;
      float* sw = A.swing + ((long long)e * F + f) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) sw[k] = (R[k] * d0 + R[3 + k] * d1) + R[6 + k] * d2;
      // 7. outputs
      A.stance[(long long)e * F + f] = (s && touching) ? 1 : 0;
      A.phase[(long long)e * F + f] = (float)phi / (float)P;
      sc[f] = s ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 3; k++) an[3 * f + k] = ac[f][k];
    }
  }
  A.tick[e] = tick + 1;
}

__global__ void __launch_bounds__(GAIT_T) k_leg_effort_mix(const float* stance_eff, const float* swing_eff, const unsigned char* stance,
                                                           const unsigned char* chain, const float* limit, int n, int nf, int nd,
                                                           float* out) {
  const int e = blockIdx.x * GAIT_T + threadIdx.x;
  if (e >= n) return;
  unsigned int lifted = 0;                       // bit f: foot f is not in stance
  for (int f = 0; f < nf; f++) lifted |= (stance[(long long)e * nf + f] == 0 ? 1u : 0u) << f;
  for (int d = 0; d < nd; d++) {
    bool on = false;
    for (int f = 0; f < nf; f++) on = on || (((lifted >> f) & 1u) && chain[f * nd + d] != 0);
    const float m = on ? 1.0f : 0.0f;
    float v = stance_eff[(long long)e * nd + d] + m * swing_eff[(long long)e * nd + d];
    const float lim = limit ? limit[d] : 0.0f;
    if (lim > 0.0f) v = fmaxf(fminf(v, lim), -lim);
    out[(long long)e * nd + d] = v;
  }
}

}  // namespace

extern "C" int shf_gait_plan(const float* root_pose, int64_t root_env_stride, const float* foot_pos, int64_t foot_env_stride,
                             int64_t foot_stride, const float* contact_z_or_null, int64_t contact_env_stride,
                             int64_t contact_foot_stride, const float* command, const float* nominal, const uint8_t* reset_or_null,
                             int32_t period_ticks, const int32_t* offset_ticks, const int32_t* stance_ticks, ShfGaitParams params,
                             int32_t* tick, uint8_t* sched, float* anchor, float* target, float* yaw, int32_t n, int32_t num_feet,
                             uint8_t* stance_out, float* swing_target_out, float* phase_out, void* stream) {
  if (!root_pose || !foot_pos || !command || !nominal || !offset_ticks || !stance_ticks || !tick || !sched || !anchor || !target ||
      !yaw || !stance_out || !swing_target_out || !phase_out)
    return shf_set_error("shf_gait_plan: null tensor");
  if (num_feet < 1 || num_feet > GAIT_MAX_FEET) return shf_set_error("shf_gait_plan: 1 to 4 feet");
  if (period_ticks < 1) return shf_set_error("shf_gait_plan: period_ticks must be at least 1");
  for (int f = 0; f < num_feet; f++) {
    if (stance_ticks[f] < 1 || stance_ticks[f] > period_ticks) return shf_set_error("shf_gait_plan: stance_ticks outside 1..period_ticks");
    if (offset_ticks[f] < 0 || offset_ticks[f] >= period_ticks) return shf_set_error("shf_gait_plan: offset_ticks outside 0..period_ticks-1");
  }
  if (!(params.dt > 0.0f)) return shf_set_error("shf_gait_plan: dt must be positive");
  if (!(params.max_step >= 0.0f)) return shf_set_error("shf_gait_plan: max_step must not be negative");
  if (n <= 0) return 0;
  GaitArgs A = {};
  A.root = root_pose; A.root_env = (long long)root_env_stride;
  A.foot = foot_pos; A.foot_env = (long long)foot_env_stride; A.foot_stride = (long long)foot_stride;
  A.contact = contact_z_or_null; A.contact_env = (long long)contact_env_stride; A.contact_foot = (long long)contact_foot_stride;
  A.command = command; A.nominal = nominal; A.reset = reset_or_null;
  A.period = (int)period_ticks;
  for (int f = 0; f < GAIT_MAX_FEET; f++) {
    A.offset[f] = f < num_feet ? (int)offset_ticks[f] : 0;
    A.stance_ticks[f] = f < num_feet ? (int)stance_ticks[f] : 1;
  }
  A.P = params;
  A.tick = tick; A.sched = sched; A.anchor = anchor; A.target = target; A.yaw = yaw;
  A.n = (int)n; A.nf = (int)num_feet;
  A.stance = stance_out; A.swing = swing_target_out; A.phase = phase_out;
  hipLaunchKernelGGL(k_gait_plan, dim3((n + GAIT_T - 1) / GAIT_T), dim3(GAIT_T), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_gait_plan: launch failed");
}

extern "C" int shf_leg_effort_mix(const float* stance_efforts, const float* swing_efforts, const uint8_t* stance,
                                  const uint8_t* chain_mask, const float* effort_limit_or_null, int32_t n, int32_t num_feet,
                                  int32_t num_dof, float* efforts_out, void* stream) {
  if (!stance_efforts || !swing_efforts || !stance || !chain_mask || !efforts_out) return shf_set_error("shf_leg_effort_mix: null tensor");
  if (num_feet < 1 || num_feet > 32) return shf_set_error("shf_leg_effort_mix: 1 to 32 feet");
  if (num_dof < 1) return shf_set_error("shf_leg_effort_mix: at least one dof");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_leg_effort_mix, dim3((n + GAIT_T - 1) / GAIT_T), dim3(GAIT_T), 0, (hipStream_t)stream, stance_efforts,
                     swing_efforts, stance, chain_mask, effort_limit_or_null, (int)n, (int)num_feet, (int)num_dof, efforts_out);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_leg_effort_mix: launch failed");
}
