// shf_proprio.hip -- what a legged robot measures about itself: IMUs (gyro and accelerometer with bias, noise and a bias random
// walk), joint encoders (offset, noise, quantisation, a measured or a differenced velocity) and foot contact switches (hysteresis
// and the air / contact time bookkeeping), each behind a per-env latency.  One launch (k_proprioception) is one sensor read of
// every env.  A work item is one (env e, unit) pair -- a unit is one IMU, one dof or one foot -- 256 to a block; blockIdx.y
// names the class (0 IMUs, 1 encoders, 2 feet), so that a wavefront runs one class's code.  A pair reads and writes its own
// state rows only: there is no atomic, no count, and nothing two lanes could race on; an env's units may lie in different
// wavefronts or blocks, and a captured launch replays correctly.  A translation unit of its own, so that no other kernel's
// machine code moves.
//
// Inputs, read in place (element strides between envs and between rows are arguments; a row itself is contiguous):
//   body_state (N, nb, 13): position (3), quaternion xyzw (4), linear velocity (3), angular velocity (3), all in world axes.
//     The linear velocity is the velocity of the BODY FRAME'S ORIGIN (the link frame's origin, not the centre of mass): the
//     step kernels and shf_sim_refresh write J_b nu there, and J_b's first three rows are "the velocity of b's origin"
//     (csrc/shf_dyn.h; tests/test_gpu_floating_dynamics.py checks the two against each other).  The rigid-body formula
//     carries it to the sensor point: v_s = v_b + w_b x (R_b p_s).
//   dof_state (N, nd, 2): position, velocity.    contact (N, nb, 3): the net contact force on a body, world axes.
//   reset (N) uint8 or NULL: 1 = this env was teleported since the last read.  The kernel reads the flags and leaves them.
//   delay (N, 3) int32: the latency in reads of the env's IMUs, encoders, feet; D = min(max(delay, 0), max_delay).
//   params (SHF_PROPRIO_NUM_PARAMS) float32 on the device, so that a captured launch sees a changed noise level:
//     [0] sg  gyro noise            [1] sa  accelerometer noise        [2] wg = sigma_walk_gyro sqrt(dt)  [3] wa (accel)
//     [4] b0g gyro bias range       [5] b0a accelerometer bias range   [6] sq  encoder position noise     [7] sv  velocity noise
//     [8] o   encoder offset range  [9] r   encoder resolution (0: no quantisation)  [10] 1 / r (0 when r = 0)
//     [11] f_on^2  [12] f_off^2  (the products are formed on the host)
// State, owned by the caller, zero before the first read, read and written in place:
//   counter (N, U, 2) int32, U = I + nd + F units in the order IMUs, dofs, feet: [the env's read counter c (uint32, never
//     reset), the ring's head h].  Every unit of an env carries its own copy of c -- all equal -- because one shared word
//     would be read by some lanes after another had already written it.
//   imu_state  (N, I, 9 + 6 L):  v_prev (3), bias_g (3), bias_a (3), ring (L, 6) of (gyro, accel)
//   enc_state  (N, nd, 2 + 2 L): offset, q_meas_prev, ring (L, 2) of (q_meas, qd_meas)
//   foot_state (N, F, 5 + 6 L):  switch, air_time, contact_time, last_air_time, last_contact_time, ring (L, 6) of the outputs
// Outputs: out (N, D) float32, D = 6 I + 2 nd + 6 F: gyro (I, 3) | accel (I, 3) | dof_pos (nd) | dof_vel (nd) | contact (F) |
//   first_contact (F) | air_time (F) | contact_time (F) | last_air_time (F) | last_contact_time (F), the two switches as 0 / 1;
//   switch_out (N, 2 F) uint8 or NULL: contact (F) | first_contact (F) again, as bytes.
//
// Randomness.  Philox4x32-10 as csrc/shf_task.h has it (philox4x32, u01), key = the sensor's seed, counter words
// (gid low, c, stream, gid high), gid = global_ids[e] when that tensor is given, else env_id_offset + e: a sharded run draws
// what the unsharded one draws, and c never repeats.  One block of four words gives either a unit normal
//     gauss(stream) = (((u0 + u1) + (u2 + u3)) - 2) * 1.7320508f          (Irwin-Hall of order 4: variance 4 / 12, scaled to 1)
// or up to three uniforms  U_k(stream, b) = ((b - (-b)) u_k) + (-b).   u_k = u01(word k).  Streams:
//     IMU i:  S = 0x50000000 + 16 i;  S + a: gyro noise axis a;  S + 3 + a: accel noise;  S + 6 + a: gyro walk;  S + 9 + a: accel
//             walk (a = 0, 1, 2);  S + 12: the gyro bias redraw (axis a takes u_a);  S + 13: the accel bias redraw.
//     dof d:  S = 0x50001000 + 4 d;  S: position noise;  S + 1: velocity noise;  S + 2: the offset redraw (u_0).
//
// The algorithm.  tests/proprio_ref.py `step32` is this text in NumPy float32, operation by operation; no multiply-add is fused
// (the arithmetic contract of csrc/shf_device.h), no division and no maths-library call is made, so every line is a sequence of
// correctly rounded float32 operations in the order written; sums of three go left to right.
// Every unit:  c, h = counter[e, u];  rs = (reset[e] != 0) or (c == 0).  At the end:  counter[e, u] = (c + 1, h + 1 == L ? 0 : h + 1).
// Quaternion product a * b (xyzw):   x = ((aw bx + ax bw) + ay bz) - az by;   y = ((aw by - ax bz) + ay bw) + az bx;
//     z = ((aw bz + ax by) - ay bx) + az bw;   w = ((aw bw - ax bx) - ay by) - az bz.
// Rotation matrix of q:  R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz),
//     R12 = 2 (yz - wx), R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy);   (R v)_i = (Ri0 v0 + Ri1 v1) + Ri2 v2;
//     (R^T v)_i = (R0i v0 + R1i v1) + R2i v2.    Cross product (a x b)_0 = a1 b2 - a2 b1, and cyclically.
// Latency (every class, C channels, measurement m):  out = (rs or D == 0) ? m : ring[h - D (+ L if negative)];  then
//     rs: every slot of the ring = m (the rule of the actuator's command history);  else ring[h] = m.
//
// 1. IMU i on body b = imu_body[i] at (p_s, q_s):
//    a. R = matrix(q_b * q_s);  Rb = matrix(q_b);  v_s = v_b + (w_b x (Rb p_s)).
//    b. rs:  bias_g[a] = U_a(S + 12, b0g),  bias_a[a] = U_a(S + 13, b0a),  v_prev = v_s.
//    c. gyro[a] = ((R^T w_b)[a] + bias_g[a]) + (sg gauss(S + a)).
//    d. acc_w[a] = ((v_s[a] - v_prev[a]) inv_dt) - g[a];   accel[a] = ((R^T acc_w)[a] + bias_a[a]) + (sa gauss(S + 3 + a)).
//    e. latency with m = (gyro, accel).
//    f. bias_g[a] = bias_g[a] + (wg gauss(S + 6 + a));   bias_a[a] = bias_a[a] + (wa gauss(S + 9 + a));   v_prev = v_s.
// 2. Encoder of dof d, (q, qd) = dof_state[e, d]:
//    a. rs:  offset = U_0(S + 2, o).
//    b. x = (q + offset) + (sq gauss(S));   r > 0:  x = r rintf(x inv_r);   q_meas = x.
//    c. SHF_PROPRIO_VEL_DIRECT:  qd_meas = qd + (sv gauss(S + 1)).
//       SHF_PROPRIO_VEL_DIFFERENCE:  rs: q_meas_prev = q_meas;   qd_meas = (q_meas - q_meas_prev) inv_dt.
//    d. latency with m = (q_meas, qd_meas);   q_meas_prev = q_meas.
// 3. Foot f on body b = foot_body[f], force (fx, fy, fz) = contact[e, b]; p = the stored switch:
//    a. s = (fx fx + fy fy) + fz fz  (SHF_PROPRIO_CONTACT_NORM)  or  fz |fz|  (SHF_PROPRIO_CONTACT_Z).
//    b. rs:  p = 0 and the four times = 0.     on = s > f_on^2 ? 1 : (s < f_off^2 ? 0 : p).
//    c. first = on and not p and not rs;   left = p and not on   (a reset is a teleport: no touch-down is reported across it).
//    d. first: last_air_time = air_time + dt.    left: last_contact_time = contact_time + dt.
//       air_time = on ? 0 : air_time + dt;   contact_time = on ? contact_time + dt : 0.
//    e. latency with m = (on, first, air_time, contact_time, last_air_time, last_contact_time);  the stored switch = on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "shf_task.h"          // philox4x32, u01

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns

namespace {

constexpr int PRO_T = 256;                     // threads per block
constexpr uint32_t PRO_STREAM_IMU = 0x50000000u, PRO_STREAM_ENC = 0x50001000u;

struct ProArgs {
  const float* body; long long body_env, body_row;
  const float* dof; long long dof_env, dof_row;
  const float* contact; long long con_env, con_row;
  const unsigned char* reset; const float* params; const int* delay; const long long* gids;
  int* counter; float* imu; float* enc; float* foot;
  float* out; unsigned char* sw;
  int n, nd, I, F, L, maxd, cmode, vmode;
  int imu_body[SHF_PROPRIO_MAX_IMUS]; float imu_pos[SHF_PROPRIO_MAX_IMUS][3]; float imu_quat[SHF_PROPRIO_MAX_IMUS][4];
  int foot_body[SHF_PROPRIO_MAX_FEET];
  float g[3]; float dt, inv_dt;
  uint32_t k0, k1; long long gid0;
};

struct Draw { uint32_t k0, k1, c; long long gid; };

DEV void block(const Draw& w, uint32_t stream, float (&u)[4]) {
  uint32_t r[4];
  philox4x32((uint32_t)w.gid, w.c, stream, (uint32_t)((unsigned long long)w.gid >> 32), w.k0, w.k1, r);
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] = u01(r[k]);
}
DEV float gauss(const Draw& w, uint32_t stream) {
  float u[4];
  block(w, stream, u);
  return (((u[0] + u[1]) + (u[2] + u[3])) - 2.0f) * 1.7320508f;
}
DEV float usym(float u, float b) { return ((b - (-b)) * u) + (-b); }

struct Quat { float x, y, z, w; };
struct Mat3 { float m[3][3]; };
DEV Quat qmul(const Quat a, const Quat b) {
  Quat q;
  q.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
  q.y = ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x;
  q.z = ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w;
  q.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
  return q;
}
DEV Mat3 matrix(const Quat q) {
  Mat3 R;
  R.m[0][0] = 1.0f - 2.0f * (q.y * q.y + q.z * q.z); R.m[0][1] = 2.0f * (q.x * q.y - q.w * q.z); R.m[0][2] = 2.0f * (q.x * q.z + q.w * q.y);
  R.m[1][0] = 2.0f * (q.x * q.y + q.w * q.z); R.m[1][1] = 1.0f - 2.0f * (q.x * q.x + q.z * q.z); R.m[1][2] = 2.0f * (q.y * q.z - q.w * q.x);
  R.m[2][0] = 2.0f * (q.x * q.z - q.w * q.y); R.m[2][1] = 2.0f * (q.y * q.z + q.w * q.x); R.m[2][2] = 1.0f - 2.0f * (q.x * q.x + q.y * q.y);
  return R;
}

// the latency ring of one unit: `ring` (L, C).  Reads its slot before it writes; the slot read (D >= 1) is never the one written.
template <int C>
DEV void latency(float* ring, int L, int h, int D, bool rs, const float (&m)[C], float (&o)[C]) {
  int slot = h - D;
  if (slot < 0) slot += L;
  // the slot is loaded whatever D is and the select is between values: a select between m and a conditional load becomes a
  // load from a selected address, and m lands on the stack
  const bool direct = rs || D == 0;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const float old = ring[slot * C + c];
    o[c] = direct ? m[c] : old;
  }
  if (rs) {
    for (int k = 0; k < L; k++)
#pragma unroll
      for (int c = 0; c < C; c++) ring[k * C + c] = m[c];
  } else {
#pragma unroll
    for (int c = 0; c < C; c++) ring[h * C + c] = m[c];
  }
}

DEV void imu_unit(const ProArgs& A, int e, int i, const Draw& w, bool rs, int h, int D, float* orow) {
  // the mounting: a select over the (at most four) IMUs by value, so that the table stays in scalar registers
  int b = A.imu_body[0];
  float ps[3] = {A.imu_pos[0][0], A.imu_pos[0][1], A.imu_pos[0][2]};
  Quat qs = {A.imu_quat[0][0], A.imu_quat[0][1], A.imu_quat[0][2], A.imu_quat[0][3]};
#pragma unroll
  for (int k = 1; k < SHF_PROPRIO_MAX_IMUS; k++)
    if (i == k) {
      b = A.imu_body[k];
      ps[0] = A.imu_pos[k][0]; ps[1] = A.imu_pos[k][1]; ps[2] = A.imu_pos[k][2];
      qs = Quat{A.imu_quat[k][0], A.imu_quat[k][1], A.imu_quat[k][2], A.imu_quat[k][3]};
    }
  const float* bs = A.body + (long long)e * A.body_env + (long long)b * A.body_row;
  const Quat qb = {bs[3], bs[4], bs[5], bs[6]};
  const float vb[3] = {bs[7], bs[8], bs[9]}, wb[3] = {bs[10], bs[11], bs[12]};
  const Mat3 R = matrix(qmul(qb, qs)), Rb = matrix(qb);
  float arm[3], vs[3];
#pragma unroll
  for (int a = 0; a < 3; a++) arm[a] = (Rb.m[a][0] * ps[0] + Rb.m[a][1] * ps[1]) + Rb.m[a][2] * ps[2];
  vs[0] = vb[0] + (wb[1] * arm[2] - wb[2] * arm[1]);
  vs[1] = vb[1] + (wb[2] * arm[0] - wb[0] * arm[2]);
  vs[2] = vb[2] + (wb[0] * arm[1] - wb[1] * arm[0]);
  float* st = A.imu + ((long long)e * A.I + i) * (9 + 6 * A.L);
  const uint32_t S = PRO_STREAM_IMU + 16u * (uint32_t)i;
  const float sg = A.params[0], sa = A.params[1], wg = A.params[2], wa = A.params[3];
  float vp[3], bg[3], ba[3];
  if (rs) {
    float ug[4], ua[4];
    block(w, S + 12u, ug);
    block(w, S + 13u, ua);
    const float b0g = A.params[4], b0a = A.params[5];
#pragma unroll
    for (int a = 0; a < 3; a++) { bg[a] = usym(ug[a], b0g); ba[a] = usym(ua[a], b0a); vp[a] = vs[a]; }
  } else {
#pragma unroll
    for (int a = 0; a < 3; a++) { vp[a] = st[a]; bg[a] = st[3 + a]; ba[a] = st[6 + a]; }
  }
  float m[6], accw[3];
#pragma unroll
  for (int a = 0; a < 3; a++) accw[a] = ((vs[a] - vp[a]) * A.inv_dt) - A.g[a];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float gw = (R.m[0][a] * wb[0] + R.m[1][a] * wb[1]) + R.m[2][a] * wb[2];
    const float aw = (R.m[0][a] * accw[0] + R.m[1][a] * accw[1]) + R.m[2][a] * accw[2];
    m[a] = (gw + bg[a]) + (sg * gauss(w, S + (uint32_t)a));
    m[3 + a] = (aw + ba[a]) + (sa * gauss(w, S + 3u + (uint32_t)a));
  }
  float o[6];
  latency<6>(st + 9, A.L, h, D, rs, m, o);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    st[a] = vs[a];
    st[3 + a] = bg[a] + (wg * gauss(w, S + 6u + (uint32_t)a));
    st[6 + a] = ba[a] + (wa * gauss(w, S + 9u + (uint32_t)a));
    orow[i * 3 + a] = o[a];
    orow[A.I * 3 + i * 3 + a] = o[3 + a];
  }
}

DEV void enc_unit(const ProArgs& A, int e, int d, const Draw& w, bool rs, int h, int D, float* orow) {
  const float* ds = A.dof + (long long)e * A.dof_env + (long long)d * A.dof_row;
  const float q = ds[0], qd = ds[1];
  float* st = A.enc + ((long long)e * A.nd + d) * (2 + 2 * A.L);
  const uint32_t S = PRO_STREAM_ENC + 4u * (uint32_t)d;
  float off;
  if (rs) {
    float u[4];
    block(w, S + 2u, u);
    off = usym(u[0], A.params[8]);
    st[0] = off;
  } else {
    off = st[0];
  }
  const float r = A.params[9], inv_r = A.params[10];
  float x = (q + off) + (A.params[6] * gauss(w, S));
  if (r > 0.0f) x = r * rintf(x * inv_r);
  float m[2];
  m[0] = x;
  if (A.vmode == SHF_PROPRIO_VEL_DIFFERENCE) {
    const float prev = rs ? x : st[1];
    m[1] = (x - prev) * A.inv_dt;
  } else {
    m[1] = qd + (A.params[7] * gauss(w, S + 1u));
  }
  float o[2];
  latency<2>(st + 2, A.L, h, D, rs, m, o);
  st[1] = x;
  orow[6 * A.I + d] = o[0];
  orow[6 * A.I + A.nd + d] = o[1];
}

DEV void foot_unit(const ProArgs& A, int e, int f, bool rs, int h, int D, float* orow) {
  int b = A.foot_body[0];
#pragma unroll
  for (int k = 1; k < SHF_PROPRIO_MAX_FEET; k++) b = f == k ? A.foot_body[k] : b;
  const float* cf = A.contact + (long long)e * A.con_env + (long long)b * A.con_row;
  const float fx = cf[0], fy = cf[1], fz = cf[2];
  const float s = A.cmode == SHF_PROPRIO_CONTACT_Z ? fz * fabsf(fz) : (fx * fx + fy * fy) + fz * fz;
  float* st = A.foot + ((long long)e * A.F + f) * (5 + 6 * A.L);
  const bool p = rs ? false : st[0] != 0.0f;
  float air = rs ? 0.0f : st[1], con = rs ? 0.0f : st[2], lair = rs ? 0.0f : st[3], lcon = rs ? 0.0f : st[4];
  const bool on = s > A.params[11] ? true : (s < A.params[12] ? false : p);
  const bool first = on && !p && !rs, left = p && !on;
  if (first) lair = air + A.dt;
  if (left) lcon = con + A.dt;
  air = on ? 0.0f : air + A.dt;
  con = on ? con + A.dt : 0.0f;
  const float m[6] = {on ? 1.0f : 0.0f, first ? 1.0f : 0.0f, air, con, lair, lcon};
  float o[6];
  latency<6>(st + 5, A.L, h, D, rs, m, o);
  st[0] = m[0]; st[1] = air; st[2] = con; st[3] = lair; st[4] = lcon;
  float* of = orow + 6 * A.I + 2 * A.nd;
#pragma unroll
  for (int c = 0; c < 6; c++) of[c * A.F + f] = o[c];
  if (A.sw) {
    unsigned char* sw = A.sw + (long long)e * 2 * A.F;
    sw[f] = o[0] != 0.0f;
    sw[A.F + f] = o[1] != 0.0f;
  }
}

__global__ void __launch_bounds__(PRO_T) k_proprioception(ProArgs A) {
  const int cls = blockIdx.y;
  const int per = cls == 0 ? A.I : (cls == 1 ? A.nd : A.F);        // units of this class per env
  const long long r = (long long)blockIdx.x * PRO_T + threadIdx.x;
  if (r >= (long long)A.n * per) return;
  const int e = (int)(r / per), j = (int)(r - (long long)e * per);
  const int U = A.I + A.nd + A.F, u = (cls == 0 ? 0 : (cls == 1 ? A.I : A.I + A.nd)) + j;
  int* cnt = A.counter + ((long long)e * U + u) * 2;
  const uint32_t c = (uint32_t)cnt[0];
  const int h = cnt[1];
  const bool rs = c == 0u || (A.reset != nullptr && A.reset[e] != 0);
  const int D = min(max(A.delay[(long long)e * 3 + cls], 0), A.maxd);
  const Draw w = {A.k0, A.k1, c, A.gids ? A.gids[e] : A.gid0 + e};
  float* orow = A.out + (long long)e * (6 * A.I + 2 * A.nd + 6 * A.F);
  if (cls == 0) imu_unit(A, e, j, w, rs, h, D, orow);
  else if (cls == 1) enc_unit(A, e, j, w, rs, h, D, orow);
  else foot_unit(A, e, j, rs, h, D, orow);
  cnt[0] = (int)(c + 1u);
  cnt[1] = h + 1 == A.L ? 0 : h + 1;
}

}  // namespace

extern "C" int shf_proprioception_step(const float* body_state, int64_t body_env_stride, int64_t body_row_stride,
                                       const float* dof_state, int64_t dof_env_stride, int64_t dof_row_stride, const float* contact,
                                       int64_t contact_env_stride, int64_t contact_row_stride, const uint8_t* reset_or_null,
                                       const ShfProprioConfig* config, const float* params, const int32_t* delay, const int64_t* global_ids_or_null,
                                       int32_t* counter,
                                       float* imu_state, float* enc_state, float* foot_state, int32_t n, int32_t num_bodies,
                                       int32_t num_dof, float* out, uint8_t* switch_out_or_null, void* stream) {
  if (!config) return shf_set_error("shf_proprioception_step: null config");
  const ShfProprioConfig& K = *config;
  if (K.num_imus < 0 || K.num_imus > SHF_PROPRIO_MAX_IMUS) return shf_set_error("shf_proprioception_step: more than 4 IMUs (num_imus outside 0..4)");
  if (K.num_feet < 0 || K.num_feet > SHF_PROPRIO_MAX_FEET) return shf_set_error("shf_proprioception_step: more than 8 feet (num_feet outside 0..8)");
  if (K.slots < 1 || K.slots > SHF_PROPRIO_MAX_SLOTS) return shf_set_error("shf_proprioception_step: slots outside 1..8");
  if (K.max_delay < 0 || K.max_delay >= K.slots) return shf_set_error("shf_proprioception_step: a delay of slots or more (max_delay outside 0..slots-1)");
  if (!(K.dt > 0.0f) || !(K.inv_dt > 0.0f)) return shf_set_error("shf_proprioception_step: dt must be positive");
  if (n < 1) return shf_set_error("shf_proprioception_step: n must be at least 1");
  if (num_dof < 1 || num_dof > SHF_MAX_DOFS) return shf_set_error("shf_proprioception_step: num_dof outside 1..SHF_MAX_DOFS");
  if (num_bodies < 1) return shf_set_error("shf_proprioception_step: num_bodies must be at least 1");
  for (int i = 0; i < K.num_imus; i++)
    if (K.imu_body[i] < 0 || K.imu_body[i] >= num_bodies) return shf_set_error("shf_proprioception_step: an IMU's body index outside 0..num_bodies-1");
  for (int f = 0; f < K.num_feet; f++)
    if (K.foot_body[f] < 0 || K.foot_body[f] >= num_bodies) return shf_set_error("shf_proprioception_step: a foot's body index outside 0..num_bodies-1");
  if (K.contact_mode != SHF_PROPRIO_CONTACT_NORM && K.contact_mode != SHF_PROPRIO_CONTACT_Z) return shf_set_error("shf_proprioception_step: unknown contact_mode");
  if (K.velocity_mode != SHF_PROPRIO_VEL_DIRECT && K.velocity_mode != SHF_PROPRIO_VEL_DIFFERENCE) return shf_set_error("shf_proprioception_step: unknown velocity_mode");
  if (!dof_state || !params || !delay || !counter || !enc_state || !out) return shf_set_error("shf_proprioception_step: null tensor");
  if (K.num_imus > 0 && (!body_state || !imu_state)) return shf_set_error("shf_proprioception_step: null tensor (IMUs need body_state and imu_state)");
  if (K.num_feet > 0 && (!contact || !foot_state)) return shf_set_error("shf_proprioception_step: null tensor (feet need contact and foot_state)");
  if (dof_row_stride < 2 || (K.num_imus > 0 && body_row_stride < 13) || (K.num_feet > 0 && contact_row_stride < 3))
    return shf_set_error("shf_proprioception_step: a row stride shorter than the row");
  ProArgs A = {};
  A.body = body_state; A.body_env = body_env_stride; A.body_row = body_row_stride;
  A.dof = dof_state; A.dof_env = dof_env_stride; A.dof_row = dof_row_stride;
  A.contact = contact; A.con_env = contact_env_stride; A.con_row = contact_row_stride;
  A.reset = reset_or_null; A.params = params; A.delay = delay; A.gids = (const long long*)global_ids_or_null;
  A.counter = counter; A.imu = imu_state; A.enc = enc_state; A.foot = foot_state;
  A.out = out; A.sw = switch_out_or_null;
  A.n = n; A.nd = num_dof; A.I = K.num_imus; A.F = K.num_feet; A.L = K.slots; A.maxd = K.max_delay;
  A.cmode = K.contact_mode; A.vmode = K.velocity_mode;
  for (int i = 0; i < SHF_PROPRIO_MAX_IMUS; i++) {
    A.imu_body[i] = i < K.num_imus ? K.imu_body[i] : 0;
    for (int a = 0; a < 3; a++) A.imu_pos[i][a] = K.imu_pos[i][a];
    for (int a = 0; a < 4; a++) A.imu_quat[i][a] = K.imu_quat[i][a];
  }
  for (int f = 0; f < SHF_PROPRIO_MAX_FEET; f++) A.foot_body[f] = f < K.num_feet ? K.foot_body[f] : 0;
  for (int a = 0; a < 3; a++) A.g[a] = K.gravity[a];
  A.dt = K.dt; A.inv_dt = K.inv_dt;
  A.k0 = K.seed_lo; A.k1 = K.seed_hi; A.gid0 = K.env_id_offset;
  const int widest = K.num_imus > num_dof ? (K.num_imus > K.num_feet ? K.num_imus : K.num_feet) : (num_dof > K.num_feet ? num_dof : K.num_feet);
  const unsigned blocks = (unsigned)(((long long)n * widest + PRO_T - 1) / PRO_T);
  hipLaunchKernelGGL(k_proprioception, dim3(blocks, 3), dim3(PRO_T), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_proprioception_step: launch failed");
}
