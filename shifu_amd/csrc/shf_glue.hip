// shf_glue.hip -- the library glue of the hook-compatible path as single launches (K3 base_frame_state,
// K4 sample_heights, K7 episode log, K9 history shift).  On the path a user edits -- ShifuVecEnv with
// torch hooks -- these were ~60 small torch launches per vec-step of LIBRARY code (LeggedRobot.post_step,
// TerrainGymEnv.get_heights, HistoryRecorder, ShifuVecEnv.log_info / compute_reward); the hooks themselves stay torch.
// Same arithmetic as the fused kernels' in-kernel versions and as the oracle's glue_* functions (tests/test_gpu_glue.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"
#include "shf_quat.h"

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns
#define GLUE_LAUNCH_OK(who) (hipGetLastError() == hipSuccess ? 0 : shf_set_error(std::string(who) + ": launch failed"))

// isaacgym.torch_utils.quat_rotate_inverse (xyzw), the operations of the oracle's quat_rotate_inverse in its order
static __device__ __forceinline__ void qri(const float* q, const float* v, float* o) {
  const float w = q[3];
  const float s = 2.0f * (w * w) - 1.0f;
  const float cx = q[1] * v[2] - q[2] * v[1], cy = q[2] * v[0] - q[0] * v[2], cz = q[0] * v[1] - q[1] * v[0];
  const float d = q[0] * v[0] + q[1] * v[1] + q[2] * v[2];
  o[0] = v[0] * s - cx * w * 2.0f + q[0] * d * 2.0f;
  o[1] = v[1] * s - cy * w * 2.0f + q[1] * d * 2.0f;
  o[2] = v[2] * s - cz * w * 2.0f + q[2] * d * 2.0f;
}

// K3 -- LeggedRobot.post_step (shifu/units/robot.py:222-229)
__global__ void k_base_frame_state(const float* root_state, const int64_t* root_idx, int64_t num_rows, int n, int up_axis,
                                   float* lin, float* ang, float* pg, float* gvec) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t row = root_idx ? root_idx[e] : (int64_t)e;
  if (row < 0 || row >= num_rows) return;
  const float* r = root_state + row * 13;
  const float q[4] = {r[3], r[4], r[5], r[6]}, lv[3] = {r[7], r[8], r[9]}, av[3] = {r[10], r[11], r[12]};
  float gv[3] = {0.0f, 0.0f, 0.0f}, a[3], b[3], c[3];
  gv[up_axis] = -1.0f;
  qri(q, lv, a); qri(q, av, b); qri(q, gv, c);
#pragma unroll
  for (int k = 0; k < 3; k++) { lin[3 * e + k] = a[k]; ang[3 * e + k] = b[k]; pg[3 * e + k] = c[k]; gvec[3 * e + k] = gv[k]; }
}

// K4 -- TerrainGymEnv.get_heights (shifu/gym/isaac_gym.py:412-433): one thread per (env, point)
__global__ void k_get_heights(ShfTerrain t, const int16_t* h, const float* root_state, const int64_t* root_idx, int64_t num_rows,
                              const float* hpoints, int n, int P, float* out) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long long)n * P) return;
  const int e = (int)(tid / P), i = (int)(tid % P);
  const int64_t row = root_idx ? root_idx[e] : (int64_t)e;
  if (row < 0 || row >= num_rows) return;
  const float* r = root_state + row * 13;
  float qz = r[5], qw = r[6];
  const float nr = sqrtf(qz * qz + qw * qw);
  const float nrm = nr > 1e-9f ? nr : 1e-9f;
  qz = qz / nrm; qw = qw / nrm;
  const float bx = hpoints[2 * i], by = hpoints[2 * i + 1];
  float hh = 0.0f;
  if (t.rows > 0) {
    const float tx = (-qz * by) * 2.0f, ty = (qz * bx) * 2.0f;
    float px = bx + qw * tx + (-qz * ty) + r[0];
    float py = by + qw * ty + (qz * tx) + r[1];
    px += t.border; py += t.border;
    // `points / horizontal_scale` as torch evaluates it on a GPU tensor with a Python-float divisor: x * (1 / s)
    // (ATen BinaryDivTrueKernel.cu); tests/test_gpu_glue.py holds this to the torch expression on cell-boundary points
    const float inv_hs = 1.0f / t.hscale;
    int ix = (int)truncf(px * inv_hs), iy = (int)truncf(py * inv_hs);
    ix = ix < 0 ? 0 : ix; ix = ix > t.rows - 2 ? t.rows - 2 : ix;
    iy = iy < 0 ? 0 : iy; iy = iy > t.cols - 2 ? t.cols - 2 : iy;
    const int16_t* p0 = h + (size_t)ix * t.cols + iy;
    const int16_t h1 = p0[0], h2 = p0[t.cols], h3 = p0[1];
    int16_t hm = h1 < h2 ? h1 : h2;
    hm = hm < h3 ? hm : h3;
    hh = (float)hm * t.vscale;
  }
  out[tid] = hh;
}

// K9 -- HistoryRecorder.add / reset_idx (shifu/utils/train.py:12-17): (rows, H) with the newest sample at column 0
__global__ void k_history_add(float* hist, const float* x, long long rows, int H) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  float* o = hist + j * H;
  for (int hh = H - 1; hh >= 1; hh--) o[hh] = o[hh - 1];
  o[0] = x[j];
}
__global__ void k_rows_fill_indexed(float* buf, const int64_t* idx, int nidx, long long num_rows, int row_words, float value) {
  const int i = blockIdx.x;
  if (i >= nidx) return;
  const int64_t r = idx[i];
  if (r < 0 || r >= num_rows) return;
  for (int k = threadIdx.x; k < row_words; k += blockDim.x) buf[r * row_words + k] = value;
}

// K7 -- ShifuVecEnv.log_info (shifu/gym/env.py:149-158) and the buffer part of reset_idx (env.py:114-130) for the env
// ids of one reset: per key mean(sums[ids]) / T, sums[ids] = 0.  Exact: 2^-20 fixed-point integer sums (the fused
// kernels' statistics and oracle a1_stats), so the result does not depend on the order of the atomics.
#define GLUE_MAX_KEYS 16
struct GlueKeys { float* p[GLUE_MAX_KEYS]; };
// (ep_len / reset_buf / history: the rest of ShifuVecEnv.reset_idx's buffer writes for the same ids, shf_reset_bookkeeping; all NULL
// for shf_episode_log)
__global__ void k_episode_log(GlueKeys sums, int K, const int64_t* ids, int nids, long long n, float T, unsigned long long* acc,
                              float* out, int64_t* ep_len, void* reset_buf, int reset_bytes, float* history, int hist_words) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nids) {
    const int64_t e = ids[i];
    if (e >= 0 && e < n) {
      if (ep_len) ep_len[e] = 0;
      if (reset_buf) {
        if (reset_bytes == 8) reinterpret_cast<int64_t*>(reset_buf)[e] = 1;
        else reinterpret_cast<uint8_t*>(reset_buf)[e] = 1;
      }
      if (history)
        for (int k = 0; k < hist_words; k++) history[e * hist_words + k] = 0.0f;
      for (int k = 0; k < K; k++) {
        const float v = sums.p[k][e];
        sums.p[k][e] = 0.0f;
        const long long f = (long long)rintf(v * 1048576.0f);
        if (f != 0) atomicAdd(&acc[k], (unsigned long long)f);
      }
    }
  }
  __syncthreads();
  __shared__ unsigned ticket;
  if (threadIdx.x == 0) {
    __threadfence();
    ticket = (unsigned)atomicAdd(&acc[GLUE_MAX_KEYS], 1ull);
  }
  __syncthreads();
  if (ticket != gridDim.x - 1) return;
  // last block: every block's additions are visible (each fenced before taking its ticket)
  if ((int)threadIdx.x < K) {
    const long long tot = (long long)atomicExch(&acc[threadIdx.x], 0ull);
    const float sum = (float)tot * (1.0f / 1048576.0f), c = (float)nids;
    out[threadIdx.x] = c > 0.0f ? sum / c / T : 0.0f;
  }
  if (threadIdx.x == 0) atomicExch(&acc[GLUE_MAX_KEYS], 0ull);
}

// ShifuVecEnv.compute_reward's accumulation (env.py:180-185): rew = r_0 + r_1 + ... (that order), sums_k += r_k
struct GlueConstKeys { const float* p[GLUE_MAX_KEYS]; };
__global__ void k_reward_accumulate(GlueConstKeys r, GlueKeys sums, int K, long long n, float* rew) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float acc = 0.0f;
  for (int k = 0; k < K; k++) {
    const float v = r.p[k][e];
    sums.p[k][e] += v;
    acc += v;
  }
  rew[e] = acc;
}

// Robot._reset_dof_state (shifu/units/robot.py:74-86) before its two indexed commits: targets and positions to the
// defaults, velocities to zero, and the int32 actor indices the commits take -- one block per env id
__global__ void k_reset_dof_rows(float* dof_state, float* dof_targets, const float* default_pos, const int64_t* env_ids, int nids,
                                 long long num_envs, int nd, const int64_t* root_idx, int32_t* actor_ids_out) {
  const int i = blockIdx.x;
  if (i >= nids) return;
  const int64_t e = env_ids[i];
  if (e < 0 || e >= num_envs) { if (threadIdx.x == 0 && actor_ids_out) actor_ids_out[i] = -1; return; }
  for (int d = threadIdx.x; d < nd; d += blockDim.x) {
    const float q0 = default_pos[d];
    dof_targets[e * nd + d] = q0;
    dof_state[(e * nd + d) * 2] = q0;
    dof_state[(e * nd + d) * 2 + 1] = 0.0f;
  }
  if (threadIdx.x == 0 && actor_ids_out) actor_ids_out[i] = (int32_t)(root_idx ? root_idx[e] : e);
}

extern "C" int shf_reset_dof_rows(float* dof_state, float* dof_targets, const float* default_dof_pos, const int64_t* env_ids,
                                  int32_t n_ids, int64_t num_envs, int32_t num_dof, const int64_t* root_idx_or_null,
                                  int32_t* actor_ids_out_or_null, void* stream) {
  if (!dof_state || !dof_targets || !default_dof_pos || (!env_ids && n_ids > 0)) return shf_set_error("shf_reset_dof_rows: null tensor");
  if (n_ids <= 0 || num_dof <= 0) return 0;
  hipLaunchKernelGGL(k_reset_dof_rows, dim3(n_ids), dim3(32), 0, (hipStream_t)stream, dof_state, dof_targets, default_dof_pos, env_ids,
                     (int)n_ids, (long long)num_envs, (int)num_dof, root_idx_or_null, actor_ids_out_or_null);
  return GLUE_LAUNCH_OK("shf_reset_dof_rows");
}

// K10 -- ArmRobot.inverse_kinematics (shifu/units/robot.py:162-182; shifu/utils/torch_utils.py:12-58): damped least
// squares u = J^T (J J^T + lambda^2 I)^-1 dpose on the end effector's (6, nd) Jacobian block, dof_pos + u; the 6x6
// system by LDL^T in packed storage -- the arithmetic of the fused ABB step and of the oracle's glue_ik_dls
#define GSYM(i, j) ((i) * 6 - ((i) * ((i) - 1)) / 2 + ((j) - (i)))
static __device__ __forceinline__ float glue_rcp_spec(float x) {   // the oracle's rcp_spec (csrc/shf_device.h has the same)
  float y = __uint_as_float(0x7EF311C7u - __float_as_uint(x));
#pragma unroll
  for (int k = 0; k < 3; k++) { const float e = fmaf(-x, y, 1.0f); y = fmaf(y, e, y); }
  return y;
}
static __device__ __forceinline__ void glue_ldlt_solve6(const float* IA, const float* pA, float* x) {   // IA x = -pA
  float Lm[6][6], Dg[6], iD[6], y[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    float d = IA[GSYM(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) d = fmaf(-(Lm[j][k] * Lm[j][k]), Dg[k], d);
    Dg[j] = d;
    const float id = glue_rcp_spec(d);
    iD[j] = id;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      float v = IA[GSYM(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) v = fmaf(-(Lm[i][k] * Lm[j][k]), Dg[k], v);
      Lm[i][j] = v * id;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float v = -pA[i];
#pragma unroll
    for (int k = 0; k < i; k++) v = fmaf(-Lm[i][k], y[k], v);
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) y[i] = y[i] * iD[i];
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    float v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) v = fmaf(-Lm[k][i], x[k], v);
    x[i] = v;
  }
}
__global__ void k_ik_dls(const float* j_ee, long long j_stride, const float* dof_pos, int dof_stride, const float* ee_pose,
                         long long ee_stride, const float* goal_pose, int n, int nd, float damping, float* out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float* J = j_ee + (long long)e * j_stride;
  const float* ee = ee_pose + (long long)e * ee_stride;
  const float* gp = goal_pose + (long long)e * 7;
  float dpose[6], cc[4], qr[4];
#pragma unroll
  for (int k = 0; k < 3; k++) dpose[k] = gp[k] - ee[k];
  cc[0] = -ee[3]; cc[1] = -ee[4]; cc[2] = -ee[5]; cc[3] = ee[6];
  const float tq[4] = {gp[3], gp[4], gp[5], gp[6]};
  shf_quat_mul(tq, cc, qr);
  const float sg = qr[3] > 0.0f ? 1.0f : (qr[3] < 0.0f ? -1.0f : 0.0f);
#pragma unroll
  for (int k = 0; k < 3; k++) dpose[3 + k] = qr[k] * sg;
  float Am[21], neg[6], x[6];
  const float lam2 = damping * damping;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) {
      float acc = J[i * nd] * J[j * nd];
      for (int d = 1; d < nd; d++) acc = fmaf(J[i * nd + d], J[j * nd + d], acc);
      Am[GSYM(i, j)] = (i == j) ? acc + lam2 : acc;
    }
#pragma unroll
  for (int k = 0; k < 6; k++) neg[k] = -dpose[k];
  glue_ldlt_solve6(Am, neg, x);
  for (int d = 0; d < nd; d++) {
    float u = J[d] * x[0];
#pragma unroll
    for (int k = 1; k < 6; k++) u = fmaf(J[k * nd + d], x[k], u);
    out[(long long)e * nd + d] = dof_pos[(long long)e * nd * dof_stride + d * dof_stride] + u;
  }
}

extern "C" int shf_ik_dls(const float* j_ee, int64_t j_env_stride, const float* dof_pos, int32_t dof_elem_stride,
                          const float* ee_pose, int64_t ee_env_stride, const float* goal_pose, int32_t n, int32_t num_dof,
                          float damping, float* dof_targets_out, void* stream) {
  if (!j_ee || !dof_pos || !ee_pose || !goal_pose || !dof_targets_out) return shf_set_error("shf_ik_dls: null tensor");
  if (n <= 0 || num_dof <= 0) return 0;
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_ik_dls: too many dofs");
  hipLaunchKernelGGL(k_ik_dls, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, j_ee, (long long)j_env_stride, dof_pos,
                     (int)dof_elem_stride, ee_pose, (long long)ee_env_stride, goal_pose, (int)n, (int)num_dof, damping,
                     dof_targets_out);
  return GLUE_LAUNCH_OK("shf_ik_dls");
}

// K11 -- ArmRobot.operational_space_control: the torque-level controller of Isaac Gym's arm examples,
//   tau = J^T A^-1 (kp (.) e - kd (.) J qd),  A = J M^-1 J^T + damping^2 I,
// plus, with q_rest and nd > 6, the posture term M u - J^T A^-1 J u (u = kp_null wrap_to_pi(q_rest - q) - kd_null qd), which
// shares the one 6x6 solve: tau = J^T A^-1 (a - J u) + M u.  Then + bias, then the effort clamp.
// One thread per env, as k_ik_dls.  M^-1 J^T by LDL^T of M (any nd <= SHF_MAX_DOFS): the factor, X = M^-1 J^T, J and u live in
// LDS, word k of thread t at [k * T + t] (a thread touches its own words only: no barrier, no bank conflict); the 6x6 system in
// registers by the packed LDL^T of k_ik_dls.  The host sizes the block (T <= 64 threads) so that the LDS stays within 48 KiB.
struct OscArgs {
  const float* j_ee; long long j_stride;
  const float* mass; const float* bias;
  const float* dof; int dof_stride;
  const float* ee; long long ee_stride;
  const float* goal; const float* kp6; const float* kd6;
  float lam2;
  const float* q_rest; float kp_null, kd_null;
  const float* limit;
  int n, nd;
  float* out;
};
static int osc_words(int nd) { return nd * (nd + 1) / 2 + nd + 6 * nd + nd + 6 * nd; }
__global__ void k_osc(OscArgs A) {
  extern __shared__ float osc_lds[];
  const int T = blockDim.x, t = threadIdx.x, nd = A.nd;
  const int e = blockIdx.x * T + t;
  if (e >= A.n) return;
  float* Lw = osc_lds + t;                       // LDL^T of M: L below the diagonal, D on it, row-packed lower triangle
  float* iD = Lw + (nd * (nd + 1) / 2) * T;      // 1 / D
  float* Xw = iD + nd * T;                       // X[d][c]
  float* Uw = Xw + 6 * nd * T;                   // u[d]
  float* Jw = Uw + nd * T;                       // J[k][d]
#define OSC_L(i, j) Lw[((i) * ((i) + 1) / 2 + (j)) * T]
#define OSC_X(d, c) Xw[((d) * 6 + (c)) * T]
#define OSC_J(k, d) Jw[((k) * nd + (d)) * T]
  const float* J = A.j_ee + (long long)e * A.j_stride;
  const float* Mg = A.mass + (long long)e * nd * nd;
  const float* ds = A.dof + (long long)e * nd * A.dof_stride;
  const float* ee = A.ee + (long long)e * A.ee_stride;
  const float* gp = A.goal + (long long)e * 7;
  for (int k = 0; k < 6 * nd; k++) Jw[k * T] = J[k];
  float a[6], cc[4], qr[4];
#pragma unroll
  for (int k = 0; k < 3; k++) a[k] = gp[k] - ee[k];
  cc[0] = -ee[3]; cc[1] = -ee[4]; cc[2] = -ee[5]; cc[3] = ee[6];
  const float tq[4] = {gp[3], gp[4], gp[5], gp[6]};
  shf_quat_mul(tq, cc, qr);
  const float sg = qr[3] > 0.0f ? 1.0f : (qr[3] < 0.0f ? -1.0f : 0.0f);
#pragma unroll
  for (int k = 0; k < 3; k++) a[3 + k] = qr[k] * sg;
  // a = kp (.) e - kd (.) J qd  [- J u]
  const bool posture = A.q_rest && nd > 6;
  float xd[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, ju[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int d = 0; d < nd; d++) {
    const float q = ds[d * A.dof_stride], qd = ds[d * A.dof_stride + 1];
    float u = 0.0f;
    if (posture) {
      float x = A.q_rest[d] - q;
      x = fmaf(-6.283185307179586f, rintf(x * 0.15915494309189535f), x);   // wrap_to_pi
      u = A.kp_null * x - A.kd_null * qd;
      Uw[d * T] = u;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) { xd[k] = fmaf(OSC_J(k, d), qd, xd[k]); ju[k] = fmaf(OSC_J(k, d), u, ju[k]); }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) a[k] = A.kp6[k] * a[k] - A.kd6[k] * xd[k] - ju[k];
  // M = L D L^T
  for (int j = 0; j < nd; j++) {
    float dj = Mg[j * nd + j];
    for (int k = 0; k < j; k++) { const float v = OSC_L(j, k); dj = fmaf(-(v * v), OSC_L(k, k), dj); }
    OSC_L(j, j) = dj;
    const float id = glue_rcp_spec(dj);
    iD[j * T] = id;
    for (int i = j + 1; i < nd; i++) {
      float v = Mg[i * nd + j];
      for (int k = 0; k < j; k++) v = fmaf(-(OSC_L(i, k) * OSC_L(j, k)), OSC_L(k, k), v);
      OSC_L(i, j) = v * id;
    }
  }
  // X = M^-1 J^T, column by column
  for (int c = 0; c < 6; c++) {
    for (int i = 0; i < nd; i++) {
      float v = OSC_J(c, i);
      for (int k = 0; k < i; k++) v = fmaf(-OSC_L(i, k), OSC_X(k, c), v);
      OSC_X(i, c) = v;
    }
    for (int i = 0; i < nd; i++) OSC_X(i, c) = OSC_X(i, c) * iD[i * T];
    for (int i = nd - 1; i >= 0; i--) {
      float v = OSC_X(i, c);
      for (int k = i + 1; k < nd; k++) v = fmaf(-OSC_L(k, i), OSC_X(k, c), v);
      OSC_X(i, c) = v;
    }
  }
  // A = (J X + (J X)^T) / 2 + damping^2 I, packed
  float Am[21], neg[6], F[6];
#pragma unroll
  for (int k = 0; k < 21; k++) Am[k] = 0.0f;
  for (int d = 0; d < nd; d++) {
    float Jd[6], Xd[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { Jd[k] = OSC_J(k, d); Xd[k] = OSC_X(d, k); }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = i; j < 6; j++) Am[GSYM(i, j)] = fmaf(Jd[j], Xd[i], fmaf(Jd[i], Xd[j], Am[GSYM(i, j)]));
  }
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) Am[GSYM(i, j)] = (i == j) ? fmaf(0.5f, Am[GSYM(i, j)], A.lam2) : 0.5f * Am[GSYM(i, j)];
#pragma unroll
  for (int k = 0; k < 6; k++) neg[k] = -a[k];
  glue_ldlt_solve6(Am, neg, F);
  for (int d = 0; d < nd; d++) {
    float tau = OSC_J(0, d) * F[0];
#pragma unroll
    for (int k = 1; k < 6; k++) tau = fmaf(OSC_J(k, d), F[k], tau);
    if (posture) {
      float mu = Mg[d * nd] * Uw[0];
      for (int j = 1; j < nd; j++) mu = fmaf(Mg[d * nd + j], Uw[j * T], mu);
      tau += mu;
    }
    if (A.bias) tau += A.bias[(long long)e * nd + d];
    const float lim = A.limit ? A.limit[d] : 0.0f;
    if (lim > 0.0f) tau = tau > lim ? lim : (tau < -lim ? -lim : tau);
    A.out[(long long)e * nd + d] = tau;
  }
#undef OSC_L
#undef OSC_X
#undef OSC_J
}

extern "C" int shf_osc(const float* j_ee, int64_t j_env_stride, const float* mass_matrix, const float* bias_or_null,
                       const float* dof_state, int32_t dof_elem_stride, const float* ee_pose, int64_t ee_env_stride,
                       const float* goal_pose, const float* kp6, const float* kd6, float damping, const float* q_rest_or_null,
                       float kp_null, float kd_null, const float* effort_limit_or_null, int32_t n, int32_t num_dof,
                       float* efforts_out, void* stream) {
  if (!j_ee || !mass_matrix || !dof_state || !ee_pose || !goal_pose || !kp6 || !kd6 || !efforts_out) return shf_set_error("shf_osc: null tensor");
  if (n <= 0 || num_dof <= 0) return 0;
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_osc: too many dofs");
  if (dof_elem_stride < 2) return shf_set_error("shf_osc: dof_state holds position and velocity (element stride >= 2)");
  int T = 64;
  while ((size_t)T * osc_words(num_dof) * 4 > 48 * 1024) T >>= 1;
  OscArgs A = {j_ee, (long long)j_env_stride, mass_matrix, bias_or_null, dof_state, (int)dof_elem_stride, ee_pose, (long long)ee_env_stride,
               goal_pose, kp6, kd6, damping * damping, q_rest_or_null, kp_null, kd_null, effort_limit_or_null, (int)n, (int)num_dof, efforts_out};
  hipLaunchKernelGGL(k_osc, dim3((n + T - 1) / T), dim3(T), (size_t)T * osc_words(num_dof) * 4, (hipStream_t)stream, A);
  return GLUE_LAUNCH_OK("shf_osc");
}

// K12 -- LeggedRobot.foot_impedance_control: Cartesian spring-damper on every foot in the base frame, the legged twin of K11.
// Per foot f, with R the root's rotation and Jl = the dof columns of the foot's linear Jacobian rows (the foot's velocity
// relative to the base):  p = R^T (p_f - p_root),  pd = R^T (Jl qd),  F = R (kp (.) (target - p) - kd (.) pd),  tau += Jl^T F.
// Then + bias[6:] (gravity and Coriolis compensation of the legs), then the effort clamp.
// One thread per env looping over its feet, so end bodies that share an ancestor dof accumulate in one thread; tau (run-time
// sized) lives in LDS, word d of thread t at [d * T + t], as K11's arrays.
struct FootArgs {
  const float* j; long long j_env, j_foot;
  const float* dof; int dof_stride;
  const float* root; long long root_env;
  const float* foot; long long foot_env, foot_stride;
  const float* target; const float* kp3; const float* kd3;
  const float* bias; const float* limit;
  int n, nf, nd;
  float* out;
};
__global__ void k_foot_impedance(FootArgs A) {
  extern __shared__ float foot_lds[];
  const int T = blockDim.x, t = threadIdx.x, nd = A.nd, D = A.nd + 6;
  const int e = blockIdx.x * T + t;
  if (e >= A.n) return;
  float* tau = foot_lds + t;
  const float* ds = A.dof + (long long)e * nd * A.dof_stride;
  const float* rp = A.root + (long long)e * A.root_env;
  for (int d = 0; d < nd; d++) tau[d * T] = 0.0f;
  const float x = rp[3], y = rp[4], z = rp[5], w = rp[6];
  const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y),
                      2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x),
                      2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)};
  const float kp[3] = {A.kp3[0], A.kp3[1], A.kp3[2]}, kd[3] = {A.kd3[0], A.kd3[1], A.kd3[2]};
  for (int f = 0; f < A.nf; f++) {
    const float* J = A.j + (long long)e * A.j_env + (long long)f * A.j_foot + 6;   // linear rows, dof columns
    const float* pf = A.foot + (long long)e * A.foot_env + (long long)f * A.foot_stride;
    const float* tg = A.target + ((long long)e * A.nf + f) * 3;
    float vw[3] = {0.0f, 0.0f, 0.0f};
    for (int d = 0; d < nd; d++) {
      const float qd = ds[d * A.dof_stride + 1];
#pragma unroll
      for (int k = 0; k < 3; k++) vw[k] = fmaf(J[k * D + d], qd, vw[k]);
    }
    const float dw[3] = {pf[0] - rp[0], pf[1] - rp[1], pf[2] - rp[2]};
    float g[3], F[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float p = fmaf(R[6 + k], dw[2], fmaf(R[3 + k], dw[1], R[k] * dw[0]));      // R^T
      const float pd = fmaf(R[6 + k], vw[2], fmaf(R[3 + k], vw[1], R[k] * vw[0]));
      g[k] = kp[k] * (tg[k] - p) - kd[k] * pd;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) F[k] = fmaf(R[3 * k + 2], g[2], fmaf(R[3 * k + 1], g[1], R[3 * k] * g[0]));
    for (int d = 0; d < nd; d++)
      tau[d * T] = fmaf(J[2 * D + d], F[2], fmaf(J[D + d], F[1], fmaf(J[d], F[0], tau[d * T])));
  }
  for (int d = 0; d < nd; d++) {
    float v = tau[d * T];
    if (A.bias) v += A.bias[(long long)e * D + 6 + d];
    const float lim = A.limit ? A.limit[d] : 0.0f;
    if (lim > 0.0f) v = v > lim ? lim : (v < -lim ? -lim : v);
    A.out[(long long)e * nd + d] = v;
  }
}

extern "C" int shf_foot_impedance(const float* j_feet, int64_t j_env_stride, int64_t j_foot_stride, const float* dof_state,
                                  int32_t dof_elem_stride, const float* root_pose, int64_t root_env_stride, const float* foot_pos,
                                  int64_t foot_env_stride, int64_t foot_stride, const float* target, const float* kp3,
                                  const float* kd3, const float* bias_or_null, const float* effort_limit_or_null, int32_t n,
                                  int32_t num_feet, int32_t num_dof, float* efforts_out, void* stream) {
  if (!j_feet || !dof_state || !root_pose || !foot_pos || !target || !kp3 || !kd3 || !efforts_out) return shf_set_error("shf_foot_impedance: null tensor");
  if (n <= 0 || num_dof <= 0) return 0;
  if (num_feet < 0) return shf_set_error("shf_foot_impedance: negative foot count");
  if (num_dof > SHF_MAX_DOFS) return shf_set_error("shf_foot_impedance: too many dofs");
  if (dof_elem_stride < 2) return shf_set_error("shf_foot_impedance: dof_state holds position and velocity (element stride >= 2)");
  const int T = 64;
  FootArgs A = {j_feet, (long long)j_env_stride, (long long)j_foot_stride, dof_state, (int)dof_elem_stride, root_pose, (long long)root_env_stride,
                foot_pos, (long long)foot_env_stride, (long long)foot_stride, target, kp3, kd3, bias_or_null, effort_limit_or_null,
                (int)n, (int)num_feet, (int)num_dof, efforts_out};
  hipLaunchKernelGGL(k_foot_impedance, dim3((n + T - 1) / T), dim3(T), (size_t)T * num_dof * 4, (hipStream_t)stream, A);
  return GLUE_LAUNCH_OK("shf_foot_impedance");
}

extern "C" int shf_base_frame_state(const float* root_state, const int64_t* root_idx_or_null, int64_t num_root_rows, int32_t n,
                                    int32_t up_axis, float* base_lin_vel, float* base_ang_vel, float* projected_gravity,
                                    float* gravity_vec, void* stream) {
  if (!root_state || !base_lin_vel || !base_ang_vel || !projected_gravity || !gravity_vec) return shf_set_error("shf_base_frame_state: null tensor");
  if (n <= 0) return 0;
  if (up_axis < 0 || up_axis > 2) return shf_set_error("shf_base_frame_state: up_axis must be 0, 1 or 2");
  hipLaunchKernelGGL(k_base_frame_state, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, root_state, root_idx_or_null,
                     num_root_rows, (int)n, (int)up_axis, base_lin_vel, base_ang_vel, projected_gravity, gravity_vec);
  return GLUE_LAUNCH_OK("shf_base_frame_state");
}

extern "C" int shf_get_heights(const ShfTerrain* terrain, const int16_t* height_samples, const float* root_state,
                               const int64_t* root_idx_or_null, int64_t num_root_rows, const float* height_points_xy, int32_t n,
                               int32_t num_points, float* out, void* stream) {
  if (!terrain || !root_state || !height_points_xy || !out) return shf_set_error("shf_get_heights: null argument");
  if (terrain->rows > 0 && !height_samples) return shf_set_error("shf_get_heights: height samples not given");
  if (n <= 0 || num_points <= 0) return 0;
  const long long tot = (long long)n * num_points;
  hipLaunchKernelGGL(k_get_heights, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *terrain, height_samples,
                     root_state, root_idx_or_null, num_root_rows, height_points_xy, (int)n, (int)num_points, out);
  return GLUE_LAUNCH_OK("shf_get_heights");
}

extern "C" int shf_history_add(float* history, const float* x, int64_t rows, int32_t num_history, void* stream) {
  if (!history || !x) return shf_set_error("shf_history_add: null tensor");
  if (rows <= 0) return 0;
  if (num_history < 1) return shf_set_error("shf_history_add: num_history must be >= 1");
  hipLaunchKernelGGL(k_history_add, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, history, x, (long long)rows,
                     (int)num_history);
  return GLUE_LAUNCH_OK("shf_history_add");
}

extern "C" int shf_rows_fill_indexed(float* buf, const int64_t* idx, int32_t n_idx, int64_t num_rows, int32_t row_words,
                                     float value, void* stream) {
  if (!buf || (!idx && n_idx > 0)) return shf_set_error("shf_rows_fill_indexed: null tensor");
  if (n_idx <= 0 || row_words <= 0) return 0;
  hipLaunchKernelGGL(k_rows_fill_indexed, dim3(n_idx), dim3(64), 0, (hipStream_t)stream, buf, idx, (int)n_idx, (long long)num_rows,
                     (int)row_words, value);
  return GLUE_LAUNCH_OK("shf_rows_fill_indexed");
}

extern "C" int shf_episode_log(float* const* sums, int32_t num_keys, const int64_t* env_ids, int32_t n_ids, int64_t num_envs,
                               float episode_length_s, int64_t* workspace17, float* out_means, void* stream) {
  if (!sums || !env_ids || !workspace17 || !out_means) return shf_set_error("shf_episode_log: null argument");
  if (num_keys < 1 || num_keys > GLUE_MAX_KEYS) return shf_set_error("shf_episode_log: 1..16 keys");
  if (n_ids <= 0) return 0;
  GlueKeys G{};
  for (int k = 0; k < num_keys; k++) {
    if (!sums[k]) return shf_set_error("shf_episode_log: null sums tensor");
    G.p[k] = sums[k];
  }
  hipLaunchKernelGGL(k_episode_log, dim3((n_ids + 255) / 256), dim3(256), 0, (hipStream_t)stream, G, (int)num_keys, env_ids, (int)n_ids,
                     (long long)num_envs, episode_length_s, reinterpret_cast<unsigned long long*>(workspace17), out_means,
                     (int64_t*)nullptr, (void*)nullptr, 0, (float*)nullptr, 0);
  return GLUE_LAUNCH_OK("shf_episode_log");
}

extern "C" int shf_reset_bookkeeping(float* const* sums, int32_t num_keys, const int64_t* env_ids, int32_t n_ids, int64_t num_envs,
                                     float episode_length_s, int64_t* workspace17, float* out_means, int64_t* episode_length_or_null,
                                     void* reset_buf_or_null, int32_t reset_elem_bytes, float* history_or_null,
                                     int32_t history_row_words, void* stream) {
  if (!sums || !env_ids || !workspace17 || !out_means) return shf_set_error("shf_reset_bookkeeping: null argument");
  if (num_keys < 1 || num_keys > GLUE_MAX_KEYS) return shf_set_error("shf_reset_bookkeeping: 1..16 keys");
  if (reset_buf_or_null && reset_elem_bytes != 1 && reset_elem_bytes != 8)
    return shf_set_error("shf_reset_bookkeeping: reset_buf elements of 1 or 8 bytes");
  if (history_or_null && history_row_words < 1) return shf_set_error("shf_reset_bookkeeping: history_row_words must be >= 1");
  if (n_ids <= 0) return 0;
  GlueKeys G{};
  for (int k = 0; k < num_keys; k++) {
    if (!sums[k]) return shf_set_error("shf_reset_bookkeeping: null sums tensor");
    G.p[k] = sums[k];
  }
  hipLaunchKernelGGL(k_episode_log, dim3((n_ids + 255) / 256), dim3(256), 0, (hipStream_t)stream, G, (int)num_keys, env_ids, (int)n_ids,
                     (long long)num_envs, episode_length_s, reinterpret_cast<unsigned long long*>(workspace17), out_means,
                     episode_length_or_null, reset_buf_or_null, (int)reset_elem_bytes, history_or_null, (int)history_row_words);
  return GLUE_LAUNCH_OK("shf_reset_bookkeeping");
}

extern "C" int shf_reward_accumulate(const float* const* terms, float* const* sums, int32_t num_keys, int64_t num_envs,
                                     float* rew, void* stream) {
  if (!terms || !sums || !rew) return shf_set_error("shf_reward_accumulate: null argument");
  if (num_keys < 1 || num_keys > GLUE_MAX_KEYS) return shf_set_error("shf_reward_accumulate: 1..16 terms");
  if (num_envs <= 0) return 0;
  GlueConstKeys R{};
  GlueKeys S{};
  for (int k = 0; k < num_keys; k++) {
    if (!terms[k] || !sums[k]) return shf_set_error("shf_reward_accumulate: null tensor");
    R.p[k] = terms[k]; S.p[k] = sums[k];
  }
  hipLaunchKernelGGL(k_reward_accumulate, dim3((unsigned)((num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R, S,
                     (int)num_keys, (long long)num_envs, rew);
  return GLUE_LAUNCH_OK("shf_reward_accumulate");
}
