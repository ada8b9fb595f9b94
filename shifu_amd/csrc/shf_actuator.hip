// shf_actuator.hip -- what sits between a commanded joint angle and a joint torque on the facade / hook path: a per-env
// command delay, an ideal PD or a learned actuator network over short histories of position error and velocity, a per-dof
// motor strength factor, and the DC motor's torque-speed clip.  One launch (k_actuator_pd, or k_actuator_net at a padded
// hidden width of 32 or 64) is one simulation sub-step for every (env e, dof d) pair; a work item is one pair and reads no
// other pair's state, so there is no counter, no ring head and nothing two lanes could race on: an env's dofs may lie in
// different wavefronts or blocks, and a captured launch replays correctly.  A translation unit of its own, so that no other
// kernel's machine code moves.
//
// State, owned by the caller, read and written in place: cmd_hist (n, L, nd), L in 1..8, and in network mode err_hist and
// vel_hist (n, H, nd), H in 1..8.  Slot 0 is this call's value, slot k the value from k calls ago.
//
// The algorithm per (e, d).  tests/actuator_ref.py `step32` is this text in NumPy float32, operation by operation; no
// multiply-add is fused (the arithmetic contract of csrc/shf_device.h), so every line is a sequence of correctly rounded
// float32 operations in the order written.  t = target[e, d]; q, qd = the dof's position and velocity.
//   1. Reset (reset[e] != 0):  every slot of cmd_hist[e, :, d] = t;  every slot of err_hist[e, :, d], vel_hist[e, :, d] = 0.
//   2. Shift.  For k = L-1 .. 1: cmd_hist[e, k, d] = cmd_hist[e, k-1, d];  cmd_hist[e, 0, d] = t.
//   3. Delay.  D = clamp(delay[e], 0, L-1), or the scalar delay;  a = cmd_hist[e, D, d]  (D = 0: this call's target);
//        applied_target_out[e, d] = a  when that pointer is given.
//   4. Position error.  err = a - q.
//   5. Torque.
//        PD mode:  tau = (kp err) - (kd qd),  kp, kd at [e gain_env_stride + d].
//        Network mode:  err_hist and vel_hist shift as in step 2, err and qd entering at slot 0;
//          x[i] = err_scale err_hist[e, taps[i], d],  x[T + i] = vel_scale vel_hist[e, taps[i], d],  i = 0 .. T-1;
//          per layer, per output j:  acc = b_j;  for k ascending: acc = acc + (w_jk h_k);  the activation on every layer but
//          the last, whose one output is y;  tau = out_scale y.
//          Activations: softsign x / (1 + |x|);  relu (x > 0 ? x : 0);  tanh (tanhf);  elu (x > 0 ? x : expm1f(x)).
//   6. Strength.  tau = tau strength[e, d]  when given.
//   7. Limits, lim = effort_limit[d] (an entry <= 0 or no effort_limit: +inf).  With saturation and velocity_limit (the DC
//        motor):  r = qd / vlim[d];  hi = min(max(sat[d] (1 - r), 0), lim);  lo = max(min(sat[d] (-1 - r), 0), -lim);
//        tau = max(min(tau, hi), lo).  Else, with a finite lim:  tau = max(min(tau, lim), -lim).
//   8. efforts_out[e, d] = tau.
//
// The network's weights arrive zero-padded (the layout is stated at shf_actuator_step in include/shifu_amd.h): the inputs
// to 8, every hidden width to P = 32 or 64.  A padded unit has b = 0 and w = 0, so it is 0 after every one of the four
// activations, and the products it adds downstream are exact +0: every partial sum of step 5 stays what the unpadded net
// gives.  The block stages the weights in LDS once (at most 36 KB); every lane then reads the same address (a broadcast, no
// bank conflict).  The hidden vectors live in registers: a layer runs as P / 8 passes of 8 outputs over the unrolled inputs,
// and the output vector moves down by 8 places per pass, so every register index is a compile-time constant and nothing
// lands on the stack.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

int shf_set_error(const std::string& msg);   // shf_api.hip: the message shf_last_error() returns

namespace {

constexpr int ACT_T = 256;                     // threads per block
static_assert(SHF_ACTUATOR_MAX_SLOTS == 8, "Col8 holds eight slots");
constexpr int ACT_IN = 8;                      // padded input width: 2 x SHF_ACTUATOR_MAX_TAPS
constexpr int ACT_CH = 8;                      // outputs per pass of a layer

constexpr int net_floats(int P, int nl) {      // the padded weight buffer: first layer, nl - 2 hidden layers, last layer
  const int c = nl >= 2 ? (P * ACT_IN + P) + (nl - 2) * (P * P + P) + (P + 1) : P + 1;
  return (c + 3) / 4 * 4;
}

struct ActArgs {
  const float* target; const float* dof; int dof_stride;
  const float* kp; const float* kd; int gain_env;
  const int* delay; int delay_scalar;
  const float* strength; const float* sat; const float* vlim; const float* lim;
  const unsigned char* reset;
  float* cmd; int L; float* errh; float* velh; int H;
  int nd; long long rows;
  float* applied; float* out;
  const float* w; int wcount, nl, act, T; int xlag[2 * SHF_ACTUATOR_MAX_TAPS];   // xlag[k]: the history lag input k reads
  float err_scale, vel_scale, out_scale;
};

// A history column after its shift: s0 = this call's value .. s7 = the value from seven calls ago.  Named fields and written-out
// slots instead of arrays and loops, on purpose: over a local array the optimiser folds "select between two loads" into "load
// from a selected address" before it unrolls, and the column lands on the stack (or in LDS) behind a run-time index.
struct Col8 { float s0, s1, s2, s3, s4, s5, s6, s7; };

// one history column (slots 0 .. S-1 of one (e, d), `stride` floats apart): reset, shift, insert `v` at slot 0.  Slots at
// k >= S hold a copy of an older slot and are never selected.
__device__ __forceinline__ Col8 shift_column(float* col, long long stride, int S, bool rs, float fill, float v) {
#define ACT_OLD(k) const float o##k = rs ? fill : col[(long long)min(k, S - 1) * stride];
  ACT_OLD(0) ACT_OLD(1) ACT_OLD(2) ACT_OLD(3) ACT_OLD(4) ACT_OLD(5) ACT_OLD(6)
#undef ACT_OLD
#define ACT_PUT(k, x) if (k < S) col[(long long)k * stride] = x;
  ACT_PUT(7, o6) ACT_PUT(6, o5) ACT_PUT(5, o4) ACT_PUT(4, o3) ACT_PUT(3, o2) ACT_PUT(2, o1) ACT_PUT(1, o0)
#undef ACT_PUT
  col[0] = v;
  return Col8{v, o0, o1, o2, o3, o4, o5, o6};
}

// slot k of a column, k in 0 .. 7 at run time (the slots by value: the selects must see values, not loads)
__device__ __forceinline__ float pick8(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7, int k) {
  float a = s0;
  a = k >= 1 ? s1 : a; a = k >= 2 ? s2 : a; a = k >= 3 ? s3 : a; a = k >= 4 ? s4 : a;
  a = k >= 5 ? s5 : a; a = k >= 6 ? s6 : a; a = k >= 7 ? s7 : a;
  return a;
}
__device__ __forceinline__ float pick(const Col8 c, int k) { return pick8(c.s0, c.s1, c.s2, c.s3, c.s4, c.s5, c.s6, c.s7, k); }

// steps 1-4: the delayed command and the position error
__device__ __forceinline__ void front(const ActArgs& A, long long r, int& e, int& d, bool& rs, float& qd, float& err) {
  e = (int)(r / A.nd);
  d = (int)(r - (long long)e * A.nd);
  const float t = A.target[r];
  const float* ds = A.dof + r * (long long)A.dof_stride;
  const float q = ds[0];
  qd = ds[1];
  rs = A.reset != nullptr && A.reset[e] != 0;
  const Col8 now = shift_column(A.cmd + ((long long)e * A.L) * A.nd + d, A.nd, A.L, rs, t, t);
  int D = A.delay_scalar;
  if (A.delay) D = min(max(A.delay[e], 0), A.L - 1);
  const float a = pick(now, D);
  if (A.applied) A.applied[r] = a;
  err = a - q;
}

// steps 6-8: strength, limits, output
__device__ __forceinline__ void back(const ActArgs& A, long long r, int d, float qd, float tau) {
  if (A.strength) tau = tau * A.strength[r];
  const float lim = A.lim ? A.lim[d] : 0.0f;
  if (A.sat && A.vlim) {
    const float cap = lim > 0.0f ? lim : INFINITY;
    const float sat = A.sat[d];
    const float rr = qd / A.vlim[d];
    const float hi = fminf(fmaxf(sat * (1.0f - rr), 0.0f), cap);
    const float lo = fmaxf(fminf(sat * (-1.0f - rr), 0.0f), -cap);
    tau = fmaxf(fminf(tau, hi), lo);
  } else if (lim > 0.0f) {
    tau = fmaxf(fminf(tau, lim), -lim);
  }
  A.out[r] = tau;
}

__global__ void __launch_bounds__(ACT_T) k_actuator_pd(ActArgs A) {
  const long long r = (long long)blockIdx.x * ACT_T + threadIdx.x;
  if (r >= A.rows) return;
  int e, d;
  bool rs;
  float qd, err;
  front(A, r, e, d, rs, qd, err);
  const long long g = (long long)e * A.gain_env + d;
  back(A, r, d, qd, (A.kp[g] * err) - (A.kd[g] * qd));
}

__device__ __forceinline__ float activate(float x, int act) {
  switch (act) {
    case SHF_ACTUATOR_SOFTSIGN: return x / (1.0f + fabsf(x));
    case SHF_ACTUATOR_RELU: return x > 0.0f ? x : 0.0f;
    case SHF_ACTUATOR_TANH: return tanhf(x);
    default: return x > 0.0f ? x : expm1f(x);
  }
}

// one layer with activation: w = (P, IN) row-major then b (P), in LDS.  P / 8 passes of 8 outputs; o moves down by 8 per pass.
template <int IN, int P>
__device__ __forceinline__ void dense(const float* w, const float (&h)[IN], float (&o)[P], int act) {
  const float* b = w + P * IN;
#pragma unroll
  for (int i = 0; i < P; i++) o[i] = 0.0f;
#pragma nounroll
  for (int j0 = 0; j0 < P; j0 += ACT_CH) {
    float acc[ACT_CH];
#pragma unroll
    for (int c = 0; c < ACT_CH; c++) {
      const float* wr = w + (j0 + c) * IN;
      float a = b[j0 + c];
#pragma unroll
      for (int k = 0; k < IN; k++) a = a + (wr[k] * h[k]);
      acc[c] = activate(a, act);
    }
#pragma unroll
    for (int i = 0; i < P - ACT_CH; i++) o[i] = o[i + ACT_CH];
#pragma unroll
    for (int c = 0; c < ACT_CH; c++) o[P - ACT_CH + c] = acc[c];
  }
}

template <int P>
__global__ void __launch_bounds__(ACT_T) k_actuator_net(ActArgs A) {
  __shared__ __attribute__((aligned(16))) float sw[net_floats(P, SHF_ACTUATOR_MAX_LAYERS)];
  {
    const float4* src = reinterpret_cast<const float4*>(A.w);
    float4* dst = reinterpret_cast<float4*>(sw);
    for (int i = threadIdx.x; i < A.wcount / 4; i += ACT_T) dst[i] = src[i];   // the host has checked wcount against the layout
  }
  __syncthreads();
  const long long r = (long long)blockIdx.x * ACT_T + threadIdx.x;
  if (r >= A.rows) return;
  int e, d;
  bool rs;
  float qd, err;
  front(A, r, e, d, rs, qd, err);
  float x[ACT_IN];
  {
    const long long at = ((long long)e * A.H) * A.nd + d;
    const Col8 en = shift_column(A.errh + at, A.nd, A.H, rs, 0.0f, err);
    const Col8 vn = shift_column(A.velh + at, A.nd, A.H, rs, 0.0f, qd);
#pragma unroll
    for (int k = 0; k < ACT_IN; k++) {
      const float ev = A.err_scale * pick(en, A.xlag[k]), vv = A.vel_scale * pick(vn, A.xlag[k]);
      x[k] = k < A.T ? ev : (k < 2 * A.T ? vv : 0.0f);
    }
  }
  float h[P];
  const float* w = sw;
  if (A.nl >= 2) {
    dense<ACT_IN, P>(w, x, h, A.act);
    w += P * ACT_IN + P;
#pragma nounroll
    for (int l = 0; l < A.nl - 2; l++) {
      float g[P];
      dense<P, P>(w, h, g, A.act);
#pragma unroll
      for (int i = 0; i < P; i++) h[i] = g[i];
      w += P * P + P;
    }
  } else {
#pragma unroll
    for (int i = 0; i < P; i++) h[i] = i < ACT_IN ? x[i] : 0.0f;
  }
  float y = w[P];
#pragma unroll
  for (int k = 0; k < P; k++) y = y + (w[k] * h[k]);
  back(A, r, d, qd, A.out_scale * y);
}

}  // namespace

extern "C" int shf_actuator_step(const float* target, const float* dof_state, int32_t dof_elem_stride, const float* kp_or_null,
                                 const float* kd_or_null, int32_t gain_env_stride, const int32_t* delay_or_null, int32_t delay_scalar,
                                 const float* strength_or_null, const float* saturation_or_null, const float* velocity_limit_or_null,
                                 const float* effort_limit_or_null, const uint8_t* reset_or_null, int32_t mode,
                                 const ShfActuatorNet* net_or_null, const float* weights_or_null, int64_t weights_count,
                                 float* cmd_hist, int32_t cmd_slots, float* err_hist_or_null, float* vel_hist_or_null,
                                 int32_t hist_slots, int32_t n, int32_t num_dof, float* applied_target_out_or_null,
                                 float* efforts_out, void* stream) {
  if (!target || !dof_state || !cmd_hist || !efforts_out) return shf_set_error("shf_actuator_step: null tensor");
  if (num_dof < 1 || num_dof > SHF_MAX_DOFS) return shf_set_error("shf_actuator_step: num_dof outside 1..SHF_MAX_DOFS");
  if (n < 1) return shf_set_error("shf_actuator_step: n must be at least 1");
  if (dof_elem_stride < 2) return shf_set_error("shf_actuator_step: dof_elem_stride must be at least 2");
  if (cmd_slots < 1 || cmd_slots > SHF_ACTUATOR_MAX_SLOTS) return shf_set_error("shf_actuator_step: cmd_slots outside 1..8");
  if (!delay_or_null && (delay_scalar < 0 || delay_scalar >= cmd_slots))
    return shf_set_error("shf_actuator_step: delay_scalar outside 0..cmd_slots-1");
  if ((saturation_or_null != nullptr) != (velocity_limit_or_null != nullptr))
    return shf_set_error("shf_actuator_step: saturation and velocity_limit come together");
  if (mode != SHF_ACTUATOR_PD && mode != SHF_ACTUATOR_NET) return shf_set_error("shf_actuator_step: unknown mode");
  ActArgs A = {};
  A.target = target; A.dof = dof_state; A.dof_stride = (int)dof_elem_stride;
  A.delay = delay_or_null; A.delay_scalar = (int)delay_scalar;
  A.strength = strength_or_null; A.sat = saturation_or_null; A.vlim = velocity_limit_or_null; A.lim = effort_limit_or_null;
  A.reset = reset_or_null;
  A.cmd = cmd_hist; A.L = (int)cmd_slots;
  A.nd = (int)num_dof; A.rows = (long long)n * num_dof;
  A.applied = applied_target_out_or_null; A.out = efforts_out;
  const unsigned blocks = (unsigned)((A.rows + ACT_T - 1) / ACT_T);
  if (mode == SHF_ACTUATOR_PD) {
    if (!kp_or_null || !kd_or_null) return shf_set_error("shf_actuator_step: null tensor (PD mode needs kp and kd)");
    if (gain_env_stride != 0 && gain_env_stride != num_dof) return shf_set_error("shf_actuator_step: gain_env_stride must be 0 or num_dof");
    A.kp = kp_or_null; A.kd = kd_or_null; A.gain_env = (int)gain_env_stride;
    hipLaunchKernelGGL(k_actuator_pd, dim3(blocks), dim3(ACT_T), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_actuator_step: launch failed");
  }
  if (!net_or_null || !weights_or_null) return shf_set_error("shf_actuator_step: network mode without weights");
  if (!err_hist_or_null || !vel_hist_or_null) return shf_set_error("shf_actuator_step: network mode without histories");
  if (hist_slots < 1 || hist_slots > SHF_ACTUATOR_MAX_SLOTS) return shf_set_error("shf_actuator_step: hist_slots outside 1..8");
  const ShfActuatorNet& N = *net_or_null;
  if (N.num_taps < 1 || N.num_taps > SHF_ACTUATOR_MAX_TAPS) return shf_set_error("shf_actuator_step: num_taps outside 1..4");
  for (int i = 0; i < N.num_taps; i++)
    if (N.taps[i] < 0 || N.taps[i] >= hist_slots) return shf_set_error("shf_actuator_step: tap outside 0..hist_slots-1");
  if (N.num_layers < 1) return shf_set_error("shf_actuator_step: at least one layer");
  if (N.num_layers > SHF_ACTUATOR_MAX_LAYERS) return shf_set_error("shf_actuator_step: more than 4 layers");
  int widest = 1;
  for (int l = 0; l <= N.num_layers; l++) {
    if (N.widths[l] < 1 || N.widths[l] > SHF_ACTUATOR_MAX_WIDTH) return shf_set_error("shf_actuator_step: width outside 1..64");
    if (l > 0 && l < N.num_layers && N.widths[l] > widest) widest = N.widths[l];
  }
  if (N.widths[0] != 2 * N.num_taps) return shf_set_error("shf_actuator_step: first width must be 2 * num_taps");
  if (N.widths[N.num_layers] != 1) return shf_set_error("shf_actuator_step: last width must be 1");
  if (N.activation < SHF_ACTUATOR_SOFTSIGN || N.activation > SHF_ACTUATOR_ELU) return shf_set_error("shf_actuator_step: unknown activation");
  const int P = widest <= 32 ? 32 : 64;
  if (weights_count != (int64_t)net_floats(P, N.num_layers))
    return shf_set_error("shf_actuator_step: weights_count is not the padded layout's (" + std::to_string(net_floats(P, N.num_layers)) + " floats)");
  if ((reinterpret_cast<uintptr_t>(weights_or_null) & 15u) != 0) return shf_set_error("shf_actuator_step: weights must be 16-byte aligned");
  A.errh = err_hist_or_null; A.velh = vel_hist_or_null; A.H = (int)hist_slots;
  A.w = weights_or_null; A.wcount = (int)weights_count; A.nl = N.num_layers; A.act = N.activation; A.T = N.num_taps;
  for (int k = 0; k < 2 * SHF_ACTUATOR_MAX_TAPS; k++) A.xlag[k] = k < 2 * N.num_taps ? N.taps[k % N.num_taps] : 0;
  A.err_scale = N.err_scale; A.vel_scale = N.vel_scale; A.out_scale = N.out_scale;
  if (P == 32) hipLaunchKernelGGL(k_actuator_net<32>, dim3(blocks), dim3(ACT_T), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(k_actuator_net<64>, dim3(blocks), dim3(ACT_T), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_actuator_step: launch failed");
}
