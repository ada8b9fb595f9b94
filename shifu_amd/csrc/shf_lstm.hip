// shf_lstm.hip -- one LSTM cell step of the recurrent policy (rsl_rl's ActorCriticRecurrent, which the reference's
// PPOConfig.policy names: shifu/configs/policy_config.py:13-16, rnn_type 'lstm', 512 hidden units, one layer).
//
//   pre[m, g H + u] = sum_k [x | r h_prev][m, k] [W_ih | W_hh][g H + u, k] + b_ih[g H + u] + b_hh[g H + u]     g = i, f, g, o (torch's order)
//   c'[m, u] = sigma(pre_f) r c_prev[m, u] + sigma(pre_i) tanh(pre_g)          r = reset[m] ? 0 : 1
//   h'[m, u] = sigma(pre_o) tanh(c')
// as one GEMM on the matrix cores whose epilogue is the whole pointwise update: the pre-activations never reach memory.
// Operand scheme of shf_mlp.hip / shf_conv.hip: bf16 head + tail (a * bl, al * b, a * b; tail * tail dropped),
// v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same k order; shf_mlp_set_precision(SHF_MLP_BF16) drops the tails.
//   * A block owns 32 rows and up to four slices of 32 hidden units; wave w keeps the FOUR gate accumulators (4 x 16
//     registers) of its slice's units, so i, f, g, o of a (row, unit) pair meet in one lane's registers.
//   * The reduction index runs over [x | h]; the x part is zero-padded to a whole k step (16) so that h starts on a step
//     boundary.  The gathered rows go through LDS in chunks of 32 k, two buffers: the loads of chunk c + 1 are issued before
//     the MFMAs of chunk c and committed (head + tail) after them -- one barrier per chunk (shf_conv.hip's scheme).  The
//     reset factor is applied as the h rows are committed, and to c_prev in the epilogue.
//   * The weights are not staged: shf_lstm_pack_weights lays [W_ih | W_hh] out once in fragment order, column tiles
//     reordered so that the four gate tiles of a unit slice are adjacent ([4 slice + gate][k step][lane] -> 8 bf16); a
//     wave's B fragment is one contiguous 1 KB load from L2.
//   * h_out / c_out must not overlap h_prev / c_prev / x: the blocks of the other unit slices of the same rows still read
//     them.  The host entry refuses overlapping ranges.
// A row of the output depends on its own row of x, h_prev, c_prev only: no atomics, no split reduction, no scratch, no host
// synchronisation -- capturable, and independent of the batch size and of a row's place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

#define LSTM_DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(8))) __bf16 lbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 lbf16x4;
typedef __attribute__((ext_vector_type(16))) float lf32x16;
typedef __attribute__((ext_vector_type(4))) float lf32x4;

int shf_mlp_report_error(const char* message);     // csrc/shf_mlp.hip: sets the text shf_mlp_last_error returns; returns 1

namespace {

constexpr int LKC = 32, LLDT = LKC + 8;   // k per chunk; LDS row = 40 bf16 = 80 B (16-byte aligned fragments, staggered banks)
constexpr int LBM = 32, LNW = 4;          // rows per block; waves (= unit slices) per block

struct LstmArgs {
  const float* x;
  int ldx;
  const float* h_prev;
  const float* c_prev;
  const unsigned char* reset;   // one byte per row (nonzero: the row's h_prev and c_prev count as zero), or null
  const uint4* bhi;             // [4 ceil(H / 32)][nks][64] fragments of the bf16 heads
  const uint4* blo;             // ... of the tails
  const float* b_ih;            // [4 H] or null
  const float* b_hh;
  float* h_out;
  float* c_out;
  float* gates;                 // [M, 4 H] activated gates for the backward pass, or null
  int M, I, Ip, H;              // Ip = I rounded up to 16
  int nks, nslices;             // k steps of 16 over [x | h]; slices of 32 units
  int hvec;                     // h_prev rows are whole 16-byte chunks (H % 4 == 0, base aligned)
};

LSTM_DEV void lstm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
LSTM_DEV float lstm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <bool SPLIT>
__global__ __launch_bounds__(64 * LNW) void k_lstm_cell(LstmArgs P) {
  constexpr int PLANE = LBM * LLDT;                       // bf16 per plane (heads; tails behind them)
  constexpr int BUF = (SPLIT ? 2 : 1) * PLANE;
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * BUF];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int r0 = (int)blockIdx.x * LBM;
  const int slice = (int)blockIdx.y * LNW + wave;
  const bool wave_on = slice < P.nslices;                 // a wave without a slice only helps moving the rows
  const int nchunks = (P.nks + 1) >> 1;

  // this thread's share of a chunk: row t >> 3, the four k  4 (t & 7) .. + 3  (wholly inside x, its padding, or h: Ip % 16 == 0)
  const int kq = 4 * (t & 7);
  const int mrow = r0 + (t >> 3);
  const bool rin = mrow < P.M;
  const float rfac = (rin && P.reset && P.reset[mrow]) ? 0.0f : 1.0f;
  const float* xrow = P.x + (size_t)(rin ? mrow : 0) * P.ldx;
  const float* hrow = P.h_prev + (size_t)(rin ? mrow : 0) * P.H;

  float raw[4];
  uint32_t ok;           // bit c: element c is inside its operand
  bool from_h;
  auto issue = [&](int k0) {
    const int k = k0 + kq;
    ok = 0u;
    from_h = k >= P.Ip;
    if (!from_h) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const bool in = rin && k + c < P.I;
        raw[c] = xrow[in ? k + c : 0];
        ok |= (in ? 1u : 0u) << c;
      }
    } else {
      const int kh = k - P.Ip;
      if (P.hvec) {
        const bool in = rin && kh < P.H;                    // H % 4 == 0: the chunk is whole
        const lf32x4 v = *reinterpret_cast<const lf32x4*>(hrow + (in ? kh : 0));
#pragma unroll
        for (int c = 0; c < 4; c++) raw[c] = v[c];
        ok = in ? 0xFu : 0u;
      } else {
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const bool in = rin && kh + c < P.H;
          raw[c] = hrow[in ? kh + c : 0];
          ok |= (in ? 1u : 0u) << c;
        }
      }
    }
  };
  auto commit = [&](uint16_t* buf) {
    lbf16x4 h, l;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float v = (ok >> c) & 1u ? raw[c] : 0.0f;
      if (from_h) v *= rfac;                                // the reset, by multiplication (as the stock path's h * (1 - done))
      h[c] = (__bf16)v;
      l[c] = (__bf16)(v - (float)h[c]);
    }
    uint16_t* dst = buf + (t >> 3) * LLDT + kq;
    *reinterpret_cast<lbf16x4*>(dst) = h;
    if (SPLIT) *reinterpret_cast<lbf16x4*>(dst + PLANE) = l;
  };

  lf32x16 acc[4];        // i, f, g, o of this wave's 32 units x the block's 32 rows
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;

  issue(0);
  for (int c = 0; c < nchunks; c++) {
    uint16_t* buf = lds + (c & 1) * BUF;
    // this chunk's weight fragments: straight from the pack (L2), in flight across the commit and the barrier
    uint4 bh[2][4], bl[2][4];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int ks = 2 * c + s;
        bh[s][j] = bl[s][j] = uint4{0u, 0u, 0u, 0u};
        if (wave_on && ks < P.nks) {                          // (wave-uniform)
          const size_t e = ((size_t)(4 * slice + j) * P.nks + ks) * 64 + lane;
          bh[s][j] = P.bhi[e];
          if (SPLIT) bl[s][j] = P.blo[e];
        }
      }
    commit(buf);
    lstm_lds_barrier();          // every wave has committed chunk c, hence finished the MFMAs of chunk c - 1 (the other buffer)
    if (c + 1 < nchunks) issue((c + 1) * LKC);
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        if (2 * c + s < P.nks) {
          const uint16_t* ap = buf + (lane & 31) * LLDT + 16 * s + 8 * (lane >> 5);
          const lbf16x8 a = *reinterpret_cast<const lbf16x8*>(ap);
          lbf16x8 al;
          if (SPLIT) al = *reinterpret_cast<const lbf16x8*>(ap + PLANE);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const lbf16x8 b = __builtin_bit_cast(lbf16x8, bh[s][j]);
            if (SPLIT) {
              // the two cross terms first (small), then head * head; tail * tail (2^-18 relative) is dropped
              const lbf16x8 bt = __builtin_bit_cast(lbf16x8, bl[s][j]);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bt, acc[j], 0, 0, 0);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc[j], 0, 0, 0);
            }
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
          }
        }
      }
    }
  }

  // epilogue from the accumulators: unit = lane & 31 of the slice, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (!wave_on) return;
  const int u = 32 * slice + (lane & 31);
  if (u >= P.H) return;
  float bias[4];
#pragma unroll
  for (int j = 0; j < 4; j++) bias[j] = (P.b_ih ? P.b_ih[j * P.H + u] : 0.0f) + (P.b_hh ? P.b_hh[j * P.H + u] : 0.0f);
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    const int m = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (m < P.M) {
      const size_t e = (size_t)m * P.H + u;
      const float rf = (P.reset && P.reset[m]) ? 0.0f : 1.0f;
      const float gi = lstm_sigmoid(acc[0][reg] + bias[0]), gf = lstm_sigmoid(acc[1][reg] + bias[1]);
      const float gg = tanhf(acc[2][reg] + bias[2]), go = lstm_sigmoid(acc[3][reg] + bias[3]);
      const float cn = gf * (P.c_prev[e] * rf) + gi * gg;
      P.c_out[e] = cn;
      P.h_out[e] = go * tanhf(cn);
      if (P.gates) {
        float* gp = P.gates + (size_t)m * 4 * P.H + u;
        gp[0] = gi; gp[P.H] = gf; gp[2 * (size_t)P.H] = gg; gp[3 * (size_t)P.H] = go;
      }
    }
  }
}

// fragment order of [W_ih | W_hh]: entry (4 slice + gate, ks, lane) holds unit 32 slice + (lane & 31) of that gate,
// k = 16 ks + 8 (lane >> 5) + j over [x (I, zero-padded to Ip) | h (H)]
__global__ __launch_bounds__(256) void k_lstm_pack(const float* __restrict__ w_ih, const float* __restrict__ w_hh, uint4* __restrict__ pack, int I, int Ip,
                                                   int H, int nks, long long entries) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int lane = (int)(e & 63), ks = (int)((e >> 6) % nks), ct = (int)((e >> 6) / nks);
  const int u = 32 * (ct >> 2) + (lane & 31), g = ct & 3;
  const size_t row = (size_t)g * H + u;
  lbf16x8 h, l;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int k = 16 * ks + 8 * (lane >> 5) + j;
    float v = 0.0f;
    if (u < H) {
      if (k < Ip) { if (k < I) v = w_ih[row * I + k]; }
      else if (k - Ip < H) v = w_hh[row * H + (k - Ip)];
    }
    h[j] = (__bf16)v;
    l[j] = (__bf16)(v - (float)h[j]);
  }
  pack[e] = __builtin_bit_cast(uint4, h);
  pack[entries + e] = __builtin_bit_cast(uint4, l);
}

// Pointwise half of the cell's backward pass: from dL/dh', dL/dc' (optional), the activated gates and the cell states to the
// pre-activation gradients (M, 4 H) -- the operand of the three gradient GEMMs -- and dL/dc_prev (reset factor included).
__global__ __launch_bounds__(256) void k_lstm_cell_bwd(const float* __restrict__ dh, const float* __restrict__ dc, const float* __restrict__ gates,
                                                       const float* __restrict__ c_prev, const unsigned char* __restrict__ reset,
                                                       const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_prev,
                                                       long long M, int H) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * H) return;
  const long long m = e / H;
  const int u = (int)(e - m * H);
  const float* gp = gates + (size_t)m * 4 * H + u;
  const float gi = gp[0], gf = gp[H], gg = gp[2 * (size_t)H], go = gp[3 * (size_t)H];
  const float rf = (reset && reset[m]) ? 0.0f : 1.0f;
  const float tc = tanhf(c_out[e]);
  const float dhv = dh[e];
  const float dct = (dc ? dc[e] : 0.0f) + dhv * go * (1.0f - tc * tc);
  float* dg = dgates + (size_t)m * 4 * H + u;
  dg[0] = dct * gg * (gi * (1.0f - gi));
  dg[H] = dct * (c_prev[e] * rf) * (gf * (1.0f - gf));
  dg[2 * (size_t)H] = dct * gi * (1.0f - gg * gg);
  dg[3 * (size_t)H] = dhv * tc * (go * (1.0f - go));
  dc_prev[e] = dct * gf * rf;
}

int lstm_fail(const std::string& m) { return shf_mlp_report_error(m.c_str()); }
int lstm_ip(int I) { return (I + 15) / 16 * 16; }
int lstm_nks(int I, int H) { return lstm_ip(I) / 16 + (H + 15) / 16; }
long long lstm_entries(int I, int H) { return (long long)((H + 31) / 32) * 4 * lstm_nks(I, H) * 64; }
bool lstm_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
constexpr int LSTM_MAX_DIM = 1 << 15;

}  // namespace

extern "C" int shf_lstm_pack_bytes(int32_t I, int32_t H, int64_t* bytes) {
  if (!bytes || I <= 0 || H <= 0 || I > LSTM_MAX_DIM || H > LSTM_MAX_DIM) return lstm_fail("shf_lstm_pack_bytes: bad argument (1 <= I, H <= 32768)");
  *bytes = (int64_t)(2 * lstm_entries(I, H) * (long long)sizeof(uint4));
  return 0;
}

extern "C" int shf_lstm_pack_weights(const float* w_ih, const float* w_hh, void* pack, int32_t I, int32_t H, void* stream) {
  if (!w_ih || !w_hh || !pack) return lstm_fail("shf_lstm_pack_weights: null tensor");
  if (I <= 0 || H <= 0 || I > LSTM_MAX_DIM || H > LSTM_MAX_DIM) return lstm_fail("shf_lstm_pack_weights: bad shape (1 <= I, H <= 32768)");
  if (((uintptr_t)pack & 15u) != 0) return lstm_fail("shf_lstm_pack_weights: pack must be 16-byte aligned");
  const long long entries = lstm_entries(I, H);
  if (entries >= (1ll << 30)) return lstm_fail("shf_lstm_pack_weights: layer too large");
  hipLaunchKernelGGL(k_lstm_pack, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, (uint4*)pack, I,
                     lstm_ip(I), H, lstm_nks(I, H), entries);
  return hipGetLastError() == hipSuccess ? 0 : lstm_fail("shf_lstm_pack_weights: launch failed");
}

extern "C" int shf_lstm_cell_forward(const float* x, int32_t ldx, const float* h_prev, const float* c_prev, const unsigned char* reset_or_null,
                                     const void* pack, const float* b_ih, const float* b_hh, float* h_out, float* c_out,
                                     float* gates_or_null, int32_t M, int32_t I, int32_t H, void* stream) {
  if (!x || !h_prev || !c_prev || !pack || !h_out || !c_out) return lstm_fail("shf_lstm_cell_forward: null tensor");
  if (M <= 0 || I <= 0 || H <= 0 || ldx < I || I > LSTM_MAX_DIM || H > LSTM_MAX_DIM)
    return lstm_fail("shf_lstm_cell_forward: bad shape (M, I, H >= 1, ldx >= I, I and H <= 32768)");
  if ((long long)M * 4 * H >= (1ll << 40) || (long long)M * ldx >= (1ll << 40)) return lstm_fail("shf_lstm_cell_forward: batch too large");
  if (lstm_entries(I, H) >= (1ll << 30)) return lstm_fail("shf_lstm_cell_forward: layer too large");
  if (((uintptr_t)pack & 15u) != 0) return lstm_fail("shf_lstm_cell_forward: pack must be 16-byte aligned");
  const size_t state = (size_t)M * H * sizeof(float), xbytes = ((size_t)(M - 1) * ldx + I) * sizeof(float);
  // the blocks of the other unit slices of the same rows read h_prev / c_prev / x while this one stores: no aliasing
  const void* outs[2] = {h_out, c_out};
  for (const void* o : outs)
    if (lstm_overlap(o, state, h_prev, state) || lstm_overlap(o, state, c_prev, state) || lstm_overlap(o, state, x, xbytes))
      return lstm_fail("shf_lstm_cell_forward: h_out / c_out overlap h_prev / c_prev / x (write the next state to a buffer of its own)");
  if (lstm_overlap(h_out, state, c_out, state)) return lstm_fail("shf_lstm_cell_forward: h_out and c_out overlap");
  if (gates_or_null && (lstm_overlap(gates_or_null, 4 * state, h_prev, state) || lstm_overlap(gates_or_null, 4 * state, c_prev, state) ||
                        lstm_overlap(gates_or_null, 4 * state, x, xbytes) || lstm_overlap(gates_or_null, 4 * state, h_out, state) ||
                        lstm_overlap(gates_or_null, 4 * state, c_out, state)))
    return lstm_fail("shf_lstm_cell_forward: gates overlap another tensor");
  LstmArgs P{};
  P.x = x; P.ldx = ldx; P.h_prev = h_prev; P.c_prev = c_prev; P.reset = reset_or_null;
  P.bhi = (const uint4*)pack; P.blo = (const uint4*)pack + lstm_entries(I, H);
  P.b_ih = b_ih; P.b_hh = b_hh; P.h_out = h_out; P.c_out = c_out; P.gates = gates_or_null;
  P.M = M; P.I = I; P.Ip = lstm_ip(I); P.H = H; P.nks = lstm_nks(I, H); P.nslices = (H + 31) / 32;
  P.hvec = (H % 4 == 0 && ((uintptr_t)h_prev & 15u) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((M + LBM - 1) / LBM), (unsigned)((P.nslices + LNW - 1) / LNW));
  if (grid.y > 65535u) return lstm_fail("shf_lstm_cell_forward: layer too large");
  if (shf_mlp_get_precision() != SHF_MLP_BF16) hipLaunchKernelGGL(k_lstm_cell<true>, grid, dim3(64 * LNW), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL(k_lstm_cell<false>, grid, dim3(64 * LNW), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : lstm_fail("shf_lstm_cell_forward: launch failed");
}

extern "C" int shf_lstm_cell_backward_pointwise(const float* dh, const float* dc_or_null, const float* gates, const float* c_prev,
                                                const unsigned char* reset_or_null, const float* c_out, float* dgates, float* dc_prev,
                                                int32_t M, int32_t H, void* stream) {
  if (!dh || !gates || !c_prev || !c_out || !dgates || !dc_prev) return lstm_fail("shf_lstm_cell_backward_pointwise: null tensor");
  if (M <= 0 || H <= 0 || H > LSTM_MAX_DIM || (long long)M * 4 * H >= (1ll << 40)) return lstm_fail("shf_lstm_cell_backward_pointwise: bad shape");
  const long long n = (long long)M * H;
  hipLaunchKernelGGL(k_lstm_cell_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, dc_or_null, gates, c_prev,
                     reset_or_null, c_out, dgates, dc_prev, (long long)M, (int)H);
  return hipGetLastError() == hipSuccess ? 0 : lstm_fail("shf_lstm_cell_backward_pointwise: launch failed");
}
