// shf_lstm.hip -- one LSTM cell step of the recurrent policy (rsl_rl's ActorCriticRecurrent, which the reference's
// PPOConfig.policy names: shifu/configs/policy_config.py:13-16, rnn_type 'lstm', 512 hidden units, one layer).
//
//   pre[m, g H + u] = sum_k [x | r h_prev][m, k] [W_ih | W_hh][g H + u, k] + b_ih[g H + u] + b_hh[g H + u]     g = i, f, g, o (torch's order)
//   c'[m, u] = sigma(pre_f) r c_prev[m, u] + sigma(pre_i) tanh(pre_g)          r = reset[m] ? 0 : 1
//   h'[m, u] = sigma(pre_o) tanh(c')
// on the GEMM core of shf_rnn_cell.h (operand scheme, k padding, LDS pipeline, pack layout, aliasing rule: there) with four
// column tiles per unit slice: wave w keeps the FOUR gate accumulators of its slice's units, so i, f, g, o of a (row, unit)
// pair meet in one lane's registers.  The reset factor is applied to c_prev in the epilogue.  h_out / c_out must not
// overlap h_prev / c_prev / x.
#include "shf_rnn_cell.h"

namespace {

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

struct LstmCell {
  using Args = LstmArgs;
  static constexpr int NT = 4;                // i, f, g, o
  static constexpr bool SPLIT_LAST = false;

  static RNN_DEV void epilogue(const LstmArgs& P, const rf32x16 (&acc)[4], int u, int r0, int lane) {
    float bias[4];
#pragma unroll
    for (int j = 0; j < 4; j++) bias[j] = (P.b_ih ? P.b_ih[j * P.H + u] : 0.0f) + (P.b_hh ? P.b_hh[j * P.H + u] : 0.0f);
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int m = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (m < P.M) {
        const size_t e = (size_t)m * P.H + u;
        const float rf = (P.reset && P.reset[m]) ? 0.0f : 1.0f;
        const float gi = rnn_sigmoid(acc[0][reg] + bias[0]), gf = rnn_sigmoid(acc[1][reg] + bias[1]);
        const float gg = tanhf(acc[2][reg] + bias[2]), go = rnn_sigmoid(acc[3][reg] + bias[3]);
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
};

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

}  // namespace

extern "C" int shf_lstm_pack_bytes(int32_t I, int32_t H, int64_t* bytes) { return rnn_pack_bytes("shf_lstm_pack_bytes", LstmCell::NT, I, H, bytes); }

extern "C" int shf_lstm_pack_weights(const float* w_ih, const float* w_hh, void* pack, int32_t I, int32_t H, void* stream) {
  return rnn_pack_weights<LstmCell::NT>("shf_lstm_pack_weights", w_ih, w_hh, pack, I, H, stream);
}

extern "C" int shf_lstm_cell_forward(const float* x, int32_t ldx, const float* h_prev, const float* c_prev, const unsigned char* reset_or_null,
                                     const void* pack, const float* b_ih, const float* b_hh, float* h_out, float* c_out,
                                     float* gates_or_null, int32_t M, int32_t I, int32_t H, void* stream) {
  if (!x || !h_prev || !c_prev || !pack || !h_out || !c_out) return rnn_fail("shf_lstm_cell_forward: null tensor");
  if (const int rc = rnn_forward_check("shf_lstm_cell_forward", LstmCell::NT, pack, ldx, M, I, H)) return rc;
  const size_t state = (size_t)M * H * sizeof(float), xbytes = ((size_t)(M - 1) * ldx + I) * sizeof(float);
  // the blocks of the other unit slices of the same rows read h_prev / c_prev / x while this one stores: no aliasing
  const void* outs[2] = {h_out, c_out};
  for (const void* o : outs)
    if (rnn_overlap(o, state, h_prev, state) || rnn_overlap(o, state, c_prev, state) || rnn_overlap(o, state, x, xbytes))
      return rnn_fail("shf_lstm_cell_forward: h_out / c_out overlap h_prev / c_prev / x (write the next state to a buffer of its own)");
  if (rnn_overlap(h_out, state, c_out, state)) return rnn_fail("shf_lstm_cell_forward: h_out and c_out overlap");
  if (gates_or_null && (rnn_overlap(gates_or_null, 4 * state, h_prev, state) || rnn_overlap(gates_or_null, 4 * state, c_prev, state) ||
                        rnn_overlap(gates_or_null, 4 * state, x, xbytes) || rnn_overlap(gates_or_null, 4 * state, h_out, state) ||
                        rnn_overlap(gates_or_null, 4 * state, c_out, state)))
    return rnn_fail("shf_lstm_cell_forward: gates overlap another tensor");
  LstmArgs P{};
  P.c_prev = c_prev; P.b_ih = b_ih; P.b_hh = b_hh; P.h_out = h_out; P.c_out = c_out; P.gates = gates_or_null;
  return rnn_launch<LstmCell>("shf_lstm_cell_forward", P, x, ldx, h_prev, reset_or_null, pack, M, I, H, stream);
}

extern "C" int shf_lstm_cell_backward_pointwise(const float* dh, const float* dc_or_null, const float* gates, const float* c_prev,
                                                const unsigned char* reset_or_null, const float* c_out, float* dgates, float* dc_prev,
                                                int32_t M, int32_t H, void* stream) {
  if (!dh || !gates || !c_prev || !c_out || !dgates || !dc_prev) return rnn_fail("shf_lstm_cell_backward_pointwise: null tensor");
  if (M <= 0 || H <= 0 || H > RNN_MAX_DIM || (long long)M * 4 * H >= (1ll << 40)) return rnn_fail("shf_lstm_cell_backward_pointwise: bad shape");
  const long long n = (long long)M * H;
  hipLaunchKernelGGL(k_lstm_cell_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, dc_or_null, gates, c_prev,
                     reset_or_null, c_out, dgates, dc_prev, (long long)M, (int)H);
  return hipGetLastError() == hipSuccess ? 0 : rnn_fail("shf_lstm_cell_backward_pointwise: launch failed");
}
