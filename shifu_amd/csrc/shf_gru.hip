// shf_gru.hip -- one GRU cell step of the recurrent policy (rsl_rl's ActorCriticRecurrent with rnn_type 'gru'; the LSTM
// counterpart is shf_lstm.hip).  torch.nn.GRU's equations, gate order (r, z, n):
//
//   a_r  = x W_ir^T + (rho h) W_hr^T          r  = sigma(a_r + b_ir + b_hr)              rho = reset[m] ? 0 : 1
//   a_z  = x W_iz^T + (rho h) W_hz^T          z  = sigma(a_z + b_iz + b_hz)
//   a_nx = x W_in^T                           hn = a_nh + b_hn
//   a_nh = (rho h) W_hn^T                     n  = tanh(a_nx + b_in + r * hn)
//   h'   = (1 - z) * n + z * (rho h)
// on the GEMM core of shf_rnn_cell.h (operand scheme, k padding, LDS pipeline, pack layout, aliasing rule: there).
//   * The pack has THREE column tiles per slice (r, z, n) and the wave keeps FOUR accumulators: r, z, n_x, n_h.  r and z
//     accumulate over every k step, the n tile's product goes into n_x for the k steps of the x part and into n_h for those
//     of the h part (the core's SPLIT_LAST) -- the n gate needs the two halves of its sum apart, because r multiplies only
//     the h half.
//   * The reset factor is applied to h_prev in the epilogue.  h_out must not overlap h_prev / x.
#include "shf_rnn_cell.h"

namespace {

struct GruArgs {
  const float* x;
  int ldx;
  const float* h_prev;
  const unsigned char* reset;   // one byte per row (nonzero: the row's h_prev counts as zero), or null
  const uint4* bhi;             // [3 ceil(H / 32)][nks][64] fragments of the bf16 heads
  const uint4* blo;             // ... of the tails
  const float* b_ih;            // [3 H] or null
  const float* b_hh;
  float* h_out;
  float* gates;                 // [M, 4 H]: r, z, n, hn for the backward pass, or null
  int M, I, Ip, H;              // Ip = I rounded up to 16
  int nks, nslices;             // k steps of 16 over [x | h]; slices of 32 units
  int hvec;                     // h_prev rows are whole 16-byte chunks (H % 4 == 0, base aligned)
};

struct GruCell {
  using Args = GruArgs;
  static constexpr int NT = 3;                // r, z, n
  static constexpr bool SPLIT_LAST = true;    // acc: r, z, n_x, n_h

  static RNN_DEV void epilogue(const GruArgs& P, const rf32x16 (&acc)[4], int u, int r0, int lane) {
    const size_t H = (size_t)P.H;
    const float b_r = (P.b_ih ? P.b_ih[u] : 0.0f) + (P.b_hh ? P.b_hh[u] : 0.0f);
    const float b_z = (P.b_ih ? P.b_ih[H + u] : 0.0f) + (P.b_hh ? P.b_hh[H + u] : 0.0f);
    const float b_in = P.b_ih ? P.b_ih[2 * H + u] : 0.0f, b_hn = P.b_hh ? P.b_hh[2 * H + u] : 0.0f;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int m = r0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (m < P.M) {
        const size_t e = (size_t)m * H + u;
        const float rf = (P.reset && P.reset[m]) ? 0.0f : 1.0f;
        const float he = P.h_prev[e] * rf;
        const float gr = rnn_sigmoid(acc[0][reg] + b_r), gz = rnn_sigmoid(acc[1][reg] + b_z);
        const float hn = acc[3][reg] + b_hn;
        const float gn = tanhf(acc[2][reg] + b_in + gr * hn);
        P.h_out[e] = (1.0f - gz) * gn + gz * he;              // this form: z == 1 gives rho h_prev bit for bit
        if (P.gates) {
          float* gp = P.gates + (size_t)m * 4 * H + u;
          gp[0] = gr; gp[H] = gz; gp[2 * H] = gn; gp[3 * H] = hn;
        }
      }
    }
  }
};

// Pointwise half of the cell's backward pass: from dL/dh', the kept (r, z, n, hn) and he = rho h_prev to the pre-activation
// gradients of the x side (dgx) and of the h side (dgh: the n column carries r) -- the operands of the gradient GEMMs -- and
// the part of dL/dh_prev that does not pass through a GEMM (reset factor included).
__global__ __launch_bounds__(256) void k_gru_cell_bwd(const float* __restrict__ dh, const float* __restrict__ gates, const float* __restrict__ h_prev,
                                                      const unsigned char* __restrict__ reset, float* __restrict__ dgx, float* __restrict__ dgh,
                                                      float* __restrict__ dh_direct, long long M, int H) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * H) return;
  const long long m = e / H;
  const int u = (int)(e - m * H);
  const float* gp = gates + (size_t)m * 4 * H + u;
  const float gr = gp[0], gz = gp[H], gn = gp[2 * (size_t)H], hn = gp[3 * (size_t)H];
  const float rf = (reset && reset[m]) ? 0.0f : 1.0f;
  const float he = h_prev[e] * rf;
  const float dhv = dh[e];
  const float dn = dhv * (1.0f - gz) * (1.0f - gn * gn);
  const float dz = dhv * (he - gn) * (gz * (1.0f - gz));
  const float dr = dn * hn * (gr * (1.0f - gr));
  float* px = dgx + (size_t)m * 3 * H + u;
  float* ph = dgh + (size_t)m * 3 * H + u;
  px[0] = dr; px[H] = dz; px[2 * (size_t)H] = dn;
  ph[0] = dr; ph[H] = dz; ph[2 * (size_t)H] = dn * gr;
  dh_direct[e] = dhv * gz * rf;
}

}  // namespace

extern "C" int shf_gru_pack_bytes(int32_t I, int32_t H, int64_t* bytes) { return rnn_pack_bytes("shf_gru_pack_bytes", GruCell::NT, I, H, bytes); }

extern "C" int shf_gru_pack_weights(const float* w_ih, const float* w_hh, void* pack, int32_t I, int32_t H, void* stream) {
  return rnn_pack_weights<GruCell::NT>("shf_gru_pack_weights", w_ih, w_hh, pack, I, H, stream);
}

extern "C" int shf_gru_cell_forward(const float* x, int32_t ldx, const float* h_prev, const unsigned char* reset_or_null, const void* pack,
                                    const float* b_ih, const float* b_hh, float* h_out, float* gates_or_null, int32_t M, int32_t I, int32_t H,
                                    void* stream) {
  if (!x || !h_prev || !pack || !h_out) return rnn_fail("shf_gru_cell_forward: null tensor");
  if (const int rc = rnn_forward_check("shf_gru_cell_forward", GruCell::NT, pack, ldx, M, I, H)) return rc;
  const size_t state = (size_t)M * H * sizeof(float), xbytes = ((size_t)(M - 1) * ldx + I) * sizeof(float);
  // the blocks of the other unit slices of the same rows read h_prev / x while this one stores: no aliasing
  if (rnn_overlap(h_out, state, h_prev, state) || rnn_overlap(h_out, state, x, xbytes))
    return rnn_fail("shf_gru_cell_forward: h_out overlaps h_prev / x (write the next state to a buffer of its own)");
  if (gates_or_null && (rnn_overlap(gates_or_null, 4 * state, h_prev, state) || rnn_overlap(gates_or_null, 4 * state, x, xbytes) ||
                        rnn_overlap(gates_or_null, 4 * state, h_out, state)))
    return rnn_fail("shf_gru_cell_forward: gates overlap another tensor");
  GruArgs P{};
  P.b_ih = b_ih; P.b_hh = b_hh; P.h_out = h_out; P.gates = gates_or_null;
  return rnn_launch<GruCell>("shf_gru_cell_forward", P, x, ldx, h_prev, reset_or_null, pack, M, I, H, stream);
}

extern "C" int shf_gru_cell_backward_pointwise(const float* dh, const float* gates, const float* h_prev, const unsigned char* reset_or_null,
                                               float* dgx, float* dgh, float* dh_direct, int32_t M, int32_t H, void* stream) {
  if (!dh || !gates || !h_prev || !dgx || !dgh || !dh_direct) return rnn_fail("shf_gru_cell_backward_pointwise: null tensor");
  if (M <= 0 || H <= 0 || H > RNN_MAX_DIM || (long long)M * 4 * H >= (1ll << 40)) return rnn_fail("shf_gru_cell_backward_pointwise: bad shape");
  const long long n = (long long)M * H;
  hipLaunchKernelGGL(k_gru_cell_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, gates, h_prev, reset_or_null, dgx,
                     dgh, dh_direct, (long long)M, (int)H);
  return hipGetLastError() == hipSuccess ? 0 : rnn_fail("shf_gru_cell_backward_pointwise: launch failed");
}
