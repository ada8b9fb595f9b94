// shf_gru.hip -- one GRU cell step of the recurrent policy (rsl_rl's ActorCriticRecurrent with rnn_type 'gru'; the LSTM
// counterpart is shf_lstm.hip, whose structure this kernel keeps).  torch.nn.GRU's equations, gate order (r, z, n):
//
//   a_r  = x W_ir^T + (rho h) W_hr^T          r  = sigma(a_r + b_ir + b_hr)              rho = reset[m] ? 0 : 1
//   a_z  = x W_iz^T + (rho h) W_hz^T          z  = sigma(a_z + b_iz + b_hz)
//   a_nx = x W_in^T                           hn = a_nh + b_hn
//   a_nh = (rho h) W_hn^T                     n  = tanh(a_nx + b_in + r * hn)
//   h'   = (1 - z) * n + z * (rho h)
// as one GEMM on the matrix cores over [x | rho h_prev] whose epilogue is the whole pointwise update: the pre-activations
// never reach memory.  Operand scheme of shf_mlp.hip / shf_lstm.hip: bf16 head + tail (a * bl, al * b, a * b; tail * tail
// dropped), v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same k order; shf_mlp_set_precision(SHF_MLP_BF16) drops the tails.
//   * A block owns 32 rows and up to four slices of 32 hidden units; wave w keeps FOUR accumulators (4 x 16 registers) of its
//     slice's units: r, z, n_x, n_h.  The pack has THREE column tiles per slice (r, z, n): r and z accumulate over every k
//     step, the n tile's product goes into n_x for the k steps of the x part (ks < Ip / 16) and into n_h for those of the h
//     part -- the n gate needs the two halves of its sum apart, because r multiplies only the h half.  The test is
//     wave-uniform and each side names its accumulator at compile time.
//   * The reduction index runs over [x | h]; the x part is zero-padded to a whole k step (16) so that h starts on a step
//     boundary (Ip is a multiple of 16, not of the chunk's 32: the switch can fall between the two k steps of one chunk).
//     The gathered rows go through LDS in chunks of 32 k, two buffers: the loads of chunk c + 1 are issued before the MFMAs
//     of chunk c and committed (head + tail) after them -- one barrier per chunk.  The reset factor is applied as the h rows
//     are committed, and to h_prev in the epilogue.
//   * The weights are not staged: shf_gru_pack_weights lays [W_ih | W_hh] out once in fragment order
//     ([3 slice + gate][k step][lane] -> 8 bf16); a wave's B fragment is one contiguous 1 KB load from L2.
//   * h_out must not overlap h_prev / x: the blocks of the other unit slices of the same rows still read them.  The host
//     entry refuses overlapping ranges.
// A row of the output depends on its own row of x, h_prev only: no atomics, no split reduction, no scratch, no host
// synchronisation -- capturable, and independent of the batch size and of a row's place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

#define GRU_DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(8))) __bf16 gbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 gbf16x4;
typedef __attribute__((ext_vector_type(16))) float gf32x16;
typedef __attribute__((ext_vector_type(4))) float gf32x4;

int shf_mlp_report_error(const char* message);     // csrc/shf_mlp.hip: sets the text shf_mlp_last_error returns; returns 1

namespace {

constexpr int GKC = 32, GLDT = GKC + 8;   // k per chunk; LDS row = 40 bf16 = 80 B (16-byte aligned fragments, staggered banks)
constexpr int GBM = 32, GNW = 4;          // rows per block; waves (= unit slices) per block

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

GRU_DEV void gru_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
GRU_DEV float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// acc += a * b with the head + tail scheme: the two cross terms first (small), then head * head; tail * tail (2^-18
// relative) is dropped
template <bool SPLIT>
GRU_DEV void gru_mfma(gf32x16& acc, const gbf16x8& a, const gbf16x8& al, const uint4& bh, const uint4& bl) {
  const gbf16x8 b = __builtin_bit_cast(gbf16x8, bh);
  if (SPLIT) {
    const gbf16x8 bt = __builtin_bit_cast(gbf16x8, bl);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bt, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc, 0, 0, 0);
  }
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

template <bool SPLIT>
__global__ __launch_bounds__(64 * GNW) void k_gru_cell(GruArgs P) {
  constexpr int PLANE = GBM * GLDT;                       // bf16 per plane (heads; tails behind them)
  constexpr int BUF = (SPLIT ? 2 : 1) * PLANE;
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * BUF];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int r0 = (int)blockIdx.x * GBM;
  const int slice = (int)blockIdx.y * GNW + wave;
  const bool wave_on = slice < P.nslices;                 // a wave without a slice only helps moving the rows
  const int nchunks = (P.nks + 1) >> 1;
  const int xsteps = P.Ip >> 4;                           // k steps of the x part: the n tile feeds n_x there, n_h behind

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
        const gf32x4 v = *reinterpret_cast<const gf32x4*>(hrow + (in ? kh : 0));
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
    gbf16x4 h, l;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float v = (ok >> c) & 1u ? raw[c] : 0.0f;
      if (from_h) v *= rfac;                                // the reset, by multiplication (as the stock path's h * (1 - done))
      h[c] = (__bf16)v;
      l[c] = (__bf16)(v - (float)h[c]);
    }
    uint16_t* dst = buf + (t >> 3) * GLDT + kq;
    *reinterpret_cast<gbf16x4*>(dst) = h;
    if (SPLIT) *reinterpret_cast<gbf16x4*>(dst + PLANE) = l;
  };

  gf32x16 acc_r, acc_z, acc_nx, acc_nh;        // of this wave's 32 units x the block's 32 rows
#pragma unroll
  for (int r = 0; r < 16; r++) acc_r[r] = acc_z[r] = acc_nx[r] = acc_nh[r] = 0.0f;

  issue(0);
  for (int c = 0; c < nchunks; c++) {
    uint16_t* buf = lds + (c & 1) * BUF;
    // this chunk's weight fragments: straight from the pack (L2), in flight across the commit and the barrier
    uint4 bh[2][3], bl[2][3];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int ks = 2 * c + s;
        bh[s][j] = bl[s][j] = uint4{0u, 0u, 0u, 0u};
        if (wave_on && ks < P.nks) {                          // (wave-uniform)
          const size_t e = ((size_t)(3 * slice + j) * P.nks + ks) * 64 + lane;
          bh[s][j] = P.bhi[e];
          if (SPLIT) bl[s][j] = P.blo[e];
        }
      }
    commit(buf);
    gru_lds_barrier();           // every wave has committed chunk c, hence finished the MFMAs of chunk c - 1 (the other buffer)
    if (c + 1 < nchunks) issue((c + 1) * GKC);
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int ks = 2 * c + s;
        if (ks < P.nks) {
          const uint16_t* ap = buf + (lane & 31) * GLDT + 16 * s + 8 * (lane >> 5);
          const gbf16x8 a = *reinterpret_cast<const gbf16x8*>(ap);
          gbf16x8 al = a;
          if (SPLIT) al = *reinterpret_cast<const gbf16x8*>(ap + PLANE);
          gru_mfma<SPLIT>(acc_r, a, al, bh[s][0], bl[s][0]);
          gru_mfma<SPLIT>(acc_z, a, al, bh[s][1], bl[s][1]);
          if (ks < xsteps) gru_mfma<SPLIT>(acc_nx, a, al, bh[s][2], bl[s][2]);      // (wave-uniform)
          else gru_mfma<SPLIT>(acc_nh, a, al, bh[s][2], bl[s][2]);
        }
      }
    }
  }

  // epilogue from the accumulators: unit = lane & 31 of the slice, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (!wave_on) return;
  const int u = 32 * slice + (lane & 31);
  if (u >= P.H) return;
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
      const float gr = gru_sigmoid(acc_r[reg] + b_r), gz = gru_sigmoid(acc_z[reg] + b_z);
      const float hn = acc_nh[reg] + b_hn;
      const float gn = tanhf(acc_nx[reg] + b_in + gr * hn);
      P.h_out[e] = (1.0f - gz) * gn + gz * he;              // this form: z == 1 gives rho h_prev bit for bit
      if (P.gates) {
        float* gp = P.gates + (size_t)m * 4 * H + u;
        gp[0] = gr; gp[H] = gz; gp[2 * H] = gn; gp[3 * H] = hn;
      }
    }
  }
}

// fragment order of [W_ih | W_hh]: entry (3 slice + gate, ks, lane) holds unit 32 slice + (lane & 31) of that gate,
// k = 16 ks + 8 (lane >> 5) + j over [x (I, zero-padded to Ip) | h (H)]
__global__ __launch_bounds__(256) void k_gru_pack(const float* __restrict__ w_ih, const float* __restrict__ w_hh, uint4* __restrict__ pack, int I, int Ip,
                                                  int H, int nks, long long entries) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int lane = (int)(e & 63), ks = (int)((e >> 6) % nks), ct = (int)((e >> 6) / nks);
  const int u = 32 * (ct / 3) + (lane & 31), g = ct % 3;
  const size_t row = (size_t)g * H + u;
  gbf16x8 h, l;
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

int gru_fail(const std::string& m) { return shf_mlp_report_error(m.c_str()); }
int gru_ip(int I) { return (I + 15) / 16 * 16; }
int gru_nks(int I, int H) { return gru_ip(I) / 16 + (H + 15) / 16; }
long long gru_entries(int I, int H) { return (long long)((H + 31) / 32) * 3 * gru_nks(I, H) * 64; }
bool gru_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
constexpr int GRU_MAX_DIM = 1 << 15;

}  // namespace

extern "C" int shf_gru_pack_bytes(int32_t I, int32_t H, int64_t* bytes) {
  if (!bytes || I <= 0 || H <= 0 || I > GRU_MAX_DIM || H > GRU_MAX_DIM) return gru_fail("shf_gru_pack_bytes: bad argument (1 <= I, H <= 32768)");
  *bytes = (int64_t)(2 * gru_entries(I, H) * (long long)sizeof(uint4));
  return 0;
}

extern "C" int shf_gru_pack_weights(const float* w_ih, const float* w_hh, void* pack, int32_t I, int32_t H, void* stream) {
  if (!w_ih || !w_hh || !pack) return gru_fail("shf_gru_pack_weights: null tensor");
  if (I <= 0 || H <= 0 || I > GRU_MAX_DIM || H > GRU_MAX_DIM) return gru_fail("shf_gru_pack_weights: bad shape (1 <= I, H <= 32768)");
  if (((uintptr_t)pack & 15u) != 0) return gru_fail("shf_gru_pack_weights: pack must be 16-byte aligned");
  const long long entries = gru_entries(I, H);
  if (entries >= (1ll << 30)) return gru_fail("shf_gru_pack_weights: layer too large");
  hipLaunchKernelGGL(k_gru_pack, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, (uint4*)pack, I,
                     gru_ip(I), H, gru_nks(I, H), entries);
  return hipGetLastError() == hipSuccess ? 0 : gru_fail("shf_gru_pack_weights: launch failed");
}

extern "C" int shf_gru_cell_forward(const float* x, int32_t ldx, const float* h_prev, const unsigned char* reset_or_null, const void* pack,
                                    const float* b_ih, const float* b_hh, float* h_out, float* gates_or_null, int32_t M, int32_t I, int32_t H,
                                    void* stream) {
  if (!x || !h_prev || !pack || !h_out) return gru_fail("shf_gru_cell_forward: null tensor");
  if (M <= 0 || I <= 0 || H <= 0 || ldx < I || I > GRU_MAX_DIM || H > GRU_MAX_DIM)
    return gru_fail("shf_gru_cell_forward: bad shape (M, I, H >= 1, ldx >= I, I and H <= 32768)");
  if ((long long)M * 4 * H >= (1ll << 40) || (long long)M * ldx >= (1ll << 40)) return gru_fail("shf_gru_cell_forward: batch too large");
  if (gru_entries(I, H) >= (1ll << 30)) return gru_fail("shf_gru_cell_forward: layer too large");
  if (((uintptr_t)pack & 15u) != 0) return gru_fail("shf_gru_cell_forward: pack must be 16-byte aligned");
  const size_t state = (size_t)M * H * sizeof(float), xbytes = ((size_t)(M - 1) * ldx + I) * sizeof(float);
  // the blocks of the other unit slices of the same rows read h_prev / x while this one stores: no aliasing
  if (gru_overlap(h_out, state, h_prev, state) || gru_overlap(h_out, state, x, xbytes))
    return gru_fail("shf_gru_cell_forward: h_out overlaps h_prev / x (write the next state to a buffer of its own)");
  if (gates_or_null && (gru_overlap(gates_or_null, 4 * state, h_prev, state) || gru_overlap(gates_or_null, 4 * state, x, xbytes) ||
                        gru_overlap(gates_or_null, 4 * state, h_out, state)))
    return gru_fail("shf_gru_cell_forward: gates overlap another tensor");
  GruArgs P{};
  P.x = x; P.ldx = ldx; P.h_prev = h_prev; P.reset = reset_or_null;
  P.bhi = (const uint4*)pack; P.blo = (const uint4*)pack + gru_entries(I, H);
  P.b_ih = b_ih; P.b_hh = b_hh; P.h_out = h_out; P.gates = gates_or_null;
  P.M = M; P.I = I; P.Ip = gru_ip(I); P.H = H; P.nks = gru_nks(I, H); P.nslices = (H + 31) / 32;
  P.hvec = (H % 4 == 0 && ((uintptr_t)h_prev & 15u) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((M + GBM - 1) / GBM), (unsigned)((P.nslices + GNW - 1) / GNW));
  if (grid.y > 65535u) return gru_fail("shf_gru_cell_forward: layer too large");
  if (shf_mlp_get_precision() != SHF_MLP_BF16) hipLaunchKernelGGL(k_gru_cell<true>, grid, dim3(64 * GNW), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL(k_gru_cell<false>, grid, dim3(64 * GNW), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : gru_fail("shf_gru_cell_forward: launch failed");
}

extern "C" int shf_gru_cell_backward_pointwise(const float* dh, const float* gates, const float* h_prev, const unsigned char* reset_or_null,
                                               float* dgx, float* dgh, float* dh_direct, int32_t M, int32_t H, void* stream) {
  if (!dh || !gates || !h_prev || !dgx || !dgh || !dh_direct) return gru_fail("shf_gru_cell_backward_pointwise: null tensor");
  if (M <= 0 || H <= 0 || H > GRU_MAX_DIM || (long long)M * 4 * H >= (1ll << 40)) return gru_fail("shf_gru_cell_backward_pointwise: bad shape");
  const long long n = (long long)M * H;
  hipLaunchKernelGGL(k_gru_cell_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, gates, h_prev, reset_or_null, dgx,
                     dgh, dh_direct, (long long)M, (int)H);
  return hipGetLastError() == hipSuccess ? 0 : gru_fail("shf_gru_cell_backward_pointwise: launch failed");
}
