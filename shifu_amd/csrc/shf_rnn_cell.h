// shf_rnn_cell.h -- the GEMM core the recurrent cell kernels share (shf_lstm.hip, shf_gru.hip): one cell step is
//   pre[m, g H + u] = sum_k [x | rho h_prev][m, k] [W_ih | W_hh][g H + u, k]          rho = reset[m] ? 0 : 1
// as one GEMM on the matrix cores whose epilogue is the cell's whole pointwise update: the pre-activations never reach
// memory.  A cell type supplies a policy (below) -- its argument struct, its number of column tiles per unit slice and its
// epilogue -- and its own extern "C" entries; everything else is here, once.
//   * Operand scheme of shf_mlp.hip / shf_conv.hip: bf16 head + tail (a * bl, al * b, a * b; tail * tail dropped),
//     v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same k order; shf_mlp_set_precision(SHF_MLP_BF16) drops the tails.
//   * A block owns 32 rows and up to four slices of 32 hidden units; wave w keeps FOUR accumulators (4 x 16 registers) of
//     its slice's units, so everything the update of a (row, unit) pair needs meets in one lane's registers.  The pack has
//     NT column tiles per slice (one per gate).  With NT = 4 tile j feeds accumulator j.  A cell with NT = 3 may ask
//     (SPLIT_LAST) for its last tile's product to go into accumulator 2 for the k steps of the x part (ks < Ip / 16) and into
//     accumulator 3 for those of the h part; the test is wave-uniform and each side names its accumulator at compile time.
//   * k padding: the reduction index runs over [x | h]; the x part is zero-padded to a whole k step (16) so that h starts on
//     a step boundary (Ip is a multiple of 16, not of the chunk's 32: the switch can fall between the two k steps of one
//     chunk).
//   * Two-buffer pipeline: the gathered rows go through LDS in chunks of 32 k, two buffers: the loads of chunk c + 1 are
//     issued before the MFMAs of chunk c and committed (head + tail) after them -- one barrier per chunk (shf_conv.hip's
//     scheme).  The reset factor is applied as the h rows are committed; the epilogue applies it to whatever else it reads
//     of the previous state.
//   * The weights are not staged: k_rnn_pack lays [W_ih | W_hh] out once in fragment order, column tiles reordered so
//     that the NT gate tiles of a unit slice are adjacent ([NT slice + gate][k step][lane] -> 8 bf16); a wave's B fragment
//     is one contiguous 1 KB load from L2.
//   * Aliasing: the outputs must not overlap h_prev / x (or any other previous state the epilogue reads): the blocks of the
//     other unit slices of the same rows still read them.  The host entries refuse overlapping ranges (rnn_overlap).
// A row of the output depends on its own rows of the inputs only: no atomics, no split reduction, no scratch, no host
// synchronisation -- capturable, and independent of the batch size and of a row's place in the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

#define RNN_DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(8))) __bf16 rbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 rbf16x4;
typedef __attribute__((ext_vector_type(16))) float rf32x16;
typedef __attribute__((ext_vector_type(4))) float rf32x4;

int shf_mlp_report_error(const char* message);     // csrc/shf_mlp.hip: sets the text shf_mlp_last_error returns; returns 1

namespace {

constexpr int RKC = 32, RLDT = RKC + 8;   // k per chunk; LDS row = 40 bf16 = 80 B (16-byte aligned fragments, staggered banks)
constexpr int RBM = 32, RNW = 4;          // rows per block; waves (= unit slices) per block

RNN_DEV void rnn_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
RNN_DEV float rnn_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// acc += a * b with the head + tail scheme: the two cross terms first (small), then head * head; tail * tail (2^-18
// relative) is dropped
template <bool SPLIT>
RNN_DEV void rnn_mfma(rf32x16& acc, const rbf16x8& a, const rbf16x8& al, const uint4& bh, const uint4& bl) {
  const rbf16x8 b = __builtin_bit_cast(rbf16x8, bh);
  if (SPLIT) {
    const rbf16x8 bt = __builtin_bit_cast(rbf16x8, bl);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bt, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc, 0, 0, 0);
  }
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// The cell step.  A policy `Cell` gives
//   Args        the kernel's argument struct.  The core reads x, ldx, h_prev, reset (one byte per row, or null), bhi / blo
//               (the pack's heads and tails), M, I, Ip (I rounded up to 16), H, nks (k steps of 16 over [x | h]), nslices
//               (slices of 32 units) and hvec (h_prev rows are whole 16-byte chunks: H % 4 == 0, base aligned); rnn_launch
//               fills the derived ones.  The rest is the epilogue's.
//   NT          column tiles per unit slice in the pack (3 or 4)
//   SPLIT_LAST  route the last tile's product to accumulator 3 for the k steps of the h part (needs NT == 3)
//   epilogue(P, acc, u, r0, lane)   from the four accumulators to the stores: this lane holds unit u (< H) of rows
//               r0 + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), reg = 0 .. 15, of which those < M exist
template <class Cell, bool SPLIT>
__global__ __launch_bounds__(64 * RNW) void k_rnn_cell(typename Cell::Args P) {
  constexpr int NT = Cell::NT;
  static_assert(Cell::SPLIT_LAST ? NT == 3 : NT == 4, "four accumulators: four tiles, or three with the last one split");
  constexpr int PLANE = RBM * RLDT;                       // bf16 per plane (heads; tails behind them)
  constexpr int BUF = (SPLIT ? 2 : 1) * PLANE;
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * BUF];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int r0 = (int)blockIdx.x * RBM;
  const int slice = (int)blockIdx.y * RNW + wave;
  const bool wave_on = slice < P.nslices;                 // a wave without a slice only helps moving the rows
  const int nchunks = (P.nks + 1) >> 1;
  const int xsteps = P.Ip >> 4;                           // k steps of the x part (SPLIT_LAST)

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
        const rf32x4 v = *reinterpret_cast<const rf32x4*>(hrow + (in ? kh : 0));
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
    rbf16x4 h, l;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float v = (ok >> c) & 1u ? raw[c] : 0.0f;
      if (from_h) v *= rfac;                                // the reset, by multiplication (as the stock path's h * (1 - done))
      h[c] = (__bf16)v;
      l[c] = (__bf16)(v - (float)h[c]);
    }
    uint16_t* dst = buf + (t >> 3) * RLDT + kq;
    *reinterpret_cast<rbf16x4*>(dst) = h;
    if (SPLIT) *reinterpret_cast<rbf16x4*>(dst + PLANE) = l;
  };

  rf32x16 acc[4];        // of this wave's 32 units x the block's 32 rows
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;

  issue(0);
  for (int c = 0; c < nchunks; c++) {
    uint16_t* buf = lds + (c & 1) * BUF;
    // this chunk's weight fragments: straight from the pack (L2), in flight across the commit and the barrier
    uint4 bh[2][NT], bl[2][NT];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const int ks = 2 * c + s;
        bh[s][j] = bl[s][j] = uint4{0u, 0u, 0u, 0u};
        if (wave_on && ks < P.nks) {                          // (wave-uniform)
          const size_t e = ((size_t)(NT * slice + j) * P.nks + ks) * 64 + lane;
          bh[s][j] = P.bhi[e];
          if (SPLIT) bl[s][j] = P.blo[e];
        }
      }
    commit(buf);
    rnn_lds_barrier();           // every wave has committed chunk c, hence finished the MFMAs of chunk c - 1 (the other buffer)
    if (c + 1 < nchunks) issue((c + 1) * RKC);
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int ks = 2 * c + s;
        if (ks < P.nks) {
          const uint16_t* ap = buf + (lane & 31) * RLDT + 16 * s + 8 * (lane >> 5);
          const rbf16x8 a = *reinterpret_cast<const rbf16x8*>(ap);
          rbf16x8 al = a;
          if (SPLIT) al = *reinterpret_cast<const rbf16x8*>(ap + PLANE);
#pragma unroll
          for (int j = 0; j < (Cell::SPLIT_LAST ? 2 : 4); j++) rnn_mfma<SPLIT>(acc[j], a, al, bh[s][j], bl[s][j]);
          if (Cell::SPLIT_LAST) {
            if (ks < xsteps) rnn_mfma<SPLIT>(acc[2], a, al, bh[s][2], bl[s][2]);      // (wave-uniform)
            else rnn_mfma<SPLIT>(acc[3], a, al, bh[s][2], bl[s][2]);
          }
        }
      }
    }
  }

  if (!wave_on) return;
  const int u = 32 * slice + (lane & 31);
  if (u >= P.H) return;
  Cell::epilogue(P, acc, u, r0, lane);
}

// fragment order of [W_ih | W_hh]: entry (NT slice + gate, ks, lane) holds unit 32 slice + (lane & 31) of that gate,
// k = 16 ks + 8 (lane >> 5) + j over [x (I, zero-padded to Ip) | h (H)]
template <int NT>
__global__ __launch_bounds__(256) void k_rnn_pack(const float* __restrict__ w_ih, const float* __restrict__ w_hh, uint4* __restrict__ pack, int I, int Ip,
                                                  int H, int nks, long long entries) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int lane = (int)(e & 63), ks = (int)((e >> 6) % nks);
  const unsigned ct = (unsigned)((e >> 6) / nks);           // (unsigned: / and % by a power of two stay a shift and a mask)
  const int u = (int)(32u * (ct / NT)) + (lane & 31), g = (int)(ct % NT);
  const size_t row = (size_t)g * H + u;
  rbf16x8 h, l;
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

// ---------------------------------------------------------------- host side: what the extern "C" entries share
int rnn_fail(const std::string& m) { return shf_mlp_report_error(m.c_str()); }
int rnn_ip(int I) { return (I + 15) / 16 * 16; }
int rnn_nks(int I, int H) { return rnn_ip(I) / 16 + (H + 15) / 16; }
long long rnn_entries(int NT, int I, int H) { return (long long)((H + 31) / 32) * NT * rnn_nks(I, H) * 64; }
bool rnn_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
constexpr int RNN_MAX_DIM = 1 << 15;

// `name`: the entry's, for the message
int rnn_pack_bytes(const char* name, int NT, int32_t I, int32_t H, int64_t* bytes) {
  if (!bytes || I <= 0 || H <= 0 || I > RNN_MAX_DIM || H > RNN_MAX_DIM) return rnn_fail(std::string(name) + ": bad argument (1 <= I, H <= 32768)");
  *bytes = (int64_t)(2 * rnn_entries(NT, I, H) * (long long)sizeof(uint4));
  return 0;
}

template <int NT>
int rnn_pack_weights(const char* name, const float* w_ih, const float* w_hh, void* pack, int32_t I, int32_t H, void* stream) {
  const std::string n(name);
  if (!w_ih || !w_hh || !pack) return rnn_fail(n + ": null tensor");
  if (I <= 0 || H <= 0 || I > RNN_MAX_DIM || H > RNN_MAX_DIM) return rnn_fail(n + ": bad shape (1 <= I, H <= 32768)");
  if (((uintptr_t)pack & 15u) != 0) return rnn_fail(n + ": pack must be 16-byte aligned");
  const long long entries = rnn_entries(NT, I, H);
  if (entries >= (1ll << 30)) return rnn_fail(n + ": layer too large");
  hipLaunchKernelGGL(k_rnn_pack<NT>, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, (uint4*)pack, I,
                     rnn_ip(I), H, rnn_nks(I, H), entries);
  return hipGetLastError() == hipSuccess ? 0 : rnn_fail(n + ": launch failed");
}

// the checks of a cell_forward entry that do not depend on the cell's own tensors (after its null check, before its overlap list)
int rnn_forward_check(const char* name, int NT, const void* pack, int32_t ldx, int32_t M, int32_t I, int32_t H) {
  const std::string n(name);
  if (M <= 0 || I <= 0 || H <= 0 || ldx < I || I > RNN_MAX_DIM || H > RNN_MAX_DIM)
    return rnn_fail(n + ": bad shape (M, I, H >= 1, ldx >= I, I and H <= 32768)");
  if ((long long)M * 4 * H >= (1ll << 40) || (long long)M * ldx >= (1ll << 40)) return rnn_fail(n + ": batch too large");
  if (rnn_entries(NT, I, H) >= (1ll << 30)) return rnn_fail(n + ": layer too large");
  if (((uintptr_t)pack & 15u) != 0) return rnn_fail(n + ": pack must be 16-byte aligned");
  return 0;
}

// fills what the core reads of P (the epilogue's own fields are the caller's) and launches the cell at the current precision
template <class Cell>
int rnn_launch(const char* name, typename Cell::Args& P, const float* x, int32_t ldx, const float* h_prev, const unsigned char* reset_or_null,
               const void* pack, int32_t M, int32_t I, int32_t H, void* stream) {
  P.x = x; P.ldx = ldx; P.h_prev = h_prev; P.reset = reset_or_null;
  P.bhi = (const uint4*)pack; P.blo = (const uint4*)pack + rnn_entries(Cell::NT, I, H);
  P.M = M; P.I = I; P.Ip = rnn_ip(I); P.H = H; P.nks = rnn_nks(I, H); P.nslices = (H + 31) / 32;
  P.hvec = (H % 4 == 0 && ((uintptr_t)h_prev & 15u) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((M + RBM - 1) / RBM), (unsigned)((P.nslices + RNW - 1) / RNW));
  if (grid.y > 65535u) return rnn_fail(std::string(name) + ": layer too large");
  if (shf_mlp_get_precision() != SHF_MLP_BF16) hipLaunchKernelGGL((k_rnn_cell<Cell, true>), grid, dim3(64 * RNW), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL((k_rnn_cell<Cell, false>), grid, dim3(64 * RNW), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : rnn_fail(std::string(name) + ": launch failed");
}

}  // namespace
