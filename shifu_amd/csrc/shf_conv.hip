// shf_conv.hip -- inference of the vision stage's conv encoders (reference shifu/models/autoencoders.py:26-47,184-200: stacks of
// Conv2d(3 x 3, stride 2, padding 1) + BatchNorm2d + ReLU; examples/abb_pushbox_vision/b_regression_stage.py:106-126).
//
// One layer = one implicit GEMM on the matrix cores:
//   Y[m, co] = relu( (sum_k A[m, k] W[co, k]) * s[co] + t[co] ),   m = (image, oy, ox),   k = (ky, kx, ci) with ci fastest
//   A[m, k]  = X[image, ci, 2 oy + ky - 1, 2 ox + kx - 1]   (zero outside the image)
// Operand scheme of shf_mlp.hip: values are split into a bf16 head and the bf16 of what the head lost (bf16 x 3: a * bl,
// al * b, a * b; tail * tail dropped), v_mfma_f32_32x32x16_bf16, fp32 accumulation; shf_mlp_set_precision(SHF_MLP_BF16)
// drops the tails.  s and t are the eval-mode batch norm and the conv bias, applied in fp32 in the epilogue (they are
// NOT folded into the bf16 weights).
//   * A block owns 32 NW output pixels (one 32-row MFMA tile per wave) and up to 128 output channels (four column tiles,
//     all of them accumulated by every wave, so the gathered A rows are read once per 128 channels).
//   * A goes through LDS in chunks of 32 k: the loads of chunk c + 1 are issued before the MFMAs of chunk c and committed
//     (head + tail) to the other buffer after them -- one barrier per chunk.
//   * W is not staged: shf_conv_pack_weights lays it out once in fragment order ([column tile][k step][lane] -> 8 bf16),
//     a wave's B fragment is one contiguous 1 KB load from L2.
//   * A row of the output depends on its own image only: no atomics, no split reduction, the k order is fixed -- results
//     do not depend on the batch size or on an image's place in the batch.
// Activations between layers are fp32 NHWC (a k run is contiguous: 16-byte loads when C_in % 4 == 0); the first layer reads
// the caller's tensor in place through element strides -- fp32, fp32 negated (the camera's depth image) or u8 scaled to
// [0, 1] (its rgba image); the last layer can store in NCHW (torch.flatten) order for the fully connected layers behind it.
// Non-finite input: an infinite pixel gives head = inf, tail = inf - inf = NaN, so every output of THAT image that the
// pixel reaches becomes NaN (the ReLU here keeps NaN, as torch's does); other images never read it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

#define CONV_DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(8))) __bf16 cbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 cbf16x4;
typedef __attribute__((ext_vector_type(16))) float cf32x16;
typedef __attribute__((ext_vector_type(4))) float cf32x4;

namespace {

constexpr int CKC = 32, CLDT = CKC + 8;   // k per chunk; LDS row = 40 bf16 = 80 B (16-byte aligned fragments, staggered banks)
constexpr int CMAXCT = 4;                 // column tiles (of 32 output channels) per block

struct ConvArgs {
  const void* x;
  long long sn, sc, sh, sw;   // element strides of the input's (image, channel, row, column)
  int kind;                   // SHF_CONV_SRC_*
  int cin, H, W, Ho, Wo, cout;
  int K, nks;                 // 9 cin; k steps of 16 (K rounded up)
  uint32_t cin_magic;         // floor(2^32 / cin) + 1: k / cin = umulhi(k, magic) for k < 2^16 (cin >= 2)
  const uint4* bhi;           // [ceil(cout / 32)][nks][64] fragments of the bf16 heads
  const uint4* blo;           // ... of the tails
  const float* scale;         // [cout]
  const float* shift;         // [cout]
  float* y;
  int flatten;                // 0: y[m][co] (NHWC), 1: y[image][co][oy][ox]
  int M;                      // images * Ho * Wo
};

CONV_DEV int conv_tap(const ConvArgs& P, int k) { return P.cin == 1 ? k : (int)__umulhi((uint32_t)k, P.cin_magic); }
CONV_DEV void conv_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// NW waves per block (32 output pixels each).  VEC: fp32 NHWC input with C_in % 4 == 0, 16-byte loads.
template <int NW, bool VEC, bool SPLIT>
__global__ __launch_bounds__(64 * NW) void k_conv3x3s2(ConvArgs P) {
  constexpr int T = 64 * NW, BM = 32 * NW;
  constexpr int PLANE = BM * CLDT;                        // bf16 per plane (heads; tails behind them)
  constexpr int BUF = (SPLIT ? 2 : 1) * PLANE;
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * BUF];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int r0 = (int)blockIdx.x * BM;
  const int ct0 = (int)blockIdx.y * CMAXCT;
  const int nct_all = (P.cout + 31) >> 5;
  const int nct = nct_all - ct0 < CMAXCT ? nct_all - ct0 : CMAXCT;
  const int nchunks = (P.nks + 1) >> 1;

  // this thread's share of a chunk: rows (t >> 3) + (T / 8) u, u = 0 .. 3, the four k  4 (t & 7) .. + 3  of each
  const int kq = 4 * (t & 7);
  long long base[4];
  int iy0[4], ix0[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int m = r0 + (t >> 3) + (T / 8) * u;
    const bool in = m < P.M;
    const int mm = in ? m : 0;
    const int img = mm / (P.Ho * P.Wo), p = mm - img * (P.Ho * P.Wo);
    const int oy = p / P.Wo, ox = p - oy * P.Wo;
    base[u] = (long long)img * P.sn;
    iy0[u] = in ? 2 * oy - 1 : -(1 << 20);               // rows beyond M: every tap is outside the image
    ix0[u] = 2 * ox - 1;
  }

  uint32_t raw[16];      // VEC: 4 x 16 bytes; else 16 scalars (a byte each for the u8 source)
  uint32_t ok;           // bit (4 u + c): element is inside the image and below K
  auto issue = [&](int k0) {
    ok = 0u;
    if (VEC) {
      const int k = k0 + kq;
      const int tap = conv_tap(P, k), ci = k - tap * P.cin;
      const int ky = tap / 3, kx = tap - 3 * ky;
      const float* xp = reinterpret_cast<const float*>(P.x);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int iy = iy0[u] + ky, ix = ix0[u] + kx;
        const bool in = k < P.K && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
        const long long off = in ? base[u] + (long long)iy * P.sh + (long long)ix * P.sw + ci : 0ll;
        const cf32x4 v = *reinterpret_cast<const cf32x4*>(xp + off);
#pragma unroll
        for (int c = 0; c < 4; c++) raw[4 * u + c] = __float_as_uint(v[c]);
        ok |= (in ? 0xFu : 0u) << (4 * u);
      }
    } else {
      int ky[4], kx[4];
      long long coff[4];
      bool kin[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int k = k0 + kq + c;
        const int tap = conv_tap(P, k), ci = k - tap * P.cin;
        ky[c] = tap / 3; kx[c] = tap - 3 * ky[c];
        coff[c] = (long long)ci * P.sc;
        kin[c] = k < P.K;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int iy = iy0[u] + ky[c], ix = ix0[u] + kx[c];
          const bool in = kin[c] && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
          const long long off = in ? base[u] + coff[c] + (long long)iy * P.sh + (long long)ix * P.sw : 0ll;
          if (P.kind == SHF_CONV_SRC_U8_UNORM) raw[4 * u + c] = reinterpret_cast<const unsigned char*>(P.x)[off];
          else raw[4 * u + c] = reinterpret_cast<const uint32_t*>(P.x)[off];
          ok |= (in ? 1u : 0u) << (4 * u + c);
        }
    }
  };
  auto commit = [&](uint16_t* buf) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      cbf16x4 h, l;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        float v;
        if (!VEC && P.kind == SHF_CONV_SRC_U8_UNORM) v = (float)raw[4 * u + c] * (1.0f / 255.0f);   // as torch.div(u8, 255.0): see the header
        else if (!VEC && P.kind == SHF_CONV_SRC_F32_NEG) v = -__uint_as_float(raw[4 * u + c]);
        else v = __uint_as_float(raw[4 * u + c]);
        v = (ok >> (4 * u + c)) & 1u ? v : 0.0f;
        h[c] = (__bf16)v;
        l[c] = (__bf16)(v - (float)h[c]);
      }
      uint16_t* dst = buf + ((t >> 3) + (T / 8) * u) * CLDT + kq;
      *reinterpret_cast<cbf16x4*>(dst) = h;
      if (SPLIT) *reinterpret_cast<cbf16x4*>(dst + PLANE) = l;
    }
  };

  cf32x16 acc[CMAXCT];
#pragma unroll
  for (int j = 0; j < CMAXCT; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;

  issue(0);
  for (int c = 0; c < nchunks; c++) {
    uint16_t* buf = lds + (c & 1) * BUF;
    // this chunk's weight fragments: straight from the pack (L2), in flight across the commit and the barrier
    uint4 bh[2][CMAXCT], bl[2][CMAXCT];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
      for (int j = 0; j < CMAXCT; j++) {
        const int ks = 2 * c + s;
        const bool in = j < nct && ks < P.nks;
        bh[s][j] = bl[s][j] = uint4{0u, 0u, 0u, 0u};
        if (in) {                                            // (uniform: narrow layers skip the tiles they do not have)
          const size_t e = ((size_t)(ct0 + j) * P.nks + ks) * 64 + lane;
          bh[s][j] = P.bhi[e];
          if (SPLIT) bl[s][j] = P.blo[e];
        }
      }
    commit(buf);
    conv_lds_barrier();          // every wave has committed chunk c, hence finished the MFMAs of chunk c - 1 (the other buffer)
    if (c + 1 < nchunks) issue((c + 1) * CKC);
#pragma unroll
    for (int s = 0; s < 2; s++) {
      if (2 * c + s < P.nks) {
        const uint16_t* ap = buf + (wave * 32 + (lane & 31)) * CLDT + 16 * s + 8 * (lane >> 5);
        const cbf16x8 a = *reinterpret_cast<const cbf16x8*>(ap);
        cbf16x8 al;
        if (SPLIT) al = *reinterpret_cast<const cbf16x8*>(ap + PLANE);
#pragma unroll
        for (int j = 0; j < CMAXCT; j++)
          if (j < nct) {
            const cbf16x8 b = __builtin_bit_cast(cbf16x8, bh[s][j]);
            if (SPLIT) {
              // the two cross terms first (small), then head * head; tail * tail (2^-18 relative) is dropped
              const cbf16x8 bt = __builtin_bit_cast(cbf16x8, bl[s][j]);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bt, acc[j], 0, 0, 0);
              acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc[j], 0, 0, 0);
            }
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
          }
      }
    }
  }

  // epilogue from the accumulators: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int hw = P.Ho * P.Wo;
#pragma unroll
  for (int j = 0; j < CMAXCT; j++)
    if (j < nct) {
      const int col = (ct0 + j) * 32 + (lane & 31);
      if (col < P.cout) {
        const float s = P.scale[col], sh = P.shift[col];
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int m = r0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
          if (m < P.M) {
            float v = acc[j][reg] * s + sh;
            v = v < 0.0f ? 0.0f : v;                       // ReLU that keeps NaN
            if (P.flatten) {
              const int img = m / hw, p = m - img * hw;
              P.y[((size_t)img * P.cout + col) * hw + p] = v;
            } else {
              P.y[(size_t)m * P.cout + col] = v;
            }
          }
        }
      }
    }
}

// fragment order of W[co][ci][ky][kx]: entry (ct, ks, lane) holds column ct * 32 + (lane & 31), k = 16 ks + 8 (lane >> 5) + j
__global__ void k_conv_pack(const float* w, uint4* pack, int cin, int cout, int nks, int entries) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= entries) return;
  const int lane = e & 63, ks = (e >> 6) % nks, ct = (e >> 6) / nks;
  const int col = ct * 32 + (lane & 31);
  cbf16x8 h, l;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int k = 16 * ks + 8 * (lane >> 5) + j;
    const int tap = k / cin, ci = k - tap * cin;
    const float v = (col < cout && tap < 9) ? w[((size_t)col * cin + ci) * 9 + tap] : 0.0f;
    h[j] = (__bf16)v;
    l[j] = (__bf16)(v - (float)h[j]);
  }
  pack[e] = __builtin_bit_cast(uint4, h);
  pack[entries + e] = __builtin_bit_cast(uint4, l);
}

thread_local std::string g_conv_err;
int conv_fail(const std::string& m) { g_conv_err = m; return 1; }
int conv_nks(int cin) { return (9 * cin + 15) / 16; }
long long conv_entries(int cin, int cout) { return (long long)((cout + 31) / 32) * conv_nks(cin) * 64; }

template <int NW, bool VEC>
void conv_launch(dim3 grid, hipStream_t st, const ConvArgs& P, bool split) {
  if (split) hipLaunchKernelGGL((k_conv3x3s2<NW, VEC, true>), grid, dim3(64 * NW), 0, st, P);
  else hipLaunchKernelGGL((k_conv3x3s2<NW, VEC, false>), grid, dim3(64 * NW), 0, st, P);
}

}  // namespace

extern "C" const char* shf_conv_last_error(void) { return g_conv_err.c_str(); }

extern "C" int shf_conv_pack_bytes(int32_t cin, int32_t cout, int64_t* bytes) {
  if (!bytes || cin <= 0 || cout <= 0 || cin > 7000) return conv_fail("shf_conv_pack_bytes: bad argument (1 <= C_in <= 7000, C_out >= 1)");
  *bytes = (int64_t)(2 * conv_entries(cin, cout) * (long long)sizeof(uint4));
  return 0;
}

extern "C" int shf_conv_pack_weights(const float* w, void* pack, int32_t cin, int32_t cout, void* stream) {
  if (!w || !pack || cin <= 0 || cout <= 0 || cin > 7000) return conv_fail("shf_conv_pack_weights: bad argument");
  if (((uintptr_t)pack & 15u) != 0) return conv_fail("shf_conv_pack_weights: pack must be 16-byte aligned");
  const long long entries = conv_entries(cin, cout);
  if (entries >= (1ll << 30)) return conv_fail("shf_conv_pack_weights: layer too large");
  hipLaunchKernelGGL(k_conv_pack, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (uint4*)pack, cin, cout,
                     conv_nks(cin), (int)entries);
  return hipGetLastError() == hipSuccess ? 0 : conv_fail("shf_conv_pack_weights: launch failed");
}

extern "C" int shf_conv3x3s2_forward(const void* x, int32_t src_kind, const int64_t* strides, const void* pack, const float* scale,
                                     const float* shift, float* y, int32_t flatten, int32_t nimg, int32_t cin, int32_t h, int32_t w,
                                     int32_t cout, void* stream) {
  if (!x || !strides || !pack || !scale || !shift || !y) return conv_fail("shf_conv3x3s2_forward: null argument");
  if (src_kind != SHF_CONV_SRC_F32 && src_kind != SHF_CONV_SRC_F32_NEG && src_kind != SHF_CONV_SRC_U8_UNORM)
    return conv_fail("shf_conv3x3s2_forward: unknown source kind");
  if (nimg <= 0 || cin <= 0 || cin > 7000 || cout <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1))
    return conv_fail("shf_conv3x3s2_forward: bad shape (H and W even, 1 <= C_in <= 7000)");
  for (int i = 0; i < 4; i++)
    if (strides[i] < 0) return conv_fail("shf_conv3x3s2_forward: negative stride");
  const int ho = h / 2, wo = w / 2;
  const long long M = (long long)nimg * ho * wo;
  if (M >= (1ll << 31) - 256 || M * cout >= (1ll << 40)) return conv_fail("shf_conv3x3s2_forward: batch too large");
  ConvArgs P{};
  P.x = x; P.sn = strides[0]; P.sc = strides[1]; P.sh = strides[2]; P.sw = strides[3];
  P.kind = src_kind; P.cin = cin; P.H = h; P.W = w; P.Ho = ho; P.Wo = wo; P.cout = cout;
  P.K = 9 * cin; P.nks = conv_nks(cin);
  P.cin_magic = cin > 1 ? (uint32_t)((1ull << 32) / (uint32_t)cin) + 1u : 0u;
  P.bhi = (const uint4*)pack; P.blo = (const uint4*)pack + conv_entries(cin, cout);
  P.scale = scale; P.shift = shift; P.y = y; P.flatten = flatten ? 1 : 0; P.M = (int)M;
  const bool split = shf_mlp_get_precision() != SHF_MLP_BF16;
  const bool vec = src_kind == SHF_CONV_SRC_F32 && cin % 4 == 0 && strides[1] == 1 && strides[3] % 4 == 0 && strides[2] % 4 == 0 &&
                   strides[0] % 4 == 0 && ((uintptr_t)x & 15u) == 0;
  const int gy = ((cout + 31) / 32 + CMAXCT - 1) / CMAXCT;
  // waves per block: fewer when 128-pixel blocks would leave CUs (256) without work
  const int nw = (M + 127) / 128 * gy >= 512 ? 4 : (M + 63) / 64 * gy >= 512 ? 2 : 1;
  const dim3 grid((unsigned)((M + 32 * nw - 1) / (32 * nw)), (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
#define SHF_CONV_GO(NWV) do { if (vec) conv_launch<NWV, true>(grid, st, P, split); else conv_launch<NWV, false>(grid, st, P, split); } while (0)
  if (nw == 4) SHF_CONV_GO(4); else if (nw == 2) SHF_CONV_GO(2); else SHF_CONV_GO(1);
#undef SHF_CONV_GO
  return hipGetLastError() == hipSuccess ? 0 : conv_fail("shf_conv3x3s2_forward: launch failed");
}
