// shf_k_cap_select_test.hip -- the selection at the contact cap (csrc/shf_chain_hard.h: hard_cap_select) on given candidates, outside
// any env step: the entry point tests/test_gpu_cap_select.py holds to a stable sort by (gap, position).
#include <hip/hip_runtime.h>

#include "shf_chain.h"
#include "shf_chain_hard.h"

int shf_set_error(const std::string& msg);

// Two envs per wavefront at 32 lanes each, as in the step: lane l holds the slots l, l + 32, l + 64 (88 slots: the last eight
// lanes have no third) and self entry l.  A wavefront's second half beyond n is an env without candidates and stores nothing.
__global__ __launch_bounds__(64) void k_cap_select_test(int n, const float* gaps, const unsigned char* flags, const int* kmax, unsigned char* kept) {
  constexpr int G = 32, NR = 3, NS = SHF_CAP_TEST_SLOTS, ROW = NS + G;
  const int l = threadIdx.x % G, lane0 = (int)(threadIdx.x & 63u) - l;
  const int e = blockIdx.x * 2 + threadIdx.x / G;
  const bool on = e < n;
  const size_t base = (size_t)(on ? e : 0) * ROW;
  float ph[NR], sph = 0.0f;
  bool cand[NR], scand;
  int total = 0;
#pragma unroll
  for (int k = 0; k < NR; k++) {
    const int s = l + k * G;
    cand[k] = on && s < NS && flags[base + (s < NS ? s : 0)] != 0;
    ph[k] = cand[k] ? gaps[base + s] : 0.0f;
    total += __popcll((__ballot(cand[k]) >> lane0) & ((1ull << G) - 1ull));
  }
  scand = on && flags[base + NS + l] != 0;
  if (scand) sph = gaps[base + NS + l];
  total += __popcll((__ballot(scand) >> lane0) & ((1ull << G) - 1ull));
  const int km = on ? kmax[e] : 1;
  if (__ballot(total > km) != 0ull) hard_cap_select<G, NR, true>(l, lane0, total, km, ph, cand, sph, scand);
  if (on) {
#pragma unroll
    for (int k = 0; k < NR; k++) {
      const int s = l + k * G;
      if (s < NS) kept[base + s] = cand[k] ? 1 : 0;
    }
    kept[base + NS + l] = scand ? 1 : 0;
  }
}

extern "C" int shf_cap_select_test(int32_t n, const float* gaps_dev, const uint8_t* flags_dev, const int32_t* kmax_dev, uint8_t* kept_dev, void* stream) {
  if (n <= 0 || !gaps_dev || !flags_dev || !kmax_dev || !kept_dev) return shf_set_error("shf_cap_select_test: bad argument");
  hipLaunchKernelGGL(k_cap_select_test, dim3((n + 1) / 2), dim3(64), 0, (hipStream_t)stream, n, gaps_dev, flags_dev, kmax_dev, kept_dev);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_cap_select_test: launch failed");
}
