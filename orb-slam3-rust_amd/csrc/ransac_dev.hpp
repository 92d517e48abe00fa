// ransac_dev.hpp — the sampler of the RANSAC kernels (PnP: pnp_kernels.hip, Sim3: loop_verify_kernels.hip), DESIGN.md §2.
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

constexpr int RANSAC_DRAWS = 64;         // sampler draws per hypothesis

// The sampler [spec]: hypothesis h, draw a -> splitmix64(seed + golden * (h*64 + a + 1)); idx = ((z >> 32) * n) >> 32; duplicates
// skipped.  True when m <= M_MAX distinct indices were drawn within 64 draws.  A function of (seed, h, n, m) alone: a problem's
// samples are the same alone and inside any batch.
template <int M_MAX>
__device__ __forceinline__ bool ransac_sample(uint64_t seed, int h, int n, int m, int (&idx)[M_MAX]) {
  int k = 0;
  for (int a = 0; a < RANSAC_DRAWS && k < m; ++a) {
    const uint64_t x = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(h * 64 + a + 1);
    uint64_t z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const int i = (int)(((z >> 32) * (uint64_t)n) >> 32);
    bool dup = false;
#pragma unroll
    for (int j = 0; j < M_MAX; ++j) dup |= (j < k && idx[j] == i);
    if (dup) continue;
#pragma unroll
    for (int j = 0; j < M_MAX; ++j) if (j == k) idx[j] = i;   // (constant register index: no scratch)
    ++k;
  }
  return k == m;
}

}  // namespace
