// block_dev.hpp — workgroup primitives shared by the kernels: the fixed-order block sum (int or f64) and the ordered append
// ("Workgroup primitives").  Every thread of the workgroup must reach each call; THREADS is the workgroup's size, a
// multiple of 64.
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Fixed-order sum of NV values (int or double) over the workgroup, in every thread: shuffle tree inside each wave, then every thread
// adds the wave totals in wave order (the same bits in every thread, whatever the batch).  s_w: LDS [THREADS / 64][NV].  One barrier
// before the store (s_w may still be read from an earlier use) and one after.
template <int THREADS, int NV, typename T>
__device__ __forceinline__ void block_sum(T (&v)[NV], T* __restrict__ s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s_w[wave * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    T t = 0;
    for (int w = 0; w < THREADS / 64; ++w) t += s_w[w * NV + k];
    v[k] = t;
  }
}

// The workgroup's sum of one int.  wave_tot: LDS [THREADS / 64].
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int* wave_tot) {
  int a[1] = {v};
  block_sum<THREADS, 1>(a, wave_tot);
  return a[0];
}

// Ordered append of NF flag sets at once.  Each round every thread passes its flags; at[f] is the number of threads flagged in f
// before this one, in thread order, over this and all earlier rounds, plus whatever total[f] started from — the place of a flagged
// thread's entry.  total[f] is the same in every thread: the count so far, which a caller may set between rounds (a list that
// continues another's).  Two barriers per round; the first also covers an earlier use of the same LDS.
template <int THREADS, int NF>
struct BlockAppend {
  int* wave_tot;      // LDS [THREADS / 64][NF]
  int total[NF];
  __device__ __forceinline__ explicit BlockAppend(int* lds) : wave_tot(lds) {
#pragma unroll
    for (int f = 0; f < NF; ++f) total[f] = 0;
  }
  __device__ __forceinline__ void round(const bool (&flag)[NF], int (&at)[NF]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) m[f] = __ballot(flag[f]);
    __syncthreads();                                                      // (the previous round's totals are no longer read)
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < NF; ++f) wave_tot[wave * NF + f] = __popcll(m[f]);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < THREADS / 64; ++w) { const int t = wave_tot[w * NF + f]; before += w < wave ? t : 0; all += t; }
      at[f] = total[f] + before + __popcll(m[f] & ((1ull << lane) - 1ull));
      total[f] += all;
    }
  }
  __device__ __forceinline__ int round(bool flag) {                       // NF == 1
    const bool fl[1] = {flag};
    int at[1];
    round(fl, at);
    return at[0];
  }
};

}  // namespace
