// The workgroup scan of the metric kernels (metrics.hip, segmental.hip): one step of a chunked scan and the scan of an array in place.
#pragma once
#include "common.h"

// The workgroup scan (256 threads, integer values: exact in any order).  OP: the combine operation.
struct ScanSum { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a + b; } };
struct ScanMax { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a > b ? a : b; } };
struct ScanMin { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a < b ? a : b; } };

template <typename T> __device__ __forceinline__ T wave_uniform(T v) {      // v is the same in every lane: it can live in scalar registers
  if constexpr (sizeof(T) == 8) {
    const unsigned long long x = (unsigned long long)v;
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((int)x);
    return (T)(((unsigned long long)hi << 32) | lo);
  } else {
    return (T)__builtin_amdgcn_readfirstlane((int)v);
  }
}

// One chunk of a scan.  mine: the combination of this thread's own elements of the chunk (one, or several consecutive ones).
// Returns the combination of everything in front of this thread - the earlier chunks (carry), the earlier waves, the earlier lanes -
// and takes the chunk into carry, which every thread holds (the same value in all of them; initialise it to the identity).  wsum:
// shared, used alternately by `parity` (the chunk's number & 1), so that the one barrier of a step also separates it from the step
// after the next.  Every thread of the workgroup calls it, the same number of times.
template <typename OP, typename T>
__device__ __forceinline__ T wg_scan_step(T mine, T& carry, T (*wsum)[4], int parity) {
  const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
  T incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(incl, o, 64); if (lane >= o) incl = OP::op(incl, u); }
  if (lane == 63) wsum[parity][wave] = incl;
  __syncthreads();
  const T before = __shfl_up(incl, 1, 64);
  T front = carry;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const T total = wave_uniform(wsum[parity][w]);
    if (w < wave) front = OP::op(front, total);
    carry = OP::op(carry, total);
  }
  return lane == 0 ? front : OP::op(front, before);
}

// exclusive scan of v[0 .. m) in place by one workgroup, E consecutive elements per thread; REV: from the back
template <typename OP, bool REV, int E, typename T>
__device__ void wg_scan_array(T* v, int m, T identity, T (*wsum)[4]) {
  T carry = identity;
  for (int base = 0, parity = 0; base < m; base += 256 * E, parity ^= 1) {
    const int j = base + (int)threadIdx.x * E;
    T x[E], mine = identity;
#pragma unroll
    for (int e = 0; e < E; ++e) { x[e] = j + e < m ? v[REV ? m - 1 - (j + e) : j + e] : identity; mine = OP::op(mine, x[e]); }
    T run = wg_scan_step<OP>(mine, carry, wsum, parity);
#pragma unroll
    for (int e = 0; e < E; ++e) { if (j + e < m) v[REV ? m - 1 - (j + e) : j + e] = run; run = OP::op(run, x[e]); }
  }
  __syncthreads();                                              // the result is the workgroup's; wsum is free again
}
