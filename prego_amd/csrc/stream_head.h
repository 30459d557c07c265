// The tail of the streaming classifiers (stream_gates_head of stream_step.hip, stream_ant_head of stream_ant.hip): one frame's logits
// from the four K-quarter partials, then softmax / argmax.  One copy, so that the two heads cannot drift apart.
#pragma once
#include "common.h"

// sl[c] = logit of class c: the partials of the four waves (redh[q][class tile][g][e], class c = tile c / 16, row c % 16 = 4 g + e) added
// in K order, plus the bias.  All 256 threads call; a __syncthreads() before (redh complete) and after (sl complete) is the caller's.
template <int NT>
__device__ __forceinline__ void stream_head_logits(const f32x4 (&redh)[4][NT][4], float* sl, int tid, int C, float bc_t) {
  if (tid < C) {
    const int ct = tid >> 4, r = tid & 15, gg = r >> 2, e = r & 3;
    sl[tid] = ((redh[0][ct][gg][e] + redh[1][ct][gg][e]) + (redh[2][ct][gg][e] + redh[3][ct][gg][e])) + bc_t;
  }
}

// One wave: eval softmax (or the logits) of sl[0 .. C) to out_row and np.argmax (first max wins) to *argmax_row; each nullable.  C <= 128.
__device__ __forceinline__ void stream_head_finish(const float* sl, int lane, int C, int softmax, float* __restrict__ out_row,
                                                   int* __restrict__ argmax_row) {
  // C <= 128: two classes per lane
  const float v0 = lane < C ? sl[lane] : -INFINITY, v1 = lane + 64 < C ? sl[lane + 64] : -INFINITY;
  const float mx = wave_max(fmaxf(v0, v1));
  // first index holding the maximum (np.argmax)
  int cand = v0 == mx ? lane : (v1 == mx ? lane + 64 : 0x7fffffff);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(cand, o, 64); cand = other < cand ? other : cand; }
  if (argmax_row != nullptr && lane == 0) *argmax_row = cand;
  if (out_row != nullptr) {
    if (softmax) {
      const float e0 = lane < C ? __expf(v0 - mx) : 0.f, e1 = lane + 64 < C ? __expf(v1 - mx) : 0.f;
      const float inv = 1.0f / wave_sum(e0 + e1);
      if (lane < C) out_row[lane] = e0 * inv;
      if (lane + 64 < C) out_row[lane + 64] = e1 * inv;
    } else {
      if (lane < C) out_row[lane] = v0;
      if (lane + 64 < C) out_row[lane + 64] = v1;
    }
  }
}
