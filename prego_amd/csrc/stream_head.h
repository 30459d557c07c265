// The classifier of the streaming heads (stream_gates_head of stream_step.hip, stream_ant_head of stream_ant.hip, wide_ant_head of
// stream_wide.hip): logits^T = W_c x^T on the MFMA with wave q the K-quarter of every class tile, the four partials joined in K order,
// bias, then softmax / argmax.  One copy: the heads differ only in where their operand rows come from.
#pragma once
#include "stream_tile.h"

// every W_c fragment of the wave (NT class tiles x 8 k-steps) and the thread's bias, requested at once: a late load is one more ~2 us
// round trip.  wc holds NT * 16 rows of kStreamH
template <int NT>
__device__ __forceinline__ void head_request(const bf16_t* __restrict__ wc, const float* __restrict__ bc, int C, const Lane& c,
                                             bf16x8 (&wf)[NT][8], float& bc_t) {
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) wf[ct][ks] = *(const bf16x8*)(wc + (size_t)(ct * 16 + c.l15) * kStreamH + c.q * 256 + ks * 32 + 8 * c.g);
  bc_t = c.tid < C ? bc[c.tid] : 0.f;
}
// the wave's partial logits of NCOL operand rows (1: the row on MFMA column 0, the other columns zero; 16: one row per column) into
// redh[column].  xfrag(ks): the lane's operand fragment of k-step ks, elements q * 256 + ks * 32 + 8 g .. + 7 of its column's row
template <int NT, typename OT, int NCOL, typename XF>
__device__ __forceinline__ void head_products(const bf16x8 (&wf)[NT][8], const Lane& c, XF&& xfrag, f32x4 (&redh)[NCOL][4][NT][4]) {
  f32x4 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const u32x4 x = xfrag(ks);
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = op16<OT>::mfma(wf[ct][ks], __builtin_bit_cast(bf16x8, x), acc[ct]);
  }
  if (NCOL == 16 || c.l15 == 0) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) redh[c.l15][c.q][ct][c.g] = acc[ct];
  }
}
// a row's 8 operand fragments from memory, requested at once (zeros for lanes that are not live); row points at the row's first element
__device__ __forceinline__ void head_load_row(const bf16_t* row, bool live, const Lane& c, u32x4 (&af)[8]) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    af[ks] = (u32x4){0u, 0u, 0u, 0u};
    if (live) af[ks] = *(const u32x4*)(row + c.q * 256 + 8 * c.g + ks * 32);
  }
}

// sl[c] = logit of class c: the partials of the four waves (redh[q][class tile][g][e], class c = tile c / 16, row c % 16 = 4 g + e) added
// in K order, plus the bias.  All 256 threads call; a __syncthreads() before (redh complete) and after (sl complete) is the caller's.
template <int NT>
__device__ __forceinline__ void stream_head_logits(const f32x4 (&redh)[4][NT][4], float* sl, int tid, int C, float bc_t) {
  if (tid < C) {
    const int ct = tid >> 4, r = tid & 15, gg = r >> 2, e = r & 3;
    sl[tid] = join_quarters(redh[0][ct][gg][e], redh[1][ct][gg][e], redh[2][ct][gg][e], redh[3][ct][gg][e]) + bc_t;
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
