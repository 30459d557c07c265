// One token row of a ViTEnc window, shared by the two kernels that build windows from per-frame encodings: vit_sliding_tokens_kernel
// (vit.hip: the rows of one video's encoding buffer) and vit_ring_tokens_kernel (vit_stream.hip: the rows of a stream's ring).  They
// differ only in where `src` points; the arithmetic below is one piece of code, so a window has the same bits from either source.
#pragma once
#include "common.h"

// row = src + per (ViT.py:129: frame encoding, or the bias row, or the cls token, plus the positional row), one wave per row, lane
// `lane` owning the 4-column groups (i * 64 + lane) * 4, i < E / 256 <= MAXV.  Outputs, each optional (nullptr = not wanted):
//   x_row   fp32 [E]: the residual-stream row        x0_row  fp32 [E]: the same values again (token 0 of the window)
//   xn_row  16-bit [E]: LayerNorm(ln_w, ln_b) of the row in the operand type OT - two-pass statistics over the wave, sums in the order
//           (v0 + v1) + (v2 + v3) per group, pack2_sat
template <int MAXV, typename OT>
__device__ __forceinline__ void vit_token_row(const float* __restrict__ src, const float* __restrict__ per, int E, int lane,
                                              float* __restrict__ x_row, float* __restrict__ x0_row, const float* __restrict__ ln_w,
                                              const float* __restrict__ ln_b, bf16_t* __restrict__ xn_row) {
  const int nv = E / 256;                                 // 4-column groups per lane
  float v[MAXV][4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) {
      const int c = (i * 64 + lane) * 4;
      const float4 a = *(const float4*)(src + c), p = *(const float4*)(per + c);
      v[i][0] = a.x + p.x; v[i][1] = a.y + p.y; v[i][2] = a.z + p.z; v[i][3] = a.w + p.w;
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      if (x_row) *(float4*)(x_row + c) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
      if (x0_row) *(float4*)(x0_row + c) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
    }
  if (xn_row == nullptr) return;
  const float mu = wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[i][k] - mu; q += d * d; }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + 1e-5f);
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (i < nv) {
      const int c = (i * 64 + lane) * 4;
      const float4 g = *(const float4*)(ln_w + c), bb = *(const float4*)(ln_b + c);
      uint2 o;
      o.x = op16<OT>::pack2_sat((v[i][0] - mu) * rstd * g.x + bb.x, (v[i][1] - mu) * rstd * g.y + bb.y);
      o.y = op16<OT>::pack2_sat((v[i][2] - mu) * rstd * g.z + bb.z, (v[i][3] - mu) * rstd * g.w + bb.w);
      *(uint2*)(xn_row + c) = o;
    }
}
