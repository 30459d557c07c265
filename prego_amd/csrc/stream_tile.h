// The tile primitives of the streaming family (stream_step.hip, stream_ant.hip, stream_wide.hip, stream_frames.hip): the ONE place where
// the order of operations of a streaming product is defined.  Device code only.  A product here is y^T = W x^T on the 16x16x32 MFMA: 16
// (or 8) weight rows on M, up to 16 streams on N, wave q of the workgroup's four the K-quarter [q K/4, (q + 1) K/4) walked in pairs of
// k-steps, the four partial tiles joined in LDS in K order.  A lane requests 32 CONTIGUOUS bytes of its row per pair (the four lanes of a
// row cover one 128-byte line), so the contraction index is permuted - MFMA 2p takes columns 16 g .. 16 g + 7 of the pair's 64, MFMA
// 2p + 1 columns 16 g + 8 .. 16 g + 15 - and weight and input fragments are loaded with the same permutation (quarter_col).
// OT: 16-bit operand type tag (bf16_t / f16_t, common.h).  MAXP: pairs of k-steps a wave may hold (K <= 256 MAXP).
#pragma once
#include "common.h"

constexpr int kStreamH = 1024;    // the streaming step's hidden size

// lane (l15, g) of wave q: row / stream l15 of the tile, column group g of a pair; accumulator element e is tile row 4 g + e of column l15
struct Lane { int tid, lane, q, l15, g; };
__device__ __forceinline__ Lane lane_coords() {
  const int tid = threadIdx.x, lane = tid & 63;
  return Lane{tid, lane, __builtin_amdgcn_readfirstlane(tid >> 6), lane & 15, lane >> 4};
}
// first contraction column of the lane's fragments of pair 0 (pair pr: + 64 pr); kq = K / 4
__device__ __forceinline__ int quarter_col(const Lane& c, int kq) { return c.q * kq + 16 * c.g; }

// the wave's weight fragments, all requested at once (zeros past npair and for rows that are not live).  NONTEMPORAL: read once per call,
// the stream goes past the L2
template <int MAXP, bool NONTEMPORAL>
__device__ __forceinline__ void load_w_pairs(const bf16_t* wrow, int npair, bool wlive, u32x4 (&w)[MAXP][2]) {
#pragma unroll
  for (int pr = 0; pr < MAXP; ++pr) {
    w[pr][0] = (u32x4){0u, 0u, 0u, 0u}; w[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (pr < npair && wlive) {
      if (NONTEMPORAL) {
        w[pr][0] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64));
        w[pr][1] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64 + 8));
      } else {
        w[pr][0] = *(const u32x4*)(wrow + pr * 64);
        w[pr][1] = *(const u32x4*)(wrow + pr * 64 + 8);
      }
    }
  }
}
// 16-bit input fragments of one stream row (zeros past npair and for lanes that are not live)
template <int MAXP>
__device__ __forceinline__ void load_x_pairs(const bf16_t* xrow, int npair, bool live, u32x4 (&x)[MAXP][2]) {
#pragma unroll
  for (int pr = 0; pr < MAXP; ++pr) {
    x[pr][0] = (u32x4){0u, 0u, 0u, 0u}; x[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (pr < npair && live) { x[pr][0] = *(const u32x4*)(xrow + pr * 64); x[pr][1] = *(const u32x4*)(xrow + pr * 64 + 8); }
  }
}
// fp32 state fragments of one stream row of kStreamH: 16 values per pair (zeros for lanes that are not live)
__device__ __forceinline__ void load_h_pairs(const float* xrow, bool live, f32x4 (&x)[4][4]) {
#pragma unroll
  for (int pr = 0; pr < 4; ++pr)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      x[pr][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (live) x[pr][v] = *(const f32x4*)(xrow + pr * 64 + 4 * v);
    }
}

// fp32 -> operand fragments.  _sat: the input conversion (saturating for fp16); _relu: relu(h) as the classifier multiplies it (no
// saturation there either).  8 consecutive values make one fragment, 16 the two fragments of a pair.
template <typename OT>
__device__ __forceinline__ u32x4 pack8_sat(f32x4 f0, f32x4 f1) {
  return (u32x4){op16<OT>::pack2_sat(f0[0], f0[1]), op16<OT>::pack2_sat(f0[2], f0[3]), op16<OT>::pack2_sat(f1[0], f1[1]), op16<OT>::pack2_sat(f1[2], f1[3])};
}
template <typename OT>
__device__ __forceinline__ u32x2 pack4_relu(f32x4 f) {
  return (u32x2){op16<OT>::pack2(fmaxf(f[0], 0.f), fmaxf(f[1], 0.f)), op16<OT>::pack2(fmaxf(f[2], 0.f), fmaxf(f[3], 0.f))};
}
template <typename OT>
__device__ __forceinline__ void pack16_sat(f32x4 f0, f32x4 f1, f32x4 f2, f32x4 f3, u32x4& x0, u32x4& x1) {
  x0 = pack8_sat<OT>(f0, f1); x1 = pack8_sat<OT>(f2, f3);
}
template <typename OT>
__device__ __forceinline__ void pack16_relu(f32x4 f0, f32x4 f1, f32x4 f2, f32x4 f3, u32x4& x0, u32x4& x1) {
  const u32x2 a = pack4_relu<OT>(f0), b = pack4_relu<OT>(f1), c = pack4_relu<OT>(f2), d = pack4_relu<OT>(f3);
  x0 = (u32x4){a[0], a[1], b[0], b[1]}; x1 = (u32x4){c[0], c[1], d[0], d[1]};
}
// relu(h_new) of four consecutive hidden units in the operand type: the classifier's operand row
template <typename OT>
__device__ __forceinline__ void store_relu4(bf16_t* dst, f32x4 hnew) { *(u32x2*)dst = pack4_relu<OT>(hnew); }
// the anticipation product's epilogue: ReLU, operand type, fp16 saturating
template <typename OT>
__device__ __forceinline__ u32x2 relu_cvt_sat4(f32x4 r) {
  return (u32x2){(unsigned)op16<OT>::cvt_sat(fmaxf(r[0], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[1], 0.f)) << 16),
                 (unsigned)op16<OT>::cvt_sat(fmaxf(r[2], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[3], 0.f)) << 16)};
}

// the wave's partial tile: pairs in ascending order, two MFMAs per pair.  xfrag(pr, x0, x1) hands over the input fragments of pair pr
template <typename OT, int MAXP, typename XF>
__device__ __forceinline__ f32x4 mfma_pairs(const u32x4 (&w)[MAXP][2], int npair, XF&& xfrag) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pr = 0; pr < MAXP; ++pr)
    if (pr < npair) {
      u32x4 x0, x1;
      xfrag(pr, x0, x1);
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][0]), __builtin_bit_cast(bf16x8, x0), acc);
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][1]), __builtin_bit_cast(bf16x8, x1), acc);
    }
  return acc;
}

// the four K-quarter partials in K order.  A bias is added AFTER the join, as a separate step at the call site
template <typename T>
__device__ __forceinline__ T join_quarters(T q0, T q1, T q2, T q3) { return (q0 + q1) + (q2 + q3); }
template <typename T, int N>
__device__ __forceinline__ T join_quarters(const T (&rd)[4][N], int idx) { return join_quarters(rd[0][idx], rd[1][idx], rd[2][idx], rd[3][idx]); }
// the partials of the four waves meet in LDS buffer t mod NB, one barrier: with NB = 2 the other buffer is free again once every wave is
// past it, so a tile loop needs no second barrier
template <int NB>
__device__ __forceinline__ auto& meet_quarters(f32x4 (&red)[NB][4][64], int t, const Lane& c, f32x4 acc) {
  f32x4 (&rd)[4][64] = red[t & (NB - 1)];
  rd[c.q][c.lane] = acc;
  __syncthreads();
  return rd;
}

// stream tiles of 16 with two register buffers: tile t + 1 is requested, a scheduling fence keeps those requests in front of tile t's first
// MFMA, then tile t is computed.  load(t, buf) requests, tile(t, buf) computes and stores
template <typename B, typename LD, typename TL>
__device__ __forceinline__ void for_stream_tiles(int ntiles, LD&& load, TL&& tile, B& a, B& b) {
  load(0, a);
  for (int t = 0; t < ntiles; t += 2) {
    if (t + 1 < ntiles) load(t + 1, b);
    __builtin_amdgcn_sched_barrier(0);
    tile(t, a);
    if (t + 1 < ntiles) {
      if (t + 2 < ntiles) load(t + 2, a);
      __builtin_amdgcn_sched_barrier(0);
      tile(t + 1, b);
    }
  }
}

// rows [n][d] fp32 -> 16-bit rows of leading dimension ldd, 8 values per thread and trip (grid-stride); zero_rows: the same rows as zeros
template <typename OT>
__device__ __forceinline__ void cast_rows(const float* __restrict__ src, int n, int d, bf16_t* __restrict__ dst, int ldd) {
  const int per_row = d >> 3, total = n * per_row;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / per_row, c = (i - r * per_row) << 3;
    *(u32x4*)(dst + (size_t)r * ldd + c) = pack8_sat<OT>(*(const f32x4*)(src + (size_t)r * d + c), *(const f32x4*)(src + (size_t)r * d + c + 4));
  }
}
__device__ __forceinline__ void zero_rows(int n, int d, bf16_t* __restrict__ dst, int ldd) {
  const int per_row = d >> 3, total = n * per_row;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / per_row, c = (i - r * per_row) << 3;
    *(u32x4*)(dst + (size_t)r * ldd + c) = (u32x4){0u, 0u, 0u, 0u};
  }
}
// xb [rows][d_rgb + d_flow] <- [rgb | flow] in the operand type, a NULL half as zeros (the zero fragments stream_gemv multiplies there)
template <typename OT>
__device__ __forceinline__ void cast_features(const float* __restrict__ rgb, const float* __restrict__ flow, int rows, int d_rgb, int d_flow,
                                              bf16_t* __restrict__ xb) {
  if (rgb != nullptr) cast_rows<OT>(rgb, rows, d_rgb, xb, d_rgb + d_flow);
  else zero_rows(rows, d_rgb, xb, d_rgb + d_flow);
  if (flow != nullptr) cast_rows<OT>(flow, rows, d_flow, xb + d_rgb, d_rgb + d_flow);
  else zero_rows(rows, d_flow, xb + d_rgb, d_rgb + d_flow);
}

// one hidden unit of the GRU update (torch.nn.GRU's equations): gi holds b_ih (+ b_hh for r and z), gh = h W_hh^T has no bias
__device__ __forceinline__ float gru_unit(float ir, float hr, float iz, float hz, float in_, float hn_, float bn, float hp) {
  const float r = sigmoidf_(ir + hr);
  const float z = sigmoidf_(iz + hz);
  const float n = tanhf_(in_ + r * (hn_ + bn));
  return (1.0f - z) * n + z * hp;
}
