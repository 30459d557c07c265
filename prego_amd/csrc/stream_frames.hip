// Multi-frame streaming step (prego_miniroad_step_frames / _anticipation; host side: stream_frames.cpp): K <= 32 new frames for each of n
// streams, n K <= 256, in one call.  Everything that does not depend on time runs once over the n K rows (row s K + t = frame t of stream
// s) with the wide step's launchers (stream_wide.hip); only W_hh sits on the sequential path, and it gets one launch per frame:
//   frames_cast    [rgb | flow] rows -> 16-bit (wide_cast's conversion) and a copy of h_state, so that the last frame may overwrite h_state
//   frames_recur   frame t of every stream: gh = op16(h_{t-1}) W_hh^T, the GRU gates, h_t into the fp32 history [n K][H] and relu(h_t) in the
//                  operand type into the head's row list; the last frame also into the caller's h_state
// frames_recur: a workgroup owns 4 hidden units and their r, z, n rows of W_hh - 12 rows of one 16-row MFMA tile, 256 workgroups - so gh never
// goes through memory and the gates need no second launch.  Every gh element keeps wide_gemv_kernel's order of operations (wave q the
// K-quarter, the same pair order and permuted contraction index, partials joined as (q0 + q1) + (q2 + q3), pack2_sat on the state); the
// gate expression is stream_gates_head_kernel's.  No workgroup waits for another: the order between frames is the order of the launches.
#include "common.h"
#include "kernels.h"

namespace {
constexpr int kH = 1024;          // the streaming step's hidden size
constexpr int kU = 4;             // hidden units per workgroup: 3 gates x 4 units = 12 of the 16 MFMA rows

template <typename OT>
__device__ __forceinline__ void cast_rows(const float* __restrict__ src, int n, int d, bf16_t* __restrict__ dst, int ldd) {
  const int per_row = d >> 3, total = n * per_row;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / per_row, c = (i - r * per_row) << 3;
    const f32x4 f0 = *(const f32x4*)(src + (size_t)r * d + c), f1 = *(const f32x4*)(src + (size_t)r * d + c + 4);
    const u32x4 o = {op16<OT>::pack2_sat(f0[0], f0[1]), op16<OT>::pack2_sat(f0[2], f0[3]), op16<OT>::pack2_sat(f1[0], f1[1]),
                     op16<OT>::pack2_sat(f1[2], f1[3])};
    *(u32x4*)(dst + (size_t)r * ldd + c) = o;
  }
}
__device__ __forceinline__ void zero_rows(int n, int d, bf16_t* __restrict__ dst, int ldd) {
  const int per_row = d >> 3, total = n * per_row;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / per_row, c = (i - r * per_row) << 3;
    *(u32x4*)(dst + (size_t)r * ldd + c) = (u32x4){0u, 0u, 0u, 0u};
  }
}

// one hidden unit of the GRU update: stream_gates_head_kernel's expression (gi holds b_ih, + b_hh for r and z; gh has no bias)
__device__ __forceinline__ float gru_unit(float ir, float hr, float iz, float hz, float in_, float hn_, float bn, float hp) {
  const float r = sigmoidf_(ir + hr);
  const float z = sigmoidf_(iz + hz);
  const float n = tanhf_(in_ + r * (hn_ + bn));
  return (1.0f - z) * n + z * hp;
}

struct RecurArgs {
  const bf16_t* whh;           // [3H][H] 16-bit
  const float* gi;             // [n K][3H] fp32, biases folded in
  const float* b_hn;           // [H]
  const float* h0;             // [n][H] fp32: the state before the burst
  float* hist;                 // [n K][H] fp32: the state after every frame
  bf16_t* hr;                  // [n K][H] 16-bit: relu(h_t), the classifier's operand
  float* h_state;              // [n][H], non-null on the last frame only
  int n, K, t;
};
}  // namespace

// xb [rows][d_rgb + d_flow] <- [rgb | flow], a NULL half as zeros; h0 [n][H] <- h_state (fp32, unchanged)
template <typename OT>
__global__ __launch_bounds__(256) void frames_cast_kernel(const float* __restrict__ rgb, const float* __restrict__ flow,
                                                          const float* __restrict__ hs, bf16_t* __restrict__ xb, float* __restrict__ h0,
                                                          int rows, int n, int d_rgb, int d_flow) {
  if (rgb != nullptr) cast_rows<OT>(rgb, rows, d_rgb, xb, d_rgb + d_flow);
  else zero_rows(rows, d_rgb, xb, d_rgb + d_flow);
  if (flow != nullptr) cast_rows<OT>(flow, rows, d_flow, xb + d_rgb, d_rgb + d_flow);
  else zero_rows(rows, d_flow, xb + d_rgb, d_rgb + d_flow);
  const int total = n * (kH >> 2);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) ((f32x4*)h0)[i] = ((const f32x4*)hs)[i];
}

// Lane (l15, g) of wave q holds 32 contiguous bytes per pair of k-steps of W_hh row gate(l15) H + j0 + unit(l15) (gate = l15 / 4, unit =
// l15 % 4; rows 12..15 of the tile are zero) and of stream 16 tile + l15's previous state, converted in registers as stream_gemv_kernel
// converts its fp32 input.  Accumulator element e of lane (column l15 = stream, g) is gate g of unit j0 + e, so the 16 lanes with g == 0
// of wave 0 find r, z and n of their stream's four units in lanes l15, 16 + l15 and 32 + l15 of the reduction tile.
// NT: W_hh requested non-temporally (one frame per call: read once, as wide_gemv does); otherwise it stays in the L2 for the next frame.
template <typename OT, bool NT>
__global__ __launch_bounds__(256, 1) void frames_recur_kernel(RecurArgs a) {
  __shared__ f32x4 red[2][4][64];
  const int tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int j0 = (int)blockIdx.x * kU;
  const bool wlive = l15 < 3 * kU;
  const bf16_t* wrow = a.whh + (size_t)(wlive ? (l15 >> 2) * kH + j0 + (l15 & 3) : 0) * kH + q * 256 + 16 * g;
  u32x4 wa[4][2];
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    wa[pr][0] = (u32x4){0u, 0u, 0u, 0u}; wa[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (wlive) {
      if (NT) {
        wa[pr][0] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64));
        wa[pr][1] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64 + 8));
      } else {
        wa[pr][0] = *(const u32x4*)(wrow + pr * 64);
        wa[pr][1] = *(const u32x4*)(wrow + pr * 64 + 8);
      }
    }
  }
  const bool gate_lane = q == 0 && g == 0;                   // the lanes that finish a stream's four units
  f32x4 bn = {0.f, 0.f, 0.f, 0.f};
  if (gate_lane) bn = *(const f32x4*)(a.b_hn + j0);
  const int ntiles = (a.n + 15) >> 4;
  struct Frag { f32x4 x[4][4]; f32x4 ir, iz, in_, hp; };
  // the previous state of stream s: the copy of h_state for the first frame of the burst, the history row of frame t - 1 after it
  auto load_x = [&](int tl, Frag& f) {
    const int s = 16 * tl + l15;
    const bool live = s < a.n;
    const float* hprev = a.t == 0 ? a.h0 + (size_t)(live ? s : 0) * kH : a.hist + ((size_t)(live ? s : 0) * a.K + a.t - 1) * kH;
    const float* xrow = hprev + q * 256 + 16 * g;
#pragma unroll
    for (int pr = 0; pr < 4; ++pr)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        f.x[pr][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live) f.x[pr][v] = *(const f32x4*)(xrow + pr * 64 + 4 * v);
      }
    f.ir = f.iz = f.in_ = f.hp = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (gate_lane && live) {
      const float* gis = a.gi + ((size_t)s * a.K + a.t) * 3 * kH + j0;
      f.ir = *(const f32x4*)gis; f.iz = *(const f32x4*)(gis + kH); f.in_ = *(const f32x4*)(gis + 2 * kH);
      f.hp = *(const f32x4*)(hprev + j0);
    }
  };
  auto tile = [&](int tl, const Frag& f) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      const f32x4 f0 = f.x[pr][0], f1 = f.x[pr][1], f2 = f.x[pr][2], f3 = f.x[pr][3];
      const u32x4 x0 = {op16<OT>::pack2_sat(f0[0], f0[1]), op16<OT>::pack2_sat(f0[2], f0[3]), op16<OT>::pack2_sat(f1[0], f1[1]), op16<OT>::pack2_sat(f1[2], f1[3])};
      const u32x4 x1 = {op16<OT>::pack2_sat(f2[0], f2[1]), op16<OT>::pack2_sat(f2[2], f2[3]), op16<OT>::pack2_sat(f3[0], f3[1]), op16<OT>::pack2_sat(f3[2], f3[3])};
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, wa[pr][0]), __builtin_bit_cast(bf16x8, x0), acc);
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, wa[pr][1]), __builtin_bit_cast(bf16x8, x1), acc);
    }
    f32x4 (&rd)[4][64] = red[tl & 1];
    rd[q][lane] = acc;
    __syncthreads();                                         // the other buffer is free again once every wave is past this barrier
    const int s = 16 * tl + l15;
    if (gate_lane && s < a.n) {
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};              // wide_gemv adds its (absent) bias as zeros: -0 becomes +0 there, so here too
      f32x4 hr = (rd[0][l15] + rd[1][l15]) + (rd[2][l15] + rd[3][l15]);
      f32x4 hz = (rd[0][16 + l15] + rd[1][16 + l15]) + (rd[2][16 + l15] + rd[3][16 + l15]);
      f32x4 hn = (rd[0][32 + l15] + rd[1][32 + l15]) + (rd[2][32 + l15] + rd[3][32 + l15]);
      hr += zero4; hz += zero4; hn += zero4;
      f32x4 hnew;
#pragma unroll
      for (int e = 0; e < 4; ++e) hnew[e] = gru_unit(f.ir[e], hr[e], f.iz[e], hz[e], f.in_[e], hn[e], bn[e], f.hp[e]);
      const size_t row = (size_t)s * a.K + a.t;
      *(f32x4*)(a.hist + row * kH + j0) = hnew;
      u32x2 w;
      w[0] = op16<OT>::pack2(fmaxf(hnew[0], 0.f), fmaxf(hnew[1], 0.f)); w[1] = op16<OT>::pack2(fmaxf(hnew[2], 0.f), fmaxf(hnew[3], 0.f));
      *(u32x2*)(a.hr + row * kH + j0) = w;
      if (a.h_state != nullptr) *(f32x4*)(a.h_state + (size_t)s * kH + j0) = hnew;
    }
  };
  Frag fa, fb;
  load_x(0, fa);
  for (int tl = 0; tl < ntiles; tl += 2) {
    if (tl + 1 < ntiles) load_x(tl + 1, fb);
    __builtin_amdgcn_sched_barrier(0);                       // the next tile's requests are out before this tile's first MFMA
    tile(tl, fa);
    if (tl + 1 < ntiles) {
      if (tl + 2 < ntiles) load_x(tl + 2, fa);
      __builtin_amdgcn_sched_barrier(0);
      tile(tl + 1, fb);
    }
  }
}

// xb [rows][d_rgb + d_flow] in the operand type from the fp32 frames (rows = n K); h0 [n][H] = h_state
int launch_frames_cast(const float* rgb, const float* flow, const float* h_state, void* xb, float* h0, int rows, int n, int d_rgb, int d_flow,
                       int H, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || rows < n || rows > 256 || d_rgb % 8 || d_flow % 8 || !h_state || !xb || !h0) return -1;
  const int units = (rows * (d_rgb + d_flow) + n * H) / 8;
  const int grid = (units + 255) / 256;
  if (f16) frames_cast_kernel<f16_t><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, h0, rows, n, d_rgb, d_flow);
  else frames_cast_kernel<bf16_t><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, h0, rows, n, d_rgb, d_flow);
  return 0;
}

// frame t of a burst of K for n streams (n K <= 256); h_state non-null: the new state goes there as well (the last frame)
int launch_frames_recur(const void* whh, const float* gi, const float* b_hn, const float* h0, float* hist, void* hr, float* h_state, int n,
                        int K, int t, int H, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || K < 1 || K > 32 || n * K > 256 || t < 0 || t >= K || !whh || !gi || !b_hn || !h0 || !hist || !hr) return -1;
  const RecurArgs a{(const bf16_t*)whh, gi, b_hn, h0, hist, (bf16_t*)hr, h_state, n, K, t};
  const int grid = kH / kU;
  if (K == 1) {
    if (f16) frames_recur_kernel<f16_t, true><<<grid, 256, 0, s>>>(a); else frames_recur_kernel<bf16_t, true><<<grid, 256, 0, s>>>(a);
  } else {
    if (f16) frames_recur_kernel<f16_t, false><<<grid, 256, 0, s>>>(a); else frames_recur_kernel<bf16_t, false><<<grid, 256, 0, s>>>(a);
  }
  return 0;
}
