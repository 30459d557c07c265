// Multi-frame streaming step (prego_miniroad_step_frames / _anticipation; host side: stream_frames.cpp): K <= 32 new frames for each of n
// streams, n K <= 256, in one call.  Everything that does not depend on time runs once over the n K rows (row s K + t = frame t of stream
// s) with the wide step's launchers (stream_wide.hip); only W_hh sits on the sequential path, and it gets one launch per frame:
//   frames_cast    [rgb | flow] rows -> 16-bit (cast_features) and a copy of h_state, so that the last frame may overwrite h_state
//   frames_recur   frame t of every stream: gh = op16(h_{t-1}) W_hh^T, the GRU gates, h_t into the fp32 history [n K][H] and relu(h_t) in the
//                  operand type into the head's row list; the last frame also into the caller's h_state
// What this file adds on top of stream_tile.h is frames_recur's row ownership: a workgroup owns 4 hidden units and their r, z, n rows of
// W_hh - 12 rows of one 16-row MFMA tile, 256 workgroups - so gh never goes through memory and the gates (gru_unit) need no second
// launch.  The product, the tile walk and the conversions are the shared ones.  No workgroup waits for another: the order between frames
// is the order of the launches.
#include "stream_launch.h"

namespace {
constexpr int kU = 4;             // hidden units per workgroup: 3 gates x 4 units = 12 of the 16 MFMA rows

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

// xb [rows][d_rgb + d_flow] <- [rgb | flow]; h0 [n][H] <- h_state (fp32, unchanged)
template <typename OT>
__global__ __launch_bounds__(256) void frames_cast_kernel(const float* __restrict__ rgb, const float* __restrict__ flow,
                                                          const float* __restrict__ hs, bf16_t* __restrict__ xb, float* __restrict__ h0,
                                                          int rows, int n, int d_rgb, int d_flow) {
  cast_features<OT>(rgb, flow, rows, d_rgb, d_flow, xb);
  const int total = n * (kStreamH >> 2);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) ((f32x4*)h0)[i] = ((const f32x4*)hs)[i];
}

// Lane (l15, g) of wave q holds the fragments of W_hh row gate(l15) H + j0 + unit(l15) (gate = l15 / 4, unit = l15 % 4; rows 12..15 of the
// tile are zero) and of stream 16 tile + l15's previous state, converted in registers (pack16_sat).  Accumulator element e of lane
// (column l15 = stream, g) is gate g of unit j0 + e, so the 16 lanes with g == 0 of wave 0 find r, z and n of their stream's four units
// in lanes l15, 16 + l15 and 32 + l15 of the reduction tile.
// NT: W_hh requested non-temporally (one frame per call: read once, as wide_gemv does); otherwise it stays in the L2 for the next frame.
template <typename OT, bool NT>
__global__ __launch_bounds__(256, 1) void frames_recur_kernel(RecurArgs a) {
  __shared__ f32x4 red[2][4][64];
  const Lane L = lane_coords();
  const int l15 = L.l15;
  const int j0 = (int)blockIdx.x * kU;
  const bool wlive = l15 < 3 * kU;
  const bf16_t* wrow = a.whh + (size_t)(wlive ? (l15 >> 2) * kStreamH + j0 + (l15 & 3) : 0) * kStreamH + quarter_col(L, 256);
  u32x4 wa[4][2];
  load_w_pairs<4, NT>(wrow, 4, wlive, wa);
  const bool gate_lane = L.q == 0 && L.g == 0;               // the lanes that finish a stream's four units
  f32x4 bn = {0.f, 0.f, 0.f, 0.f};
  if (gate_lane) bn = *(const f32x4*)(a.b_hn + j0);
  struct Frag { f32x4 x[4][4]; f32x4 ir, iz, in_, hp; };
  // the previous state of stream s: the copy of h_state for the first frame of the burst, the history row of frame t - 1 after it
  auto load_x = [&](int tl, Frag& f) {
    const int s = 16 * tl + l15;
    const bool live = s < a.n;
    const float* hprev = a.t == 0 ? a.h0 + (size_t)(live ? s : 0) * kStreamH : a.hist + ((size_t)(live ? s : 0) * a.K + a.t - 1) * kStreamH;
    load_h_pairs(hprev + quarter_col(L, 256), live, f.x);
    f.ir = f.iz = f.in_ = f.hp = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (gate_lane && live) {
      const float* gis = a.gi + ((size_t)s * a.K + a.t) * 3 * kStreamH + j0;
      f.ir = *(const f32x4*)gis; f.iz = *(const f32x4*)(gis + kStreamH); f.in_ = *(const f32x4*)(gis + 2 * kStreamH);
      f.hp = *(const f32x4*)(hprev + j0);
    }
  };
  auto tile = [&](int tl, const Frag& f) {
    const f32x4 acc = mfma_pairs<OT, 4>(wa, 4, [&](int pr, u32x4& x0, u32x4& x1) { pack16_sat<OT>(f.x[pr][0], f.x[pr][1], f.x[pr][2], f.x[pr][3], x0, x1); });
    const auto& rd = meet_quarters(red, tl, L, acc);
    const int s = 16 * tl + l15;
    if (gate_lane && s < a.n) {
      f32x4 hr = join_quarters(rd, l15), hz = join_quarters(rd, 16 + l15), hn = join_quarters(rd, 32 + l15);
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      hr += zero4; hz += zero4; hn += zero4;                 // +0: normalises -0 as the biased paths do (gh of wide_gemv has no bias and adds zeros)
      f32x4 hnew;
#pragma unroll
      for (int e = 0; e < 4; ++e) hnew[e] = gru_unit(f.ir[e], hr[e], f.iz[e], hz[e], f.in_[e], hn[e], bn[e], f.hp[e]);
      const size_t row = (size_t)s * a.K + a.t;
      *(f32x4*)(a.hist + row * kStreamH + j0) = hnew;
      store_relu4<OT>(a.hr + row * kStreamH + j0, hnew);
      if (a.h_state != nullptr) *(f32x4*)(a.h_state + (size_t)s * kStreamH + j0) = hnew;
    }
  };
  Frag fa, fb;
  for_stream_tiles((a.n + 15) >> 4, load_x, tile, fa, fb);
}

// xb [rows][d_rgb + d_flow] in the operand type from the fp32 frames (rows = n K); h0 [n][H] = h_state
int launch_frames_cast(const float* rgb, const float* flow, const float* h_state, void* xb, float* h0, int rows, int n, int d_rgb, int d_flow,
                       int H, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || rows < n || rows > 256 || d_rgb % 8 || d_flow % 8 || !h_state || !xb || !h0) return -1;
  const int units = (rows * (d_rgb + d_flow) + n * H) / 8;
  const int grid = (units + 255) / 256;
  for_operand(f16, [&](auto ot) {
    frames_cast_kernel<typename decltype(ot)::type><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, h0, rows, n, d_rgb, d_flow);
  });
  return 0;
}

// frame t of a burst of K for n streams (n K <= 256); h_state non-null: the new state goes there as well (the last frame)
int launch_frames_recur(const void* whh, const float* gi, const float* b_hn, const float* h0, float* hist, void* hr, float* h_state, int n,
                        int K, int t, int H, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || K < 1 || K > 32 || n * K > 256 || t < 0 || t >= K || !whh || !gi || !b_hn || !h0 || !hist || !hr) return -1;
  const RecurArgs a{(const bf16_t*)whh, gi, b_hn, h0, hist, (bf16_t*)hr, h_state, n, K, t};
  const int grid = kStreamH / kU;
  for_operand(f16, [&](auto ot) {
    using OT = typename decltype(ot)::type;
    if (K == 1) frames_recur_kernel<OT, true><<<grid, 256, 0, s>>>(a); else frames_recur_kernel<OT, false><<<grid, 256, 0, s>>>(a);
  });
  return 0;
}
