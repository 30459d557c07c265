// Multi-frame streaming step (prego_miniroad_step_frames / _anticipation; host side: stream_frames.cpp): K <= 32 new frames for each of n
// streams, n K <= 256, in one call.  Everything that does not depend on time runs once over the n K rows (row s K + t = frame t of stream
// s) with the wide step's launchers (stream_wide.hip); only W_hh sits on the sequential path, and it gets one launch per frame:
//   frames_cast    [rgb | flow] rows -> 16-bit (cast_features) and a copy of h_state, so that the last frame may overwrite h_state
//   frames_recur   frame t of every stream: gh = op16(h_{t-1}) W_hh^T, the GRU gates, h_t into the fp32 history [n K][H] and relu(h_t) in the
//                  operand type into the head's row list; the last frame also into the caller's h_state
//   frames_recur_ragged  the same body with a second row map (prego_miniroad_step_ragged): a frame count per stream, packed rows, launch t
//                  walks only the streams that have a frame t
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
  float* h_state;              // [n][H]; step_frames: non-null on the last frame only
  int t;
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

// Which stream and which row a walk position stands for.  A map has: walk() = positions the launch walks (tiles of 16), fetch(tile, l15) =
// what position 16 tile + l15 needs from memory (requested with the tile's other loads), stream(i, e) = its row of h0 / h_state, row(i, e, t) = its row of
// gi / hist / hr in frame t, last(e, t) = frame t is the stream's last (the state also goes to h_state).
// step_frames: position = stream, row s K + t, every stream ends in the call's last launch (the host passes h_state there only)
struct UniformRows {
  int n, K;
  struct Entry {};
  __device__ __forceinline__ int walk() const { return n; }
  __device__ __forceinline__ Entry fetch(int, int) const { return Entry{}; }
  __device__ __forceinline__ int stream(int i, Entry) const { return i; }
  __device__ __forceinline__ size_t row(int i, Entry, int t) const { return (size_t)i * K + t; }
  __device__ __forceinline__ bool last(Entry, int) const { return true; }
};
// step_ragged: the streams in descending order of their frame count, so that the n_t streams alive in frame t are the positions
// [0, n_t); the caller's order - rows off[s] .., h_state row s - comes back through the table (RaggedMap, kernels.h)
struct RaggedRows {
  const RaggedMap* tab;        // the kernel's own argument
  int n_t;
  using Entry = unsigned;
  __device__ __forceinline__ int walk() const { return n_t; }
  // the 16 entries of a tile sit at a wave-uniform address: scalar loads, issued with the kernel's other arguments for the first tile
  // (a per-lane load would put one more memory round trip in front of the state loads), then each lane keeps its own
  __device__ __forceinline__ Entry fetch(int tl, int l15) const {
    Entry e = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const Entry v = tab->e[16 * tl + k];
      e = l15 == k ? v : e;
    }
    return e;
  }
  __device__ __forceinline__ int stream(int, Entry e) const { return (int)ragged_stream(e); }
  __device__ __forceinline__ size_t row(int, Entry e, int t) const { return (size_t)(ragged_off(e) + (unsigned)t); }
  __device__ __forceinline__ bool last(Entry e, int t) const { return (int)ragged_count(e) == t + 1; }
};

// Lane (l15, g) of wave q holds the fragments of W_hh row gate(l15) H + j0 + unit(l15) (gate = l15 / 4, unit = l15 % 4; rows 12..15 of the
// tile are zero) and of walk position 16 tile + l15's previous state, converted in registers (pack16_sat).  Accumulator element e of lane
// (column l15 = position, g) is gate g of unit j0 + e, so the 16 lanes with g == 0 of wave 0 find r, z and n of their stream's four units
// in lanes l15, 16 + l15 and 32 + l15 of the reduction tile.
// NT: W_hh requested non-temporally (one frame per call: read once, as wide_gemv does); otherwise it stays in the L2 for the next frame.
template <typename OT, bool NT, typename Map>
__device__ __forceinline__ void frames_recur_body(const RecurArgs& a, const Map& m) {
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
  struct Frag { f32x4 x[4][4]; f32x4 ir, iz, in_, hp; typename Map::Entry e; };
  // the previous state of a stream: the copy of h_state for the first frame of the burst, the history row of frame t - 1 after it
  auto load_x = [&](int tl, Frag& f) {
    const int i = 16 * tl + l15;
    const bool live = i < m.walk();
    f.e = m.fetch(tl, l15);
    const float* hprev = a.t == 0 ? a.h0 + (size_t)(live ? m.stream(i, f.e) : 0) * kStreamH
                                  : a.hist + ((live ? m.row(i, f.e, a.t) : (size_t)a.t) - 1) * kStreamH;
    load_h_pairs(hprev + quarter_col(L, 256), live, f.x);
    f.ir = f.iz = f.in_ = f.hp = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (gate_lane && live) {
      const float* gis = a.gi + m.row(i, f.e, a.t) * 3 * kStreamH + j0;
      f.ir = *(const f32x4*)gis; f.iz = *(const f32x4*)(gis + kStreamH); f.in_ = *(const f32x4*)(gis + 2 * kStreamH);
      f.hp = *(const f32x4*)(hprev + j0);
    }
  };
  auto tile = [&](int tl, const Frag& f) {
    const f32x4 acc = mfma_pairs<OT, 4>(wa, 4, [&](int pr, u32x4& x0, u32x4& x1) { pack16_sat<OT>(f.x[pr][0], f.x[pr][1], f.x[pr][2], f.x[pr][3], x0, x1); });
    const auto& rd = meet_quarters(red, tl, L, acc);
    const int i = 16 * tl + l15;
    if (gate_lane && i < m.walk()) {
      f32x4 hr = join_quarters(rd, l15), hz = join_quarters(rd, 16 + l15), hn = join_quarters(rd, 32 + l15);
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      hr += zero4; hz += zero4; hn += zero4;                 // +0: normalises -0 as the biased paths do (gh of wide_gemv has no bias and adds zeros)
      f32x4 hnew;
#pragma unroll
      for (int e = 0; e < 4; ++e) hnew[e] = gru_unit(f.ir[e], hr[e], f.iz[e], hz[e], f.in_[e], hn[e], bn[e], f.hp[e]);
      const size_t row = m.row(i, f.e, a.t);
      *(f32x4*)(a.hist + row * kStreamH + j0) = hnew;
      store_relu4<OT>(a.hr + row * kStreamH + j0, hnew);
      if (a.h_state != nullptr && m.last(f.e, a.t)) *(f32x4*)(a.h_state + (size_t)m.stream(i, f.e) * kStreamH + j0) = hnew;
    }
  };
  Frag fa, fb;
  for_stream_tiles((m.walk() + 15) >> 4, load_x, tile, fa, fb);
}

template <typename OT, bool NT>
__global__ __launch_bounds__(256, 1) void frames_recur_kernel(RecurArgs a, UniformRows m) { frames_recur_body<OT, NT>(a, m); }

// frame t of a ragged call: the n_t streams with more than t frames, the table by value in the arguments (nothing of the caller's host
// array outlives the call)
template <typename OT, bool NT>
__global__ __launch_bounds__(256, 1) void frames_recur_ragged_kernel(RecurArgs a, int n_t, RaggedMap tab) {
  frames_recur_body<OT, NT>(a, RaggedRows{&tab, n_t});
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
  const RecurArgs a{(const bf16_t*)whh, gi, b_hn, h0, hist, (bf16_t*)hr, h_state, t};
  const UniformRows m{n, K};
  const int grid = kStreamH / kU;
  for_operand(f16, [&](auto ot) {
    using OT = typename decltype(ot)::type;
    if (K == 1) frames_recur_kernel<OT, true><<<grid, 256, 0, s>>>(a, m); else frames_recur_kernel<OT, false><<<grid, 256, 0, s>>>(a, m);
  });
  return 0;
}

// frame t of a ragged call of n streams and `rows` rows in all: walk positions [0, n_t) of `walk` (descending frame counts).  Every
// entry the launch will use is checked against n and rows here, so no lane leaves the caller's buffers; -1 = nothing launched
int launch_frames_recur_ragged(const void* whh, const float* gi, const float* b_hn, const float* h0, float* hist, void* hr, float* h_state,
                               const RaggedMap& walk, int n, int rows, int n_t, int t, bool single_frame, int H, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > kRaggedMaxStreams || rows < n || rows > 256 || n_t < 1 || n_t > n || t < 0 || t >= 32 || !whh || !gi ||
      !b_hn || !h0 || !hist || !hr || !h_state) return -1;
  for (int i = 0; i < n_t; ++i) {
    const unsigned e = walk.e[i];
    if ((int)ragged_stream(e) >= n || (int)ragged_count(e) <= t || (int)(ragged_off(e) + ragged_count(e)) > rows) return -1;
  }
  const RecurArgs a{(const bf16_t*)whh, gi, b_hn, h0, hist, (bf16_t*)hr, h_state, t};
  const int grid = kStreamH / kU;
  for_operand(f16, [&](auto ot) {
    using OT = typename decltype(ot)::type;
    if (single_frame) frames_recur_ragged_kernel<OT, true><<<grid, 256, 0, s>>>(a, n_t, walk);
    else frames_recur_ragged_kernel<OT, false><<<grid, 256, 0, s>>>(a, n_t, walk);
  });
  return 0;
}
