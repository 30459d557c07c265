// Wide streaming step (prego_miniroad_step_wide / _anticipation): ONE new frame for each of n <= 256 independent streams, the weights
// crossing the memory system once per call whatever n is.  Every kernel here is built from the primitives of stream_tile.h /
// stream_head.h that the 5..16-stream step (stream_step.hip, stream_ant.hip) is built from, so every output element has that step's order
// of operations; a stream's bits depend neither on n nor on its place.
//   wide_cast          [rgb | flow] and h_state -> 16-bit rows with pack8_sat (the conversion stream_gemv does in registers)
//   wide_gemv          layer1: y = x W1^T + b1                       stream tiles of 16 walked on the MFMA N dimension,
//   ln_relu_rows       LayerNorm + ReLU (rowwise.hip), unchanged     weight fragments held in registers across the tiles,
//   wide_gemv x 2      gi = e W_ih^T + bias2, gh = h W_hh^T          the next tile's input fragments requested before this tile's MFMAs
//   stream_gates_head  stream_step.hip's kernel at grid n (one workgroup per stream; W_c, 192 KB at most, is L2-resident)
//   wide_ant_hidden    A = op16(relu(op16(relu(h_new)) W_a^T + b_a)) over the stream tiles
//   wide_ant_head      16 rows of the [n L] row list per workgroup on the 16 MFMA columns, one pull of the W_c fragments for all of them
// An MFMA column's result does not depend on the other columns, which is what makes the tiling free.  What this file adds on top of the
// shared primitives: the walk over the stream tiles (for_stream_tiles: weights requested once, two register sets of input fragments, two
// LDS tiles and so one barrier per tile) and the 16-column use of the classifier.
#include "stream_head.h"
#include "stream_launch.h"

// xb [n][d_rgb + d_flow] <- [rgb | flow]; hb [n][H] <- h_state
template <typename OT>
__global__ __launch_bounds__(256) void wide_cast_kernel(const float* __restrict__ rgb, const float* __restrict__ flow,
                                                        const float* __restrict__ hs, bf16_t* __restrict__ xb, bf16_t* __restrict__ hb,
                                                        int n, int d_rgb, int d_flow) {
  cast_features<OT>(rgb, flow, n, d_rgb, d_flow, xb);
  cast_rows<OT>(hs, n, kStreamH, hb, kStreamH);
}

// stream_gemv's product over ceil(n / 16) stream tiles, for 16-bit input rows in one piece (x_bf16, kx1 == K; no LayerNorm fusion)
template <int MAXKS, typename OT>
__global__ __launch_bounds__(256, MAXKS > 16 ? 1 : 2) void wide_gemv_kernel(GemvArgs a) {
  __shared__ f32x4 red[2][4][64];
  const int pi = (a.nprob > 1 && (int)blockIdx.x >= a.p[1].block0) ? 1 : 0;
  const GemvProb p = a.p[pi];
  const Lane L = lane_coords();
  const int j0 = ((int)blockIdx.x - p.block0) * a.rows;
  const int kq = p.K >> 2, npair = kq >> 6;                  // K % 256 == 0
  const bool wlive = L.l15 < a.rows;
  const bf16_t* wrow = p.W + (size_t)(j0 + (wlive ? L.l15 : 0)) * p.K + quarter_col(L, kq);
  constexpr int MAXP = MAXKS / 2;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && L.q == 0 && 4 * L.g < a.rows) bias4 = *(const f32x4*)(p.bias + j0 + 4 * L.g);
  u32x4 wa[MAXP][2];
  load_w_pairs<MAXP, true>(wrow, npair, wlive, wa);
  // the input fragments of stream tile t: stream 16 t + l15 on column l15 (zeros past n)
  const bf16_t* xlane = (const bf16_t*)p.X + (size_t)L.l15 * p.ldx + quarter_col(L, kq);
  auto load_x = [&](int t, u32x4 (&xr)[MAXP][2]) { load_x_pairs<MAXP>(xlane + (size_t)16 * t * p.ldx, npair, 16 * t + L.l15 < a.n, xr); };
  auto tile = [&](int t, const u32x4 (&xr)[MAXP][2]) {
    const f32x4 acc = mfma_pairs<OT, MAXP>(wa, npair, [&](int pr, u32x4& x0, u32x4& x1) { x0 = xr[pr][0]; x1 = xr[pr][1]; });
    const auto& rd = meet_quarters(red, t, L, acc);
    const int row = 16 * t + L.l15;
    if (L.q == 0 && 4 * L.g < a.rows && row < a.n) {
      // accumulator element e of lane (column l15 = stream, g): output feature j0 + 4 g + e
      f32x4 r = join_quarters(rd, L.lane);
      r += bias4;
      *(f32x4*)(p.Y + (size_t)row * p.Nout + j0 + 4 * L.g) = r;
    }
  };
  u32x4 xa[MAXP][2], xb[MAXP][2];
  for_stream_tiles((a.n + 15) >> 4, load_x, tile, xa, xb);
}

// stream_ant_hidden's product over the stream tiles: W_a fragments requested once, the fp32 state fragments double-buffered
template <typename OT>
__global__ __launch_bounds__(256, 2) void wide_ant_hidden_kernel(const bf16_t* __restrict__ wa, const float* __restrict__ ba,
                                                                 const float* __restrict__ h_state, bf16_t* __restrict__ A, int n,
                                                                 int LH, int rows) {
  __shared__ f32x4 red[2][4][64];
  const Lane L = lane_coords();
  const int j0 = (int)blockIdx.x * rows;
  const bool wlive = L.l15 < rows;
  const bf16_t* wrow = wa + (size_t)(j0 + (wlive ? L.l15 : 0)) * kStreamH + quarter_col(L, 256);
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (L.q == 0 && 4 * L.g < rows) bias4 = *(const f32x4*)(ba + j0 + 4 * L.g);
  u32x4 w[4][2];
  load_w_pairs<4, true>(wrow, 4, wlive, w);
  auto load_x = [&](int t, f32x4 (&x)[4][4]) {
    const int row = 16 * t + L.l15;
    load_h_pairs(h_state + (size_t)(row < n ? row : 0) * kStreamH + quarter_col(L, 256), row < n, x);
  };
  auto tile = [&](int t, const f32x4 (&x)[4][4]) {
    const f32x4 acc = mfma_pairs<OT, 4>(w, 4, [&](int pr, u32x4& x0, u32x4& x1) { pack16_relu<OT>(x[pr][0], x[pr][1], x[pr][2], x[pr][3], x0, x1); });
    const auto& rd = meet_quarters(red, t, L, acc);
    const int row = 16 * t + L.l15;
    if (L.q == 0 && 4 * L.g < rows && row < n) {
      f32x4 r = join_quarters(rd, L.lane);
      r += bias4;
      *(u32x2*)(A + (size_t)row * LH + j0 + 4 * L.g) = relu_cvt_sat4<OT>(r);
    }
  };
  f32x4 xa[4][4], xb[4][4];
  for_stream_tiles((n + 15) >> 4, load_x, tile, xa, xb);
}

// The classifier for 16 rows of A [nrows][H] (row s L + l of the [n L] list; every row meets the same W_c): row 16 blockIdx.x + c on column
// c of the MFMA N dimension - the columns the one-row heads leave zero.  The partials of column c go to redh[c], and stream_head_logits /
// stream_head_finish run per row as they do there (finish: wave q takes rows q, q + 4, q + 8, q + 12).
template <int NT, typename OT>
__global__ __launch_bounds__(256, 1) void wide_ant_head_kernel(const bf16_t* __restrict__ A, int nrows, const bf16_t* __restrict__ wc,
                                                               const float* __restrict__ bc, int C, int softmax,
                                                               float* __restrict__ out, int* __restrict__ argmax) {
  __shared__ f32x4 redh[16][4][NT][4];
  __shared__ float sl[16][128];
  const int b0 = blockIdx.x * 16;
  const Lane L = lane_coords();
  bf16x8 wf[NT][8];
  float bc_t;
  head_request<NT>(wc, bc, C, L, wf, bc_t);
  const bool live = b0 + L.l15 < nrows;
  u32x4 af[8];
  head_load_row(A + (size_t)(live ? b0 + L.l15 : 0) * kStreamH, live, L, af);
  head_products<NT, OT>(wf, L, [&](int ks) { return af[ks]; }, redh);
  __syncthreads();
  for (int r = 0; r < 16; ++r) stream_head_logits<NT>(redh[r], sl[r], L.tid, C, bc_t);
  __syncthreads();
  for (int r = L.q; r < 16; r += 4) {
    const int b = b0 + r;                                    // wave-uniform
    if (b < nrows)
      stream_head_finish(sl[r], L.lane, C, softmax, out != nullptr ? out + (size_t)b * C : nullptr, argmax != nullptr ? argmax + b : nullptr);
  }
}

// xb [n][d_rgb + d_flow], hb [n][H] in the operand type from the fp32 frame and state.  A NULL rgb / flow half is written as zeros.
int launch_wide_cast(const float* rgb, const float* flow, const float* h_state, void* xb, void* hb, int n, int d_rgb, int d_flow, int H,
                     hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > 256 || d_rgb % 8 || d_flow % 8) return -1;
  const int units = n * (d_rgb + d_flow + H) / 8;
  const int grid = (units + 255) / 256;
  for_operand(f16, [&](auto ot) {
    wide_cast_kernel<typename decltype(ot)::type><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, (bf16_t*)hb, n, d_rgb, d_flow);
  });
  return 0;
}

// y[n][Nout] = x[n][K] W^T + bias for one or two problems in one launch, n <= 256, x 16-bit in one piece (x_bf16, kx1 == K; no
// LayerNorm fusion).  Returns -1 on an unsupported shape.
int launch_wide_gemv(int nprob, const StreamGemv* pr, int n, hipStream_t s, bool f16) {
  if (nprob < 1 || nprob > 2 || n < 1 || n > 256) return -1;
  for (int i = 0; i < nprob; ++i)
    if (pr[i].Nout % 16 || pr[i].K % 256 || pr[i].K > 4096 || pr[i].kx1 != pr[i].K || !pr[i].x_bf16 || pr[i].ln_g) return -1;
  GemvArgs a{};
  int kmax = 0;
  const int blocks = fill_gemv_args(nprob, pr, n, a, &kmax);
  for_operand(f16, [&](auto ot) {
    using OT = typename decltype(ot)::type;
    if (kmax > 2048) wide_gemv_kernel<32, OT><<<blocks, 256, 0, s>>>(a); else wide_gemv_kernel<16, OT><<<blocks, 256, 0, s>>>(a);
  });
  return 0;
}

// A [n][L * H] (16-bit) from the fp32 state h_state [n][H].  H == 1024, n <= 256, L <= 32
int launch_wide_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > 256 || L < 1 || L > 32) return -1;
  const int LH = L * H, rows = stream_rows_per_wg(LH / 16);      // L <= 3: the halved tile
  for_operand(f16, [&](auto ot) {
    wide_ant_hidden_kernel<typename decltype(ot)::type><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  });
  return 0;
}

// ant_out [n][L][C] / ant_argmax [n][L] (each nullable) from A [n][L * H]; wc holds ceil(C / 16) * 16 rows
int launch_wide_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                         int* ant_argmax, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > 256 || L < 1 || L > 32 || C < 1 || C > 128) return -1;
  const int nrows = n * L, grid = (nrows + 15) / 16;
  for_class_tiles(C, f16, [&](auto nt, auto ot) {
    wide_ant_head_kernel<decltype(nt)::value, typename decltype(ot)::type><<<grid, 256, 0, s>>>((const bf16_t*)A, nrows, (const bf16_t*)wc, bc, C,
                                                                                                  softmax, ant_out, ant_argmax);
  });
  return 0;
}
