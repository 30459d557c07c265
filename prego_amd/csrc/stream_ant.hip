// MiniROADA streaming (MROADA.forward, model/rnn/rnn.py:113-136, at T = 1 with h0 = the caller's state): the anticipation head behind the
// streaming step of stream_step.hip, for the same n <= 16 streams, on the same stream, in two launches:
//   stream_ant_hidden  A[s][l H + j] = op16(relu(sum_k op16(relu(h_new[s][k])) W_a[l H + j][k] + b_a[l H + j]))     16-bit [n][L H]
//   stream_ant_head    logits_l = A_l W_c^T + b_c, softmax, argmax (first maximum wins): one workgroup per (stream, l)
// h_new is the fp32 state stream_gates_head has just written; ReLU + rounding on load (pack16_relu) gives bit for bit the operand its
// classifier multiplied (store_relu4), so the trunk's launches run unchanged in front.  The epilogue of the first product is the batch
// head's (ant_head.hip: bias, ReLU, operand type, fp16 saturating).
// W_a is L H H operands (16.8 MB at L = 8), read once per frame: the batch head's one-workgroup-per-128-rows layout would pull all of it
// through one CU.  Here a workgroup owns 16 (or 8) output features of the product of stream_tile.h: L H / 16 workgroups (512 at L = 8), no
// atomics, repeat calls give the same bits.  On top of stream_tile.h / stream_head.h this file adds only the operands' sources: the
// fp32 state for the first product, the row A[s][l] for the classifier.
#include "stream_head.h"
#include "stream_launch.h"

// rows: output features per workgroup, 8 or 16 (stream_rows_per_wg).  Every request of the kernel goes out up front.
template <typename OT>
__global__ __launch_bounds__(256, 2) void stream_ant_hidden_kernel(const bf16_t* __restrict__ wa, const float* __restrict__ ba,
                                                                   const float* __restrict__ h_state, bf16_t* __restrict__ A, int n,
                                                                   int LH, int rows) {
  __shared__ f32x4 red[1][4][64];
  const Lane L = lane_coords();
  const int j0 = (int)blockIdx.x * rows;
  const bool live = L.l15 < n, wlive = L.l15 < rows;
  const bf16_t* wrow = wa + (size_t)(j0 + (wlive ? L.l15 : 0)) * kStreamH + quarter_col(L, 256);
  const float* xrow = h_state + (size_t)(live ? L.l15 : 0) * kStreamH + quarter_col(L, 256);
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (L.q == 0 && 4 * L.g < rows) bias4 = *(const f32x4*)(ba + j0 + 4 * L.g);
  u32x4 w[4][2];
  f32x4 x[4][4];
  load_w_pairs<4, true>(wrow, 4, wlive, w);
  load_h_pairs(xrow, live, x);
  __builtin_amdgcn_sched_barrier(0);                         // every request is out before the first use
  const f32x4 acc = mfma_pairs<OT, 4>(w, 4, [&](int pr, u32x4& x0, u32x4& x1) { pack16_relu<OT>(x[pr][0], x[pr][1], x[pr][2], x[pr][3], x0, x1); });
  const auto& rd = meet_quarters(red, 0, L, acc);
  if (L.q == 0 && 4 * L.g < rows && live) {
    // accumulator element e of lane (column l15 = stream, g): output feature j0 + 4 g + e
    f32x4 r = join_quarters(rd, L.lane);
    r += bias4;
    *(u32x2*)(A + (size_t)L.l15 * LH + j0 + 4 * L.g) = relu_cvt_sat4<OT>(r);
  }
}

// logits_l = A_l W_c^T + b_c for one (stream, l): the classifier of stream_head.h on the row A[s][l H .. l H + H), the frame in column 0
// of the MFMA N dimension, with its softmax / argmax.  The W_c fragments are requested before the A row.  blockIdx.x = s L + l is also
// the row of the outputs.
template <int NT, typename OT>
__global__ __launch_bounds__(256, 1) void stream_ant_head_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ wc,
                                                                 const float* __restrict__ bc, int C, int softmax,
                                                                 float* __restrict__ out, int* __restrict__ argmax) {
  __shared__ f32x4 redh[1][4][NT][4];
  __shared__ float sl[128];
  const int b = blockIdx.x;
  const Lane L = lane_coords();
  bf16x8 wf[NT][8];
  float bc_t;
  head_request<NT>(wc, bc, C, L, wf, bc_t);
  u32x4 af[8];
  head_load_row(A + (size_t)b * kStreamH, L.l15 == 0, L, af);      // A is [n][L][H]: row s L + l
  head_products<NT, OT>(wf, L, [&](int ks) { return af[ks]; }, redh);
  __syncthreads();
  stream_head_logits<NT>(redh[0], sl, L.tid, C, bc_t);
  __syncthreads();
  if (L.q == 0)
    stream_head_finish(sl, L.lane, C, softmax, out != nullptr ? out + (size_t)b * C : nullptr, argmax != nullptr ? argmax + b : nullptr);
}

// A [n][L * H] (16-bit) from the fp32 state h_state [n][H].  H == 1024, n <= 16, L <= 32
int launch_stream_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > 16 || L < 1 || L > 32) return -1;
  const int LH = L * H, rows = stream_rows_per_wg(LH / 16);      // L <= 3: the halved tile
  for_operand(f16, [&](auto ot) {
    stream_ant_hidden_kernel<typename decltype(ot)::type><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  });
  return 0;
}

// ant_out [n][L][C] / ant_argmax [n][L] (each nullable) from A [n][L * H]; wc holds ceil(C / 16) * 16 rows
int launch_stream_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                           int* ant_argmax, hipStream_t s, bool f16) {
  if (H != kStreamH || n < 1 || n > 16 || L < 1 || L > 32 || C < 1 || C > 128) return -1;
  for_class_tiles(C, f16, [&](auto nt, auto ot) {
    stream_ant_head_kernel<decltype(nt)::value, typename decltype(ot)::type><<<n * L, 256, 0, s>>>((const bf16_t*)A, (const bf16_t*)wc, bc, C,
                                                                                                     softmax, ant_out, ant_argmax);
  });
  return 0;
}
