// MiniROADA streaming (MROADA.forward, model/rnn/rnn.py:113-136, at T = 1 with h0 = the caller's state): the anticipation head behind the
// streaming step of stream_step.hip, for the same n <= 16 streams, on the same stream, in two launches:
//   stream_ant_hidden  A[s][l H + j] = op16(relu(sum_k op16(relu(h_new[s][k])) W_a[l H + j][k] + b_a[l H + j]))     16-bit [n][L H]
//   stream_ant_head    logits_l = A_l W_c^T + b_c, softmax, argmax (first maximum wins): one workgroup per (stream, l)
// h_new is the fp32 state stream_gates_head has just written; ReLU + rounding on load gives bit for bit the operand its classifier
// multiplied (stream_step.hip: shb), so the trunk's launches run unchanged in front.  The epilogue of the first product is the batch head's
// (ant_head.hip: bias, ReLU, operand type, fp16 saturating).
// W_a is L H H operands (16.8 MB at L = 8), read once per frame: the batch head's one-workgroup-per-128-rows layout would pull all of it
// through one CU.  Here, as in stream_gemv, a workgroup owns 16 (or 8) output features, wave q the K-quarter [256 q, 256 q + 256), every
// weight fragment of the wave is requested before the first MFMA, the streams ride on the MFMA N dimension, and the four partial tiles
// meet in LDS and are added in K order: L H / 16 workgroups (512 at L = 8), no atomics, repeat calls give the same bits.
#include "common.h"
#include "kernels.h"
#include "stream_head.h"

namespace {
constexpr int kH = 1024;          // the streaming step's hidden size
}

// rows: output features per workgroup, 8 or 16 (8 = half an MFMA M tile, when 16 would leave fewer than ~one workgroup per CU).
// A lane requests 32 contiguous bytes of its weight row per pair of k-steps and the contraction index is permuted accordingly, exactly as
// in stream_gemv_kernel; the input fragment (16 fp32 state elements per pair) is loaded with the same permutation.
template <typename OT>
__global__ __launch_bounds__(256, 2) void stream_ant_hidden_kernel(const bf16_t* __restrict__ wa, const float* __restrict__ ba,
                                                                   const float* __restrict__ h_state, bf16_t* __restrict__ A, int n,
                                                                   int LH, int rows) {
  __shared__ f32x4 red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int j0 = (int)blockIdx.x * rows;
  const bool live = l15 < n, wlive = l15 < rows;
  const bf16_t* wrow = wa + (size_t)(j0 + (wlive ? l15 : 0)) * kH + q * 256 + 16 * g;
  const float* xrow = h_state + (size_t)(live ? l15 : 0) * kH + q * 256 + 16 * g;
  // every global request of the kernel goes out up front
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (q == 0 && 4 * g < rows) bias4 = *(const f32x4*)(ba + j0 + 4 * g);
  u32x4 w[4][2];
  f32x4 x[4][4];
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    w[pr][0] = (u32x4){0u, 0u, 0u, 0u}; w[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (wlive) {                                             // read once per frame: streams past the L2
      w[pr][0] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64));
      w[pr][1] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64 + 8));
    }
  }
#pragma unroll
  for (int pr = 0; pr < 4; ++pr)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      x[pr][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (live) x[pr][v] = *(const f32x4*)(xrow + pr * 64 + 4 * v);
    }
  __builtin_amdgcn_sched_barrier(0);                         // every request is out before the first use
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    u32x4 x0, x1;
#pragma unroll
    for (int v = 0; v < 2; ++v) {                            // relu(h) in the operand type: the classifier's own operand (no saturation there either)
      x0[2 * v] = op16<OT>::pack2(fmaxf(x[pr][v][0], 0.f), fmaxf(x[pr][v][1], 0.f));
      x0[2 * v + 1] = op16<OT>::pack2(fmaxf(x[pr][v][2], 0.f), fmaxf(x[pr][v][3], 0.f));
      x1[2 * v] = op16<OT>::pack2(fmaxf(x[pr][2 + v][0], 0.f), fmaxf(x[pr][2 + v][1], 0.f));
      x1[2 * v + 1] = op16<OT>::pack2(fmaxf(x[pr][2 + v][2], 0.f), fmaxf(x[pr][2 + v][3], 0.f));
    }
    acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][0]), __builtin_bit_cast(bf16x8, x0), acc);
    acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][1]), __builtin_bit_cast(bf16x8, x1), acc);
  }
  red[q][lane] = acc;
  __syncthreads();
  if (q == 0 && 4 * g < rows && live) {
    // accumulator element e of lane (column l15 = stream, g): output feature j0 + 4 g + e
    f32x4 r = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    r += bias4;
    u32x2 o;
    o[0] = (unsigned)op16<OT>::cvt_sat(fmaxf(r[0], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[1], 0.f)) << 16);
    o[1] = (unsigned)op16<OT>::cvt_sat(fmaxf(r[2], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[3], 0.f)) << 16);
    *(u32x2*)(A + (size_t)l15 * LH + j0 + 4 * g) = o;
  }
}

// logits_l = A_l W_c^T + b_c for one (stream, l): stream_gates_head's classifier on the row A[s][l H .. l H + H) - the frame in column 0
// of the MFMA N dimension, wave q the K-quarter of every class tile, the four partials added in K order - with its softmax / argmax.
// The W_c fragments are requested before the A row.  blockIdx.x = s L + l is also the row of the outputs.
template <int NT, typename OT>
__global__ __launch_bounds__(256, 1) void stream_ant_head_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ wc,
                                                                 const float* __restrict__ bc, int C, int softmax,
                                                                 float* __restrict__ out, int* __restrict__ argmax) {
  __shared__ f32x4 redh[4][NT][4];
  __shared__ float sl[128];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  bf16x8 wf[NT][8];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) wf[ct][ks] = *(const bf16x8*)(wc + (size_t)(ct * 16 + l15) * kH + q * 256 + ks * 32 + 8 * g);
  const float bc_t = tid < C ? bc[tid] : 0.f;
  const bf16_t* arow = A + (size_t)b * kH + q * 256 + 8 * g;  // A is [n][L][H]: row s L + l
  u32x4 af[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    af[ks] = (u32x4){0u, 0u, 0u, 0u};                        // the frame is column 0 of the N dimension
    if (l15 == 0) af[ks] = *(const u32x4*)(arow + ks * 32);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = op16<OT>::mfma(wf[ct][ks], __builtin_bit_cast(bf16x8, af[ks]), acc[ct]);
  if (l15 == 0) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) redh[q][ct][g] = acc[ct];
  }
  __syncthreads();
  stream_head_logits<NT>(redh, sl, tid, C, bc_t);
  __syncthreads();
  if (q == 0)
    stream_head_finish(sl, lane, C, softmax, out != nullptr ? out + (size_t)b * C : nullptr, argmax != nullptr ? argmax + b : nullptr);
}

// A [n][L * H] (16-bit) from the fp32 state h_state [n][H].  H == 1024, n <= 16, L <= 32
int launch_stream_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || n > 16 || L < 1 || L > 32) return -1;
  const int LH = L * H;
  const int rows = LH / 16 < 200 ? 8 : 16;                   // fewer than ~one workgroup per CU at 16 rows: halve the tile (L <= 3)
  if (f16) stream_ant_hidden_kernel<f16_t><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  else stream_ant_hidden_kernel<bf16_t><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  return 0;
}

// ant_out [n][L][C] / ant_argmax [n][L] (each nullable) from A [n][L * H]; wc holds ceil(C / 16) * 16 rows
int launch_stream_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                           int* ant_argmax, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || n > 16 || L < 1 || L > 32 || C < 1 || C > 128) return -1;
#define SAH(NT)                                                                                                                              \
  do {                                                                                                                                       \
    if (f16) stream_ant_head_kernel<NT, f16_t><<<n * L, 256, 0, s>>>((const bf16_t*)A, (const bf16_t*)wc, bc, C, softmax, ant_out, ant_argmax);   \
    else stream_ant_head_kernel<NT, bf16_t><<<n * L, 256, 0, s>>>((const bf16_t*)A, (const bf16_t*)wc, bc, C, softmax, ant_out, ant_argmax);      \
  } while (0)
  switch ((C + 15) / 16) {
    case 1: SAH(1); break; case 2: SAH(2); break; case 3: SAH(3); break; case 4: SAH(4); break;
    case 5: SAH(5); break; case 6: SAH(6); break; case 7: SAH(7); break; default: SAH(8); break;
  }
#undef SAH
  return 0;
}
