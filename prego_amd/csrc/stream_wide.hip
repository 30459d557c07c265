// Wide streaming step (prego_miniroad_step_wide / _anticipation): ONE new frame for each of n <= 256 independent streams, the weights
// crossing the memory system once per call whatever n is.  Every output element keeps the order of operations of the 5..16-stream step
// (stream_step.hip, stream_ant.hip), so those kernels are the oracle bit for bit; a stream's bits depend neither on n nor on its place.
//   wide_cast          [rgb | flow] and h_state -> 16-bit rows with pack2_sat (the conversion stream_gemv does in registers)
//   wide_gemv          layer1: y = x W1^T + b1                       stream tiles of 16 walked on the MFMA N dimension,
//   ln_relu_rows       LayerNorm + ReLU (rowwise.hip), unchanged     weight fragments held in registers across the tiles,
//   wide_gemv x 2      gi = e W_ih^T + bias2, gh = h W_hh^T          the next tile's input fragments requested before this tile's MFMAs
//   stream_gates_head  stream_step.hip's kernel at grid n (one workgroup per stream; W_c, 192 KB at most, is L2-resident)
//   wide_ant_hidden    A = op16(relu(op16(relu(h_new)) W_a^T + b_a)) stream_ant_hidden's arithmetic over the stream tiles
//   wide_ant_head      16 rows of the [n L] row list per workgroup on the 16 MFMA columns, one pull of the W_c fragments for all of them
// An MFMA column's result does not depend on the other columns, which is what makes the tiling free.
#include "common.h"
#include "kernels.h"
#include "stream_head.h"

namespace {
constexpr int kH = 1024;          // the streaming step's hidden size

struct WideProb {
  const bf16_t* W;             // [Nout][K] 16-bit, row-major
  const bf16_t* X;             // [n][ldx] 16-bit input rows
  const float* bias;           // [Nout], nullable
  float* Y;                    // [n][Nout] fp32
  int Nout, K, ldx, block0;
};
struct WideArgs { WideProb p[2]; int nprob, n, rows; };

// 8 consecutive fp32 -> 8 operands, pairs packed as stream_gemv_kernel packs its fp32 input fragments
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
}  // namespace

// xb [n][d_rgb + d_flow] <- [rgb | flow], a NULL half as zeros (the zero fragments stream_gemv multiplies there); hb [n][H] <- h_state
template <typename OT>
__global__ __launch_bounds__(256) void wide_cast_kernel(const float* __restrict__ rgb, const float* __restrict__ flow,
                                                        const float* __restrict__ hs, bf16_t* __restrict__ xb, bf16_t* __restrict__ hb,
                                                        int n, int d_rgb, int d_flow) {
  if (rgb != nullptr) cast_rows<OT>(rgb, n, d_rgb, xb, d_rgb + d_flow);
  else zero_rows(n, d_rgb, xb, d_rgb + d_flow);
  if (flow != nullptr) cast_rows<OT>(flow, n, d_flow, xb + d_rgb, d_rgb + d_flow);
  else zero_rows(n, d_flow, xb + d_rgb, d_rgb + d_flow);
  cast_rows<OT>(hs, n, kH, hb, kH);
}

// stream_gemv_kernel (stream_step.hip) over ceil(n / 16) stream tiles: the same 16 (or 8) output features per workgroup, wave q the same
// K-quarter in the same pair order with the same permuted contraction index, the four partials joined as (q0 + q1) + (q2 + q3), then the
// bias.  The weight fragments are requested once and stay in registers; the input fragments (16-bit rows, x_bf16 of GemvProb) are
// double-buffered by hand (two named register sets, the tile loop unrolled by two) and so is the LDS tile the partials meet in, which
// leaves one barrier per tile.
template <int MAXKS, typename OT>
__global__ __launch_bounds__(256, MAXKS > 16 ? 1 : 2) void wide_gemv_kernel(WideArgs a) {
  __shared__ f32x4 red[2][4][64];
  const int pi = (a.nprob > 1 && (int)blockIdx.x >= a.p[1].block0) ? 1 : 0;
  const WideProb p = a.p[pi];
  const int tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int j0 = ((int)blockIdx.x - p.block0) * a.rows;
  const int kq = p.K >> 2, npair = kq >> 6;                  // K % 256 == 0
  const bool wlive = l15 < a.rows;
  const bf16_t* wrow = p.W + (size_t)(j0 + (wlive ? l15 : 0)) * p.K + q * kq + 16 * g;
  constexpr int MAXP = MAXKS / 2;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && q == 0 && 4 * g < a.rows) bias4 = *(const f32x4*)(p.bias + j0 + 4 * g);
  u32x4 wa[MAXP][2];
#pragma unroll
  for (int pr = 0; pr < MAXP; ++pr) {
    wa[pr][0] = (u32x4){0u, 0u, 0u, 0u}; wa[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (pr < npair && wlive) {                               // read once: streams past the L2
      wa[pr][0] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64));
      wa[pr][1] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64 + 8));
    }
  }
  const int ntiles = (a.n + 15) >> 4;
  // the input fragments of stream tile t: stream 16 t + l15 on column l15 (zeros past n)
  const bf16_t* xlane = p.X + (size_t)l15 * p.ldx + q * kq + 16 * g;
  auto load_x = [&](int t, u32x4 (&xr)[MAXP][2]) {
    const bf16_t* src = xlane + (size_t)16 * t * p.ldx;
    const bool live = 16 * t + l15 < a.n;
#pragma unroll
    for (int pr = 0; pr < MAXP; ++pr) {
      xr[pr][0] = (u32x4){0u, 0u, 0u, 0u}; xr[pr][1] = (u32x4){0u, 0u, 0u, 0u};
      if (pr < npair && live) { xr[pr][0] = *(const u32x4*)(src + pr * 64); xr[pr][1] = *(const u32x4*)(src + pr * 64 + 8); }
    }
  };
  auto tile = [&](int t, const u32x4 (&xr)[MAXP][2]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < MAXP; ++pr)
      if (pr < npair) {
        acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, wa[pr][0]), __builtin_bit_cast(bf16x8, xr[pr][0]), acc);
        acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, wa[pr][1]), __builtin_bit_cast(bf16x8, xr[pr][1]), acc);
      }
    f32x4 (&rd)[4][64] = red[t & 1];
    rd[q][lane] = acc;
    __syncthreads();                                         // the other buffer is free again once every wave is past this barrier
    const int row = 16 * t + l15;
    if (q == 0 && 4 * g < a.rows && row < a.n) {
      // accumulator element e of lane (column l15 = stream, g): output feature j0 + 4 g + e
      f32x4 r = (rd[0][lane] + rd[1][lane]) + (rd[2][lane] + rd[3][lane]);
      r += bias4;
      *(f32x4*)(p.Y + (size_t)row * p.Nout + j0 + 4 * g) = r;
    }
  };
  u32x4 xa[MAXP][2], xb[MAXP][2];
  load_x(0, xa);
  for (int t = 0; t < ntiles; t += 2) {
    if (t + 1 < ntiles) load_x(t + 1, xb);
    __builtin_amdgcn_sched_barrier(0);                       // the next tile's requests are out before this tile's first MFMA
    tile(t, xa);
    if (t + 1 < ntiles) {
      if (t + 2 < ntiles) load_x(t + 2, xa);
      __builtin_amdgcn_sched_barrier(0);
      tile(t + 1, xb);
    }
  }
}

// stream_ant_hidden_kernel (stream_ant.hip) over the stream tiles: W_a fragments requested once, the fp32 state fragments double-buffered
template <typename OT>
__global__ __launch_bounds__(256, 2) void wide_ant_hidden_kernel(const bf16_t* __restrict__ wa, const float* __restrict__ ba,
                                                                 const float* __restrict__ h_state, bf16_t* __restrict__ A, int n,
                                                                 int LH, int rows) {
  __shared__ f32x4 red[2][4][64];
  const int tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int j0 = (int)blockIdx.x * rows;
  const bool wlive = l15 < rows;
  const bf16_t* wrow = wa + (size_t)(j0 + (wlive ? l15 : 0)) * kH + q * 256 + 16 * g;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (q == 0 && 4 * g < rows) bias4 = *(const f32x4*)(ba + j0 + 4 * g);
  u32x4 w[4][2];
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    w[pr][0] = (u32x4){0u, 0u, 0u, 0u}; w[pr][1] = (u32x4){0u, 0u, 0u, 0u};
    if (wlive) {                                             // read once per frame: streams past the L2
      w[pr][0] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64));
      w[pr][1] = __builtin_nontemporal_load((const u32x4*)(wrow + pr * 64 + 8));
    }
  }
  const int ntiles = (n + 15) >> 4;
  auto load_x = [&](int t, f32x4 (&x)[4][4]) {
    const int row = 16 * t + l15;
    const float* xrow = h_state + (size_t)(row < n ? row : 0) * kH + q * 256 + 16 * g;
#pragma unroll
    for (int pr = 0; pr < 4; ++pr)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        x[pr][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (row < n) x[pr][v] = *(const f32x4*)(xrow + pr * 64 + 4 * v);
      }
  };
  auto tile = [&](int t, const f32x4 (&x)[4][4]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      u32x4 x0, x1;
#pragma unroll
      for (int v = 0; v < 2; ++v) {                          // relu(h) in the operand type: the classifier's own operand (no saturation there either)
        x0[2 * v] = op16<OT>::pack2(fmaxf(x[pr][v][0], 0.f), fmaxf(x[pr][v][1], 0.f));
        x0[2 * v + 1] = op16<OT>::pack2(fmaxf(x[pr][v][2], 0.f), fmaxf(x[pr][v][3], 0.f));
        x1[2 * v] = op16<OT>::pack2(fmaxf(x[pr][2 + v][0], 0.f), fmaxf(x[pr][2 + v][1], 0.f));
        x1[2 * v + 1] = op16<OT>::pack2(fmaxf(x[pr][2 + v][2], 0.f), fmaxf(x[pr][2 + v][3], 0.f));
      }
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][0]), __builtin_bit_cast(bf16x8, x0), acc);
      acc = op16<OT>::mfma(__builtin_bit_cast(bf16x8, w[pr][1]), __builtin_bit_cast(bf16x8, x1), acc);
    }
    f32x4 (&rd)[4][64] = red[t & 1];
    rd[q][lane] = acc;
    __syncthreads();
    const int row = 16 * t + l15;
    if (q == 0 && 4 * g < rows && row < n) {
      f32x4 r = (rd[0][lane] + rd[1][lane]) + (rd[2][lane] + rd[3][lane]);
      r += bias4;
      u32x2 o;
      o[0] = (unsigned)op16<OT>::cvt_sat(fmaxf(r[0], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[1], 0.f)) << 16);
      o[1] = (unsigned)op16<OT>::cvt_sat(fmaxf(r[2], 0.f)) | ((unsigned)op16<OT>::cvt_sat(fmaxf(r[3], 0.f)) << 16);
      *(u32x2*)(A + (size_t)row * LH + j0 + 4 * g) = o;
    }
  };
  f32x4 xa[4][4], xb[4][4];
  load_x(0, xa);
  for (int t = 0; t < ntiles; t += 2) {
    if (t + 1 < ntiles) load_x(t + 1, xb);
    __builtin_amdgcn_sched_barrier(0);
    tile(t, xa);
    if (t + 1 < ntiles) {
      if (t + 2 < ntiles) load_x(t + 2, xa);
      __builtin_amdgcn_sched_barrier(0);
      tile(t + 1, xb);
    }
  }
}

// stream_ant_head_kernel's classifier for 16 rows of A [nrows][H] (row s L + l of the [n L] list; every row meets the same W_c): row
// 16 blockIdx.x + c on column c of the MFMA N dimension - the columns the one-row kernel leaves zero - wave q the K-quarter of every class
// tile in the same k order.  The partials of column c go to redh[c], and stream_head_logits / stream_head_finish run per row as they do
// there (finish: wave q takes rows q, q + 4, q + 8, q + 12).
template <int NT, typename OT>
__global__ __launch_bounds__(256, 1) void wide_ant_head_kernel(const bf16_t* __restrict__ A, int nrows, const bf16_t* __restrict__ wc,
                                                               const float* __restrict__ bc, int C, int softmax,
                                                               float* __restrict__ out, int* __restrict__ argmax) {
  __shared__ f32x4 redh[16][4][NT][4];
  __shared__ float sl[16][128];
  const int b0 = blockIdx.x * 16, tid = threadIdx.x, lane = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  bf16x8 wf[NT][8];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) wf[ct][ks] = *(const bf16x8*)(wc + (size_t)(ct * 16 + l15) * kH + q * 256 + ks * 32 + 8 * g);
  const float bc_t = tid < C ? bc[tid] : 0.f;
  const bool live = b0 + l15 < nrows;
  const bf16_t* arow = A + (size_t)(live ? b0 + l15 : 0) * kH + q * 256 + 8 * g;
  u32x4 af[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    af[ks] = (u32x4){0u, 0u, 0u, 0u};
    if (live) af[ks] = *(const u32x4*)(arow + ks * 32);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = op16<OT>::mfma(wf[ct][ks], __builtin_bit_cast(bf16x8, af[ks]), acc[ct]);
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) redh[l15][q][ct][g] = acc[ct];
  __syncthreads();
  for (int r = 0; r < 16; ++r) stream_head_logits<NT>(redh[r], sl[r], tid, C, bc_t);
  __syncthreads();
  for (int r = q; r < 16; r += 4) {
    const int b = b0 + r;                                    // wave-uniform
    if (b < nrows)
      stream_head_finish(sl[r], lane, C, softmax, out != nullptr ? out + (size_t)b * C : nullptr, argmax != nullptr ? argmax + b : nullptr);
  }
}

// xb [n][d_rgb + d_flow], hb [n][H] in the operand type from the fp32 frame and state.  A NULL rgb / flow half is written as zeros.
int launch_wide_cast(const float* rgb, const float* flow, const float* h_state, void* xb, void* hb, int n, int d_rgb, int d_flow, int H,
                     hipStream_t s, bool f16) {
  if (H != kH || n < 1 || n > 256 || d_rgb % 8 || d_flow % 8) return -1;
  const int units = n * (d_rgb + d_flow + H) / 8;
  const int grid = (units + 255) / 256;
  if (f16) wide_cast_kernel<f16_t><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, (bf16_t*)hb, n, d_rgb, d_flow);
  else wide_cast_kernel<bf16_t><<<grid, 256, 0, s>>>(rgb, flow, h_state, (bf16_t*)xb, (bf16_t*)hb, n, d_rgb, d_flow);
  return 0;
}

// y[n][Nout] = x[n][K] W^T + bias for one or two problems in one launch, n <= 256, x 16-bit in one piece (x_bf16, kx1 == K; no
// LayerNorm fusion).  Returns -1 on an unsupported shape.
int launch_wide_gemv(int nprob, const StreamGemv* pr, int n, hipStream_t s, bool f16) {
  if (nprob < 1 || nprob > 2 || n < 1 || n > 256) return -1;
  WideArgs a{};
  a.nprob = nprob; a.n = n;
  int kmax = 0, tiles16 = 0;
  for (int i = 0; i < nprob; ++i) {
    if (pr[i].Nout % 16 || pr[i].K % 256 || pr[i].K > 4096 || pr[i].kx1 != pr[i].K || !pr[i].x_bf16 || pr[i].ln_g) return -1;
    kmax = pr[i].K > kmax ? pr[i].K : kmax;
    tiles16 += pr[i].Nout / 16;
  }
  a.rows = tiles16 < 200 ? 8 : 16;                           // stream_gemv's rule: fewer than ~one workgroup per CU at 16 rows: halve the tile
  int blocks = 0;
  for (int i = 0; i < nprob; ++i) {
    a.p[i] = WideProb{(const bf16_t*)pr[i].W, (const bf16_t*)pr[i].X, pr[i].bias, pr[i].Y, pr[i].Nout, pr[i].K, pr[i].ldx, blocks};
    blocks += pr[i].Nout / a.rows;
  }
  if (f16) { if (kmax > 2048) wide_gemv_kernel<32, f16_t><<<blocks, 256, 0, s>>>(a); else wide_gemv_kernel<16, f16_t><<<blocks, 256, 0, s>>>(a); }
  else { if (kmax > 2048) wide_gemv_kernel<32, bf16_t><<<blocks, 256, 0, s>>>(a); else wide_gemv_kernel<16, bf16_t><<<blocks, 256, 0, s>>>(a); }
  return 0;
}

// A [n][L * H] (16-bit) from the fp32 state h_state [n][H].  H == 1024, n <= 256, L <= 32
int launch_wide_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || n > 256 || L < 1 || L > 32) return -1;
  const int LH = L * H;
  const int rows = LH / 16 < 200 ? 8 : 16;                   // stream_ant_hidden's rule (L <= 3: halve the tile)
  if (f16) wide_ant_hidden_kernel<f16_t><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  else wide_ant_hidden_kernel<bf16_t><<<LH / rows, 256, 0, s>>>((const bf16_t*)wa, ba, h_state, (bf16_t*)A, n, LH, rows);
  return 0;
}

// ant_out [n][L][C] / ant_argmax [n][L] (each nullable) from A [n][L * H]; wc holds ceil(C / 16) * 16 rows
int launch_wide_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                         int* ant_argmax, hipStream_t s, bool f16) {
  if (H != kH || n < 1 || n > 256 || L < 1 || L > 32 || C < 1 || C > 128) return -1;
  const int nrows = n * L, grid = (nrows + 15) / 16;
#define WAH(NT)                                                                                                                               \
  do {                                                                                                                                        \
    if (f16) wide_ant_head_kernel<NT, f16_t><<<grid, 256, 0, s>>>((const bf16_t*)A, nrows, (const bf16_t*)wc, bc, C, softmax, ant_out, ant_argmax);   \
    else wide_ant_head_kernel<NT, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)A, nrows, (const bf16_t*)wc, bc, C, softmax, ant_out, ant_argmax);      \
  } while (0)
  switch ((C + 15) / 16) {
    case 1: WAH(1); break; case 2: WAH(2); break; case 3: WAH(3); break; case 4: WAH(4); break;
    case 5: WAH(5); break; case 6: WAH(6); break; case 7: WAH(7); break; default: WAH(8); break;
  }
#undef WAH
  return 0;
}
