// Streaming inference: ONE new frame for each of n <= 16 independent streams, the GRU state carried by
// the caller - MROAD.forward (model/rnn/rnn.py:51-71) with T = 1 and h0 = the state the previous call left.  The reference never
// exposes this (its eval loop runs whole videos), but it is how an online detector is driven.
//
// With one row per stream every layer is a skinny product that reads its whole weight matrix once (36 MB of bf16 per frame):
// HBM-latency bound, so the design goal is "everything in flight at once, as few launches as possible" - not the batched
// path's tiling.  Three (<= 4 streams: LayerNorm inside the second product) or four launches per frame instead of the batched path's seven plus its plan / table staging:
//   stream_gemv        layer1: y = [rgb | flow] W1^T + b1            (fp32 features converted in registers, no pack kernel)
//   ln_relu_rows       LayerNorm + ReLU (the batched path's kernel, rowwise.hip)
//   stream_gemv x 2    gi = e W_ih^T + b_ih (+ b_hh for r, z)  and  gh = h W_hh^T   in ONE launch (two problem descriptors)
//   stream_gates_head  GRU gates + state update, ReLU, classifier, softmax, argmax: one workgroup per stream
// The product itself - who owns which rows, the K-quarters, the permuted contraction index, the K-order join - is stream_tile.h's, the
// classifier stream_head.h's.  This file adds: stream_gemv's input side (two fp32 or 16-bit halves converted in registers, or the
// LayerNorm fusion), with every request of the kernel out before the first MFMA, and the GRU gates in front of the classifier.
#include "stream_head.h"
#include "stream_launch.h"

#define SG_MAXKS 32            // k-steps of 32 per wave: K <= 4096

// MAXKS: k-steps of 32 a wave may hold (32: K <= 4096, one workgroup per CU; 16: K <= 2048, 192 registers, two per CU).
// a.rows: output features per workgroup, 8 or 16 (stream_rows_per_wg).  Lanes whose stream index is >= n load nothing.
// LNX: problems whose ln_g is set take their input through LayerNorm + ReLU (rnn.py:41-42) inside the kernel: the workgroup loads
// the <= 4 pre-LayerNorm rows (requests issued BEFORE the weight requests, so that waiting for them leaves the weights in
// flight), computes the two-pass statistics with two block reductions, and reads its input fragments from the normalised bf16
// rows in LDS.  384 workgroups repeat the same 8 KB row: cheaper than the extra launch of a LayerNorm kernel (5.9 us).
template <int MAXKS, bool LNX, typename OT = bf16_t>
__global__ __launch_bounds__(256, MAXKS > 16 ? 1 : 2) void stream_gemv_kernel(GemvArgs a) {
  __shared__ f32x4 red[1][4][64];
  __shared__ __attribute__((aligned(16))) bf16_t xs[LNX ? 4 : 1][LNX ? MAXKS * 128 : 8];
  __shared__ float sred[2][4][4];
  const int pi = (a.nprob > 1 && (int)blockIdx.x >= a.p[1].block0) ? 1 : 0;
  const GemvProb p = a.p[pi];
  const Lane L = lane_coords();
  const int tid = L.tid, lane = L.lane, q = L.q, l15 = L.l15, g = L.g;
  const int j0 = ((int)blockIdx.x - p.block0) * a.rows;
  const int kq = p.K >> 2, npair = kq >> 6;                  // K % 256 == 0
  const bool live = l15 < a.n, wlive = l15 < a.rows;
  const bf16_t* wrow = p.W + (size_t)(j0 + (wlive ? l15 : 0)) * p.K + quarter_col(L, kq);
  constexpr int MAXP = MAXKS / 2;
  // every global request of the kernel goes out up front: a dependent round trip to memory costs ~2 us here, the arithmetic nothing
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && q == 0 && 4 * g < a.rows) bias4 = *(const f32x4*)(p.bias + j0 + 4 * g);
  const bool ln = LNX && p.ln_g != nullptr;                  // workgroup-uniform
  constexpr int EPL = MAXKS / 2;                             // elements of a row per thread at the largest K (K / 256)
  float yv[LNX ? 4 : 1][LNX ? EPL : 1], gv[LNX ? EPL : 1], bv[LNX ? EPL : 1];
  const int epl = p.K >> 8;                                  // K % 2048 == 0 in this mode: 8 or 16 elements per thread
  if constexpr (LNX) {
    if (ln) {
#pragma unroll
      for (int c = 0; c < EPL; c += 4)
        if (c < epl) {
          const f32x4 g4 = *(const f32x4*)(p.ln_g + tid * epl + c), b4 = *(const f32x4*)(p.ln_b + tid * epl + c);
#pragma unroll
          for (int k = 0; k < 4; ++k) { gv[c + k] = g4[k]; bv[c + k] = b4[k]; }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 y4 = r < a.n ? *(const f32x4*)((const float*)p.X + (size_t)r * p.ldx + tid * epl + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) yv[r][c + k] = y4[k];
          }
        }
    }
  }

  u32x4 wa[MAXP][2];
  u32x4 xr[MAXP][4];
  load_w_pairs<MAXP, true>(wrow, npair, wlive, wa);
  if constexpr (LNX) {
    if (ln) {
      const float invK = 1.0f / (float)p.K;
      float mu[4], rstd[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) if (r < a.n) {
        float sacc = 0.f;
#pragma unroll
        for (int c = 0; c < EPL; ++c) if (c < epl) sacc += yv[r][c];
        sacc = wave_sum(sacc);
        if (lane == 0) sred[0][q][r] = sacc;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) if (r < a.n) {
        mu[r] = join_quarters(sred[0][0][r], sred[0][1][r], sred[0][2][r], sred[0][3][r]) * invK;
        float qacc = 0.f;
#pragma unroll
        for (int c = 0; c < EPL; ++c) if (c < epl) { const float d = yv[r][c] - mu[r]; qacc += d * d; }
        qacc = wave_sum(qacc);
        if (lane == 0) sred[1][q][r] = qacc;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) if (r < a.n) {
        rstd[r] = 1.0f / sqrtf(join_quarters(sred[1][0][r], sred[1][1][r], sred[1][2][r], sred[1][3][r]) * invK + p.ln_eps);
#pragma unroll
        for (int c = 0; c < EPL; c += 2)
          if (c < epl) {
            const float o0 = fmaxf((yv[r][c] - mu[r]) * rstd[r] * gv[c] + bv[c], 0.f);
            const float o1 = fmaxf((yv[r][c + 1] - mu[r]) * rstd[r] * gv[c + 1] + bv[c + 1], 0.f);
            *(unsigned*)(&xs[r][tid * epl + c]) = op16<OT>::pack2_sat(o0, o1);
          }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int pr = 0; pr < MAXP; ++pr) {
#pragma unroll
    for (int v = 0; v < 4; ++v) xr[pr][v] = (u32x4){0u, 0u, 0u, 0u};
    if (LNX && ln) {
      if (pr < npair && live) {                              // n <= 4 rows: live lanes are l15 < n
        const bf16_t* src = &xs[l15][quarter_col(L, kq) + pr * 64];
        xr[pr][0] = *(const u32x4*)src; xr[pr][1] = *(const u32x4*)(src + 8);
      }
    } else if (pr < npair) {
      const int kb = q * kq + pr * 64;                       // wave-uniform: a pair lies in ONE input half (kx1 % 64 == 0)
      const bool first = kb < p.kx1;
      const void* base = first ? p.X : p.X2;
      const int ld = first ? p.ldx : p.ldx2;
      const size_t off = (size_t)l15 * ld + (first ? kb : kb - p.kx1) + 16 * g;
      if (base != nullptr && live) {
        if (p.x_bf16) {
          xr[pr][0] = *(const u32x4*)((const bf16_t*)base + off); xr[pr][1] = *(const u32x4*)((const bf16_t*)base + off + 8);
        } else {
#pragma unroll
          for (int v = 0; v < 4; ++v) xr[pr][v] = *(const u32x4*)((const float*)base + off + 4 * v);
        }
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);                         // every request is out before the first use
  const f32x4 acc = mfma_pairs<OT, MAXP>(wa, npair, [&](int pr, u32x4& x0, u32x4& x1) {
    x0 = xr[pr][0]; x1 = xr[pr][1];
    if (!p.x_bf16 && !(LNX && ln))
      pack16_sat<OT>(__builtin_bit_cast(f32x4, xr[pr][0]), __builtin_bit_cast(f32x4, xr[pr][1]), __builtin_bit_cast(f32x4, xr[pr][2]),
                     __builtin_bit_cast(f32x4, xr[pr][3]), x0, x1);
  });
  const auto& rd = meet_quarters(red, 0, L, acc);
  if (q == 0 && 4 * g < a.rows) {
    // accumulator element e of lane (column l15 = stream, g): output feature j0 + 4 g + e
    f32x4 r = join_quarters(rd, lane);
    r += bias4;
    if (live) *(f32x4*)(p.Y + (size_t)l15 * p.Nout + j0 + 4 * g) = r;
  }
}

// GRU gates + state update (rnn.py:61, gru_unit), ReLU + classifier (rnn.py:62-64), eval softmax (rnn.py:66-70), np.argmax (eval.py:53,
// first max wins).  gi already holds b_ih (+ b_hh for the r, z rows), gh = h W_hh^T without bias.  One workgroup per stream; the
// classifier's operand row is relu(h_t) in LDS, on MFMA column 0.
template <int NT, typename OT = bf16_t>
__global__ __launch_bounds__(256, 1) void stream_gates_head_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                                   const float* __restrict__ b_hn, float* __restrict__ h_state,
                                                                   const bf16_t* __restrict__ wc, const float* __restrict__ bc, int C,
                                                                   int softmax, float* __restrict__ out, int* __restrict__ argmax) {
  constexpr int H = kStreamH;
  __shared__ __attribute__((aligned(16))) bf16_t shb[H];      // relu(h_t) as the bf16 the head multiplies
  __shared__ f32x4 redh[1][4][NT][4];
  __shared__ float sl[128];
  const int s = blockIdx.x;
  const Lane L = lane_coords();
  // classifier weights first: they do not depend on the gates (requests in flight under the gate math)
  bf16x8 wa[NT][8];
  float bc_t;
  head_request<NT>(wc, bc, C, L, wa, bc_t);
  const float* gis = gi + (size_t)s * 3 * H;
  const float* ghs = gh + (size_t)s * 3 * H;
  {
    const int u = L.tid * 4;                                  // four consecutive hidden units per thread
    const f32x4 ir = *(const f32x4*)(gis + u), iz = *(const f32x4*)(gis + H + u), in_ = *(const f32x4*)(gis + 2 * H + u);
    const f32x4 hr = *(const f32x4*)(ghs + u), hz = *(const f32x4*)(ghs + H + u), hn_ = *(const f32x4*)(ghs + 2 * H + u);
    const f32x4 bn = *(const f32x4*)(b_hn + u), hp = *(const f32x4*)(h_state + (size_t)s * H + u);
    f32x4 hnew;
#pragma unroll
    for (int e = 0; e < 4; ++e) hnew[e] = gru_unit(ir[e], hr[e], iz[e], hz[e], in_[e], hn_[e], bn[e], hp[e]);
    *(f32x4*)(h_state + (size_t)s * H + u) = hnew;
    store_relu4<OT>(shb + u, hnew);
  }
  __syncthreads();
  head_products<NT, OT>(wa, L, [&](int ks) {
    u32x4 hb = *(const u32x4*)(shb + L.q * 256 + ks * 32 + 8 * L.g);
    if (L.l15 != 0) hb = (u32x4){0u, 0u, 0u, 0u};            // the frame is column 0 of the N dimension
    return hb;
  }, redh);
  __syncthreads();
  stream_head_logits<NT>(redh[0], sl, L.tid, C, bc_t);
  __syncthreads();
  if (L.q == 0)
    stream_head_finish(sl, L.lane, C, softmax, out != nullptr ? out + (size_t)s * C : nullptr, argmax != nullptr ? argmax + s : nullptr);
}

// y[n][Nout] = x[n][K] W^T + bias for one or two problems in one launch.  Returns -1 on an unsupported shape.
int launch_stream_gemv(int nprob, const StreamGemv* pr, int n, hipStream_t s, bool f16) {
  if (nprob < 1 || nprob > 2 || n < 1 || n > 16) return -1;
  bool any_ln = false;
  for (int i = 0; i < nprob; ++i) {
    if (pr[i].Nout % 16 || pr[i].K % 256 || pr[i].K > 128 * SG_MAXKS || pr[i].kx1 % 64 || pr[i].kx1 > pr[i].K) return -1;
    if (pr[i].ln_g != nullptr) {
      if (n > 4 || pr[i].K % 2048 || pr[i].kx1 != pr[i].K || pr[i].x_bf16 || !pr[i].ln_b) return -1;
      any_ln = true;
    }
  }
  GemvArgs a{};
  int kmax = 0;
  const int blocks = fill_gemv_args(nprob, pr, n, a, &kmax);
  for_operand(f16, [&](auto ot) {
    using OT = typename decltype(ot)::type;
    if (kmax > 2048) { if (any_ln) stream_gemv_kernel<32, true, OT><<<blocks, 256, 0, s>>>(a); else stream_gemv_kernel<32, false, OT><<<blocks, 256, 0, s>>>(a); }
    else { if (any_ln) stream_gemv_kernel<16, true, OT><<<blocks, 256, 0, s>>>(a); else stream_gemv_kernel<16, false, OT><<<blocks, 256, 0, s>>>(a); }
  });
  return 0;
}

// H == 1024 (the handle's hidden size); C <= 128, wc holds ceil(C / 16) * 16 rows
int launch_stream_gates_head(const float* gi, const float* gh, const float* b_hn, float* h_state, const void* wc, const float* bc, int n,
                             int H, int C, int softmax, float* out, int* argmax, hipStream_t s, bool f16) {
  if (H != kStreamH || C < 1 || C > 128) return -1;
  for_class_tiles(C, f16, [&](auto nt, auto ot) {
    stream_gates_head_kernel<decltype(nt)::value, typename decltype(ot)::type><<<n, 256, 0, s>>>(gi, gh, b_hn, h_state, (const bf16_t*)wc, bc, C,
                                                                                                   softmax, out, argmax);
  });
  return 0;
}
