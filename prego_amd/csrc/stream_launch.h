// Launch side of the streaming family: the product descriptor stream_gemv and wide_gemv share, the rows-per-workgroup rule, and the
// dispatch of a launch over the operand type and the number of class tiles.
#pragma once
#include "kernels.h"
#include "stream_tile.h"

#include <type_traits>

struct GemvProb {
  const bf16_t* W;             // [Nout][K] 16-bit, row-major
  const void* X;               // input columns [0, kx1): [n][ldx], fp32 or 16-bit
  const void* X2;              // input columns [kx1, K): [n][ldx2]; nullptr = zeros (all-zero flow half)
  const float* bias;           // [Nout], nullable
  float* Y;                    // [n][Nout] fp32
  const float* ln_g;           // non-null: X is the fp32 PRE-LayerNorm row [n][K] (n <= 4): the workgroup normalises it itself
  const float* ln_b;
  float ln_eps;
  int Nout, K, kx1, ldx, ldx2, x_bf16, block0;
};
struct GemvArgs { GemvProb p[2]; int nprob, n, rows; };

// output features per workgroup, 8 or 16: with fewer than ~one workgroup per CU at 16 rows, halve the tile (8 = half an MFMA M tile: the
// matrix pipe is idle anyway, and every CU pulls its share of the weights; the per-CU request rate, not HBM, bounds these kernels)
static inline int stream_rows_per_wg(int tiles16) { return tiles16 < 200 ? 8 : 16; }

// the one or two problems of a launch -> kernel arguments: a.rows, every problem's first block.  Returns the grid; *kmax = the largest K.
// The shape refusals are the caller's
static inline int fill_gemv_args(int nprob, const StreamGemv* pr, int n, GemvArgs& a, int* kmax) {
  a.nprob = nprob; a.n = n;
  int tiles16 = 0, blocks = 0;
  *kmax = 0;
  for (int i = 0; i < nprob; ++i) {
    *kmax = pr[i].K > *kmax ? pr[i].K : *kmax;
    tiles16 += pr[i].Nout / 16;
  }
  a.rows = stream_rows_per_wg(tiles16);
  for (int i = 0; i < nprob; ++i) {
    a.p[i] = GemvProb{(const bf16_t*)pr[i].W, pr[i].X, pr[i].X2, pr[i].bias, pr[i].Y, pr[i].ln_g, pr[i].ln_b, pr[i].ln_eps, pr[i].Nout, pr[i].K,
                      pr[i].kx1, pr[i].ldx, pr[i].ldx2, pr[i].x_bf16, blocks};
    blocks += pr[i].Nout / a.rows;
  }
  return blocks;
}

// f(op_tag<OT>{}) with the handle's 16-bit operand type; in f: `using OT = typename decltype(ot)::type`
template <typename OT> struct op_tag { using type = OT; };
template <typename F>
static inline void for_operand(bool f16, F&& f) {
  if (f16) f(op_tag<f16_t>{}); else f(op_tag<bf16_t>{});
}
// f(std::integral_constant<int, NT>{}, op_tag<OT>{}) with NT = ceil(C / 16) class tiles, 1..8 (C <= 128 is the caller's check)
template <typename F>
static inline void for_class_tiles(int C, bool f16, F&& f) {
  for_operand(f16, [&](auto ot) {
    switch ((C + 15) / 16) {
      case 1: f(std::integral_constant<int, 1>{}, ot); break;
      case 2: f(std::integral_constant<int, 2>{}, ot); break;
      case 3: f(std::integral_constant<int, 3>{}, ot); break;
      case 4: f(std::integral_constant<int, 4>{}, ot); break;
      case 5: f(std::integral_constant<int, 5>{}, ot); break;
      case 6: f(std::integral_constant<int, 6>{}, ot); break;
      case 7: f(std::integral_constant<int, 7>{}, ot); break;
      default: f(std::integral_constant<int, 8>{}, ot); break;
    }
  });
}
