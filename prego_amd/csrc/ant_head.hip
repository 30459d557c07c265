// Anticipation head of MiniROADA (MROADA.forward, model/rnn/rnn.py:113-136), fused, eval mode:
//   A_l      = relu(relu(h) W_a[l]^T + b_a[l])      anticipation_layer, rows l H .. l H + H - 1 of its weight (.view(B,S,L,H))
//   logits_l = A_l W_c^T + b_c                      the SAME f_classification weights as the frame's own logits
//   probs_l  = softmax(logits_l)                    eval branch (PREGO_FWD_SOFTMAX); argmax_l: first maximum wins
// for l = 0 .. L - 1, and the scatter from packed time-major rows to the caller's per-clip [T, L, C] / [T, L] arrays.
//
// One workgroup (4 waves) owns RB = 128 packed rows for the whole launch and walks (l, column block nb) in the same order as every other
// workgroup: step l's block nb of A_l ([128 rows][NB columns]) is a K = H product staged through LDS (both operands, double buffered, one
// barrier per k-step), its epilogue (bias, ReLU, operand type) writes it to LDS, and the four waves multiply it straight into their
// logits accumulators (wave w: rows 32 w .. 32 w + 31, all classes).  The [rows, L H] intermediate never exists in global memory, and the
// column blocks of one step meet in one register accumulator in nb order: no atomics, no cross-workgroup sums, bit-reproducible, and a
// row's result does not depend on where in the call it sits (the chunked pass and the split pass give the same bits).
// Traffic: W_a block nb of step l is read by every resident workgroup at about the same time (one L2 copy per XCD),
// the relu(h) tile of a workgroup is re-read once per (l, nb) block.
#include <type_traits>
#include "common.h"
#include "kernels.h"

namespace {
constexpr int kRB = 128;          // packed rows per workgroup
constexpr int kStageLd = 40;      // 16-bit elements per staged row: 32 k + 8 pad (80 B: 16 rows x 16 B hit 16 distinct bank slots)

template <typename WT> struct AntOps;
template <> struct AntOps<float> {
  static constexpr int EPV = 4;                   // elements per 16-byte vector
  typedef f32x4 vec;
};
template <> struct AntOps<bf16_t> { static constexpr int EPV = 8; typedef bf16x8 vec; };
template <> struct AntOps<f16_t> { static constexpr int EPV = 8; typedef bf16x8 vec; };

template <typename WT> __device__ __forceinline__ unsigned short to_op(float x);
template <> __device__ __forceinline__ unsigned short to_op<bf16_t>(float x) { return op16<bf16_t>::cvt(x); }
template <> __device__ __forceinline__ unsigned short to_op<f16_t>(float x) { return op16<f16_t>::cvt_sat(x); }

// one 16-row x 16-col tile, one k-vector (16-bit: k 32, fp32: k 16 as four 16x16x4 products)
template <typename WT>
__device__ __forceinline__ f32x4 mma(const typename AntOps<WT>::vec& a, const typename AntOps<WT>::vec& b, f32x4 c) {
  if constexpr (sizeof(WT) == 4) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
    return c;
  } else {
    return op16<WT>::mfma(a, b, c);
  }
}
}  // namespace

// STORE_A (training backward, ant_head_bwd.hip): the first product only, for the 128-row blocks that meet the device-side packed-row span
// [span[0], span[1]): A_l of those rows goes to a_out [rows][L * HID] in the operand type, with the bits of the forward (same k order,
// same epilogue).  The inference instantiations (STORE_A = false) are unchanged.
template <typename WT, int NTC, int NB, bool STORE_A = false>
__global__ __launch_bounds__(256) void ant_head_kernel(
    const WT* __restrict__ Hrelu,      // [nrows][HID] chunk-relative packed rows
    const WT* __restrict__ Wa,         // [L*HID][HID]
    const float* __restrict__ ba,      // [L*HID]
    const WT* __restrict__ Wc,         // [16*NTC][HID] zero padded rows
    const float* __restrict__ bc,      // [16*NTC] zero padded
    SlotPlan plan, int row0, int nrows, int HID, int L, int C, int apply_softmax,
    float* const* __restrict__ out_ptrs,     // per clip [T][L][C] fp32, entries nullable
    int* const* __restrict__ argmax_ptrs,    // per clip [T][L] int32, nullable array / entries
    const int2* __restrict__ rowmap,         // nullable: (clip, frame) of every row of this launch (chunk-relative index)
    WT* __restrict__ a_out = nullptr, const int* __restrict__ span = nullptr) {
  typedef AntOps<WT> O;
  typedef typename O::vec vec;
  constexpr int EPV = O::EPV;
  constexpr int ES = sizeof(WT);
  constexpr int BK = 4 * EPV;                         // k per stage: 64 bytes of a row
  constexpr int SLD = kStageLd * 2 / ES;              // staged row stride in elements (80 B)
  constexpr int NT = NB / 32;                         // 16-col tiles per wave (2 x 2 wave grid: wave owns 64 rows x NB / 2 cols)
  constexpr int ALD = NB + 16 / ES;                   // A_l block row stride in elements (+16 B: 16 rows on 16 distinct bank slots)
  constexpr int BCH = NB / 64;                        // 16-byte chunks of the W_a stage per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  WT* stA = (WT*)smem;                                // [2][kRB][SLD]
  WT* stB = stA + 2 * kRB * SLD;                      // [2][NB][SLD]
  WT* sA = stB + 2 * NB * SLD;                        // [kRB][ALD]   A_l block, the second product's operand
  unsigned long long* s_out = (unsigned long long*)(sA + kRB * ALD);   // [kRB] &out[clip][t][0][0] or 0
  unsigned long long* s_arg = s_out + kRB;                             // [kRB] &argmax[clip][t][0] or 0

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const int rbase = blockIdx.x * kRB;
  int span_lo = 0, span_hi = 0;
  if constexpr (STORE_A) {
    span_lo = span[0]; span_hi = span[1];
    if (rbase >= span_hi || rbase + kRB <= span_lo) return;      // the whole workgroup: no barrier has been reached
  }

  // ---- destinations of the workgroup's rows: one lookup per row, once
  if (!STORE_A && tid < kRB) {
    int r = rbase + tid;
    const bool live = r < nrows;
    if (!live) r = nrows - 1;
    int clip, t;
    if (rowmap != nullptr) {
      const int2 ct = rowmap[r];
      clip = ct.x; t = ct.y;
    } else {
      // plan tables as plain pointers (the SlotPlan struct indexed as a whole would live in scratch)
      const int* __restrict__ p_rowoff = plan.rowoff; const int* __restrict__ p_seg_off = plan.seg_off;
      const int* __restrict__ p_seg_clip = plan.seg_clip; const int* __restrict__ p_seg_start = plan.seg_start;
      const int row = row0 + r;
      int lo = 0, hi = plan.s_max;                    // rowoff[lo] <= row < rowoff[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p_rowoff[mid] <= row) lo = mid; else hi = mid;
      }
      const int slot = row - p_rowoff[lo];
      int k = p_seg_off[slot];
      const int kend = p_seg_off[slot + 1];
      while (k + 1 < kend && p_seg_start[k + 1] <= lo) ++k;
      clip = p_seg_clip[k]; t = lo - p_seg_start[k];
    }
    float* op = (live && out_ptrs) ? out_ptrs[clip] : nullptr;
    int* ap = (live && argmax_ptrs) ? argmax_ptrs[clip] : nullptr;
    s_out[tid] = op ? (unsigned long long)(op + (size_t)t * L * C) : 0ull;
    s_arg[tid] = ap ? (unsigned long long)(ap + (size_t)t * L) : 0ull;
  }

  // staging: this thread's 16-byte chunks of the relu(h) tile (2) and of the W_a block (BCH); rows beyond nrows repeat the last one
  int a_row[2], a_part[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i;
    a_row[i] = c >> 2; a_part[i] = c & 3;
  }
  const WT* a_src[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int r = rbase + a_row[i]; if (r > nrows - 1) r = nrows - 1;
    a_src[i] = Hrelu + (size_t)r * HID + a_part[i] * EPV;
  }
  const int nk = HID / BK, nnb = HID / NB;
  // STORE_A: one (step l, column block nb) per workgroup (grid.y, grid.z) - the span is a few row blocks, the steps and blocks give the
  // launch its width; the inference kernel walks every (l, nb) itself
  const int l_lo = STORE_A ? (int)blockIdx.y : 0, l_hi = STORE_A ? (int)blockIdx.y + 1 : L;
  const int nb_lo = STORE_A ? (int)blockIdx.z : 0, nb_hi = STORE_A ? (int)blockIdx.z + 1 : nnb;

  for (int l = l_lo; l < l_hi; ++l) {
    f32x4 acc2[2][NTC];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < NTC; ++j) acc2[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int nb = nb_lo; nb < nb_hi; ++nb) {
      const int col0 = l * HID + nb * NB;             // first W_a row of this block
      const WT* b_src[BCH];
#pragma unroll
      for (int i = 0; i < BCH; ++i) {
        const int c = tid + 256 * i;
        b_src[i] = Wa + (size_t)(col0 + (c >> 2)) * HID + (c & 3) * EPV;
      }
      f32x4 acc1[4][NT];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc1[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

      vec ra[2], rb[BCH];
      auto gload = [&](int ks) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ra[i] = *(const vec*)(a_src[i] + ks * BK);
#pragma unroll
        for (int i = 0; i < BCH; ++i) rb[i] = *(const vec*)(b_src[i] + ks * BK);
      };
      auto sstore = [&](int buf) {
        WT* A_ = stA + buf * kRB * SLD;
        WT* B_ = stB + buf * NB * SLD;
#pragma unroll
        for (int i = 0; i < 2; ++i) *(vec*)(A_ + a_row[i] * SLD + a_part[i] * EPV) = ra[i];
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
          const int c = tid + 256 * i;
          *(vec*)(B_ + (c >> 2) * SLD + (c & 3) * EPV) = rb[i];
        }
      };
      gload(0);
      sstore(0);
      __syncthreads();
      for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk) gload(ks + 1);
        const WT* A_ = stA + buf * kRB * SLD;
        const WT* B_ = stB + buf * NB * SLD;
        vec af[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) af[m] = *(const vec*)(A_ + (wr * 64 + m * 16 + l15) * SLD + l4 * EPV);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const vec bf = *(const vec*)(B_ + (wc * (NB / 2) + j * 16 + l15) * SLD + l4 * EPV);
#pragma unroll
          for (int m = 0; m < 4; ++m) acc1[m][j] = mma<WT>(af[m], bf, acc1[m][j]);
        }
        if (ks + 1 < nk) sstore(buf ^ 1);
        __syncthreads();
      }
      // epilogue of the block: bias, ReLU, operand type -> LDS.  Lane holds rows m*16 + l4*4 + e, columns j*16 + l15 of its tile
      if constexpr (STORE_A) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int cl = wc * (NB / 2) + j * 16 + l15;
          const float bias = ba[col0 + cl];
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc1[m][j][e] + bias;
              v = v > 0.f ? v : 0.f;
              const int r = rbase + wr * 64 + m * 16 + l4 * 4 + e;
              if (r >= span_lo && r < span_hi && r < nrows) {
                WT* dst = a_out + (size_t)r * L * HID + col0 + cl;
                if constexpr (ES == 4) *dst = v;
                else *(unsigned short*)dst = to_op<WT>(v);
              }
            }
        }
        continue;                                       // no second product: the next block's K loop starts with its own barriers
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int cl = wc * (NB / 2) + j * 16 + l15;
        const float bias = ba[col0 + cl];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc1[m][j][e] + bias;
            v = v > 0.f ? v : 0.f;
            const int rr = wr * 64 + m * 16 + l4 * 4 + e;
            if constexpr (ES == 4) sA[rr * ALD + cl] = v;
            else ((unsigned short*)sA)[rr * ALD + cl] = to_op<WT>(v);
          }
      }
      __syncthreads();
      // logits_l += A_l[:, block] W_c[:, block]^T : wave w, rows 32 w + 16 t + ..., every class tile; k in block order
#pragma unroll
      for (int kk = 0; kk < NB; kk += BK) {
        vec af2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) af2[t] = *(const vec*)(sA + (wave * 32 + t * 16 + l15) * ALD + kk + l4 * EPV);
#pragma unroll
        for (int j = 0; j < NTC; ++j) {
          const vec bf = *(const vec*)(Wc + (size_t)(j * 16 + l15) * HID + nb * NB + kk + l4 * EPV);
#pragma unroll
          for (int t = 0; t < 2; ++t) acc2[t][j] = mma<WT>(af2[t], bf, acc2[t][j]);
        }
      }
      // (the next block's first LDS write of sA is behind at least two barriers of its K loop)
    }

    if constexpr (STORE_A) continue;
    // step l done: softmax / argmax of each row's logits_l, rows 32 wave + 16 t + 4 l4 + e, classes 16 j + l15
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[NTC];
        float mx = -INFINITY;
        int mi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NTC; ++j) {
          const int c = j * 16 + l15;
          v[j] = acc2[t][j][e] + bc[c];
          if (c < C && v[j] > mx) { mx = v[j]; mi = c; }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float omx = __shfl_xor(mx, o, 64);
          const int omi = __shfl_xor(mi, o, 64);
          if (omx > mx || (omx == mx && omi < mi)) { mx = omx; mi = omi; }
        }
        if (apply_softmax) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < NTC; ++j) {
            const int c = j * 16 + l15;
            v[j] = (c < C) ? __expf(v[j] - mx) : 0.f;
            s += v[j];
          }
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
          const float inv = 1.0f / s;
#pragma unroll
          for (int j = 0; j < NTC; ++j) v[j] *= inv;
        }
        const int rr = wave * 32 + t * 16 + l4 * 4 + e;
        float* op = (float*)s_out[rr];
        if (op) {
          op += (size_t)l * C;
#pragma unroll
          for (int j = 0; j < NTC; ++j) {
            const int c = j * 16 + l15;
            if (c < C) op[c] = v[j];
          }
        }
        if (l15 == 0) {
          int* ap = (int*)s_arg[rr];
          if (ap) ap[l] = mi;
        }
      }
  }
}

template <typename WT, int NTC, int NB>
static int ant_launch(const void* Hrelu, const void* Wa, const float* ba, const void* Wc, const float* bc, const SlotPlan& plan, int row0,
                      int nrows, int hid, int L, int C, int apply_softmax, float* const* out_ptrs, int* const* argmax_ptrs, const void* rowmap,
                      hipStream_t s) {
  constexpr int ES = sizeof(WT);
  const size_t lds = (size_t)(2 * kRB * (kStageLd * 2 / ES) + 2 * NB * (kStageLd * 2 / ES) + kRB * (NB + 16 / ES)) * ES + 2 * kRB * 8;
  static DeviceOnce once;
  once.run([&] { (void)hipFuncSetAttribute((const void*)ant_head_kernel<WT, NTC, NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
  const int grid = (nrows + kRB - 1) / kRB;
  ant_head_kernel<WT, NTC, NB><<<grid, 256, lds, s>>>((const WT*)Hrelu, (const WT*)Wa, ba, (const WT*)Wc, bc, plan, row0, nrows, hid, L, C,
                                                      apply_softmax, out_ptrs, argmax_ptrs, (const int2*)rowmap);
  return 0;
}

int launch_ant_head(bool bf16, bool f16, const void* Hrelu, const void* Wa, const float* ba, const void* Wc, const float* bc,
                    const SlotPlan& plan, int row0, int nrows, int hid, int L, int C, int apply_softmax, float* const* out_ptrs,
                    int* const* argmax_ptrs, const void* rowmap, hipStream_t s) {
  if (nrows <= 0) return 0;
  if (L < 1 || L > 32 || C < 1 || C > 128 || hid % 256 != 0) return -1;
  const int ntc = (C + 15) / 16;
  // 16-bit operands: column blocks of 256 (128 KB of LDS, the relu(h) tile is re-read H / 256 times per step); fp32: blocks of 128
#define AL(WT, N, NBV) return ant_launch<WT, N, NBV>(Hrelu, Wa, ba, Wc, bc, plan, row0, nrows, hid, L, C, apply_softmax, out_ptrs, argmax_ptrs, rowmap, s)
#define AD(N)                                 \
  case N:                                     \
    if (bf16 && f16) AL(f16_t, N, 256);       \
    else if (bf16) AL(bf16_t, N, 256);        \
    else AL(float, N, 128);
  switch (ntc) {
    AD(1) AD(2) AD(3) AD(4) AD(5) AD(6) AD(7) AD(8)
    default: return -1;
  }
#undef AD
#undef AL
}

// A_l = relu(relu(h) W_a[l]^T + b_a[l]) in the operand type for the packed rows [span[0], span[1]) of [0, nrows) (device-side span), into
// a_out [nrows][L * hid]: the forward's first product and epilogue, bit for bit (ant_head_kernel<..., STORE_A>)
int launch_ant_head_store_a(bool bf16, const void* Hrelu, const void* Wa, const float* ba, int nrows, int hid, int L, void* a_out,
                            const int* span, hipStream_t s) {
  if (nrows <= 0) return 0;
  if (L < 1 || L > 32 || hid % 256 != 0) return -1;
  auto go = [&](auto tag, auto nbc) {
    typedef decltype(tag) WT;
    constexpr int NB = decltype(nbc)::value;
    constexpr int ES = sizeof(WT);
    // the two staging buffers only: STORE_A never touches the A_l block or the destination tables behind them (61 KB on bf16: two
    // workgroups per CU instead of one)
    const size_t lds = (size_t)(2 * kRB * (kStageLd * 2 / ES) + 2 * NB * (kStageLd * 2 / ES)) * ES;
    static DeviceOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)ant_head_kernel<WT, 1, NB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    const SlotPlan plan{};
    ant_head_kernel<WT, 1, NB, true><<<dim3((nrows + kRB - 1) / kRB, L, hid / NB), 256, lds, s>>>((const WT*)Hrelu, (const WT*)Wa, ba, nullptr, nullptr, plan, 0,
                                                                                nrows, hid, L, 1, 0, nullptr, nullptr, nullptr, (WT*)a_out, span);
    return 0;
  };
  return bf16 ? go(bf16_t{}, std::integral_constant<int, 256>{}) : go(float{}, std::integral_constant<int, 128>{});
}
