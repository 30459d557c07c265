// THUMOS post-processing of an eval pass on the device (the reference's utils/postprocessing.py:4-29, applied in front of every metric
// when the data set is THUMOS): the optional 5-frame temporal max ("smooth"), the optional CliffDiving -> Diving merge ("switch") and the
// removal of the frames whose "ambiguous" target column is 1 - the kept rows of scores and targets written densely, in frame order.
//
// Three launches, nothing returns to the host between them:
//   thumos_count_kernel    one block per tile of kThumosTileRows rows: the kept rows of the tile -> cnt[tile]
//   thumos_scan_kernel     one block: cnt -> exclusive offsets in place, the total -> *n_valid (int64)
//   thumos_scatter_kernel  one block per tile: the keep flags again (4 bytes per row), a block scan gives every kept row its output row
//                          (offset of the tile + kept rows in front of it: stable, no atomics), then the tile is copied.
// The scatter with `smooth` stages the tile's rows plus the two rows above and below it in LDS, once (a flat 16-byte-aligned span of
// the score matrix when its rows are contiguous, whatever 4 C is: the LDS image is shifted by the span's misalignment so that every
// 16-byte global load lands on a 16-byte LDS slot), and every output takes its five values from there; without `smooth` there is no
// reuse and the rows go from HBM to HBM.  More than kThumosChunkCols classes: the columns are done in chunks of that many.
// Only comparisons and copies: every output bit is the input's.  max is numpy's: NaN propagates, first operand on equality.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kRows = kThumosTileRows;      // rows per tile
constexpr int kHalo = 2;                    // rows of a neighbour tile the 5-frame window reaches into
constexpr int kBlock = 256;
constexpr int kStage = kRows + 2 * kHalo;
// dynamic LDS (everything, so that the score image starts on a 16-byte boundary): dest[kRows] | wave sums[4] | score image
constexpr int kDestBytes = kRows * 4, kSumBytes = 16;

__device__ __forceinline__ bool keep_row(const float* __restrict__ target, long long ldt, const int* __restrict__ labels, long long i,
                                         int amb) {
  if (amb < 0) return true;
  return labels ? labels[i] != amb : target[i * ldt + amb] != 1.0f;
}

__device__ __forceinline__ float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }      // np.maximum(a, b)

__global__ __launch_bounds__(kRows) void thumos_count_kernel(const float* __restrict__ target, long long ldt, const int* __restrict__ labels,
                                                             long long n, int amb, int* __restrict__ cnt) {
  __shared__ int part[kRows / 64];
  const long long i = (long long)blockIdx.x * kRows + threadIdx.x;
  const bool keep = i < n && keep_row(target, ldt, labels, i, amb);
  const int c = __popcll(__ballot(keep));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kRows / 64; ++w) s += part[w];
    cnt[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(1024) void thumos_scan_kernel(int* __restrict__ cnt, long long ntiles, long long* __restrict__ n_valid) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (long long base = 0; base < ntiles; base += 1024) {      // block-uniform trip count
    const long long t = base + threadIdx.x;
    const int v = t < ntiles ? cnt[t] : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (t < ntiles) cnt[t] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_valid = carry_s;
}

struct ThumosArgs {
  const float* scores; long long lds;
  const float* target; long long ldt;
  const int* labels;
  long long n;
  int C, sw_from, sw_to, amb;      // sw_to < 0: no switch
  const int* offs;
  float* scores_out; float* target_out; int* labels_out;
  int chunk;                       // columns per pass over the tile
};

template <bool SMOOTH>
__global__ __launch_bounds__(kBlock) void thumos_scatter_kernel(const ThumosArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* dest = (int*)smem;
  int* wsum = (int*)(smem + kDestBytes);
  float* img = (float*)(smem + kDestBytes + kSumBytes);
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kRows;
  const int rows = (int)(a.n - r0 < kRows ? a.n - r0 : kRows);
  const int C = a.C;

  // ---- every kept row's output row
  {
    const bool keep = tid < rows && keep_row(a.target, a.ldt, a.labels, r0 + tid, a.amb);
    const unsigned long long m = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (tid < kRows) {
      int before = a.offs[blockIdx.x];
      for (int w = 0; w < wave; ++w) before += wsum[w];
      dest[tid] = keep ? before + rank : -1;
    }
    __syncthreads();
  }

  // ---- scores
  const long long lo = r0 - kHalo < 0 ? 0 : r0 - kHalo;                                 // staged rows [lo, hi)
  const long long hi = r0 + rows + kHalo > a.n ? a.n : r0 + rows + kHalo;
  for (int c0 = 0; c0 < C; c0 += a.chunk) {
    const int cc = C - c0 < a.chunk ? C - c0 : a.chunk;
    int shift = 0;
    if (SMOOTH) {
      const int nst = (int)(hi - lo);
      if (cc == C && a.lds == C) {
        // contiguous rows: one flat span of nst * C floats, read in 16-byte pieces from the aligned address below it
        const float* g0 = a.scores + lo * (long long)C;
        shift = (int)(((unsigned long long)(uintptr_t)g0 >> 2) & 3);
        const float* ga = g0 - shift;
        const int end = shift + nst * C;
        for (int j = tid * 4; j < end; j += kBlock * 4) {
          if (j >= shift && j + 4 <= end) {
            *(float4*)(img + j) = *(const float4*)(ga + j);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (j + k >= shift && j + k < end) img[j + k] = ga[j + k];
          }
        }
      } else {
        const int total = nst * cc, dr = kBlock / cc, dc = kBlock % cc;
        int row = tid / cc, col = tid % cc;
        for (int e = tid; e < total; e += kBlock) {
          img[e] = a.scores[(lo + row) * a.lds + c0 + col];
          row += dr; col += dc;
          if (col >= cc) { col -= cc; ++row; }
        }
      }
      __syncthreads();
    }
    // value of the smoothed (or plain) matrix at row i, column c: from the image when the column is in this chunk
    auto plain = [&](long long i, int c) -> float {
      if (SMOOTH && c >= c0 && c < c0 + cc) return img[shift + (int)(i - lo) * cc + (c - c0)];
      return a.scores[i * a.lds + c];
    };
    auto value = [&](long long i, int c) -> float {
      float v = plain(i, c);
      if (SMOOTH) {      // the reference's order: the row, one back, one ahead, two back, two ahead; outside [0, n): the row itself
        v = np_max(v, plain(i - 1 >= 0 ? i - 1 : i, c));
        v = np_max(v, plain(i + 1 < a.n ? i + 1 : i, c));
        v = np_max(v, plain(i - 2 >= 0 ? i - 2 : i, c));
        v = np_max(v, plain(i + 2 < a.n ? i + 2 : i, c));
      }
      return v;
    };
    {
      const int total = rows * cc, dr = kBlock / cc, dc = kBlock % cc;
      int row = tid / cc, col = tid % cc;
      for (int e = tid; e < total; e += kBlock) {
        const int d = dest[row];
        if (d >= 0) {
          const long long i = r0 + row;
          const int c = c0 + col;
          float v = value(i, c);
          if (c == a.sw_to) {
            const float f = value(i, a.sw_from);
            if (f > v) v = f;
          }
          a.scores_out[(long long)d * C + c] = v;
        }
        row += dr; col += dc;
        if (col >= cc) { col -= cc; ++row; }
      }
    }
    if (SMOOTH) __syncthreads();      // the image is overwritten by the next chunk
  }

  // ---- targets
  if (a.labels) {
    if (tid < rows && dest[tid] >= 0) a.labels_out[dest[tid]] = a.labels[r0 + tid];
  } else {
    // rows wider than the block are walked by column blocks (dr = 0, dc = kBlock would never wrap with the stepping above)
    if (C >= kBlock) {
      for (int row = 0; row < rows; ++row) {
        const int d = dest[row];
        if (d < 0) continue;
        for (int c = tid; c < C; c += kBlock) a.target_out[(long long)d * C + c] = a.target[(r0 + row) * a.ldt + c];
      }
    } else {
      const int total = rows * C, dr = kBlock / C, dc = kBlock % C;
      int row = tid / C, col = tid % C;
      for (int e = tid; e < total; e += kBlock) {
        const int d = dest[row];
        if (d >= 0) a.target_out[(long long)d * C + col] = a.target[(r0 + row) * a.ldt + col];
        row += dr; col += dc;
        if (col >= C) { col -= C; ++row; }
      }
    }
  }
}

long long n_tiles(long long n) { return (n + kRows - 1) / kRows; }

}  // namespace

size_t thumos_postprocess_workspace_bytes(long long n, int C) {
  (void)C;
  return (((size_t)n_tiles(n) * 4 + 15) & ~(size_t)15) + 16;      // the tiles' counts / offsets (int32), on a 16-byte boundary
}

int launch_thumos_postprocess(const float* scores, long long lds, const float* target, long long ldt, const int* labels, long long n, int C,
                              bool smooth, int sw_from, int sw_to, int amb, float* scores_out, float* target_out, int* labels_out,
                              long long* n_valid, void* ws, hipStream_t s) {
  if (n <= 0 || n >= (1ll << 31) || C < 1 || C > 65535 || !scores || (!target && !labels) || !scores_out || !n_valid || !ws) return -1;
  if (labels ? !labels_out : !target_out) return -1;
  if (sw_to >= 0 && (sw_to >= C || sw_from < 0 || sw_from >= C || sw_from == sw_to)) return -1;
  if (amb >= C || lds < C || (!labels && ldt < C)) return -1;
  int* cnt = (int*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
  const long long nt = n_tiles(n);
  thumos_count_kernel<<<(unsigned)nt, kRows, 0, s>>>(target, ldt, labels, n, amb, cnt);
  thumos_scan_kernel<<<1, 1024, 0, s>>>(cnt, nt, n_valid);
  ThumosArgs a;
  a.scores = scores; a.lds = lds; a.target = labels ? nullptr : target; a.ldt = ldt; a.labels = labels; a.n = n;
  a.C = C; a.sw_from = sw_from; a.sw_to = sw_to < 0 ? -1 : sw_to; a.amb = amb; a.offs = cnt;
  a.scores_out = scores_out; a.target_out = target_out; a.labels_out = labels_out;
  a.chunk = C < kThumosChunkCols ? C : kThumosChunkCols;
  if (smooth) {
    const size_t lds_bytes = kDestBytes + kSumBytes + ((size_t)kStage * a.chunk + 4) * 4;
    thumos_scatter_kernel<true><<<(unsigned)nt, kBlock, lds_bytes, s>>>(a);
  } else {
    thumos_scatter_kernel<false><<<(unsigned)nt, kBlock, kDestBytes + kSumBytes, s>>>(a);
  }
  return 0;
}
