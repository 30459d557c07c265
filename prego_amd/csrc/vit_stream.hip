// Transformer stream pool (prego_vit_stream_pool_*, prego_vit_step_pool; host side: vit_stream.cpp): every live video owns a SLOT of the
// caller's device block - a ring of its last `window` encoded frames, two ring words and the vote record of stream_pool.hip - and one call
// gives any subset of the slots one new frame and runs one ViTEnc window per slot.  linear_encoding (ViT.py:124) does not depend on the
// position inside the window (the positional row is added afterwards, ViT.py:129), so a frame is encoded ONCE, when it arrives, and the
// ring keeps the fp32 row prego_vit_forward_frames keeps in its `enc` buffer.
//   vit_ring_commit   ring[slots[i]][head] <- enc[i]; head <- (head + 1) mod T, fill <- min(fill + 1, T)     one workgroup per slot
//   vit_ring_tokens   vit_sliding_tokens_kernel (vit.hip) with the rings as its source: the row body is vit_token_row.h, shared
//   vit_ring_window   a slot's logical window, oldest frame first, for inspection
//   vit_burst_tokens        a burst (count[i] frames for slots[i], packed rows): one window per packed row out of the rings as they stood
//                           BEFORE the call and the call's own encoded rows; the same row body
//   vit_ring_commit_burst   the count[i] rows of each slot into its ring, then head and fill advance; one workgroup per slot
// Token j of slot's window, T = window, the newest frame just committed (ViT.py:124-129, dataset.py:53-55 for the zero rows in front):
//   j == T          cls + pe[T]
//   j <  T - fill   enc_b + pe[j]                        a zero feature row encodes to the bias alone
//   otherwise       ring[(head + j) mod T] + pe[j]       = (head - (T - j)) mod T: token T - 1 is row head - 1, the newest
// Window of (slot i, burst frame k), head / fill the ring words before the call, d = T - 1 - j frames back from token j < T:
//   d <= k          enc[off[i] + k - d] + pe[j]          a row of this call
//   d - k > fill    enc_b + pe[j]
//   otherwise       ring[(head - (d - k)) mod T] + pe[j] the ring as it was: vit_burst_tokens runs before vit_ring_commit_burst
// The slot list travels by value in the kernel arguments (PoolSlots), as in every pool kernel; the host has checked every slot against
// the capacity and the list for duplicates, so no two workgroups meet on a slot.  No atomics, no LDS, no spins.
#include "common.h"
#include "kernels.h"
#include "vit_token_row.h"

namespace {
__device__ __forceinline__ const float* ring_row(const VitRing& r, int slot, int head, int j) {
  int at = head + j;                                     // head, j in [0, T)
  if (at >= r.T) at -= r.T;
  return r.ring + ((size_t)slot * r.T + at) * r.E;
}
}  // namespace

__global__ __launch_bounds__(256) void vit_ring_commit_kernel(VitRing r, PoolSlots sl, const float* __restrict__ enc) {
  const int i = blockIdx.x, slot = sl.s[i];
  int* hf = r.hf + (size_t)slot * kVitRingStateWords;
  const int head = hf[0], fill = hf[1];
  const f32x4* src = (const f32x4*)(enc + (size_t)i * r.E);
  f32x4* dst = (f32x4*)(r.ring + ((size_t)slot * r.T + head) * r.E);
  for (int k = threadIdx.x; k < (r.E >> 2); k += 256) dst[k] = src[k];
  __syncthreads();                                       // every wave has read head before lane 0 moves it
  if (threadIdx.x == 0) {
    hf[0] = head + 1 == r.T ? 0 : head + 1;
    hf[1] = fill < r.T ? fill + 1 : r.T;
  }
}

template <int MAXV, typename OT>
__global__ __launch_bounds__(256) void vit_ring_tokens_kernel(VitRing r, PoolSlots sl, int n, const float* __restrict__ enc_b,
                                                              const float* __restrict__ cls, const float* __restrict__ pe,
                                                              float* __restrict__ x, const float* __restrict__ ln_w,
                                                              const float* __restrict__ ln_b, bf16_t* __restrict__ xn,
                                                              float* __restrict__ x0) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform: the slot and its ring words are scalar loads
  const int T = r.T, N = T + 1, E = r.E;
  for (int row = blockIdx.x * 4 + wave; row < n * N; row += gridDim.x * 4) {      // n <= 256 windows: n N fits an int
    const int b = row / N, j = row - b * N;
    const int slot = sl.s[b];
    const int* hf = r.hf + (size_t)slot * kVitRingStateWords;
    const int head = hf[0], fill = hf[1];
    const float* src = j == T ? cls : (j < T - fill ? enc_b : ring_row(r, slot, head, j));
    vit_token_row<MAXV, OT>(src, pe + (size_t)j * E, E, lane, x ? x + (size_t)row * E : nullptr,
                            (x0 && j == 0) ? x0 + (size_t)b * E : nullptr, ln_w, ln_b, xn ? xn + (size_t)row * E : nullptr);
  }
}

__global__ __launch_bounds__(256) void vit_ring_window_kernel(VitRing r, int slot, const float* __restrict__ enc_b, float* __restrict__ out,
                                                              int* __restrict__ fill_out) {
  const int j = blockIdx.x;
  const int* hf = r.hf + (size_t)slot * kVitRingStateWords;
  const int head = hf[0], fill = hf[1];
  const f32x4* src = (const f32x4*)(j < r.T - fill ? enc_b : ring_row(r, slot, head, j));
  f32x4* dst = (f32x4*)(out + (size_t)j * r.E);
  for (int k = threadIdx.x; k < (r.E >> 2); k += 256) dst[k] = src[k];
  if (j == 0 && threadIdx.x == 0 && fill_out) *fill_out = fill;
}

// vit_ring_tokens with two sources.  Packed row b belongs to the slot of by_row.e[b] (entry = off | i << 16 | count << 24, kernels.h), its
// burst frame is k = b - off; all of it is wave-uniform, so slot, head, fill, off and k are scalar
template <int MAXV, typename OT>
__global__ __launch_bounds__(256) void vit_burst_tokens_kernel(VitRing r, PoolSlots sl, RaggedMap by_row, int R, const float* __restrict__ enc,
                                                               const float* __restrict__ enc_b, const float* __restrict__ cls,
                                                               const float* __restrict__ pe, float* __restrict__ x,
                                                               const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                               bf16_t* __restrict__ xn, float* __restrict__ x0) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = r.T, N = T + 1, E = r.E;
  for (int row = blockIdx.x * 4 + wave; row < R * N; row += gridDim.x * 4) {      // R <= 256 windows: R N fits an int
    const int b = row / N, j = row - b * N;
    const unsigned e = by_row.e[b];
    const int k = b - (int)ragged_off(e);                  // 0 <= k < count <= T
    const int slot = sl.s[ragged_stream(e)];
    const int* hf = r.hf + (size_t)slot * kVitRingStateWords;
    const int head = hf[0], fill = hf[1];
    const int d = T - 1 - j;                               // frames back from the window's newest; -1 for the cls row
    const float* src;
    if (j == T) src = cls;
    else if (d <= k) src = enc + (size_t)(b - d) * E;      // b - d >= b - k = off
    else if (d - k > fill) src = enc_b;
    else {
      int at = head - (d - k);                             // 1 <= d - k <= T - 1, head in [0, T)
      if (at < 0) at += T;
      src = r.ring + ((size_t)slot * T + at) * E;
    }
    vit_token_row<MAXV, OT>(src, pe + (size_t)j * E, E, lane, x ? x + (size_t)row * E : nullptr,
                            (x0 && j == 0) ? x0 + (size_t)b * E : nullptr, ln_w, ln_b, xn ? xn + (size_t)row * E : nullptr);
  }
}

// One workgroup per slot: its count <= T rows go to count different ring rows, so the only hazard is the one vit_ring_commit has - every
// wave reads head and fill before the barrier, lane 0 moves them after it - and no other workgroup touches the slot
__global__ __launch_bounds__(256) void vit_ring_commit_burst_kernel(VitRing r, PoolSlots sl, RaggedMap by_slot, const float* __restrict__ enc) {
  const int i = blockIdx.x, slot = sl.s[i];
  const unsigned e = by_slot.e[i];
  const int off = (int)ragged_off(e), K = (int)ragged_count(e);
  int* hf = r.hf + (size_t)slot * kVitRingStateWords;
  const int head = hf[0], fill = hf[1];
  for (int k = 0; k < K; ++k) {
    int at = head + k;                                     // k < K <= T
    if (at >= r.T) at -= r.T;
    const f32x4* src = (const f32x4*)(enc + (size_t)(off + k) * r.E);
    f32x4* dst = (f32x4*)(r.ring + ((size_t)slot * r.T + at) * r.E);
    for (int c = threadIdx.x; c < (r.E >> 2); c += 256) dst[c] = src[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int h2 = head + K;
    if (h2 >= r.T) h2 -= r.T;
    hf[0] = h2;
    hf[1] = fill + K < r.T ? fill + K : r.T;
  }
}

// Every launcher: 1 <= n <= 256 host slot numbers, each in [0, r.capacity) (vit_stream.cpp also checks that none is named twice); E a
// multiple of 256, at most 4096 (prego_vit_create: a multiple of 512); -1 = nothing launched
static bool ring_slots(const VitRing& r, const int* slots, int n, PoolSlots* sl) {
  if (!r.ring || !r.hf || !slots || n < 1 || n > kPoolMaxActive || r.T < 1 || r.E < 256 || r.E % 256 || r.E > 4096) return false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= r.capacity) return false;
    sl->s[i] = slots[i];
  }
  for (int i = n; i < kPoolMaxActive; ++i) sl->s[i] = 0;
  return true;
}

int launch_vit_ring_commit(const VitRing& r, const int* slots, int n, const float* enc, hipStream_t s) {
  PoolSlots sl;
  if (!enc || !ring_slots(r, slots, n, &sl)) return -1;
  vit_ring_commit_kernel<<<n, 256, 0, s>>>(r, sl, enc);
  return 0;
}

int launch_vit_ring_tokens(const VitRing& r, const int* slots, int n, const float* enc_b, const float* cls, const float* pe, float* x,
                           const float* ln_w, const float* ln_b, void* xn, float* x0, hipStream_t s, bool f16) {
  PoolSlots sl;
  if (!enc_b || !cls || !pe || (xn && (!ln_w || !ln_b)) || r.T > (1 << 22) || !ring_slots(r, slots, n, &sl)) return -1;
  const int rows = n * (r.T + 1);
  const int grid = (rows + 3) / 4 < 32768 ? (rows + 3) / 4 : 32768;
#define VRT(MV, OT) vit_ring_tokens_kernel<MV, OT><<<grid, 256, 0, s>>>(r, sl, n, enc_b, cls, pe, x, ln_w, ln_b, (bf16_t*)xn, x0)
  if (r.E <= 2048) { if (f16) VRT(8, f16_t); else VRT(8, bf16_t); }
  else { if (f16) VRT(16, f16_t); else VRT(16, bf16_t); }
#undef VRT
  return 0;
}

int launch_vit_ring_window(const VitRing& r, int slot, const float* enc_b, float* out, int* fill_out, hipStream_t s) {
  PoolSlots sl;
  if (!enc_b || !out || !ring_slots(r, &slot, 1, &sl)) return -1;
  vit_ring_window_kernel<<<r.T, 256, 0, s>>>(r, slot, enc_b, out, fill_out);
  return 0;
}

// by_slot: entry i = off | i << 16 | count << 24 with the offsets the prefix sums of the counts, every count in 1..min(32, T), the counts
// summing to n_rows <= 256
static bool burst_map(const VitRing& r, const RaggedMap& by_slot, int n, int n_rows) {
  if (n_rows < n || n_rows > kPoolMaxActive) return false;
  const unsigned kmax = r.T < 32 ? (unsigned)r.T : 32u;
  unsigned at = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned e = by_slot.e[i];
    if (ragged_off(e) != at || ragged_stream(e) != (unsigned)i || ragged_count(e) < 1u || ragged_count(e) > kmax) return false;
    at += ragged_count(e);
  }
  return at == (unsigned)n_rows;
}

int launch_vit_burst_tokens(const VitRing& r, const int* slots, int n, const RaggedMap& by_slot, const RaggedMap& by_row, int n_rows,
                            const float* enc, const float* enc_b, const float* cls, const float* pe, float* x, const float* ln_w,
                            const float* ln_b, void* xn, float* x0, hipStream_t s, bool f16) {
  PoolSlots sl;
  if (!enc || !enc_b || !cls || !pe || (xn && (!ln_w || !ln_b)) || r.T > (1 << 22) || !ring_slots(r, slots, n, &sl) ||
      !burst_map(r, by_slot, n, n_rows))
    return -1;
  for (int i = 0; i < n; ++i)
    for (unsigned b = ragged_off(by_slot.e[i]); b < ragged_off(by_slot.e[i]) + ragged_count(by_slot.e[i]); ++b)
      if (by_row.e[b] != by_slot.e[i]) return -1;
  const int rows = n_rows * (r.T + 1);
  const int grid = (rows + 3) / 4 < 32768 ? (rows + 3) / 4 : 32768;
#define VBT(MV, OT) vit_burst_tokens_kernel<MV, OT><<<grid, 256, 0, s>>>(r, sl, by_row, n_rows, enc, enc_b, cls, pe, x, ln_w, ln_b, (bf16_t*)xn, x0)
  if (r.E <= 2048) { if (f16) VBT(8, f16_t); else VBT(8, bf16_t); }
  else { if (f16) VBT(16, f16_t); else VBT(16, bf16_t); }
#undef VBT
  return 0;
}

int launch_vit_ring_commit_burst(const VitRing& r, const int* slots, int n, const RaggedMap& by_slot, int n_rows, const float* enc,
                                 hipStream_t s) {
  PoolSlots sl;
  if (!enc || !ring_slots(r, slots, n, &sl) || !burst_map(r, by_slot, n, n_rows)) return -1;
  vit_ring_commit_burst_kernel<<<n, 256, 0, s>>>(r, sl, by_slot, enc);
  return 0;
}
