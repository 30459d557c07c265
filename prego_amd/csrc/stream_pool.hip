// Stream pool (prego_stream_pool_*, prego_miniroad_step_pool; host side: stream_pool.cpp): every live video owns a SLOT of the caller's
// device block - its GRU state row and its running aggregation record (utils/aggregate.py:55-78, one id at a time) - and one call advances
// any subset of the slots by one frame.  The kernels here only move state rows and count votes; the frame itself is the unchanged wide
// step on a dense copy of the active rows (stream_wide.hip), so the pool adds no arithmetic.
//   pool_gather   h_ws[i] <- pool.h[slots[i]]                       one workgroup per active stream, 16-byte accesses
//   pool_commit<Span>  pool.h[slots[i]] <- h_ws[i], then lane 0 of workgroup i votes the ids of slot i in frame order into its record
//   pool_vote<Span>    the vote alone, ids from the caller's device vector  (one lane per stream)
//     Span says which ids belong to active stream i: UniformSpan [i K, i K + K) - K by value, K = 1 the one-frame call, no table in the
//     kernel arguments - or RaggedSpan [off, off + count) of a RaggedMap entry (packed rows, by value as the slots)
//   pool_flush    votes a slot's unfinished window (the reference's shorter last window, aggregate.py:57-58)
//   pool_reset    zeroes a slot's state row and record
// The slot list travels by value in the kernel arguments (PoolSlots, 1 KB): no staging buffer, no H2D copy, nothing for the caller to
// keep alive.  The host has checked every slot against the capacity and the list for duplicates, so no two lanes meet on a slot.
// Record of a slot (PoolGeom::rec_words 32-bit words, 16-byte aligned; kPoolRecHeader = 4):
//   [0] frames   [1] last vote + 1 (0 = no window voted yet)   [2] n_events   [3] overflow (bit 0: record full, bit 1: id out of range)
//   [4 ..) counts[ncls_pad]   event_id[max_events]   event_start[max_events]
// An all-zero slot is an empty one, which is why opening a stream launches nothing.
#include "common.h"
#include "kernels.h"
#include "pool_record.h"

__global__ __launch_bounds__(256) void pool_gather_kernel(PoolGeom g, PoolSlots sl, float* __restrict__ h_ws) {
  const int i = blockIdx.x;
  const f32x4* src = (const f32x4*)(g.h + (size_t)sl.s[i] * g.hid);
  f32x4* dst = (f32x4*)(h_ws + (size_t)i * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
}

// which ids of a call belong to active stream i, the policy of pool_commit and pool_vote (as UniformRows / RaggedRows of stream_frames.hip)
struct UniformSpan {                     // K ids per stream, stream-major; a window boundary may fall inside a burst any number of times
  int K;
  __device__ __forceinline__ int off(int i) const { return i * K; }
  __device__ __forceinline__ int count(int) const { return K; }
};
struct RaggedSpan {                      // entry i of the table: packed rows in the caller's order
  RaggedMap rows;
  __device__ __forceinline__ int off(int i) const { return (int)ragged_off(rows.e[i]); }
  __device__ __forceinline__ int count(int i) const { return (int)ragged_count(rows.e[i]); }
};

template <class Span>
__device__ __forceinline__ void pool_vote_span(const PoolGeom& g, int slot, const Span& span, int i, const int* __restrict__ ids) {
  int* rec = pool_record(g, slot);
  const int off = span.off(i), K = span.count(i);
  for (int t = 0; t < K; ++t) pool_vote_update(rec, g, ids[off + t]);
}

template <class Span>
__global__ __launch_bounds__(256) void pool_commit_kernel(PoolGeom g, PoolSlots sl, Span span, const float* __restrict__ h_ws,
                                                          const int* __restrict__ argmax) {
  const int i = blockIdx.x, slot = sl.s[i];
  const f32x4* src = (const f32x4*)(h_ws + (size_t)i * g.hid);
  f32x4* dst = (f32x4*)(g.h + (size_t)slot * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
  if (threadIdx.x == 0) pool_vote_span(g, slot, span, i, argmax);
}

template <class Span>
__global__ __launch_bounds__(64) void pool_vote_kernel(PoolGeom g, PoolSlots sl, Span span, int n, const int* __restrict__ ids) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) pool_vote_span(g, sl.s[i], span, i, ids);
}

__global__ __launch_bounds__(64) void pool_flush_kernel(PoolGeom g, PoolSlots sl, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  pool_flush_window(pool_record(g, sl.s[i]), g);
}

__global__ __launch_bounds__(256) void pool_reset_kernel(PoolGeom g, PoolSlots sl) {
  const int slot = sl.s[blockIdx.x];
  f32x4* hrow = (f32x4*)(g.h + (size_t)slot * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) hrow[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4* rec = (u32x4*)pool_record(g, slot);
  for (int k = threadIdx.x; k < (g.rec_words >> 2); k += 256) rec[k] = (u32x4){0u, 0u, 0u, 0u};
}

// Every launcher: 1 <= n <= 256 host slot numbers, each in [0, g.capacity) and named once (stream_pool.cpp checks); -1 = nothing launched
static bool pool_slots(const PoolGeom& g, const int* slots, int n, PoolSlots* sl) {
  if (!g.h || !g.rec || !slots || n < 1 || n > kPoolMaxActive || (g.hid & 3) || (g.rec_words & 3)) return false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= g.capacity) return false;
    sl->s[i] = slots[i];
  }
  for (int i = n; i < kPoolMaxActive; ++i) sl->s[i] = 0;
  return true;
}

int launch_pool_gather(const PoolGeom& g, const int* slots, int n, float* h_ws, hipStream_t s) {
  PoolSlots sl;
  if (!h_ws || !pool_slots(g, slots, n, &sl)) return -1;
  pool_gather_kernel<<<n, 256, 0, s>>>(g, sl, h_ws);
  return 0;
}

// a ragged call's table: 1..32 ids per entry, every span inside the n_rows <= 256 packed rows
static bool ragged_span(const RaggedMap& rows, int n, int n_rows, RaggedSpan* span) {
  if (n_rows < n || n_rows > kPoolMaxActive) return false;
  for (int i = 0; i < n; ++i)
    if (ragged_count(rows.e[i]) < 1u || ragged_count(rows.e[i]) > 32u || ragged_off(rows.e[i]) + ragged_count(rows.e[i]) > (unsigned)n_rows) return false;
  span->rows = rows;
  return true;
}

template <class Span>
static int pool_commit(const PoolGeom& g, const int* slots, int n, const Span& span, const float* h_ws, const int* argmax, hipStream_t s) {
  PoolSlots sl;
  if (!h_ws || !argmax || !pool_slots(g, slots, n, &sl)) return -1;
  pool_commit_kernel<Span><<<n, 256, 0, s>>>(g, sl, span, h_ws, argmax);
  return 0;
}

template <class Span>
static int pool_vote(const PoolGeom& g, const int* slots, int n, const Span& span, const int* ids, hipStream_t s) {
  PoolSlots sl;
  if (!ids || !pool_slots(g, slots, n, &sl)) return -1;
  pool_vote_kernel<Span><<<(n + 63) / 64, 64, 0, s>>>(g, sl, span, n, ids);
  return 0;
}

int launch_pool_commit(const PoolGeom& g, const int* slots, int n, int K, const float* h_ws, const int* argmax, hipStream_t s) {
  if (K < 1 || K > 32 || n < 1 || n > kPoolMaxActive || n * K > kPoolMaxActive) return -1;
  return pool_commit(g, slots, n, UniformSpan{K}, h_ws, argmax, s);
}

int launch_pool_commit_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const float* h_ws,
                              const int* argmax, hipStream_t s) {
  RaggedSpan span;
  return ragged_span(rows, n, n_rows, &span) ? pool_commit(g, slots, n, span, h_ws, argmax, s) : -1;
}

int launch_pool_vote(const PoolGeom& g, const int* slots, int n, const int* ids, hipStream_t s) {
  return pool_vote(g, slots, n, UniformSpan{1}, ids, s);
}

int launch_pool_vote_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const int* ids, hipStream_t s) {
  RaggedSpan span;
  return ragged_span(rows, n, n_rows, &span) ? pool_vote(g, slots, n, span, ids, s) : -1;
}

int launch_pool_flush(const PoolGeom& g, const int* slots, int n, hipStream_t s) {
  PoolSlots sl;
  if (!pool_slots(g, slots, n, &sl)) return -1;
  pool_flush_kernel<<<(n + 63) / 64, 64, 0, s>>>(g, sl, n);
  return 0;
}

int launch_pool_reset(const PoolGeom& g, const int* slots, int n, hipStream_t s) {
  PoolSlots sl;
  if (!pool_slots(g, slots, n, &sl)) return -1;
  pool_reset_kernel<<<n, 256, 0, s>>>(g, sl);
  return 0;
}
