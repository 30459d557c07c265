// Stream pool (prego_stream_pool_*, prego_miniroad_step_pool; host side: stream_pool.cpp): every live video owns a SLOT of the caller's
// device block - its GRU state row and its running aggregation record (utils/aggregate.py:55-78, one id at a time) - and one call advances
// any subset of the slots by one frame.  The kernels here only move state rows and count votes; the frame itself is the unchanged wide
// step on a dense copy of the active rows (stream_wide.hip), so the pool adds no arithmetic.
//   pool_gather   h_ws[i] <- pool.h[slots[i]]                       one workgroup per active stream, 16-byte accesses
//   pool_commit   pool.h[slots[i]] <- h_ws[i], then lane 0 of workgroup i votes argmax[i] into the slot's record
//   pool_commit_frames  pool_commit after a burst of K frames per slot: the state once, K votes in frame order by the slot's lane
//   pool_commit_ragged  pool_commit after a ragged burst: a frame count per slot, the ids in packed rows (RaggedMap, by value as the slots)
//   pool_vote     the vote alone, ids from the caller's device vector  (one lane per stream)
//   pool_vote_ragged  the vote alone for a ragged burst: a frame count per slot, the ids in packed rows (the Transformer pool's bursts)
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

namespace {
__device__ __forceinline__ int* pool_record(const PoolGeom& g, int slot) { return g.rec + (size_t)slot * g.rec_words; }

// the window [start, frames) is complete: np.argmax(np.bincount(.)) - the lowest id with the maximal count -, counts cleared, and an
// event appended when the vote differs from the previous window's (aggregate.py:75-78) or is the first
__device__ __forceinline__ void pool_close_window(int* __restrict__ rec, const PoolGeom& g, int start) {
  unsigned* counts = (unsigned*)(rec + kPoolRecHeader);
  int best = 0;
  unsigned best_n = counts[0];
  for (int c = 1; c < g.ncls; ++c) {
    const unsigned v = counts[c];
    if (v > best_n) { best_n = v; best = c; }
  }
  for (int c = 0; c < g.ncls; ++c) counts[c] = 0u;
  if (best + 1 != rec[1]) {
    const int n = rec[2];
    if (n < g.max_events) {
      rec[kPoolRecHeader + g.ncls_pad + n] = best;
      rec[kPoolRecHeader + g.ncls_pad + g.max_events + n] = start;
      rec[2] = n + 1;
    } else {
      rec[3] |= kPoolOverflowFull;                           // the event is dropped: nothing is written past max_events
    }
  }
  rec[1] = best + 1;
}

// one frame's id into a slot's record: the update rule shared by pool_commit and pool_vote
__device__ __forceinline__ void pool_vote_update(int* __restrict__ rec, const PoolGeom& g, int id) {
  if ((unsigned)id >= (unsigned)g.ncls) { rec[3] |= kPoolOverflowBadId; return; }     // np.bincount would raise: nothing is counted
  unsigned* counts = (unsigned*)(rec + kPoolRecHeader);
  counts[id] += 1u;
  const int frames = rec[0] + 1;
  rec[0] = frames;
  if (frames % g.window == 0) pool_close_window(rec, g, frames - g.window);
}
}  // namespace

__global__ __launch_bounds__(256) void pool_gather_kernel(PoolGeom g, PoolSlots sl, float* __restrict__ h_ws) {
  const int i = blockIdx.x;
  const f32x4* src = (const f32x4*)(g.h + (size_t)sl.s[i] * g.hid);
  f32x4* dst = (f32x4*)(h_ws + (size_t)i * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
}

__global__ __launch_bounds__(256) void pool_commit_kernel(PoolGeom g, PoolSlots sl, const float* __restrict__ h_ws,
                                                          const int* __restrict__ argmax) {
  const int i = blockIdx.x, slot = sl.s[i];
  const f32x4* src = (const f32x4*)(h_ws + (size_t)i * g.hid);
  f32x4* dst = (f32x4*)(g.h + (size_t)slot * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
  if (threadIdx.x == 0) pool_vote_update(pool_record(g, slot), g, argmax[i]);
}

// pool_commit for a burst of K frames per slot: the ids of slot i are argmax[i K .. i K + K), voted in frame order by one lane, so a window
// boundary may fall inside the burst any number of times
__global__ __launch_bounds__(256) void pool_commit_frames_kernel(PoolGeom g, PoolSlots sl, int K, const float* __restrict__ h_ws,
                                                                 const int* __restrict__ argmax) {
  const int i = blockIdx.x, slot = sl.s[i];
  const f32x4* src = (const f32x4*)(h_ws + (size_t)i * g.hid);
  f32x4* dst = (f32x4*)(g.h + (size_t)slot * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
  if (threadIdx.x == 0) {
    int* rec = pool_record(g, slot);
    for (int t = 0; t < K; ++t) pool_vote_update(rec, g, argmax[(size_t)i * K + t]);
  }
}

// pool_commit for a ragged burst: the ids of slot i are argmax[off .. off + count) of its table entry (packed rows, the caller's order)
__global__ __launch_bounds__(256) void pool_commit_ragged_kernel(PoolGeom g, PoolSlots sl, RaggedMap rows, const float* __restrict__ h_ws,
                                                                 const int* __restrict__ argmax) {
  const int i = blockIdx.x, slot = sl.s[i];
  const f32x4* src = (const f32x4*)(h_ws + (size_t)i * g.hid);
  f32x4* dst = (f32x4*)(g.h + (size_t)slot * g.hid);
  for (int k = threadIdx.x; k < (g.hid >> 2); k += 256) dst[k] = src[k];
  if (threadIdx.x == 0) {
    int* rec = pool_record(g, slot);
    const unsigned e = rows.e[i];
    const int off = (int)ragged_off(e), K = (int)ragged_count(e);
    for (int t = 0; t < K; ++t) pool_vote_update(rec, g, argmax[off + t]);
  }
}

__global__ __launch_bounds__(64) void pool_vote_kernel(PoolGeom g, PoolSlots sl, int n, const int* __restrict__ ids) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) pool_vote_update(pool_record(g, sl.s[i]), g, ids[i]);
}

// pool_vote for a ragged burst: lane i votes ids[off .. off + count) of its table entry in frame order
__global__ __launch_bounds__(64) void pool_vote_ragged_kernel(PoolGeom g, PoolSlots sl, RaggedMap rows, int n, const int* __restrict__ ids) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int* rec = pool_record(g, sl.s[i]);
  const unsigned e = rows.e[i];
  const int off = (int)ragged_off(e), K = (int)ragged_count(e);
  for (int t = 0; t < K; ++t) pool_vote_update(rec, g, ids[off + t]);
}

__global__ __launch_bounds__(64) void pool_flush_kernel(PoolGeom g, PoolSlots sl, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int* rec = pool_record(g, sl.s[i]);
  const int frames = rec[0], rest = frames % g.window;
  if (rest == 0) return;
  const unsigned* counts = (const unsigned*)(rec + kPoolRecHeader);
  unsigned any = 0u;
  for (int c = 0; c < g.ncls; ++c) any |= counts[c];
  if (any) pool_close_window(rec, g, frames - rest);         // a second flush finds the counts cleared and votes nothing
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

int launch_pool_commit(const PoolGeom& g, const int* slots, int n, const float* h_ws, const int* argmax, hipStream_t s) {
  PoolSlots sl;
  if (!h_ws || !argmax || !pool_slots(g, slots, n, &sl)) return -1;
  pool_commit_kernel<<<n, 256, 0, s>>>(g, sl, h_ws, argmax);
  return 0;
}

int launch_pool_commit_frames(const PoolGeom& g, const int* slots, int n, int K, const float* h_ws, const int* argmax, hipStream_t s) {
  PoolSlots sl;
  if (!h_ws || !argmax || K < 1 || K > 32 || n * K > kPoolMaxActive || !pool_slots(g, slots, n, &sl)) return -1;
  pool_commit_frames_kernel<<<n, 256, 0, s>>>(g, sl, K, h_ws, argmax);
  return 0;
}

int launch_pool_commit_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const float* h_ws,
                              const int* argmax, hipStream_t s) {
  PoolSlots sl;
  if (!h_ws || !argmax || n_rows < n || n_rows > kPoolMaxActive || !pool_slots(g, slots, n, &sl)) return -1;
  for (int i = 0; i < n; ++i)
    if (ragged_count(rows.e[i]) < 1u || ragged_count(rows.e[i]) > 32u || ragged_off(rows.e[i]) + ragged_count(rows.e[i]) > (unsigned)n_rows) return -1;
  pool_commit_ragged_kernel<<<n, 256, 0, s>>>(g, sl, rows, h_ws, argmax);
  return 0;
}

int launch_pool_vote(const PoolGeom& g, const int* slots, int n, const int* ids, hipStream_t s) {
  PoolSlots sl;
  if (!ids || !pool_slots(g, slots, n, &sl)) return -1;
  pool_vote_kernel<<<(n + 63) / 64, 64, 0, s>>>(g, sl, n, ids);
  return 0;
}

int launch_pool_vote_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const int* ids, hipStream_t s) {
  PoolSlots sl;
  if (!ids || n_rows < n || n_rows > kPoolMaxActive || !pool_slots(g, slots, n, &sl)) return -1;
  for (int i = 0; i < n; ++i)
    if (ragged_count(rows.e[i]) < 1u || ragged_count(rows.e[i]) > 32u || ragged_off(rows.e[i]) + ragged_count(rows.e[i]) > (unsigned)n_rows) return -1;
  pool_vote_ragged_kernel<<<(n + 63) / 64, 64, 0, s>>>(g, sl, rows, n, ids);
  return 0;
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
