// A slot's vote record on the device: the update rule of every pool that keeps one (stream_pool.hip: the GRU and Transformer pools'
// commit and vote; decode_pool.hip: the decode pool's committed labels).  The layout is stream_pool.hip's header comment.
#pragma once
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

// the end of a stream: its unfinished window is voted (the reference's shorter last window, aggregate.py:57-58)
__device__ __forceinline__ void pool_flush_window(int* __restrict__ rec, const PoolGeom& g) {
  const int frames = rec[0], rest = frames % g.window;
  if (rest == 0) return;
  const unsigned* counts = (const unsigned*)(rec + kPoolRecHeader);
  unsigned any = 0u;
  for (int c = 0; c < g.ncls; ++c) any |= counts[c];
  if (any) pool_close_window(rec, g, frames - rest);         // a second flush finds the counts cleared and votes nothing
}
}  // namespace
