// Event feed of a stream pool (prego_stream_pool_feed_*; host side: stream_feed.cpp): one drain scans the vote record of EVERY slot
// (stream_pool.hip: [2] n_events, [3] overflow, the event arrays) and writes each event appended since the previous drain into one small
// report, ascending slot, then ascending index.  The pool's block is only read; what the feed remembers lives in its own block:
//   cursor [capacity]   bits 0..29 the slot's events already delivered, bits 30..31 the overflow bits already reported
//   seq                 drains so far
//   wg_due [workgroups] entries due per workgroup of the current drain
// Report (int32): count | pending | seq | 0, then max_out entries slot | index | step id | first frame, each one 16-byte store.  A slot's
// newly set overflow bits are one entry slot | -1 | bits | frames, in front of the slot's events (-1 is the lowest index).
//   feed_count   workgroup b: the entries due in slots [256 b, 256 b + 256) -> wg_due[b]              (not launched for one workgroup)
//   feed_write   workgroup b: base = sum of wg_due[0 .. b), an exclusive scan of its 256 lanes' due counts on top of it, every lane
//                writes its slot's entries at its offset while they are below max_out and moves its cursor past what it wrote; the
//                last workgroup writes the header
//   feed_forget  cursor[slots[i]] <- 0
// The order is a function of the slot number alone: no atomic decides a position and no workgroup waits for another - the second launch
// starts when the first has ended.  One lane per slot: a slot with many events due (the first drain after a long silence) is written by
// its lane alone.  The scan: a wave64 inclusive scan by __shfl_up (6 steps, no LDS), the four wave totals through 16 bytes of LDS.
#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {
constexpr unsigned kFeedCountMask = 0x3fffffffu;
constexpr int kFeedRepShift = 30;

// what is due for one slot: the cursor as it stands after the reset rule, the clamped n_events and the overflow bits not yet reported
struct SlotDue { unsigned old_cur; int delivered, rep, n, fresh, frames, due; };

__device__ __forceinline__ SlotDue feed_slot_due(const PoolGeom& g, const int* __restrict__ cursor, int slot) {
  SlotDue d{0u, 0, 0, 0, 0, 0, 0};
  if (slot >= g.capacity) return d;
  const i32x4 hdr = *(const i32x4*)(g.rec + (size_t)slot * g.rec_words);       // frames | last vote + 1 | n_events | overflow
  d.old_cur = (unsigned)cursor[slot];
  d.delivered = (int)(d.old_cur & kFeedCountMask);
  d.rep = (int)(d.old_cur >> kFeedRepShift);
  d.frames = hdr.x;
  d.n = min(max(hdr.z, 0), g.max_events);                    // the block is the caller's: a garbage word sends no lane out of bounds
  const int ov = hdr.w & (kPoolOverflowFull | kPoolOverflowBadId);
  if (d.n < d.delivered || (d.rep & ~ov)) {                  // fewer events than delivered, or a reported bit gone: the record was reset
    d.delivered = 0;
    d.rep = 0;
  }
  d.fresh = ov & ~d.rep;
  d.due = d.n - d.delivered + (d.fresh ? 1 : 0);
  return d;
}

__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// the sum of v over the lanes in front of this one in the workgroup (256 lanes), *total = the sum over all of them
__device__ __forceinline__ int block_exclusive_scan(int v, int* __restrict__ wave_tot, int* total) {
  const int inc = wave_inclusive_scan(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wave_tot[w] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kFeedWg / 64; ++k) {
    const int t = wave_tot[k];
    before += k < w ? t : 0;
    tot += t;
  }
  *total = tot;
  return before + inc - v;
}
}  // namespace

__global__ __launch_bounds__(kFeedWg) void feed_count_kernel(PoolGeom g, FeedGeom f) {
  __shared__ int wave_tot[kFeedWg / 64];
  const SlotDue d = feed_slot_due(g, f.cursor, blockIdx.x * kFeedWg + threadIdx.x);
  int total;
  block_exclusive_scan(d.due, wave_tot, &total);
  if (threadIdx.x == 0) f.wg_due[blockIdx.x] = total;        // at most 256 (max_events + 1) < 2^31
}

__global__ __launch_bounds__(kFeedWg) void feed_write_kernel(PoolGeom g, FeedGeom f, int* __restrict__ report) {
  __shared__ int wave_tot[kFeedWg / 64];
  __shared__ long long base_part[kFeedWg / 64];
  const int slot = blockIdx.x * kFeedWg + threadIdx.x;
  // the entries due in the workgroups in front of this one (64 bits: capacity x (max_events + 1) may pass 2^31)
  long long mine = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += kFeedWg) mine += f.wg_due[k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
  if ((threadIdx.x & 63) == 0) base_part[threadIdx.x >> 6] = mine;
  const SlotDue d = feed_slot_due(g, f.cursor, slot);
  int total;
  const int before = block_exclusive_scan(d.due, wave_tot, &total);           // its barrier publishes base_part as well
  long long base = 0;
#pragma unroll
  for (int k = 0; k < kFeedWg / 64; ++k) base += base_part[k];

  if (slot < g.capacity) {
    const long long at = base + before, room = (long long)f.max_out - at;
    const int w = room >= d.due ? d.due : room > 0 ? (int)room : 0;           // entries of this slot that fit the report
    int delivered = d.delivered, rep = d.rep;
    if (w > 0) {
      i32x4* out = (i32x4*)report + 1 + at;
      const int* ev = g.rec + (size_t)slot * g.rec_words + kPoolRecHeader + g.ncls_pad;
      int k = 0;
      if (d.fresh) {
        out[k++] = (i32x4){slot, -1, d.fresh, d.frames};
        rep |= d.fresh;
      }
      for (; k < w; ++k, ++delivered) out[k] = (i32x4){slot, delivered, ev[delivered], ev[g.max_events + delivered]};      // delivered < n <= max_events
    }
    const unsigned cur = (unsigned)delivered | (unsigned)rep << kFeedRepShift;
    if (cur != d.old_cur) f.cursor[slot] = (int)cur;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const long long all = base + total, count = all < f.max_out ? all : f.max_out, left = all - count;
    const int seq = *f.seq + 1;
    *f.seq = seq;
    *(i32x4*)report = (i32x4){(int)count, left > 0x7fffffffLL ? 0x7fffffff : (int)left, seq, 0};
  }
}

__global__ __launch_bounds__(64) void feed_forget_kernel(FeedGeom f, PoolSlots sl, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) f.cursor[sl.s[i]] = 0;
}

int launch_feed_drain(const PoolGeom& g, const FeedGeom& f, int* report, hipStream_t s) {
  if (!g.rec || !f.cursor || !f.seq || !f.wg_due || !report || g.capacity < 1 || g.max_events < 1 || f.max_out < 1 || (g.rec_words & 3)) return -1;
  const int nwg = (g.capacity + kFeedWg - 1) / kFeedWg;
  if (nwg > 1) feed_count_kernel<<<nwg, kFeedWg, 0, s>>>(g, f);               // one workgroup has nothing in front of it: base = 0
  feed_write_kernel<<<nwg, kFeedWg, 0, s>>>(g, f, report);
  return 0;
}

int launch_feed_forget(const FeedGeom& f, int capacity, const int* slots, int n, hipStream_t s) {
  if (!f.cursor || !slots || n < 1 || n > kPoolMaxActive) return -1;
  PoolSlots sl;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= capacity) return -1;
    sl.s[i] = slots[i];
  }
  for (int i = n; i < kPoolMaxActive; ++i) sl.s[i] = 0;
  feed_forget_kernel<<<(n + 63) / 64, 64, 0, s>>>(f, sl, n);
  return 0;
}
