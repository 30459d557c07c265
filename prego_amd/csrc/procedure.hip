// Procedure model (prego_procedure_*, prego_stream_pool_feed_judge; host side: procedure.cpp): is the step that just came one the corpus
// of correct transcripts has seen after this history?  One wave judges one item against the examples of the item's group:
//   query    cur, its group, and ctx: the last len = min(order, steps in front + 1) symbols in front of cur, newest in byte 0, the virtual
//            START (kProcStart) where the sequence begins; a symbol outside [0, ncls) is kProcNoMatch, equal to nothing in the corpus
//   example  ex[e] = the position in sym of its next symbol; its context is the bytes in front of it, back to its transcript's START
//   match    m(e) = how many trailing symbols of the two contexts are equal, at most len.  START equals only START, and the two STARTs can
//            only meet at the query's last byte, so the compare never runs into the transcript in front
//   j*       the largest m(e) of the group; 0: UNKNOWN.  The examples with m(e) = j* are exactly those that match at j*
//   counts   every lane adds its examples into hist[m(e) - 1][next symbol] (LDS, integer adds: any order gives the same words); row
//            j* - 1 is cnt(.), its sum tot; class c is allowed when cnt(c) > 0 and cnt(c) den >= tot num (64-bit products)
//   verdict  flags | cnt(cur) | tot | group | allowed mask [4], two 16-byte stores by lane 0
//   forecast the same scan over a history that is all context (no cur): row j* - 1 handed out ranked - flags | n_cand | tot | group |
//            allowed mask [4] | the first 8 classes by (count descending, id ascending) | their counts, six 16-byte stores by lane 0
// The kernels differ in where a query comes from: flat sequences (the offline entries), the entries of a feed report with the history
// in the slot's vote record, or a caller's list of slots.  No float, no global atomic; the model, the pool and the report are only read.
// A garbage word in the caller's blocks sends no lane out of bounds: positions, counts and ids are clamped or skipped.
#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {
constexpr int kProcRow = kProcMaxClasses;                    // counters per match length
constexpr int kProcHist = kProcMaxOrder * kProcRow;          // per wave: 4 KB

struct ProcQuery {
  unsigned long long ctx;
  int len, cur, group;
  bool skip;
};

__device__ __forceinline__ unsigned long long proc_symbol(int s, int ncls) {
  return (unsigned)s < (unsigned)ncls ? (unsigned long long)s : (unsigned long long)kProcNoMatch;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
  return v;
}

// The scan both item routines share: one wave, one query.  Zeroes the wave's kProcHist counters, adds every example of the query's group
// into hist[m(e) - 1][next symbol] and returns j* (0: none), the same word in every lane.  `live` false: a wave without an item in this
// trip, it only keeps the workgroup's two barriers company.  Every wave of the workgroup calls this the same number of times.
__device__ __forceinline__ int proc_scan(const ProcGeom& m, const ProcQuery& q, bool live, int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  for (int k = lane; k < m.order * kProcRow; k += 64) hist[k] = 0;
  __syncthreads();
  int best = 0;
  if (live && !q.skip) {
    int lo = 0, hi = 0;
    if (q.group == -1) {
      hi = m.n_examples;
    } else if (q.group >= 0 && q.group < m.n_groups) {
      lo = max(m.goff[q.group], 0);
      hi = min(m.goff[q.group + 1], m.n_examples);
    }
    for (int e = lo + lane; e < hi; e += 64) {
      const int pos = m.ex[e];
      if (pos < 1 || pos >= m.n_sym) continue;
      const int lim = min(q.len, pos);
      unsigned long long have = 0;
#pragma unroll
      for (int k = 0; k < kProcMaxOrder; ++k)
        if (k < lim) have |= (unsigned long long)m.sym[pos - 1 - k] << (8 * k);
      unsigned long long diff = have ^ q.ctx;
      if (lim < kProcMaxOrder) diff |= ~0ull << (8 * lim);
      const int mlen = diff ? __builtin_ctzll(diff) >> 3 : kProcMaxOrder;
      const int next = m.sym[pos];
      if (mlen > 0 && next < kProcRow) {
        atomicAdd(&hist[(mlen - 1) * kProcRow + next], 1);
        best = max(best, mlen);
      }
    }
  }
  best = wave_max(best);
  __syncthreads();
  return best;
}

// One wave, one judged item; hist: the wave's own kProcHist counters
__device__ __forceinline__ void proc_judge_item(const ProcGeom& m, const ProcQuery& q, bool live, int* __restrict__ hist,
                                                int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int best = proc_scan(m, q, live, hist);
  if (!live) return;
  i32x4 head = {kProcSkipped, 0, 0, -1}, mask = {0, 0, 0, 0};
  if (!q.skip) {
    head = (i32x4){kProcJudged | kProcUnknown, 0, 0, q.group};
    if (best > 0) {
      const int* row = hist + (best - 1) * kProcRow;
      const int c0 = row[lane], c1 = row[lane + 64];
      const int tot = wave_sum(c0 + c1);
      const long long need = (long long)tot * m.num;
      const unsigned long long m0 = __ballot(c0 > 0 && (long long)c0 * m.den >= need);
      const unsigned long long m1 = __ballot(c1 > 0 && (long long)c1 * m.den >= need);
      const bool in = (unsigned)q.cur < (unsigned)kProcRow;
      const int cnt = in ? row[q.cur] : 0;
      const bool ok = in && (((q.cur < 64 ? m0 >> q.cur : m1 >> (q.cur - 64)) & 1ull) != 0);
      head = (i32x4){kProcJudged | (ok ? 0 : kProcMistake) | best << kProcJstarShift, cnt, tot, q.group};
      mask = (i32x4){(int)(unsigned)m0, (int)(unsigned)(m0 >> 32), (int)(unsigned)m1, (int)(unsigned)(m1 >> 32)};
    }
  }
  if (lane == 0) {
    ((i32x4*)out)[0] = head;
    ((i32x4*)out)[1] = mask;
  }
}

// One wave, one forecast: q holds the whole history as context (q.cur is not read).  After the scan lane l holds row[l] and row[l + 64]
// of row j* - 1; eight rounds of a wave maximum over cnt << 7 | (127 - id) - cnt <= 2^24, so the key needs all 32 bits unsigned - pick
// the ranked classes, count descending and equal counts by ascending id, and the winner's lane clears its entry.  0 is no candidate.
__device__ __forceinline__ void proc_forecast_item(const ProcGeom& m, const ProcQuery& q, bool live, int* __restrict__ hist,
                                                   int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int best = proc_scan(m, q, live, hist);
  if (!live) return;
  i32x4 head = {kProcSkipped, 0, 0, -1}, mask = {0, 0, 0, 0};
  int id[kProcRanks], cnt[kProcRanks];
#pragma unroll
  for (int r = 0; r < kProcRanks; ++r) id[r] = -1, cnt[r] = 0;
  if (!q.skip) {
    head = (i32x4){kProcMade | kProcUnknown, 0, 0, q.group};
    if (best > 0) {
      const int* row = hist + (best - 1) * kProcRow;
      const int c0 = row[lane], c1 = row[lane + 64];
      const int tot = wave_sum(c0 + c1);
      const long long need = (long long)tot * m.num;
      const unsigned long long m0 = __ballot(c0 > 0 && (long long)c0 * m.den >= need);
      const unsigned long long m1 = __ballot(c1 > 0 && (long long)c1 * m.den >= need);
      const int n_cand = __popcll(__ballot(c0 > 0)) + __popcll(__ballot(c1 > 0));
      unsigned k0 = c0 > 0 ? (unsigned)c0 << 7 | (unsigned)(127 - lane) : 0u;
      unsigned k1 = c1 > 0 ? (unsigned)c1 << 7 | (unsigned)(63 - lane) : 0u;
#pragma unroll
      for (int r = 0; r < kProcRanks; ++r) {
        const unsigned top = wave_umax(max(k0, k1));
        if (top) {
          id[r] = 127 - (int)(top & 127u);
          cnt[r] = (int)(top >> 7);
          if (id[r] == lane) k0 = 0u;
          if (id[r] == lane + 64) k1 = 0u;
        }
      }
      head = (i32x4){kProcMade | best << kProcJstarShift | min(n_cand, kProcRanks) << kProcRankedShift, n_cand, tot, q.group};
      mask = (i32x4){(int)(unsigned)m0, (int)(unsigned)(m0 >> 32), (int)(unsigned)m1, (int)(unsigned)(m1 >> 32)};
    }
  }
  if (lane == 0) {
    ((i32x4*)out)[0] = head;
    ((i32x4*)out)[1] = mask;
    ((i32x4*)out)[2] = (i32x4){id[0], id[1], id[2], id[3]};
    ((i32x4*)out)[3] = (i32x4){id[4], id[5], id[6], id[7]};
    ((i32x4*)out)[4] = (i32x4){cnt[0], cnt[1], cnt[2], cnt[3]};
    ((i32x4*)out)[5] = (i32x4){cnt[4], cnt[5], cnt[6], cnt[7]};
  }
}

// the query of a history h[0 .. n - 1], all of it context: byte k is h[n - 1 - k], START behind the oldest step
template <class At>
__device__ __forceinline__ void proc_history_query(const ProcGeom& m, int n, At at, ProcQuery& q) {
  q.len = min(m.order, n + 1);
  for (int k = 0; k < q.len; ++k) q.ctx |= (k < n ? proc_symbol(at(n - 1 - k), m.ncls) : (unsigned long long)kProcStart) << (8 * k);
}
}  // namespace

// item t = position t of the flat symbols; its sequence is found by bisection of offsets
__global__ __launch_bounds__(kProcWaves * 64) void procedure_judge_kernel(ProcGeom m, int n_seq, int n_pos,
                                                                          const int* __restrict__ offsets, const int* __restrict__ symbols,
                                                                          const int* __restrict__ groups, int* __restrict__ verdicts) {
  __shared__ int hist[kProcWaves][kProcHist];
  const int w = threadIdx.x >> 6;
  for (int base = blockIdx.x * kProcWaves; base < n_pos; base += gridDim.x * kProcWaves) {
    const int t = base + w;
    const bool live = t < n_pos;
    ProcQuery q{0ull, 0, 0, -1, false};
    if (live) {
      int lo = 0, hi = n_seq - 1;                              // the last sequence that starts at or in front of t
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= t) lo = mid; else hi = mid - 1;
      }
      const int front = t - min(max(offsets[lo], 0), t);       // steps of the sequence in front of t
      q.cur = symbols[t];
      q.group = groups[lo];
      q.len = min(m.order, front + 1);
      for (int k = 0; k < q.len; ++k) q.ctx |= (k < front ? proc_symbol(symbols[t - 1 - k], m.ncls) : (unsigned long long)kProcStart) << (8 * k);
    }
    proc_judge_item(m, q, live, hist[w], verdicts + (size_t)(live ? t : 0) * kProcVerdictWords);
  }
}

// item e = entry e of the report; the history is event_id[.. index - 1] of the entry's slot
__global__ __launch_bounds__(kProcWaves * 64) void feed_judge_kernel(ProcGeom m, PoolGeom g, int max_out, const int* __restrict__ report,
                                                                     const int* __restrict__ slot_groups, int* __restrict__ verdicts) {
  __shared__ int hist[kProcWaves][kProcHist];
  const int w = threadIdx.x >> 6;
  const int count = min(max(report[0], 0), max_out);
  for (int base = blockIdx.x * kProcWaves; base < count; base += gridDim.x * kProcWaves) {
    const int e = base + w;
    const bool live = e < count;
    ProcQuery q{0ull, 0, 0, -1, true};
    if (live) {
      const i32x4 ent = ((const i32x4*)report)[1 + e];          // slot | index | step id | first frame
      const int slot = ent.x, index = ent.y;
      if ((unsigned)slot < (unsigned)g.capacity && index >= 0) {
        const int* rec = g.rec + (size_t)slot * g.rec_words;
        if (index < min(max(rec[2], 0), g.max_events)) {
          const int* ev = rec + kPoolRecHeader + g.ncls_pad;
          q.skip = false;
          q.cur = ent.z;
          q.group = slot_groups[slot];
          q.len = min(m.order, index + 1);
          for (int k = 0; k < q.len; ++k) q.ctx |= (k < index ? proc_symbol(ev[index - 1 - k], m.ncls) : (unsigned long long)kProcStart) << (8 * k);
        }
      }
    }
    proc_judge_item(m, q, live, hist[w], verdicts + (size_t)(live ? e : 0) * kProcVerdictWords);
  }
}

// item r = row offsets[s] + s + p: the forecast after the first p symbols of sequence s, found by bisection of offsets[s] + s
__global__ __launch_bounds__(kProcWaves * 64) void procedure_forecast_kernel(ProcGeom m, int n_seq, int n_pos, const int* __restrict__ offsets,
                                                                             const int* __restrict__ symbols, const int* __restrict__ groups,
                                                                             int* __restrict__ forecasts) {
  __shared__ int hist[kProcWaves][kProcHist];
  const int w = threadIdx.x >> 6;
  const int n_rows = n_pos + n_seq;
  for (int base = blockIdx.x * kProcWaves; base < n_rows; base += gridDim.x * kProcWaves) {
    const int r = base + w;
    const bool live = r < n_rows;
    ProcQuery q{0ull, 0, 0, -1, false};
    if (live) {
      int lo = 0, hi = n_seq - 1;                              // the last sequence whose first row is at or in front of r
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)offsets[mid] + mid <= r) lo = mid; else hi = mid - 1;
      }
      const int first = min(max(offsets[lo], 0), n_pos);       // of the sequence's symbols; the p in front end inside symbols
      const int p = min(max(r - lo - first, 0), n_pos - first);
      q.group = groups[lo];
      proc_history_query(m, p, [&](int i) { return symbols[first + i]; }, q);
    }
    proc_forecast_item(m, q, live, hist[w], forecasts + (size_t)(live ? r : 0) * kProcForecastWords);
  }
}

// item e = entry e of the report; the history is event_id[.. index - 1] of the entry's slot and the entry's own step id behind it
__global__ __launch_bounds__(kProcWaves * 64) void feed_forecast_kernel(ProcGeom m, PoolGeom g, int max_out, const int* __restrict__ report,
                                                                        const int* __restrict__ slot_groups, int* __restrict__ forecasts) {
  __shared__ int hist[kProcWaves][kProcHist];
  const int w = threadIdx.x >> 6;
  const int count = min(max(report[0], 0), max_out);
  for (int base = blockIdx.x * kProcWaves; base < count; base += gridDim.x * kProcWaves) {
    const int e = base + w;
    const bool live = e < count;
    ProcQuery q{0ull, 0, 0, -1, true};
    if (live) {
      const i32x4 ent = ((const i32x4*)report)[1 + e];          // slot | index | step id | first frame
      const int slot = ent.x, index = ent.y;
      if ((unsigned)slot < (unsigned)g.capacity && index >= 0) {
        const int* rec = g.rec + (size_t)slot * g.rec_words;
        if (index < min(max(rec[2], 0), g.max_events)) {
          const int* ev = rec + kPoolRecHeader + g.ncls_pad;
          q.skip = false;
          q.group = slot_groups[slot];
          proc_history_query(m, index + 1, [&](int i) { return i < index ? ev[i] : ent.z; }, q);
        }
      }
    }
    proc_forecast_item(m, q, live, hist[w], forecasts + (size_t)(live ? e : 0) * kProcForecastWords);
  }
}

// item i = slot slots[i] of the caller's list; the history is every event the slot's record holds
__global__ __launch_bounds__(kProcWaves * 64) void pool_forecast_kernel(ProcGeom m, PoolGeom g, int n, const int* __restrict__ slots,
                                                                        const int* __restrict__ slot_groups, int* __restrict__ forecasts) {
  __shared__ int hist[kProcWaves][kProcHist];
  const int w = threadIdx.x >> 6;
  for (int base = blockIdx.x * kProcWaves; base < n; base += gridDim.x * kProcWaves) {
    const int i = base + w;
    const bool live = i < n;
    ProcQuery q{0ull, 0, 0, -1, true};
    if (live) {
      const int slot = slots[i];
      if ((unsigned)slot < (unsigned)g.capacity) {
        const int* rec = g.rec + (size_t)slot * g.rec_words;
        const int* ev = rec + kPoolRecHeader + g.ncls_pad;
        q.skip = false;
        q.group = slot_groups[slot];
        proc_history_query(m, min(max(rec[2], 0), g.max_events), [&](int k) { return ev[k]; }, q);
      }
    }
    proc_forecast_item(m, q, live, hist[w], forecasts + (size_t)(live ? i : 0) * kProcForecastWords);
  }
}

namespace {
bool proc_geom_ok(const ProcGeom& m) {
  return m.goff && m.ex && m.sym && m.ncls >= 1 && m.ncls <= kProcMaxClasses && m.order >= 1 && m.order <= kProcMaxOrder && m.n_groups >= 0 &&
         m.n_examples >= 0 && m.n_sym >= 0 && m.num >= 0 && m.num <= m.den && m.den >= 1 && m.den <= kProcMaxDen;
}
bool pool_records_ok(const PoolGeom& g) { return g.rec && g.capacity >= 1 && g.max_events >= 1 && !(g.rec_words & 3); }
int proc_grid(int items) { return min((items + kProcWaves - 1) / kProcWaves, kProcMaxGrid); }
}  // namespace

int launch_procedure_judge(const ProcGeom& m, int n_seq, int n_pos, const int* offsets, const int* symbols, const int* groups,
                           int* verdicts, hipStream_t s) {
  if (!proc_geom_ok(m) || n_seq < 1 || n_pos < 1 || !offsets || !symbols || !groups || !verdicts || ((uintptr_t)verdicts & 15)) return -1;
  procedure_judge_kernel<<<proc_grid(n_pos), kProcWaves * 64, 0, s>>>(m, n_seq, n_pos, offsets, symbols, groups, verdicts);
  return 0;
}

int launch_feed_judge(const ProcGeom& m, const PoolGeom& g, int max_out, const int* report, const int* slot_groups, int* verdicts,
                      hipStream_t s) {
  if (!proc_geom_ok(m) || !pool_records_ok(g) || max_out < 1 || !report || ((uintptr_t)report & 15) || !slot_groups || !verdicts ||
      ((uintptr_t)verdicts & 15))
    return -1;
  feed_judge_kernel<<<proc_grid(max_out), kProcWaves * 64, 0, s>>>(m, g, max_out, report, slot_groups, verdicts);
  return 0;
}

int launch_procedure_forecast(const ProcGeom& m, int n_seq, int n_pos, const int* offsets, const int* symbols, const int* groups,
                              int* forecasts, hipStream_t s) {
  if (!proc_geom_ok(m) || n_seq < 1 || n_pos < 0 || n_pos > (1 << 30) || n_seq > (1 << 30) || !offsets || !symbols || !groups || !forecasts ||
      ((uintptr_t)forecasts & 15))
    return -1;
  procedure_forecast_kernel<<<proc_grid(n_pos + n_seq), kProcWaves * 64, 0, s>>>(m, n_seq, n_pos, offsets, symbols, groups, forecasts);
  return 0;
}

int launch_feed_forecast(const ProcGeom& m, const PoolGeom& g, int max_out, const int* report, const int* slot_groups, int* forecasts,
                         hipStream_t s) {
  if (!proc_geom_ok(m) || !pool_records_ok(g) || max_out < 1 || !report || ((uintptr_t)report & 15) || !slot_groups || !forecasts ||
      ((uintptr_t)forecasts & 15))
    return -1;
  feed_forecast_kernel<<<proc_grid(max_out), kProcWaves * 64, 0, s>>>(m, g, max_out, report, slot_groups, forecasts);
  return 0;
}

int launch_pool_forecast(const ProcGeom& m, const PoolGeom& g, int n, const int* slots, const int* slot_groups, int* forecasts, hipStream_t s) {
  if (!proc_geom_ok(m) || !pool_records_ok(g) || n < 1 || n > g.capacity || !slots || !slot_groups || !forecasts || ((uintptr_t)forecasts & 15))
    return -1;
  pool_forecast_kernel<<<proc_grid(n), kProcWaves * 64, 0, s>>>(m, g, n, slots, slot_groups, forecasts);
  return 0;
}
