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
// The two kernels differ in where a query comes from: flat sequences (the offline entry), or the entries of a feed report with the
// history in the slot's vote record.  No float, no global atomic; the model, the pool and the report are only read.  A garbage word in
// the caller's blocks sends no lane out of bounds: positions, counts and ids are clamped or skipped.
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

// One wave, one item; `live` false: a wave without an item in this trip, it only keeps the workgroup's barriers company.  hist: the
// wave's own kProcHist counters.  Every wave of the workgroup calls this the same number of times.
__device__ __forceinline__ void proc_judge_item(const ProcGeom& m, const ProcQuery& q, bool live, int* __restrict__ hist,
                                                int* __restrict__ out) {
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

namespace {
bool proc_geom_ok(const ProcGeom& m) {
  return m.goff && m.ex && m.sym && m.ncls >= 1 && m.ncls <= kProcMaxClasses && m.order >= 1 && m.order <= kProcMaxOrder && m.n_groups >= 0 &&
         m.n_examples >= 0 && m.n_sym >= 0 && m.num >= 0 && m.num <= m.den && m.den >= 1 && m.den <= kProcMaxDen;
}
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
  if (!proc_geom_ok(m) || !g.rec || g.capacity < 1 || g.max_events < 1 || (g.rec_words & 3) || max_out < 1 || !report ||
      ((uintptr_t)report & 15) || !slot_groups || !verdicts || ((uintptr_t)verdicts & 15))
    return -1;
  feed_judge_kernel<<<proc_grid(max_out), kProcWaves * 64, 0, s>>>(m, g, max_out, report, slot_groups, verdicts);
  return 0;
}
