// Per-frame average precision on the device: step_recognition/utils/metrics.py:25-62 calls
// sklearn.metrics.average_precision_score once per class on the [frames x classes] score matrix of an eval pass (main.py:101 runs
// that after every epoch).  The definition (sklearn: precision_recall_curve + step-wise sum): a class's thresholds are its DISTINCT
// score values in descending order (ties share one threshold); with tps_k / cnt_k = positives / samples at or above threshold k and
// P positives in all,   AP = sum_k (tps_k - tps_{k-1}) / P * tps_k / cnt_k.
//
// Only thresholds that hold a positive contribute, so only the POSITIVES need ranks (round 5; rounds 2-4 sorted every one of the
// frames x classes pairs: four radix passes of scattered 8-byte stores, 18-25 ms for the eval set - the tail of `Evaluate`):
//   ap_extract   one pass over scores / targets [frames][classes] (row-major, as the head kernel writes them): every score becomes a
//                32-bit order-reversing key (ascending key = descending score), written class-major (column c = n keys in a row);
//                the keys of a class's positives are appended to that class's list (order irrelevant: the list is sorted next)
//   ap32_hist / ap32_scan / ap32_scatter   four stable LSD radix passes over 8-bit digits, one segment per class of ITS OWN length
//                P_c (read from the device: nothing returns to the host) -> q_c[0 .. P_c) ascending.  One wave per 4096-key tile.
//   ap_count     for every key k of column c: b = lower_bound(q_c, k) = the first positive at or below this score; cnt_c[b] += 1
//                unless b = P_c (a score below every positive is at or above no threshold).  A workgroup owns a range of q_c and
//                its counters in LDS and streams a slice of the column (comment at the kernel; multi-label targets with more
//                positives than 16 workgroups hold fall back to a sampled table + one device atomic per key).
//                samples at or above positive i's score = cnt_c[0] + ... + cnt_c[i]   (lower_bound never returns the inside of a
//                tie run, so the inclusive prefix is the same for every member of the run)
//   ap_walk<ApWalk>   one workgroup per class walks q_c and cnt_c once: running prefix of cnt, run ends of q, fp64 accumulation of
//                (positives in the run) * (positives so far) / (samples so far).
// Exact integer ranks; the only floating-point work is the final fp64 sum (differs from sklearn's by summation order, ~1e-16) and
// the per-class score mass (fixed summation order: the same bits on every run).
// The kernels up to ap_count are templates over what a list holds per positive: the key (AP), or the key above the frame index (the
// calibrated metric further down, which ranks frames of equal score in frame order).
// One of each: wg_scan_step / wg_scan_array (every workgroup scan), ap_walk_kernel (the walk over a class's list: per-frame and
// per-stage, AP and cAP are four policies of it), ps_run_edges (label runs), ApLayout (the workspace).
#include "common.h"
#include "kernels.h"
#include "wg_scan.h"     // wg_scan_step / wg_scan_array

#define AP_TILE 4096          // keys per radix tile (one wave, 64 steps of 64)
#define AP_RADIX 256
#define AP_PASSES 4           // 32-bit keys, 8-bit digits
#define AP_TGRID 128          // radix tiles of a class are walked by at most this many workgroups
#define AP_XF 128             // ap_extract: frames per tile
#define AP_XC 96              // ap_extract: classes per tile (column blocks of wider matrices)
#define AP_TAB 16384          // ap_count: LDS words (64 KB: two 1024-thread workgroups per CU)
#define AP_OWN (AP_TAB / 2)   // ap_count: positives a workgroup owns (their keys + their counters in LDS)
#define AP_SPLITS_MAX 64      // ap_count: workgroups per class
#define PS_STAGES 10          // per-stage metric: tenths of an action
#define PS_BLK 1024           // per-stage metric: frames per block of the run scans (256 threads x 4)

// order-reversing key of a float score: larger score -> smaller key; -0.0 == +0.0 (sklearn compares values, not bits)
__device__ __forceinline__ unsigned ap_desc_key(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned b = __float_as_uint(s);
  const unsigned asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);     // ascending-order key of an IEEE float
  return ~asc;
}
__device__ __forceinline__ float ap_key_score(unsigned k) {
  const unsigned asc = ~k;
  const unsigned b = (asc & 0x80000000u) ? (asc & 0x7FFFFFFFu) : ~asc;
  return __uint_as_float(b);
}

// the order of a class's list: by key alone (unsigned), or by key and then by frame (64 bits: the key above the frame index, n < 2^31)
typedef unsigned long long ap_u64;
template <typename T> __device__ __forceinline__ T ap_entry(unsigned key, long long frame);
template <> __device__ __forceinline__ unsigned ap_entry<unsigned>(unsigned key, long long) { return key; }
template <> __device__ __forceinline__ ap_u64 ap_entry<ap_u64>(unsigned key, long long frame) { return ((ap_u64)key << 32) | (ap_u64)(unsigned)frame; }

// [AP_XF frames] x [<= AP_XC classes] tile: keys written class-major through an LDS transpose, positives appended per class
// LABELS: the positives are given as one class id per frame (one-hot targets the feeder reduced on the host: 4 bytes per frame over
// the link instead of 4 x classes); a frame whose id is outside [0, C) has no positive
// T: what a class's list holds per positive - the key (AP: ties share a threshold) or the (key, frame) composite (cAP: ties in frame order)
template <bool LABELS, typename T>
__global__ __launch_bounds__(256) void ap_extract_kernel(const float* __restrict__ scores, const float* __restrict__ target,
                                                         const int* __restrict__ labels, long long n, int C, unsigned* __restrict__ keys,
                                                         T* __restrict__ pos, unsigned* __restrict__ cursor) {
  __shared__ unsigned tile[AP_XC][AP_XF + 1];
  __shared__ unsigned lcnt[AP_XC], lbase[AP_XC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long f0 = (long long)blockIdx.x * AP_XF;
  const int c0 = blockIdx.y * AP_XC;
  const int cb = min(AP_XC, C - c0);
  const int nf = (int)min((long long)AP_XF, n - f0);
  if (tid < AP_XC) lcnt[tid] = 0u;
  __syncthreads();
  const int total = nf * cb;
  for (int idx = tid; idx < total; idx += 256) {
    const int f = idx / cb, c = idx - f * cb;
    const size_t g = (size_t)(f0 + f) * C + c0 + c;
    tile[c][f] = ap_desc_key(scores[g]);
    const bool positive = LABELS ? labels[f0 + f] == c0 + c : target[g] != 0.f;
    if (positive) atomicAdd(&lcnt[c], 1u);
  }
  __syncthreads();
  if (tid < cb) {
    const unsigned m = lcnt[tid];
    lbase[tid] = m ? atomicAdd(&cursor[c0 + tid], m) : 0u;
    lcnt[tid] = 0u;
  }
  __syncthreads();
  for (int idx = tid; idx < total; idx += 256) {
    const int f = idx / cb, c = idx - f * cb;
    const bool positive = LABELS ? labels[f0 + f] == c0 + c : target[(size_t)(f0 + f) * C + c0 + c] != 0.f;
    if (positive)
      pos[(size_t)(c0 + c) * n + lbase[c] + atomicAdd(&lcnt[c], 1u)] = ap_entry<T>(tile[c][f], f0 + f);
  }
  for (int c = wave; c < cb; c += 4) {
    unsigned* col = keys + (size_t)(c0 + c) * n + f0;
    for (int f = lane; f < nf; f += 64) col[f] = tile[c][f];
  }
}

// digit histogram of a class's tiles: hist[c][digit][tile] with the class's own tile count as the stride; the first pass also
// clears the class's counters for ap_count
template <typename T>
__global__ __launch_bounds__(64) void ap32_hist_kernel(const T* __restrict__ keys, const unsigned* __restrict__ len, long long n,
                                                       int ntiles_max, int shift, unsigned* __restrict__ hist, unsigned* __restrict__ zero) {
  __shared__ unsigned h[AP_RADIX];
  const int c = blockIdx.y, lane = threadIdx.x;
  const unsigned P = len[c];
  const int ntc = (int)((P + AP_TILE - 1) / AP_TILE);
  const T* col = keys + (size_t)c * n;
  unsigned* hc = hist + (size_t)c * AP_RADIX * ntiles_max;
  for (int tile = blockIdx.x; tile < ntc; tile += gridDim.x) {
    for (int d = lane; d < AP_RADIX; d += 64) h[d] = 0u;
    __syncthreads();
    const unsigned i0 = (unsigned)tile * AP_TILE;
    for (int j = lane; j < AP_TILE; j += 64) {
      const unsigned i = i0 + j;
      if (i < P) {
        atomicAdd(&h[(unsigned)(col[i] >> shift) & (AP_RADIX - 1)], 1u);
        if (zero) zero[(size_t)c * n + i] = 0u;
      }
    }
    __syncthreads();
    for (int d = lane; d < AP_RADIX; d += 64) hc[(size_t)d * ntc + tile] = h[d];
    __syncthreads();
  }
}

// per class: exclusive scan over its (digit, tile) counts in place (digit-major = the order a stable scatter fills the output)
__global__ __launch_bounds__(256) void ap32_scan_kernel(unsigned* __restrict__ hist, const unsigned* __restrict__ len, int ntiles_max) {
  __shared__ unsigned wsum[2][4];
  const int ntc = (int)((len[blockIdx.x] + AP_TILE - 1) / AP_TILE);
  wg_scan_array<ScanSum, false, 4>(hist + (size_t)blockIdx.x * AP_RADIX * ntiles_max, AP_RADIX * ntc, 0u, wsum);
}

// stable scatter of a class's tiles by the current digit
template <typename T>
__global__ __launch_bounds__(64) void ap32_scatter_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                          const unsigned* __restrict__ len, long long n, int ntiles_max, int shift,
                                                          const unsigned* __restrict__ hist) {
  __shared__ unsigned cur[AP_RADIX];
  const int c = blockIdx.y, lane = threadIdx.x;
  const unsigned P = len[c];
  const int ntc = (int)((P + AP_TILE - 1) / AP_TILE);
  const T* col = src + (size_t)c * n;
  T* out = dst + (size_t)c * n;
  const unsigned* hc = hist + (size_t)c * AP_RADIX * ntiles_max;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int tile = blockIdx.x; tile < ntc; tile += gridDim.x) {
    __syncthreads();
    for (int d = lane; d < AP_RADIX; d += 64) cur[d] = hc[(size_t)d * ntc + tile];
    __syncthreads();
    const unsigned i0 = (unsigned)tile * AP_TILE;
    for (int j = 0; j < AP_TILE; j += 64) {
      const unsigned i = i0 + j + lane;
      const bool live = i < P;
      const T k = live ? col[i] : (T)0;
      const unsigned d = (unsigned)(k >> shift) & (AP_RADIX - 1);
      // lanes of this step that hold my digit: AND over the digit's bits of (ballot if my bit is set, else its complement)
      unsigned long long same = __ballot(live);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot(live && ((d >> b) & 1u));
        same &= ((d >> b) & 1u) ? m : ~m;
      }
      const unsigned rank = (unsigned)__popcll(same & below);
      const unsigned base = live ? cur[d] : 0u;
      __syncthreads();                                            // every lane has read its digit's cursor
      if (live) {
        out[base + rank] = k;
        if ((same >> lane) >> 1 == 0ull) cur[d] = base + rank + 1u;   // the highest lane of the group moves the cursor
      }
      __syncthreads();
    }
  }
}

// branch-free lower_bound over t[0 .. m), m >= 1: the first index whose key is >= k (m if none)
template <typename T>
__device__ __forceinline__ unsigned ap_lower_bound(const T* t, unsigned m, T k) {
  unsigned base = 0u, nn = m;
  while (nn > 1u) {
    const unsigned half = nn >> 1;
    base += (t[base + half - 1u] < k) ? half : 0u;
    nn -= half;
  }
  return base + (t[base] < k ? 1u : 0u);
}

// ap_count: the keys of class c against the class's sorted positives q[0 .. P).  Workgroup (x, c) of AP_SPLITS per class.
// * OWNED RANGES (P <= AP_SPLITS * AP_OWN, every eval set of the shipped configs): the positives are cut into Sb = ceil(P / AP_OWN)
//   ranges, the frames into Sf = AP_SPLITS / Sb slices; a workgroup holds ITS range of q and its counters in LDS, streams its slice of
//   the column, keeps the keys whose lower_bound falls into its range (two compares) and counts them with LDS atomics - hot counters
//   (ties, a constant column) cost LDS cycles, not device-wide atomics.  The Sf slices of a range add their counters into cnt behind
//   the loop: P * Sf adds per class instead of one per key (measured: one device atomic per key = 5.6 ms of the eval set's 7.0 with
//   distinct scores, 14.5 of 17.9 with heavy ties).
// * FALLBACK (more positives than that: multi-label targets): every AP_SPLITS-th slice of the column against a table of every sub-th
//   positive + a second search level in the list itself, one device atomic per counted key (equal counters of a wave merged first).
// * T = the (key, frame) composite (cAP): the column's entry i is (keys[i], i) and the list holds composites; every positive is its own
//   lower_bound, so the inclusive prefix of cnt at positive i is its 1-based rank in the stable order.  The same LDS bytes hold
//   fewer 8-byte entries: OWN 5456 instead of 8192, a fallback table of 8192 instead of 16384.
template <typename T> struct ApLds {
  static constexpr unsigned OWN = sizeof(T) == 4 ? AP_OWN : (AP_TAB * 4 / (sizeof(T) + 4)) / 16 * 16;    // entries + their counters
  static constexpr unsigned TAB = AP_TAB * 4 / sizeof(T);                                                // entries alone (fallback)
};
template <typename T>
__global__ __launch_bounds__(1024) void ap_count_kernel(const unsigned* __restrict__ keys, const T* __restrict__ q_all,
                                                        const unsigned* __restrict__ len, long long n, int C, unsigned* __restrict__ cnt_all,
                                                        double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned ap_lds[];
  constexpr unsigned OWN = ApLds<T>::OWN, TABN = ApLds<T>::TAB;
  T* tab = (T*)ap_lds;                                     // OWN entries + OWN counters, or TABN entries (fallback)
  unsigned* lc = (unsigned*)(tab + OWN);
  double* red = (double*)(ap_lds + AP_TAB);                // 16 wave sums
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = gridDim.x;
  const unsigned P = len[c];
  const T* q = q_all + (size_t)c * n;
  unsigned* cnt = cnt_all + (size_t)c * n;
  const unsigned* col = keys + (size_t)c * n;
  const unsigned Sb = (P + OWN - 1) / OWN;
  double ss = 0.0;
  if (Sb <= (unsigned)S) {
    // ---- owned ranges (P = 0: one range of nothing, the score mass only) ----
    const unsigned sbn = Sb ? Sb : 1u;
    const unsigned Sf = (unsigned)S / sbn;
    const unsigned sb = blockIdx.x % sbn, sf = blockIdx.x / sbn;
    if (sf < Sf) {
      const unsigned per = (P + sbn - 1) / sbn;
      const unsigned b0 = min(P, sb * per), b1 = min(P, b0 + per), m = b1 - b0;
      for (unsigned j = tid; j < m; j += 1024) { tab[j] = q[b0 + j]; lc[j] = 0u; }
      const bool open_lo = b0 == 0u;
      const T klo = open_lo ? (T)0 : q[b0 - 1];              // a key belongs here iff klo < k <= khi
      const T khi = m ? q[b1 - 1] : (T)0;
      __syncthreads();
      const long long chunk = (n + Sf - 1) / Sf;
      const long long lo = (long long)sf * chunk, hi = min(n, lo + chunk);
      const bool mass = sb == 0u;                            // one range per slice adds up the scores
      for (long long base = lo; base < hi; base += 4096) {
        T k[4];
        bool mine[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long i = base + e * 1024 + tid;
          const bool live = i < hi;
          const unsigned raw = live ? col[i] : 0xFFFFFFFFu;
          k[e] = ap_entry<T>(raw, i);
          if (live && mass) ss += (double)ap_key_score(raw);
          mine[e] = live && m && (open_lo || k[e] > klo) && k[e] <= khi;
        }
        if (!(mine[0] || mine[1] || mine[2] || mine[3])) continue;
        unsigned bs[4] = {0u, 0u, 0u, 0u}, nn = m;
        while (nn > 1u) {
          const unsigned half = nn >> 1;
#pragma unroll
          for (int e = 0; e < 4; ++e) if (mine[e]) bs[e] += (tab[bs[e] + half - 1u] < k[e]) ? half : 0u;
          nn -= half;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) if (mine[e]) atomicAdd(&lc[bs[e] + (tab[bs[e]] < k[e] ? 1u : 0u)], 1u);
      }
      __syncthreads();
      for (unsigned j = tid; j < m; j += 1024) {
        const unsigned v = lc[j];
        if (v) { if (Sf == 1u) cnt[b0 + j] = v; else atomicAdd(&cnt[b0 + j], v); }
      }
    }
  } else {
    // ---- fallback: one device atomic per counted key ----
    const unsigned sub = (P + TABN - 1) / TABN;              // >= 2 here
    const unsigned m = (P + sub - 1) / sub;                  // table entry j = the LAST key of block j (blocks of `sub` keys)
    for (unsigned j = tid; j < m; j += 1024) { const unsigned long long e = (unsigned long long)(j + 1) * sub - 1; tab[j] = q[e < P ? e : P - 1]; }
    __syncthreads();
    const long long chunk = (n + S - 1) / S;
    const long long lo = (long long)blockIdx.x * chunk, hi = min(n, lo + chunk);
    for (long long base = lo; base < hi; base += 4096) {
      T k[4];
      unsigned b[4];
      bool live[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long i = base + e * 1024 + tid;
        live[e] = i < hi;
        const unsigned raw = live[e] ? col[i] : 0xFFFFFFFFu;
        k[e] = ap_entry<T>(raw, i);
        if (live[e]) ss += (double)ap_key_score(raw);
      }
      {                                                       // four searches in step (same trip count for every lane)
        unsigned bs[4] = {0u, 0u, 0u, 0u}, nn = m;
        while (nn > 1u) {
          const unsigned half = nn >> 1;
#pragma unroll
          for (int e = 0; e < 4; ++e) bs[e] += (tab[bs[e] + half - 1u] < k[e]) ? half : 0u;
          nn -= half;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = bs[e] + (tab[bs[e]] < k[e] ? 1u : 0u);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {                           // second level: inside block b[e] of the list itself
        if (b[e] >= m) { b[e] = P; continue; }
        const unsigned s0 = b[e] * sub, cntk = min(sub, P - s0);
        b[e] = s0 + ap_lower_bound(q + s0, cntk, k[e]);       // < s0 + cntk: the block's last key is >= k
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool todo = live[e] && b[e] < P;
        // equal counters inside the wave first (a constant column, a score above every positive, heavy ties): one add for all of them
        for (int r = 0; r < 2; ++r) {
          const unsigned long long act = __ballot(todo);
          if (act == 0ull) break;
          const int first = __ffsll((long long)act) - 1;
          const unsigned bf = (unsigned)__shfl((int)b[e], first, 64);
          const unsigned long long same = __ballot(todo && b[e] == bf);
          const int ns = __popcll(same);
          if (ns < 8 && r == 0) break;                        // no hot counter in this wave
          if (lane == first) atomicAdd(&cnt[bf], (unsigned)ns);
          if (todo && b[e] == bf) todo = false;
        }
        if (todo) atomicAdd(&cnt[b[e]], 1u);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    for (int w = 0; w < 16; ++w) a += red[w];
    partial[(size_t)blockIdx.x * C + c] = a;
  }
}

#define CAP_EPS 2.220446049250313e-16     // 2^-52, numpy's finfo(float).eps

__device__ __forceinline__ double cap_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// ap_walk: one workgroup over one sorted list and its counters - a class (per frame), or a class and a stage (per stage): AP and the
// calibrated metric, each per frame and per stage (the two sections further down say what they compute), are four policies of it.
// The workgroup walks [0, P) in chunks of 1024, four consecutive elements per thread, and keeps for element i
//   seen   the inclusive prefix of cnt_c: the column's entries at or above q_i (AP), the rank of positive i among all frames (cAP)
//   hits   the set's positives among q_0 .. q_i: i + 1, or (STAGE) the inclusive prefix of st_cs
//   fps    = seen - (i + 1): the class's negatives at or above q_i, which are every stage's negatives too
// A policy says: STAGE; TIES - one term per tie run of q_c that holds d > 0 positives of the set, formed at the run's end against the
// exclusive max-scan of `hits` at the earlier run ends (AP) - or one term per member (cAP: its lists are tie-free); term(); empty(),
// what a list or a set without a positive scores.  A thread adds its terms in index order, then the 64-lane tree, then
// (w0 + w1) + (w2 + w3): a fixed order, the same bits on every run.
struct ApTerm {      // (positives in the run) * (positives so far) / (samples so far)
  static constexpr bool TIES = true;
  static __device__ __forceinline__ double term(long long d, long long hits, long long fps, double) {
    return (double)d * ((double)hits / (double)(fps + hits));
  }
};
struct CapTerm {     // tps / (tps + fps / (w + eps) + eps), wd = w + eps
  static constexpr bool TIES = false;
  static __device__ __forceinline__ double term(long long, long long hits, long long fps, double wd) {
    const double tps = (double)hits;
    return tps / (tps + (double)fps / wd + CAP_EPS);
  }
};
template <typename TERM, bool STAGE_, bool EMPTY_NAN>
struct WalkPolicy : TERM {
  static constexpr bool STAGE = STAGE_;
  static __device__ __forceinline__ double empty() { return EMPTY_NAN ? cap_nan() : 0.0; }
};
typedef WalkPolicy<ApTerm, false, true> ApWalk;       // per-frame AP: NaN for a class without positives
typedef WalkPolicy<CapTerm, false, true> CapWalk;     // per-frame cAP: the same
typedef WalkPolicy<ApTerm, true, false> PsWalk;       // per-stage AP: a class without a run scores 0.0, as the reference reports it
typedef WalkPolicy<CapTerm, true, true> CpsWalk;      // per-stage cAP: no member: NaN, as the host form

// grid (C) or, STAGE, (C, PS_STAGES); q_all: TIES only; st_all / off: STAGE only; partial / splits / score_sum: the per-frame entries
template <typename POL>
__global__ __launch_bounds__(256) void ap_walk_kernel(const unsigned* __restrict__ q_all, const unsigned* __restrict__ cnt_all,
                                                      const unsigned* __restrict__ len, long long n, int C, const unsigned* __restrict__ st_all,
                                                      const int* __restrict__ off, const double* __restrict__ partial, int splits,
                                                      double* __restrict__ ap, long long* __restrict__ n_pos, double* __restrict__ score_sum) {
  constexpr bool STAGE = POL::STAGE, TIES = POL::TIES;
  __shared__ long long ws_cnt[2][4], ws_st[2][4], ws_end[2][4];
  __shared__ double w_acc[4];
  const int c = blockIdx.x, sg = blockIdx.y;
  const long long P = (long long)len[c];
  const unsigned* q = TIES ? q_all + (size_t)c * n : nullptr;
  const unsigned* cnt = cnt_all + (size_t)c * n;
  const unsigned* st = STAGE ? st_all + (size_t)sg * n + (size_t)off[c] : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long members = P;                                    // cAP: w = (n - P) / members is needed before the first term
  if constexpr (STAGE && !TIES) {                           // so the stage's members are counted in a pre-step
    long long ms = 0;
    for (long long j = tid; j < P; j += 256) ms += (long long)st[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ms += __shfl_xor(ms, o, 64);
    if (lane == 0) ws_st[0][wave] = ms;
    __syncthreads();
    members = (ws_st[0][0] + ws_st[0][1]) + (ws_st[0][2] + ws_st[0][3]);
    __syncthreads();
  }
  const double wd = (double)(n - P) / (double)members + CAP_EPS;       // no member: no term is formed
  long long c_cnt = 0, c_st = 0, c_end = 0;                 // the scans' carries
  double acc = 0.0;
  int parity = 0;
  for (long long base = 0; base < P; base += 1024, parity ^= 1) {
    const long long j = base + (long long)tid * 4;
    unsigned k[5] = {0u, 0u, 0u, 0u, 0u};                   // k[4]: the neighbour behind my last element
    long long v[4], u[4], mine = 0, mine_st = 0;
    if constexpr (TIES) {
#pragma unroll
      for (int e = 0; e < 5; ++e) k[e] = j + e < P ? q[j + e] : 0u;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = j + e < P ? (long long)cnt[j + e] : 0;
      u[e] = STAGE && j + e < P ? (long long)st[j + e] : 0;
      mine += v[e];
      mine_st += u[e];
    }
    long long seen = wg_scan_step<ScanSum>(mine, c_cnt, ws_cnt, parity), hits = j;       // in front of my first element
    if constexpr (STAGE) hits = wg_scan_step<ScanSum>(mine_st, c_st, ws_st, parity);
    long long fps[4], h[4], end_local = 0;                  // end_local: hits at my last run end (0 = none: hits is monotone)
    bool act[4];                                            // forms a term: a run end (TIES) or a member
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      seen += v[e];
      hits += STAGE ? u[e] : 1;
      fps[e] = seen - (j + e + 1);
      h[e] = hits;
      if (TIES) {
        act[e] = (j + e < P) && ((j + e + 1 >= P) || (k[e] != k[e + 1]));       // the last positive ends a run
        if (act[e]) end_local = hits;
      } else {
        act[e] = STAGE ? u[e] != 0 : j + e < P;
      }
    }
    long long prev = 0;                                     // hits at the most recent run end before my first element
    if constexpr (TIES) prev = wg_scan_step<ScanMax>(end_local, c_end, ws_end, parity);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (act[e]) {
        const long long d = h[e] - prev;                    // the set's positives in this tie run
        if (!TIES || d > 0) {
          acc += POL::term(d, h[e], fps[e], wd);
          prev = h[e];
        }
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) w_acc[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const long long m = STAGE ? c_st : P;                   // the set's positives
    const size_t at = (size_t)sg * C + c;
    const double a = (w_acc[0] + w_acc[1]) + (w_acc[2] + w_acc[3]);
    ap[at] = m > 0 ? a / (double)m : POL::empty();
    if (n_pos) n_pos[at] = m;
    if constexpr (!STAGE) {
      if (score_sum) {
        double t = 0.0;
        for (int sp = 0; sp < splits; ++sp) t += partial[(size_t)sp * C + c];
        score_sum[c] = t;
      }
    }
  }
}

// ================================================================================================================================
// Calibrated average precision (step_recognition/utils/metrics.py:10-22, metric 'cAP'): the order is descending score and, inside a
// run of equal scores, ascending frame index (the host form's stable sort; the reference's unstable argsort leaves ties to chance).
// The same pipeline over (key, frame) composites: ap_extract<.., ap_u64> appends (key << 32 | frame) per positive, the radix passes
// run over the frame's digits (as many as n - 1 has) and then the key's four, ap_count<ap_u64> counts every (key, frame) of the column
// against the list.  Composites are distinct, so a positive is its own lower_bound and the inclusive prefix of cnt at positive i is
// rank_i, its 1-based position among all n frames.  With tps = i + 1, fps = rank_i - tps, w = (n - P) / P, eps = 2^-52:
//   cAP = (1 / P) * sum_i tps / (tps + fps / (w + eps) + eps)
//   ap_walk<CapWalk>   one workgroup per class: running prefix of cnt, one term per positive.
// ================================================================================================================================

// n_frames == 0: NaN, no positives, no score mass
__global__ void cap_empty_kernel(int C, double* __restrict__ ap, long long* __restrict__ n_pos, double* __restrict__ score_sum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  ap[c] = cap_nan();
  if (n_pos) n_pos[c] = 0;
  if (score_sum) score_sum[c] = 0.0;
}

static int ap_splits(int C) {
  int s = 1024 / C;                      // workgroups per class: 16 (owned ranges up to 131 072 positives per class) or, for few classes, enough to fill the chip
  return s < 16 ? 16 : (s > AP_SPLITS_MAX ? AP_SPLITS_MAX : s);
}

// The workspace of an entry, carved once: the four *_workspace_bytes functions return its totals, the launches take their pointers
// from it.  T: what a list holds per positive (the calibrated metric's 8-byte composites; 8 more bytes align them behind the keys).
// The per-stage buffers lie behind the per-frame workspace, rounded up to 16 bytes.
template <typename T>
struct ApLayout {
  int ntiles, nblk;                      // radix tiles of n keys; 1024-frame blocks of the run scans
  unsigned* keys;                        // [C][n] order-reversing keys, class-major
  T *p0, *p1;                            // [C][n] each: the lists, and where a radix pass scatters them
  unsigned *cnt, *hist, *cursor;         // [C][n] ap_count's counters; [C][256][ntiles]; [C] positives per class
  double* partial;                       // [AP_SPLITS_MAX][C] score mass
  unsigned* st;                          // [PS_STAGES][n] stage counters, the classes back to back
  int *off, *bl_head, *bl_tail;          // [C] where a class's stage counters start; [nblk] each: the run scans' block carries
  size_t frame_bytes, stage_bytes;       // what a per-frame / a per-stage entry needs

  ApLayout(void* ws, long long n, int C) : ntiles((int)((n + AP_TILE - 1) / AP_TILE)), nblk((int)((n + PS_BLK - 1) / PS_BLK)) {
    const size_t cn = (size_t)C * (size_t)n;
    at = (uintptr_t)ws;
    keys = take<unsigned>(cn);
    p0 = take<T>(2 * cn);
    p1 = p0 + cn;
    cnt = take<unsigned>(cn);
    hist = take<unsigned>((size_t)C * AP_RADIX * (size_t)ntiles);
    cursor = take<unsigned>((size_t)C);
    partial = take<double>((size_t)AP_SPLITS_MAX * C);
    frame_bytes = bytes + 1024;
    bytes = (frame_bytes + 15) & ~(size_t)15;
    at = (uintptr_t)ws + bytes;
    st = take<unsigned>((size_t)PS_STAGES * (size_t)n);
    off = take<int>((size_t)C);
    bl_head = take<int>((size_t)nblk);
    bl_tail = take<int>((size_t)nblk);
    stage_bytes = bytes + 64;
  }

 private:
  uintptr_t at;                          // the address reached
  size_t bytes = 0;                      // the bytes budgeted so far: every buffer, and 8 for the gap in front of an 8-byte-aligned one
  template <typename U> U* take(size_t count) {
    if (sizeof(U) == 8) { at = (at + 7) & ~(uintptr_t)7; bytes += 8; }
    U* p = (U*)at;
    at += count * sizeof(U);
    bytes += count * sizeof(U);
    return p;
  }
};

size_t perframe_ap_workspace_bytes(long long n, int C) { return ApLayout<unsigned>(nullptr, n, C).frame_bytes; }
size_t perframe_cap_workspace_bytes(long long n, int C) { return ApLayout<ap_u64>(nullptr, n, C).frame_bytes; }
size_t perstage_ap_workspace_bytes(long long n, int C) { return ApLayout<unsigned>(nullptr, n, C).stage_bytes; }
size_t perstage_cap_workspace_bytes(long long n, int C) { return ApLayout<ap_u64>(nullptr, n, C).stage_bytes; }

// what the per-frame and the per-stage metric share: keys, every class's positives sorted, every score counted against them
// (T = unsigned: by key, AP; T = ap_u64: by (key, frame), cAP)
template <typename T>
struct ApRanked {
  T* q;                // [C][n] class c: its len[c] positives ascending (descending score)
  unsigned* cnt;       // [C][n] class c: cnt[b] = entries whose lower_bound in q is b (AP: nonzero at the first member of a tie run only)
  unsigned* len;       // [C] positives per class
  double* partial;     // [splits][C] score mass
  int splits;
};

template <typename T>
static ApRanked<T> ap_rank_positives(const float* scores, const float* target, const int* labels, long long n, int C, const ApLayout<T>& L,
                                     hipStream_t s) {
  static DeviceOnce once;
  once.run([] { (void)hipFuncSetAttribute((const void*)ap_count_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, AP_TAB * 4 + 128); });
  const int ntiles = L.ntiles;
  T *p0 = L.p0, *p1 = L.p1;
  (void)hipMemsetAsync(L.cursor, 0, (size_t)C * 4, s);
  const dim3 xg((unsigned)((n + AP_XF - 1) / AP_XF), (unsigned)((C + AP_XC - 1) / AP_XC));
  if (labels) ap_extract_kernel<true, T><<<xg, 256, 0, s>>>(scores, nullptr, labels, n, C, L.keys, p0, L.cursor);
  else ap_extract_kernel<false, T><<<xg, 256, 0, s>>>(scores, target, nullptr, n, C, L.keys, p0, L.cursor);
  const int tg = ntiles < AP_TGRID ? ntiles : AP_TGRID;
  // digit shifts, least significant first: the key's four, below them (composites) the digits that frame indices up to n - 1 have
  int shifts[8], np = 0;
  if (sizeof(T) == 8) {
    for (int p = 0; p < 4 && ((n - 1) >> (8 * p)) != 0; ++p) shifts[np++] = 8 * p;
    for (int p = 0; p < AP_PASSES; ++p) shifts[np++] = 32 + 8 * p;
  } else {
    for (int p = 0; p < AP_PASSES; ++p) shifts[np++] = 8 * p;
  }
  for (int p = 0; p < np; ++p) {
    ap32_hist_kernel<T><<<dim3(tg, C), 64, 0, s>>>(p0, L.cursor, n, ntiles, shifts[p], L.hist, p == 0 ? L.cnt : nullptr);
    ap32_scan_kernel<<<C, 256, 0, s>>>(L.hist, L.cursor, ntiles);
    ap32_scatter_kernel<T><<<dim3(tg, C), 64, 0, s>>>(p0, p1, L.cursor, n, ntiles, shifts[p], L.hist);
    T* t = p0; p0 = p1; p1 = t;
  }
  const int splits = ap_splits(C);
  ap_count_kernel<T><<<dim3(splits, C), 1024, AP_TAB * 4 + 128, s>>>(L.keys, p0, L.cursor, n, C, L.cnt, L.partial);
  return ApRanked<T>{p0, L.cnt, L.cursor, L.partial, splits};
}

// Returns 0, or -1 on a bad argument.  ws must hold perframe_ap_workspace_bytes(n, C) bytes.  Positives: target != 0, or (labels != NULL)
// the frame's class id.
int launch_perframe_ap(const float* scores, const float* target, const int* labels, long long n, int C, double* ap, long long* n_pos,
                       double* score_sum, void* ws, hipStream_t s) {
  if (n <= 0 || C <= 0 || C > 65535 || n >= (1ll << 31)) return -1;    // per-class cursors are 32-bit
  const ApRanked<unsigned> r = ap_rank_positives(scores, target, labels, n, C, ApLayout<unsigned>(ws, n, C), s);
  ap_walk_kernel<ApWalk><<<C, 256, 0, s>>>(r.q, r.cnt, r.len, n, C, nullptr, nullptr, r.partial, r.splits, ap, n_pos, score_sum);
  return 0;
}

// The calibrated metric, same arguments.  ws must hold perframe_cap_workspace_bytes(n, C) bytes (n > 0); n == 0 writes NaN / 0 / 0.0.
int launch_perframe_cap(const float* scores, const float* target, const int* labels, long long n, int C, double* ap, long long* n_pos,
                        double* score_sum, void* ws, hipStream_t s) {
  if (n < 0 || C <= 0 || C > 65535 || n >= (1ll << 31)) return -1;     // frame indices and per-class cursors are 32-bit
  if (n == 0) {
    cap_empty_kernel<<<(C + 255) / 256, 256, 0, s>>>(C, ap, n_pos, score_sum);
    return 0;
  }
  const ApRanked<ap_u64> r = ap_rank_positives(scores, target, labels, n, C, ApLayout<ap_u64>(ws, n, C), s);
  ap_walk_kernel<CapWalk><<<C, 256, 0, s>>>(nullptr, r.cnt, r.len, n, C, nullptr, nullptr, r.partial, r.splits, ap, n_pos, score_sum);
  return 0;
}

// ================================================================================================================================
// Per-stage average precision (step_recognition/utils/metrics.py:64-130 with metrics='AP'): the same metric by tenth of each action.
// Per class c the instances are the maximal runs of labels == c; a run [a, b] has len = b - a and its stage s = 0..9 holds the frames
// [a + trunc(len * (s / 10.0)), max(that + 1, a + trunc(len * ((s + 1) / 10.0)))) - IEEE double products, as the reference's
// int(len * perc).  The sample set of (c, s) = the frames with labels != c (negatives) + the stage-s frames of every run of c.
//
// Every stage positive is one of the class's positives, so no list is sorted again: with q_c / cnt_c from the per-frame pipeline
// (ap_extract, the radix passes, ap_count) and a threshold t = the score of a tie run of q_c that ends at rank r,
//   samples of (c, s) at or above t = (column c at or above t) - (positives of c at or above t) + (stage-s positives of c at or above t)
//                                   = (cnt_c[0] + ... + cnt_c[r])  -  (r + 1)                   +  (st_cs[0] + ... + st_cs[r])
// where st_cs[b] = the stage-s positives of c whose lower_bound in q_c is b (b = the first member of their tie run).
//   ps_edges     per 1024-frame block: its last run head (labels[i] != labels[i-1]) and its first run tail
//   ps_carry     one workgroup: running max of the heads in front of each block, running min of the tails behind it, and the offset
//                of each class's counters (exclusive sum of the positives per class: the labels are single, so they sum to <= n)
//   ps_stage     per frame: run start (forward max-scan of the heads) and run end (backward min-scan of the tails); a positive derives
//                its 10-bit stage mask from (i - a, len), finds its key's lower_bound in q_c and adds 1 to st_cs[b] of its stages
//   ap_walk<PsWalk>   one workgroup per (class, stage) walks q_c, cnt_c and st_cs once: two running prefixes, the tie-run ends of q, fp64
//                accumulation of (stage positives in the run) * (stage positives so far) / (samples so far).
// Integer atomics only (any order gives the same counters); the one floating-point sum has a fixed order: the same bits on every run.
//
// Per-stage calibrated average precision (metrics='cAP'), T = the (key, frame) composite: the lower_bound of a positive is its own
// index, so st_cs holds the stage's member flags and cnt_c the ranks in the stable order.  ap_walk<CpsWalk> counts the members P_cs
// first (w = (n - P_c) / P_cs) and accumulates, for a member at index i with rank r, tps / (tps + fps / (w + eps) + eps) with
// tps = the members up to i and fps = r - (i + 1), the negatives in front of it.
// ================================================================================================================================

// the labels around a thread's four frames i0 .. i0 + 3 (lab[e + 1]: frame i0 + e; 0 outside [0, n)), which of the four start (head) or
// end (tail) a run of equal labels, the thread's last head h (-1: none) and its first tail t (0x7FFFFFFF: none)
struct PsRunEdges {
  int lab[6];
  bool head[4], tail[4];
  int h, t;
};
__device__ __forceinline__ PsRunEdges ps_run_edges(const int* __restrict__ labels, long long n, long long i0) {
  PsRunEdges r;
  r.h = -1;
  r.t = 0x7FFFFFFF;
#pragma unroll
  for (int e = 0; e < 6; ++e) { const long long i = i0 - 1 + e; r.lab[e] = (i >= 0 && i < n) ? labels[i] : 0; }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long i = i0 + e;
    r.head[e] = i < n && (i == 0 || r.lab[e + 1] != r.lab[e]);
    r.tail[e] = i < n && (i == n - 1 || r.lab[e + 1] != r.lab[e + 2]);
    if (r.head[e]) r.h = (int)i;
    if (r.tail[e] && r.t == 0x7FFFFFFF) r.t = (int)i;
  }
  return r;
}

__global__ __launch_bounds__(256) void ps_edges_kernel(const int* __restrict__ labels, long long n, int* __restrict__ bl_head,
                                                       int* __restrict__ bl_tail) {
  __shared__ int wh[4], wt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PsRunEdges r = ps_run_edges(labels, n, (long long)blockIdx.x * PS_BLK + (long long)tid * 4);
  int h = r.h, t = r.t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { h = max(h, __shfl_xor(h, o, 64)); t = min(t, __shfl_xor(t, o, 64)); }
  if (lane == 0) { wh[wave] = h; wt[wave] = t; }
  __syncthreads();
  if (tid == 0) {
    bl_head[blockIdx.x] = max(max(wh[0], wh[1]), max(wh[2], wh[3]));
    bl_tail[blockIdx.x] = min(min(wt[0], wt[1]), min(wt[2], wt[3]));
  }
}

__global__ __launch_bounds__(256) void ps_carry_kernel(int* __restrict__ bl_head, int* __restrict__ bl_tail, int nblk,
                                                       const unsigned* __restrict__ len, int C, int* __restrict__ off) {
  __shared__ int wsum[2][4];
  wg_scan_array<ScanMax, false, 1>(bl_head, nblk, -1, wsum);            // -> the last head in front of the block
  wg_scan_array<ScanMin, true, 1>(bl_tail, nblk, 0x7FFFFFFF, wsum);     // -> the first tail behind the block
  for (int c = threadIdx.x; c < C; c += 256) off[c] = (int)len[c];
  __syncthreads();
  wg_scan_array<ScanSum, false, 1>(off, C, 0, wsum);                    // positives of the classes in front (their sum is <= n < 2^31)
}

// T = the (key, frame) composite (cAP): the lower_bound of a positive is its own index, st_cs marks the stage's members
template <typename T>
__global__ __launch_bounds__(256) void ps_stage_kernel(const float* __restrict__ scores, const int* __restrict__ labels, long long n, int C,
                                                       const int* __restrict__ carry_head, const int* __restrict__ carry_tail,
                                                       const T* __restrict__ q_all, const unsigned* __restrict__ len,
                                                       const int* __restrict__ off, unsigned* __restrict__ st) {
  __shared__ int wh[4], wt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i0 = (long long)blockIdx.x * PS_BLK + (long long)tid * 4;
  const PsRunEdges r = ps_run_edges(labels, n, i0);
  int hs = r.h, ts = r.t;                                   // inclusive scans over the wave: heads from the front, tails from the back
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(hs, o, 64), d = __shfl_down(ts, o, 64);
    if (lane >= o) hs = max(hs, u);
    if (lane + o < 64) ts = min(ts, d);
  }
  if (lane == 63) wh[wave] = hs;
  if (lane == 0) wt[wave] = ts;
  __syncthreads();
  int a_run = __shfl_up(hs, 1, 64), b_run = __shfl_down(ts, 1, 64);
  if (lane == 0) a_run = -1;
  if (lane == 63) b_run = 0x7FFFFFFF;
  a_run = max(a_run, carry_head[blockIdx.x]);
  b_run = min(b_run, carry_tail[blockIdx.x]);
  for (int w = 0; w < 4; ++w) {
    if (w < wave) a_run = max(a_run, wh[w]);
    if (w > wave) b_run = min(b_run, wt[w]);
  }
  int a[4], b[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { if (r.head[e]) a_run = (int)(i0 + e); a[e] = a_run; }
#pragma unroll
  for (int e = 3; e >= 0; --e) { if (r.tail[e]) b_run = (int)(i0 + e); b[e] = b_run; }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long i = i0 + e;
    const int c = r.lab[e + 1];
    if (i >= n || c < 0 || c >= C) continue;
    const double rl = (double)(b[e] - a[e]);
    const long long at = i - a[e];
    unsigned mask = 0u;
#pragma unroll
    for (int sg = 0; sg < PS_STAGES; ++sg) {
      const long long lo = (long long)(rl * ((double)sg / 10.0));
      const long long hi = max(lo + 1, (long long)(rl * ((double)(sg + 1) / 10.0)));
      if (at >= lo && at < hi) mask |= 1u << sg;
    }
    if (!mask) continue;                                    // the last frame of a run of two or more
    const unsigned P = len[c];
    if (P == 0u) continue;
    const T k = ap_entry<T>(ap_desc_key(scores[(size_t)i * C + c]), i);
    const unsigned lb = ap_lower_bound(q_all + (size_t)c * n, P, k);
    if (lb >= P) continue;                                  // cannot happen: k is in the list
    unsigned* dst = st + (size_t)off[c] + lb;
#pragma unroll
    for (int sg = 0; sg < PS_STAGES; ++sg)
      if (mask >> sg & 1u) atomicAdd(dst + (size_t)sg * n, 1u);
  }
}

template <typename T>
static int perstage_launch(const float* scores, const int* labels, long long n, int C, double* ap, long long* n_pos, void* ws, hipStream_t s) {
  if (n < 0 || C <= 0 || C > 65535 || n >= (1ll << 31)) return -1;
  if (n == 0) {
    (void)hipMemsetAsync(ap, 0, (size_t)PS_STAGES * C * 8, s);
    if (n_pos) (void)hipMemsetAsync(n_pos, 0, (size_t)PS_STAGES * C * 8, s);
    return 0;
  }
  const ApLayout<T> L(ws, n, C);
  const ApRanked<T> r = ap_rank_positives(scores, nullptr, labels, n, C, L, s);
  (void)hipMemsetAsync(L.st, 0, (size_t)PS_STAGES * (size_t)n * 4, s);
  ps_edges_kernel<<<L.nblk, 256, 0, s>>>(labels, n, L.bl_head, L.bl_tail);
  ps_carry_kernel<<<1, 256, 0, s>>>(L.bl_head, L.bl_tail, L.nblk, r.len, C, L.off);
  ps_stage_kernel<T><<<L.nblk, 256, 0, s>>>(scores, labels, n, C, L.bl_head, L.bl_tail, r.q, r.len, L.off, L.st);
  const dim3 grid(C, PS_STAGES);
  if constexpr (sizeof(T) == 4) ap_walk_kernel<PsWalk><<<grid, 256, 0, s>>>(r.q, r.cnt, r.len, n, C, L.st, L.off, nullptr, 0, ap, n_pos, nullptr);
  else ap_walk_kernel<CpsWalk><<<grid, 256, 0, s>>>(nullptr, r.cnt, r.len, n, C, L.st, L.off, nullptr, 0, ap, n_pos, nullptr);
  return 0;
}

// Returns 0, or -1 on a bad argument.  ws must hold perstage_ap_workspace_bytes(n, C) bytes (n > 0).  ap / n_pos: [10][C].
int launch_perstage_ap(const float* scores, const int* labels, long long n, int C, double* ap, long long* n_pos, void* ws, hipStream_t s) {
  return perstage_launch<unsigned>(scores, labels, n, C, ap, n_pos, ws, s);
}
// The calibrated metric by stage: ws must hold perstage_cap_workspace_bytes(n, C) bytes (n > 0); NaN where a (stage, class) has no member.
int launch_perstage_cap(const float* scores, const int* labels, long long n, int C, double* ap, long long* n_pos, void* ws, hipStream_t s) {
  return perstage_launch<ap_u64>(scores, labels, n, C, ap, n_pos, ws, s);
}
