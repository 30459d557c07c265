// Viterbi decoding on the device (include/prego_amd.h, prego_viterbi_decode): the cheapest label sequence of V videos under per-frame
// emission costs and a first-order transition matrix.  ONE launch, one 256-thread workgroup per video (the grid strides over the videos
// when there are more of them than workgroups); no workgroup waits for another, integers only, no global atomics.
//
// FORWARD.  The T steps of a video are sequential, so the step is the whole cost.  Thread tid owns the pair (j = tid / 2, half = tid % 2):
// column j of `trans`, rows [half LEN, half LEN + LEN), LEN = the instantiation's slice (2 LEN >= C), kept in registers for the whole
// launch as 64-bit words trans << 7 (forbidden: DEC_INF, so the one addition also says "not allowed").  d_{t-1} lives in LDS as KEYS,
// key(i) = d(i) << 7 | i (no path: DEC_INF), double-buffered, one barrier per step; a thread reads its slice as LEN / 2 16-byte reads,
// all issued before the first candidate is formed (every lane of a half reads the same address: broadcasts; the second half's slice
// sits two words further so that the two addresses of a wave never share a bank).  A candidate is key(i) + (trans << 7): the minimum
// over the keys IS the minimum over the costs with the lowest i on a tie, because i rides in the low bits; four independent chains of
// minima per thread, and the two halves of a j are neighbouring lanes that meet by one cross-lane exchange (this is the 64-bit form of
// the step; its 32-bit form, which most stretches run in, is below).  The thread of half 0 adds the emission cost, writes the new key
// and the back-pointer, one byte per (t, j), into the workspace row of the frame (coalesced).  Emission rows are requested
// PREGO_DECODE_PREFETCH frames ahead into registers (the time loop is unrolled by that depth, so the ring is addressed statically) and
// quantised on arrival; the step's barrier waits for LDS only (raw s_barrier behind s_waitcnt lgkmcnt(0): __syncthreads would drain the
// rows in flight).
// EXACTNESS.  d is exact for every accepted input and nothing saturates.  The state of a video is its 64-bit keys: a finite d is at
// most T (CAP + CAP) < 2^31 * 2^16 = 2^47, its key below 2^54; DEC_INF = 2^62 and DEC_INF + DEC_INF = 2^63 does not wrap, so "no path"
// (an infinite d, a forbidden transition, or both) is simply key >= DEC_INF after the one addition, and a state far above the step's
// minimum keeps its exact value for as long as it lives.  That argument needs every word a step reads to be a key: the slots of both
// widths, those of the states i >= C and the padding included, are set to "no path" when the kernel starts and only the slots of the
// states below C are ever written after that.
// 32-BIT STRETCHES.  The 64-bit candidate costs a 64-bit add, a 64-bit compare and two selects; a 32-bit one a saturating add and a
// third of a v_min3.  So the steps run in stretches of at most BLK (frames [1, BLK), [BLK, 2 BLK), ...), and in front of each the
// workgroup looks at the exact keys: m and M, the smallest and the largest FINITE d.  If M - m < DEC_FAST_SPREAD = 2^24 - BLK (CAP + CAP)
// the stretch runs on 32-bit keys relative to the base m, rkey(i) = (d(i) - m) << 7 | i, "no path" = a forbidden transition = 2^32 - 1,
// candidates by a saturating add; otherwise - some state IS far above the minimum - it runs on the exact 64-bit keys as they are.
// Proof that a 32-bit stretch cannot overflow: costs are non-negative, so every later finite d is >= m and the relative values never go
// below 0; a finite d_t(j) is some finite d_{t-1}(i) + trans + e <= max finite d_{t-1} + CAP + CAP, so after s <= BLK steps every
// finite relative value is < DEC_FAST_SPREAD + s (CAP + CAP) <= 2^24, its key < 2^31, and a candidate key + (trans << 7) < 2^31 + 2^22
// neither wraps nor reaches 2^32 - 1: the saturating add saturates exactly when one side is "no path".  The minimum over such keys is the
// minimum over the exact costs with the lowest i on a tie (the base is common), so a stretch leaves the same keys, to the bit, in
// either width; behind a 32-bit stretch the keys go back to 64 bits (base << 7 + rkey) before anything else reads them.  A frame
// with no finite state at the start of a stretch ends the forward pass: the video is infeasible whatever follows.
// BACKTRACE.  Not T dependent loads from HBM: the video is cut into blocks of PREGO_DECODE_BLOCK frames.  (a) for every (block, state at
// the block's last frame) in parallel, the walk down the block's back-pointers gives the state at the last frame of the block in front
// of it: the block's map, C bytes; (b) the maps are composed from the end state backwards, staged through LDS DEC_MAP_CHUNK blocks at
// a time, one lane, one LDS read per block: the state at every block's last frame; (c) every block is walked once more from that
// state, a thread per block, writing the labels.  Every byte read back from the workspace is clamped below C before it indexes.
#include "common.h"
#include "decode_model.h"
#include "kernels.h"

#define DEC_GRID 1024                      // workgroups of a launch at most: four per CU; more videos than that are strided over
#define DEC_INF (1ull << 62)
#define DEC_INF32 0xFFFFFFFFu              // "no path" among the 32-bit keys, and a forbidden transition beside them
#define DEC_SLOTS 132                      // 64-bit keys of one buffer: 128 states + the second half's shift of 2 + padding to 16 bytes
#define DEC_SLOTS32 136                    // 32-bit keys of one buffer: 128 states + the second half's shift of 4 + padding to 16 bytes
// the spread of the finite d at the start of a stretch below which its BLK steps fit 32-bit keys: 2^24 - BLK (CAP + CAP) = 12 583 040
#define DEC_FAST_SPREAD ((1ll << 24) - (long long)kDecodeBlock * 2 * kDecodeCap)
#define DEC_MAP_CHUNK 64                   // block maps staged in LDS at a time
#define DEC_WALKS 4                        // (block, state) walks a thread of the backtrace runs side by side
#define PF kDecodePrefetch
#define BLK kDecodeBlock

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));

struct DecArgs {
  const unsigned* src;        // [n_frames][ld] words: fp32 probabilities or int32 costs
  long long ld;
  const int* offsets;
  int n_videos, C;
  long long n_frames;
  const int *trans, *init;    // init nullable
  int* labels;
  long long* records;
  // workspace: back-pointers [n_frames][C], block maps [n_frames / BLK + n_videos + 1][C], block end states [n_frames / BLK + n_videos + 1]
  unsigned char *bp, *maps, *ends;
};

static size_t dec_align16(size_t v) { return (v + 15) / 16 * 16; }
size_t viterbi_workspace_bytes(long long n, int V, int C) {
  const size_t blocks = (size_t)n / BLK + (size_t)V + 1;
  return dec_align16((size_t)n * C) + dec_align16(blocks * C) + dec_align16(blocks);
}

// the LDS slot of state i: the second half's slice starts 16 bytes further (two 64-bit keys, four 32-bit keys)
template <int LEN> __device__ __forceinline__ int dec_slot(int i) { return i + (i >= LEN ? 2 : 0); }
template <int LEN> __device__ __forceinline__ int dec_slot32(int i) { return i + (i >= LEN ? 4 : 0); }

// the step's barrier: my LDS writes are done, nothing else is waited for (the emission rows in flight stay in flight)
__device__ __forceinline__ void dec_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the smallest and the largest FINITE key of a step (kmin = DEC_INF: none); every wave for itself, the same values in all
template <int LEN> __device__ __forceinline__ void dec_key_range(const u64* keys, int C, u64& kmin, u64& kmax) {
  const int lane = threadIdx.x & 63;
  kmin = DEC_INF;
  kmax = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = lane + 64 * r;
    if (i < C) {
      const u64 k = keys[dec_slot<LEN>(i)];
      if (k < DEC_INF) { kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 lo = (u64)__shfl_xor((long long)kmin, o, 64), hi = (u64)__shfl_xor((long long)kmax, o, 64);
    kmin = lo < kmin ? lo : kmin;
    kmax = hi > kmax ? hi : kmax;
  }
}

template <int LEN, bool COSTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void viterbi_kernel(const DecArgs A) {
  __shared__ __attribute__((aligned(16))) u64 dk[2][DEC_SLOTS];
  __shared__ __attribute__((aligned(16))) unsigned rk[2][DEC_SLOTS32];
  __shared__ unsigned short lut[256];
  __shared__ unsigned char mapch[DEC_MAP_CHUNK * kDecodeMaxClasses];
  __shared__ unsigned char endch[DEC_MAP_CHUNK];
  const int tid = threadIdx.x, j = tid >> 1, half = tid & 1, C = A.C;
  const bool owner = half == 0 && j < C;                    // writes state j: its key, its back-pointer; loads its emissions
  const long long nf = A.n_frames;
  // ---- the model: this thread's slice of column j, in both key widths, and init[j] ----
  u64 trk[LEN];
  unsigned trk32[LEN];
#pragma unroll
  for (int k = 0; k < LEN; ++k) {
    const int i = half * LEN + k;
    const int w = (i < C && j < C) ? dec_model_word(A.trans[(size_t)i * C + j]) : -1;
    trk[k] = w < 0 ? DEC_INF : (u64)w << 7;
    trk32[k] = w < 0 ? DEC_INF32 : (unsigned)w << 7;
  }
  const int ini = j < C ? (A.init ? dec_model_word(A.init[j]) : 0) : -1;
  lut[tid] = kDecodeLut[tid];
  // every key slot starts as "no path".  The slots of the states i >= C (a slice covers LEN of them, 2 LEN >= C) and the padding are
  // never written again, so no step ever reads a word this kernel did not write: whatever an earlier kernel left in the CU's LDS
  // could otherwise wrap a 64-bit candidate (stale + DEC_INF) below DEC_INF and win a minimum
  for (int q = tid; q < 2 * DEC_SLOTS; q += 256) (&dk[0][0])[q] = DEC_INF;
  for (int q = tid; q < 2 * DEC_SLOTS32; q += 256) (&rk[0][0])[q] = DEC_INF32;
  __syncthreads();

  for (int v = blockIdx.x; v < A.n_videos; v += gridDim.x) {
    long long a = (long long)A.offsets[v], b = (long long)A.offsets[v + 1];
    a = a < 0 ? 0 : (a > nf ? nf : a);
    b = b < 0 ? 0 : (b > nf ? nf : b);
    if (b < a) b = a;
    const long long T = b - a;
    if (T == 0) {                                           // uniform: nobody passes a barrier
      if (tid == 0) { A.records[2 * (size_t)v] = 0; A.records[2 * (size_t)v + 1] = -1; }
      continue;
    }
    // ---- forward ----
    const unsigned* row = A.src + (size_t)a * (size_t)A.ld + (owner ? j : 0);
    unsigned char* bprow = A.bp + (size_t)a * C;
    unsigned raw[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) raw[u] = (owner && u < T) ? row[(size_t)u * (size_t)A.ld] : 0u;
    {                                                       // frame 0: d_0(j) = init[j] + e_0(j)
      const int ec = COSTS ? dec_cost_of_word(raw[0]) : dec_cost_of_prob(raw[0], lut);
      if (owner && PF < T) raw[0] = row[(size_t)PF * (size_t)A.ld];
      if (owner) dk[0][dec_slot<LEN>(j)] = ini < 0 ? DEC_INF : ((((u64)ini + (u64)ec) << 7) | (u64)j);
      dec_lds_barrier();
    }
    bool fast = false, no_path = false;                     // the running stretch uses 32-bit keys; a frame without a finite state was met
    u64 base7 = 0;                                          // fast: the stretch's base cost << 7
    for (long long t0 = 0; t0 < T && !no_path; t0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const long long t = t0 + u;
        if (t == 0) continue;
        if (t >= T) break;
        const int rb = (int)((t + 1) & 1), wb = (int)(t & 1);
        if (t == 1 || (t & (BLK - 1)) == 0) {
          // ---- a stretch of at most BLK steps begins: which key width it runs in (uniform: every wave sees the same keys) ----
          if (fast) {                                       // back to the exact 64-bit keys
            if (owner) { const unsigned k = rk[rb][dec_slot32<LEN>(j)]; dk[rb][dec_slot<LEN>(j)] = k == DEC_INF32 ? DEC_INF : base7 + k; }
            dec_lds_barrier();
          }
          u64 kmin, kmax;
          dec_key_range<LEN>(dk[rb], C, kmin, kmax);
          if (kmin >= DEC_INF) { no_path = true; break; }   // infeasible for good: every later d is infinite
          fast = (long long)((kmax >> 7) - (kmin >> 7)) < DEC_FAST_SPREAD;
          base7 = (kmin >> 7) << 7;
          if (fast) {
            if (owner) { const u64 k = dk[rb][dec_slot<LEN>(j)]; rk[rb][dec_slot32<LEN>(j)] = k >= DEC_INF ? DEC_INF32 : (unsigned)(k - base7); }
            dec_lds_barrier();
          }
        }
        const int ec = COSTS ? dec_cost_of_word(raw[u]) : dec_cost_of_prob(raw[u], lut);
        if (owner && t + PF < T) raw[u] = row[(size_t)(t + PF) * (size_t)A.ld];
        if (fast) {
          // 32-bit keys relative to the stretch's base: one saturating add and one min per candidate
          const u32x4_* slice = (const u32x4_*)&rk[rb][half * (LEN + 4)];
          u32x4_ q[LEN / 4];                                 // every read is issued before the first candidate waits for one
#pragma unroll
          for (int m = 0; m < LEN / 4; ++m) q[m] = slice[m];
          unsigned b0 = DEC_INF32, b1 = DEC_INF32, b2 = DEC_INF32, b3 = DEC_INF32;
#pragma unroll
          for (int m = 0; m < LEN / 4; ++m) {
            b0 = min(b0, __builtin_elementwise_add_sat(q[m].x, trk32[4 * m]));
            b1 = min(b1, __builtin_elementwise_add_sat(q[m].y, trk32[4 * m + 1]));
            b2 = min(b2, __builtin_elementwise_add_sat(q[m].z, trk32[4 * m + 2]));
            b3 = min(b3, __builtin_elementwise_add_sat(q[m].w, trk32[4 * m + 3]));
          }
          unsigned best = min(min(b0, b1), min(b2, b3));
          best = min(best, (unsigned)__shfl_xor((int)best, 1, 64));
          if (owner) {
            const bool dead = best == DEC_INF32;
            rk[wb][dec_slot32<LEN>(j)] = dead ? DEC_INF32 : ((((best >> 7) + (unsigned)ec) << 7) | (unsigned)j);
            bprow[(size_t)t * C + j] = dead ? (unsigned char)0 : (unsigned char)(best & 127u);
          }
        } else {
          const u64x2* slice = (const u64x2*)&dk[rb][half * (LEN + 2)];
          u64x2 q[LEN / 2];
#pragma unroll
          for (int m = 0; m < LEN / 2; ++m) q[m] = slice[m];
          u64 b0 = DEC_INF, b1 = DEC_INF, b2 = DEC_INF, b3 = DEC_INF;      // four independent chains of minima
#pragma unroll
          for (int m = 0; m < LEN / 2; m += 2) {
            const u64 c0 = q[m].x + trk[2 * m], c1 = q[m].y + trk[2 * m + 1], c2 = q[m + 1].x + trk[2 * m + 2], c3 = q[m + 1].y + trk[2 * m + 3];
            b0 = c0 < b0 ? c0 : b0;
            b1 = c1 < b1 ? c1 : b1;
            b2 = c2 < b2 ? c2 : b2;
            b3 = c3 < b3 ? c3 : b3;
          }
          b0 = b1 < b0 ? b1 : b0;
          b2 = b3 < b2 ? b3 : b2;
          u64 best = b2 < b0 ? b2 : b0;
          const u64 other = (u64)__shfl_xor((long long)best, 1, 64);
          best = other < best ? other : best;
          if (owner) {
            const bool dead = best >= DEC_INF;
            dk[wb][dec_slot<LEN>(j)] = dead ? DEC_INF : ((((best >> 7) + (u64)ec) << 7) | (u64)j);
            bprow[(size_t)t * C + j] = dead ? (unsigned char)0 : (unsigned char)(best & 127u);
          }
        }
        dec_lds_barrier();
      }
    }
    // ---- the end state: the smallest key of the last step ----
    u64 endkey = DEC_INF, unused_max;
    if (!no_path) {
      const int lb = (int)((T - 1) & 1);
      if (fast) {                                           // the last stretch ran in 32 bits
        if (owner) { const unsigned k = rk[lb][dec_slot32<LEN>(j)]; dk[lb][dec_slot<LEN>(j)] = k == DEC_INF32 ? DEC_INF : base7 + k; }
        dec_lds_barrier();
      }
      dec_key_range<LEN>(dk[lb], C, endkey, unused_max);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // my back-pointers have left
    __syncthreads();                                        // the back-pointers are the workgroup's; nobody still reads the keys
    int* labels = A.labels + a;
    if (endkey >= DEC_INF) {                                // infeasible: at some frame no state was finite
      for (long long t = tid; t < T; t += 256) labels[t] = -1;
      if (tid == 0) { A.records[2 * (size_t)v] = -1; A.records[2 * (size_t)v + 1] = -1; }
      continue;                                             // uniform; the barrier above separates this video's keys from the next's
    }
    const int end_state = (int)(endkey & 127u);
    if (tid == 0) { A.records[2 * (size_t)v] = (long long)(endkey >> 7); A.records[2 * (size_t)v + 1] = end_state; }
    // ---- backtrace (a): the map of every block ----
    const long long nb = (T + BLK - 1) / BLK;
    const size_t mb = (size_t)(a / BLK) + (size_t)v;         // the video's first block in maps / ends (disjoint for ascending offsets)
    unsigned char* maps = A.maps + mb * C;
    unsigned char* ends = A.ends + mb;
    for (long long first = 0; first < nb * C; first += 256 * DEC_WALKS) {      // DEC_WALKS independent walks per thread: loads in flight
      long long item[DEC_WALKS], hi[DEC_WALKS], lo[DEC_WALKS];
      int s[DEC_WALKS];
#pragma unroll
      for (int c = 0; c < DEC_WALKS; ++c) {
        item[c] = first + c * 256 + tid;
        const long long blk = item[c] / C;
        s[c] = (int)(item[c] - blk * C);
        hi[c] = (blk + 1) * BLK < T ? (blk + 1) * BLK : T;
        lo[c] = blk * BLK > 1 ? blk * BLK : 1;                // frame 0 has no back-pointer
        if (item[c] >= nb * C) lo[c] = hi[c];                 // no such item: no step
      }
      for (int k = 1; k <= BLK; ++k) {
#pragma unroll
        for (int c = 0; c < DEC_WALKS; ++c) {
          const long long t = hi[c] - k;
          if (t >= lo[c]) { const int p = bprow[(size_t)t * C + s[c]]; s[c] = p < C ? p : C - 1; }
        }
      }
#pragma unroll
      for (int c = 0; c < DEC_WALKS; ++c)
        if (item[c] < nb * C) maps[(size_t)item[c]] = (unsigned char)s[c];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- (b): the state at the last frame of every block, from the end state backwards ----
    int s_run = end_state;                                  // lane 0's: the state at the last frame of the block it is about to enter
    for (long long top = nb; top > 0; top -= DEC_MAP_CHUNK) {
      const long long bot = top > DEC_MAP_CHUNK ? top - DEC_MAP_CHUNK : 0;
      const int nblk = (int)(top - bot);
      for (int q = tid; q < nblk * C; q += 256) mapch[q] = maps[(size_t)bot * C + q];
      __syncthreads();
      if (tid == 0) {
        for (int k = nblk - 1; k >= 0; --k) {
          endch[k] = (unsigned char)s_run;
          const int p = mapch[k * C + s_run];
          s_run = p < C ? p : C - 1;
        }
      }
      __syncthreads();
      if (tid < nblk) ends[bot + tid] = endch[tid];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- (c): the labels, a thread per block ----
    for (long long blk = tid; blk < nb; blk += 256) {
      long long hi = (blk + 1) * BLK;
      if (hi > T) hi = T;
      const int e0 = ends[blk];
      int s = e0 < C ? e0 : C - 1;
      for (long long t = hi - 1; t >= blk * BLK; --t) {
        labels[t] = s;
        if (t > 0) { const int p = bprow[(size_t)t * C + s]; s = p < C ? p : C - 1; }
      }
    }
    __syncthreads();                                        // mapch, endch and the keys are free for the next video
  }
}

// probabilities [n][ld] -> costs [n][C], one element per thread (the grid strides when n C exceeds it)
__global__ __launch_bounds__(256) void emission_costs_kernel(const unsigned* __restrict__ probs, long long ld, long long n, int C,
                                                             int* __restrict__ costs) {
  const long long total = n * C;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long r = idx / C;
    const int c = (int)(idx - r * C);
    costs[idx] = dec_cost_of_prob(probs[(size_t)r * (size_t)ld + c], kDecodeLut);
  }
}

template <bool COSTS> static void dec_launch(int C, int grid, const DecArgs& A, hipStream_t s) {
  if (2 * 8 >= C) viterbi_kernel<8, COSTS><<<grid, 256, 0, s>>>(A);
  else if (2 * 16 >= C) viterbi_kernel<16, COSTS><<<grid, 256, 0, s>>>(A);
  else if (2 * 32 >= C) viterbi_kernel<32, COSTS><<<grid, 256, 0, s>>>(A);
  else if (2 * 48 >= C) viterbi_kernel<48, COSTS><<<grid, 256, 0, s>>>(A);
  else viterbi_kernel<64, COSTS><<<grid, 256, 0, s>>>(A);
}

// Returns 0, or -1 on a bad argument (nothing launched).  ws must hold viterbi_workspace_bytes(n_frames, n_videos, n_classes) bytes;
// n_frames == 0: every video is empty, src and ws are not touched.
int launch_viterbi(bool costs, const void* src, long long ld, const int* offsets, int n_videos, long long n_frames, int C, const int* trans,
                   const int* init, int* labels, long long* records, void* ws, hipStream_t s) {
  if (n_videos < 1 || n_frames < 0 || n_frames >= (1ll << 31) || C < 1 || C > kDecodeMaxClasses || ld < C) return -1;
  DecArgs A;
  A.src = (const unsigned*)src; A.ld = ld; A.offsets = offsets; A.n_videos = n_videos; A.C = C; A.n_frames = n_frames;
  A.trans = trans; A.init = init; A.labels = labels; A.records = records;
  const size_t blocks = (size_t)n_frames / BLK + (size_t)n_videos + 1;
  A.bp = (unsigned char*)ws;
  A.maps = A.bp + dec_align16((size_t)n_frames * C);
  A.ends = A.maps + dec_align16(blocks * C);
  const int grid = n_videos < DEC_GRID ? n_videos : DEC_GRID;
  if (costs) dec_launch<true>(C, grid, A, s); else dec_launch<false>(C, grid, A, s);
  return 0;
}

int launch_emission_costs(const float* probs, long long ld, long long n_frames, int C, int* costs, hipStream_t s) {
  if (n_frames < 1 || C < 1 || ld < C) return -1;
  const long long blocks = (n_frames * C + 255) / 256;
  emission_costs_kernel<<<(int)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>((const unsigned*)probs, ld, n_frames, C, costs);
  return 0;
}
