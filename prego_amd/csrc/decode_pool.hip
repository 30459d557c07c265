// Decode pool (include/prego_amd.h, prego_decode_pool_*; host side: decode_pool.cpp): online fixed-lag Viterbi.  Every live stream owns a
// SLOT of the caller's device block - header, the 64-bit keys of its last frame, a ring of back-pointer rows (kernels.h, DecodePoolGeom)
// - and one launch advances any subset of the slots by 1..32 frames each: one 256-thread workgroup per named slot, no workgroup waits
// for another, integers only, no workspace, no global atomic.  The model, the costs and the tie rules are decode.hip's (section 9b).
//
// FIXED LAG L.  After frame t of a stream is ingested and t >= L, frame f = t - L is committed: label(f) = the state at frame f on the
// back-pointer chain that starts at e_t, the lowest j with the smallest finite d_t(j).  Flush commits the frames [max(0, T - L), T) from
// the chain that starts at e_{T-1}.  A frame at which no state is finite makes the stream DEAD: every label committed from then on is
// -1, at flush too; labels already committed stay.  So label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f].  Consecutive labels
// come from different chains: the committed sequence need not be an allowed path.
//
// PUSH, per slot.  (1) Staging: the call's K emission rows are quantised into LDS (16-bit costs; 4-byte loads, so a row needs no
// alignment and the words behind n_classes are never read); the min(frames, L) ring rows the commit will walk through come from the slot
// into an LDS copy of the ring (same row index, 128 bytes a row: at most 288 rows = 36 KB); the keys come into LDS.  (2) Forward: the
// offline kernel's step.  Thread (j, half) holds its slice of column j of trans in registers as 32-bit words trans << 7; d_{t-1} sits in
// LDS as keys d << 7 | i, double-buffered, one barrier per step.  In front of the call's steps (a call has at most 32 <= BLK of them)
// the workgroup makes decode.hip's spread test on the exact keys: below DEC_FAST_SPREAD the steps run on 32-bit keys relative to the
// smallest finite d (saturating add, min), else on the 64-bit keys as they are (the slice widened on the fly: such calls are rare).
// decode.hip carries the proof that both leave the same 64-bit keys; they are what goes back to the slot, so nothing saturates and a state
// far above the minimum keeps its exact value from call to call.  The fourth wave, beside its share of the step, reduces the keys of
// the frame in front (the step's read buffer) to e_t.  A dead stream needs no path of its own: every key is "no path" and stays so.
// The back-pointer byte of (t, j) goes into the LDS ring.  (3) Commit: lane k < K walks from e_{F+k} down L rows of the LDS ring, K
// walks side by side, every byte clamped below C before it indexes; one lane feeds the labels in frame order through the pools' update
// rule (pool_record.h) into the slot's record and writes the header; the K new ring rows go to the slot in 16-byte stores.
// The result depends on the frames only: the commit never looks at where a call began.
#include "common.h"
#include "decode_model.h"
#include "kernels.h"
#include "pool_record.h"

#define DP_INF (1ull << 62)
#define DP_INF32 0xFFFFFFFFu
#define DP_SLOTS 132                       // as decode.hip: 128 states + the second half's shift + padding to 16 bytes
#define DP_SLOTS32 136
#define DP_FAST_SPREAD ((1ll << 24) - (long long)kDecodeBlock * 2 * kDecodeCap)
#define DP_RING_MAX (kDecodePoolMaxLag + kDecodePoolBurst)
#define DP_ROW 128                         // bytes of a ring row in LDS

typedef unsigned long long u64;
typedef u64 dp_u64x2 __attribute__((ext_vector_type(2)));
typedef int dp_i32x4 __attribute__((ext_vector_type(4)));

static_assert(kDecodePoolBurst <= kDecodeBlock, "a call's steps are one stretch of the spread test");

namespace {
template <int LEN> __device__ __forceinline__ int dp_slot(int i) { return i + (i >= LEN ? 2 : 0); }
template <int LEN> __device__ __forceinline__ int dp_slot32(int i) { return i + (i >= LEN ? 4 : 0); }

// the smallest and the largest finite key (kmin = DP_INF: none); every wave for itself, the same values in all.  The slots of the states
// >= C hold "no path"
template <int LEN> __device__ __forceinline__ void dp_key_range(const u64* keys, u64& kmin, u64& kmax) {
  const int lane = threadIdx.x & 63;
  kmin = DP_INF;
  kmax = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const u64 k = keys[dp_slot<LEN>(lane + 64 * r)];
    if (k < DP_INF) { kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 lo = (u64)__shfl_xor((long long)kmin, o, 64), hi = (u64)__shfl_xor((long long)kmax, o, 64);
    kmin = lo < kmin ? lo : kmin;
    kmax = hi > kmax ? hi : kmax;
  }
}

// e_t of one frame's 32-bit keys, by one wave: the state in the low bits of the smallest key, -1 when none is finite
template <int LEN> __device__ __forceinline__ int dp_end32(const unsigned* keys) {
  const int lane = threadIdx.x & 63;
  unsigned k = min(keys[dp_slot32<LEN>(lane)], keys[dp_slot32<LEN>(lane + 64)]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = min(k, (unsigned)__shfl_xor((int)k, o, 64));
  return k == DP_INF32 ? -1 : (int)(k & 127u);
}

__device__ __forceinline__ char* dp_state(const DecodePoolGeom& g, int slot) { return g.state + (size_t)slot * g.slot_bytes; }
}  // namespace

template <int LEN, bool COSTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void decode_pool_push_kernel(
    const DecodePoolGeom g, const PoolSlots sl, const RaggedMap rows, const unsigned* __restrict__ src, long long ld, int* __restrict__ labels,
    int* __restrict__ commit, int* __restrict__ now) {
  __shared__ __attribute__((aligned(16))) u64 dk[2][DP_SLOTS];
  __shared__ __attribute__((aligned(16))) unsigned rk[2][DP_SLOTS32];
  __shared__ __attribute__((aligned(16))) unsigned char ring[DP_RING_MAX * DP_ROW];
  __shared__ unsigned short ec[kDecodePoolBurst * 128];
  __shared__ unsigned short lut[256];
  __shared__ int ends[kDecodePoolBurst];
  __shared__ int lab[kDecodePoolBurst];
  const int tid = threadIdx.x, j = tid >> 1, half = tid & 1, C = g.rec.ncls, L = g.lag, RL = g.ring_rows;
  const int i = blockIdx.x, slot = sl.s[i];
  const int off = (int)ragged_off(rows.e[i]), K = (int)ragged_count(rows.e[i]);
  const bool owner = half == 0 && j < C;
  char* st = dp_state(g, slot);
  int* hdr = (int*)st;
  u64* keys = (u64*)(st + kDecodePoolHeaderWords * 4);
  unsigned char* gring = (unsigned char*)(st + g.ring_off);
  const int F = hdr[0], Cm = hdr[1], status = hdr[2];
  if (status & kDecodeFlushed) {                             // uniform.  Nothing is ingested: fillers, and the status says so
    for (int k = tid; k < K; k += 256) {
      if (labels) labels[off + k] = kDecodePending;
      if (now) now[off + k] = kDecodePending;
    }
    if (tid == 0) {
      if (commit) { commit[2 * i] = Cm; commit[2 * i + 1] = 0; }
      hdr[2] = status | kDecodePushedAfterFlush;
    }
    return;
  }
  // ---- the model: this thread's slice of column j and init[j] ----
  unsigned trk32[LEN];
  {
    const dp_i32x4* mt = (const dp_i32x4*)(g.model + 128 + ((size_t)(j < C ? j : 0) * 2 + half) * LEN);
#pragma unroll
    for (int m = 0; m < LEN / 4; ++m) {
      const dp_i32x4 w = mt[m];
      trk32[4 * m] = (w.x < 0 || j >= C) ? DP_INF32 : (unsigned)w.x << 7;
      trk32[4 * m + 1] = (w.y < 0 || j >= C) ? DP_INF32 : (unsigned)w.y << 7;
      trk32[4 * m + 2] = (w.z < 0 || j >= C) ? DP_INF32 : (unsigned)w.z << 7;
      trk32[4 * m + 3] = (w.w < 0 || j >= C) ? DP_INF32 : (unsigned)w.w << 7;
    }
  }
  const int ini = g.model[j];
  lut[tid] = kDecodeLut[tid];
  // every key slot starts as "no path" (decode.hip: no step may read a word this kernel did not write)
  for (int q = tid; q < 2 * DP_SLOTS; q += 256) (&dk[0][0])[q] = DP_INF;
  for (int q = tid; q < 2 * DP_SLOTS32; q += 256) (&rk[0][0])[q] = DP_INF32;
  const int r0 = F % RL;                                     // the ring row of the call's first frame
  const int rb16 = g.row_bytes >> 4;
  __syncthreads();
  // ---- staging: emission costs, the ring rows behind the call, zeros for the call's own rows, the keys ----
  for (int q = tid; q < K * C; q += 256) {
    const int r = q / C, c = q - r * C;
    const unsigned w = src[(size_t)(off + r) * (size_t)ld + c];
    ec[r * 128 + c] = (unsigned short)(COSTS ? dec_cost_of_word(w) : dec_cost_of_prob(w, lut));
  }
  {
    const int nold = F < L ? F : L;
    for (int q = tid; q < nold * rb16; q += 256) {
      const int fr = F - nold + q / rb16, part = q % rb16, row = fr % RL;
      ((u32x4*)(ring + row * DP_ROW))[part] = ((const u32x4*)(gring + (size_t)row * g.row_bytes))[part];
    }
    for (int q = tid; q < K * (DP_ROW / 16); q += 256) {
      int row = r0 + q / (DP_ROW / 16);
      row = row >= RL ? row - RL : row;
      ((u32x4*)(ring + row * DP_ROW))[q % (DP_ROW / 16)] = (u32x4){0u, 0u, 0u, 0u};
    }
  }
  if (F > 0 && owner) dk[(F - 1) & 1][dp_slot<LEN>(j)] = keys[j];
  __syncthreads();
  int k0 = 0;
  if (F == 0) {                                              // uniform.  Frame 0: d_0(j) = init[j] + e_0(j)
    if (owner) dk[0][dp_slot<LEN>(j)] = ini < 0 ? DP_INF : ((((u64)ini + (u64)ec[j]) << 7) | (u64)j);
    __syncthreads();
    k0 = 1;
  }
  // ---- which key width the call's steps run in (uniform: every wave sees the same keys) ----
  bool fast = false;
  u64 base7 = 0;
  if (k0 < K) {
    const int rb = (F + k0 + 1) & 1;
    u64 kmin, kmax;
    dp_key_range<LEN>(dk[rb], kmin, kmax);
    fast = kmin < DP_INF && (long long)((kmax >> 7) - (kmin >> 7)) < DP_FAST_SPREAD;
    base7 = (kmin >> 7) << 7;
    if (fast) {
      if (owner) { const u64 k = dk[rb][dp_slot<LEN>(j)]; rk[rb][dp_slot32<LEN>(j)] = k >= DP_INF ? DP_INF32 : (unsigned)(k - base7); }
      __syncthreads();
    }
  }
  // ---- forward ----
  for (int k = k0; k < K; ++k) {
    const int t = F + k, rb = (t + 1) & 1, wb = t & 1;
    int row = r0 + k;
    row = row >= RL ? row - RL : row;
    const unsigned e = ec[k * 128 + j];
    if (fast) {
      const u32x4* slice = (const u32x4*)&rk[rb][half * (LEN + 4)];
      u32x4 q[LEN / 4];
#pragma unroll
      for (int m = 0; m < LEN / 4; ++m) q[m] = slice[m];
      unsigned b0 = DP_INF32, b1 = DP_INF32, b2 = DP_INF32, b3 = DP_INF32;
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
        const bool none = best == DP_INF32;
        rk[wb][dp_slot32<LEN>(j)] = none ? DP_INF32 : ((((best >> 7) + e) << 7) | (unsigned)j);
        ring[row * DP_ROW + j] = none ? (unsigned char)0 : (unsigned char)(best & 127u);
      }
      if (tid >= 192 && k >= 1) {                            // e of the frame in front, off the other waves' path
        const int en = dp_end32<LEN>(rk[rb]);
        if (tid == 192) ends[k - 1] = en;
      }
    } else {
      const dp_u64x2* slice = (const dp_u64x2*)&dk[rb][half * (LEN + 2)];
      u64 b0 = DP_INF, b1 = DP_INF;
#pragma unroll
      for (int m = 0; m < LEN / 2; ++m) {
        const dp_u64x2 q = slice[m];
        const u64 t0 = trk32[2 * m] == DP_INF32 ? DP_INF : (u64)trk32[2 * m], t1 = trk32[2 * m + 1] == DP_INF32 ? DP_INF : (u64)trk32[2 * m + 1];
        const u64 c0 = q.x + t0, c1 = q.y + t1;
        b0 = c0 < b0 ? c0 : b0;
        b1 = c1 < b1 ? c1 : b1;
      }
      u64 best = b1 < b0 ? b1 : b0;
      const u64 other = (u64)__shfl_xor((long long)best, 1, 64);
      best = other < best ? other : best;
      if (owner) {
        const bool none = best >= DP_INF;
        dk[wb][dp_slot<LEN>(j)] = none ? DP_INF : ((((best >> 7) + (u64)e) << 7) | (u64)j);
        ring[row * DP_ROW + j] = none ? (unsigned char)0 : (unsigned char)(best & 127u);
      }
      if (tid >= 192 && k >= 1) {
        u64 kmin, kmax;
        dp_key_range<LEN>(dk[rb], kmin, kmax);
        if (tid == 192) ends[k - 1] = kmin >= DP_INF ? -1 : (int)(kmin & 127u);
      }
    }
    __syncthreads();
  }
  // ---- the call's last frame: back to the exact keys, its e_t, the total cost ----
  const int lb = (F + K - 1) & 1;
  if (fast) {
    if (owner) { const unsigned k = rk[lb][dp_slot32<LEN>(j)]; dk[lb][dp_slot<LEN>(j)] = k == DP_INF32 ? DP_INF : base7 + k; }
    __syncthreads();
  }
  u64 endkey, unused_max;
  dp_key_range<LEN>(dk[lb], endkey, unused_max);
  const int end_state = endkey >= DP_INF ? -1 : (int)(endkey & 127u);
  if (owner) keys[j] = dk[lb][dp_slot<LEN>(j)];
  if (tid == 0) ends[K - 1] = end_state;
  __syncthreads();
  // ---- commit: frame t - L from the chain that starts at e_t, the K walks side by side ----
  const int M = (F + K > L ? F + K - L : 0) - Cm;            // labels this call commits: Cm == max(0, F - L) for a slot not flushed
  if (tid < K) {
    const int t = F + tid;
    if (t >= L) {
      int s = ends[tid];
      if (s >= 0) {
        int row = r0 + tid;
        row = row >= RL ? row - RL : row;
        for (int u = 0; u < L; ++u) {
          const int p = ring[row * DP_ROW + s];
          s = p < C ? p : C - 1;
          row = row == 0 ? RL - 1 : row - 1;
        }
      }
      const int m = t - L - Cm;
      if (m >= 0 && m < kDecodePoolBurst) lab[m] = s;
    }
  }
  for (int q = tid; q < K * rb16; q += 256) {                // the call's ring rows to the slot
    int row = r0 + q / rb16;
    row = row >= RL ? row - RL : row;
    ((u32x4*)(gring + (size_t)row * g.row_bytes))[q % rb16] = ((const u32x4*)(ring + row * DP_ROW))[q % rb16];
  }
  __syncthreads();
  if (tid < K) {
    if (labels) labels[off + tid] = tid < M ? lab[tid] : kDecodePending;
    if (now) now[off + tid] = ends[tid];
  }
  if (tid == 0) {
    int* rec = pool_record(g.rec, slot);
    for (int m = 0; m < M; ++m) pool_vote_update(rec, g.rec, lab[m]);
    hdr[0] = F + K;
    hdr[1] = Cm + (M > 0 ? M : 0);
    hdr[2] = status | (end_state < 0 ? kDecodeDead : 0);
    hdr[3] = end_state;
    *(long long*)(hdr + 4) = end_state < 0 ? -1ll : (long long)(endkey >> 7);
    if (commit) { commit[2 * i] = Cm; commit[2 * i + 1] = M > 0 ? M : 0; }
  }
}

// the tail [committed, frames) from the chain that starts at e_{frames-1}, then the record's unfinished window; the slot is marked flushed
__global__ __launch_bounds__(256) void decode_pool_flush_kernel(const DecodePoolGeom g, const PoolSlots sl, int* __restrict__ labels,
                                                                int* __restrict__ commit) {
  __shared__ __attribute__((aligned(16))) unsigned char ring[DP_RING_MAX * DP_ROW];
  __shared__ int lab[kDecodePoolMaxLag];
  const int tid = threadIdx.x, C = g.rec.ncls, L = g.lag, RL = g.ring_rows, i = blockIdx.x, slot = sl.s[i];
  char* st = dp_state(g, slot);
  int* hdr = (int*)st;
  const unsigned char* gring = (const unsigned char*)(st + g.ring_off);
  const int F = hdr[0], Cm = hdr[1], status = hdr[2], end_state = hdr[3];
  int cnt = (status & kDecodeFlushed) ? 0 : F - Cm;
  cnt = cnt < 0 ? 0 : (cnt > L ? L : cnt);                   // 0 .. L by the push's invariant; clamped all the same
  const int rb16 = g.row_bytes >> 4;
  for (int q = tid; q < cnt * rb16; q += 256) {
    const int row = (F - cnt + q / rb16) % RL;
    ((u32x4*)(ring + row * DP_ROW))[q % rb16] = ((const u32x4*)(gring + (size_t)row * g.row_bytes))[q % rb16];
  }
  __syncthreads();
  if (tid == 0) {
    int s = (status & kDecodeDead) || end_state < 0 || end_state >= C ? -1 : end_state;
    int row = (F - 1 + RL) % RL;
    for (int m = cnt - 1; m >= 0; --m) {
      lab[m] = s;
      if (s >= 0 && m > 0) { const int p = ring[row * DP_ROW + s]; s = p < C ? p : C - 1; }
      row = row == 0 ? RL - 1 : row - 1;
    }
    int* rec = pool_record(g.rec, slot);
    for (int m = 0; m < cnt; ++m) pool_vote_update(rec, g.rec, lab[m]);
    pool_flush_window(rec, g.rec);
    if (!(status & kDecodeFlushed)) { hdr[1] = Cm + cnt; hdr[2] = status | kDecodeFlushed; }
    if (commit) { commit[2 * i] = Cm; commit[2 * i + 1] = cnt; }
  }
  __syncthreads();
  if (labels)
    for (int m = tid; m < L; m += 256) labels[(size_t)i * L + m] = m < cnt ? lab[m] : kDecodePending;
}

__global__ __launch_bounds__(256) void decode_pool_reset_kernel(const DecodePoolGeom g, const PoolSlots sl) {
  const int slot = sl.s[blockIdx.x];
  u32x4* st = (u32x4*)dp_state(g, slot);
  for (int k = threadIdx.x; k < (g.slot_bytes >> 4); k += 256) st[k] = (u32x4){0u, 0u, 0u, 0u};
  u32x4* rec = (u32x4*)pool_record(g.rec, slot);
  for (int k = threadIdx.x; k < (g.rec.rec_words >> 2); k += 256) rec[k] = (u32x4){0u, 0u, 0u, 0u};
}

// trans / init clamped into the block in the step's order: init [128], then word (j, i) = trans[i][j] for i < 2 len
__global__ __launch_bounds__(256) void decode_pool_model_kernel(const DecodePoolGeom g, const int* __restrict__ trans, const int* __restrict__ init) {
  const int C = g.rec.ncls, W = 2 * g.len, total = C * W;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 128) g.model[idx] = idx < C ? (init ? dec_model_word(init[idx]) : 0) : -1;
  if (idx < total) {
    const int j = idx / W, i = idx - j * W;
    g.model[128 + idx] = i < C ? dec_model_word(trans[(size_t)i * C + j]) : -1;
  }
}

int decode_pool_len(int C) { return 2 * 8 >= C ? 8 : 2 * 16 >= C ? 16 : 2 * 32 >= C ? 32 : 2 * 48 >= C ? 48 : 64; }

static bool dp_geom_ok(const DecodePoolGeom& g) {
  const int C = g.rec.ncls;
  return g.model && g.state && g.rec.rec && C >= 1 && C <= kDecodeMaxClasses && g.lag >= 0 && g.lag <= kDecodePoolMaxLag &&
         g.ring_rows == g.lag + kDecodePoolBurst && g.row_bytes >= C && g.row_bytes <= DP_ROW && (g.row_bytes & 15) == 0 &&
         g.len == decode_pool_len(C) && (g.slot_bytes & 15) == 0 && (g.ring_off & 15) == 0 &&
         g.ring_off >= kDecodePoolHeaderWords * 4 + g.rec.ncls_pad * 8 && g.slot_bytes >= g.ring_off + g.ring_rows * g.row_bytes &&
         (g.rec.rec_words & 3) == 0 && g.rec.window >= 1 && g.rec.capacity >= 1;
}

static bool dp_slots(const DecodePoolGeom& g, const int* slots, int n, PoolSlots* sl) {
  if (!dp_geom_ok(g) || !slots || n < 1 || n > kPoolMaxActive) return false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= g.rec.capacity) return false;
    sl->s[i] = slots[i];
  }
  for (int i = n; i < kPoolMaxActive; ++i) sl->s[i] = 0;
  return true;
}

int launch_decode_pool_model(const DecodePoolGeom& g, const int* trans, const int* init, hipStream_t s) {
  if (!dp_geom_ok(g) || !trans) return -1;
  const int total = g.rec.ncls * 2 * g.len;
  decode_pool_model_kernel<<<((total > 128 ? total : 128) + 255) / 256, 256, 0, s>>>(g, trans, init);
  return 0;
}

template <bool COSTS> static void dp_launch(const DecodePoolGeom& g, const PoolSlots& sl, int n, const RaggedMap& rows, const unsigned* src,
                                            long long ld, int* labels, int* commit, int* now, hipStream_t s) {
  switch (g.len) {
    case 8: decode_pool_push_kernel<8, COSTS><<<n, 256, 0, s>>>(g, sl, rows, src, ld, labels, commit, now); break;
    case 16: decode_pool_push_kernel<16, COSTS><<<n, 256, 0, s>>>(g, sl, rows, src, ld, labels, commit, now); break;
    case 32: decode_pool_push_kernel<32, COSTS><<<n, 256, 0, s>>>(g, sl, rows, src, ld, labels, commit, now); break;
    case 48: decode_pool_push_kernel<48, COSTS><<<n, 256, 0, s>>>(g, sl, rows, src, ld, labels, commit, now); break;
    default: decode_pool_push_kernel<64, COSTS><<<n, 256, 0, s>>>(g, sl, rows, src, ld, labels, commit, now); break;
  }
}

int launch_decode_pool_push(const DecodePoolGeom& g, bool costs, const int* slots, int n, const RaggedMap& rows, int n_rows, const void* src,
                            long long ld, int* labels, int* commit, int* now, hipStream_t s) {
  PoolSlots sl;
  if (!src || ld < g.rec.ncls || n_rows < n || n_rows > kPoolMaxActive || !dp_slots(g, slots, n, &sl)) return -1;
  for (int i = 0; i < n; ++i)
    if (ragged_count(rows.e[i]) < 1u || ragged_count(rows.e[i]) > (unsigned)kDecodePoolBurst ||
        ragged_off(rows.e[i]) + ragged_count(rows.e[i]) > (unsigned)n_rows) return -1;
  if (costs) dp_launch<true>(g, sl, n, rows, (const unsigned*)src, ld, labels, commit, now, s);
  else dp_launch<false>(g, sl, n, rows, (const unsigned*)src, ld, labels, commit, now, s);
  return 0;
}

int launch_decode_pool_flush(const DecodePoolGeom& g, const int* slots, int n, int* labels, int* commit, hipStream_t s) {
  PoolSlots sl;
  if (!dp_slots(g, slots, n, &sl)) return -1;
  decode_pool_flush_kernel<<<n, 256, 0, s>>>(g, sl, labels, commit);
  return 0;
}

int launch_decode_pool_reset(const DecodePoolGeom& g, const int* slots, int n, hipStream_t s) {
  PoolSlots sl;
  if (!dp_slots(g, slots, n, &sl)) return -1;
  decode_pool_reset_kernel<<<n, 256, 0, s>>>(g, sl);
  return 0;
}
