// Slot images of the stream pools (prego_stream_pool_snapshot / _restore and their prego_vit_ counterparts; host side: stream_image.cpp;
// the layout and the validity rule: pool_image.h).  Both pool types through PoolGeom plus ImageRing, as stream_feed.hip serves both:
//   pool_snapshot  images[i] <- slot slots[i]: tag, state (GRU: the state row; Transformer: the ring, rows that fill does not cover as
//                  zeros - the block's stale bytes are never read), record, zero padding.  The pool and the feed's cursors are only read
//   pool_restore   slot slots[i] <- images[i]: state or ring, ring words, record and (a feed named) the cursor word, where the image
//                  passes pool_image_fault; an image that does not leaves its slot and cursor byte for byte as they were
// Grid: (chunks, n) workgroups of 256 lanes, a chunk = kImageChunkVecs 16-byte vectors of the image (64 KB), so a GRU image is one
// workgroup and an 8 MB ring 128.  Every workgroup of a restored slot evaluates the rule itself from the image's tag, record header
// and counters (at most 150 words that no launch of this file writes): all reach the same verdict, no atomic, no workgroup waits for
// another, and nothing of a slot is written before its verdict.  Workgroup 0 of a slot writes status, the ring words and the cursor.
// Memory policy: each byte is read once and written once.  The source side (the ring for a snapshot, the image for a restore) is loaded
// non-temporally - it bypasses L1 and is served by L2 like a plain load; an image is stored non-temporally as well (nobody on the device
// reads it next), while a restored slot is stored plainly: the next push reads it.
#include "common.h"
#include "kernels.h"
#include "pool_image.h"

namespace {
__device__ __forceinline__ int image_tag_word(const PoolGeom& g, const PoolImageDims& d, bool vit, const int* __restrict__ cursor, int slot,
                                              int k) {
  if (k < 8) return pool_image_geometry_word(d, k);
  if (k == kTagFrames) return g.rec[(size_t)slot * g.rec_words];
  if (k == kTagHead) return vit ? ((const int*)g.h)[(size_t)slot * kVitRingStateWords] : 0;
  if (k == kTagFill) return vit ? ((const int*)g.h)[(size_t)slot * kVitRingStateWords + 1] : 0;
  if (k == kTagCursor) return cursor ? cursor[slot] : 0;
  return 0;
}
}  // namespace

__global__ __launch_bounds__(256) void pool_snapshot_kernel(PoolGeom g, ImageRing r, PoolImageDims d, const int* __restrict__ cursor,
                                                            PoolSlots sl, int* __restrict__ images) {
  const int i = blockIdx.y, slot = sl.s[i];
  const bool vit = r.ring != nullptr;
  const int V = d.image_words >> 2, tv = kPoolImageTagWords >> 2, sv = d.state_words >> 2, rv = d.rec_words >> 2;
  const int v0 = blockIdx.x * kImageChunkVecs, v1 = min(v0 + kImageChunkVecs, V);
  u32x4* dst = (u32x4*)(images + (size_t)i * d.image_words);
  const u32x4* rec = (const u32x4*)(g.rec + (size_t)slot * g.rec_words);
  const u32x4* state = vit ? (const u32x4*)(r.ring + (size_t)slot * r.T * r.E) : (const u32x4*)(g.h + (size_t)slot * g.hid);
  int covered = sv;                                           // state vectors that hold the stream: the GRU row, the ring rows [0, fill)
  if (vit) covered = min(max(((const int*)g.h)[(size_t)slot * kVitRingStateWords + 1], 0), r.T) * (r.E >> 2);
  for (int v = v0 + threadIdx.x; v < v1; v += 256) {
    u32x4 w = (u32x4){0u, 0u, 0u, 0u};
    if (v < tv) {
      w = (u32x4){(unsigned)image_tag_word(g, d, vit, cursor, slot, 4 * v), (unsigned)image_tag_word(g, d, vit, cursor, slot, 4 * v + 1),
                  (unsigned)image_tag_word(g, d, vit, cursor, slot, 4 * v + 2), (unsigned)image_tag_word(g, d, vit, cursor, slot, 4 * v + 3)};
    } else if (v < tv + sv) {
      if (v - tv < covered) w = __builtin_nontemporal_load(state + (v - tv));
    } else if (v < tv + sv + rv) {
      w = rec[v - tv - sv];
    }
    __builtin_nontemporal_store(w, dst + v);
  }
}

__global__ __launch_bounds__(256) void pool_restore_kernel(PoolGeom g, ImageRing r, PoolImageDims d, int* __restrict__ cursor, PoolSlots sl,
                                                           const int* __restrict__ images, int* __restrict__ status) {
  __shared__ int wave_fault[4];
  const int i = blockIdx.y, slot = sl.s[i];
  const bool vit = r.ring != nullptr;
  const int* img = images + (size_t)i * d.image_words;
  const int* rec_img = img + kPoolImageTagWords + d.state_words;
  // the verdict, from words this launch never writes: every workgroup of the slot computes the same one
  int f = pool_image_fault_words(d, img, rec_img);
  for (int c = threadIdx.x; c < d.ncls_pad; c += 256) f |= pool_image_fault_counter(d, rec_img[kPoolImageRecHeader + c]);
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) f |= __shfl_xor(f, k, 64);
  if ((threadIdx.x & 63) == 0) wave_fault[threadIdx.x >> 6] = f;
  __syncthreads();
  const int fault = wave_fault[0] | wave_fault[1] | wave_fault[2] | wave_fault[3];
  if (blockIdx.x == 0 && threadIdx.x == 0 && status) status[i] = fault;
  if (fault) return;                                          // nothing of the slot is written

  const int tv = kPoolImageTagWords >> 2, sv = d.state_words >> 2, rv = d.rec_words >> 2;
  const int v0 = max(blockIdx.x * kImageChunkVecs, tv), v1 = min(blockIdx.x * kImageChunkVecs + kImageChunkVecs, tv + sv + rv);
  const u32x4* src = (const u32x4*)img;
  u32x4* rec = (u32x4*)(g.rec + (size_t)slot * g.rec_words);
  u32x4* state = vit ? (u32x4*)(r.ring + (size_t)slot * r.T * r.E) : (u32x4*)(g.h + (size_t)slot * g.hid);
  for (int v = v0 + threadIdx.x; v < v1; v += 256) {
    const u32x4 w = __builtin_nontemporal_load(src + v);
    if (v < tv + sv) state[v - tv] = w;
    else rec[v - tv - sv] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (vit) *(u32x4*)((int*)g.h + (size_t)slot * kVitRingStateWords) = (u32x4){(unsigned)img[kTagHead], (unsigned)img[kTagFill], 0u, 0u};
    if (cursor) cursor[slot] = img[kTagCursor];
  }
}

// what both launchers refuse: the geometry the kernels index by must be the pool's own
static bool image_args(const PoolGeom& g, const ImageRing& r, const PoolImageDims& d, const int* slots, int n, const void* images,
                       PoolSlots* sl) {
  if (!g.h || !g.rec || !slots || !images || ((size_t)images & 15) || n < 1 || n > kPoolMaxActive || n > g.capacity) return false;
  if ((g.hid & 3) || (g.rec_words & 3) || g.rec_words < kPoolRecHeader + g.ncls_pad || d.rec_words != g.rec_words || d.ncls_pad != g.ncls_pad)
    return false;
  if (r.ring ? (r.T < 1 || r.E < 4 || (r.E & 3) || g.hid != kVitRingStateWords || d.kind != kPoolImageVit || d.window_size != r.T ||
                d.dim != r.E || (long long)r.T * r.E != d.state_words)
             : (d.kind != kPoolImageGru || d.dim != g.hid || d.state_words != g.hid)) return false;
  if ((d.image_words & 63) || (long long)d.image_words < (long long)kPoolImageTagWords + d.state_words + d.rec_words) return false;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= g.capacity) return false;
    sl->s[i] = slots[i];
  }
  for (int i = n; i < kPoolMaxActive; ++i) sl->s[i] = 0;
  return true;
}

int launch_pool_snapshot(const PoolGeom& g, const ImageRing& r, const PoolImageDims& d, const int* cursor, const int* slots, int n,
                         int* images, hipStream_t s) {
  PoolSlots sl;
  if (!image_args(g, r, d, slots, n, images, &sl)) return -1;
  const int chunks = ((d.image_words >> 2) + kImageChunkVecs - 1) / kImageChunkVecs;
  pool_snapshot_kernel<<<dim3(chunks, n), 256, 0, s>>>(g, r, d, cursor, sl, images);
  return 0;
}

int launch_pool_restore(const PoolGeom& g, const ImageRing& r, const PoolImageDims& d, int* cursor, const int* slots, int n,
                        const int* images, int* status, hipStream_t s) {
  PoolSlots sl;
  if (!image_args(g, r, d, slots, n, images, &sl)) return -1;
  const int chunks = (((kPoolImageTagWords + d.state_words + d.rec_words) >> 2) + kImageChunkVecs - 1) / kImageChunkVecs;      // not the padding
  pool_restore_kernel<<<dim3(chunks, n), 256, 0, s>>>(g, r, d, cursor, sl, images, status);
  return 0;
}
