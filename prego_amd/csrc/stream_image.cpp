// Host side of the stream pools' slot images (include/prego_amd.h: prego_stream_pool_image_bytes / _snapshot / _restore and their
// prego_vit_ counterparts; kernels: stream_image.hip; layout and validity rule: pool_image.h).  Both pool types go through one
// implementation on their PoolGeom, the Transformer pool adding its ring.  Every entry point decides all its refusals before its one
// launch, so a refused call has written nothing; nothing here allocates device memory or waits on the host.
#include "pool_image.h"
#include "pool_slot_check.h"

#include <cstdint>

namespace {
// one pool of either type as the image code sees it
struct ImagePool {
  const PoolGeom* g;
  ImageRing r;
  SlotStamps* stamps;
  PoolBlock block;
};
ImagePool image_pool(prego_stream_pool* p) {
  return ImagePool{stream_pool_geom(p), ImageRing{nullptr, 0, 0}, stream_pool_stamps(p), stream_pool_block(p)};
}
ImagePool image_pool(prego_vit_stream_pool* p) {
  const VitRing* r = vit_stream_pool_ring(p);
  return ImagePool{vit_stream_pool_geom(p), ImageRing{r->ring, r->T, r->E}, vit_stream_pool_stamps(p), vit_stream_pool_block(p)};
}

// false: an image of this pool would not fit the int word counts of the kernels (a ring of 8 GB or more per slot)
bool image_dims(const ImagePool& ip, PoolImageDims* d) {
  const PoolGeom& g = *ip.g;
  const bool vit = ip.r.ring != nullptr;
  const unsigned long long state = vit ? (unsigned long long)ip.r.T * (unsigned long long)ip.r.E : (unsigned long long)g.hid;
  if (state + (unsigned long long)g.rec_words + kPoolImageTagWords + 64 > 0x7fffffffull) return false;
  *d = pool_image_dims(vit ? kPoolImageVit : kPoolImageGru, vit ? ip.r.E : g.hid, vit ? ip.r.T : 0, g.ncls, g.ncls_pad, g.window, g.max_events,
                       g.rec_words);
  return true;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// the refusals both calls share; on success *d and *cursor (the feed's cursor words, nullptr without a feed) are set
int image_refusals(const char* who, const ImagePool& ip, const prego_stream_pool_feed* feed, int n, const int32_t* slots, const void* images,
                   size_t bytes, PoolImageDims* d, int** cursor) {
  if (!image_dims(ip, d)) return prego_fail_(PREGO_EINVAL, "%s: a slot of this pool is too large for an image", who);
  *cursor = nullptr;
  if (feed) {
    const PoolGeom* fg = stream_pool_feed_pool(feed);
    if (fg->rec != ip.g->rec || fg->capacity != ip.g->capacity)
      return prego_fail_(PREGO_EINVAL, "%s: the feed belongs to another pool", who);
    *cursor = stream_pool_feed_geom(feed)->cursor;
  }
  if (int rc = check_slot_list(*ip.stamps, ip.g->capacity, who, n, slots)) return rc;
  if (!images) return prego_fail_(PREGO_EINVAL, "%s: images is NULL", who);
  if ((uintptr_t)images & 255) return prego_fail_(PREGO_EINVAL, "%s: the images must be 256-byte aligned", who);
  const size_t each = (size_t)d->image_words * 4;
  if (bytes / each < (size_t)n)
    return prego_fail_(PREGO_EWORKSPACE, "%s: images with %zu bytes, %d images of %zu bytes need %zu (prego_stream_pool_image_bytes)", who, bytes,
                       n, each, (size_t)n * each);
  if (overlap(images, (size_t)n * each, ip.block.base, ip.block.bytes))
    return prego_fail_(PREGO_EINVAL, "%s: the images overlap the pool's block", who);
  if (*cursor && overlap(images, (size_t)n * each, *cursor, (size_t)ip.g->capacity * 4))
    return prego_fail_(PREGO_EINVAL, "%s: the images overlap the feed's block", who);
  return 0;
}

size_t image_bytes(const ImagePool& ip) {
  PoolImageDims d;
  return image_dims(ip, &d) ? (size_t)d.image_words * 4 : 0;
}

int snapshot(const char* who, const ImagePool& ip, const prego_stream_pool_feed* feed, int n, const int32_t* slots, void* images, size_t bytes,
             prego_stream_t stream) {
  PoolImageDims d;
  int* cursor;
  if (int rc = image_refusals(who, ip, feed, n, slots, images, bytes, &d, &cursor)) return rc;
  if (launch_pool_snapshot(*ip.g, ip.r, d, cursor, slots, n, (int*)images, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

int restore(const char* who, const ImagePool& ip, prego_stream_pool_feed* feed, int n, const int32_t* slots, const void* images, size_t bytes,
            int32_t* status, prego_stream_t stream) {
  PoolImageDims d;
  int* cursor;
  if (int rc = image_refusals(who, ip, feed, n, slots, images, bytes, &d, &cursor)) return rc;
  if (status && ((uintptr_t)status & 3)) return prego_fail_(PREGO_EINVAL, "%s: status must be 4-byte aligned", who);
  if (status && (overlap(status, (size_t)n * 4, images, (size_t)n * d.image_words * 4) ||
                 overlap(status, (size_t)n * 4, ip.block.base, ip.block.bytes)))
    return prego_fail_(PREGO_EINVAL, "%s: status overlaps the images or the pool's block", who);
  if (launch_pool_restore(*ip.g, ip.r, d, cursor, slots, n, (const int*)images, (int*)status, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" size_t prego_stream_pool_image_bytes(const prego_stream_pool* p) {
  return p ? image_bytes(image_pool(const_cast<prego_stream_pool*>(p))) : 0;
}

extern "C" int prego_stream_pool_snapshot(prego_stream_pool* p, const prego_stream_pool_feed* feed, int n, const int32_t* slots, void* images,
                                          size_t bytes, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "stream_pool_snapshot: pool is NULL");
  return snapshot("stream_pool_snapshot", image_pool(p), feed, n, slots, images, bytes, stream);
}

extern "C" int prego_stream_pool_restore(prego_stream_pool* p, prego_stream_pool_feed* feed, int n, const int32_t* slots, const void* images,
                                         size_t bytes, int32_t* status, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "stream_pool_restore: pool is NULL");
  return restore("stream_pool_restore", image_pool(p), feed, n, slots, images, bytes, status, stream);
}

extern "C" size_t prego_vit_stream_pool_image_bytes(const prego_vit_stream_pool* p) {
  return p ? image_bytes(image_pool(const_cast<prego_vit_stream_pool*>(p))) : 0;
}

extern "C" int prego_vit_stream_pool_snapshot(prego_vit_stream_pool* p, const prego_stream_pool_feed* feed, int n, const int32_t* slots,
                                              void* images, size_t bytes, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_snapshot: pool is NULL");
  return snapshot("vit_stream_pool_snapshot", image_pool(p), feed, n, slots, images, bytes, stream);
}

extern "C" int prego_vit_stream_pool_restore(prego_vit_stream_pool* p, prego_stream_pool_feed* feed, int n, const int32_t* slots,
                                             const void* images, size_t bytes, int32_t* status, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_restore: pool is NULL");
  return restore("vit_stream_pool_restore", image_pool(p), feed, n, slots, images, bytes, status, stream);
}

#ifdef PREGO_DEBUG_ABI
// unit-test hook, no device: pool_image_fault on HOST words (tag[16], rec[4 + ncls_pad]) for a geometry given as
// kind | dim | window_size | n_classes | vote window | max_events - the C++ statement of the rule, for the Python model to be held against
extern "C" int prego_debug_pool_image_fault(const int32_t* geometry6, const int32_t* tag, const int32_t* rec) {
  if (!geometry6 || !tag || !rec) return -1;
  const int ncls_pad = (int)align_up((size_t)geometry6[3], 4);
  const int rec_words = (int)align_up((size_t)kPoolRecHeader + ncls_pad + 2 * (size_t)geometry6[5], 4);
  const PoolImageDims d = pool_image_dims(geometry6[0], geometry6[1], geometry6[2], geometry6[3], ncls_pad, geometry6[4], geometry6[5], rec_words);
  return pool_image_fault(d, tag, rec);
}
#endif
