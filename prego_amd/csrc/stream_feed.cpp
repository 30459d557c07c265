// Host side of a stream pool's event feed (include/prego_amd.h: prego_stream_pool_feed_*; kernels: stream_feed.hip).  The feed object is
// host memory only: a copy of the pool's record geometry, the addresses inside the caller's feed block and a stamp table for forget's
// duplicate check.  Both pool types keep their records in a PoolGeom, so one feed serves both.  Every entry point decides all its
// refusals before its first launch, so a refused call has written nothing.
#include "pool_slot_check.h"

#include <cstdint>

struct prego_stream_pool_feed {
  PoolGeom g;                            // the pool's records (read only)
  FeedGeom f;
  size_t bytes;                          // of the feed block, as laid out
  SlotStamps stamps;
};

const PoolGeom* stream_pool_feed_pool(const prego_stream_pool_feed* f) { return &f->g; }      // pool_slot_check.h
const FeedGeom* stream_pool_feed_geom(const prego_stream_pool_feed* f) { return &f->f; }

namespace {
constexpr int kFeedMaxOut = 1 << 24;

// block: cursor [capacity] int32 | seq (one word) | wg_due [ceil(capacity / 256)] int32, each part 256-byte aligned
struct FeedLayout { size_t seq, wg_due, total; };
FeedLayout feed_layout(int capacity) {
  FeedLayout l{};
  l.seq = align_up((size_t)capacity * 4, 256);
  l.wg_due = l.seq + 256;
  l.total = l.wg_due + align_up(((size_t)capacity + kFeedWg - 1) / kFeedWg * 4, 256);
  return l;
}
size_t report_bytes(int max_out) { return align_up(((size_t)max_out + 1) * 16, 256); }

int feed_create(const char* who, prego_stream_pool_feed** out, const PoolGeom* g, int max_out, void* device_block, size_t bytes,
                prego_stream_t stream) {
  if (!out) return prego_fail_(PREGO_EINVAL, "%s: out is NULL", who);
  *out = nullptr;
  if (!g) return prego_fail_(PREGO_EINVAL, "%s: pool is NULL", who);
  if (max_out < 1 || max_out > kFeedMaxOut) return prego_fail_(PREGO_EINVAL, "%s: max_out %d (1..%d entries per report)", who, max_out, kFeedMaxOut);
  const FeedLayout l = feed_layout(g->capacity);
  if (!device_block) return prego_fail_(PREGO_EINVAL, "%s: block is NULL", who);
  if ((uintptr_t)device_block & 255) return prego_fail_(PREGO_EINVAL, "%s: the block must be 256-byte aligned", who);
  if (bytes < l.total)
    return prego_fail_(PREGO_EWORKSPACE, "%s: block with %zu bytes, a feed over %d slots need %zu (prego_stream_pool_feed_bytes)", who, bytes,
                       g->capacity, l.total);
  prego_stream_pool_feed* fd = new prego_stream_pool_feed();
  char* base = (char*)device_block;
  fd->g = *g;
  fd->f = FeedGeom{(int*)base, (int*)(base + l.seq), (int*)(base + l.wg_due), max_out};
  fd->bytes = l.total;
  fd->stamps.stamp.assign((size_t)g->capacity, 0u);
  const hipError_t e = hipMemsetAsync(device_block, 0, l.total, (hipStream_t)stream);      // every cursor at 0, seq 0
  if (e != hipSuccess) {
    delete fd;
    return prego_fail_(PREGO_EHIP, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(e));
  }
  *out = fd;
  return PREGO_OK;
}
}  // namespace

extern "C" size_t prego_stream_pool_feed_bytes(int capacity, int max_out) {
  if (capacity < 1 || max_out < 1 || max_out > kFeedMaxOut) return 0;
  return feed_layout(capacity).total;
}

extern "C" size_t prego_stream_pool_feed_report_bytes(int max_out) {
  if (max_out < 1 || max_out > kFeedMaxOut) return 0;
  return report_bytes(max_out);
}

extern "C" int prego_stream_pool_feed_create(prego_stream_pool_feed** out, const prego_stream_pool* p, int max_out, void* device_block,
                                             size_t bytes, prego_stream_t stream) {
  return feed_create("stream_pool_feed_create", out, p ? stream_pool_geom(p) : nullptr, max_out, device_block, bytes, stream);
}

extern "C" int prego_vit_stream_pool_feed_create(prego_stream_pool_feed** out, const prego_vit_stream_pool* p, int max_out,
                                                 void* device_block, size_t bytes, prego_stream_t stream) {
  return feed_create("vit_stream_pool_feed_create", out, p ? vit_stream_pool_geom(p) : nullptr, max_out, device_block, bytes, stream);
}

extern "C" int prego_decode_pool_feed_create(prego_stream_pool_feed** out, const prego_decode_pool* p, int max_out, void* device_block,
                                             size_t bytes, prego_stream_t stream) {
  return feed_create("decode_pool_feed_create", out, p ? decode_pool_geom(p) : nullptr, max_out, device_block, bytes, stream);
}

extern "C" void prego_stream_pool_feed_destroy(prego_stream_pool_feed* f) { delete f; }

extern "C" int prego_stream_pool_feed_drain(prego_stream_pool_feed* f, void* report, size_t report_bytes_, prego_stream_t stream) {
  if (!f) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_drain: feed is NULL");
  if (!report) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_drain: report is NULL");
  if ((uintptr_t)report & 255) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_drain: the report must be 256-byte aligned");
  const size_t need = report_bytes(f->f.max_out);
  if (report_bytes_ < need)
    return prego_fail_(PREGO_EWORKSPACE, "stream_pool_feed_drain: report with %zu bytes, %d entries need %zu (prego_stream_pool_feed_report_bytes)",
                       report_bytes_, f->f.max_out, need);
  if (launch_feed_drain(f->g, f->f, (int*)report, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_drain: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_stream_pool_feed_forget(prego_stream_pool_feed* f, int n, const int32_t* slots, prego_stream_t stream) {
  if (!f) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_forget: feed is NULL");
  if (int rc = check_slot_list(f->stamps, f->g.capacity, "stream_pool_feed_forget", n, slots)) return rc;
  if (launch_feed_forget(f->f, f->g.capacity, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "stream_pool_feed_forget: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
