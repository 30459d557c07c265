// Host side of the decode pool (include/prego_amd.h: prego_decode_pool_*; kernels: decode_pool.hip).  The pool object is host memory
// only: the geometry, the addresses inside the caller's device block and a stamp table for the duplicate check.  Every entry point decides
// all its refusals before its first launch, so a refused call has written nothing; nothing is allocated on the device, nothing waits.
#include "pool_slot_check.h"
#ifdef PREGO_DEBUG_ABI
#include "miniroad_handle.h"      // the allocation / wait counters of prego_debug_alloc_count cover these entries as well
#endif

#include <cstdint>

static_assert(kDecodePoolMaxLag == PREGO_DECODE_POOL_MAX_LAG && kDecodePending == PREGO_DECODE_PENDING,
              "the header documents the kernel's constants");

struct prego_decode_pool {
  DecodePoolGeom g;
  char* block;
  size_t bytes;                          // of the block, as laid out
  SlotStamps stamps;
};
const PoolGeom* decode_pool_geom(const prego_decode_pool* p) { return &p->g.rec; }      // pool_slot_check.h

namespace {
// block: model | slots [capacity][slot_bytes] | records [capacity][rec_words] int32, each part 256-byte aligned
struct DecodeLayout { size_t state, rec, total; int len, row_bytes, ring_rows, ring_off, slot_bytes, ncls_pad, rec_words; };

DecodeLayout decode_layout(int capacity, int C, int lag, int max_events) {
  DecodeLayout l{};
  l.len = decode_pool_len(C);
  l.ncls_pad = (int)align_up((size_t)C, 4);
  l.row_bytes = (int)align_up((size_t)C, 16);
  l.ring_rows = lag + kDecodePoolBurst;
  l.ring_off = kDecodePoolHeaderWords * 4 + l.ncls_pad * 8;
  l.slot_bytes = (int)align_up((size_t)l.ring_off + (size_t)l.ring_rows * l.row_bytes, 256);
  l.rec_words = (int)align_up((size_t)kPoolRecHeader + l.ncls_pad + 2 * (size_t)max_events, 4);
  l.state = align_up((128 + (size_t)C * 2 * l.len) * 4, 256);
  l.rec = l.state + (size_t)capacity * l.slot_bytes;
  l.total = l.rec + align_up((size_t)capacity * l.rec_words * 4, 256);
  return l;
}

bool shape_ok(int capacity, int C, int lag, int max_events) {
  return capacity >= 1 && capacity <= (1 << 20) && max_events >= 1 && max_events <= (1 << 20) && C >= 1 && C <= kDecodeMaxClasses && lag >= 0 &&
         lag <= kDecodePoolMaxLag;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte (an empty or NULL range shares none)
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na > 0 && nb > 0 && x < y + nb && y < x + na;
}

struct Range { const void* p; size_t n; const char* name; };
// the outputs (nullable) against the inputs and each other
int outputs_ok(const char* who, const Range* out, int n_out, const Range* in, int n_in) {
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      if (overlap(out[o].p, out[o].n, in[i].p, in[i].n))
        return prego_fail_(PREGO_EINVAL, "%s: %s must not overlap %s", who, out[o].name, in[i].name);
    for (int q = o + 1; q < n_out; ++q)
      if (overlap(out[o].p, out[o].n, out[q].p, out[q].n))
        return prego_fail_(PREGO_EINVAL, "%s: %s must not overlap %s", who, out[o].name, out[q].name);
  }
  return 0;
}

int push_entry(const char* who, bool costs, prego_decode_pool* p, int n, const int32_t* slots, const int32_t* counts, const void* rows, int64_t ld,
               int32_t* labels, int32_t* commit, int32_t* now, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "%s: pool is NULL", who);
  const int C = p->g.rec.ncls;
  if (!rows) return prego_fail_(PREGO_EINVAL, "%s: the rows are NULL", who);
  if (ld < C) return prego_fail_(PREGO_EINVAL, "%s: ld %lld (>= n_classes %d)", who, (long long)ld, C);
  if (n >= 1 && n <= kPoolMaxActive && !counts) return prego_fail_(PREGO_EINVAL, "%s: counts is NULL", who);
  RaggedMap map{};
  long long R = 0;
  if (counts && n >= 1 && n <= kPoolMaxActive) {
    for (int i = 0; i < n; ++i) {
      if (counts[i] < 1 || counts[i] > kDecodePoolBurst)
        return prego_fail_(PREGO_EINVAL, "%s: counts[%d] = %d (1..%d frames per slot per call)", who, i, counts[i], kDecodePoolBurst);
      map.e[i] = ragged_entry((unsigned)R, (unsigned)(i & 0xff), (unsigned)counts[i]);
      R += counts[i];
    }
    if (R > kPoolMaxActive) return prego_fail_(PREGO_EINVAL, "%s: the counts sum to %lld rows (at most %d per call)", who, R, kPoolMaxActive);
  }
  if (int rc = check_slot_list(p->stamps, p->g.rec.capacity, who, n, slots)) return rc;
  const Range in[2] = {{rows, ((size_t)(R - 1) * (size_t)ld + (size_t)C) * 4, "the rows"}, {p->block, p->bytes, "the pool's block"}};
  const Range out[3] = {{labels, (size_t)R * 4, "labels"}, {commit, (size_t)n * 8, "commit"}, {now, (size_t)R * 4, "now"}};
  if (int rc = outputs_ok(who, out, 3, in, 2)) return rc;
  if (launch_decode_pool_push(p->g, costs, slots, n, map, (int)R, rows, ld, labels, commit, now, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" size_t prego_decode_pool_bytes(int capacity, int n_classes, int lag, int max_events) {
  if (!shape_ok(capacity, n_classes, lag, max_events)) return 0;
  return decode_layout(capacity, n_classes, lag, max_events).total;
}

extern "C" int prego_decode_pool_create(prego_decode_pool** out, int capacity, int n_classes, int lag, int vote_window, int max_events,
                                        const int32_t* trans, const int32_t* init, void* device_block, size_t bytes, prego_stream_t stream) {
  const char* who = "decode_pool_create";
  if (!out) return prego_fail_(PREGO_EINVAL, "%s: out is NULL", who);
  *out = nullptr;
  if (n_classes < 1 || n_classes > kDecodeMaxClasses) return prego_fail_(PREGO_EINVAL, "%s: n_classes %d (1..%d)", who, n_classes, kDecodeMaxClasses);
  if (lag < 0 || lag > kDecodePoolMaxLag) return prego_fail_(PREGO_EINVAL, "%s: lag %d (0..%d)", who, lag, kDecodePoolMaxLag);
  if (vote_window < 1) return prego_fail_(PREGO_EINVAL, "%s: vote_window %d (>= 1)", who, vote_window);
  if (!shape_ok(capacity, n_classes, lag, max_events))
    return prego_fail_(PREGO_EINVAL, "%s: capacity %d, max_events %d (each 1..%d)", who, capacity, max_events, 1 << 20);
  if (!trans) return prego_fail_(PREGO_EINVAL, "%s: trans is NULL", who);
  const DecodeLayout l = decode_layout(capacity, n_classes, lag, max_events);
  if (!device_block || bytes < l.total)
    return prego_fail_(PREGO_EINVAL, "%s: block %p with %zu bytes, %d slots of %d classes, lag %d and %d events need %zu (prego_decode_pool_bytes)",
                       who, device_block, bytes, capacity, n_classes, lag, max_events, l.total);
  if ((uintptr_t)device_block & 255) return prego_fail_(PREGO_EINVAL, "%s: the block must be 256-byte aligned", who);
  if (overlap(device_block, l.total, trans, (size_t)n_classes * n_classes * 4) || overlap(device_block, l.total, init, (size_t)n_classes * 4))
    return prego_fail_(PREGO_EINVAL, "%s: trans and init must not lie in the block", who);
  prego_decode_pool* p = new prego_decode_pool();
  char* base = (char*)device_block;
  p->g.rec = PoolGeom{nullptr, (int*)(base + l.rec), 0, n_classes, l.ncls_pad, vote_window, max_events, l.rec_words, capacity};
  p->g.model = (int*)base;
  p->g.state = base + l.state;
  p->g.lag = lag; p->g.ring_rows = l.ring_rows; p->g.row_bytes = l.row_bytes; p->g.len = l.len; p->g.ring_off = l.ring_off;
  p->g.slot_bytes = l.slot_bytes;
  p->block = base;
  p->bytes = l.total;
  p->stamps.stamp.assign((size_t)capacity, 0u);
  const hipError_t e = hipMemsetAsync(device_block, 0, l.total, (hipStream_t)stream);      // every slot empty: open launches nothing
  if (e != hipSuccess) {
    delete p;
    return prego_fail_(PREGO_EHIP, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(e));
  }
  if (launch_decode_pool_model(p->g, (const int*)trans, (const int*)init, (hipStream_t)stream)) {
    delete p;
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  }
  *out = p;
  return PREGO_OK;
}

extern "C" void prego_decode_pool_destroy(prego_decode_pool* p) { delete p; }

extern "C" int prego_decode_pool_push(prego_decode_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* probs, int64_t ld,
                                      int32_t* labels, int32_t* commit, int32_t* now, prego_stream_t stream) {
  return push_entry("decode_pool_push", false, p, n, slots, counts, probs, ld, labels, commit, now, stream);
}

extern "C" int prego_decode_pool_push_costs(prego_decode_pool* p, int n, const int32_t* slots, const int32_t* counts, const int32_t* costs,
                                            int64_t ld, int32_t* labels, int32_t* commit, int32_t* now, prego_stream_t stream) {
  return push_entry("decode_pool_push_costs", true, p, n, slots, counts, costs, ld, labels, commit, now, stream);
}

extern "C" int prego_decode_pool_flush(prego_decode_pool* p, int n, const int32_t* slots, int32_t* labels, int32_t* commit, prego_stream_t stream) {
  const char* who = "decode_pool_flush";
  if (!p) return prego_fail_(PREGO_EINVAL, "%s: pool is NULL", who);
  if (int rc = check_slot_list(p->stamps, p->g.rec.capacity, who, n, slots)) return rc;
  const Range in[1] = {{p->block, p->bytes, "the pool's block"}};
  const Range out[2] = {{labels, (size_t)n * p->g.lag * 4, "labels"}, {commit, (size_t)n * 8, "commit"}};
  if (int rc = outputs_ok(who, out, 2, in, 1)) return rc;
  if (launch_decode_pool_flush(p->g, slots, n, labels, commit, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_decode_pool_reset(prego_decode_pool* p, int n, const int32_t* slots, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "decode_pool_reset: pool is NULL");
  if (int rc = check_slot_list(p->stamps, p->g.rec.capacity, "decode_pool_reset", n, slots)) return rc;
  if (launch_decode_pool_reset(p->g, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "decode_pool_reset: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_decode_pool_record(const prego_decode_pool* p, int slot, const void** device_record, size_t* bytes) {
  if (!p || !device_record || !bytes) return prego_fail_(PREGO_EINVAL, "decode_pool_record: NULL argument");
  if (slot < 0 || slot >= p->g.rec.capacity)
    return prego_fail_(PREGO_EINVAL, "decode_pool_record: slot %d is outside the pool (capacity %d)", slot, p->g.rec.capacity);
  *device_record = p->g.rec.rec + (size_t)slot * p->g.rec.rec_words;
  *bytes = (size_t)p->g.rec.rec_words * 4;
  return PREGO_OK;
}

extern "C" int prego_decode_pool_state(const prego_decode_pool* p, int slot, const void** device_state, size_t* bytes) {
  if (!p || !device_state || !bytes) return prego_fail_(PREGO_EINVAL, "decode_pool_state: NULL argument");
  if (slot < 0 || slot >= p->g.rec.capacity)
    return prego_fail_(PREGO_EINVAL, "decode_pool_state: slot %d is outside the pool (capacity %d)", slot, p->g.rec.capacity);
  *device_state = p->g.state + (size_t)slot * p->g.slot_bytes;
  *bytes = (size_t)p->g.ring_off;                            // the header and the keys; the ring lies behind them
  return PREGO_OK;
}
