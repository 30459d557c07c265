// Host side of the stream pool (include/prego_amd.h: prego_stream_pool_*, prego_miniroad_step_pool (_frames, _ragged); kernels: stream_pool.hip).  The pool
// object is host memory only: the geometry, the addresses inside the caller's device block and a stamp table for the duplicate check.
// Every entry point validates the whole slot list before its first launch, so a refused call has launched nothing.
#include "miniroad_handle.h"
#include "pool_slot_check.h"

#include <algorithm>
#include <cstdint>
#include <vector>

struct prego_stream_pool {
  PoolGeom g;
  size_t bytes;                          // of the block, as laid out
  SlotStamps stamps;                     // the duplicate check without a per-call allocation
};
const PoolGeom* stream_pool_geom(const prego_stream_pool* p) { return &p->g; }      // pool_slot_check.h
SlotStamps* stream_pool_stamps(prego_stream_pool* p) { return &p->stamps; }
PoolBlock stream_pool_block(const prego_stream_pool* p) { return PoolBlock{(const char*)p->g.h, p->bytes}; }

namespace {
struct PoolLayout { size_t h_bytes, rec_words, total; };

// block: h [capacity][hid] fp32 | records [capacity][rec_words] int32, each part 256-byte aligned
PoolLayout pool_layout(int hid, int ncls, int capacity, int max_events) {
  PoolLayout l{};
  const size_t ncls_pad = align_up((size_t)ncls, 4);
  l.rec_words = align_up((size_t)kPoolRecHeader + ncls_pad + 2 * (size_t)max_events, 4);
  l.h_bytes = align_up((size_t)capacity * hid * 4, 256);
  l.total = l.h_bytes + align_up((size_t)capacity * l.rec_words * 4, 256);
  return l;
}

bool pool_shape_ok(int capacity, int max_events) { return capacity >= 1 && capacity <= (1 << 20) && max_events >= 1 && max_events <= (1 << 20); }

// the slot list of one call: n in 1..min(256, capacity), every slot inside the pool and named once (pool_slot_check.h)
int check_slots(prego_stream_pool* p, const char* who, int n, const int32_t* slots) {
  return check_slot_list(p->stamps, p->g.capacity, who, n, slots);
}

// what the three step entries differ in: the dense call behind them and, with it, the ids slot i votes.  kOne: one frame through
// step_wide (its workspace is 0 bytes up to 16 streams: step's launches on the handle's scratch), ids [i]; kFrames: K frames per slot
// through step_frames, ids [i K, i K + K); kRagged: a count per slot through step_ragged, ids in packed rows (RaggedPlan)
enum class Burst { kOne, kFrames, kRagged };

// the step calls' workspace: dense state [n][hid] fp32 | argmax [rows] int32 | the dense call's own workspace.  per: kFrames: K (rows =
// n K), kRagged: the rows, kOne: unused (rows = n)
struct StepPoolLayout { size_t am, wide, wide_bytes, total; };
StepPoolLayout step_pool_layout(const prego_miniroad* h, Burst kind, int n, int per) {
  StepPoolLayout l{};
  WsCarver c;
  c.take((size_t)n * h->hid * 4);
  l.am = c.take((size_t)(kind == Burst::kOne ? n : kind == Burst::kFrames ? n * per : per) * 4);
  l.wide = c.o;
  l.wide_bytes = kind == Burst::kOne      ? prego_miniroad_step_wide_workspace_bytes(h, n)
                 : kind == Burst::kFrames ? prego_miniroad_step_frames_workspace_bytes(h, n, per)
                                          : prego_miniroad_step_ragged_workspace_bytes(h, n, per);
  l.total = l.wide + l.wide_bytes;
  return l;
}

// prego_miniroad_step_pool (kOne, K = 1), _frames (kFrames, K = n_frames) and _ragged (kRagged, n_frames[i] per slot): gather the slots'
// states into the workspace, make the dense call a caller without a pool would make, through the same entry point (the pool adds no
// arithmetic), commit.  The refusals of all three are decided before the gather
int step_pool_impl(const char* who, Burst kind, prego_miniroad* h, prego_stream_pool* p, int n_active, int K, const int32_t* n_frames,
                   const int32_t* slots, const float* rgb, const float* flow, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax,
                   int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  const bool ant = ant_out != nullptr || ant_argmax != nullptr;
  StepPoolLayout l{};
  RaggedPlan plan;                                            // kRagged only
  {
    HandleScope scope_(h);
    if (!p) return prego_fail_(PREGO_EINVAL, "%s: pool is NULL", who);
    if (kind == Burst::kFrames && (K < 1 || K > 32)) return prego_fail_(PREGO_EINVAL, "%s: %d frames per stream (1..32 per call)", who, K);
    if (kind == Burst::kFrames && n_active >= 1 && (long long)n_active * K > kPoolMaxActive)
      return prego_fail_(PREGO_EINVAL, "%s: %d streams x %d frames = %lld rows (at most %d per call: use forward() with h0 / h_last)", who,
                         n_active, K, (long long)n_active * K, kPoolMaxActive);
    if (kind == Burst::kRagged)
      if (int rc = ragged_plan(who, n_active, n_frames, &plan)) return rc;
    // everything the dense call would refuse, before the gather is launched (the state it will be handed is the workspace's dense copy)
    if (int rc = step_refusals(h, n_active, kPoolMaxActive, rgb, flow, p->g.h, ant)) return rc;
    if (p->g.hid != h->hid || p->g.ncls != h->ncls)
      return prego_fail_(PREGO_EINVAL, "%s: the pool was created for hidden_dim %d / %d classes, the handle has %d / %d", who, p->g.hid,
                         p->g.ncls, h->hid, h->ncls);
    if (int rc = check_slots(p, who, n_active, slots)) return rc;
    l = step_pool_layout(h, kind, n_active, kind == Burst::kRagged ? plan.rows : K);
    if (int rc = kind == Burst::kOne      ? workspace_refusal(who, "prego_miniroad_step_pool_workspace_bytes", workspace, workspace_bytes, l.total,
                                                              "%d active streams", n_active)
                 : kind == Burst::kFrames ? workspace_refusal(who, "prego_miniroad_step_pool_frames_workspace_bytes", workspace, workspace_bytes,
                                                              l.total, "%d active streams x %d frames", n_active, K)
                                          : workspace_refusal(who, "prego_miniroad_step_pool_ragged_workspace_bytes", workspace, workspace_bytes,
                                                              l.total, "%d active streams with %d frames in all", n_active, plan.rows)) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* h_ws = (float*)ws;
  int32_t* am = argmax ? argmax : (int32_t*)(ws + l.am);      // the vote always has its ids
  if (launch_pool_gather(p->g, slots, n_active, h_ws, s)) return prego_fail_(PREGO_EINVAL, "%s: gather refused its arguments", who);
  void* dws = ws + l.wide;
  const size_t db = l.wide_bytes;
  int rc;
  if (kind == Burst::kOne)
    rc = ant ? prego_miniroad_step_wide_anticipation(h, n_active, rgb, flow, h_ws, out, am, ant_out, ant_argmax, flags, dws, db, stream)
             : prego_miniroad_step_wide(h, n_active, rgb, flow, h_ws, out, am, flags, dws, db, stream);
  else if (kind == Burst::kFrames)
    rc = ant ? prego_miniroad_step_frames_anticipation(h, n_active, K, rgb, flow, h_ws, out, am, ant_out, ant_argmax, flags, dws, db, stream)
             : prego_miniroad_step_frames(h, n_active, K, rgb, flow, h_ws, out, am, flags, dws, db, stream);
  else
    rc = ant ? prego_miniroad_step_ragged_anticipation(h, n_active, n_frames, rgb, flow, h_ws, out, am, ant_out, ant_argmax, flags, dws, db, stream)
             : prego_miniroad_step_ragged(h, n_active, n_frames, rgb, flow, h_ws, out, am, flags, dws, db, stream);
  if (rc) return rc;                                          // the pool itself is untouched: only the commit writes it
  if (kind == Burst::kRagged ? launch_pool_commit_ragged(p->g, slots, n_active, plan.by_stream, plan.rows, h_ws, am, s)
                             : launch_pool_commit(p->g, slots, n_active, K, h_ws, am, s))
    return prego_fail_(PREGO_EINVAL, "%s: commit refused its arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" size_t prego_stream_pool_bytes(const prego_miniroad* h, int capacity, int max_events) {
  if (!h || !pool_shape_ok(capacity, max_events)) return 0;
  return pool_layout(h->hid, h->ncls, capacity, max_events).total;
}

extern "C" int prego_stream_pool_create(prego_stream_pool** out, const prego_miniroad* h, int capacity, int window, int max_events,
                                        void* device_block, size_t bytes, prego_stream_t stream) {
  if (!out) return prego_fail_(PREGO_EINVAL, "stream_pool_create: out is NULL");
  *out = nullptr;
  if (!h) return prego_fail_(PREGO_EINVAL, "stream_pool_create: handle is NULL");
  if (window < 1) return prego_fail_(PREGO_EINVAL, "stream_pool_create: window %d (>= 1)", window);
  if (!pool_shape_ok(capacity, max_events))
    return prego_fail_(PREGO_EINVAL, "stream_pool_create: capacity %d, max_events %d (each 1..%d)", capacity, max_events, 1 << 20);
  const PoolLayout l = pool_layout(h->hid, h->ncls, capacity, max_events);
  if (!device_block || bytes < l.total)
    return prego_fail_(PREGO_EINVAL, "stream_pool_create: block %p with %zu bytes, %d slots of %d events need %zu (prego_stream_pool_bytes)",
                       device_block, bytes, capacity, max_events, l.total);
  if ((uintptr_t)device_block & 255) return prego_fail_(PREGO_EINVAL, "stream_pool_create: the block must be 256-byte aligned");
  prego_stream_pool* p = new prego_stream_pool();
  p->g = PoolGeom{(float*)device_block, (int*)((char*)device_block + l.h_bytes), h->hid, h->ncls, (int)align_up((size_t)h->ncls, 4), window,
                  max_events, (int)l.rec_words, capacity};
  p->bytes = l.total;
  p->stamps.stamp.assign((size_t)capacity, 0u);
  const hipError_t e = hipMemsetAsync(device_block, 0, l.total, (hipStream_t)stream);      // every slot empty: open launches nothing
  if (e != hipSuccess) {
    delete p;
    return prego_fail_(PREGO_EHIP, "stream_pool_create: hipMemsetAsync failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return PREGO_OK;
}

extern "C" void prego_stream_pool_destroy(prego_stream_pool* p) { delete p; }

extern "C" size_t prego_miniroad_step_pool_workspace_bytes(const prego_miniroad* h, int n_active) {
  if (!h || n_active < 1 || n_active > kPoolMaxActive) return 0;
  return step_pool_layout(h, Burst::kOne, n_active, 1).total;
}

extern "C" int prego_miniroad_step_pool(prego_miniroad* h, prego_stream_pool* p, int n_active, const int32_t* slots, const float* rgb,
                                        const float* flow, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags,
                                        void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return step_pool_impl("step_pool", Burst::kOne, h, p, n_active, 1, nullptr, slots, rgb, flow, out, argmax, ant_out, ant_argmax, flags, workspace,
                        workspace_bytes, stream);
}

extern "C" size_t prego_miniroad_step_pool_frames_workspace_bytes(const prego_miniroad* h, int n_active, int n_frames) {
  if (!h || prego_miniroad_step_frames_workspace_bytes(h, n_active, n_frames) == 0) return 0;
  return step_pool_layout(h, Burst::kFrames, n_active, n_frames).total;
}

extern "C" int prego_miniroad_step_pool_frames(prego_miniroad* h, prego_stream_pool* p, int n_active, int n_frames, const int32_t* slots,
                                               const float* rgb, const float* flow, float* out, int32_t* argmax, float* ant_out,
                                               int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                                               prego_stream_t stream) {
  return step_pool_impl("step_pool_frames", Burst::kFrames, h, p, n_active, n_frames, nullptr, slots, rgb, flow, out, argmax, ant_out, ant_argmax,
                        flags, workspace, workspace_bytes, stream);
}

extern "C" size_t prego_miniroad_step_pool_ragged_workspace_bytes(const prego_miniroad* h, int n_active, int n_rows) {
  if (!h || prego_miniroad_step_ragged_workspace_bytes(h, n_active, n_rows) == 0) return 0;
  return step_pool_layout(h, Burst::kRagged, n_active, n_rows).total;
}

extern "C" int prego_miniroad_step_pool_ragged(prego_miniroad* h, prego_stream_pool* p, int n_active, const int32_t* n_frames,
                                               const int32_t* slots, const float* rgb, const float* flow, float* out, int32_t* argmax,
                                               float* ant_out, int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                                               prego_stream_t stream) {
  return step_pool_impl("step_pool_ragged", Burst::kRagged, h, p, n_active, 0, n_frames, slots, rgb, flow, out, argmax, ant_out, ant_argmax, flags,
                        workspace, workspace_bytes, stream);
}

extern "C" int prego_stream_pool_vote(prego_stream_pool* p, int n, const int32_t* slots, const int32_t* ids, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "stream_pool_vote: pool is NULL");
  if (!ids) return prego_fail_(PREGO_EINVAL, "stream_pool_vote: ids is NULL");
  if (int rc = check_slots(p, "stream_pool_vote", n, slots)) return rc;
  if (launch_pool_vote(p->g, slots, n, ids, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "stream_pool_vote: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_stream_pool_flush(prego_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "stream_pool_flush: pool is NULL");
  if (int rc = check_slots(p, "stream_pool_flush", n, slots)) return rc;
  if (launch_pool_flush(p->g, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "stream_pool_flush: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_stream_pool_reset(prego_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "stream_pool_reset: pool is NULL");
  if (int rc = check_slots(p, "stream_pool_reset", n, slots)) return rc;
  if (launch_pool_reset(p->g, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "stream_pool_reset: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_stream_pool_record(const prego_stream_pool* p, int slot, const void** device_record, size_t* bytes) {
  if (!p || !device_record || !bytes) return prego_fail_(PREGO_EINVAL, "stream_pool_record: NULL argument");
  if (slot < 0 || slot >= p->g.capacity) return prego_fail_(PREGO_EINVAL, "stream_pool_record: slot %d is outside the pool (capacity %d)", slot, p->g.capacity);
  *device_record = p->g.rec + (size_t)slot * p->g.rec_words;
  *bytes = (size_t)p->g.rec_words * 4;
  return PREGO_OK;
}
