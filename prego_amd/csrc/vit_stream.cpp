// Host side of the Transformer stream pool (include/prego_amd.h: prego_vit_stream_pool_*, prego_vit_step_pool(_bursts); kernels: vit_stream.hip,
// the vote record and its kernels: stream_pool.hip).  The pool object is host memory only: the geometry, the addresses inside the caller's
// device block and a stamp table for the duplicate check.  Every entry point decides all its refusals before its first launch, so a
// refused call has written nothing.
#include "vit_handle.h"
#include "pool_slot_check.h"

#include <cstdint>

struct prego_vit_stream_pool {
  VitRing r;
  PoolGeom g;                            // the vote records; g.h = the ring words [capacity][4], so pool_reset zeroes head, fill and the record
  const prego_vit* owner;                // the handle the pool was created for: prego_vit_stream_pool_window reads its encoding bias
  size_t bytes;                          // of the block, as laid out
  SlotStamps stamps;
};
const PoolGeom* vit_stream_pool_geom(const prego_vit_stream_pool* p) { return &p->g; }      // pool_slot_check.h
SlotStamps* vit_stream_pool_stamps(prego_vit_stream_pool* p) { return &p->stamps; }
PoolBlock vit_stream_pool_block(const prego_vit_stream_pool* p) { return PoolBlock{(const char*)p->r.ring, p->bytes}; }
const VitRing* vit_stream_pool_ring(const prego_vit_stream_pool* p) { return &p->r; }

namespace {
// block: ring [capacity][window][E] fp32 | ring words [capacity][4] int32 | records [capacity][rec_words] int32, each part 256-byte aligned
struct VitPoolLayout { size_t ring_bytes, hf_bytes, rec_words, total; };

// false: capacity or max_events below 1, max_events above 1 048 576 (the record's word count is an int), or a block that size_t cannot hold
bool vit_pool_layout(const prego_vit* h, int capacity, int max_events, VitPoolLayout* l) {
  if (capacity < 1 || max_events < 1 || max_events > (1 << 20)) return false;
  using u128 = unsigned __int128;
  const u128 rec_words = align_up((size_t)kPoolRecHeader + align_up((size_t)h->ncls, 4) + 2 * (size_t)max_events, 4);
  const u128 ring = (u128)capacity * (u128)h->window * (u128)h->emb * 4, hf = (u128)capacity * kVitRingStateWords * 4;
  const u128 rec = (u128)capacity * rec_words * 4;
  if (rec_words > 0x7fffffffu || ring + hf + rec + 3 * 256 > (u128)SIZE_MAX) return false;
  l->rec_words = (size_t)rec_words;
  l->ring_bytes = align_up((size_t)ring, 256);
  l->hf_bytes = align_up((size_t)hf, 256);
  l->total = l->ring_bytes + l->hf_bytes + align_up((size_t)rec, 256);
  return true;
}

// a burst call's host arrays turned into kernel arguments: by_slot = entry i for slots[i], by_row = the owner's entry for every packed
// row, rows = the sum of the counts.  n is already known to be in 1..256.  0 = fine, else PREGO_EINVAL with a message
struct BurstPlan { RaggedMap by_slot, by_row; int rows; };
int burst_plan(const char* who, int window, int n, const int32_t* counts, BurstPlan* bp) {
  if (!counts) return prego_fail_(PREGO_EINVAL, "%s: counts is NULL", who);
  const int kmax = window < 32 ? window : 32;
  int rows = 0;
  for (int i = 0; i < n; ++i) {
    if (counts[i] < 1 || counts[i] > kmax)
      return prego_fail_(PREGO_EINVAL, "%s: counts[%d] = %d (1..%d frames per slot per call: at most 32, window_size %d; split a longer "
                         "backlog)", who, i, counts[i], kmax, window);
    rows += counts[i];
  }
  if (rows > kPoolMaxActive)
    return prego_fail_(PREGO_EINVAL, "%s: the counts sum to %d rows (at most %d windows per call)", who, rows, kPoolMaxActive);
  for (int i = 0, at = 0; i < kRaggedMaxStreams; ++i) {
    bp->by_slot.e[i] = i < n ? ragged_entry((unsigned)at, (unsigned)i, (unsigned)counts[i]) : 0u;
    if (i < n) at += counts[i];
  }
  for (int i = 0, b = 0; i < n; ++i)
    for (int k = 0; k < counts[i]; ++k) bp->by_row.e[b++] = bp->by_slot.e[i];
  for (int b = rows; b < kRaggedMaxStreams; ++b) bp->by_row.e[b] = 0u;
  bp->rows = rows;
  return 0;
}

// what both step entries refuse first, in this order: NULL arguments, an fp32-operand handle (that sentence names the symbol, prego_<who>),
// missing weights, missing input, a pool of another geometry, the slot list
int vit_step_refusals(const char* who, const prego_vit* h, prego_vit_stream_pool* p, int n_active, const int32_t* slots,
                      const float* rgb, const float* flow, const float* out_logits) {
  if (!h || !p || !out_logits) return prego_fail_(PREGO_EINVAL, "%s: NULL argument", who);
  if (h->f32) return prego_fail_(PREGO_EINVAL, "prego_%s on an fp32-operand handle: the parity mode covers prego_vit_forward", who);
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "%s before set_weights", who);
  if ((h->d_rgb > 0 && !rgb) || (h->d_rgb == 0 && !flow)) return prego_fail_(PREGO_EINVAL, "%s: missing input", who);
  if (p->r.T != h->window || p->r.E != h->emb || p->g.ncls != h->ncls)
    return prego_fail_(PREGO_EINVAL, "%s: the pool was created for window_size %d / embedding_dim %d / %d classes, the handle has %d / %d / %d",
                       who, p->r.T, p->r.E, p->g.ncls, h->window, h->emb, h->ncls);
  return check_slot_list(p->stamps, p->r.capacity, who, n_active, slots);
}

// the caller's workspace, refused when NULL, misaligned or small (rows: the burst entry's, 0 = the one-frame entry: each words its own size
// refusal), carved as f lays it out: ws = the per-batch arena, as prego_vit_forward's; am = the caller's argmax or the workspace's
struct VitStepBufs { char *xb, *ws; float* enc; int32_t* am; };
int vit_step_carve(const char* who, void* workspace, size_t workspace_bytes, const VitStepWs& f, int n_active, int rows, int32_t* argmax,
                   VitStepBufs* b) {
  if (!workspace) return prego_fail_(PREGO_EINVAL, "%s: workspace is NULL", who);
  if ((uintptr_t)workspace & 255) return prego_fail_(PREGO_EINVAL, "%s: the workspace must be 256-byte aligned", who);
  if (workspace_bytes < f.total)
    return rows ? prego_fail_(PREGO_EWORKSPACE, "%s: workspace %zu < %zu for %d rows of %d active streams (prego_vit_step_pool_bursts_workspace_bytes)",
                              who, workspace_bytes, f.total, rows, n_active)
                : prego_fail_(PREGO_EWORKSPACE, "%s: workspace %zu < %zu for %d active streams (prego_vit_step_pool_workspace_bytes)", who,
                              workspace_bytes, f.total, n_active);
  char* base = (char*)workspace;
  *b = VitStepBufs{base + f.xb, base + f.win, (float*)(base + f.enc), argmax ? argmax : (int32_t*)(base + f.am)};
  return 0;
}

int slot_in_pool(const prego_vit_stream_pool* p, const char* who, int slot) {
  if (slot < 0 || slot >= p->r.capacity) return prego_fail_(PREGO_EINVAL, "%s: slot %d is outside the pool (capacity %d)", who, slot, p->r.capacity);
  return 0;
}
}  // namespace

extern "C" size_t prego_vit_stream_pool_bytes(const prego_vit* h, int capacity, int max_events) {
  VitPoolLayout l{};
  return (h && vit_pool_layout(h, capacity, max_events, &l)) ? l.total : 0;
}

extern "C" int prego_vit_stream_pool_create(prego_vit_stream_pool** out, const prego_vit* h, int capacity, int vote_window, int max_events,
                                            void* device_block, size_t bytes, prego_stream_t stream) {
  if (!out) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: out is NULL");
  *out = nullptr;
  if (!h) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: handle is NULL");
  if (vote_window < 1) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: vote_window %d (>= 1)", vote_window);
  VitPoolLayout l{};
  if (!vit_pool_layout(h, capacity, max_events, &l))
    return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: capacity %d (>= 1), max_events %d (1..%d), or a block of %d x %d x %d fp32 rows is "
                       "beyond size_t", capacity, max_events, 1 << 20, capacity, h->window, h->emb);
  if (!device_block || bytes < l.total)
    return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: block %p with %zu bytes, %d slots of %d x %d ring rows and %d events need %zu "
                       "(prego_vit_stream_pool_bytes)", device_block, bytes, capacity, h->window, h->emb, max_events, l.total);
  if ((uintptr_t)device_block & 255) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_create: the block must be 256-byte aligned");
  prego_vit_stream_pool* p = new prego_vit_stream_pool();
  char* base = (char*)device_block;
  p->r = VitRing{(float*)base, (int*)(base + l.ring_bytes), h->window, h->emb, capacity};
  p->g = PoolGeom{(float*)(base + l.ring_bytes), (int*)(base + l.ring_bytes + l.hf_bytes), kVitRingStateWords, h->ncls,
                  (int)align_up((size_t)h->ncls, 4), vote_window, max_events, (int)l.rec_words, capacity};
  p->owner = h;
  p->bytes = l.total;
  p->stamps.stamp.assign((size_t)capacity, 0u);
  const hipError_t e = hipMemsetAsync(device_block, 0, l.total, (hipStream_t)stream);      // every slot empty: open launches nothing
  if (e != hipSuccess) {
    delete p;
    return prego_fail_(PREGO_EHIP, "vit_stream_pool_create: hipMemsetAsync failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return PREGO_OK;
}

extern "C" void prego_vit_stream_pool_destroy(prego_vit_stream_pool* p) { delete p; }

extern "C" size_t prego_vit_step_pool_workspace_bytes(const prego_vit* h, int n_active) {
  if (!h || n_active < 1 || n_active > kPoolMaxActive) return 0;
  return vit_step_ws(*h, n_active, n_active, true).total;
}

// One new frame for the slots named: cat + convert, the encoding GEMM on n_active rows, the rows into their rings, one window per slot out
// of the rings, then the blocks, the head and the vote exactly as prego_vit_forward_frames runs them for a batch of n_active windows
extern "C" int prego_vit_step_pool(prego_vit* h, prego_vit_stream_pool* p, int n_active, const int32_t* slots, const float* rgb,
                                   const float* flow, float* out_logits, int32_t* argmax, int flags, void* workspace, size_t workspace_bytes,
                                   prego_stream_t stream) {
  const char* who = "vit_step_pool";
  if (int rc = vit_step_refusals(who, h, p, n_active, slots, rgb, flow, out_logits)) return rc;
  const VitStepWs f = vit_step_ws(*h, n_active, n_active, true);
  VitStepBufs b;
  if (int rc = vit_step_carve(who, workspace, workspace_bytes, f, n_active, 0, argmax, &b)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = b.ws;
  const VitWs& w = f.w;
  const int n = n_active, E = h->emb, din = h->d_rgb + h->d_flow;
  const int causal = (flags & 1) ? 1 : 0;
  launch_cat_convert(rgb, flow, n, h->d_rgb, h->d_flow, b.xb, s, h->f16);
  launch_gemm_bf16_nt(b.xb, din, h->enc_w, din, h->enc_b, b.enc, E, n, E, din, s, h->f16);       // ViT.py:124, once per frame
  if (launch_vit_ring_commit(p->r, slots, n, b.enc, s)) return prego_fail_(PREGO_EINVAL, "%s: ring commit refused its arguments", who);
  const bool fused = h->layers == 1;            // one layer: the token kernel writes LayerNorm1(x) and x0; x is never materialised
  const VitLayer& l0 = h->L[0];
  if (launch_vit_ring_tokens(p->r, slots, n, h->enc_b, h->cls, h->pe, fused ? nullptr : (float*)(ws + w.x), l0.ln1_w, l0.ln1_b,
                             fused ? ws + w.xn : nullptr, fused ? (float*)(ws + w.x0) : nullptr, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "%s: ring tokens refused its arguments", who);
  if (int rc = blocks_and_head(h, who, ws, w, n, causal, fused, out_logits, b.am, s)) return rc;
  if (launch_pool_vote(p->g, slots, n, (const int*)b.am, s)) return prego_fail_(PREGO_EINVAL, "%s: vote refused its arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" size_t prego_vit_step_pool_bursts_workspace_bytes(const prego_vit* h, int n_active, int n_rows) {
  if (!h || n_active < 1 || n_active > kPoolMaxActive || n_rows < n_active || n_rows > kPoolMaxActive) return 0;
  if ((long long)n_rows > (long long)n_active * (h->window < 32 ? h->window : 32)) return 0;
  return vit_step_ws(*h, n_rows, n_rows, true).total;
}

// counts[i] new frames for slots[i], R packed rows: cat + convert and the encoding GEMM on R rows, one window per packed row out of the
// rings as they stand and the call's own rows, THEN the rows into their rings (the token kernel reads what the commit overwrites), the
// blocks and the head for a batch of R windows, and every slot's record takes its ids in frame order
extern "C" int prego_vit_step_pool_bursts(prego_vit* h, prego_vit_stream_pool* p, int n_active, const int32_t* counts, const int32_t* slots,
                                          const float* rgb, const float* flow, float* out_logits, int32_t* argmax, int flags, void* workspace,
                                          size_t workspace_bytes, prego_stream_t stream) {
  const char* who = "vit_step_pool_bursts";
  if (int rc = vit_step_refusals(who, h, p, n_active, slots, rgb, flow, out_logits)) return rc;      // the slot list before the counts
  BurstPlan bp;
  if (int rc = burst_plan(who, h->window, n_active, counts, &bp)) return rc;
  const int n = n_active, R = bp.rows, E = h->emb, din = h->d_rgb + h->d_flow;
  const VitStepWs f = vit_step_ws(*h, R, R, true);
  VitStepBufs b;
  if (int rc = vit_step_carve(who, workspace, workspace_bytes, f, n, R, argmax, &b)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = b.ws;
  const VitWs& w = f.w;
  const int causal = (flags & 1) ? 1 : 0;
  launch_cat_convert(rgb, flow, R, h->d_rgb, h->d_flow, b.xb, s, h->f16);
  launch_gemm_bf16_nt(b.xb, din, h->enc_w, din, h->enc_b, b.enc, E, R, E, din, s, h->f16);       // ViT.py:124, once per frame
  const bool fused = h->layers == 1;
  const VitLayer& l0 = h->L[0];
  if (launch_vit_burst_tokens(p->r, slots, n, bp.by_slot, bp.by_row, R, b.enc, h->enc_b, h->cls, h->pe, fused ? nullptr : (float*)(ws + w.x),
                              l0.ln1_w, l0.ln1_b, fused ? ws + w.xn : nullptr, fused ? (float*)(ws + w.x0) : nullptr, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "%s: burst tokens refused its arguments", who);
  if (launch_vit_ring_commit_burst(p->r, slots, n, bp.by_slot, R, b.enc, s))
    return prego_fail_(PREGO_EINVAL, "%s: ring commit refused its arguments", who);
  if (int rc = blocks_and_head(h, who, ws, w, R, causal, fused, out_logits, b.am, s)) return rc;
  if (launch_pool_vote_ragged(p->g, slots, n, bp.by_slot, R, (const int*)b.am, s))
    return prego_fail_(PREGO_EINVAL, "%s: vote refused its arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_vit_stream_pool_flush(prego_vit_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_flush: pool is NULL");
  if (int rc = check_slot_list(p->stamps, p->r.capacity, "vit_stream_pool_flush", n, slots)) return rc;
  if (launch_pool_flush(p->g, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_flush: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// head, fill and the record go to zero; the ring rows stay, since nothing reads a row that fill does not cover
extern "C" int prego_vit_stream_pool_reset(prego_vit_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream) {
  if (!p) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_reset: pool is NULL");
  if (int rc = check_slot_list(p->stamps, p->r.capacity, "vit_stream_pool_reset", n, slots)) return rc;
  if (launch_pool_reset(p->g, slots, n, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_reset: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_vit_stream_pool_record(const prego_vit_stream_pool* p, int slot, const void** device_record, size_t* bytes) {
  if (!p || !device_record || !bytes) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_record: NULL argument");
  if (int rc = slot_in_pool(p, "vit_stream_pool_record", slot)) return rc;
  *device_record = p->g.rec + (size_t)slot * p->g.rec_words;
  *bytes = (size_t)p->g.rec_words * 4;
  return PREGO_OK;
}

extern "C" int prego_vit_stream_pool_window(prego_vit_stream_pool* p, int slot, float* out, int32_t* fill_out, prego_stream_t stream) {
  if (!p || !out) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_window: NULL argument");
  if (int rc = slot_in_pool(p, "vit_stream_pool_window", slot)) return rc;
  if (!p->owner->have_weights) return prego_fail_(PREGO_EINVAL, "vit_stream_pool_window before set_weights");
  if (launch_vit_ring_window(p->r, slot, p->owner->enc_b, out, (int*)fill_out, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "vit_stream_pool_window: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
// unit-test hook: vit_ring_tokens alone, only x wanted, on the pool as it stands (no commit)
extern "C" int prego_debug_vit_ring_tokens(prego_vit_stream_pool* p, int n, const int32_t* slots, float* x_out, prego_stream_t stream) {
  if (!p || !x_out) return prego_fail_(PREGO_EINVAL, "debug_vit_ring_tokens: NULL argument");
  if (!p->owner->have_weights) return prego_fail_(PREGO_EINVAL, "debug_vit_ring_tokens before set_weights");
  if (int rc = check_slot_list(p->stamps, p->r.capacity, "debug_vit_ring_tokens", n, slots)) return rc;
  const prego_vit* h = p->owner;
  if (launch_vit_ring_tokens(p->r, slots, n, h->enc_b, h->cls, h->pe, x_out, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, h->f16))
    return prego_fail_(PREGO_EINVAL, "debug_vit_ring_tokens: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// unit-test hook: vit_burst_tokens alone, only x wanted, on the pool as it stands (no commit) and the caller's enc [sum counts][E]
extern "C" int prego_debug_vit_burst_tokens(prego_vit_stream_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* enc,
                                            float* x_out, prego_stream_t stream) {
  const char* who = "debug_vit_burst_tokens";
  if (!p || !enc || !x_out) return prego_fail_(PREGO_EINVAL, "%s: NULL argument", who);
  if (!p->owner->have_weights) return prego_fail_(PREGO_EINVAL, "%s before set_weights", who);
  if (int rc = check_slot_list(p->stamps, p->r.capacity, who, n, slots)) return rc;
  BurstPlan bp;
  if (int rc = burst_plan(who, p->r.T, n, counts, &bp)) return rc;
  const prego_vit* h = p->owner;
  if (launch_vit_burst_tokens(p->r, slots, n, bp.by_slot, bp.by_row, bp.rows, enc, h->enc_b, h->cls, h->pe, x_out, nullptr, nullptr, nullptr,
                              nullptr, (hipStream_t)stream, h->f16))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// unit-test hook: vit_ring_commit_burst alone on the caller's enc [sum counts][E]
extern "C" int prego_debug_vit_burst_commit(prego_vit_stream_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* enc,
                                            prego_stream_t stream) {
  const char* who = "debug_vit_burst_commit";
  if (!p || !enc) return prego_fail_(PREGO_EINVAL, "%s: NULL argument", who);
  if (int rc = check_slot_list(p->stamps, p->r.capacity, who, n, slots)) return rc;
  BurstPlan bp;
  if (int rc = burst_plan(who, p->r.T, n, counts, &bp)) return rc;
  if (launch_vit_ring_commit_burst(p->r, slots, n, bp.by_slot, bp.rows, enc, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
#endif
