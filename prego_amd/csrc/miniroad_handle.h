// Private to the MiniROAD host files (miniroad*.cpp): the handle, the layouts of its workspaces, and the few internal functions that
// cross files.  Which file defines what:
//   miniroad.cpp          error state (g_err, g_cur), create / destroy, weight setters, check, timing (ev_begin / ev_end), pass_info,
//                         the debug library's allocation / wait counters (g_dbg_mallocs, g_dbg_syncs)
//   miniroad_plan.cpp     build_plan, device_plan, stage_tables, feed events, row_bytes / fwd_layout and the workspace size
//   miniroad_forward.cpp  validate_forward, choose_pass, run_chunked_pass, the forward entry points, ant_head
//   stream_step.cpp       step_refusals, prego_miniroad_step (_anticipation), prego_miniroad_step_wide (_anticipation)
//   stream_frames.cpp     prego_miniroad_step_frames (_anticipation), prego_miniroad_step_ragged (_anticipation), ragged_plan
//   stream_pool.cpp       the stream pool: prego_stream_pool_*, prego_miniroad_step_pool (kernels: stream_pool.hip)
//   miniroad_split.cpp    ring / resident-buffer sizing, forward_split; the per-device order of split passes (g_split_mu, g_split_last)
//   miniroad_train.cpp    dropout, loss, bwd_layout, backward, AdamW; the debug library's g_ant_full_span
#pragma once
#include "host_common.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#ifdef PREGO_DEBUG_ABI
#include <atomic>
#endif

#ifdef PREGO_DEBUG_ABI
// unit-test hook (prego_debug_alloc_count): every device allocation and every stream / event wait the MiniROAD host files make is
// counted, so a test can hold "a hot call allocates nothing and waits for nothing" to zero.  The counters live in miniroad.cpp
extern __attribute__((visibility("hidden"))) std::atomic<long long> g_dbg_mallocs, g_dbg_syncs;
#define hipMalloc(p, n) (++g_dbg_mallocs, (hipMalloc)(p, n))
#define hipStreamSynchronize(s) (++g_dbg_syncs, (hipStreamSynchronize)(s))
#define hipEventSynchronize(e) (++g_dbg_syncs, (hipEventSynchronize)(e))
#endif

struct EventPair { hipEvent_t a, b; };

struct prego_miniroad {
  int d_rgb, d_flow, emb, hid, ncls, ncls_pad;
  bool bf16;                    // 16-bit MFMA operands (bf16, or IEEE fp16 when f16 is set as well); false = exact-fp32 MFMA
  bool f16 = false;             // PREGO_F16: the 16-bit operand / intermediate type is fp16 (inference entry points only)
  bool x2 = false;              // PREGO_F16X2: split fp16 operands (hi + lo, three products; csrc/common.h), fp32 intermediates; bf16 is false
  float* x2_scale = nullptr;    // device [3][2]: (scale, 1 / scale) of w1, w_ih, w_hh (powers of two chosen by set_weights)
  int n_cu;
  int G, P;                     // recurrence groups / workgroups per group
  // ingested weights (device, handle-owned)
  void* w1 = nullptr;           // [emb][d_rgb+d_flow] WT
  float* b1 = nullptr;
  float* ln_g = nullptr;
  float* ln_b = nullptr;
  void* w_ih = nullptr;         // [3H][emb] WT
  void* w_hh = nullptr;         // [3H][H] WT
  float* bias2 = nullptr;       // b_ih + (b_hh for r,z rows)
  // split pass (round 6): W_ih / bias2 with their rows PERMUTED so that a recurrence lane's r / z / n pairs of a GI row are 12 adjacent
  // bytes: row (u / 2) * 6 + 2 * gate + u % 2 holds nn.GRU's row gate * H + u.  Built lazily in front of a split pass when the weights
  // have changed since (set_weights, the fused AdamW step); 16-bit handles of hidden_dim 1024 / one layer only
  void* w_ih_perm = nullptr; float* bias2_perm = nullptr; bool perm_stale = true;
  float* b_hn = nullptr;        // [H]
  void* w_c = nullptr;          // [ncls_pad][H] WT zero padded
  float* b_c = nullptr;         // [ncls_pad]
  bool have_weights = false;
  // MiniROADA anticipation head (prego_miniroad_set_anticipation): anticipation_layer.0.weight [L*H][H] in the operand type, its bias fp32
  int ant_len = 0; void* w_a = nullptr; float* b_a = nullptr; size_t w_a_cap = 0;
  void* st_ant = nullptr;       // streaming step with anticipation: A [16][ant_len * H] in the operand type (16-bit handles; set_anticipation)
  // MiniROADA training: the last PREGO_FWD_KEEP forward was forward_anticipation's (its backward then needs set_anticipation_grads), and
  // what prego_miniroad_set_anticipation_grads handed to the NEXT backward (d_ant NULL = zero anticipation gradient)
  bool ant_kept = false; bool ant_grads_set = false;
  std::vector<const float*> ant_d; float* ant_g_w = nullptr; float* ant_g_b = nullptr;
  // nn.GRU(embedding_dim, hidden_dim, num_layers) with num_layers == 2 (rnn.py:32,38): layer 1's operands (gru.*_l1; its input is layer 0's
  // h_t, so weight_ih_l1 is [3H][H]).  Inference only; hidden state [layers][slots][H]
  int layers = 1;
  void* l2_w_ih = nullptr; void* l2_w_hh = nullptr; float* l2_bias2 = nullptr; float* l2_b_hn = nullptr; bool have_layer2 = false;
  // recurrence scratch
  void* hx = nullptr;           // [G][2][64][H] WT
  unsigned* flags = nullptr;    // [G*P] + abort word
  unsigned* abort_word = nullptr;
  float* h_state = nullptr;     // [max_clips][H]
  unsigned long long* stamps = nullptr;   // debug phase counters (PREGO_GRU_STAMPS=1)
  char* st_scratch = nullptr;   // streaming step: y [16][emb] f32 | e [16][emb] bf16 | gi [16][3H] f32 | gh [16][3H] f32
  bool use_stamps = false;
  // training
  float drop_p = 0.f;
  unsigned long long drop_seed = 0;
  int kept_kx = 0;              // K of layer1 actually multiplied by the last PREGO_FWD_KEEP forward
  int kept_rows = 0;
  // data-parallel training: events the NEXT backward records when a group of gradient tensors is final (prego_miniroad_backward_events),
  // so that the caller can start reducing that bucket on another stream while the rest of the backward runs
  float* g_l2[4] = {nullptr, nullptr, nullptr, nullptr};     // prego_miniroad_set_gru_layer_grads: dW_ih_l1, dW_hh_l1, db_ih_l1, db_hh_l1
  hipEvent_t bwd_ev[2] = {nullptr, nullptr};
  prego_bucket_fn bwd_cb = nullptr; void* bwd_cb_user = nullptr;     // prego_miniroad_backward_callback: called right behind each event record
  // plan cache
  std::vector<int32_t> plan_lens;
  std::vector<int> h_rowoff, h_nact, h_sorted;      // h_sorted: first clip of each slot (slot order)
  std::vector<int> h_seg_off, h_seg_clip, h_seg_start;
  std::vector<int> h_blkstep;    // step of packed row 32 b
  int* d_blkstep = nullptr; size_t cap_b = 0;
  int n_slots = 0;
  bool plan_single = true;       // one clip per slot (required for h0 / h_last / training)
  bool plan_want_single = false;
  int plan_host_row_bytes = 0;   // PCIe bytes per packed row the cached plan was costed with (0 = features in HBM)
  // feed events of the NEXT forward (prego_miniroad_set_feed_events): rows of steps < feed_upto[j] are valid once feed_ev[0..j] have fired
  std::vector<int> feed_upto; std::vector<hipEvent_t> feed_ev; size_t feed_pos = 0; int feed_row_bytes = 0;
  int t_max = 0;
  int* d_rowoff = nullptr; int* d_nact = nullptr; int* d_sorted = nullptr;
  int* d_seg_off = nullptr; int* d_seg_clip = nullptr; int* d_seg_start = nullptr;
  size_t cap_t = 0, cap_c = 0;
  // per-call pointer tables (device)
  void** d_ptrs = nullptr;      // [6][max_clips]: rgb, flow, out, argmax, anticipation out, anticipation argmax
  // pinned host staging for the per-call tables (pointer table, plan arrays): the async H2D copies read it after the call
  // returns, so it is handle-owned and fenced by an event (never a stack or pageable buffer)
  char* pin = nullptr; size_t pin_bytes = 0; hipEvent_t pin_ev = nullptr; bool pin_busy = false;
  bool plan_dirty = false;      // host plan arrays changed, device copies pending
  bool no_local = false;        // PREGO_GRU_NO_LOCAL (read once at create): skip the XCD-local hand-off fast path
  bool no_mt = false;           // PREGO_GRU_NO_MT (read once at create): multi-tile steps on the classic kernel
  // feature streaming of chunk c+1 under the recurrence of chunk c: the pack kernel (22 registers, no LDS) fits beside a
  // recurrence workgroup on every CU, so it runs on a handle-owned side stream, forked from and joined to the caller's stream
  // by events (the caller still sees one in-order stream)
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; bool pack_prefetch = true;
  // layer1 GEMM of chunk c + 1 on the XCDs the (compacted) recurrence of chunk c does not hold (off: PREGO_NO_XCD_OVERLAP=1):
  // one tile counter per chunk, zeroed once per forward
  unsigned* tile_ctr = nullptr; bool xcd_overlap = false;
  // host mirror of the kernel's verified-placement word (rendezvous word 20: 1 = an earlier full-width launch found exactly 32 workgroups
  // on every XCD).  The device decides whether a launch is really compacted; the host only launches the layer1 worker beside a
  // recurrence it KNOWS will be compacted (advisor, round 3: with word 20 != 1 the recurrence ran full width while the persistent
  // worker competed for the same CUs).  -1 = not read yet: copied out behind the first full-width launch, read when that copy is done
  int placement = -1; unsigned* pin_place = nullptr; hipEvent_t ev_place = nullptr; bool place_pending = false;
  int prefetch_grid = 0;        // workgroup cap of the prefetching pack launch (0 = unthrottled)
  // split pass: recurrence on XCDs 0 .. split_r - 1 and the feed-forward of the whole pass on the others, two persistent
  // launches.  Their whole-call buffer [relu(h) rows of the pass | row map | counters] is the CALLER's resident buffer (res_buf,
  // prego_miniroad_set_resident): forward() allocates nothing and synchronises nothing for it (round 6)
  int split_r = 0; int plan_force_slots = 0;
  double plan_cost_us = 0;      // recurrence cost estimate of the cached plan (kStepCost tables)
  // Which pass a call takes (choose_pass, miniroad_forward.cpp): everything the policy remembers between calls.  Only choose_pass and
  // note_split_fallback write it, except: forward_split and the end of either pass clear / consume meas_armed, prego_miniroad_check sets
  // split_env = 0 after a timeout inside a split pass, create reads PREGO_SPLIT_PASS into split_env
  struct Chooser {
    int split_env = -1;         // PREGO_SPLIT_PASS at create: -1 unset = decide per call (cost model), 0 = never, R = whenever a call is eligible
    std::vector<int32_t> split_seen_lens; int split_seen_key = -1, split_seen_r = 3; double split_seen_est_c = 0, split_seen_est_s = 0;   // the last estimates (same clips, same call shape)
    // the cost model is corrected by what passes of either kind actually took on THIS device (devices of one pool differ: a sustained
    // split pass runs its GEMM tiles 35 % slower on some, where it then loses to the chunked pass): measured / estimated, per kind
    hipEvent_t ev_meas[2] = {nullptr, nullptr}; bool meas_pending = false, meas_armed = false; int meas_mode = 0; double meas_est = 0;
    double ratio_chunked = 1.0, ratio_split = 1.0; bool have_ratio_chunked = false, have_ratio_split = false, split_warm = false;
    // back-off after a failed start handshake (the call itself is re-run as a chunked pass: no call is ever lost)
    int split_fails = 0; long long split_skip = 0; long long split_fallbacks = 0;
  } chooser;
  char* res_buf = nullptr; size_t res_bytes = 0;       // caller-owned (prego_miniroad_set_resident); NULL = per-chunk head, chunked pass
  const float* peer_guard = nullptr;                   // caller-owned device word (prego_miniroad_set_peer_guard); NULL = none
  // start handshake of a split pass (kernels.h: PassHandshake): the pinned word the two launches report their GO / FAIL decision in and
  // the pass counter (the back-off after a FAIL is the chooser's)
  unsigned* pin_hs = nullptr; unsigned hs_seq = 0;
  int dbg_fault = 0;            // debug library only (prego_debug_split_fault): what the NEXT split pass does differently, one shot
  // chunked pass with the classifier ONCE behind the pass (as the split pass runs it): relu(h) of every packed row of the call stays
  // in the caller's resident buffer (capped at 24 GB) instead of one head launch per chunk
  hipEvent_t ev_split[4] = {nullptr, nullptr, nullptr, nullptr};   // timing of the two launches (timing_enable)
  double split_rec_ms = 0, split_ff_ms = 0; long long split_passes = 0, split_steps = 0; bool split_ev_pending = false;
  std::string err;              // last error of THIS handle (prego_miniroad_last_error)
  // timing
  bool timing = false;
  std::vector<EventPair> ev_pool;
  std::vector<int> ev_kind;     // 0 gemm (static launches), 1 gru, 2 pack, 3 overlapped layer1 worker
  size_t ev_used = 0;
  double gemm_flop = 0, pack_bytes = 0;
};

// nothing declared here is part of the library's ABI: the functions and variables that cross files stay out of its dynamic symbol table
#pragma GCC visibility push(hidden)

// Marks the handle whose entry point is running on this thread: prego_fail_ records errors in it as well, so that
// prego_miniroad_last_error(h) of one handle is never overwritten by another handle's failure.  Defined in miniroad.cpp beside the
// thread-local it sets (g_cur), out of line on purpose: an `extern thread_local` declared here under hidden visibility makes every user
// call a weak, undefined TLS initialiser through a PC-relative address, which is not NULL in a shared library (a crash at the first call)
struct HandleScope {
  explicit HandleScope(prego_miniroad* h);
  ~HandleScope();
};

// split-operand recurrence: two clip tiles per group at most (the four-tile instantiation would spill: 2 x 96 weight registers)
static inline int max_slots_of(const prego_miniroad* h) { return gru_max_slots(h->G, h->x2); }
#define PREGO_MAX_CLIPS 8192     // clips per call (continuous batching packs them into <= max_slots slots)
static inline int max_clips_of(const prego_miniroad*) { return PREGO_MAX_CLIPS; }

// ---- miniroad.cpp: timing events around a launch (no-ops unless prego_miniroad_timing_enable)
EventPair* ev_begin(prego_miniroad* h, int kind, hipStream_t s);
void ev_end(EventPair* p, hipStream_t s);

// ---- miniroad_plan.cpp
int build_plan(prego_miniroad* h, int n, const int32_t* lens, bool want_single, int host_row_bytes = 0, int slots_arg = 0);
SlotPlan device_plan(const prego_miniroad* h);
int stage_tables(prego_miniroad* h, const void* const* tab4, size_t tab_count, hipStream_t s);

struct RowBytes { size_t x, y, e, gi, hr, hraw, gates, stats, map, l2keep, total; };
bool inter16(const prego_miniroad* h, int flags);
RowBytes row_bytes(const prego_miniroad* h, bool with_flow, int flags);
// The forward workspace: byte offsets of every per-row buffer of a chunked pass, each for cap_rows rows and 256-byte aligned, in the order
// the pass has always laid them out.  X is at offset 0; a buffer the flags do not need has offset 0 (at() then gives NULL):
// HRAW .. STATS exist with PREGO_FWD_KEEP, HR0 .. KG2 with PREGO_FWD_KEEP on a two-layer handle.  The backward reads the kept buffers
// through the same function (flags = PREGO_FWD_KEEP), so the two sides cannot disagree.
struct FwdLayout {
  RowBytes rb;
  long long cap_rows;          // rows every buffer holds: what fits workspace_bytes, rounded down to a multiple of 128
  size_t X, Y, E, GI, HR, HRAW, KR, KZ, KN, KG, STATS, HR0, HRAW2, KR2, KZ2, KN2, KG2, RM;
  size_t total;                // <= workspace_bytes
  void* at(void* workspace, size_t off) const { return off ? (char*)workspace + off : nullptr; }      // optional buffers (not X)
};
FwdLayout fwd_layout(const prego_miniroad* h, bool with_flow, int flags, size_t workspace_bytes);
long long fwd_rows_fit(const RowBytes& rb, size_t workspace_bytes);      // rows a workspace holds, before the rounding to 128
size_t fwd_bytes_for_rows(const RowBytes& rb, long long rows);           // workspace for `rows` rows (rounded up to 128)

// ---- miniroad_split.cpp
struct SplitRings { size_t x, y, e, gi, total; int ring_units; };
SplitRings split_rings(const prego_miniroad* h, int R);
bool split_workspace_ok(const prego_miniroad* h, int R, size_t workspace_bytes);
size_t split_buf_need(const prego_miniroad* h, long long total);
bool split_resident_ok(const prego_miniroad* h, long long total);

// AntOut: the anticipation outputs of a forward_anticipation call (host pointer arrays; their device tables are d_ptrs rows 4 and 5)
struct AntOut {
  bool call = false;                   // forward_anticipation (rather than forward)
  float* const* out = nullptr;         // per clip [T][L][C], nullable
  int32_t* const* arg = nullptr;       // per clip [T][L], nullable
  bool wanted() const { return call && (out || arg); }
};
// the device pointer tables of one forward call (rows of h->d_ptrs; NULL = the caller did not pass that array)
struct FwdTables { const float* const* rgb; const float* const* flow; float* const* out; int* const* arg; };
// *fell_back = true (with PREGO_OK): the start handshake of the two launches failed - they left without writing anything, the caller
// runs the chunked pass for this call.
int forward_split(prego_miniroad* h, const AntOut& ao, int R, int flags, bool with_flow, bool in16, int kx, const SlotPlan& plan,
                  const FwdTables& tb, void* workspace, size_t workspace_bytes, hipStream_t s, bool* fell_back);

// ---- miniroad_forward.cpp
// the anticipation head of a forward_anticipation call over packed rows [row0, row0 + nrows) of the plan, relu(h) rows at HR (chunk-relative);
// the destinations come from the plan (the same lookup in every pass: which pass ran changes no bit)
int ant_head(prego_miniroad* h, const AntOut& ao, const void* HR, const SlotPlan& plan, int row0, int nrows, int flags, hipStream_t s);

// ---- stream_step.cpp
// what every streaming step refuses, n_max streams per call (16: step, 256: step_wide, step_pool); 0 = the call may go ahead.  Under a HandleScope
int step_refusals(prego_miniroad* h, int n_streams, int n_max, const float* rgb, const float* flow, const float* h_state, bool ant);

// ---- stream_frames.cpp
// a ragged call's host array turned into kernel arguments (nothing of the array outlives the call): by_stream = entry i for stream i in
// the caller's order, walk = the same entries in descending order of count (stable), alive[t] = streams with more than t frames,
// kmax = the largest count, rows = their sum.  0 = fine; n outside 1..256 is NOT refused here (rows = 0: the caller's own check refuses it)
struct RaggedPlan { RaggedMap by_stream, walk; int alive[32]; int kmax, rows; };
int ragged_plan(const char* who, int n, const int32_t* n_frames, RaggedPlan* p);

// ---- the caller's workspace of a streaming entry point
// carves it into parts that each start 256-byte aligned: take() returns the part's offset, `o` is the size so far
struct WsCarver {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; }
};
// refuses a workspace that is NULL, smaller than `need` or not 256-byte aligned; 0 = it will do.  who: the entry point's short name,
// hint: the function that tells the size, what...: printf-style, what it is that needs `need` bytes
__attribute__((format(printf, 6, 7))) static inline int workspace_refusal(const char* who, const char* hint, void* ws, size_t bytes, size_t need,
                                                                          const char* what, ...) {
  if (!ws || bytes < need) {
    char buf[96];
    va_list ap;
    va_start(ap, what);
    vsnprintf(buf, sizeof buf, what, ap);
    va_end(ap);
    return prego_fail_(PREGO_EINVAL, "%s: workspace %p with %zu bytes, %s need %zu (%s)", who, ws, bytes, buf, need, hint);
  }
  if ((uintptr_t)ws & 255) return prego_fail_(PREGO_EINVAL, "%s: the workspace must be 256-byte aligned", who);
  return 0;
}

#pragma GCC visibility pop
