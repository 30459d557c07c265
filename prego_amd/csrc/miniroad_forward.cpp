// MiniROAD host side: the forward entry points - argument checks, the choice between the chunked and the split pass, and the chunked
// pass.
#include "miniroad_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

// the side stream was created with the LEAST priority so that it never shares a hardware queue with a normal-priority caller (create);
// a caller's stream of that same priority might: two persistent launches that wait for each other must not be queued one behind the other
static bool side_queue_differs(const prego_miniroad* h, hipStream_t s) {
  int ps = 0, pside = 0;
  if (hipStreamGetPriority(s, &ps) != hipSuccess || hipStreamGetPriority(h->side, &pside) != hipSuccess) return false;
  return ps != pside;
}
static void refresh_placement(prego_miniroad* h) {
  if (h->placement < 0 && h->place_pending && hipEventQuery(h->ev_place) == hipSuccess) {
    const int v = (int)*h->pin_place;             // 1: group := XCD verified; 2: another placement; 0: that launch did not run the
    h->placement = v == 0 ? -1 : v;               // full-width rendezvous (multi-tile kernel): look again behind a later launch
    h->place_pending = false;
  }
}

int ant_head(prego_miniroad* h, const AntOut& ao, const void* HR, const SlotPlan& plan, int row0, int nrows, int flags, hipStream_t s) {
  if (!ao.wanted()) return PREGO_OK;
  const int MC = max_clips_of(h);
  float* const* d_ao = ao.out ? (float* const*)(h->d_ptrs + 4 * MC) : nullptr;
  int* const* d_aa = ao.arg ? (int* const*)(h->d_ptrs + 5 * MC) : nullptr;
  if (launch_ant_head(h->bf16, h->f16, HR, h->w_a, h->b_a, h->w_c, h->b_c, plan, row0, nrows, h->hid, h->ant_len, h->ncls,
                      (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, d_ao, d_aa, nullptr, s))
    return prego_fail_(PREGO_EINVAL, "anticipation head: unsupported shape (hid %d, L %d, num_classes %d)", h->hid, h->ant_len, h->ncls);
  return PREGO_OK;
}

// One forward call: the caller's arguments, and what validate_forward derives from them
struct FwdCall {
  int n_clips; const int32_t* lens; const float* const* rgb; const float* const* flow; float* const* out; int32_t* const* argmax;
  AntOut ao; const float* h0; float* h_last; int flags; void* workspace; size_t workspace_bytes; hipStream_t s;
  bool in16 = false;           // PREGO_FWD_IN16
  bool want_single = false;    // one clip per slot: h0 / h_last / PREGO_FWD_KEEP
  bool hostfeat = false;       // link-fed call (prego_miniroad_set_feed_events): the feature arrays are being filled over the host link while this call runs
  bool head_wanted() const { return out || argmax || ao.wanted(); }
};

static int validate_forward(prego_miniroad* h, FwdCall& c) {
  const int flags = c.flags;
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "forward before set_weights");
  if (h->layers == 2 && !h->have_layer2) return prego_fail_(PREGO_EINVAL, "forward of a 2-layer handle before set_gru_layer(1)");
  if ((flags & PREGO_FWD_KEEP) && !h->bf16 && h->hid == 2048)
    return prego_fail_(PREGO_EINVAL, "PREGO_FWD_KEEP (training) with hidden_dim 2048 needs bf16 operands (an fp32 W_hh slice of 2048 does not fit the register file)");
  if (c.n_clips <= 0 || !c.lens) return prego_fail_(PREGO_EINVAL, "no clips");
  if (c.n_clips > max_clips_of(h)) return prego_fail_(PREGO_EINVAL, "%d clips > max_clips %d per call", c.n_clips, max_clips_of(h));
  if (h->d_rgb > 0 && !c.rgb) return prego_fail_(PREGO_EINVAL, "rgb pointer array is NULL");
  if (!c.workspace) return prego_fail_(PREGO_EINVAL, "workspace is NULL");
  if (h->f16 && (flags & PREGO_FWD_KEEP))
    return prego_fail_(PREGO_EINVAL, "PREGO_FWD_KEEP (training) on an fp16-operand handle: training runs on bf16 / fp32 handles");
  if (h->x2 && (flags & PREGO_FWD_KEEP))
    return prego_fail_(PREGO_EINVAL, "PREGO_FWD_KEEP (training) on a split-operand (fp16x2) handle: training runs on bf16 / fp32 handles");
  c.in16 = (flags & PREGO_FWD_IN16) != 0;
  if (c.in16 && !h->bf16) return prego_fail_(PREGO_EINVAL, "PREGO_FWD_IN16 on an fp32-operand handle (16-bit features go with bf16 / fp16 handles)");
  if (c.in16 && (flags & PREGO_FWD_KEEP)) return prego_fail_(PREGO_EINVAL, "PREGO_FWD_IN16 with PREGO_FWD_KEEP: training takes fp32 features");
  c.want_single = c.h0 != nullptr || c.h_last != nullptr || (flags & PREGO_FWD_KEEP) != 0;
  c.hostfeat = !h->feed_ev.empty();
  if (c.hostfeat && c.want_single) { h->feed_ev.clear(); return prego_fail_(PREGO_EINVAL, "feed events with h0 / h_last / PREGO_FWD_KEEP: link-fed calls are plain inference"); }
  return PREGO_OK;
}

// split pass: the recurrence of the whole call on XCDs 0 .. R - 1 (16 R slots, continuous batching) and its feed-forward on
// the other XCDs, two persistent launches instead of a chain of launches per chunk.  Plain inference calls of 16-bit handles with
// enough clips to fill the slots and enough frames to amortise the pipeline fill; needs the verified placement (group := XCD) that an
// earlier full-width launch of this handle established, so a handle's first call is always the chunked pass.
// *split_r = 0: the chunked pass; R > 0: the split pass with the recurrence on R XCDs.  May wait for two events (the placement word of
// an earlier launch, the first measurement of a kind of pass) and records the start of a measured call.
static int choose_pass(prego_miniroad* h, const FwdCall& c, int* split_r_out) {
  prego_miniroad::Chooser& ch = h->chooser;
  const int n_clips = c.n_clips, flags = c.flags;
  const int32_t* lens = c.lens;
  const size_t workspace_bytes = c.workspace_bytes;
  hipStream_t s = c.s;
  int split_r = 0;
  ch.meas_armed = false;
  long long frames = 0;
  for (int i = 0; i < n_clips; ++i) frames += lens[i] > 0 ? lens[i] : 0;
  int r_try = ch.split_env > 0 ? ch.split_env : 3;       // unset: the candidate with the best estimate (below); 3 until estimated
  const bool with_flow_ = c.flow != nullptr && h->d_flow > 0 && c.flow[0] != nullptr;
  // everything but the placement (which a handle's first, chunked, call establishes)
  const bool shape_ok = ch.split_env != 0 && r_try >= 1 && r_try <= 6 && h->bf16 && h->hid == 1024 && h->layers == 1 && !c.want_single && !c.hostfeat && h->G == 8 && !h->no_local &&
                        h->side != nullptr && side_queue_differs(h, s) && n_clips >= 16 * r_try && frames >= 262144 &&
                        frames < (1ll << 31) - 65536 && c.head_wanted() && split_workspace_ok(h, r_try, workspace_bytes) &&
                        (h->d_rgb > 0 ? h->d_rgb : h->d_flow) >= 128 &&
                        (size_t)frames * (h->hid * 2 + 8) <= ((size_t)24 << 30) && split_resident_ok(h, frames);
  // a call of this class is worth one wait for the placement word of an earlier launch (the handle's second call otherwise races it)
  if (shape_ok && h->placement < 0 && h->place_pending) { (void)hipEventSynchronize(h->ev_place); refresh_placement(h); }
  bool backing_off = false;                       // a failed start handshake keeps the next eligible calls chunked
  if (shape_ok && ch.split_skip > 0) { --ch.split_skip; backing_off = true; }
  const bool eligible = shape_ok && h->placement == 1 && !backing_off;
  if (eligible && ch.split_env > 0) split_r = r_try;
  else if (shape_ok) {
    // cost model (ms), calibrated on the bench workloads.  Chunked pass: the plan's recurrence estimate + the feed-forward of
    // every row on the whole chip (projections at 1.4 PFLOP/s, 3 ns of LayerNorm + head; the pack hides under the recurrence) + 30 us
    // per chunk.  Split pass: the slower of the 16 R-slot recurrence at 2.0 us per step and the feed-forward on 8 - R of 8 XCDs (pack
    // included, at 5.3 TB/s), + 1.5 ms of pipeline fill and the head behind the pass.  Both are scaled by what passes of that kind
    // took on this device so far (measured / estimated, events around every call of this shape class).
    // while one of the two kinds has never been timed on this handle, the host waits here for the pending measurement (at most the
    // handle's first two calls of this class lose their run-ahead); afterwards measurements are picked up when they happen to be done
    // (only for the FIRST measurement of a kind: a handle whose model never trials the split pass stops waiting after one chunked call)
    if (ch.meas_pending && !(ch.meas_mode ? ch.have_ratio_split : ch.have_ratio_chunked)) (void)hipEventSynchronize(ch.ev_meas[1]);
    if (ch.meas_pending && hipEventQuery(ch.ev_meas[1]) == hipSuccess) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ch.ev_meas[0], ch.ev_meas[1]) == hipSuccess && ms > 0 && ch.meas_est > 0) {
        const double r = ms / ch.meas_est;
        double& ratio = ch.meas_mode ? ch.ratio_split : ch.ratio_chunked;
        bool& have = ch.meas_mode ? ch.have_ratio_split : ch.have_ratio_chunked;
        ratio = have ? 0.25 * ratio + 0.75 * r : r;
        have = true;
      }
      ch.meas_pending = false;
    }
    const int key = (with_flow_ ? 1 : 0) | (c.in16 ? 2 : 0) | (int)((workspace_bytes >> 20) << 2);
    if (!(key == ch.split_seen_key && (int)ch.split_seen_lens.size() == n_clips && std::equal(lens, lens + n_clips, ch.split_seen_lens.begin()))) {
      const double kx_ = h->d_rgb + (with_flow_ ? h->d_flow : 0), E_ = h->emb, H3 = 3.0 * h->hid;
      const double gemm_ns = (2.0 * kx_ * E_ + 2.0 * E_ * H3) / 1.4e15 * 1e9;
      const double pack_ns = kx_ * ((c.in16 ? 2.0 : 4.0) + 2.0) / 5.3e12 * 1e9;
      int rc0 = build_plan(h, n_clips, lens, false, 0, 0);
      if (rc0) return rc0;
      const RowBytes rb0 = row_bytes(h, with_flow_, flags);
      const double chunk_rows = std::max(1.0, (double)fwd_rows_fit(rb0, workspace_bytes));
      ch.split_seen_est_c = h->plan_cost_us * 1e-3 + frames * (gemm_ns + 3.0) * 1e-6 + 0.03 * std::ceil(frames / chunk_rows);
      // how many XCDs for the recurrence: more slots shorten it (steps = frames / 16 R once every slot is busy), fewer XCDs lengthen the
      // feed-forward: R = 3 balances the rgb + flow workload, a zero-flow call (half of layer1's K) is better off with R = 4
      ch.split_seen_est_s = 1e30; ch.split_seen_r = r_try;
      for (int r = 3; r <= 4; ++r) {
        if (n_clips < 16 * r || !split_workspace_ok(h, r, workspace_bytes)) continue;
        rc0 = build_plan(h, n_clips, lens, false, 0, 16 * r);
        if (rc0) return rc0;
        const double e = std::max(h->t_max * 2.0e-3, frames * (gemm_ns + pack_ns + 1.5) * 1e-6 * 8.0 / (8 - r)) + 1.5;
        if (e < ch.split_seen_est_s) { ch.split_seen_est_s = e; ch.split_seen_r = r; }
      }
      ch.split_seen_lens.assign(lens, lens + n_clips); ch.split_seen_key = key;
    }
    r_try = ch.split_seen_r;
    if (eligible) {
      // learning order: a chunked pass first (the handle's very first call does not count: kernels are still being loaded, and it ran
      // before the placement was known), then a split trial if the model says it is close, then the corrected comparison
      const double es = ch.split_seen_est_s * ch.ratio_split, ec = ch.split_seen_est_c * ch.ratio_chunked;
      if (!ch.have_ratio_chunked) split_r = 0;
      else if (!ch.have_ratio_split) split_r = es < 1.05 * ec ? r_try : 0;
      else split_r = es < 0.98 * ec ? r_try : 0;
    }
    if (eligible && !ch.meas_pending) {       // time this call (one measurement in flight at a time)
      ch.meas_armed = true; ch.meas_mode = split_r > 0 ? 1 : 0;
      ch.meas_est = split_r > 0 ? ch.split_seen_est_s : ch.split_seen_est_c;
      HIPCHK(hipEventRecord(ch.ev_meas[0], s));
    }
  }
  *split_r_out = split_r;
  return PREGO_OK;
}

// The two launches of a split pass could not run side by side (a profiler that serialises dispatches, another tenant on the XCDs) and left
// before touching anything; the call is re-run as a chunked pass.  Back-off: the next 16, then 64 eligible calls stay chunked, a third
// failure keeps the handle chunked for good
static void note_split_fallback(prego_miniroad* h) {
  prego_miniroad::Chooser& ch = h->chooser;
  ch.split_fails++; ch.split_fallbacks++;
  if (ch.split_fails >= 3) ch.split_env = 0;
  else ch.split_skip = 16ll << (2 * (ch.split_fails - 1));
}

// the call's pointer tables -> device (rows of h->d_ptrs)
static int stage_call_tables(prego_miniroad* h, const FwdCall& c, FwdTables* tb) {
  const int MC = max_clips_of(h);
  bool any_flow = false;
  std::vector<const void*> tab((size_t)(c.ao.call ? 6 : 4) * MC, nullptr);
  for (int i = 0; i < c.n_clips; ++i) {
    tab[0 * MC + i] = c.rgb ? c.rgb[i] : nullptr;
    if (h->d_rgb > 0 && !tab[i]) return prego_fail_(PREGO_EINVAL, "rgb[%d] is NULL", i);
    tab[1 * MC + i] = (c.flow && h->d_flow > 0) ? c.flow[i] : nullptr;
    any_flow |= tab[1 * MC + i] != nullptr;
    tab[2 * MC + i] = c.out ? c.out[i] : nullptr;
    tab[3 * MC + i] = c.argmax ? c.argmax[i] : nullptr;
    if (c.ao.call) {
      tab[4 * MC + i] = c.ao.out ? c.ao.out[i] : nullptr;
      tab[5 * MC + i] = c.ao.arg ? c.ao.arg[i] : nullptr;
    }
  }
  const int rc = stage_tables(h, tab.data(), tab.size(), c.s);
  if (rc) return rc;
  tb->rgb = h->d_rgb > 0 ? (const float* const*)(h->d_ptrs + 0 * MC) : nullptr;
  tb->flow = any_flow ? (const float* const*)(h->d_ptrs + 1 * MC) : nullptr;
  tb->out = c.out ? (float* const*)(h->d_ptrs + 2 * MC) : nullptr;
  tb->arg = c.argmax ? (int* const*)(h->d_ptrs + 3 * MC) : nullptr;
  return PREGO_OK;
}

// XCD overlap: a recurrence launch is compacted (so that the next chunk's layer1 GEMM gets the other XCDs) while its live slots fit at
// most this many groups; 7 of 8 measured best (DESIGN_HISTORY)
static constexpr int kOverlapMaxGroups = 7;

// The chunked pass: as many time steps per chunk as the workspace holds rows for, per chunk
//   pack -> GEMM(layer1) -> LayerNorm+ReLU -> GEMM(W_ih) -> recurrence -> head,
// with the next chunk's pack (and, on a verified placement, its layer1 GEMM) on the side stream under this chunk's recurrence.
static int run_chunked_pass(prego_miniroad* h, const FwdCall& c, const SlotPlan& plan, const FwdTables& tb, int kx) {
  const int n_clips = c.n_clips, flags = c.flags, n_slots = h->n_slots;
  float* const* out = c.out; int32_t* const* argmax = c.argmax; const AntOut& ao = c.ao;
  const float* h0 = c.h0; float* h_last = c.h_last;
  const bool in16 = c.in16, hostfeat = c.hostfeat, ant_wanted = ao.wanted(), with_flow = tb.flow != nullptr;
  hipStream_t s = c.s;
  const int din = h->d_rgb + h->d_flow;
  const int total_rows = h->h_rowoff[h->t_max];
  const RowBytes rb = row_bytes(h, with_flow, flags);
  if (c.workspace_bytes < fwd_bytes_for_rows(rb, 1)) return prego_fail_(PREGO_EWORKSPACE, "workspace %zu B is too small", c.workspace_bytes);
  const FwdLayout F = fwd_layout(h, with_flow, flags, c.workspace_bytes);
  const long long cap_rows = F.cap_rows;
  if (cap_rows < n_slots) return prego_fail_(PREGO_EWORKSPACE, "workspace holds %lld rows, need >= %d (one time step)", cap_rows, n_slots);
  if ((flags & PREGO_FWD_KEEP) && cap_rows < total_rows)
    return prego_fail_(PREGO_EWORKSPACE, "PREGO_FWD_KEEP needs the whole batch resident: %d rows, workspace holds %lld", total_rows, cap_rows);
  void* const ws = c.workspace;
  void* X = ws; void* Y = F.at(ws, F.Y); void* Eb = F.at(ws, F.E); void* GI = F.at(ws, F.GI); void* HR = F.at(ws, F.HR);
  char* RM = (char*)F.at(ws, F.RM);
  // The classifier once per pass.  A pass of many chunks pays the head kernel's launch, its fill and its scatter per chunk (split
  // operands: 71 launches of the fp32 head = 10.3 ms of a 280 ms pass; 16-bit operands: 47 x ~123 us): with relu(h) of the whole call
  // resident - 4 KB (fp32 / fp16x2) or 2 KB per frame in the CALLER's resident buffer (prego_miniroad_set_resident) - ONE launch behind
  // the last chunk does the same work at its HBM rate.  Inference calls of one GRU layer whose rows span four or more chunks; a link-fed
  // call keeps the per-chunk head (its last chunk ends with the link, and a whole-pass head behind it would be pure tail); no resident
  // buffer, or one that is too small = per-chunk head.  Nothing is allocated and nothing is waited for here.
  bool defer_head = false;
  char* HRall = nullptr;
  if (!(flags & PREGO_FWD_KEEP) && !hostfeat && h->layers == 1 && (out || argmax || ant_wanted) && (long long)total_rows >= 4 * cap_rows &&
      (size_t)total_rows * rb.hr <= ((size_t)24 << 30)) {
    const size_t need = align_up((size_t)total_rows * rb.hr, 256);
    if (h->res_buf && need <= h->res_bytes) { defer_head = true; HRall = h->res_buf; }
  }
  const bool i16 = inter16(h, flags);
  // projection with fp32 or bf16 output: ping-pong kernel for whole-chip shapes, the 128x128 kernel with a bf16-store epilogue below
  auto proj = [&](const void* A, int lda, const void* Wt, int ldb, const float* bias, void* Cout, int ldc, int M, int N, int K) {
    if (h->x2) {                    // A rows [K hi | K lo] (lda = K), W rows [ldb hi | ldb lo]: three fp16 products, fp32 C
      const float* inv = h->x2_scale + (Wt == h->w1 ? 1 : 3);
      (void)launch_gemm_x2_pingpong(A, 2 * lda, lda, Wt, 2 * ldb, ldb, inv, bias, (float*)Cout, ldc, M, N, K, s);
      return;
    }
    if (!h->bf16) { launch_gemm_f32_nt((const float*)A, lda, (const float*)Wt, ldb, bias, (float*)Cout, ldc, M, N, K, s); return; }
    GemmEpi epi{};
    epi.f16 = h->f16 ? 1 : 0;
    if (i16) { epi.mode = EPI_STORE_BF16; epi.out_b = Cout; } else epi.mode = EPI_STORE;
    launch_gemm_nt(!i16 && !h->f16 ? GEMM_NT_PLAIN : GEMM_NT_PROJ16, A, lda, Wt, ldb, bias, i16 ? nullptr : (float*)Cout, ldc, M, N, K, epi,
                   (flags & PREGO_FWD_KEEP) != 0, s);
  };
  const bool keep = (flags & PREGO_FWD_KEEP) != 0;
  if (keep) {
    if (h0) return prego_fail_(PREGO_EINVAL, "PREGO_FWD_KEEP (training) runs from h0 = 0 (rnn.py:49,60): h0 must be NULL");
    h->kept_kx = kx; h->kept_rows = total_rows;
    h->ant_kept = ao.call;
  }
  // what the backward reads again (NULL without PREGO_FWD_KEEP): raw state, gate activations, LayerNorm statistics; with two layers
  // layer 0's h_t and layer 1's raw state and gates
  float* HRAW = (float*)F.at(ws, F.HRAW); float* STATS = (float*)F.at(ws, F.STATS);
  float* KR = (float*)F.at(ws, F.KR); float* KZ = (float*)F.at(ws, F.KZ); float* KN = (float*)F.at(ws, F.KN); float* KG = (float*)F.at(ws, F.KG);
  void* HR0 = F.at(ws, F.HR0); float* HRAW2 = (float*)F.at(ws, F.HRAW2);
  float* KR2 = (float*)F.at(ws, F.KR2); float* KZ2 = (float*)F.at(ws, F.KZ2); float* KN2 = (float*)F.at(ws, F.KN2); float* KG2 = (float*)F.at(ws, F.KG2);
  // initial state (sorted order)
  const int H = h->hid, E = h->emb;
  // state of layer l: h_state + l * slot_stride; h0 / h_last of a 2-layer handle are [layers][n_clips][H] (nn.GRU's h_0 / h_n layout)
  const size_t slot_stride = (size_t)max_slots_of(h) * H;
  for (int l = 0; l < h->layers; ++l) {
    if (h0) launch_permute_rows(h0 + (size_t)l * n_clips * H, h->h_state + l * slot_stride, h->d_sorted, n_slots, H, 1, s);        // one clip per slot here
    else HIPCHK(hipMemsetAsync(h->h_state + l * slot_stride, 0, (size_t)n_slots * H * 4, s));
  }

  const int slots = (n_slots + h->G - 1) / h->G;
  const int nct = (slots + 15) / 16;          // live 16-clip tiles per group (kernels: 1, 2, 4, 8)

  // chunk [t0, t1): the largest t1 with rowoff[t1] - rowoff[t0] <= cap_rows
  auto chunk_end = [&](int t0_) {
    const int base_ = h->h_rowoff[t0_];
    int t1_ = (int)(std::upper_bound(h->h_rowoff.begin() + t0_, h->h_rowoff.end(), base_ + (int)std::min<long long>(cap_rows, total_rows)) -
                    h->h_rowoff.begin()) - 1;
    if (t1_ <= t0_) t1_ = t0_ + 1;
    if (t1_ > h->t_max) t1_ = h->t_max;
    return t1_;
  };
  auto pack_chunk = [&](int t0_, int t1_, hipStream_t st, int ci_) {
    const int base_ = h->h_rowoff[t0_], rows_ = h->h_rowoff[t1_] - base_;
    // link-fed call: this chunk reads rows of steps < t1_; make the packing stream wait for every feed event that covers them
    while (h->feed_pos < h->feed_ev.size() && (h->feed_pos == 0 || h->feed_upto[h->feed_pos - 1] < t1_)) {
      (void)hipStreamWaitEvent(st, h->feed_ev[h->feed_pos], 0);
      ++h->feed_pos;
    }
    EventPair* evp = ev_begin(h, 2, st);
    if (h->x2)
      launch_pack_rows_x2(tb.rgb, tb.flow, plan, base_, rows_, h->d_rgb, with_flow ? h->d_flow : 0, X, st,
                          st == s ? 0 : h->prefetch_grid, RM + (size_t)(ci_ & 1) * cap_rows * 8);
    else
    launch_pack_rows(h->bf16, tb.rgb, tb.flow, plan, base_, rows_, h->d_rgb, with_flow ? h->d_flow : 0, X, st,
                     st == s ? 0 : h->prefetch_grid, RM + (size_t)(ci_ & 1) * cap_rows * 8, h->f16, in16);
    ev_end(evp, st);
    if (h->timing) h->pack_bytes += (double)rows_ * (kx * (in16 ? 2.0 : 4.0) + rb.x);
  };
  const bool prefetch = h->pack_prefetch && !keep && h->side != nullptr;
  bool packed = false;            // X already holds this chunk (packed on the side stream under the previous recurrence)
  bool l1_done = false;           // Y already holds layer1 of this chunk (XCD overlap: the worker GEMM ran under the previous recurrence)
  refresh_placement(h);
  const bool overlap_ok = h->xcd_overlap && prefetch && i16 && h->bf16 && h->G == 8 && h->placement == 1 && !h->no_local && h->layers == 1 && h->hid == 1024;
  if (overlap_ok) HIPCHK(hipMemsetAsync(h->tile_ctr, 0, 4096 * sizeof(unsigned), s));
  // every exit path after a fork joins the side stream: an error return while the next chunk's pack is still writing X / RM
  // would leave the caller's stream unordered against it (the next forward on this handle could race with that pack)
  struct SideJoin {
    prego_miniroad* h; bool pending = false;
    ~SideJoin() { if (pending) (void)hipStreamSynchronize(h->side); }
  } side_join{h};
  int t0 = 0, ci = 0;             // ci: chunk counter (parity of the row-map half)
  while (t0 < h->t_max) {
    const int base = h->h_rowoff[t0];
    const int t1 = chunk_end(t0);
    const int rows = h->h_rowoff[t1] - base;
    EventPair* ev;
    if (!packed) pack_chunk(t0, t1, s, ci);
    packed = false;

    if (!l1_done) {
      ev = ev_begin(h, 0, s);
      proj(X, kx, h->w1, din, h->b1, Y, E, rows, E, kx);
      ev_end(ev, s);
      if (h->timing) h->gemm_flop += 2.0 * rows * (double)E * kx;
    }
    l1_done = false;
    // the LayerNorm launch also re-arms the recurrence's exchange buffers and rendezvous words (it runs after the previous recurrence
    // launch of this stream and before the next): one launch and one launch gap fewer per chunk than a separate arm launch
    const GruArm arm = h->x2 ? gru_x2_arm_desc(h->hid, h->G, h->hx, h->no_local ? nullptr : h->flags)
                             : gru_arm_desc(h->bf16, h->hid, h->G, h->hx, h->no_local ? nullptr : h->flags);
    if (h->x2) launch_ln_relu_x2((const float*)Y, h->ln_g, h->ln_b, rows, E, 1e-5f, Eb, s, &arm);
    else
    launch_ln_relu(h->bf16, Y, h->ln_g, h->ln_b, rows, E, 1e-5f, Eb, STATS, keep ? h->drop_p : 0.f, h->drop_seed, base, s, 1, i16, h->f16,
                   &arm);
    ev = ev_begin(h, 0, s);
    proj(Eb, E, h->w_ih, E, h->bias2, GI, 3 * H, rows, 3 * H, E);
    ev_end(ev, s);
    if (h->timing) h->gemm_flop += 2.0 * rows * 3.0 * H * E;

    GruArgs ga{};
    ga.whh = h->w_hh; ga.b_hn = h->b_hn; ga.gi = GI; ga.gi_bf16 = i16 ? 1 : 0; ga.f16 = h->f16 ? 1 : 0; ga.h_raw_out = HRAW;
    ga.h_relu_out = defer_head ? (void*)(HRall + (size_t)base * rb.hr) : HR;        // the kernels index relu(h) by chunk-relative row
    ga.h_state = h->h_state; ga.hx = h->hx; ga.flags = h->flags; ga.abort_word = h->abort_word;
    ga.rowoff = h->d_rowoff; ga.nact = h->d_nact; ga.t0 = t0; ga.t1 = t1; ga.row_base = base; ga.rows = rows;
    ga.keep_r = KR; ga.keep_z = KZ; ga.keep_n = KN; ga.keep_ghn = KG;
    ga.n_clips = n_slots; ga.G = h->G; ga.seg_off = h->plan_single ? nullptr : h->d_seg_off;
    ga.seg_start = h->plan_single ? nullptr : h->d_seg_start; ga.stamps = h->use_stamps ? h->stamps : nullptr;
    ga.sync = h->no_local ? nullptr : h->flags;   // flags[0..15] double as the rendezvous words
    ga.armed = rows > 0 ? 1 : 0;
    ga.no_mt = h->no_mt ? 1 : 0;
    ga.out_floor = h->layers == 2 ? -INFINITY : 0.f;      // 2 layers: layer 0 hands h_t itself to layer 1 (below)
    if (HR0) ga.h_relu_out = HR0;                         // ... and when training, into a buffer of its own (backward needs it again)
    // full width unless the XCD overlap below compacts this launch: spreading the live slots over all groups is 2.6 ms per pass faster than
    // packing them into the fewest (the step cost grows with the fullest group's columns)
    ga.Gd = 0;
    const bool prefetch_next = prefetch && t1 < h->t_max;
    // XCD overlap: when the live slots fit fewer than eight groups, this launch is compacted onto XCDs 0 .. Gd - 1
    // and the NEXT chunk's layer1 GEMM runs as a persistent worker on the side stream behind its pack: its workgroups can only be
    // dispatched where no recurrence workgroup is resident, i.e. on the free XCDs, until this launch ends; the tile queue balances
    bool ov = false;
    if (overlap_ok && prefetch_next && ci + 1 < 4096) {
      const int live0 = h->h_nact[t0];
      const int gd0 = (live0 + 15) / 16;
      const int rows_n = h->h_rowoff[chunk_end(t1)] - h->h_rowoff[t1];
      if (live0 <= 16 * h->G && gd0 < h->G && gd0 <= kOverlapMaxGroups && rows_n >= 4096) {
        // how many groups?  The fewest (gd0) frees the most XCDs; more groups mean fewer columns per group and a faster step
        // (1.67 us + 0.0102 us per live column of the fullest group).  Take the widest spread that still leaves the worker enough
        // XCD-time for the whole layer1 GEMM of the next chunk (13 ns per row on the whole chip, probe: >= proportional on a part)
        const double l1_ms = rows_n * 13.0e-6;
        int pick = std::max(1, gd0);
        for (int g2 = h->G - 1; g2 > pick; --g2) {      // (always the fewest groups instead: 127.2 vs 125.5 ms on the same device)
          const double rec_ms = (t1 - t0) * (1.67 + 0.0102 * ((live0 + g2 - 1) / g2)) * 1e-3;
          if (l1_ms * h->G / (h->G - g2) <= 0.85 * rec_ms) { pick = g2; break; }
        }
        ov = true; ga.Gd = pick;
      }
    }
    ev = ev_begin(h, 1, s);
    if (prefetch_next) HIPCHK(hipEventRecord(h->ev_fork, s));      // fork point: everything before the recurrence launch
    // clip tiles per group that are still alive at this launch's first step (nact never grows): later launches of a pass whose
    // slots have thinned out run the kernels for fewer tiles (fewer registers; one tile = the classic kernel)
    const int live_slots = h->h_nact[t0];
    const int nct_l = std::max(1, std::min(nct, (((live_slots + h->G - 1) / h->G) + 15) / 16));
    if (h->x2 ? launch_gru_recurrence_x2(H, nct_l, ga, h->x2_scale + 5, s) : launch_gru_recurrence(h->bf16, H, nct_l, ga, s))
      return prego_fail_(PREGO_EINVAL, "recurrence: unsupported hid=%d nct=%d", H, nct_l);
    if (h->placement < 0 && !h->place_pending && h->xcd_overlap && h->bf16 && h->G == 8 && !h->no_local && ga.Gd == 0) {
      // the first full-width launch writes the verified-placement word: mirror it to the host behind that launch
      HIPCHK(hipMemcpyAsync(h->pin_place, h->flags + 20, sizeof(unsigned), hipMemcpyDeviceToHost, s));
      HIPCHK(hipEventRecord(h->ev_place, s));
      h->place_pending = true;
    }
    ev_end(ev, s);
    if (prefetch_next) {
      // X is dead once the layer1 GEMM of this chunk has run: stream the next chunk's features into it while the recurrence
      // (latency-bound, one wave per SIMD) holds the CUs.  The recurrence is launched FIRST so that its 256 workgroups are
      // resident (placement rendezvous) before the copy's workgroups fill the wave slots
      HIPCHK(hipStreamWaitEvent(h->side, h->ev_fork, 0));
      pack_chunk(t1, chunk_end(t1), h->side, ci + 1);
      side_join.pending = true;
      if (ov) {
        const int rows_n = h->h_rowoff[chunk_end(t1)] - h->h_rowoff[t1];
        EventPair* evw = ev_begin(h, 3, h->side);       // kind 3: overlapped worker (its span includes waiting for the recurrence's XCDs)
        if (launch_gemm_bf16_pingpong_worker(X, kx, h->w1, din, h->b1, Y, E, rows_n, E, kx, 0, h->tile_ctr + (ci + 1), 256, h->side, true, h->f16) == 0)
          l1_done = true;
        ev_end(evw, h->side);
      }
      HIPCHK(hipEventRecord(h->ev_join, h->side));
      packed = true;
    }

    if (h->layers == 2) {
      // second GRU layer (nn.GRU num_layers = 2, rnn.py:38,61): its input is layer 0's h_t - the first launch stored h_t itself
      // (out_floor = -inf) in HR -, GI and HR are reused in place: gi' = h W_ih_l1^T + b (GI of layer 0 is dead), then the recurrence of
      // layer 1 over the same steps from its own state, relu(h'_t) -> HR for the classifier
      ev = ev_begin(h, 0, s);
      proj(HR0 ? HR0 : HR, H, h->l2_w_ih, H, h->l2_bias2, GI, 3 * H, rows, 3 * H, H);
      ev_end(ev, s);
      if (h->timing) h->gemm_flop += 2.0 * rows * 3.0 * H * H;
      GruArgs g2 = ga;
      g2.whh = h->l2_w_hh; g2.b_hn = h->l2_b_hn; g2.h_state = h->h_state + slot_stride; g2.out_floor = 0.f;
      if (HR0) { g2.h_relu_out = HR; g2.h_raw_out = HRAW2; g2.keep_r = KR2; g2.keep_z = KZ2; g2.keep_n = KN2; g2.keep_ghn = KG2; }
      g2.armed = 0;                 // the exchange buffers / rendezvous words were used by layer 0's launch: re-arm (launcher)
      g2.Gd = 0;
      ev = ev_begin(h, 1, s);
      if (launch_gru_recurrence(h->bf16, H, nct_l, g2, s)) return prego_fail_(PREGO_EINVAL, "recurrence (layer 1): unsupported hid=%d nct=%d", H, nct_l);
      ev_end(ev, s);
    }
    if ((out || argmax) && !defer_head) {
      if (launch_head_softmax(h->bf16, HR, h->w_c, h->b_c, plan, base, rows, H, h->ncls,
                              (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, tb.out, tb.arg, s, RM + (size_t)(ci & 1) * cap_rows * 8, h->f16))
        return prego_fail_(PREGO_EINVAL, "head: unsupported num_classes %d", h->ncls);
    }
    if (ant_wanted && !defer_head) {
      if (int rc_a = ant_head(h, ao, HR, plan, base, rows, flags, s)) return rc_a;
    }
    if (packed) { HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0)); side_join.pending = false; }
    t0 = t1;
    ++ci;
  }
  if (defer_head) {                      // the classifier of the whole call, once (16-bit operands: no row map at hand - the kernel looks rows up in the plan)
    if ((out || argmax) && launch_head_softmax(h->bf16, HRall, h->w_c, h->b_c, plan, 0, total_rows, H, h->ncls, (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, tb.out,
                            tb.arg, s, nullptr, h->f16))
      return prego_fail_(PREGO_EINVAL, "head: unsupported num_classes %d", h->ncls);
    if (int rc_a = ant_head(h, ao, HRall, plan, 0, total_rows, flags, s)) return rc_a;
  }
  if (h_last)
    for (int l = 0; l < h->layers; ++l) launch_permute_rows(h->h_state + l * slot_stride, h_last + (size_t)l * n_clips * H, h->d_sorted, n_slots, H, 0, s);
  if (hostfeat && (h->feed_upto.empty() || h->feed_upto.back() < h->t_max))
    return prego_fail_(PREGO_EINVAL, "feed events cover steps < %d, the call has %d", h->feed_upto.empty() ? 0 : h->feed_upto.back(), h->t_max);
  if (h->chooser.meas_armed) { HIPCHK(hipEventRecord(h->chooser.ev_meas[1], s)); h->chooser.meas_pending = true; h->chooser.meas_armed = false; }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// prego_miniroad_forward and prego_miniroad_forward_anticipation (c.ao.call)
static int forward_impl(prego_miniroad* h, FwdCall c) {
  HandleScope scope_(h);
  if (int rc = validate_forward(h, c)) return rc;
  struct FeedClear { prego_miniroad* h; ~FeedClear() { h->feed_ev.clear(); h->feed_upto.clear(); h->feed_pos = 0; } } feed_clear{h};   // one call only
  refresh_placement(h);
  int split_r = 0;
  if (int rc = choose_pass(h, c, &split_r)) return rc;
  h->split_r = split_r;
  if (int rc = build_plan(h, c.n_clips, c.lens, c.want_single, c.hostfeat ? h->feed_row_bytes : 0, split_r > 0 ? 16 * split_r : 0)) return rc;
  const SlotPlan plan = device_plan(h);
  FwdTables tb{};
  if (int rc = stage_call_tables(h, c, &tb)) return rc;
  const bool with_flow = tb.flow != nullptr;
  const int kx = h->d_rgb + (with_flow ? h->d_flow : 0);      // K of the layer1 GEMM actually multiplied
  if (kx == 0) return prego_fail_(PREGO_EINVAL, "a model without rgb features (--no_rgb) needs the flow tensors");
  if (split_r == 0) return run_chunked_pass(h, c, plan, tb, kx);
  bool fell_back = false;
  const int rc = forward_split(h, c.ao, split_r, c.flags, with_flow, c.in16, kx, plan, tb, c.workspace, c.workspace_bytes, c.s, &fell_back);
  if (rc || !fell_back) return rc;
  // the two launches left before touching anything: THIS call runs as a chunked pass, right here, behind them in the stream (the chooser
  // is backing off now and returns 0)
  note_split_fallback(h);
  return forward_impl(h, c);
}

extern "C" int prego_miniroad_forward(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* rgb,
                                      const float* const* flow, float* const* out, int32_t* const* argmax,
                                      const float* h0, float* h_last, int flags, void* workspace,
                                      size_t workspace_bytes, prego_stream_t stream) {
  return forward_impl(h, FwdCall{n_clips, lens, rgb, flow, out, argmax, AntOut{}, h0, h_last, flags, workspace, workspace_bytes, (hipStream_t)stream});
}

extern "C" int prego_miniroad_forward_anticipation(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* rgb,
                                                   const float* const* flow, float* const* out, int32_t* const* argmax,
                                                   float* const* ant_out, int32_t* const* ant_argmax, const float* h0, float* h_last,
                                                   int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  {
    HandleScope scope_(h);
    if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
    if (h->ant_len <= 0 || !h->w_a) return prego_fail_(PREGO_EINVAL, "forward_anticipation before set_anticipation");
    if ((flags & PREGO_FWD_KEEP) && (h->f16 || h->x2))
      return prego_fail_(PREGO_EINVAL, "forward_anticipation: PREGO_FWD_KEEP (MiniROADA training) on an fp16 / fp16x2-operand handle: training runs on bf16 / fp32 handles");
    if ((flags & PREGO_FWD_KEEP) && (flags & PREGO_FWD_SOFTMAX))
      return prego_fail_(PREGO_EINVAL, "forward_anticipation: PREGO_FWD_KEEP returns raw logits (rnn.py:128-130): PREGO_FWD_SOFTMAX is not taken with it");
  }
  AntOut ao;
  ao.call = true; ao.out = ant_out; ao.arg = ant_argmax;
  return forward_impl(h, FwdCall{n_clips, lens, rgb, flow, out, argmax, ao, h0, h_last, flags, workspace, workspace_bytes, (hipStream_t)stream});
}

#ifdef PREGO_DEBUG_ABI
// debug / probe: ONLY the recurrence kernel, one launch over n_steps steps of n_slots equally long slots dealt to `gd` groups
// (0 = all), on caller-supplied gi rows [n_steps * n_slots][3H] (16-bit, the handle's operand type) -> relu(h) [rows][H].
// scripts/probes/xcd_overlap_probe.py runs it beside an XCD-filtered GEMM worker.
extern "C" int prego_debug_recurrence_only(prego_miniroad* h, int n_slots, int n_steps, int gd, const void* gi, void* h_relu,
                                           prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !gi || !h_relu) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (!h->have_weights || !h->bf16) return prego_fail_(PREGO_EINVAL, "debug recurrence: a bf16 / fp16 handle with weights");
  if (n_slots < 1 || n_slots > 16 * h->G || n_steps < 1) return prego_fail_(PREGO_EINVAL, "debug recurrence: %d slots, %d steps", n_slots, n_steps);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> lens((size_t)n_slots, n_steps);
  int rc = build_plan(h, n_slots, lens.data(), true);
  if (rc) return rc;
  std::vector<const void*> tab((size_t)4 * max_clips_of(h), nullptr);
  rc = stage_tables(h, tab.data(), tab.size(), s);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(h->h_state, 0, (size_t)n_slots * h->hid * 4, s));
  GruArgs ga{};
  ga.whh = h->w_hh; ga.b_hn = h->b_hn; ga.gi = gi; ga.gi_bf16 = 1; ga.f16 = h->f16 ? 1 : 0; ga.h_relu_out = h_relu; ga.h_raw_out = nullptr;
  ga.h_state = h->h_state; ga.hx = h->hx; ga.flags = h->flags; ga.abort_word = h->abort_word;
  ga.rowoff = h->d_rowoff; ga.nact = h->d_nact; ga.t0 = 0; ga.t1 = n_steps; ga.row_base = 0; ga.rows = n_slots * n_steps;
  ga.n_clips = n_slots; ga.G = h->G; ga.Gd = gd; ga.seg_off = nullptr; ga.seg_start = nullptr; ga.stamps = nullptr;
  ga.sync = h->no_local ? nullptr : h->flags;
  if (launch_gru_recurrence(true, h->hid, 1, ga, s)) return prego_fail_(PREGO_EINVAL, "debug recurrence: launch failed");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// debug / probe: ONLY the head kernel (relu(h) rows -> probabilities + argmax) over n_slots equal slots x n_steps steps;
// out [n_slots][n_steps][C] fp32, argmax [n_slots][n_steps].  scripts/probes/head_probe.py
extern "C" int prego_debug_head_only(prego_miniroad* h, int n_slots, int n_steps, const void* h_relu, float* out, int32_t* argmax,
                                     const void* rowmap, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !h_relu || !out || !argmax) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (!h->have_weights || !h->bf16) return prego_fail_(PREGO_EINVAL, "debug head: a bf16 / fp16 handle with weights");
  if (n_slots < 1 || n_slots > max_clips_of(h) || n_steps < 1) return prego_fail_(PREGO_EINVAL, "debug head: %d slots, %d steps", n_slots, n_steps);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> lens((size_t)n_slots, n_steps);
  int rc = build_plan(h, n_slots, lens.data(), true);
  if (rc) return rc;
  const SlotPlan plan = device_plan(h);
  const int MC = max_clips_of(h);
  std::vector<const void*> tab((size_t)4 * MC, nullptr);
  for (int i = 0; i < n_slots; ++i) {
    tab[2 * MC + i] = out + (size_t)i * n_steps * h->ncls;
    tab[3 * MC + i] = argmax + (size_t)i * n_steps;
  }
  rc = stage_tables(h, tab.data(), tab.size(), s);
  if (rc) return rc;
  if (launch_head_softmax(true, h_relu, h->w_c, h->b_c, plan, 0, n_slots * n_steps, h->hid, h->ncls, 1, (float* const*)(h->d_ptrs + 2 * MC),
                          (int* const*)(h->d_ptrs + 3 * MC), s, rowmap, h->f16))
    return prego_fail_(PREGO_EINVAL, "debug head: unsupported num_classes %d", h->ncls);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_split_state(const prego_miniroad* h, int64_t* fallbacks, int32_t* fails, int64_t* skip, int32_t* split_env) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (fallbacks) *fallbacks = h->chooser.split_fallbacks;
  if (fails) *fails = h->chooser.split_fails;
  if (skip) *skip = h->chooser.split_skip;
  if (split_env) *split_env = h->chooser.split_env;
  return PREGO_OK;
}
#endif  // PREGO_DEBUG_ABI
