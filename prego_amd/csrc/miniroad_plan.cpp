// MiniROAD host side: the packing plan of a call (sort clips by length, packed time-major rows, slots), its device tables, the feed
// events of a link-fed call, and the layout of the forward workspace.
#include "miniroad_handle.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

// ---- plan -------------------------------------------------------------------------------------
// recurrence cost per time step (us) by live 16-clip tiles per group, measured (scripts/probes/slot_sweep.sh, round 2: 512 clips x
// 512 frames forced into 128 / 256 / 512 slots = 2.01 / 4.03 / 8.55 us per step): the tiles of a step run one after the other,
// so the cost is linear in the tile count and the fewest slots that cover the clips win unless a longer slot chain dominates
// Round 3: two or more tiles run on the software-pipelined kernel (gru_recurrence_mt_kernel): 2.0 / 3.84 / 7.41 us per step for
// 1 / 2 / 4 tiles (scripts/probes/mt_ab2.sh; the classic kernel: 2.0 / 3.99 / 8.47 on the same device).
static const double kStepCost[5] = {0.0, 2.0, 3.84, 5.7, 7.41};
// Round 4, the 64-workgroup groups (G = 4): split fp16 operands 3.14 / 4.64 us for 1 / 2 tiles (two tiles at most), exact-fp32 operands
// 6.89 / 9.25 (bench workload forced into 64 / 128 slots, PREGO_PLAN_SLOTS; three and four tiles extrapolated): a second tile costs
// less than the first there (its gather rides under the first tile's MFMAs), so equal-length batches prefer more slots than the
// 16-bit table would choose
static const double kStepCostX2[5] = {0.0, 3.14, 4.64, 1e9, 1e9};
static const double kStepCostF32[5] = {0.0, 6.89, 9.25, 11.6, 14.0};

// Slot schedule.  want_single: one clip per slot (needed when the caller passes h0 / h_last or keeps activations for
// backward); otherwise the clips are packed longest-first into the number of slots (128 / 256 / 512 for bf16) that
// minimises the estimated recurrence time: sequential steps = max(longest clip, frames / slots).
// host_row_bytes > 0: the features live in pinned HOST memory and every packed row costs that many bytes over PCIe (PREGO_FWD_HOSTFEAT):
// a step can then be bound by the link - live slots x row bytes at ~50 GB/s - instead of by the recurrence, and the slot count that
// minimises the pass is the one that keeps the link evenly busy for the whole run (about frames / longest clip slots: every slot
// alive to the end), not the one that minimises the number of steps.
int build_plan(prego_miniroad* h, int n, const int32_t* lens, bool want_single, int host_row_bytes, int slots_arg) {
  if ((int)h->plan_lens.size() == n && std::equal(lens, lens + n, h->plan_lens.begin()) && h->plan_want_single == want_single &&
      h->plan_host_row_bytes == host_row_bytes && h->plan_force_slots == slots_arg)
    return PREGO_OK;
  long long total = 0;
  int lmax = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] <= 0) return prego_fail_(PREGO_EINVAL, "clip %d has %d frames", i, lens[i]);
    lmax = std::max(lmax, lens[i]);
    total += lens[i];
  }
  if (total >= (1ll << 31)) return prego_fail_(PREGO_EINVAL, "more than 2^31 frames in one call");
  const int per_layer = h->G * 16, max_slots = max_slots_of(h);
  if (want_single && n > max_slots) return prego_fail_(PREGO_EINVAL, "%d clips > %d per call when h0/h_last/training is used", n, max_slots);
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });

  // candidate slot counts; LPT packing; exact cost = sum over steps of cost(live tiles)
  struct Cand { int S; std::vector<std::vector<int>> bins; std::vector<long long> load; double cost; };
  auto pack = [&](int S) {
    Cand c; c.S = S; c.bins.assign(S, {}); c.load.assign(S, 0);
    // min-heap on (load, slot)
    std::vector<std::pair<long long, int>> heap;
    for (int i = 0; i < S; ++i) heap.push_back({0, i});
    auto cmp = [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int idx : order) {
      std::pop_heap(heap.begin(), heap.end(), cmp);
      auto top = heap.back(); heap.pop_back();
      c.bins[top.second].push_back(idx);
      c.load[top.second] += lens[idx];
      top.first += lens[idx];
      heap.push_back(top); std::push_heap(heap.begin(), heap.end(), cmp);
    }
    std::vector<long long> sorted_load = c.load;
    std::sort(sorted_load.begin(), sorted_load.end(), std::greater<long long>());
    const double* tab = h->x2 ? kStepCostX2 : h->bf16 ? kStepCost : kStepCostF32;
    double cost = 0; long long prev = 0;
    if (host_row_bytes <= 0) {
      const int layers = (S + per_layer - 1) / per_layer;
      for (int k = layers - 1; k >= 0; --k) {            // layer k lives as long as its most loaded slot = sorted_load[k*per_layer]
        const long long life = sorted_load[(size_t)k * per_layer];
        cost += (double)(life - prev) * tab[std::min(4, k + 1)];
        prev = life;
      }
    } else {
      // steps (sorted_load[k + 1], sorted_load[k]] have k + 1 live slots: the step costs what the slower of the recurrence and the
      // link needs (us; 50 GB/s = 50 000 bytes per us: what a throttled pack kernel pulls from pinned memory, h2d copies reach 57)
      for (int k = S - 1; k >= 0; --k) {
        const long long life = sorted_load[(size_t)k];
        if (life <= prev) continue;
        const double rec = tab[std::min(4, k / per_layer + 1)];
        const double link = (double)(k + 1) * host_row_bytes / 50000.0;
        cost += (double)(life - prev) * std::max(rec, link);
        prev = life;
      }
    }
    c.cost = cost;
    return c;
  };
  Cand best;
  static const int force_slots = prego_tune_env("PREGO_PLAN_SLOTS") ? atoi(prego_tune_env("PREGO_PLAN_SLOTS")) : 0;   // debug / calibration of kStepCost
  if (slots_arg > 0) {                                                    // split pass: one tile on each of its groups
    best = pack(std::min(n, slots_arg));
    // every slot is alive to the end of a split pass, so the pass takes as long as the most loaded slot: LPT leaves it a few percent above
    // frames / slots (bench workload: 50 126 vs 48 045 steps).  Local search on the LPT result: move or swap clips between the most loaded
    // slot and any other while that lowers the larger of the two loads
    const int S2 = best.S;
    for (int iter = 0; iter < 4096; ++iter) {
      int A = 0;
      for (int i = 1; i < S2; ++i) if (best.load[i] > best.load[A]) A = i;
      long long best_gain = 0; int bB = -1, ba = -1, bb = -1;
      for (int B = 0; B < S2; ++B) {
        if (B == A) continue;
        const long long la = best.load[A], lb = best.load[B];
        for (size_t ia = 0; ia < best.bins[A].size(); ++ia) {
          const long long a = lens[best.bins[A][ia]];
          if (best.bins[A].size() > 1) {                                  // move a: A -> B
            const long long gain = la - std::max(la - a, lb + a);
            if (gain > best_gain) { best_gain = gain; bB = B; ba = (int)ia; bb = -1; }
          }
          for (size_t ib = 0; ib < best.bins[B].size(); ++ib) {           // swap a <-> b
            const long long b = lens[best.bins[B][ib]];
            if (b >= a) continue;
            const long long gain = la - std::max(la - a + b, lb - b + a);
            if (gain > best_gain) { best_gain = gain; bB = B; ba = (int)ia; bb = (int)ib; }
          }
        }
      }
      if (bB < 0) break;
      const int ca = best.bins[A][ba];
      if (bb < 0) {
        best.bins[A].erase(best.bins[A].begin() + ba); best.bins[bB].push_back(ca);
        best.load[A] -= lens[ca]; best.load[bB] += lens[ca];
      } else {
        const int cb = best.bins[bB][bb];
        best.bins[A][ba] = cb; best.bins[bB][bb] = ca;
        best.load[A] += lens[cb] - lens[ca]; best.load[bB] += lens[ca] - lens[cb];
      }
    }
    long long mx = 0;
    for (int i = 0; i < S2; ++i) mx = std::max(mx, best.load[i]);
    best.cost = (double)mx * (h->x2 ? kStepCostX2 : h->bf16 ? kStepCost : kStepCostF32)[1];
  }
  else if (want_single || (n <= per_layer && host_row_bytes <= 0)) best = pack(n);
  else if (force_slots > 0) best = pack(std::min(n, std::min(force_slots, max_slots)));
  else {
    best = pack(std::min(n, per_layer));
    for (int S = 2 * per_layer; S <= max_slots && n > per_layer; S *= 2) {
      Cand c = pack(std::min(n, S));
      if (c.cost < best.cost) best = std::move(c);
      if (S >= n) break;
    }
    if (host_row_bytes > 0)                              // link-bound candidates: fewer slots than one tile layer, in steps of 8
      for (int S = 8; S < std::min(n, per_layer); S += 8) {
        Cand c = pack(S);
        if (c.cost < best.cost) best = std::move(c);
      }
  }
  const int S = best.S;
  std::vector<int> slot_order(S);
  std::iota(slot_order.begin(), slot_order.end(), 0);
  std::stable_sort(slot_order.begin(), slot_order.end(), [&](int a, int b) { return best.load[a] > best.load[b]; });
  const int smax = (int)best.load[slot_order[0]];
  h->h_seg_off.assign(S + 1, 0); h->h_seg_clip.clear(); h->h_seg_start.clear(); h->h_sorted.assign(S, 0);
  std::vector<int> cnt((size_t)smax + 1, 0);
  bool single = true;
  for (int i = 0; i < S; ++i) {
    const auto& bin = best.bins[slot_order[i]];
    int start = 0;
    for (int idx : bin) { h->h_seg_clip.push_back(idx); h->h_seg_start.push_back(start); start += lens[idx]; }
    h->h_seg_off[i + 1] = (int)h->h_seg_clip.size();
    h->h_sorted[i] = bin.empty() ? 0 : bin[0];
    single = single && bin.size() == 1;
    cnt[start]++;
  }
  h->h_nact.assign(smax, 0);
  int alive = 0;
  for (int t = smax; t >= 1; --t) { alive += cnt[t]; h->h_nact[t - 1] = alive; }
  h->h_rowoff.assign((size_t)smax + 1, 0);
  for (int t = 0; t < smax; ++t) h->h_rowoff[t + 1] = h->h_rowoff[t] + h->h_nact[t];
  {                                  // step of every 32nd packed row (the head kernel's row -> step lookup starts there)
    const int total = h->h_rowoff[smax];
    h->h_blkstep.assign((size_t)(total + 31) / 32, 0);
    int st = 0;
    for (size_t b = 0; b < h->h_blkstep.size(); ++b) {
      const int row = (int)b * 32;
      while (st + 1 < smax && h->h_rowoff[st + 1] <= row) ++st;
      h->h_blkstep[b] = st;
    }
  }
  h->plan_dirty = true;              // device copies are staged by the caller (stage_tables)
  h->t_max = smax;
  h->n_slots = S;
  h->plan_single = single;
  h->plan_want_single = want_single;
  h->plan_host_row_bytes = host_row_bytes;
  h->plan_force_slots = slots_arg;
  h->plan_cost_us = best.cost;
  h->plan_lens.assign(lens, lens + n);
  return PREGO_OK;
}

SlotPlan device_plan(const prego_miniroad* h) {
  SlotPlan p;
  p.rowoff = h->d_rowoff; p.nact = h->d_nact; p.seg_off = h->d_seg_off; p.seg_clip = h->d_seg_clip; p.seg_start = h->d_seg_start;
  p.blk_step = h->d_blkstep;
  p.s_max = h->t_max; p.n_slots = h->n_slots;
  return p;
}

// Stage the per-call pointer table (and, when the plan changed, the plan arrays) through the handle's pinned buffer.
// `tab4` = 4 * max_clips pointers.  The previous call's copies are fenced by pin_ev before the buffer is rewritten.
// The host blocks here until the PREVIOUS call's table copies have left the pinned buffer: CPU run-ahead is one call deep
// (a second forward() can be enqueued while the first runs, a third waits for the first's H2D copies, not for its kernels).
int stage_tables(prego_miniroad* h, const void* const* tab4, size_t tab_count, hipStream_t s) {
  if (h->pin_busy) { HIPCHK(hipEventSynchronize(h->pin_ev)); h->pin_busy = false; }
  const size_t smax = (size_t)h->t_max, S = (size_t)h->n_slots, n = h->h_seg_clip.size();
  const size_t nb = h->h_blkstep.size();
  if (h->plan_dirty && (smax + 1 > h->cap_t || n + 1 > h->cap_c || nb > h->cap_b)) {
    // a clip longer than the tables reserved at create (or more clips): grow once, outside the steady state
    HIPCHK(hipStreamSynchronize(s));
    if (smax + 1 > h->cap_t) {
      (void)hipFree(h->d_rowoff); (void)hipFree(h->d_nact);
      h->cap_t = smax + 1 + 4096;
      HIPCHK(hipMalloc((void**)&h->d_rowoff, h->cap_t * 4)); HIPCHK(hipMalloc((void**)&h->d_nact, h->cap_t * 4));
    }
    if (n + 1 > h->cap_c) {
      for (int** p : {&h->d_sorted, &h->d_seg_off, &h->d_seg_clip, &h->d_seg_start}) { (void)hipFree(*p); *p = nullptr; }
      h->cap_c = n + 64;
      HIPCHK(hipMalloc((void**)&h->d_sorted, h->cap_c * 4)); HIPCHK(hipMalloc((void**)&h->d_seg_off, (h->cap_c + 1) * 4));
      HIPCHK(hipMalloc((void**)&h->d_seg_clip, h->cap_c * 4)); HIPCHK(hipMalloc((void**)&h->d_seg_start, h->cap_c * 4));
    }
    if (nb > h->cap_b) {
      (void)hipFree(h->d_blkstep);
      h->cap_b = nb + 4096;
      HIPCHK(hipMalloc((void**)&h->d_blkstep, h->cap_b * 4));
    }
    (void)hipHostFree(h->pin);
    h->pin = nullptr;
    h->pin_bytes = (size_t)6 * max_clips_of(h) * sizeof(void*) + 2 * h->cap_t * 4 + 4 * (h->cap_c + 1) * 4 + h->cap_b * 4 + 1024;
    HIPCHK(hipHostMalloc((void**)&h->pin, h->pin_bytes, hipHostMallocDefault));
  }
  char* p = h->pin;
  auto put = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    std::memcpy(p, src, bytes);
    const hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
    p += (bytes + 15) / 16 * 16;
    return e;
  };
  HIPCHK(put(h->d_ptrs, tab4, tab_count * sizeof(void*)));
  if (h->plan_dirty) {
    HIPCHK(put(h->d_rowoff, h->h_rowoff.data(), (smax + 1) * 4));
    HIPCHK(put(h->d_nact, h->h_nact.data(), smax * 4));
    HIPCHK(put(h->d_sorted, h->h_sorted.data(), S * 4));
    HIPCHK(put(h->d_seg_off, h->h_seg_off.data(), (S + 1) * 4));
    HIPCHK(put(h->d_seg_clip, h->h_seg_clip.data(), n * 4));
    HIPCHK(put(h->d_seg_start, h->h_seg_start.data(), n * 4));
    HIPCHK(put(h->d_blkstep, h->h_blkstep.data(), nb * 4));
    h->plan_dirty = false;
  }
  HIPCHK(hipEventRecord(h->pin_ev, s));
  h->pin_busy = true;
  return PREGO_OK;
}

// ---- link-fed inference: features arrive over the host link WHILE the forward runs ---------------------------------------------
// The eval loop's H2D copy of a batch (57 GB/s) and its forward (bound by the longest video's recurrence) are each ~60 ms for the
// bench's 60 videos; run one after the other they are the 46 % of the PCIe floor the round-3 verdict measured.  The caller copies the
// features in the order the packed pipeline NEEDS them (piece (clip, frames [a, b)) is needed at step start_step[clip] + a) and
// records events along the way; the pack of each chunk waits for the events that cover its steps.  plan_starts reports the schedule
// (costed for a link-bound feed: fewer slots than clips, so that rows are needed at the rate the link delivers them).
extern "C" int prego_miniroad_plan_starts(prego_miniroad* h, int n_clips, const int32_t* lens, int link_row_bytes, int32_t* start_step,
                                          int32_t* n_steps) {
  HandleScope scope_(h);
  if (!h || !lens || !start_step || n_clips <= 0) return prego_fail_(PREGO_EINVAL, "plan_starts: bad arguments");
  if (n_clips > max_clips_of(h)) return prego_fail_(PREGO_EINVAL, "%d clips > max_clips %d per call", n_clips, max_clips_of(h));
  const int rc = build_plan(h, n_clips, lens, false, link_row_bytes > 0 ? link_row_bytes : 0);
  if (rc) return rc;
  for (size_t k = 0; k < h->h_seg_clip.size(); ++k) start_step[h->h_seg_clip[k]] = h->h_seg_start[k];
  if (n_steps) *n_steps = h->t_max;
  return PREGO_OK;
}

extern "C" int prego_miniroad_set_feed_events(prego_miniroad* h, int n_events, const int32_t* upto_step, void* const* events,
                                              int link_row_bytes) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  h->feed_ev.clear(); h->feed_upto.clear(); h->feed_pos = 0; h->feed_row_bytes = 0;
  if (n_events == 0) return PREGO_OK;
  if (n_events < 0 || !upto_step || !events || link_row_bytes <= 0) return prego_fail_(PREGO_EINVAL, "set_feed_events: bad arguments");
  for (int j = 0; j < n_events; ++j) {
    if (!events[j] || (j > 0 && upto_step[j] < upto_step[j - 1])) { h->feed_ev.clear(); h->feed_upto.clear(); return prego_fail_(PREGO_EINVAL, "set_feed_events: event %d", j); }
    h->feed_ev.push_back((hipEvent_t)events[j]);
    h->feed_upto.push_back(upto_step[j]);
  }
  h->feed_row_bytes = link_row_bytes;
  return PREGO_OK;
}

// bf16 mode, inference (no PREGO_FWD_KEEP): the two projections' outputs stay bf16 between the kernels (what a bf16 autocast
// of the reference does too).  They are the largest HBM streams of the pass (20 KB per frame in fp32) and the store tail of a
// GEMM tile is bound by bytes: with fp32 C the projections run 1.23 / 1.10 PFLOP/s (K = 4096 / 2048), without any C store 1.41 /
// 1.40; the numpy emulation of the whole path moves the worst probability error from 2.0e-3 to 2.5e-3 (tolerance 1e-2).
// Training keeps them fp32 (LayerNorm backward reads Y).  PREGO_FP32_INTERMEDIATES=1 restores fp32 for A/B.
bool inter16(const prego_miniroad* h, int flags) {
  static const bool force32 = prego_tune_env("PREGO_FP32_INTERMEDIATES") != nullptr;
  return h->bf16 && !(flags & PREGO_FWD_KEEP) && !force32;
}
RowBytes row_bytes(const prego_miniroad* h, bool with_flow, int flags) {
  const size_t es = h->bf16 ? 2 : 4;
  const size_t is = inter16(h, flags) ? 2 : 4;
  RowBytes r;
  r.x = (size_t)(h->d_rgb + (with_flow ? h->d_flow : 0)) * es;
  r.y = (size_t)h->emb * is;
  r.e = (size_t)h->emb * es;
  r.gi = (size_t)3 * h->hid * is;
  r.hr = (size_t)h->hid * es;
  const bool keep = (flags & PREGO_FWD_KEEP) != 0;
  r.hraw = keep ? (size_t)h->hid * 4 : 0;
  r.gates = keep ? (size_t)h->hid * 4 * 4 : 0;      // r, z, n, W_hn h + b_hn
  r.stats = keep ? 8 : 0;                           // LayerNorm mean, rstd
  r.map = 16;                                       // row -> (clip, frame) for the head's scatter, two chunks deep
  // training a two-layer GRU (round 6): layer 0's h_t as layer 1's input operand, layer 1's raw state and its four gate activations
  r.l2keep = (keep && h->layers == 2) ? (size_t)h->hid * es + (size_t)h->hid * 4 + (size_t)h->hid * 4 * 4 : 0;
  r.total = r.x + r.y + r.e + r.gi + r.hr + r.hraw + r.gates + r.stats + r.map + r.l2keep;
  return r;
}

// Every carve of the forward workspace is rounded up to 256 bytes and the row capacity down to a multiple of 128 (the GEMM kernels' row
// tile): the slack pays for the former.
static constexpr size_t kFwdSlackBytes = 12 * 256;
static constexpr long long kFwdRowQuantum = 128;
long long fwd_rows_fit(const RowBytes& rb, size_t workspace_bytes) { return (long long)((workspace_bytes - kFwdSlackBytes) / rb.total); }
size_t fwd_bytes_for_rows(const RowBytes& rb, long long rows) {
  return align_up((size_t)rows, (size_t)kFwdRowQuantum) * rb.total + kFwdSlackBytes;
}
FwdLayout fwd_layout(const prego_miniroad* h, bool with_flow, int flags, size_t workspace_bytes) {
  FwdLayout L{};
  const RowBytes rb = L.rb = row_bytes(h, with_flow, flags);
  const size_t rows = (size_t)(L.cap_rows = fwd_rows_fit(rb, workspace_bytes) / kFwdRowQuantum * kFwdRowQuantum);
  size_t off = 0;
  auto put = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
  L.X = put(rows * rb.x); L.Y = put(rows * rb.y); L.E = put(rows * rb.e); L.GI = put(rows * rb.gi); L.HR = put(rows * rb.hr);
  const size_t gate = rows * h->hid * 4;                  // one fp32 [rows][H] buffer: a raw state or one of the four gate activations
  if (rb.hraw) {                                          // PREGO_FWD_KEEP
    L.HRAW = put(rows * rb.hraw);
    L.KR = put(gate); L.KZ = put(gate); L.KN = put(gate); L.KG = put(gate);
    L.STATS = put(rows * rb.stats);
  }
  // two-layer training: layer 0's h_t [rows][H] (operand type: layer 1's input, and the B operand of dW_ih_l1), layer 1's raw state and gates
  if (rb.l2keep) {
    L.HR0 = put(rows * h->hid * (h->bf16 ? 2 : 4));
    L.HRAW2 = put(gate);
    L.KR2 = put(gate); L.KZ2 = put(gate); L.KN2 = put(gate); L.KG2 = put(gate);
  }
  L.RM = put(rows * rb.map);       // [2][cap_rows] int2: chunk c uses half c & 1 (the pack of chunk c+1 runs under the recurrence of
                                   // chunk c, before the head of chunk c).  Behind the kept buffers; the backward does not read it
  L.total = off;
  return L;
}

extern "C" size_t prego_miniroad_workspace_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens,
                                                 int64_t rows_per_chunk, int flags) {
  if (!h || n_clips <= 0) return 0;
  long long total = 0;
  if (lens) for (int i = 0; i < n_clips; ++i) total += lens[i];
  long long rows = std::max<long long>(rows_per_chunk, n_clips);
  if (lens && rows > total) rows = std::max<long long>(total, n_clips);
  if (flags & PREGO_FWD_KEEP) rows = std::max<long long>(rows, total);
  return fwd_bytes_for_rows(row_bytes(h, true, flags), rows);
}
