// MiniROAD host side: the split pass - ring and resident-buffer sizing, and the pass itself.
#include "miniroad_handle.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <thread>

// ---- split pass ----------------------------------------------------------------------------------------------------------------
// Geometry: units of 256 packed rows; chunks of 8 units (2 048 rows) are what the two kernels tell each other about; X / Y / E rings
// of 24 units (twelve super-rounds of two) per feed-forward XCD, a GI ring of 32 units = 4 chunks.  The rings come out of the caller's
// workspace (0.54 GB: they fit the default one), relu(h) + the row map of the whole pass and the counters live in the caller's resident
// buffer (the head runs once, behind the pass).
// (debug library: PREGO_SPLIT_GI_RING = a power of two of units, at least four chunks; PREGO_SPLIT_RING_PER_XCD = an even number of units
// beyond the largest lag - sweeps of how much of the rings the 256 MB Infinity Cache can hold)
static int tuned_pow2(const char* name, int dflt) {
  const char* v = prego_tune_env(name);
  const int x = v ? atoi(v) : 0;
  return (x >= 16 && (x & (x - 1)) == 0) ? x : dflt;
}
// Round 6: a GI ring of 32 units (50 MB; 4 chunks of 8 units) instead of 256 (0.4 GB; 4 chunks of 64): same-device 91.7-92.0 against
// 93.1 ms and 93.4 against 95.1-95.2 (profiles/r06_split_rings*.log).  The feed-forward launch may run 8 192 rows (~170 recurrence steps)
// ahead instead of 65 536: what it has written and the recurrence has not yet read stays in the Infinity Cache, and so does more of its own
// X -> Y -> E chain.  64 units: -0.5...-0.8 %; 32 units in chunks of 4: -1.0 %; 16 units or two chunks of 16: the launches wait for each
// other (+0.4...+11 %).  The X / Y / E ring's size does not matter (16 / 24 / 32 units per XCD: +-0.1 %).
// The rgb-only pass on 4 + 4 XCDs is bound by its feed-forward launch, not by the recurrence, and keeps the long ring (28.1-28.2 against
// 27.8-28.0 M frames/s, profiles/r06_split_rings_zf.log).
static int split_gi_ring_units(int R) { return tuned_pow2("PREGO_SPLIT_GI_RING", R <= 3 ? 32 : 256); }
static const int kSplitRingPerXcd = (prego_tune_env("PREGO_SPLIT_RING_PER_XCD") && atoi(prego_tune_env("PREGO_SPLIT_RING_PER_XCD")) >= 12 &&
                                     atoi(prego_tune_env("PREGO_SPLIT_RING_PER_XCD")) % 4 == 0) ? atoi(prego_tune_env("PREGO_SPLIT_RING_PER_XCD")) : 24;   // ring: 12 super-rounds of 2 units
// units per super-round (debug library: sweep).  Round 6: 2 instead of 4.  ALONE the feed-forward launch is flat between 2 and 4 (93.0 / 92.3 ms,
// round 5); IN THE PASS 2 is 1.0-1.2 % faster on every box and alternation (profiles/r06_split_knobs.log: 95.6-97.7 against 96.8-98.6 ms):
// half the look-ahead in rows (lags 2 / 3 / 4 super-rounds = 4 / 6 / 8 units) keeps a unit's X -> Y -> E -> GI chain closer together in
// the XCD's L2, and a weight slab is still shared by two row blocks.  1 (no sharing) runs the GEMM tiles at 0.75 of the rate: 127 ms.
static const int kSplitSg = (prego_tune_env("PREGO_SPLIT_SG") && kSplitRingPerXcd % std::max(1, atoi(prego_tune_env("PREGO_SPLIT_SG"))) == 0)
                                ? std::max(1, atoi(prego_tune_env("PREGO_SPLIT_SG"))) : 2;
static int split_chunk_shift(int R) { return prego_tune_env("PREGO_SPLIT_CHUNK_SHIFT") ? atoi(prego_tune_env("PREGO_SPLIT_CHUNK_SHIFT")) : (R <= 3 ? 3 : 6); }
SplitRings split_rings(const prego_miniroad* h, int R) {
  SplitRings g;
  g.ring_units = kSplitRingPerXcd * (8 - R);
  g.x = align_up((size_t)g.ring_units * 256 * (size_t)(h->d_rgb + h->d_flow) * 2, 256);
  g.y = align_up((size_t)g.ring_units * 256 * (size_t)h->emb * 2, 256);
  g.e = g.y;
  g.gi = align_up((size_t)split_gi_ring_units(R) * 256 * (size_t)3 * h->hid * 2, 256);
  g.total = g.x + g.y + g.e + g.gi;
  return g;
}
bool split_workspace_ok(const prego_miniroad* h, int R, size_t workspace_bytes) { return workspace_bytes >= split_rings(h, R).total; }

// whole-call buffer of a split pass: relu(h) rows | row map | counters.  It lives in the caller's resident buffer
// (prego_miniroad_resident_bytes / _set_resident); a buffer that is too small keeps the call on the chunked pass
size_t split_buf_need(const prego_miniroad* h, long long total) {
  const long long n_units = (total + 255) / 256;
  const int shift = split_chunk_shift(1);                       // the smallest chunk any R uses: the most counters
  const long long n_chunks = (n_units + (1 << shift) - 1) >> shift;
  return align_up((size_t)total * h->hid * 2, 256) + align_up((size_t)total * 8, 256) + align_up(((size_t)4 * n_units + 2 * (size_t)n_chunks + 32) * 4, 256);
}
bool split_resident_ok(const prego_miniroad* h, long long total) { return h->res_buf && split_buf_need(h, total) <= h->res_bytes; }

// Whole-call resident buffer (round 6; SURVEY 8b: "no allocation of caller-visible memory, workspace sized by a query and passed in").
// A pass that runs the classifier once per call keeps relu(h) of every packed row (2 KB per frame with 16-bit operands, 4 KB with fp32 /
// fp16x2), the split pass also its row map and counters.  Until round 5 forward() grew a handle-owned hipMalloc for it (behind a stream
// synchronisation); now the caller sizes it here and hands it over with prego_miniroad_set_resident.
extern "C" size_t prego_miniroad_resident_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens, int flags) {
  if (!h || n_clips <= 0 || !lens) return 0;
  if ((flags & PREGO_FWD_KEEP) || h->layers != 1) return 0;
  long long total = 0;
  for (int i = 0; i < n_clips; ++i) total += lens[i] > 0 ? lens[i] : 0;
  if (total < 65536) return 0;                      // fewer than four chunks of the smallest useful size: the per-chunk head runs
  const RowBytes rb = row_bytes(h, true, flags);
  size_t need = align_up((size_t)total * rb.hr, 256);
  if (h->bf16 && h->hid == 1024) need = std::max(need, split_buf_need(h, total));
  return need <= ((size_t)24 << 30) + ((size_t)1 << 30) ? need : 0;
}

// Split passes of DIFFERENT handles on one device must not interleave: handle A's feed-forward launch resident on XCDs R .. 7 with handle
// B's recurrence launch resident on XCDs 0 .. R - 1 wait for each other's partner, which can never be dispatched (bounded, but both calls
// are lost).  Every split pass therefore starts behind the end of the previous one on the device, whatever handle / stream it came from.
static std::mutex g_split_mu;
static hipEvent_t g_split_last[64] = {};

int forward_split(prego_miniroad* h, const AntOut& ao, int R, int flags, bool with_flow, bool in16, int kx, const SlotPlan& plan,
                  const FwdTables& tb, void* workspace, size_t workspace_bytes, hipStream_t s, bool* fell_back) {
  *fell_back = false;
  const int H = h->hid, E = h->emb, din = h->d_rgb + h->d_flow;
  const int total = h->h_rowoff[h->t_max];
  const int n_units = (total + 255) / 256;
  const int chunk_shift = split_chunk_shift(R), gi_ring = split_gi_ring_units(R);
  const int upc = 1 << chunk_shift;
  const int n_chunks = (n_units + upc - 1) >> chunk_shift;
  const SplitRings rg = split_rings(h, R);
  if (workspace_bytes < rg.total) return prego_fail_(PREGO_EWORKSPACE, "split pass: workspace %zu B < %zu B of rings", workspace_bytes, rg.total);
  char* wp = (char*)workspace;
  unsigned short* X = (unsigned short*)wp; wp += rg.x;
  unsigned short* Y = (unsigned short*)wp; wp += rg.y;
  unsigned short* Eb = (unsigned short*)wp; wp += rg.e;
  unsigned short* GI = (unsigned short*)wp;
  // handle-owned: relu(h) of every packed row, the row map, the counters
  const size_t hr_bytes = align_up((size_t)total * H * 2, 256), rm_bytes = align_up((size_t)total * 8, 256);
  const size_t n_ctr = (size_t)4 * n_units + 2 * (size_t)n_chunks + 32;
  if (!h->chooser.split_warm) { h->chooser.meas_armed = false; h->chooser.split_warm = true; }       // a handle's first split pass loads kernels: not a measurement
  if (!split_resident_ok(h, total)) return prego_fail_(PREGO_EWORKSPACE, "split pass: resident buffer %zu B < %zu B", h->res_bytes, split_buf_need(h, total));
  char* HR = h->res_buf;
  char* RM = HR + hr_bytes;
  unsigned* ctr = (unsigned*)(RM + rm_bytes);
  unsigned* tick = ctr; unsigned* hs_word = ctr + 8; unsigned* ff_here = ctr + 16; unsigned* pack_done = ctr + 32; unsigned* l1_cnt = pack_done + n_units; unsigned* ln_done = l1_cnt + n_units;
  unsigned* wih_cnt = ln_done + n_units; unsigned* gi_cnt = wih_cnt + n_units; unsigned* rec_cnt = gi_cnt + n_chunks;
  HIPCHK(hipMemsetAsync(ctr, 0, n_ctr * 4, s));
  HIPCHK(hipMemsetAsync(h->h_state, 0, (size_t)h->n_slots * H * 4, s));
  // start handshake (kernels.h: PassHandshake).  Bounds: the two launches are released by the same fork point and start microseconds
  // apart; 50 / 100 ms leave room for another stream's kernels draining from the CUs first.  A pass that cannot run side by side costs
  // that long ONCE (the back-off in prego_miniroad_forward keeps the handle chunked afterwards)
  PassHandshake hs{};
  h->hs_seq = (h->hs_seq + 1u) & 0x3FFFFFFFu;
  if (h->hs_seq == 0u) h->hs_seq = 1u;
  hs.word = hs_word; hs.ff_here = ff_here; hs.host = h->pin_hs; hs.seq = h->hs_seq; hs.ticks_lead = 5000000u; hs.ticks_all = 10000000u;
  int fault = 0;
#ifdef PREGO_DEBUG_ABI
  fault = h->dbg_fault; h->dbg_fault = 0;           // prego_debug_split_fault: one shot
  if (fault == 3 || fault == 4) {
    // replay of ONE of the two launches alone (counter collection serialises dispatches, so the pair cannot run under it): the handshake
    // is pre-decided and the other side's counters pre-armed - the feed-forward launch never waits for a GI ring slot, the recurrence
    // launch reads whatever finite rows an earlier pass left in the ring.  Same instruction stream and memory traffic, meaningless outputs
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)hs_word, PREGO_HS_GO, 1, s));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ff_here, 1, 8, s));
    if (fault == 3) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)rec_cnt, R * h->P * 4, n_chunks, s));
    else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)gi_cnt, upc, n_chunks, s));
    hs.host = nullptr;
  }
#endif

  FfPassArgs fa{};
  fa.rgb_ptrs = tb.rgb; fa.flow_ptrs = with_flow ? tb.flow : nullptr; fa.plan = plan; fa.rowmap = RM;
  fa.d_rgb = h->d_rgb; fa.d_flow = with_flow ? h->d_flow : 0; fa.in16 = in16 ? 1 : 0; fa.kx = kx;
  fa.w1 = (const unsigned short*)h->w1; fa.ld_w1 = din; fa.b1 = h->b1; fa.ln_g = h->ln_g; fa.ln_b = h->ln_b; fa.ln_eps = 1e-5f;
  fa.w_ih = (const unsigned short*)h->w_ih_perm; fa.bias2 = h->bias2_perm; fa.E = E; fa.n3 = 3 * H;      // permuted rows: GI rows in (unit pair, gate) order
  fa.X = X; fa.Y = Y; fa.Eb = Eb; fa.GI = GI; fa.ring_units = rg.ring_units; fa.gi_ring_units = gi_ring;
  fa.total_rows = total; fa.n_units = n_units; fa.xcd_lo = R; fa.chunk_unit_shift = chunk_shift;
  fa.rec_expect = R * h->P * 4; fa.nt1 = E / 256; fa.nt2 = 3 * H / 256;
  static const int lag1 = prego_tune_env("PREGO_SPLIT_LAG1") ? atoi(prego_tune_env("PREGO_SPLIT_LAG1")) : 2;
  static const int lag2 = prego_tune_env("PREGO_SPLIT_LAG2") ? atoi(prego_tune_env("PREGO_SPLIT_LAG2")) : 3;
  static const int lag3 = prego_tune_env("PREGO_SPLIT_LAG3") ? atoi(prego_tune_env("PREGO_SPLIT_LAG3")) : 4;
  static const bool want_stats = prego_tune_env("PREGO_SPLIT_STATS") != nullptr;
  fa.sg = kSplitSg; fa.lag1 = lag1; fa.lag2 = lag2; fa.lag3 = lag3; fa.f16 = h->f16 ? 1 : 0;
  static const int ff_cus = prego_tune_env("PREGO_SPLIT_FF_CUS") ? atoi(prego_tune_env("PREGO_SPLIT_FF_CUS")) : 0;        // debug library only
  fa.max_wg = ff_cus;
  fa.stats = want_stats ? h->stamps : nullptr;
#ifdef PREGO_DEBUG_ABI
  static const int dbg = prego_tune_env("PREGO_SPLIT_DBG") ? atoi(prego_tune_env("PREGO_SPLIT_DBG")) : 0;     // timing experiments (wrong results): debug library only
  fa.dbg = dbg;
#endif
  fa.tick = tick; fa.pack_done = pack_done; fa.l1_cnt = l1_cnt; fa.ln_done = ln_done; fa.wih_cnt = wih_cnt; fa.gi_cnt = gi_cnt;
  fa.rec_cnt = rec_cnt; fa.abort_word = h->abort_word; fa.hs = hs;
  // a job may only ever wait for jobs with earlier tickets: the previous holder of a ring slot (ring / sg super-rounds back) must have been
  // issued before the job that overwrites the slot
  const int ring_sr = kSplitRingPerXcd / kSplitSg;
  if (lag1 < 1 || lag2 <= lag1 || lag3 <= lag2 || lag1 >= ring_sr || lag2 - ring_sr >= lag1 || lag3 - ring_sr >= lag2)
    return prego_fail_(PREGO_EINVAL, "split pass: lags %d %d %d", lag1, lag2, lag3);

  GruArgs ga{};
  ga.whh = h->w_hh; ga.b_hn = h->b_hn; ga.gi = GI; ga.gi_bf16 = 1; ga.f16 = h->f16 ? 1 : 0; ga.h_relu_out = HR; ga.h_raw_out = nullptr;
  ga.h_state = h->h_state; ga.hx = h->hx; ga.flags = h->flags; ga.abort_word = h->abort_word;
  ga.rowoff = h->d_rowoff; ga.nact = h->d_nact; ga.t0 = 0; ga.t1 = h->t_max; ga.row_base = 0; ga.rows = 0;
  ga.n_clips = h->n_slots; ga.G = h->G; ga.seg_off = h->plan_single ? nullptr : h->d_seg_off;
  ga.seg_start = h->plan_single ? nullptr : h->d_seg_start; ga.stamps = (h->use_stamps && !want_stats) ? h->stamps : nullptr;
  ga.sync = h->flags; ga.armed = 0; ga.Gd = R;
  ga.gi_cnt = gi_cnt; ga.rec_cnt = rec_cnt; ga.chunk_shift = chunk_shift + 8; ga.n_chunks = n_chunks;
  ga.units_per_chunk = upc; ga.units_last = n_units - upc * (n_chunks - 1); ga.gi_row_mask = (unsigned)gi_ring * 256u - 1u;
  ga.hs = hs;

  // the feed-forward launch goes to the side stream (another hardware queue: it must be resident TOGETHER with the recurrence), forked
  // from and joined to the caller's stream by events
  struct SideJoin {
    prego_miniroad* h; bool pending = false;
    ~SideJoin() { if (pending) (void)hipStreamSynchronize(h->side); }
  } side_join{h};
  // everything the recurrence launch needs done first goes IN FRONT of the fork: once the feed-forward kernel is resident it fills its CUs
  // completely, and an ordinary kernel of the caller's stream (the arm kernel, a memset) would wait for it - with the recurrence queued behind
  launch_gru_arm(gru_arm_desc(true, H, h->G, h->hx, h->flags), s);
  if (h->perm_stale) {                       // in front of the fork, like the arm kernel: nothing of this stream may sit between the two launches
    launch_permute_gi_rows(h->w_ih, h->bias2, h->w_ih_perm, h->bias2_perm, H, E, s);
    h->perm_stale = false;
  }
  std::lock_guard<std::mutex> split_lock(g_split_mu);          // held until this pass is enqueued and its end event recorded
  int dev_ = 0;
  HIPCHK(hipGetDevice(&dev_));
  const bool dev_ok = dev_ >= 0 && dev_ < 64;
  if (dev_ok && g_split_last[dev_]) HIPCHK(hipStreamWaitEvent(s, g_split_last[dev_], 0));
  HIPCHK(hipEventRecord(h->ev_fork, s));
  HIPCHK(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  const bool run_ff = fault != 2 && fault != 4, run_rec = fault != 1 && fault != 3;
  const size_t ev_mark = h->ev_used;
  EventPair* evf = run_ff ? ev_begin(h, 2, h->side) : nullptr;       // timing_read: the feed-forward launch of a split pass is reported in the pack slot
  if (run_ff && launch_ff_pass(fa, h->side)) return prego_fail_(PREGO_EINVAL, "split pass: feed-forward shape E=%d kx=%d", E, kx);
  ev_end(evf, h->side);
  side_join.pending = true;
  HIPCHK(hipEventRecord(h->ev_join, h->side));
  EventPair* evr = run_rec ? ev_begin(h, 1, s) : nullptr;
  if (run_rec && launch_gru_recurrence_pass(H, ga, s)) return prego_fail_(PREGO_EINVAL, "split pass: recurrence launch");
  ev_end(evr, s);
  HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
  side_join.pending = false;
  if (dev_ok) {
    if (!g_split_last[dev_]) HIPCHK(hipEventCreateWithFlags(&g_split_last[dev_], hipEventDisableTiming));
    HIPCHK(hipEventRecord(g_split_last[dev_], s));
  }
  if (fault == 3 || fault == 4) { HIPCHK(hipGetLastError()); return PREGO_OK; }      // replay of one launch: no head, outputs untouched
  // The calling thread waits here until the two launches have met (normally: the moment the stream reaches them).  GO: both are resident,
  // every wait of the pass has a running producer, the head is enqueued behind it.  FAIL: they have left without writing anything
  {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    unsigned state = 0u; long long polls = 0;
    for (;;) {
      const unsigned v = __atomic_load_n(h->pin_hs, __ATOMIC_ACQUIRE);
      if ((v >> 2) == hs.seq && (v & 3u)) { state = v & 3u; break; }
      if ((++polls & 63) == 0) {
        // both launches gone and nobody decided (cannot happen: every workgroup of either launch votes within its bound): not a pass
        if (hipStreamQuery(s) == hipSuccess) {
          const unsigned v2 = __atomic_load_n(h->pin_hs, __ATOMIC_ACQUIRE);
          state = ((v2 >> 2) == hs.seq && (v2 & 3u)) ? (v2 & 3u) : PREGO_HS_FAIL;
          break;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(300))
          return prego_fail_(PREGO_ETIMEOUT, "split pass: the stream did not reach the pass within 300 s");
      }
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if (state != PREGO_HS_GO) {
      h->ev_used = ev_mark;                    // the two launches' timing events do not describe a pass
      h->chooser.meas_armed = false;
      *fell_back = true;
      HIPCHK(hipGetLastError());
      return PREGO_OK;
    }
  }
  if (h->timing) { h->gemm_flop += 2.0 * total * ((double)E * kx + 3.0 * H * E); h->split_passes++; h->split_steps += h->t_max; }
  if ((tb.out || tb.arg) &&
      launch_head_softmax(true, HR, h->w_c, h->b_c, plan, 0, total, H, h->ncls, (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, tb.out, tb.arg, s,
                          RM, h->f16))
    return prego_fail_(PREGO_EINVAL, "head: unsupported num_classes %d", h->ncls);
  if (int rc_a = ant_head(h, ao, HR, plan, 0, total, flags, s)) return rc_a;
  if (h->chooser.meas_armed) { HIPCHK(hipEventRecord(h->chooser.ev_meas[1], s)); h->chooser.meas_pending = true; h->chooser.meas_armed = false; }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
// fault injection / replay for the NEXT split pass of the handle (one shot; include/prego_amd_debug.h)
extern "C" int prego_debug_split_fault(prego_miniroad* h, int mode) {
  if (!h || mode < 0 || mode > 4) return prego_fail_(PREGO_EINVAL, "debug split fault: mode %d", mode);
  h->dbg_fault = mode;
  return PREGO_OK;
}
#endif
