// Host side of the multi-frame streaming steps (include/prego_amd.h: prego_miniroad_step_frames / _anticipation, the same K for every
// stream, and prego_miniroad_step_ragged / _anticipation, a host array of frame counts; kernels: stream_frames.hip and the wide step's
// launchers, stream_wide.hip).  One call advances n streams by their frames: the products that do not depend on time run once over all
// rows, the recurrence takes one fused launch per frame index, the heads follow over all rows.  Every refusal is decided before the first
// launch.
#include "miniroad_handle.h"

namespace {
constexpr int kMaxFrames = 32, kMaxRows = 256;

// the caller's workspace, every part 256-byte aligned (R rows; step_frames: R = n K, row s K + t = frame t of stream s; step_ragged: stream
// s owns rows off[s] .. off[s] + n_frames[s])):
//   xb [R][d_rgb + d_flow] 16-bit | h0 [n][H] f32 | y [R][emb] f32 | e [R][emb] 16-bit | gi [R][3H] f32 | hist [R][H] f32 | hr [R][H] 16-bit
//   | A [R][L H] 16-bit (after set_anticipation)
struct FramesLayout { size_t xb, h0, y, e, gi, hist, hr, a, total; };
FramesLayout frames_layout(const prego_miniroad* h, int n, int rows) {
  const size_t E = (size_t)h->emb, H = (size_t)h->hid, din = (size_t)(h->d_rgb + h->d_flow), R = (size_t)rows;
  FramesLayout w{};
  WsCarver c;
  w.xb = c.take(R * din * 2); w.h0 = c.take((size_t)n * H * 4); w.y = c.take(R * E * 4); w.e = c.take(R * E * 2);
  w.gi = c.take(R * 3 * H * 4); w.hist = c.take(R * H * 4); w.hr = c.take(R * H * 2);
  w.a = c.take(h->ant_len > 0 ? R * h->ant_len * H * 2 : 0);          // after set_anticipation: either entry point fits
  w.total = c.o;
  return w;
}

bool frames_shape_ok(int n, int K) { return n >= 1 && K >= 1 && K <= kMaxFrames && (long long)n * K <= kMaxRows; }
bool ragged_shape_ok(int n, int rows) { return n >= 1 && n <= kRaggedMaxStreams && rows >= n && rows <= kMaxRows; }

// the launches of a burst over R packed rows, refusals done: everything that does not depend on time once over the rows, recur(t) for
// t = 0 .. n_launches - 1, the heads over all rows.  who: the entry point's short name
template <typename Recur>
int frames_chain(const char* who, prego_miniroad* h, int n, int R, int n_launches, const float* rgb, const float* flow, float* h_state, float* out,
                 int32_t* argmax, bool ant, float* ant_out, int32_t* ant_argmax, int flags, char* ws, const FramesLayout& w, hipStream_t s,
                 Recur&& recur) {
  const int E = h->emb, H = h->hid, din = h->d_rgb + h->d_flow, sm = (flags & PREGO_FWD_SOFTMAX) ? 1 : 0;
  float* Y = (float*)(ws + w.y);
  float* GI = (float*)(ws + w.gi);
  float* H0 = (float*)(ws + w.h0);
  float* HIST = (float*)(ws + w.hist);
  // everything that does not depend on time, once over the R rows: the wide step's launches with R in the place of n
  if (launch_frames_cast(h->d_rgb > 0 ? rgb : nullptr, h->d_flow > 0 ? flow : nullptr, h_state, ws + w.xb, H0, R, n, h->d_rgb, h->d_flow, H, s,
                         h->f16)) return prego_fail_(PREGO_EINVAL, "%s: unsupported feature widths %d + %d", who, h->d_rgb, h->d_flow);
  StreamGemv l1{h->w1, ws + w.xb, nullptr, h->b1, Y, E, din, din, din, 0, 1};
  if (launch_wide_gemv(1, &l1, R, s, h->f16)) return prego_fail_(PREGO_EINVAL, "%s: unsupported layer1 shape %d x %d", who, E, din);
  launch_ln_relu(true, Y, h->ln_g, h->ln_b, R, E, 1e-5f, ws + w.e, nullptr, 0.f, 0ull, 0, s, 1, false, h->f16);
  StreamGemv gi{h->w_ih, ws + w.e, nullptr, h->bias2, GI, 3 * H, E, E, E, 0, 1};
  if (launch_wide_gemv(1, &gi, R, s, h->f16)) return prego_fail_(PREGO_EINVAL, "%s: unsupported GRU shape %d / %d", who, E, H);
  // the sequential part: one fused launch per frame, ordered by the stream alone
  for (int t = 0; t < n_launches; ++t)
    if (recur(t, GI, H0, HIST, ws + w.hr)) return prego_fail_(PREGO_EINVAL, "%s: unsupported GRU shape %d / %d", who, E, H);
  // the classifier over the relu(h) rows: the row-list head with one row per frame (wide_ant_head, L = 1)
  if ((out || argmax) && launch_wide_ant_head(ws + w.hr, h->w_c, h->b_c, R, H, 1, h->ncls, sm, out, (int*)argmax, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "%s: unsupported head shape %d x %d", who, h->ncls, H);
  if (ant && (ant_out || ant_argmax)) {
    if (launch_wide_ant_hidden(h->w_a, h->b_a, HIST, ws + w.a, R, H, h->ant_len, s, h->f16) ||
        launch_wide_ant_head(ws + w.a, h->w_c, h->b_c, R, H, h->ant_len, h->ncls, sm, ant_out, (int*)ant_argmax, s, h->f16))
      return prego_fail_(PREGO_EINVAL, "%s_anticipation: unsupported head shape %d x %d x %d", who, h->ant_len, h->ncls, H);
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

int step_frames_impl(prego_miniroad* h, int n, int K, const float* rgb, const float* flow, float* h_state, float* out, int32_t* argmax,
                     bool ant, float* ant_out, int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                     prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (K < 1 || K > kMaxFrames) return prego_fail_(PREGO_EINVAL, "step_frames: %d frames per stream (1..%d per call)", K, kMaxFrames);
  if (n >= 1 && (long long)n * K > kMaxRows)
    return prego_fail_(PREGO_EINVAL, "step_frames: %d streams x %d frames = %lld rows (at most %d per call: use forward() with h0 / h_last)", n, K,
                       (long long)n * K, kMaxRows);
  if (int rc = step_refusals(h, n, kMaxRows, rgb, flow, h_state, ant)) return rc;
  const FramesLayout w = frames_layout(h, n, n * K);
  if (int rc = workspace_refusal("step_frames", "prego_miniroad_step_frames_workspace_bytes", workspace, workspace_bytes, w.total,
                                 "%d streams x %d frames", n, K)) return rc;
  hipStream_t s = (hipStream_t)stream;
  return frames_chain("step_frames", h, n, n * K, K, rgb, flow, h_state, out, argmax, ant, ant_out, ant_argmax, flags, (char*)workspace, w, s,
                      [&](int t, const float* GI, const float* H0, float* HIST, void* HR) {
                        return launch_frames_recur(h->w_hh, GI, h->b_hn, H0, HIST, HR, t == K - 1 ? h_state : nullptr, n, K, t, h->hid, s, h->f16);
                      });
}

int step_ragged_impl(prego_miniroad* h, int n, const int32_t* n_frames, const float* rgb, const float* flow, float* h_state, float* out,
                     int32_t* argmax, bool ant, float* ant_out, int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                     prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  RaggedPlan plan;
  if (int rc = ragged_plan("step_ragged", n, n_frames, &plan)) return rc;
  if (int rc = step_refusals(h, n, kMaxRows, rgb, flow, h_state, ant)) return rc;      // n outside 1..256 among them
  const FramesLayout w = frames_layout(h, n, plan.rows);
  if (int rc = workspace_refusal("step_ragged", "prego_miniroad_step_ragged_workspace_bytes", workspace, workspace_bytes, w.total,
                                 "%d streams with %d frames in all", n, plan.rows)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // launch t advances the plan.alive[t] streams that have a frame t: a prefix of the walk order; from here on n_frames is not read again
  return frames_chain("step_ragged", h, n, plan.rows, plan.kmax, rgb, flow, h_state, out, argmax, ant, ant_out, ant_argmax, flags,
                      (char*)workspace, w, s, [&](int t, const float* GI, const float* H0, float* HIST, void* HR) {
                        return launch_frames_recur_ragged(h->w_hh, GI, h->b_hn, H0, HIST, HR, h_state, plan.walk, n, plan.rows, plan.alive[t], t,
                                                          plan.kmax == 1, h->hid, s, h->f16);
                      });
}
}  // namespace

// the plan of a ragged call from the caller's host array (read here and nowhere after): the prefix-sum rows in the caller's order, the
// walk order - a stable counting sort by descending count - and how many streams are alive in every launch.  Refuses (PREGO_EINVAL, under
// the caller's HandleScope) a NULL array, a count outside 1..32 and more than 256 rows; n outside 1..256 is left to the caller's own
// refusal (the plan is then empty and must not be used)
int ragged_plan(const char* who, int n, const int32_t* n_frames, RaggedPlan* p) {
  p->rows = 0; p->kmax = 0;
  for (int t = 0; t < kMaxFrames; ++t) p->alive[t] = 0;
  if (!n_frames) return prego_fail_(PREGO_EINVAL, "%s: n_frames is NULL", who);
  if (n < 1 || n > kRaggedMaxStreams) return 0;
  long long R = 0;
  int first[kMaxFrames + 1] = {0};                              // first[k]: streams with exactly k frames, then where they start in the walk
  for (int i = 0; i < n; ++i) {
    const int k = n_frames[i];
    if (k < 1 || k > kMaxFrames) return prego_fail_(PREGO_EINVAL, "%s: n_frames[%d] = %d frames (1..%d per stream and call)", who, i, k, kMaxFrames);
    R += k;
    ++first[k];
  }
  if (R > kMaxRows)
    return prego_fail_(PREGO_EINVAL, "%s: %d streams with %lld frames in all (at most %d rows per call: use forward() with h0 / h_last)", who, n, R,
                       kMaxRows);
  for (int k = kMaxFrames, at = 0; k >= 1; --k) {
    const int c = first[k];
    if (c > 0 && p->kmax == 0) p->kmax = k;
    first[k] = at;
    at += c;
    for (int t = 0; t < k; ++t) p->alive[t] += c;
  }
  for (int i = 0, off = 0; i < n; ++i) {
    const int k = n_frames[i];
    const unsigned e = ragged_entry((unsigned)off, (unsigned)i, (unsigned)k);
    p->by_stream.e[i] = e;
    p->walk.e[first[k]++] = e;
    off += k;
  }
  for (int i = n; i < kRaggedMaxStreams; ++i) p->by_stream.e[i] = p->walk.e[i] = 0u;
  p->rows = (int)R;
  return 0;
}

extern "C" size_t prego_miniroad_step_frames_workspace_bytes(const prego_miniroad* h, int n_streams, int n_frames) {
  if (!h || !frames_shape_ok(n_streams, n_frames)) return 0;
  return frames_layout(h, n_streams, n_streams * n_frames).total;
}

extern "C" int prego_miniroad_step_frames(prego_miniroad* h, int n_streams, int n_frames, const float* rgb, const float* flow, float* h_state,
                                          float* out, int32_t* argmax, int flags, void* workspace, size_t workspace_bytes,
                                          prego_stream_t stream) {
  return step_frames_impl(h, n_streams, n_frames, rgb, flow, h_state, out, argmax, false, nullptr, nullptr, flags, workspace, workspace_bytes,
                          stream);
}

extern "C" int prego_miniroad_step_frames_anticipation(prego_miniroad* h, int n_streams, int n_frames, const float* rgb, const float* flow,
                                                       float* h_state, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax,
                                                       int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return step_frames_impl(h, n_streams, n_frames, rgb, flow, h_state, out, argmax, true, ant_out, ant_argmax, flags, workspace, workspace_bytes,
                          stream);
}

extern "C" size_t prego_miniroad_step_ragged_workspace_bytes(const prego_miniroad* h, int n_streams, int n_rows) {
  if (!h || !ragged_shape_ok(n_streams, n_rows)) return 0;
  return frames_layout(h, n_streams, n_rows).total;
}

extern "C" int prego_miniroad_step_ragged(prego_miniroad* h, int n_streams, const int32_t* n_frames, const float* rgb, const float* flow,
                                          float* h_state, float* out, int32_t* argmax, int flags, void* workspace, size_t workspace_bytes,
                                          prego_stream_t stream) {
  return step_ragged_impl(h, n_streams, n_frames, rgb, flow, h_state, out, argmax, false, nullptr, nullptr, flags, workspace, workspace_bytes,
                          stream);
}

extern "C" int prego_miniroad_step_ragged_anticipation(prego_miniroad* h, int n_streams, const int32_t* n_frames, const float* rgb,
                                                       const float* flow, float* h_state, float* out, int32_t* argmax, float* ant_out,
                                                       int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                                                       prego_stream_t stream) {
  return step_ragged_impl(h, n_streams, n_frames, rgb, flow, h_state, out, argmax, true, ant_out, ant_argmax, flags, workspace, workspace_bytes,
                          stream);
}
