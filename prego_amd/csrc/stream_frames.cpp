// Host side of the multi-frame streaming step (include/prego_amd.h: prego_miniroad_step_frames / _anticipation; kernels:
// stream_frames.hip and the wide step's launchers, stream_wide.hip).  One call advances n streams by K frames each: the products that do
// not depend on time run once over the n K rows, the recurrence takes one fused launch per frame, the heads follow over all rows.
// Every refusal is decided before the first launch.
#include "miniroad_handle.h"

namespace {
constexpr int kMaxFrames = 32, kMaxRows = 256;

// the caller's workspace, every part 256-byte aligned (R = n K rows, row s K + t = frame t of stream s):
//   xb [R][d_rgb + d_flow] 16-bit | h0 [n][H] f32 | y [R][emb] f32 | e [R][emb] 16-bit | gi [R][3H] f32 | hist [R][H] f32 | hr [R][H] 16-bit
//   | A [R][L H] 16-bit (after set_anticipation)
struct FramesLayout { size_t xb, h0, y, e, gi, hist, hr, a, total; };
FramesLayout frames_layout(const prego_miniroad* h, int n, int K) {
  const size_t E = (size_t)h->emb, H = (size_t)h->hid, din = (size_t)(h->d_rgb + h->d_flow), R = (size_t)n * K;
  FramesLayout w{};
  WsCarver c;
  w.xb = c.take(R * din * 2); w.h0 = c.take((size_t)n * H * 4); w.y = c.take(R * E * 4); w.e = c.take(R * E * 2);
  w.gi = c.take(R * 3 * H * 4); w.hist = c.take(R * H * 4); w.hr = c.take(R * H * 2);
  w.a = c.take(h->ant_len > 0 ? R * h->ant_len * H * 2 : 0);          // after set_anticipation: either entry point fits
  w.total = c.o;
  return w;
}

bool frames_shape_ok(int n, int K) { return n >= 1 && K >= 1 && K <= kMaxFrames && (long long)n * K <= kMaxRows; }

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
  const FramesLayout w = frames_layout(h, n, K);
  if (int rc = workspace_refusal("step_frames", "prego_miniroad_step_frames_workspace_bytes", workspace, workspace_bytes, w.total,
                                 "%d streams x %d frames", n, K)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int E = h->emb, H = h->hid, din = h->d_rgb + h->d_flow, sm = (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, R = n * K;
  char* ws = (char*)workspace;
  float* Y = (float*)(ws + w.y);
  float* GI = (float*)(ws + w.gi);
  float* H0 = (float*)(ws + w.h0);
  float* HIST = (float*)(ws + w.hist);
  // everything that does not depend on time, once over the R rows: the wide step's launches with R in the place of n
  if (launch_frames_cast(h->d_rgb > 0 ? rgb : nullptr, h->d_flow > 0 ? flow : nullptr, h_state, ws + w.xb, H0, R, n, h->d_rgb, h->d_flow, H, s,
                         h->f16)) return prego_fail_(PREGO_EINVAL, "step_frames: unsupported feature widths %d + %d", h->d_rgb, h->d_flow);
  StreamGemv l1{h->w1, ws + w.xb, nullptr, h->b1, Y, E, din, din, din, 0, 1};
  if (launch_wide_gemv(1, &l1, R, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step_frames: unsupported layer1 shape %d x %d", E, din);
  launch_ln_relu(true, Y, h->ln_g, h->ln_b, R, E, 1e-5f, ws + w.e, nullptr, 0.f, 0ull, 0, s, 1, false, h->f16);
  StreamGemv gi{h->w_ih, ws + w.e, nullptr, h->bias2, GI, 3 * H, E, E, E, 0, 1};
  if (launch_wide_gemv(1, &gi, R, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step_frames: unsupported GRU shape %d / %d", E, H);
  // the sequential part: one fused launch per frame, ordered by the stream alone
  for (int t = 0; t < K; ++t)
    if (launch_frames_recur(h->w_hh, GI, h->b_hn, H0, HIST, ws + w.hr, t == K - 1 ? h_state : nullptr, n, K, t, H, s, h->f16))
      return prego_fail_(PREGO_EINVAL, "step_frames: unsupported GRU shape %d / %d", E, H);
  // the classifier over the relu(h) rows: the row-list head with one row per frame (wide_ant_head, L = 1)
  if ((out || argmax) && launch_wide_ant_head(ws + w.hr, h->w_c, h->b_c, R, H, 1, h->ncls, sm, out, (int*)argmax, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "step_frames: unsupported head shape %d x %d", h->ncls, H);
  if (ant && (ant_out || ant_argmax)) {
    if (launch_wide_ant_hidden(h->w_a, h->b_a, HIST, ws + w.a, R, H, h->ant_len, s, h->f16) ||
        launch_wide_ant_head(ws + w.a, h->w_c, h->b_c, R, H, h->ant_len, h->ncls, sm, ant_out, (int*)ant_argmax, s, h->f16))
      return prego_fail_(PREGO_EINVAL, "step_frames_anticipation: unsupported head shape %d x %d x %d", h->ant_len, h->ncls, H);
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" size_t prego_miniroad_step_frames_workspace_bytes(const prego_miniroad* h, int n_streams, int n_frames) {
  if (!h || !frames_shape_ok(n_streams, n_frames)) return 0;
  return frames_layout(h, n_streams, n_frames).total;
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
