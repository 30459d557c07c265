// Host side of the streaming step (include/prego_amd.h: prego_miniroad_step / _anticipation for up to 16 streams, kernels stream_step.hip
// and stream_ant.hip; prego_miniroad_step_wide / _anticipation for up to 256, kernels stream_wide.hip) and the refusals every streaming
// entry point shares.
#include "miniroad_handle.h"

// what every streaming step refuses, n_max = 16 (step) or 256 (step_wide, step_pool) streams per call; 0 = the call may go ahead
int step_refusals(prego_miniroad* h, int n_streams, int n_max, const float* rgb, const float* flow, const float* h_state, bool ant) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "step before set_weights");
  if (!h->bf16) return prego_fail_(PREGO_EINVAL, "step: the streaming fast path takes bf16 / fp16 handles (fp32 / fp16x2 operands: use forward() with h0 / h_last)");
  if (h->hid != 1024 || h->layers != 1)
    return prego_fail_(PREGO_EINVAL, "step: the streaming kernels are built for hidden_dim 1024, one GRU layer (hidden_dim %d, %d layers: use forward() with h0 / h_last)", h->hid, h->layers);
  if (n_streams < 1 || n_streams > n_max) return prego_fail_(PREGO_EINVAL, "step: %d streams (1..%d per call)", n_streams, n_max);
  if (!h_state) return prego_fail_(PREGO_EINVAL, "step: h_state is NULL");
  if (h->d_rgb > 0 && !rgb) return prego_fail_(PREGO_EINVAL, "step: rgb is NULL");
  if (h->d_rgb == 0 && !flow) return prego_fail_(PREGO_EINVAL, "a model without rgb features (--no_rgb) needs the flow frame");
  if (ant && (h->ant_len <= 0 || !h->w_a || !h->st_ant)) return prego_fail_(PREGO_EINVAL, "step_anticipation before set_anticipation");
  return 0;
}

// streaming step: one frame for each of n <= 16 streams (stream_step.hip); ant = prego_miniroad_step_anticipation, whose trunk launches
// and their arguments are these very ones, followed by the anticipation head's two (stream_ant.hip) when an output is wanted
static int step_impl(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out, int32_t* argmax,
                     bool ant, float* ant_out, int32_t* ant_argmax, int flags, prego_stream_t stream) {
  HandleScope scope_(h);
  if (int rc = step_refusals(h, n_streams, 16, rgb, flow, h_state, ant)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int E = h->emb, H = h->hid, din = h->d_rgb + h->d_flow;
  float* Y = (float*)h->st_scratch;
  void* Eb = h->st_scratch + (size_t)16 * E * 4;
  float* GI = (float*)(h->st_scratch + (size_t)16 * E * 6);
  float* GH = GI + (size_t)16 * 3 * H;
  const bool with_flow = flow != nullptr && h->d_flow > 0;
  // layer1: K = the columns actually present (a zero flow half drops its half of K, as in forward())
  StreamGemv l1{h->w1, rgb, with_flow ? flow : nullptr, h->b1, Y, E, din, h->d_rgb, h->d_rgb, h->d_flow, 0};
  if (launch_stream_gemv(1, &l1, n_streams, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step: unsupported layer1 shape %d x %d", E, din);
  // LayerNorm + ReLU: inside the W_ih product for <= 4 streams (three launches per frame), the batched kernel otherwise
  static const bool no_fuse = prego_tune_env("PREGO_STEP_NO_LN_FUSE") != nullptr;
  const bool fuse_ln = n_streams <= 4 && E % 2048 == 0 && !no_fuse;
  if (!fuse_ln) launch_ln_relu(true, Y, h->ln_g, h->ln_b, n_streams, E, 1e-5f, Eb, nullptr, 0.f, 0ull, 0, s, 1, false, h->f16);
  StreamGemv g2[2] = {{h->w_ih, fuse_ln ? (const void*)Y : (const void*)Eb, nullptr, h->bias2, GI, 3 * H, E, E, E, 0, fuse_ln ? 0 : 1},
                      {h->w_hh, h_state, nullptr, nullptr, GH, 3 * H, H, H, H, 0, 0}};
  if (fuse_ln) { g2[0].ln_g = h->ln_g; g2[0].ln_b = h->ln_b; g2[0].ln_eps = 1e-5f; }
  if (launch_stream_gemv(2, g2, n_streams, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step: unsupported GRU shape %d / %d", E, H);
  if (launch_stream_gates_head(GI, GH, h->b_hn, h_state, h->w_c, h->b_c, n_streams, H, h->ncls, (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, out,
                               (int*)argmax, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step: unsupported head shape %d x %d", h->ncls, H);
  if (ant && (ant_out || ant_argmax)) {
    // the head reads the state the launch above has just written: relu + rounding on load is the classifier's own operand
    if (launch_stream_ant_hidden(h->w_a, h->b_a, h_state, h->st_ant, n_streams, H, h->ant_len, s, h->f16) ||
        launch_stream_ant_head(h->st_ant, h->w_c, h->b_c, n_streams, H, h->ant_len, h->ncls, (flags & PREGO_FWD_SOFTMAX) ? 1 : 0, ant_out,
                               (int*)ant_argmax, s, h->f16))
      return prego_fail_(PREGO_EINVAL, "step_anticipation: unsupported head shape %d x %d x %d", h->ant_len, h->ncls, H);
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_miniroad_step(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out,
                                   int32_t* argmax, int flags, prego_stream_t stream) {
  return step_impl(h, n_streams, rgb, flow, h_state, out, argmax, false, nullptr, nullptr, flags, stream);
}

extern "C" int prego_miniroad_step_anticipation(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state,
                                                float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags,
                                                prego_stream_t stream) {
  return step_impl(h, n_streams, rgb, flow, h_state, out, argmax, true, ant_out, ant_argmax, flags, stream);
}

// wide streaming step (stream_wide.hip): the caller's workspace for 17..256 streams, every part 256-byte aligned
//   xb [n][d_rgb + d_flow] 16-bit | hb [n][H] 16-bit | y [n][emb] f32 | e [n][emb] 16-bit | gi [n][3H] f32 | gh [n][3H] f32 | A [n][L H] 16-bit
struct WideLayout { size_t xb, hb, y, e, gi, gh, a, total; };
static WideLayout wide_layout(const prego_miniroad* h, int n) {
  const size_t E = (size_t)h->emb, H = (size_t)h->hid, din = (size_t)(h->d_rgb + h->d_flow);
  WideLayout w{};
  WsCarver c;
  w.xb = c.take(n * din * 2); w.hb = c.take(n * H * 2); w.y = c.take(n * E * 4); w.e = c.take(n * E * 2);
  w.gi = c.take(n * 3 * H * 4); w.gh = c.take(n * 3 * H * 4);
  w.a = c.take(h->ant_len > 0 ? (size_t)n * h->ant_len * H * 2 : 0);       // after set_anticipation: either entry point fits
  w.total = c.o;
  return w;
}

extern "C" size_t prego_miniroad_step_wide_workspace_bytes(const prego_miniroad* h, int n_streams) {
  if (!h || n_streams <= 16 || n_streams > 256) return 0;
  return wide_layout(h, n_streams).total;
}

// <= 16 streams: step_impl itself (its launches, the handle's scratch, the fused LayerNorm up to 4).  Above: the same arithmetic per output
// element - the unfused route of step_impl launch for launch, each product walking the stream tiles - on the caller's workspace
static int step_wide_impl(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out, int32_t* argmax,
                          bool ant, float* ant_out, int32_t* ant_argmax, int flags, void* workspace, size_t workspace_bytes,
                          prego_stream_t stream) {
  if (n_streams >= 1 && n_streams <= 16) return step_impl(h, n_streams, rgb, flow, h_state, out, argmax, ant, ant_out, ant_argmax, flags, stream);
  HandleScope scope_(h);
  if (int rc = step_refusals(h, n_streams, 256, rgb, flow, h_state, ant)) return rc;
  const WideLayout w = wide_layout(h, n_streams);
  if (int rc = workspace_refusal("step_wide", "prego_miniroad_step_wide_workspace_bytes", workspace, workspace_bytes, w.total, "%d streams", n_streams))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const int E = h->emb, H = h->hid, din = h->d_rgb + h->d_flow, sm = (flags & PREGO_FWD_SOFTMAX) ? 1 : 0;
  char* ws = (char*)workspace;
  float* Y = (float*)(ws + w.y);
  float* GI = (float*)(ws + w.gi);
  float* GH = (float*)(ws + w.gh);
  if (launch_wide_cast(h->d_rgb > 0 ? rgb : nullptr, h->d_flow > 0 ? flow : nullptr, h_state, ws + w.xb, ws + w.hb, n_streams, h->d_rgb,
                       h->d_flow, H, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step_wide: unsupported feature widths %d + %d", h->d_rgb, h->d_flow);
  StreamGemv l1{h->w1, ws + w.xb, nullptr, h->b1, Y, E, din, din, din, 0, 1};
  if (launch_wide_gemv(1, &l1, n_streams, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step_wide: unsupported layer1 shape %d x %d", E, din);
  launch_ln_relu(true, Y, h->ln_g, h->ln_b, n_streams, E, 1e-5f, ws + w.e, nullptr, 0.f, 0ull, 0, s, 1, false, h->f16);
  StreamGemv g2[2] = {{h->w_ih, ws + w.e, nullptr, h->bias2, GI, 3 * H, E, E, E, 0, 1}, {h->w_hh, ws + w.hb, nullptr, nullptr, GH, 3 * H, H, H, H, 0, 1}};
  if (launch_wide_gemv(2, g2, n_streams, s, h->f16)) return prego_fail_(PREGO_EINVAL, "step_wide: unsupported GRU shape %d / %d", E, H);
  // one workgroup per stream as in step: at most 256 of them, W_c from the L2
  if (launch_stream_gates_head(GI, GH, h->b_hn, h_state, h->w_c, h->b_c, n_streams, H, h->ncls, sm, out, (int*)argmax, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "step_wide: unsupported head shape %d x %d", h->ncls, H);
  if (ant && (ant_out || ant_argmax)) {
    if (launch_wide_ant_hidden(h->w_a, h->b_a, h_state, ws + w.a, n_streams, H, h->ant_len, s, h->f16) ||
        launch_wide_ant_head(ws + w.a, h->w_c, h->b_c, n_streams, H, h->ant_len, h->ncls, sm, ant_out, (int*)ant_argmax, s, h->f16))
      return prego_fail_(PREGO_EINVAL, "step_wide_anticipation: unsupported head shape %d x %d x %d", h->ant_len, h->ncls, H);
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_miniroad_step_wide(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out,
                                        int32_t* argmax, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return step_wide_impl(h, n_streams, rgb, flow, h_state, out, argmax, false, nullptr, nullptr, flags, workspace, workspace_bytes, stream);
}

extern "C" int prego_miniroad_step_wide_anticipation(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state,
                                                     float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags,
                                                     void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return step_wide_impl(h, n_streams, rgb, flow, h_state, out, argmax, true, ant_out, ant_argmax, flags, workspace, workspace_bytes, stream);
}
