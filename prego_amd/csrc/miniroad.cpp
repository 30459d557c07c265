// C ABI of the MiniROAD hot path (include/prego_amd.h), host side: the error state, the handle's lifecycle and weight ingestion, and the
// small entry points around a pass (check, timing, pass_info, resident buffer, data-parallel guard).  The pass itself:
//   miniroad_plan.cpp (packing plan, workspace layout) -> miniroad_forward.cpp (pass choice, chunked pass:
//   pack -> GEMM(layer1) -> LayerNorm+ReLU -> GEMM(W_ih) -> persistent GRU recurrence -> head+softmax+argmax) / miniroad_split.cpp
//   (split pass); training in miniroad_train.cpp; the private declarations they share in miniroad_handle.h.
#include "miniroad_handle.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

static thread_local std::string g_err;
static thread_local prego_miniroad* g_cur = nullptr;      // the handle whose entry point is running on this thread
HandleScope::HandleScope(prego_miniroad* h) { g_cur = h; }
HandleScope::~HandleScope() { g_cur = nullptr; }
// shared by every host file (host_common.h)
int prego_fail_(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  if (g_cur) g_cur->err = buf;
  return code;
}

const char* prego_tune_env(const char* name) {          // kernels.h
#ifdef PREGO_DEBUG_ABI
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

extern "C" const char* prego_miniroad_last_error(const prego_miniroad* h) { return h ? h->err.c_str() : "handle is NULL"; }

extern "C" int prego_abi_version(void) { return PREGO_ABI_VERSION; }
#ifdef PREGO_DEBUG_ABI
std::atomic<long long> g_dbg_mallocs{0}, g_dbg_syncs{0};      // counted by the macros of miniroad_handle.h
void launch_debug_hog(int xcd_lo, int kind, int ms, const void* buf, void* wbuf, size_t bytes, float* sink, hipStream_t s);     // debug_hog.hip
extern "C" int prego_debug_hog(int kind, int xcd_lo, int ms, const void* read_buf, void* write_buf, size_t bytes, float* sink, prego_stream_t stream) {
  if (kind < 1 || kind > 3 || xcd_lo < 0 || xcd_lo > 7 || ms <= 0 || !sink || ((kind & 2) && (!read_buf || !write_buf || bytes < (1u << 20))))
    return prego_fail_(PREGO_EINVAL, "debug hog: bad arguments");
  launch_debug_hog(xcd_lo, kind, ms, read_buf, write_buf, bytes, sink, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
extern "C" int prego_debug_alloc_count(int64_t* device_mallocs, int64_t* host_waits) {
  if (device_mallocs) *device_mallocs = g_dbg_mallocs.load();
  if (host_waits) *host_waits = g_dbg_syncs.load();
  return PREGO_OK;
}
#endif

extern "C" const char* prego_last_error(void) { return g_err.c_str(); }

extern "C" int prego_miniroad_create(prego_miniroad** out, int d_rgb, int d_flow, int emb, int hid, int n_classes,
                                     int compute_dtype) {
  return prego_miniroad_create_layers(out, d_rgb, d_flow, emb, hid, n_classes, 1, compute_dtype);
}
extern "C" int prego_miniroad_create_layers(prego_miniroad** out, int d_rgb, int d_flow, int emb, int hid, int n_classes, int num_layers,
                                            int compute_dtype) {
  if (!out) return prego_fail_(PREGO_EINVAL, "out is NULL");
  *out = nullptr;
  if (compute_dtype != PREGO_F32 && compute_dtype != PREGO_BF16 && compute_dtype != PREGO_F16 && compute_dtype != PREGO_F16X2)
    return prego_fail_(PREGO_EINVAL, "compute_dtype %d", compute_dtype);
  // The recurrence keeps a workgroup's slice of W_hh in registers (3 gates x 16 or 32 rows x H): what fits decides.  16-bit operands:
  // 512, 1024, 2048; exact-fp32 operands: 512, 1024 (a 16-row slice of H = 2048 is 384 registers per lane); split operands: 1024
  {
    const bool op16 = compute_dtype == PREGO_BF16 || compute_dtype == PREGO_F16;
    const bool ok = compute_dtype == PREGO_F16X2 ? hid == 1024 : gru_hidden_supported(op16, hid);
    if (!ok) return prego_fail_(PREGO_EINVAL, "hidden_dim %d unsupported with compute_dtype %d: 512 / 1024 / 2048 with 16-bit operands, 512 / 1024 with fp32 "
                                       "operands, 1024 with fp16x2 (the recurrence keeps its W_hh slice in registers)", hid, compute_dtype);
  }
  if (num_layers < 1 || num_layers > 2) return prego_fail_(PREGO_EINVAL, "num_layers %d: 1 or 2", num_layers);
  if (num_layers == 2 && compute_dtype == PREGO_F16X2)
    return prego_fail_(PREGO_EINVAL, "num_layers 2 with fp16x2 operands: the split-operand recurrence hands fp32 relu(h) to the classifier only (use fp32)");
  if (emb <= 0 || emb % 512 || emb > 4096) return prego_fail_(PREGO_EINVAL, "embedding_dim %d must be a multiple of 512, <= 4096", emb);
  if (d_rgb < 0 || d_flow < 0 || d_rgb + d_flow <= 0 || (d_rgb % 64) || (d_flow % 64))
    return prego_fail_(PREGO_EINVAL, "feature sizes %d/%d must be multiples of 64", d_rgb, d_flow);
  if (n_classes <= 0 || n_classes > 128) return prego_fail_(PREGO_EINVAL, "num_classes %d must be in 1..128", n_classes);
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  prego_miniroad* h = new prego_miniroad();
  h->d_rgb = d_rgb; h->d_flow = d_flow; h->emb = emb; h->hid = hid; h->ncls = n_classes;
  h->ncls_pad = (n_classes + 15) / 16 * 16;
  h->bf16 = compute_dtype == PREGO_BF16 || compute_dtype == PREGO_F16;
  h->f16 = compute_dtype == PREGO_F16;
  h->x2 = compute_dtype == PREGO_F16X2;      // operand storage 4 bytes per element ([hi | lo] fp16), P = 64, G = 4 like fp32 operands
  h->n_cu = prop.multiProcessorCount;
  h->layers = num_layers;
  h->P = h->x2 ? hid / 16 : gru_group_size(h->bf16, hid);      // 1024: 32 (16-bit) / 64 workgroups per group
  h->G = std::min(h->bf16 ? 8 : 4, h->n_cu / h->P);
  if (h->G < 1) { delete h; return prego_fail_(PREGO_EINVAL, "device has %d CUs, the recurrence needs >= %d", prop.multiProcessorCount, h->bf16 ? 32 : 64); }
  const size_t es = h->bf16 ? 2 : 4;
  const int din = d_rgb + d_flow, H = hid;
  hipError_t e = hipSuccess;
  auto A = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
  A(&h->w1, (size_t)emb * din * es); A((void**)&h->b1, emb * 4); A((void**)&h->ln_g, emb * 4); A((void**)&h->ln_b, emb * 4);
  A(&h->w_ih, (size_t)3 * H * emb * es); A(&h->w_hh, (size_t)3 * H * H * es);
  A((void**)&h->bias2, 3 * H * 4); A((void**)&h->b_hn, H * 4);
  if (h->bf16 && H == 1024) { A(&h->w_ih_perm, (size_t)3 * H * emb * es); A((void**)&h->bias2_perm, 3 * H * 4); }
  A(&h->w_c, (size_t)h->ncls_pad * H * es); A((void**)&h->b_c, h->ncls_pad * 4);
  A(&h->hx, h->x2 ? gru_x2_hx_bytes(H, h->G) : gru_hx_bytes(h->bf16, H, h->G));
  if (h->x2) A((void**)&h->x2_scale, 6 * sizeof(float));
  A((void**)&h->flags, ((size_t)h->G * h->P + 16) * sizeof(unsigned));
  A((void**)&h->h_state, (size_t)num_layers * max_slots_of(h) * H * 4);
  if (num_layers == 2) {
    A(&h->l2_w_ih, (size_t)3 * H * H * es); A(&h->l2_w_hh, (size_t)3 * H * H * es);
    A((void**)&h->l2_bias2, 3 * H * 4); A((void**)&h->l2_b_hn, H * 4);
  }
  A((void**)&h->d_ptrs, (size_t)6 * max_clips_of(h) * sizeof(void*));
  // plan tables pre-sized here so that forward() allocates nothing: 131 072 steps (a 72-minute clip at 30 frames/s; the longest
  // Epic-tent-O video has 31 114 frames) and max_clips clips; only a longer clip than that makes forward() grow them
  h->cap_t = (size_t)131072 + 1;
  h->cap_c = (size_t)max_clips_of(h) + 64;
  A((void**)&h->d_rowoff, h->cap_t * 4); A((void**)&h->d_nact, h->cap_t * 4);
  A((void**)&h->d_sorted, h->cap_c * 4); A((void**)&h->d_seg_off, (h->cap_c + 1) * 4);
  A((void**)&h->d_seg_clip, h->cap_c * 4); A((void**)&h->d_seg_start, h->cap_c * 4);
  h->cap_b = (size_t)1 << 19;                    // 16.7 M packed rows per call before the table has to grow
  A((void**)&h->d_blkstep, h->cap_b * 4);
  h->pin_bytes = (size_t)6 * max_clips_of(h) * sizeof(void*) + 2 * h->cap_t * 4 + 4 * (h->cap_c + 1) * 4 + h->cap_b * 4 + 1024;
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin, h->pin_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->pin_ev, hipEventDisableTiming);
  h->no_local = getenv("PREGO_GRU_NO_LOCAL") != nullptr;
  h->no_mt = getenv("PREGO_GRU_NO_MT") != nullptr;
  h->pack_prefetch = prego_tune_env("PREGO_NO_PACK_PREFETCH") == nullptr;
  // the pack beside the recurrence slows its L2 hand-off; capped at 512 workgroups it still ends inside a 49 152-row launch and
  // costs the pass 0.9 ms less than unthrottled (sweep: scripts/probes/env_sweep.sh, 128: +10 ms, 256: +1, 512: -0.9, 1024: 0)
  h->prefetch_grid = 512;
  if (const char* pg = prego_tune_env("PREGO_PACK_PREFETCH_GRID")) h->prefetch_grid = atoi(pg);
  // The side stream must run BESIDE the caller's stream.  HIP maps streams onto a handful of hardware queues in creation order and
  // two streams on one queue execute in submission order (round 4: an eval loop whose copy stream shared the compute stream's queue
  // lost all of its overlap), and a queue has one priority: a LOW-priority side stream never shares the queue of a normal-priority
  // caller, and its pack / layer1 worker yield to the recurrence where they compete.  PREGO_SIDE_PRIO=0: the plain stream (A/B).
  if (e == hipSuccess) {
    int lo = 0, hi = 0;
    static const bool plain = prego_tune_env("PREGO_SIDE_PRIO") != nullptr && atoi(prego_tune_env("PREGO_SIDE_PRIO")) == 0;
    if (!plain && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
      e = hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo);       // lo = numerically greatest = least priority
    else
      e = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
  A((void**)&h->stamps, 8 * sizeof(unsigned long long));
  A((void**)&h->tile_ctr, 4096 * sizeof(unsigned));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin_place, 64, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_place, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin_hs, 64, hipHostMallocDefault);
  if (e == hipSuccess) *(volatile unsigned*)h->pin_hs = 0u;
  if (e == hipSuccess) e = hipEventCreate(&h->chooser.ev_meas[0]);
  if (e == hipSuccess) e = hipEventCreate(&h->chooser.ev_meas[1]);
  h->xcd_overlap = getenv("PREGO_NO_XCD_OVERLAP") == nullptr;       // A/B knob: PREGO_NO_XCD_OVERLAP=1 = the serial pass of round 2
  if (const char* sp = getenv("PREGO_SPLIT_PASS")) h->chooser.split_env = atoi(sp);
  A((void**)&h->st_scratch, (size_t)16 * ((size_t)emb * 6 + (size_t)3 * H * 8));
  if (e == hipSuccess) e = hipMemset(h->stamps, 0, 8 * sizeof(unsigned long long));
  h->use_stamps = prego_tune_env("PREGO_GRU_STAMPS") != nullptr;
  if (e == hipSuccess) e = hipMemset(h->hx, 0, h->x2 ? gru_x2_hx_bytes(H, h->G) : gru_hx_bytes(h->bf16, H, h->G));
  if (e == hipSuccess) e = hipMemset(h->flags, 0, ((size_t)h->G * h->P + 16) * sizeof(unsigned));
  if (e != hipSuccess) { prego_miniroad_destroy(h); return prego_fail_(PREGO_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
  h->abort_word = h->flags + (size_t)h->G * h->P;
  *out = h;
  return PREGO_OK;
}

// teardown calls must not leave an error code behind for whatever HIP call the process makes next (a swallowed hipErrorInvalidValue here
// surfaced in an unrelated torch kernel launch of the NEXT test): every failure is consumed, and named in the debug library
#ifdef PREGO_DEBUG_ABI
#define PREGO_TEARDOWN(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "prego_miniroad_destroy: %s -> %s\n", #x, hipGetErrorName(e_)); (void)hipGetLastError(); } } while (0)
#else
#define PREGO_TEARDOWN(x) do { if ((x) != hipSuccess) (void)hipGetLastError(); } while (0)
#endif
extern "C" void prego_miniroad_destroy(prego_miniroad* h) {
  if (!h) return;
  if (h->side) { PREGO_TEARDOWN(hipStreamSynchronize(h->side)); PREGO_TEARDOWN(hipStreamDestroy(h->side)); }
  void* ptrs[] = {h->w1, h->b1, h->ln_g, h->ln_b, h->w_ih, h->w_hh, h->bias2, h->b_hn, h->w_c, h->b_c, h->hx,
                  h->flags, h->h_state, h->stamps, h->tile_ctr, h->d_rowoff, h->d_nact, h->d_sorted, h->d_seg_off, h->d_seg_clip,
                  h->d_seg_start, h->d_ptrs, h->d_blkstep, h->st_scratch, h->x2_scale, h->l2_w_ih, h->l2_w_hh, h->l2_bias2, h->l2_b_hn, h->w_ih_perm, h->bias2_perm,
                  h->w_a, h->b_a, h->st_ant};
  for (size_t i = 0; i < sizeof ptrs / sizeof ptrs[0]; ++i)
    if (ptrs[i]) {
#ifdef PREGO_DEBUG_ABI
      const hipError_t e_ = hipFree(ptrs[i]);
      if (e_ != hipSuccess) { fprintf(stderr, "prego_miniroad_destroy: hipFree(ptrs[%zu] = %p) -> %s\n", i, ptrs[i], hipGetErrorName(e_)); (void)hipGetLastError(); }
#else
      PREGO_TEARDOWN(hipFree(ptrs[i]));
#endif
    }
  for (auto& ev : h->ev_pool) { PREGO_TEARDOWN(hipEventDestroy(ev.a)); PREGO_TEARDOWN(hipEventDestroy(ev.b)); }
  if (h->pin_ev) { if (h->pin_busy) PREGO_TEARDOWN(hipEventSynchronize(h->pin_ev)); PREGO_TEARDOWN(hipEventDestroy(h->pin_ev)); }
  if (h->pin) PREGO_TEARDOWN(hipHostFree(h->pin));
  if (h->ev_fork) PREGO_TEARDOWN(hipEventDestroy(h->ev_fork));
  if (h->ev_join) PREGO_TEARDOWN(hipEventDestroy(h->ev_join));
  if (h->ev_place) PREGO_TEARDOWN(hipEventDestroy(h->ev_place));
  for (hipEvent_t ev : h->chooser.ev_meas) if (ev) PREGO_TEARDOWN(hipEventDestroy(ev));
  for (hipEvent_t ev : h->ev_split) if (ev) PREGO_TEARDOWN(hipEventDestroy(ev));
  if (h->pin_place) PREGO_TEARDOWN(hipHostFree(h->pin_place));
  if (h->pin_hs) PREGO_TEARDOWN(hipHostFree(h->pin_hs));
  delete h;
}

extern "C" int prego_miniroad_max_clips(const prego_miniroad* h) { return h ? max_clips_of(h) : 0; }

extern "C" int prego_miniroad_set_weights(prego_miniroad* h, const float* layer1_w, const float* layer1_b,
                                          const float* ln_w, const float* ln_b, const float* w_ih, const float* w_hh,
                                          const float* b_ih, const float* b_hh, const float* fc_w, const float* fc_b,
                                          prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!layer1_w || !layer1_b || !ln_w || !ln_b || !w_ih || !w_hh || !b_ih || !b_hh || !fc_w || !fc_b)
    return prego_fail_(PREGO_EINVAL, "set_weights: NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  const int din = h->d_rgb + h->d_flow, E = h->emb, H = h->hid;
  if (h->x2) {                   // split rows [cols hi | cols lo] of W * 2^k, k per tensor (common.h)
    launch_x2_weight_split(layer1_w, E, din, h->w1, h->x2_scale + 0, s);
    launch_x2_weight_split(w_ih, 3 * H, E, h->w_ih, h->x2_scale + 2, s);
    launch_x2_weight_split(w_hh, 3 * H, H, h->w_hh, h->x2_scale + 4, s);
  } else {
    launch_pad_convert(h->bf16, layer1_w, E, din, din, h->w1, E, din, s, h->f16);
    launch_pad_convert(h->bf16, w_ih, 3 * H, E, E, h->w_ih, 3 * H, E, s, h->f16);
    launch_pad_convert(h->bf16, w_hh, 3 * H, H, H, h->w_hh, 3 * H, H, s, h->f16);
  }
  launch_pad_convert(h->bf16, fc_w, h->ncls, H, H, h->w_c, h->ncls_pad, H, s, h->f16);
  launch_pad_convert(false, fc_b, 1, h->ncls, h->ncls, h->b_c, 1, h->ncls_pad, s);
  HIPCHK(hipMemcpyAsync(h->b1, layer1_b, E * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(h->ln_g, ln_w, E * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(h->ln_b, ln_b, E * 4, hipMemcpyDeviceToDevice, s));
  launch_add_vec(b_ih, b_hh, h->bias2, 3 * H, 2 * H, s);   // r,z rows: b_ih + b_hh ; n rows: b_ih
  h->perm_stale = true;
  HIPCHK(hipMemcpyAsync(h->b_hn, b_hh + 2 * H, H * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  h->have_weights = true;
  return PREGO_OK;
}

extern "C" int prego_miniroad_set_gru_layer(prego_miniroad* h, int layer, const float* w_ih, const float* w_hh, const float* b_ih,
                                            const float* b_hh, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (layer != 1 || h->layers != 2) return prego_fail_(PREGO_EINVAL, "set_gru_layer: layer %d of a %d-layer handle (layer 0 comes with set_weights)", layer, h->layers);
  if (!w_ih || !w_hh || !b_ih || !b_hh) return prego_fail_(PREGO_EINVAL, "set_gru_layer: NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  const int H = h->hid;
  launch_pad_convert(h->bf16, w_ih, 3 * H, H, H, h->l2_w_ih, 3 * H, H, s, h->f16);
  launch_pad_convert(h->bf16, w_hh, 3 * H, H, H, h->l2_w_hh, 3 * H, H, s, h->f16);
  launch_add_vec(b_ih, b_hh, h->l2_bias2, 3 * H, 2 * H, s);
  HIPCHK(hipMemcpyAsync(h->l2_b_hn, b_hh + 2 * H, H * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  h->have_layer2 = true;
  return PREGO_OK;
}

// ---- MiniROADA (MROADA, registry name "MiniROADA"): the anticipation head (rnn.py:113-136; csrc/ant_head.hip) -----------------------
extern "C" int prego_miniroad_set_anticipation(prego_miniroad* h, int ant_len, const float* w_a, const float* b_a, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (h->x2) return prego_fail_(PREGO_EINVAL, "set_anticipation: fp16x2 (split-operand) handles have no anticipation head; use fp32, bf16 or fp16");
  if (h->layers != 1)
    return prego_fail_(PREGO_EINVAL, "set_anticipation: num_layers %d - MiniROADA runs one GRU layer (its h0 is (1, B, H), rnn.py:122)", h->layers);
  if (ant_len < 1 || ant_len > 32) return prego_fail_(PREGO_EINVAL, "set_anticipation: anticipation_length %d must be in 1..32", ant_len);
  if (!w_a || !b_a) return prego_fail_(PREGO_EINVAL, "set_anticipation: NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  const int H = h->hid;
  const size_t es = h->bf16 ? 2 : 4, need = (size_t)ant_len * H * H * es;
  if (need > h->w_a_cap || ant_len > h->ant_len) {
    // setup call, not a hot one: the old copies may still be read by enqueued work of this stream
    HIPCHK(hipStreamSynchronize(s));
    if (h->w_a) { HIPCHK(hipFree(h->w_a)); h->w_a = nullptr; }
    if (h->b_a) { HIPCHK(hipFree(h->b_a)); h->b_a = nullptr; }
    if (h->st_ant) { HIPCHK(hipFree(h->st_ant)); h->st_ant = nullptr; }
    h->w_a_cap = 0;
    HIPCHK(hipMalloc(&h->w_a, need));
    HIPCHK(hipMalloc((void**)&h->b_a, (size_t)ant_len * H * 4));
    // streaming step (prego_miniroad_step_anticipation; 16-bit handles of hidden_dim 1024): its 16-bit intermediate, allocated
    // here so that the step itself never allocates
    if (h->bf16 && H == 1024) HIPCHK(hipMalloc(&h->st_ant, (size_t)16 * ant_len * H * 2));
    h->w_a_cap = need;
  }
  launch_pad_convert(h->bf16, w_a, ant_len * H, H, H, h->w_a, ant_len * H, H, s, h->f16);
  HIPCHK(hipMemcpyAsync(h->b_a, b_a, (size_t)ant_len * H * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  h->ant_len = ant_len;
  return PREGO_OK;
}

extern "C" int prego_miniroad_set_resident(prego_miniroad* h, void* device_buffer, size_t bytes) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if ((device_buffer == nullptr) != (bytes == 0)) return prego_fail_(PREGO_EINVAL, "set_resident: buffer %p with %zu bytes", device_buffer, bytes);
  if ((uintptr_t)device_buffer & 255) return prego_fail_(PREGO_EINVAL, "set_resident: the buffer must be 256-byte aligned");
  h->res_buf = (char*)device_buffer; h->res_bytes = bytes;
  return PREGO_OK;
}

// Data-parallel guard (round 6, advisor): a rank whose recurrence / BPTT gave up must stop EVERY rank's optimizer step, not only its own.
// publish: dst[0] = 1.0f if this handle's timeout word is set, else 0.0f - enqueued; dst is an element of the gradient bucket the ranks
// all-reduce (sum).  peer guard: the address of that element; prego_miniroad_adamw_step then changes nothing while it holds a non-zero
// value and raises this handle's own word (code 0x200), so prego_miniroad_check reports the step on every rank.
void launch_guard_publish(const unsigned* abort_word, float* dst, hipStream_t s);
extern "C" int prego_miniroad_guard_publish(prego_miniroad* h, float* dst, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !dst) return prego_fail_(PREGO_EINVAL, "guard_publish: NULL argument");
  launch_guard_publish(h->abort_word, dst, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
extern "C" int prego_miniroad_set_peer_guard(prego_miniroad* h, const float* reduced_word) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  h->peer_guard = reduced_word;
  return PREGO_OK;
}

EventPair* ev_begin(prego_miniroad* h, int kind, hipStream_t s) {
  if (!h->timing) return nullptr;
  if (h->ev_used == h->ev_pool.size()) {
    EventPair p;
    if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
    h->ev_pool.push_back(p);
    h->ev_kind.push_back(kind);
  }
  h->ev_kind[h->ev_used] = kind;
  EventPair* p = &h->ev_pool[h->ev_used++];
  (void)hipEventRecord(p->a, s);
  return p;
}
void ev_end(EventPair* p, hipStream_t s) { if (p) (void)hipEventRecord(p->b, s); }

extern "C" int prego_miniroad_check(prego_miniroad* h, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned ab = 0;
  HIPCHK(hipMemcpy(&ab, h->abort_word, sizeof ab, hipMemcpyDeviceToHost));
  if (ab) {
    (void)hipMemset(h->abort_word, 0, sizeof ab);
    // codes: 1 = the recurrence's gather / rendezvous; 3 = the recurrence of a split pass
    // waiting for its input projection; 0x100 + k = wait k of the feed-forward launch of a split pass (ff_pass.hip)
    if (ab == 0x200u)       // prego_miniroad_set_peer_guard: raised by the guarded AdamW step, not by a kernel of this handle
      return prego_fail_(PREGO_ETIMEOUT, "data-parallel training: a recurrence / BPTT kernel of ANOTHER rank timed out; every rank skipped the optimizer "
                  "steps from that one on (weights unchanged since the last good step) [code 0x200]");
    if (ab >= 2) {
      // a wait INSIDE a split pass ran out although its start handshake had seen both launches resident (launches that cannot run side by
      // side never get this far: they leave at the handshake and the call is re-run chunked, prego_miniroad_forward).  A stuck workgroup or a
      // bug: report it, keep this handle on the chunked pass
      h->chooser.split_env = 0;
      return prego_fail_(PREGO_ETIMEOUT, "split pass: a wait timed out behind a successful start handshake [code 0x%x]; the results of that call are "
                  "invalid, this handle now uses the chunked pass (PREGO_SPLIT_PASS=0 selects it from the start)", ab);
    }
    return prego_fail_(PREGO_ETIMEOUT, "GRU recurrence kernel timed out waiting for a producer workgroup (not all %d workgroups resident?) [code 0x%x]",
                h->G * h->P, ab);
  }
  return PREGO_OK;
}

extern "C" int prego_miniroad_timing_enable(prego_miniroad* h, int enable) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  h->timing = enable != 0;
  h->ev_used = 0;
  h->gemm_flop = 0;
  h->pack_bytes = 0;
  return PREGO_OK;
}

extern "C" int prego_miniroad_timing_read(prego_miniroad* h, double* gemm_ms, int64_t* gemm_launches, double* gemm_flop,
                                          double* gru_ms, int64_t* gru_launches, double* pack_ms,
                                          int64_t* pack_launches, double* pack_bytes) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  double ms[5] = {0, 0, 0, 0, 0};      // kinds: 0 gemm, 1 recurrence, 2 pack, 3 overlapped layer1 worker, 4 feed-forward launch of a split pass
  int64_t n[5] = {0, 0, 0, 0, 0};
  for (size_t i = 0; i < h->ev_used; ++i) {
    HIPCHK(hipEventSynchronize(h->ev_pool[i].b));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, h->ev_pool[i].a, h->ev_pool[i].b));
    ms[h->ev_kind[i]] += t;
    n[h->ev_kind[i]]++;
  }
  if (gemm_ms) *gemm_ms = ms[0];
  if (gemm_launches) *gemm_launches = n[0];
  if (gemm_flop) *gemm_flop = h->gemm_flop;
  if (gru_ms) *gru_ms = ms[1];
  if (gru_launches) *gru_launches = n[1];
  if (pack_ms) *pack_ms = ms[2];
  if (pack_launches) *pack_launches = n[2];
  if (pack_bytes) *pack_bytes = h->pack_bytes;
  h->ev_used = 0;
  h->gemm_flop = 0;
  h->pack_bytes = 0;
  return PREGO_OK;
}

extern "C" int prego_miniroad_pass_info(const prego_miniroad* h, int32_t* mode, int32_t* n_steps, int32_t* n_slots) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (mode) *mode = h->split_r;
  if (n_steps) *n_steps = h->t_max;
  if (n_slots) *n_slots = h->n_slots;
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
// debug: per-phase shader-cycle sums of workgroup 0 / wave 0 of the recurrence kernel (PREGO_GRU_STAMPS=1):
// out[0..4] = poll, mfma, reduce+barrier, gates+publish, outputs; out[5] = poll retry rounds; out[6] = time steps
extern "C" int prego_miniroad_debug_stamps(prego_miniroad* h, unsigned long long* out8) {
  if (!h || !out8) return prego_fail_(PREGO_EINVAL, "NULL");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out8, h->stamps, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(h->stamps, 0, 8 * sizeof(unsigned long long)));
  return PREGO_OK;
}

// unit-test hook: set the handle's timeout word as a kernel that gave up would (stream-ordered)
extern "C" int prego_debug_set_abort(prego_miniroad* h, unsigned value, prego_stream_t stream) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)h->abort_word, (int)value, 1, (hipStream_t)stream));
  return PREGO_OK;
}
#endif  // PREGO_DEBUG_ABI
