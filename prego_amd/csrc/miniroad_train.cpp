// MiniROAD host side, training: dropout control, the loss, the backward pass and the AdamW steps.
#include "miniroad_handle.h"

#include <algorithm>
#include <cstring>
#include <mutex>

extern "C" int prego_miniroad_set_dropout(prego_miniroad* h, float p, uint64_t seed) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!(p >= 0.f && p < 1.f)) return prego_fail_(PREGO_EINVAL, "dropout p = %f", (double)p);
  h->drop_p = p;
  h->drop_seed = seed;
  return PREGO_OK;
}

// handle-free: OadLoss is a criterion object of its own in the reference (criterions/loss_builder.py:9-11).
// Scratch for the pointer tables is one small per-device allocation made on first use.
#define LOSS_MAX_CLIPS 4096
extern "C" int prego_oad_loss(int n_clips, const int32_t* lens, const float* const* logits, const float* const* target,
                              int n_classes, float* loss_out, float* const* dlogits, float grad_scale,
                              prego_stream_t stream) {
  return prego_oad_loss_reduce(n_clips, lens, logits, target, n_classes, 0, loss_out, dlogits, grad_scale, stream);
}
extern "C" int prego_oad_loss_reduce(int n_clips, const int32_t* lens, const float* const* logits, const float* const* target,
                                     int n_classes, int reduction, float* loss_out, float* const* dlogits, float grad_scale,
                                     prego_stream_t stream) {
  if (reduction != 0 && reduction != 1) return prego_fail_(PREGO_EINVAL, "loss: reduction %d (0 = 'mean', 1 = 'sum')", reduction);
  if (!lens || !logits || !target || !loss_out) return prego_fail_(PREGO_EINVAL, "loss: NULL argument");
  if (n_clips <= 0 || n_clips > LOSS_MAX_CLIPS) return prego_fail_(PREGO_EINVAL, "loss: %d clips (max %d)", n_clips, LOSS_MAX_CLIPS);
  if (n_classes <= 0 || n_classes > 128) return prego_fail_(PREGO_EINVAL, "loss: num_classes %d must be in 1..128", n_classes);
  // per-device scratch of this handle-free op: device pointer tables + a PINNED host staging copy fenced by an event (the
  // async H2D copy reads the staging buffer after this call has returned, so it is neither a stack nor a pageable buffer)
  struct LossScratch { void* dev = nullptr; void* pin = nullptr; hipEvent_t ev = nullptr; bool busy = false; };
  static LossScratch scratch[64];
  static std::mutex scratch_mu;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return prego_fail_(PREGO_EINVAL, "device %d", dev);
  const size_t MC = LOSS_MAX_CLIPS;
  std::lock_guard<std::mutex> guard(scratch_mu);
  LossScratch& sc = scratch[dev];
  if (!sc.dev) {
    HIPCHK(hipMalloc(&sc.dev, 4 * MC * sizeof(void*)));
    HIPCHK(hipHostMalloc(&sc.pin, 4 * MC * sizeof(void*), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  }
  if (sc.busy) { HIPCHK(hipEventSynchronize(sc.ev)); sc.busy = false; }
  void** d = (void**)sc.dev;
  hipStream_t s = (hipStream_t)stream;
  const void** tab = (const void**)sc.pin;
  // the four tables packed one behind the other (n_clips entries each): ONE host -> device copy per call (four copies of 128 bytes
  // were four 5 us blit launches in front of the loss kernel of every training step)
  const size_t n = (size_t)n_clips;
  for (int i = 0; i < n_clips; ++i) {
    if (lens[i] <= 0 || !logits[i] || !target[i]) return prego_fail_(PREGO_EINVAL, "loss: clip %d", i);
    tab[0 * n + i] = logits[i]; tab[1 * n + i] = target[i]; tab[2 * n + i] = dlogits ? dlogits[i] : nullptr;
  }
  std::memcpy(&tab[3 * n], lens, n * 4);                       // 4th table doubles as the lens array
  HIPCHK(hipMemcpyAsync(d, tab, 4 * n * sizeof(void*), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(sc.ev, s));
  sc.busy = true;
  launch_oad_loss((const float* const*)d, (const float* const*)(d + n), (const int*)(d + 3 * n), n_clips, n_classes,
                  loss_out, dlogits ? (float* const*)(d + 2 * n) : nullptr, grad_scale, s, reduction == 1);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

struct BwdLayout {
  size_t total;
  size_t dLp, dLf, dLt, HRt, WcT, dWc, dHR, carry, dhpart, WhhT, dGI, dGH, dGIop, dGHop, part, T1, T2, WihT, dE, dY, dYb, Hprev, vec, bhx, bsync;
  size_t aG, aFlags, aSpan, aA, aDZ, aPart;        // anticipation head (handles with set_anticipation only; 0 otherwise)
};
static BwdLayout bwd_layout(const prego_miniroad* h, int R, int n_clips) {
  const size_t es = h->bf16 ? 2 : 4;
  const size_t Rp = align_up((size_t)R, 64), H = h->hid, E = h->emb, Din = h->d_rgb + h->d_flow, Cp = 128;
  const size_t Bp = align_up((size_t)n_clips, 16);
  BwdLayout L{};
  size_t off = 0;
  auto put = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
  L.dLp = put((size_t)R * Cp * es); L.dLf = put((size_t)R * Cp * 4); L.dLt = put(Cp * Rp * es);
  L.HRt = put(H * Rp * es); L.WcT = put(H * Cp * es); L.dWc = put(Cp * H * 4);
  L.dHR = put((size_t)R * H * 4);
  L.carry = put(2 * Bp * H * 4); L.dhpart = put(Bp * H * 4);
  L.WhhT = put(H * 3 * H * es);
  L.dGI = put((size_t)R * 3 * H * 4); L.dGH = put((size_t)R * 3 * H * 4);
  L.dGIop = put((size_t)R * 3 * H * es); L.dGHop = put((size_t)R * 3 * H * es);
  L.part = put(std::max<size_t>(((size_t)R / 64 + 1) * 3 * H, ((size_t)R / 4 + 1) * 2 * E) * 4);
  L.T1 = put(std::max<size_t>(3 * H, E) * Rp * es);           // transposed "A" operand of a wgrad (dGIt / dGHt / dYt)
  L.T2 = put(std::max<size_t>(std::max<size_t>(E, H), Din) * Rp * es);   // transposed "B" operand (Et / Hprev_t / Xt)
  L.WihT = put(std::max(E, H) * 3 * H * es);
  L.dE = put((size_t)R * E * 4); L.dY = put((size_t)R * E * 4);
  L.dYb = put(Rp * E * 2);                                      // bf16 copy of dY: k-major A operand of layer1's wgrad
  L.Hprev = put((size_t)R * H * es);
  L.vec = put(4 * E * 4);
  L.bhx = put(gru_bptt_hx_bytes(h->bf16, h->hid, h->G)); L.bsync = put(1024 * 4);     // persistent BPTT: exchange buffers, step counters
  if (h->ant_len > 0) {
    // MiniROADA: packed anticipation gradient G [R][L C] fp32, row flags, the row span, A_l and dZ_l [R][L H] (operand type), and the L
    // partial sums of d relu(h) [L][R][H].  Sized for the whole range: the span is known on the device only
    const size_t Lh = h->ant_len;
    L.aG = put((size_t)R * Lh * h->ncls * 4); L.aFlags = put((size_t)R * 4); L.aSpan = put(64);
    L.aA = put((size_t)R * Lh * H * es); L.aDZ = put((size_t)R * Lh * H * es);
    L.aPart = put(Lh > 1 ? Lh * R * H * 4 : 4);
  }
  L.total = off;
  return L;
}

extern "C" int prego_miniroad_set_gru_layer_grads(prego_miniroad* h, int layer, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (layer != 1 || h->layers != 2) return prego_fail_(PREGO_EINVAL, "set_gru_layer_grads: layer %d of a %d-layer handle (layer 0's gradients are prego_miniroad_backward's own arguments)", layer, h->layers);
  if (!g_w_ih || !g_w_hh || !g_b_ih || !g_b_hh) return prego_fail_(PREGO_EINVAL, "set_gru_layer_grads: NULL tensor");
  h->g_l2[0] = g_w_ih; h->g_l2[1] = g_w_hh; h->g_l2[2] = g_b_ih; h->g_l2[3] = g_b_hh;
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
static bool g_ant_full_span = false;     // prego_debug_ant_full_span: the head's backward runs over every packed row (A/B against the span)
extern "C" int prego_debug_ant_full_span(int on) { g_ant_full_span = on != 0; return PREGO_OK; }
#else
static constexpr bool g_ant_full_span = false;
#endif

extern "C" int prego_miniroad_set_anticipation_grads(prego_miniroad* h, const float* const* d_ant, float* g_w_a, float* g_b_a) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (h->ant_len <= 0) return prego_fail_(PREGO_EINVAL, "set_anticipation_grads before set_anticipation");
  if (!g_w_a || !g_b_a) return prego_fail_(PREGO_EINVAL, "set_anticipation_grads: NULL gradient tensor");
  if (!h->ant_kept || h->kept_rows == 0)
    return prego_fail_(PREGO_EINVAL, "set_anticipation_grads must follow a forward_anticipation with PREGO_FWD_KEEP");
  h->ant_d.clear();
  if (d_ant) h->ant_d.assign(d_ant, d_ant + h->plan_lens.size());
  h->ant_g_w = g_w_a; h->ant_g_b = g_b_a; h->ant_grads_set = true;
  return PREGO_OK;
}

extern "C" int prego_miniroad_backward_events(prego_miniroad* h, void* ev_head_done, void* ev_gru_done) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  h->bwd_ev[0] = (hipEvent_t)ev_head_done;
  h->bwd_ev[1] = (hipEvent_t)ev_gru_done;
  return PREGO_OK;
}

extern "C" int prego_miniroad_backward_callback(prego_miniroad* h, prego_bucket_fn fn, void* user) {
  HandleScope scope_(h);
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  h->bwd_cb = fn;
  h->bwd_cb_user = user;
  return PREGO_OK;
}

extern "C" size_t prego_miniroad_backward_workspace_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens) {
  if (!h || n_clips <= 0 || !lens) return 0;
  long long total = 0;
  for (int i = 0; i < n_clips; ++i) total += lens[i];
  return bwd_layout(h, (int)total, n_clips).total;
}

static void gemm_nt(const prego_miniroad* h, const void* A, int lda, const void* B, int ldb, const float* bias, float* C,
                    int ldc, int M, int N, int K, hipStream_t s) {
  if (h->bf16) launch_gemm_bf16_nt(A, lda, B, ldb, bias, C, ldc, M, N, K, s);
  else launch_gemm_f32_nt((const float*)A, lda, (const float*)B, ldb, bias, C, ldc, M, N, K, s);
}

extern "C" int prego_miniroad_backward(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* dlogits,
                                       float* g_layer1_w, float* g_layer1_b, float* g_ln_w, float* g_ln_b, float* g_w_ih,
                                       float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_fc_w, float* g_fc_b,
                                       void* fwd_workspace, size_t fwd_bytes, void* bwd_workspace, size_t bwd_bytes,
                                       prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !lens || !dlogits || !fwd_workspace || !bwd_workspace) return prego_fail_(PREGO_EINVAL, "backward: NULL argument");
  if (!g_layer1_w || !g_layer1_b || !g_ln_w || !g_ln_b || !g_w_ih || !g_w_hh || !g_b_ih || !g_b_hh || !g_fc_w || !g_fc_b)
    return prego_fail_(PREGO_EINVAL, "backward: NULL gradient tensor");
  if (h->f16 || h->x2) return prego_fail_(PREGO_EINVAL, "backward on an fp16 / fp16x2-operand handle: training runs on bf16 / fp32 handles");
  if ((int)h->plan_lens.size() != n_clips || !std::equal(lens, lens + n_clips, h->plan_lens.begin()) || h->kept_rows == 0)
    return prego_fail_(PREGO_EINVAL, "backward must follow a forward(PREGO_FWD_KEEP) of the same clips");
  hipStream_t s = (hipStream_t)stream;
  const bool bf = h->bf16;
  const size_t es = bf ? 2 : 4;
  const int H = h->hid, E = h->emb, C = h->ncls, Cp = 128, din = h->d_rgb + h->d_flow, kx = h->kept_kx;
  const int R = h->h_rowoff[h->t_max];
  const int Rp = (int)align_up((size_t)R, 64);
  // the activations the forward kept (fwd_layout: the same offsets the PREGO_FWD_KEEP forward wrote them at)
  const FwdLayout F = fwd_layout(h, kx > h->d_rgb, PREGO_FWD_KEEP, fwd_bytes);
  if (F.cap_rows < R) return prego_fail_(PREGO_EWORKSPACE, "forward workspace does not hold the kept activations");
  if (h->layers == 2 && (!h->g_l2[0] || !h->g_l2[1] || !h->g_l2[2] || !h->g_l2[3]))
    return prego_fail_(PREGO_EINVAL, "backward of a 2-layer handle before prego_miniroad_set_gru_layer_grads(1, ...)");
  void* X = fwd_workspace;
  float* Y = (float*)F.at(fwd_workspace, F.Y);
  void* Eb = F.at(fwd_workspace, F.E);
  void* HR = F.at(fwd_workspace, F.HR);
  float* HRAW = (float*)F.at(fwd_workspace, F.HRAW);
  float* KR = (float*)F.at(fwd_workspace, F.KR); float* KZ = (float*)F.at(fwd_workspace, F.KZ);
  float* KN = (float*)F.at(fwd_workspace, F.KN); float* KG = (float*)F.at(fwd_workspace, F.KG);
  float* STATS = (float*)F.at(fwd_workspace, F.STATS);
  void* HR0 = F.at(fwd_workspace, F.HR0); float* HRAW2 = (float*)F.at(fwd_workspace, F.HRAW2);      // NULL on a one-layer handle
  float* KR2 = (float*)F.at(fwd_workspace, F.KR2); float* KZ2 = (float*)F.at(fwd_workspace, F.KZ2);
  float* KN2 = (float*)F.at(fwd_workspace, F.KN2); float* KG2 = (float*)F.at(fwd_workspace, F.KG2);
  if (h->ant_kept && !h->ant_grads_set)
    return prego_fail_(PREGO_EINVAL, "backward after a MiniROADA training forward (forward_anticipation, PREGO_FWD_KEEP) needs "
                              "prego_miniroad_set_anticipation_grads first");
  const bool ant = h->ant_kept;                       // the head's terms join this backward
  const bool ant_dense = ant && !h->ant_d.empty();    // ... with a non-zero anticipation gradient
  struct AntConsume { prego_miniroad* h; ~AntConsume() { h->ant_grads_set = false; h->ant_d.clear(); } } ant_consume{h};   // one call only
  const BwdLayout L = bwd_layout(h, R, n_clips);
  if (bwd_bytes < L.total) return prego_fail_(PREGO_EWORKSPACE, "backward workspace %zu < %zu", bwd_bytes, L.total);
  char* bw = (char*)bwd_workspace;
  float* part = (float*)(bw + L.part);

  // dlogits pointer table
  const int MC = max_clips_of(h);
  std::vector<const void*> tab((size_t)(ant_dense ? 2 : 1) * MC, nullptr);
  for (int i = 0; i < n_clips; ++i) { if (!dlogits[i]) return prego_fail_(PREGO_EINVAL, "dlogits[%d] is NULL", i); tab[i] = dlogits[i]; }
  for (int i = 0; ant_dense && i < n_clips; ++i) {
    if (!h->ant_d[i]) return prego_fail_(PREGO_EINVAL, "d_ant[%d] is NULL", i);
    tab[MC + i] = h->ant_d[i];
  }
  { const int rc = stage_tables(h, tab.data(), tab.size(), s); if (rc) return rc; }
  const float* const* d_dl = (const float* const*)h->d_ptrs;

  // ---- head: logits = relu(h) Wc^T + bc  (rnn.py:62-64)
  // bf16 handles (round 4): every wgrad / dgrad below runs on the k-major GEMM (gemm_tn.hip: operands staged as they lie in memory,
  // fragments read transposed from LDS, the bias gradient as one more MFMA per k-step) - no transposed copy of any activation or
  // weight, no separate column-sum launches.  K of a wgrad = the packed rows, padded to 64 by reading zeros (k_valid = R).
  // fp32 handles keep the transpose + NT-GEMM + two-stage column-sum path (exact-fp32 MFMA, fixed-order fp32 sums).
  const bool tn = bf;
  launch_gather_dlogits(bf, d_dl, h->d_rowoff, h->d_sorted, h->t_max, R, C, Cp, bw + L.dLp, s);
  if (tn) {
    // dWc [C][H] = dL^T . relu(h), db_c = colsum(dL): straight into the caller's gradient tensors
    if (launch_gemm_bf16_tn(true, true, bw + L.dLp, Cp, HR, H, nullptr, g_fc_w, H, C, H, Rp, R, g_fc_b, s)) return prego_fail_(PREGO_EINVAL, "backward: head wgrad shape");
  } else {
    launch_gather_dlogits(false, d_dl, h->d_rowoff, h->d_sorted, h->t_max, R, C, Cp, bw + L.dLf, s);
    launch_colsum((const float*)(bw + L.dLf), R, Cp, part, (float*)(bw + L.vec), s);
    HIPCHK(hipMemcpyAsync(g_fc_b, bw + L.vec, (size_t)C * 4, hipMemcpyDeviceToDevice, s));
    launch_transpose_convert(bf, bf, bw + L.dLp, R, Cp, Cp, bw + L.dLt, Rp, s);            // [Cp][Rp]
    launch_transpose_convert(bf, bf, HR, R, H, H, bw + L.HRt, Rp, s);                       // [H][Rp]
    gemm_nt(h, bw + L.dLt, Rp, bw + L.HRt, Rp, nullptr, (float*)(bw + L.dWc), H, Cp, H, Rp, s);   // dWc[Cp][H]
    HIPCHK(hipMemcpyAsync(g_fc_w, bw + L.dWc, (size_t)C * H * 4, hipMemcpyDeviceToDevice, s));
  }
  // ---- MiniROADA's anticipation head (ant_head_bwd.hip): its f_classification terms join the trunk's above, anticipation_layer's
  // gradients are written whole, d relu(h) gets its share below; every product touches only the device-side span of rows with gradient
  const int* a_span = (const int*)(bw + L.aSpan);
  if (ant_dense) {
    const int La = h->ant_len;
    launch_ant_gather((const float* const*)(h->d_ptrs + MC), h->d_rowoff, h->d_sorted, h->t_max, R, La * C, (float*)(bw + L.aG),
                      (int*)(bw + L.aFlags), (int*)(bw + L.aSpan), g_ant_full_span ? 1 : 0, s);
    if (launch_ant_head_store_a(bf, HR, h->w_a, h->b_a, R, H, La, bw + L.aA, a_span, s))
      return prego_fail_(PREGO_EINVAL, "backward: anticipation head shape (hid %d, L %d)", H, La);
    launch_ant_head_wgrad(bf, (const float*)(bw + L.aG), HR, h->w_c, R, H, La, C, a_span, bw + L.aA, bw + L.aDZ, g_fc_w, g_fc_b,
                          h->ant_g_w, h->ant_g_b, s);
  } else if (ant) {                                  // zero anticipation gradient: nothing of the head's backward runs
    HIPCHK(hipMemsetAsync(h->ant_g_w, 0, (size_t)h->ant_len * H * H * 4, s));
    HIPCHK(hipMemsetAsync(h->ant_g_b, 0, (size_t)h->ant_len * H * 4, s));
  }
  if (h->bwd_ev[0]) HIPCHK(hipEventRecord(h->bwd_ev[0], s));            // f_classification (and anticipation_layer) gradients are final
  if (h->bwd_cb) h->bwd_cb(h->bwd_cb_user, 0);
  if (tn) {
    // d relu(h) [R][H] = dL [R][Cp] . Wc [ncls_pad][H]: the weight as it is stored ([K][N]); rows >= ncls_pad read as zeros
    if (launch_gemm_bf16_tn(false, true, bw + L.dLp, Cp, h->w_c, H, nullptr, (float*)(bw + L.dHR), H, R, H, Cp, h->ncls_pad, nullptr, s))
      return prego_fail_(PREGO_EINVAL, "backward: head dgrad shape");
  } else {
    launch_transpose_convert(bf, bf, h->w_c, h->ncls_pad, H, H, bw + L.WcT, Cp, s);        // [H][Cp] (rows >= ncls_pad zero)
    gemm_nt(h, bw + L.dLp, Cp, bw + L.WcT, Cp, nullptr, (float*)(bw + L.dHR), H, R, H, Cp, s);    // d relu(h)
  }
  if (ant_dense)                                     // d relu(h) += sum_l dZ_l W_a[l] over the span's rows
    launch_ant_head_dgrad(bf, h->w_a, R, H, h->ant_len, a_span, bw + L.aDZ, (float*)(bw + L.aPart), (float*)(bw + L.dHR), s);
  launch_relu_mask((const float*)(bw + L.dHR), h->layers == 2 ? HRAW2 : HRAW, (size_t)R * H, (float*)(bw + L.dHR), s);   // the head reads the LAST layer's relu(h)

  // ---- BPTT through the GRU (rnn.py:61), reverse time; a stacked GRU (num_layers 2, rnn.py:32,38) runs its layers last to first:
  // layer 1 from the head's gradient, then dH0 = dGI1 . W_ih_l1 (no relu between the layers), then layer 0 from that
  const size_t Bp = align_up((size_t)n_clips, 16);
  for (int layer = h->layers - 1; layer >= 0; --layer) {
  const void* L_whh = layer == 1 ? h->l2_w_hh : h->w_hh;
  const void* L_wih = layer == 1 ? h->l2_w_ih : h->w_ih;
  const void* L_in = layer == 1 ? HR0 : Eb;                  // the layer's input rows (operand type)
  const int L_k = layer == 1 ? H : E;                        // ... and their width
  float* L_hraw = layer == 1 ? HRAW2 : HRAW;
  float* L_kr = layer == 1 ? KR2 : KR; float* L_kz = layer == 1 ? KZ2 : KZ; float* L_kn = layer == 1 ? KN2 : KN; float* L_kg = layer == 1 ? KG2 : KG;
  float* L_gwih = layer == 1 ? h->g_l2[0] : g_w_ih; float* L_gwhh = layer == 1 ? h->g_l2[1] : g_w_hh;
  float* L_gbih = layer == 1 ? h->g_l2[2] : g_b_ih; float* L_gbhh = layer == 1 ? h->g_l2[3] : g_b_hh;
  const bool last_layer = layer == 0;
  launch_transpose_convert(bf, bf, L_whh, 3 * H, H, H, bw + L.WhhT, 3 * H, s);          // [H][3H]
  float* carry[2] = {(float*)(bw + L.carry), (float*)(bw + L.carry) + Bp * H};
  float* dhpart = (float*)(bw + L.dhpart);
  // one persistent launch (gru_bptt.hip); the step-by-step loop below is the fallback for shapes it does not take and the
  // A/B reference (PREGO_BPTT_STEPWISE=1)
  bool persistent = false;
  {
    static const bool stepwise = prego_tune_env("PREGO_BPTT_STEPWISE") != nullptr;
    const int slots = (h->n_slots + h->G - 1) / h->G;
    const int nct = (slots + 15) / 16;
    if (!stepwise) {
      BpttArgs ba;
      ba.whhT = bw + L.WhhT; ba.dHout = (const float*)(bw + L.dHR); ba.R = L_kr; ba.Z = L_kz; ba.N = L_kn; ba.GHN = L_kg; ba.Hraw = L_hraw;
      // the fp32 copies of dGI / dGH are read by the exact-fp32 path only (column sums, transposes): a bf16 handle's k-major GEMMs take
      // the operand copies, so its BPTT kernel does not store them at all
      ba.dGI = tn ? nullptr : (float*)(bw + L.dGI); ba.dGH = tn ? nullptr : (float*)(bw + L.dGH); ba.dGIop = bw + L.dGIop; ba.dGHop = bw + L.dGHop;
      ba.hx = bw + L.bhx; ba.sync = (unsigned*)(bw + L.bsync); ba.abort_word = h->abort_word;
      ba.rowoff = h->d_rowoff; ba.nact = h->d_nact; ba.t_max = h->t_max; ba.n_clips = h->n_slots; ba.G = h->G;
      ba.force_sc1 = h->no_local ? 1 : 0;
      persistent = launch_gru_bptt(bf, H, nct, ba, s) == 0;
    }
  }
  for (int t = h->t_max - 1; t >= 0 && !persistent; --t) {
    const int na = h->h_nact[t];
    const int na_next = t + 1 < h->t_max ? h->h_nact[t + 1] : 0;
    const int row_t = h->h_rowoff[t], row_tm1 = t > 0 ? h->h_rowoff[t - 1] : 0;
    launch_gru_bwd_step(bf, t, na, na_next, row_t, row_tm1, H, (const float*)(bw + L.dHR), carry[(t + 1) & 1], dhpart, L_kr,
                        L_kz, L_kn, L_kg, L_hraw, carry[t & 1], (float*)(bw + L.dGI), (float*)(bw + L.dGH), bw + L.dGIop,
                        bw + L.dGHop, s);
    if (t > 0)   // dh_{t-1} += dgh_t . W_hh
      gemm_nt(h, bw + L.dGHop + (size_t)row_t * 3 * H * es, 3 * H, bw + L.WhhT, 3 * H, nullptr, dhpart, H, na, H, 3 * H, s);
  }
  launch_build_hprev(bf, L_hraw, h->d_rowoff, h->t_max, R, H, bw + L.Hprev, s);
  if (tn) {
    // dW_ih = dGI^T . e (+ db_ih), dW_hh = dGH^T . h_{t-1} (+ db_hh): bias sums from the bf16 operand copies the BPTT kernel wrote
    if (launch_gemm_bf16_tn(true, true, bw + L.dGIop, 3 * H, L_in, L_k, nullptr, L_gwih, L_k, 3 * H, L_k, Rp, R, L_gbih, s) ||
        launch_gemm_bf16_tn(true, true, bw + L.dGHop, 3 * H, bw + L.Hprev, H, nullptr, L_gwhh, H, 3 * H, H, Rp, R, L_gbhh, s))
      return prego_fail_(PREGO_EINVAL, "backward: GRU wgrad shape");
  } else {
    // biases of the GRU
    launch_colsum((const float*)(bw + L.dGI), R, 3 * H, part, L_gbih, s);
    launch_colsum((const float*)(bw + L.dGH), R, 3 * H, part, L_gbhh, s);
    // dW_ih = dGI^T . e
    launch_transpose_convert(bf, bf, bw + L.dGIop, R, 3 * H, 3 * H, bw + L.T1, Rp, s);
    launch_transpose_convert(bf, bf, L_in, R, L_k, L_k, bw + L.T2, Rp, s);
    gemm_nt(h, bw + L.T1, Rp, bw + L.T2, Rp, nullptr, L_gwih, L_k, 3 * H, L_k, Rp, s);
    // dW_hh = dGH^T . h_{t-1}
    launch_transpose_convert(bf, bf, bw + L.dGHop, R, 3 * H, 3 * H, bw + L.T1, Rp, s);
    launch_transpose_convert(bf, bf, bw + L.Hprev, R, H, H, bw + L.T2, Rp, s);
    gemm_nt(h, bw + L.T1, Rp, bw + L.T2, Rp, nullptr, L_gwhh, H, 3 * H, H, Rp, s);
  }
  if (last_layer) {
    if (h->bwd_ev[1]) HIPCHK(hipEventRecord(h->bwd_ev[1], s));          // every GRU gradient is final (layer1 / LayerNorm follow)
    if (h->bwd_cb) h->bwd_cb(h->bwd_cb_user, 1);
  }
  // gradient of the layer's input = dGI . W_ih: d e for layer 0 (LayerNorm's output), dH0 - the next BPTT's dHout, as it is - for layer 1
  float* L_din = last_layer ? (float*)(bw + L.dE) : (float*)(bw + L.dHR);
  if (tn) {
    if (launch_gemm_bf16_tn(false, true, bw + L.dGIop, 3 * H, L_wih, L_k, nullptr, L_din, L_k, R, L_k, 3 * H, 3 * H, nullptr, s))
      return prego_fail_(PREGO_EINVAL, "backward: W_ih dgrad shape");
  } else {
    launch_transpose_convert(bf, bf, L_wih, 3 * H, L_k, L_k, bw + L.WihT, 3 * H, s);        // [K][3H]
    gemm_nt(h, bw + L.dGIop, 3 * H, bw + L.WihT, 3 * H, nullptr, L_din, L_k, R, L_k, 3 * H, s);
  }
  }   // layers, last to first

  // ---- Dropout / ReLU / LayerNorm backward (rnn.py:41-43)
  const int nb = launch_ln_relu_bwd((const float*)(bw + L.dE), Y, STATS, h->ln_g, h->ln_b, R, E, h->drop_p, h->drop_seed, 0,
                                    (float*)(bw + L.dY), part, s, 1, 0, tn ? (void*)(bw + L.dYb) : nullptr);
  // d gamma | d beta: the stage-2 sum goes straight into the caller's two tensors when they are adjacent (the flat gradient bucket
  // of prego_amd/engine.py), through a scratch vector and two copies otherwise
  if (g_ln_b == g_ln_w + E) launch_colsum_stage2(part, nb, 2 * E, g_ln_w, s);
  else {
    launch_colsum_stage2(part, nb, 2 * E, (float*)(bw + L.vec), s);
    HIPCHK(hipMemcpyAsync(g_ln_w, bw + L.vec, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(g_ln_b, bw + L.vec + (size_t)E * 4, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
  }

  // ---- layer1 Linear (rnn.py:40): db = colsum(dY), dW = dY^T . x
  if (kx < din) HIPCHK(hipMemsetAsync(g_layer1_w, 0, (size_t)E * din * 4, s));          // zero-flow columns: zero gradient
  if (tn) {
    if (launch_gemm_bf16_tn(true, true, bw + L.dYb, E, X, kx, nullptr, g_layer1_w, din, E, kx, Rp, R, g_layer1_b, s))
      return prego_fail_(PREGO_EINVAL, "backward: layer1 wgrad shape");
  } else {
    launch_colsum((const float*)(bw + L.dY), R, E, part, g_layer1_b, s);
    launch_transpose_convert(false, bf, bw + L.dY, R, E, E, bw + L.T1, Rp, s);
    launch_transpose_convert(bf, bf, X, R, kx, kx, bw + L.T2, Rp, s);
    gemm_nt(h, bw + L.T1, Rp, bw + L.T2, Rp, nullptr, g_layer1_w, din, E, kx, Rp, s);
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}


// ================================================================================================
// optimizer: torch.optim.AdamW of main.py:62-67 on the ABI
// ================================================================================================
extern "C" int prego_adamw_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                float* const* exp_avg_sq, const int64_t* numel, int64_t step, float lr, float beta1, float beta2,
                                float eps, float weight_decay, prego_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel) return prego_fail_(PREGO_EINVAL, "adamw: NULL argument");
  std::vector<long long> n(numel, numel + std::max(n_tensors, 0));
  if (launch_adamw(n_tensors, params, grads, exp_avg, exp_avg_sq, nullptr, n.data(), false, step, lr, beta1, beta2, eps, weight_decay,
                   (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "adamw: bad tensor list (n = %d, step = %lld)", n_tensors, (long long)step);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// The same step for the ten MiniROAD tensors (prego_miniroad_set_weights' order) that ALSO refreshes the handle's operand copies
// (bf16 / fp32 weights, padded classifier, folded GRU biases) in the same pass: no set_weights call after the step.
extern "C" int prego_miniroad_adamw_step(prego_miniroad* h, float* const* params, const float* const* grads, float* const* exp_avg,
                                         float* const* exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float eps,
                                         float weight_decay, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !params || !grads || !exp_avg || !exp_avg_sq) return prego_fail_(PREGO_EINVAL, "adamw: NULL argument");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "adamw step before set_weights");
  if (h->f16 || h->x2) return prego_fail_(PREGO_EINVAL, "adamw step on an fp16 / fp16x2-operand handle: training runs on bf16 / fp32 handles");
  hipStream_t s = (hipStream_t)stream;
  const long long din = h->d_rgb + h->d_flow, E = h->emb, H = h->hid, C = h->ncls;
  // set_weights order: layer1.0.weight, layer1.0.bias, layer1.1.weight, layer1.1.bias, w_ih, w_hh, b_ih, b_hh, fc.weight, fc.bias
  const long long numel[10] = {E * din, E, E, E, 3 * H * E, 3 * H * H, 3 * H, 3 * H, C * H, C};
  // operand-typed copies (weights) first, fp32 copies (biases, LayerNorm) second: two launches, one element type each
  float* pw[4] = {params[0], params[4], params[5], params[8]};
  const float* gw[4] = {grads[0], grads[4], grads[5], grads[8]};
  float* mw[4] = {exp_avg[0], exp_avg[4], exp_avg[5], exp_avg[8]};
  float* vw[4] = {exp_avg_sq[0], exp_avg_sq[4], exp_avg_sq[5], exp_avg_sq[8]};
  void* cw[4] = {h->w1, h->w_ih, h->w_hh, h->w_c};            // w_c: rows >= n_classes stay zero (same linear index below them)
  const long long nw[4] = {numel[0], numel[4], numel[5], numel[8]};
  float* pb[6] = {params[1], params[2], params[3], params[6], params[7], params[9]};
  const float* gb[6] = {grads[1], grads[2], grads[3], grads[6], grads[7], grads[9]};
  float* mb[6] = {exp_avg[1], exp_avg[2], exp_avg[3], exp_avg[6], exp_avg[7], exp_avg[9]};
  float* vb[6] = {exp_avg_sq[1], exp_avg_sq[2], exp_avg_sq[3], exp_avg_sq[6], exp_avg_sq[7], exp_avg_sq[9]};
  void* cb[6] = {h->b1, h->ln_g, h->ln_b, nullptr, nullptr, h->b_c};
  const long long nb[6] = {numel[1], numel[2], numel[3], numel[6], numel[7], numel[9]};
  for (int i = 0; i < 10; ++i) if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) return prego_fail_(PREGO_EINVAL, "adamw: tensor %d is NULL", i);
  // guarded by the handle's timeout word: after a forward / backward that gave up, the step changes nothing (the add / copy below then
  // rebuild the same derived vectors from the unchanged biases)
  if (launch_adamw(4, pw, gw, mw, vw, cw, nw, h->bf16, step, lr, beta1, beta2, eps, weight_decay, s, h->abort_word, h->peer_guard) ||
      launch_adamw(6, pb, gb, mb, vb, cb, nb, false, step, lr, beta1, beta2, eps, weight_decay, s, h->abort_word, h->peer_guard))
    return prego_fail_(PREGO_EINVAL, "adamw: bad step %lld", (long long)step);
  launch_add_vec(params[6], params[7], h->bias2, (int)(3 * H), (int)(2 * H), s);      // r,z rows: b_ih + b_hh ; n rows: b_ih
  h->perm_stale = true;
  HIPCHK(hipMemcpyAsync(h->b_hn, params[7] + 2 * H, (size_t)H * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// The same step for MiniROADA's anticipation_layer.0.{weight, bias} (params[0] [L H, H], params[1] [L H]), rewriting the handle's W_a operand
// copy and its bias in the same pass; guarded by the same timeout word and peer guard as prego_miniroad_adamw_step.
extern "C" int prego_miniroad_adamw_step_anticipation(prego_miniroad* h, float* const* params, const float* const* grads, float* const* exp_avg,
                                                      float* const* exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float eps,
                                                      float weight_decay, prego_stream_t stream) {
  HandleScope scope_(h);
  if (!h || !params || !grads || !exp_avg || !exp_avg_sq) return prego_fail_(PREGO_EINVAL, "adamw (anticipation): NULL argument");
  if (h->ant_len <= 0 || !h->w_a) return prego_fail_(PREGO_EINVAL, "adamw (anticipation) before set_anticipation");
  if (h->f16 || h->x2) return prego_fail_(PREGO_EINVAL, "adamw step on an fp16 / fp16x2-operand handle: training runs on bf16 / fp32 handles");
  for (int i = 0; i < 2; ++i) if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) return prego_fail_(PREGO_EINVAL, "adamw (anticipation): tensor %d is NULL", i);
  hipStream_t s = (hipStream_t)stream;
  const long long LH = (long long)h->ant_len * h->hid;
  float* pw[1] = {params[0]}; const float* gw[1] = {grads[0]}; float* mw[1] = {exp_avg[0]}; float* vw[1] = {exp_avg_sq[0]};
  void* cw[1] = {h->w_a}; const long long nw[1] = {LH * h->hid};
  float* pb[1] = {params[1]}; const float* gb[1] = {grads[1]}; float* mb[1] = {exp_avg[1]}; float* vb[1] = {exp_avg_sq[1]};
  void* cb[1] = {h->b_a}; const long long nb[1] = {LH};
  if (launch_adamw(1, pw, gw, mw, vw, cw, nw, h->bf16, step, lr, beta1, beta2, eps, weight_decay, s, h->abort_word, h->peer_guard) ||
      launch_adamw(1, pb, gb, mb, vb, cb, nb, false, step, lr, beta1, beta2, eps, weight_decay, s, h->abort_word, h->peer_guard))
    return prego_fail_(PREGO_EINVAL, "adamw (anticipation): bad step %lld", (long long)step);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

