// C ABI of the causal AttentionLayer op (include/prego_amd.h): AttentionLayer(FullAttention(mask_flag)) of attn.py:139-170,35-57 as a
// stateless call, as a handle that keeps its converted weights, and the handle's training forward / backward.
#include "vit_handle.h"      // the layouts, epi_qkv, drop_thresh / drop_scale, refuse_non_bf16, wgrad / dgrad

// ---- layouts -----------------------------------------------------------------------------------------------------------------------
static AttnAct attn_act(Arena& a, size_t M, size_t D) {
  AttnAct t{};
  t.xb = a.put(M * D * 2); t.q = a.put(M * D * 2); t.k = a.put(M * D * 2); t.vn = a.put(M * D * 2); t.ao = a.put(M * D * 2);
  return t;
}
AttnWs attn_ws(int d_model, int batch, int len, bool f32, Arena a) {
  const size_t M = (size_t)batch * len, D = d_model;
  AttnWs w{};
  if (f32) { w.qkv32 = a.put(3 * align_up(M * D * 4, 256)); w.ao32 = a.put(M * D * 4); }
  else w.act = attn_act(a, M, D);
  w.total = a.off;
  return w;
}
AttnTrainWs attn_train_ws(int d_model, int heads, int batch, int len, Arena a) {
  const size_t M = (size_t)batch * len, D = d_model;
  AttnTrainWs w{};
  w.Mp = (int)align_up(M, 64);
  w.act = attn_act(a, M, D); w.lse = a.put((size_t)batch * heads * len * 4);
  w.dyb = a.put(M * D * 2); w.dO = a.put(M * D * 2); w.dqkv = a.put(M * 3 * D * 2); w.delta = a.put((size_t)batch * heads * len * 4);
  w.dW = a.put(3 * D * D * 4); w.vec = a.put(3 * D * 4);
  w.total = a.off;
  return w;
}
AttnOpWs attn_op_ws(int d_model, int batch, int len, Arena a) {
  const size_t M = (size_t)batch * len, D = d_model;
  AttnOpWs w{};
  w.wqkv = a.put(3 * D * D * 2); w.bqkv = a.put(3 * D * 4); w.wo = a.put(D * D * 2);
  w.act = attn_act(a, M, D);
  w.total = a.off;
  return w;
}

// the attention arithmetic shared by the stateless op and the handle: wqkv bf16 [3D][D] (rows q | k | v), bqkv fp32 [3D],
// wob bf16 [D][D]; t: the five activation buffers inside ws
static int attention_layer_run(int batch, int len, int d_model, int heads, int causal, const float* x, const void* wqkv,
                               const float* bqkv, const void* wob, const float* bo, float* out, char* ws, const AttnAct& t, hipStream_t s,
                               bool f16 = false, float* lse = nullptr, unsigned drop_thr = 0, float drop_sc = 1.f, unsigned long long drop_seed = 0) {
  const int M = batch * len, dh = d_model / heads;
  launch_cat_convert(x, nullptr, M, d_model, 0, ws + t.xb, s, f16);
  const GemmEpi e = epi_qkv(f16, ws + t.q, ws + t.k, ws + t.vn, len, heads, dh, d_model);
  launch_gemm_bf16_nt_epi(ws + t.xb, d_model, wqkv, d_model, bqkv, nullptr, 0, M, 3 * d_model, d_model, e, s);
  if (launch_flash_attention_v2(ws + t.q, ws + t.k, ws + t.vn, ws + t.ao, batch, len, len, heads, dh, causal ? 1 : 0, s, lse, drop_thr, drop_sc,
                                drop_seed, f16))
    return -1;
  launch_gemm_bf16_nt(ws + t.ao, d_model, wob, d_model, bo, out, d_model, M, d_model, d_model, s, f16);
  return 0;
}
static int attention_layer_check(int d_model, int heads) {
  if (d_model % 128 || heads <= 0 || d_model % heads) return prego_fail_(PREGO_EINVAL, "d_model %d / heads %d", d_model, heads);
  const int dh = d_model / heads;
  if (dh != 64 && dh != 128 && dh != 256) return prego_fail_(PREGO_EINVAL, "head dim %d: supported 64, 128, 256", dh);
  return 0;
}
// The q | k | v weights [D][D] and biases [D] into one operand, and the output projection's weight: converted to 16 bits (w16, wo16) or,
// with w32 given, copied as fp32 (w32, wo32); bqkv fp32 [3D].  The four weights first, then the three biases
static int pack_qkv(int d, const float* wq, const float* wk, const float* wv, const float* wo, const float* bq, const float* bk,
                    const float* bv, void* w16, void* wo16, float* w32, float* wo32, float* bqkv, bool f16, hipStream_t s) {
  const size_t D = d, DD = D * D;
  const float* w[4] = {wq, wk, wv, wo};
  const float* b[3] = {bq, bk, bv};
  for (int j = 0; j < 4; ++j) {
    if (w32) HIPCHK(hipMemcpyAsync(j < 3 ? w32 + j * DD : wo32, w[j], DD * 4, hipMemcpyDeviceToDevice, s));
    else launch_pad_convert(true, w[j], d, d, d, j < 3 ? (char*)w16 + j * DD * 2 : (char*)wo16, d, d, s, f16);
  }
  for (int j = 0; j < 3; ++j) HIPCHK(hipMemcpyAsync(bqkv + j * D, b[j], D * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// handle form: the four projection weights are converted to bf16 ONCE (set_weights), not on every call
struct prego_attn_layer {
  int d_model, heads;
  void* wqkv = nullptr; float* bqkv = nullptr; void* wo = nullptr; float* bo = nullptr;
  bool have_weights = false;
  bool f16 = false;                // IEEE fp16 operands instead of bf16 (prego_attention_layer_set_compute_dtype)
  bool f32 = false;                // fp32 operands (parity mode): wqkv32 [3D][D], wo32 [D][D]
  float* wqkv32 = nullptr; float* wo32 = nullptr;
  // FullAttention's nn.Dropout(attention_dropout) on A = softmax(scale * scores) (attn.py:39,54), training entry points only: a stateless hash
  // mask of (seed, element of A), the same in forward_train and backward (prego_attention_layer_set_dropout)
  float attn_drop_p = 0.f; unsigned long long drop_seed = 0;
};
extern "C" int prego_attention_layer_set_dropout(prego_attn_layer* h, float p, uint64_t seed) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!(p >= 0.f && p < 1.f)) return prego_fail_(PREGO_EINVAL, "attention_dropout p = %f", (double)p);
  h->attn_drop_p = p;
  h->drop_seed = seed;
  return PREGO_OK;
}
extern "C" int prego_attention_layer_set_compute_dtype(prego_attn_layer* h, int compute_dtype) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (compute_dtype != PREGO_BF16 && compute_dtype != PREGO_F16 && compute_dtype != PREGO_F32)
    return prego_fail_(PREGO_EINVAL, "AttentionLayer compute_dtype %d: PREGO_BF16, PREGO_F16 or PREGO_F32", compute_dtype);
  if ((compute_dtype == PREGO_F16) != h->f16 || (compute_dtype == PREGO_F32) != h->f32) h->have_weights = false;
  h->f16 = compute_dtype == PREGO_F16;
  h->f32 = compute_dtype == PREGO_F32;
  if (h->f32 && !h->wqkv32) {
    const size_t D = h->d_model;
    hipError_t e = hipMalloc((void**)&h->wqkv32, 3 * D * D * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->wo32, D * D * 4);
    if (e != hipSuccess) { h->f32 = false; return prego_fail_(PREGO_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
  }
  return PREGO_OK;
}
extern "C" int prego_attention_layer_create(prego_attn_layer** out, int d_model, int heads) {
  if (!out) return prego_fail_(PREGO_EINVAL, "out is NULL");
  *out = nullptr;
  if (attention_layer_check(d_model, heads)) return PREGO_EINVAL;
  prego_attn_layer* h = new prego_attn_layer();
  h->d_model = d_model; h->heads = heads;
  const size_t D = d_model;
  hipError_t e = hipMalloc(&h->wqkv, 3 * D * D * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&h->bqkv, 3 * D * 4);
  if (e == hipSuccess) e = hipMalloc(&h->wo, D * D * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&h->bo, D * 4);
  if (e != hipSuccess) { prego_attention_layer_destroy(h); return prego_fail_(PREGO_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
  *out = h;
  return PREGO_OK;
}
extern "C" void prego_attention_layer_destroy(prego_attn_layer* h) {
  if (!h) return;
  for (void* p : {h->wqkv, (void*)h->bqkv, h->wo, (void*)h->bo, (void*)h->wqkv32, (void*)h->wo32}) if (p) (void)hipFree(p);
  delete h;
}
extern "C" int prego_attention_layer_set_weights(prego_attn_layer* h, const float* wq, const float* bq, const float* wk,
                                                 const float* bk, const float* wv, const float* bv, const float* wo,
                                                 const float* bo, prego_stream_t stream) {
  if (!h || !wq || !bq || !wk || !bk || !wv || !bv || !wo || !bo) return prego_fail_(PREGO_EINVAL, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = pack_qkv(h->d_model, wq, wk, wv, wo, bq, bk, bv, h->wqkv, h->wo, h->f32 ? h->wqkv32 : nullptr, h->wo32, h->bqkv, h->f16, s)) return rc;
  HIPCHK(hipMemcpyAsync(h->bo, bo, (size_t)h->d_model * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  h->have_weights = true;
  return PREGO_OK;
}
extern "C" size_t prego_attention_layer_handle_workspace_bytes(const prego_attn_layer* h, int batch, int len) {
  return h ? attn_ws(h->d_model, batch, len, h->f32).total : 0;
}
extern "C" int prego_attention_layer_handle_forward(prego_attn_layer* h, int batch, int len, int causal, const float* x, float* out,
                                                    void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!h || !x || !out || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "forward before set_weights");
  if (batch <= 0 || len <= 0) return prego_fail_(PREGO_EINVAL, "batch %d, len %d", batch, len);
  const AttnWs w = attn_ws(h->d_model, batch, len, h->f32);
  if (workspace_bytes < w.total) return prego_fail_(PREGO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if (h->f32) {                 // attn.py:151-170 with fp32 operands: biased projections on the exact-fp32 GEMM, fp32 attention
    const int D = h->d_model, M = batch * len, dh = D / h->heads;
    float* qkv = (float*)(ws + w.qkv32);
    float* ao = (float*)(ws + w.ao32);
    launch_gemm_f32_nt(x, D, h->wqkv32, D, h->bqkv, qkv, 3 * D, M, 3 * D, D, s);
    if (launch_attention_f32(qkv, 3 * D, 0, D, 2 * D, ao, batch, len, len, h->heads, dh, causal ? 1 : 0, 1.0f / sqrtf((float)dh), s))
      return prego_fail_(PREGO_EINVAL, "attention launch failed");
    launch_gemm_f32_nt(ao, D, h->wo32, D, h->bo, out, D, M, D, D, s);
    HIPCHK(hipGetLastError());
    return PREGO_OK;
  }
  if (attention_layer_run(batch, len, h->d_model, h->heads, causal, x, h->wqkv, h->bqkv, h->wo, h->bo, out, ws, w.act, s, h->f16))
    return prego_fail_(PREGO_EINVAL, "attention launch failed");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// ---- training: forward that keeps q, k, v, the attention output and the row log-sum-exp, and the backward over them --------
// (attn.py:139-170 under autograd: the projections are nn.Linear, the attention FullAttention.forward attn.py:35-57; attention_dropout
// (attn.py:39,54: nn.Dropout on A, active under module.train()) is the handle's prego_attention_layer_set_dropout state, p = 0 by default)
extern "C" size_t prego_attention_layer_train_workspace_bytes(const prego_attn_layer* h, int batch, int len) {
  return (h && batch > 0 && len > 0) ? attn_train_ws(h->d_model, h->heads, batch, len).total : 0;
}
extern "C" int prego_attention_layer_forward_train(prego_attn_layer* h, int batch, int len, int causal, const float* x, float* out,
                                                   void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!h || !x || !out || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (refuse_non_bf16("prego_attention_layer_forward_train", h->f16, h->f32)) return PREGO_EINVAL;
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "forward before set_weights");
  if (batch <= 0 || len <= 0) return prego_fail_(PREGO_EINVAL, "batch %d, len %d", batch, len);
  const AttnTrainWs w = attn_train_ws(h->d_model, h->heads, batch, len);
  if (workspace_bytes < w.total) return prego_fail_(PREGO_EWORKSPACE, "training workspace %zu < %zu", workspace_bytes, w.total);
  char* ws = (char*)workspace;
  if (attention_layer_run(batch, len, h->d_model, h->heads, causal, x, h->wqkv, h->bqkv, h->wo, h->bo, out, ws, w.act, (hipStream_t)stream,
                          false, (float*)(ws + w.lse), drop_thresh(h->attn_drop_p), drop_scale(h->attn_drop_p), h->drop_seed))
    return prego_fail_(PREGO_EINVAL, "attention launch failed");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
// grads: 8 fp32 tensors in set_weights order (wq, bq, wk, bk, wv, bv, wo, bo), overwritten; dx [batch*len, d_model] or NULL
extern "C" int prego_attention_layer_backward(prego_attn_layer* h, int batch, int len, int causal, const float* dout, float* dx,
                                              float* const* grads, int n_tensors, void* workspace, size_t workspace_bytes,
                                              prego_stream_t stream) {
  if (!h || !dout || !grads || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (refuse_non_bf16("prego_attention_layer_backward", h->f16, h->f32)) return PREGO_EINVAL;
  if (n_tensors != 8) return prego_fail_(PREGO_EINVAL, "expected 8 gradient tensors, got %d", n_tensors);
  for (int i = 0; i < 8; ++i) if (!grads[i]) return prego_fail_(PREGO_EINVAL, "gradient tensor %d is NULL", i);
  if (batch <= 0 || len <= 0) return prego_fail_(PREGO_EINVAL, "batch %d, len %d", batch, len);
  const AttnTrainWs w = attn_train_ws(h->d_model, h->heads, batch, len);
  if (workspace_bytes < w.total) return prego_fail_(PREGO_EWORKSPACE, "training workspace %zu < %zu", workspace_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int D = h->d_model, M = batch * len, dh = D / h->heads, Mp = w.Mp;
  const size_t DD = (size_t)D * D;
  const AttnAct& t = w.act;
  float* vec = (float*)(ws + w.vec); float* dW = (float*)(ws + w.dW);
  // ---- out_projection (attn.py:170): d bo, d Wo, d (attention output)
  launch_f32_to_bf16(dout, ws + w.dyb, (size_t)M * D, s);
  if (wgrad(ws + w.dyb, D, ws + t.ao, D, M, Mp, grads[6], grads[7], s) ||                    // d Wo, d bo
      dgrad(ws + w.dyb, D, h->wo, D, M, nullptr, s, ws + w.dO)) return prego_fail_(PREGO_EINVAL, "backward: out_projection GEMM shape");
  // ---- softmax(scale * Q K^T + mask) V (attn.py:41-52)
  if (launch_attention_bwd(ws + t.q, ws + t.k, ws + t.vn, ws + t.ao, ws + w.dO, (const float*)(ws + w.lse), (float*)(ws + w.delta), ws + w.dqkv,
                           batch, len, h->heads, dh, causal ? 1 : 0, 1.0f / sqrtf((float)dh), s, drop_thresh(h->attn_drop_p),
                           drop_scale(h->attn_drop_p), h->drop_seed))
    return prego_fail_(PREGO_EINVAL, "attention backward launch failed");
  // ---- query / key / value projections (attn.py:160-162): rows of dqkv are [dq | dk | dv]
  if (wgrad(ws + w.dqkv, 3 * D, ws + t.xb, D, M, Mp, dW, vec, s)) return prego_fail_(PREGO_EINVAL, "backward: qkv GEMM shape");
  for (int j = 0; j < 3; ++j) {
    HIPCHK(hipMemcpyAsync(grads[2 * j], dW + j * DD, DD * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(grads[2 * j + 1], vec + (size_t)j * D, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
  }
  if (dx) {     // self-attention: queries = keys = values = x, the three input gradients add up = dqkv . Wqkv
    if (dgrad(ws + w.dqkv, 3 * D, h->wqkv, D, M, dx, s)) return prego_fail_(PREGO_EINVAL, "backward: qkv dgrad shape");
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// stateless op (weights passed per call and converted into the workspace first)
extern "C" size_t prego_attention_layer_workspace_bytes(int batch, int len, int d_model) { return attn_op_ws(d_model, batch, len).total; }

extern "C" int prego_attention_layer_forward(int batch, int len, int d_model, int heads, int causal, const float* x,
                                             const float* wq, const float* bq, const float* wk, const float* bk,
                                             const float* wv, const float* bv, const float* wo, const float* bo, float* out,
                                             void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!x || !wq || !bq || !wk || !bk || !wv || !bv || !wo || !bo || !out || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (attention_layer_check(d_model, heads)) return PREGO_EINVAL;
  const AttnOpWs w = attn_op_ws(d_model, batch, len);
  if (workspace_bytes < w.total) return prego_fail_(PREGO_EWORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  if (int rc = pack_qkv(d_model, wq, wk, wv, wo, bq, bk, bv, ws + w.wqkv, ws + w.wo, nullptr, nullptr, (float*)(ws + w.bqkv), false, s)) return rc;
  if (attention_layer_run(batch, len, d_model, heads, causal, x, ws + w.wqkv, (float*)(ws + w.bqkv), ws + w.wo, bo, out, ws, w.act, s))
    return prego_fail_(PREGO_EINVAL, "attention launch failed");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
// debug / unit test: the attention backward kernels alone (tests/test_gpu_vit_train.py)
extern "C" int prego_debug_attention_bwd(int batch, int len, int heads, int dh, int causal, const void* qs, const void* k, const void* v,
                                         const void* o, const void* dout, const float* lse, void* dqkv, prego_stream_t stream) {
  if (!qs || !k || !v || !o || !dout || !lse || !dqkv || batch <= 0 || len <= 0 || heads <= 0) return prego_fail_(PREGO_EINVAL, "debug attention bwd: bad arguments");
  float* delta = nullptr;
  HIPCHK(hipMalloc((void**)&delta, (size_t)batch * heads * len * 4));
  const int rc = launch_attention_bwd(qs, k, v, o, dout, lse, delta, dqkv, batch, len, heads, dh, causal, 1.0f / sqrtf((float)dh), (hipStream_t)stream);
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(delta);
  if (rc) return prego_fail_(PREGO_EINVAL, "debug attention bwd: unsupported head dim %d", dh);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// debug / unit test: the attention forward kernel alone (tests/test_gpu_transformer.py)
extern "C" int prego_debug_attention_fwd(int batch, int n_query, int len, int heads, int dh, int causal, const void* qs, const void* k,
                                         const void* v, void* out, float* lse, prego_stream_t stream) {
  if (!qs || !k || !v || !out || batch <= 0 || len <= 0 || heads <= 0 || n_query <= 0 || n_query > len)
    return prego_fail_(PREGO_EINVAL, "debug attention fwd: bad arguments");
  const int rc = launch_flash_attention_v2(qs, k, v, out, batch, n_query, len, heads, dh, causal ? 1 : 0, (hipStream_t)stream, lse);
  (void)hipStreamSynchronize((hipStream_t)stream);
  if (rc) return prego_fail_(PREGO_EINVAL, "debug attention fwd: unsupported head dim %d", dh);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
#endif  // PREGO_DEBUG_ABI
