// C ABI of the "Transformer" (ViTEnc) path (include/prego_amd.h): the handle, its weights and the inference entries.
// bf16 (or, inference only, IEEE fp16) MFMA operands, fp32 accumulation / residual stream / LayerNorm / softmax.
// Training: vit_train.cpp; the AttentionLayer op: attention_layer.cpp; the stream pool: vit_stream.cpp.
#include "vit_handle.h"

#include <algorithm>

extern "C" int prego_vit_set_dropout(prego_vit* h, float p, float attn_p, uint64_t seed) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (!(p >= 0.f && p < 1.f) || !(attn_p >= 0.f && attn_p < 1.f)) return prego_fail_(PREGO_EINVAL, "dropout p = %f, attn p = %f", (double)p, (double)attn_p);
  h->drop_p = p;
  h->attn_drop_p = attn_p;
  h->drop_seed = seed;
  return PREGO_OK;
}

std::vector<VitTensor> vit_tensors(prego_vit* h) {
  const int E = h->emb, mlp = h->mlp;
  auto mat = [](int rows, int cols, void** op, float** f32) { return VitTensor{(size_t)rows * cols, rows, cols, true, op, f32}; };
  auto vec = [](size_t n, float** f32) { return VitTensor{n, 1, (int)n, false, nullptr, f32}; };
  VitTensor front[kVitFront], tail[kVitTail], lt[kVitLayerSlots];
  front[G_ENC_W] = mat(E, h->din(), &h->enc_w, &h->enc_w32); front[G_ENC_B] = vec(E, &h->enc_b);
  front[G_CLS] = vec(E, &h->cls); front[G_PE] = vec((size_t)(h->window + 1) * E, &h->pe);
  std::vector<VitTensor> t(front, front + kVitFront);
  for (auto& l : h->L) {
    lt[G_LN1_W] = vec(E, &l.ln1_w); lt[G_LN1_B] = vec(E, &l.ln1_b);
    lt[G_QKV_W] = mat(3 * E, E, &l.qkv_w, &l.qkv_w32);
    lt[G_PROJ_W] = mat(E, E, &l.proj_w, &l.proj_w32); lt[G_PROJ_B] = vec(E, &l.proj_b);
    lt[G_LN2_W] = vec(E, &l.ln2_w); lt[G_LN2_B] = vec(E, &l.ln2_b);
    lt[G_FF1_W] = mat(mlp, E, &l.ff1_w, &l.ff1_w32); lt[G_FF1_B] = vec(mlp, &l.ff1_b);
    lt[G_FF2_W] = mat(E, mlp, &l.ff2_w, &l.ff2_w32); lt[G_FF2_B] = vec(E, &l.ff2_b);
    t.insert(t.end(), lt, lt + kVitLayerSlots);
  }
  tail[G_LNF_W] = vec(E, &h->lnf_w); tail[G_LNF_B] = vec(E, &h->lnf_b);
  tail[G_HEAD_W] = vec((size_t)h->ncls * E, &h->head_w); tail[G_HEAD_B] = vec(h->ncls, &h->head_b);
  t.insert(t.end(), tail, tail + kVitTail);
  return t;
}

static int dmalloc(prego_vit* h, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return prego_fail_(PREGO_EHIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  h->allocs.push_back(*p);
  return 0;
}

extern "C" int prego_vit_create(prego_vit** out, int d_rgb, int d_flow, int emb, int mlp, int heads, int layers, int window,
                                int n_classes) {
  if (!out) return prego_fail_(PREGO_EINVAL, "out is NULL");
  *out = nullptr;
  const int din = d_rgb + d_flow;
  if (din <= 0 || din % 64) return prego_fail_(PREGO_EINVAL, "feature size %d must be a multiple of 64", din);
  if (emb % 512 || emb > 4096) return prego_fail_(PREGO_EINVAL, "embedding_dim %d must be a multiple of 512, <= 4096", emb);
  if (mlp % 128) return prego_fail_(PREGO_EINVAL, "hidden_dim (mlp) %d must be a multiple of 128", mlp);
  if (heads <= 0 || emb % heads) return prego_fail_(PREGO_EINVAL, "num_heads %d must divide embedding_dim", heads);
  const int dh = emb / heads;
  if (dh != 64 && dh != 128 && dh != 256) return prego_fail_(PREGO_EINVAL, "head dim %d: supported 64, 128, 256", dh);
  if (layers <= 0 || window <= 0 || n_classes <= 0) return prego_fail_(PREGO_EINVAL, "bad layers/window/classes");
  prego_vit* h = new prego_vit();
  static_cast<VitDims&>(*h) = VitDims{d_rgb, d_flow, emb, mlp, heads, layers, window, n_classes};
  h->L.resize(layers);
  h->tensors = vit_tensors(h);
  int rc = 0;
  for (const VitTensor& t : h->tensors) rc |= t.matrix ? dmalloc(h, t.op, t.n * 2) : dmalloc(h, (void**)t.f32, t.n * 4);
  if (rc) { for (void* p : h->allocs) (void)hipFree(p); delete h; return PREGO_EHIP; }
  *out = h;
  return PREGO_OK;
}

extern "C" void prego_vit_destroy(prego_vit* h) {
  if (!h) return;
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
}

extern "C" int prego_vit_set_compute_dtype(prego_vit* h, int compute_dtype) {
  if (!h) return prego_fail_(PREGO_EINVAL, "handle is NULL");
  if (compute_dtype != PREGO_BF16 && compute_dtype != PREGO_F16 && compute_dtype != PREGO_F32)
    return prego_fail_(PREGO_EINVAL, "ViTEnc compute_dtype %d: PREGO_BF16, PREGO_F16 or PREGO_F32", compute_dtype);
  if ((compute_dtype == PREGO_F16) != h->f16 || (compute_dtype == PREGO_F32) != h->f32) h->have_weights = false;   // other copies: re-ingest
  h->f16 = compute_dtype == PREGO_F16;
  h->f32 = compute_dtype == PREGO_F32;
  if (h->f32 && !h->enc_w32) {          // fp32 copies of the matrices, allocated with the first switch to this mode
    int rc = 0;
    for (const VitTensor& t : h->tensors) if (t.matrix) rc |= dmalloc(h, (void**)t.f32, t.n * 4);
    if (rc) { h->f32 = false; return PREGO_EHIP; }
  }
  return PREGO_OK;
}

extern "C" int prego_vit_num_tensors(const prego_vit* h) { return h ? (int)h->tensors.size() : 0; }

extern "C" int prego_vit_set_weights(prego_vit* h, const float* const* t, int n_tensors, prego_stream_t stream) {
  if (!h || !t) return prego_fail_(PREGO_EINVAL, "NULL");
  if (n_tensors != prego_vit_num_tensors(h)) return prego_fail_(PREGO_EINVAL, "expected %d tensors, got %d", prego_vit_num_tensors(h), n_tensors);
  for (int i = 0; i < n_tensors; ++i) if (!t[i]) return prego_fail_(PREGO_EINVAL, "tensor %d is NULL", i);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n_tensors; ++i) {
    const VitTensor& e = h->tensors[i];
    // a matrix becomes the 16-bit operand; a vector, and in the parity mode every tensor, is kept as it comes
    if (e.matrix && !h->f32) launch_pad_convert(true, t[i], e.rows, e.cols, e.cols, *e.op, e.rows, e.cols, s, h->f16);
    else HIPCHK(hipMemcpyAsync(*e.f32, t[i], e.n * 4, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(hipGetLastError());
  h->have_weights = true;
  return PREGO_OK;
}

// ---- workspace layouts of the inference entries ------------------------------------------------------------------------------------
VitWs vit_ws(const VitDims& d, int B, Arena a) {
  const size_t E = d.emb, T = d.window, N = T + 1, din = d.din(), mlp = d.mlp;
  VitWs w{};
  w.xb = a.put((size_t)B * T * din * 2); w.enc = a.put((size_t)B * T * E * 4); w.x = a.put((size_t)B * N * E * 4);
  w.xn = a.put((size_t)B * N * E * 2); w.q = a.put((size_t)B * N * E * 2); w.k = a.put((size_t)B * N * E * 2);
  w.vn = a.put((size_t)B * N * E * 2); w.ao = a.put((size_t)B * N * E * 2); w.f = a.put((size_t)B * N * mlp * 2);
  // last block, token 0 only (ViT.py:136 reads x[:, 0]): one row per window
  w.x0 = a.put((size_t)B * E * 4); w.q0 = a.put((size_t)B * E * 2); w.ao0 = a.put((size_t)B * E * 2); w.xn0 = a.put((size_t)B * E * 2);
  w.f0 = a.put((size_t)B * mlp * 2);
  w.total = a.off;
  return w;
}
VitWs32 vit_ws32(const VitDims& d, int B, Arena a) {
  const size_t E = d.emb, T = d.window, N = T + 1, din = d.din(), M = (size_t)B * N, mlp = d.mlp;
  VitWs32 w{};
  w.xc = a.put((size_t)B * T * din * 4); w.enc = a.put((size_t)B * T * E * 4); w.x = a.put(M * E * 4); w.xn = a.put(M * E * 4);
  w.qkv = a.put(M * 3 * E * 4); w.ao = a.put(M * E * 4); w.tmp = a.put(M * std::max(E, mlp) * 4);
  w.total = a.off;
  return w;
}
VitStepWs vit_step_ws(const VitDims& d, int n, int wb, bool argmax, Arena a) {
  VitStepWs f{};
  f.xb = a.put((size_t)n * d.din() * 2); f.enc = a.put((size_t)n * d.emb * 4);
  if (argmax) f.am = a.put((size_t)n * 4);
  f.w = vit_ws(d, wb);
  f.win = a.put(f.w.total);
  f.total = a.off;
  return f;
}
extern "C" size_t prego_vit_workspace_bytes(const prego_vit* h, int batch) {
  if (!h || batch <= 0) return 0;
  return h->f32 ? vit_ws32(*h, batch).total : vit_ws(*h, batch).total;
}
extern "C" size_t prego_vit_frames_workspace_bytes(const prego_vit* h, int n_frames, int windows_per_batch) {
  return (h && n_frames > 0 && windows_per_batch > 0) ? vit_step_ws(*h, n_frames, windows_per_batch, false).total : 0;
}

int vit_check_call(const prego_vit* h, const char* who, int batch, const float* rgb, const float* flow, size_t need, size_t have) {
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "forward before set_weights");
  if (batch <= 0) return prego_fail_(PREGO_EINVAL, "batch %d", batch);
  if ((h->d_rgb > 0 && !rgb) || (h->d_rgb == 0 && !flow)) return prego_fail_(PREGO_EINVAL, "missing input");
  if (have < need) return prego_fail_(PREGO_EWORKSPACE, "%s %zu < %zu", who, have, need);
  return 0;
}

// ---- the encoder blocks ------------------------------------------------------------------------------------------------------------
int encoder_block_run(const prego_vit* h, const VitLayer& l, float* x, char* ws, const VitBlockBufs& b, const VitBlockDrop& dp, int B, int N,
                      int causal, hipStream_t s) {
  const int E = h->emb, M = B * N, dh = E / h->heads, mlp = h->mlp;
  const bool f16 = h->f16;
  if (b.keep) HIPCHK(hipMemcpyAsync(ws + b.x_in, x, (size_t)M * E * 4, hipMemcpyDeviceToDevice, s));
  launch_ln_relu(true, x, l.ln1_w, l.ln1_b, M, E, 1e-5f, ws + b.xn1, b.keep ? (float*)(ws + b.st1) : nullptr, 0.f, 0, 0, s, 0, false, f16);
  const GemmEpi e = epi_qkv(f16, ws + b.q, ws + b.k, ws + b.vn, N, h->heads, dh, E);
  launch_gemm_bf16_nt_epi(ws + b.xn1, E, l.qkv_w, E, nullptr, nullptr, 0, M, 3 * E, E, e, s);
  if (launch_flash_attention_v2(ws + b.q, ws + b.k, ws + b.vn, ws + b.ao, B, N, N, h->heads, dh, causal, s, b.keep ? (float*)(ws + b.lse) : nullptr,
                                dp.athr, dp.athr ? dp.asc : 1.f, dp.seed_probs, f16))
    return 1;
  GemmEpi r = epi_residual(f16);
  r.drop_thresh = dp.thr; r.drop_scale = dp.sc; r.drop_seed = dp.seed_branch;
  r.drop2_thresh = dp.athr; r.drop2_scale = dp.asc; r.drop2_seed = dp.seed_proj;                      // proj_drop, then PreNormDrop
  launch_gemm_bf16_nt_epi(ws + b.ao, E, l.proj_w, E, l.proj_b, x, E, M, E, E, r, s);                  // x += drop(proj(attn))
  if (b.keep) HIPCHK(hipMemcpyAsync(ws + b.x_mid, x, (size_t)M * E * 4, hipMemcpyDeviceToDevice, s));
  launch_ln_relu(true, x, l.ln2_w, l.ln2_b, M, E, 1e-5f, ws + b.xn2, b.keep ? (float*)(ws + b.st2) : nullptr, 0.f, 0, 0, s, 0, false, f16);
  GemmEpi g = epi_gelu(f16, ws + b.f);
  if (b.keep) g.pre_f32 = (float*)(ws + b.u);
  g.drop_thresh = dp.thr; g.drop_scale = dp.sc; g.drop_seed = dp.seed_gelu;
  launch_gemm_bf16_nt_epi(ws + b.xn2, E, l.ff1_w, E, l.ff1_b, nullptr, mlp, M, mlp, E, g, s);         // f = drop(gelu(W1 . + b1))
  r.drop_seed = dp.seed_ffn; r.drop2_thresh = 0;
  launch_gemm_bf16_nt_epi(ws + b.f, mlp, l.ff2_w, mlp, l.ff2_b, x, E, M, E, mlp, r, s);               // x += drop(W2 f + b2)
  return 0;
}
// the full block of the inference paths: nothing kept, no dropout, LN1 and LN2 share w.xn
static int encoder_block(const prego_vit* h, const VitLayer& l, float* x, char* ws, const VitWs& w, int B, int N, int causal, hipStream_t s) {
  return encoder_block_run(h, l, x, ws, VitBlockBufs{w.xn, w.q, w.k, w.vn, w.ao, w.xn, w.f}, VitBlockDrop{}, B, N, causal, s);
}

// The LAST encoder block when only token 0 of its output is read (ViT.py:136 `x[:, 0]`, then pre_head_ln and mlp_head): keys and
// values are needed for every token, but the query, the attention output, the projection, the residual stream and the whole FFN
// only for token 0 of each window - B rows instead of B*N.  Exact (the skipped rows never reach the logits); with num_layers = 1
// it removes 44 % of a window's FLOPs.  Leaves the block's token-0 output in x0 [B, E].
int encoder_block_token0(const prego_vit* h, const VitLayer& l, const float* x, char* ws, const VitWs& w, int B, int N, int causal,
                         hipStream_t s, bool have_xn) {
  const int E = h->emb, M = B * N, dh = E / h->heads;
  const bool f16 = h->f16;
  if (!have_xn) launch_ln_relu(true, x, l.ln1_w, l.ln1_b, M, E, 1e-5f, ws + w.xn, nullptr, 0.f, 0, 0, s, 0, false, f16);
  GemmEpi e = epi_qkv(f16, ws + w.q0, ws + w.k, ws + w.vn, N, h->heads, dh, E);
  e.which0 = 1;                                                                                // k | v for every token
  launch_gemm_bf16_nt_epi(ws + w.xn, E, (const char*)l.qkv_w + (size_t)E * E * 2, E, nullptr, nullptr, 0, M, 2 * E, E, e, s);
  e.which0 = 0; e.n_tok = 1;                                                                   // q for token 0: rows b * N of xn
  launch_gemm_bf16_nt_epi(ws + w.xn, N * E, l.qkv_w, E, nullptr, nullptr, 0, B, E, E, e, s);
  if (launch_flash_attention_v2(ws + w.q0, ws + w.k, ws + w.vn, ws + w.ao0, B, 1, N, h->heads, dh, causal, s, nullptr, 0, 1.f, 0, f16)) return -1;
  float* x0 = (float*)(ws + w.x0);
  if (!have_xn && hipMemcpy2DAsync(x0, (size_t)E * 4, x, (size_t)N * E * 4, (size_t)E * 4, B, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
  const GemmEpi r = epi_residual(f16);
  launch_gemm_bf16_nt_epi(ws + w.ao0, E, l.proj_w, E, l.proj_b, x0, E, B, E, E, r, s);
  launch_ln_relu(true, x0, l.ln2_w, l.ln2_b, B, E, 1e-5f, ws + w.xn0, nullptr, 0.f, 0, 0, s, 0, false, f16);
  launch_gemm_bf16_nt_epi(ws + w.xn0, E, l.ff1_w, E, l.ff1_b, nullptr, h->mlp, B, h->mlp, E, epi_gelu(f16, ws + w.f0), s);
  launch_gemm_bf16_nt_epi(ws + w.f0, h->mlp, l.ff2_w, h->mlp, l.ff2_b, x0, E, B, E, h->mlp, r, s);
  return 0;
}

int blocks_and_head(const prego_vit* h, const char* who, char* ws, const VitWs& w, int B, int causal, bool fused, float* out_logits,
                    int32_t* am, hipStream_t s) {
  const int N = h->window + 1;
  for (int li = 0; li < h->layers; ++li) {
    const bool last = li + 1 == h->layers;
    const int rc = last ? encoder_block_token0(h, h->L[li], (const float*)(ws + w.x), ws, w, B, N, causal, s, fused)
                        : encoder_block(h, h->L[li], (float*)(ws + w.x), ws, w, B, N, causal, s);
    if (rc) return who ? prego_fail_(PREGO_EINVAL, "%s: encoder block launch failed", who) : prego_fail_(PREGO_EINVAL, "encoder block launch failed");
  }
  launch_vit_head((const float*)(ws + w.x0), B, 1, h->emb, h->lnf_w, h->lnf_b, h->head_w, h->head_b, h->ncls, out_logits, s, (int*)am);
  return 0;
}

// ViTEnc.forward (ViT.py:117-143) with fp32 operands: the projections on the exact-fp32 MFMA GEMM, everything else in fp32 too
static int vit_forward_f32(prego_vit* h, int B, const float* rgb, const float* flow, float* out_logits, int causal, char* ws,
                           hipStream_t s) {
  const VitWs32 w = vit_ws32(*h, B);
  const int T = h->window, N = T + 1, E = h->emb, din = h->din(), M = B * N, dh = E / h->heads, mlp = h->mlp;
  float* xc = (float*)(ws + w.xc); float* enc = (float*)(ws + w.enc); float* x = (float*)(ws + w.x); float* xn = (float*)(ws + w.xn);
  float* qkv = (float*)(ws + w.qkv); float* ao = (float*)(ws + w.ao); float* tmp = (float*)(ws + w.tmp);
  launch_cat_rows_f32(rgb, flow, B * T, h->d_rgb, h->d_flow, xc, s);
  launch_gemm_f32_nt(xc, din, h->enc_w32, din, h->enc_b, enc, E, B * T, E, din, s);                     // ViT.py:124
  launch_vit_tokens(enc, h->cls, h->pe, B, T, E, x, s);                                                  // ViT.py:125-129
  for (int li = 0; li < h->layers; ++li) {
    const VitLayer& l = h->L[li];
    launch_ln_relu(false, x, l.ln1_w, l.ln1_b, M, E, 1e-5f, xn, nullptr, 0.f, 0, 0, s, 0);
    launch_gemm_f32_nt(xn, E, l.qkv_w32, E, nullptr, qkv, 3 * E, M, 3 * E, E, s);                       // Attention.py:23-27
    if (launch_attention_f32(qkv, 3 * E, 0, E, 2 * E, ao, B, N, N, h->heads, dh, causal, 1.0f / sqrtf((float)dh), s))
      return prego_fail_(PREGO_EINVAL, "attention launch failed");
    launch_gemm_f32_nt(ao, E, l.proj_w32, E, l.proj_b, tmp, E, M, E, E, s);
    launch_add_rows(x, tmp, (size_t)M * E, s);                                                           // Transformer.py:24-32
    launch_ln_relu(false, x, l.ln2_w, l.ln2_b, M, E, 1e-5f, xn, nullptr, 0.f, 0, 0, s, 0);
    launch_gemm_f32_nt(xn, E, l.ff1_w32, E, l.ff1_b, tmp, mlp, M, mlp, E, s);
    launch_gelu_f32(tmp, (size_t)M * mlp, s);                                                            // Transformer.py:40
    launch_gemm_f32_nt(tmp, mlp, l.ff2_w32, mlp, l.ff2_b, xn, E, M, E, mlp, s);
    launch_add_rows(x, xn, (size_t)M * E, s);
  }
  launch_vit_head(x, B, N, E, h->lnf_w, h->lnf_b, h->head_w, h->head_b, h->ncls, out_logits, s);       // token 0, ViT.py:134-141
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_vit_forward(prego_vit* h, int batch, const float* rgb, const float* flow, float* out_logits, int flags,
                                 void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!h || !out_logits || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  const VitWs w = vit_ws(*h, batch);
  if (int rc = vit_check_call(h, "workspace", batch, rgb, flow, h->f32 ? vit_ws32(*h, batch).total : w.total, workspace_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int B = batch, T = h->window, N = T + 1, E = h->emb, din = h->din();
  const int causal = (flags & 1) ? 1 : 0;
  if (h->f32) return vit_forward_f32(h, B, rgb, flow, out_logits, causal, ws, s);
  const bool all_rows = (flags & 2) != 0;             // bit 1 (debug / A-B): run the last block on every token as well
  launch_cat_convert(rgb, flow, B * T, h->d_rgb, h->d_flow, ws + w.xb, s, h->f16);
  // ViT.py:125-129: the encoding GEMM writes the residual stream itself (frame rows + positional rows in its epilogue: no fp32
  // encoding tensor, no token kernel pass); the cls row of every window is B short rows
  static const bool no_epi_tokens = prego_tune_env("PREGO_VIT_TOKENS_KERNEL") != nullptr;       // A/B: the separate token kernel
  if (no_epi_tokens || B * T < 4096) {       // small batches: the 128 x 128 kernel's per-element epilogue costs more than the token kernel
    launch_gemm_bf16_nt(ws + w.xb, din, h->enc_w, din, h->enc_b, (float*)(ws + w.enc), E, B * T, E, din, s, h->f16);
    launch_vit_tokens((const float*)(ws + w.enc), h->cls, h->pe, B, T, E, (float*)(ws + w.x), s);
  } else {
    GemmEpi te{}; te.f16 = h->f16 ? 1 : 0;
    te.mode = EPI_TOKENS; te.pe = h->pe; te.n_tok = T;
    launch_gemm_bf16_nt_epi(ws + w.xb, din, h->enc_w, din, h->enc_b, (float*)(ws + w.x), E, B * T, E, din, te, s);
    launch_vit_cls_rows(h->cls, h->pe, B, T, E, (float*)(ws + w.x), s);
  }
  if (all_rows) {
    for (const VitLayer& l : h->L)
      if (encoder_block(h, l, (float*)(ws + w.x), ws, w, B, N, causal, s)) return prego_fail_(PREGO_EINVAL, "encoder block launch failed");
    launch_vit_head((const float*)(ws + w.x), B, N, E, h->lnf_w, h->lnf_b, h->head_w, h->head_b, h->ncls, out_logits, s);
  } else if (int rc = blocks_and_head(h, nullptr, ws, w, B, causal, false, out_logits, nullptr, s)) return rc;
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// ================================================================================================
// per-frame inference over a whole video (the eval loop of trainer/eval.py:36-56 for model: 'Transformer')
// ================================================================================================
// ViTEnc emits one logit vector per window (ViT.py:136-141) and needs T == window_size; the per-frame output the eval loop
// collects is the window ENDING at every frame, zero feature rows in front of the video - the windows the training loader cuts
// (dataset.py:53-55,96-103) at stride 1.  Frame f sits in up to `window` windows, and linear_encoding (ViT.py:124, half of a
// window's FLOPs at one layer) does not depend on the position inside the window (the positional table is added afterwards,
// ViT.py:129): it runs ONCE per frame here.  Windows are processed `wb` at a time through the same blocks as prego_vit_forward.
extern "C" int prego_vit_forward_frames(prego_vit* h, int n_frames, const float* rgb, const float* flow, float* out_logits,
                                        int32_t* out_argmax, int windows_per_batch, int flags, void* workspace, size_t workspace_bytes,
                                        prego_stream_t stream) {
  if (!h || !out_logits || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (h->f32) return prego_fail_(PREGO_EINVAL, "prego_vit_forward_frames on an fp32-operand handle: the parity mode covers prego_vit_forward");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "forward before set_weights");
  if (n_frames <= 0 || windows_per_batch <= 0) return prego_fail_(PREGO_EINVAL, "n_frames %d, windows_per_batch %d", n_frames, windows_per_batch);
  const int wb = windows_per_batch;
  const VitStepWs f = vit_step_ws(*h, n_frames, wb, false);
  if (int rc = vit_check_call(h, "workspace", n_frames, rgb, flow, f.total, workspace_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  char* ws = base + f.win;                      // the per-batch arena, laid out as prego_vit_forward's
  const VitWs& w = f.w;
  const int T = h->window, E = h->emb, din = h->din();
  const int causal = (flags & 1) ? 1 : 0;
  float* enc = (float*)(base + f.enc);
  launch_cat_convert(rgb, flow, n_frames, h->d_rgb, h->d_flow, base + f.xb, s, h->f16);
  launch_gemm_bf16_nt(base + f.xb, din, h->enc_w, din, h->enc_b, enc, E, n_frames, E, din, s, h->f16);       // ViT.py:124, once per frame
  const bool fused = h->layers == 1;            // one layer: the token kernel writes LayerNorm1(x) and x0; x is never materialised
  for (int t0 = 0; t0 < n_frames; t0 += wb) {
    const int B = std::min(wb, n_frames - t0);
    const VitLayer& l0 = h->L[0];
    launch_vit_sliding_tokens(enc, h->enc_b, h->cls, h->pe, t0, B, T, E, fused ? nullptr : (float*)(ws + w.x), l0.ln1_w, l0.ln1_b,
                              fused ? ws + w.xn : nullptr, fused ? (float*)(ws + w.x0) : nullptr, s, h->f16);
    if (int rc = blocks_and_head(h, nullptr, ws, w, B, causal, fused, out_logits + (size_t)t0 * h->ncls, out_argmax ? out_argmax + t0 : nullptr, s))
      return rc;
  }
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

#ifdef PREGO_DEBUG_ABI
static prego_vit dims_only(const int32_t* v) {      // a handle without device memory: the table and the layouts read nothing else
  prego_vit h;
  static_cast<VitDims&>(h) = VitDims{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  h.L.resize(v[5] > 0 ? v[5] : 0);
  return h;
}
extern "C" int prego_debug_vit_tensor(const int32_t* dims, int i, int32_t* rows, int32_t* cols, int32_t* is_matrix) {
  if (!dims || !rows || !cols || !is_matrix) return -1;
  prego_vit h = dims_only(dims);
  const std::vector<VitTensor> t = vit_tensors(&h);
  if (i >= 0 && i < (int)t.size()) { *rows = t[i].rows; *cols = t[i].cols; *is_matrix = t[i].matrix ? 1 : 0; }
  return (int)t.size();
}
extern "C" int prego_debug_vit_layout(int kind, const int32_t* dims, int a, int b, uint64_t* offsets, int cap) {
  if (!dims || !offsets || cap < 1) return -1;
  const VitDims d{dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], dims[6], dims[7]};
  std::vector<size_t> v(2 * (size_t)cap);
  ArenaLog log{v.data(), cap, 0};
  Arena ar; ar.log = &log;
  size_t total = 0;
  switch (kind) {
    case 0: total = vit_ws(d, a, ar).total; break;
    case 1: total = vit_ws32(d, a, ar).total; break;
    case 2: total = vit_step_ws(d, a, b, false, ar).total; break;
    case 3: total = vit_step_ws(d, a, a, true, ar).total; break;
    case 4: total = vit_train_ws(d, a, ar).total; break;
    case 5: total = attn_ws(d.emb, a, b, false, ar).total; break;
    case 6: total = attn_ws(d.emb, a, b, true, ar).total; break;
    case 7: total = attn_train_ws(d.emb, d.heads, a, b, ar).total; break;
    case 8: total = attn_op_ws(d.emb, a, b, ar).total; break;
    default: return -1;
  }
  if (2 * log.n + 1 > cap) return -1;
  for (int i = 0; i < 2 * log.n; ++i) offsets[i] = v[i];
  offsets[2 * log.n] = total;
  return log.n;
}
#endif
