// ViTEnc training (include/prego_amd.h): the forward that keeps activations, the backward over them and the fused AdamW step
// (trainer/train.py:20-24 over ViT.py:117-143).  bf16 handles only.
#include "vit_handle.h"

#include <algorithm>

// per-site mask seeds: site 0 = positional dropout, per layer: 1 = attention branch, 2 = after GELU, 3 = FFN output,
// 4 = attention probabilities, 5 = proj_drop
static inline unsigned long long site_seed(const prego_vit* h, int layer, int site) {
  return h->drop_seed + 0x1000ull * (unsigned long long)(layer + 1) * (site ? 1 : 0) + (unsigned long long)site;
}
static VitBlockDrop block_drop(const prego_vit* h, int li) {
  return VitBlockDrop{drop_thresh(h->drop_p), drop_thresh(h->attn_drop_p), drop_scale(h->drop_p), drop_scale(h->attn_drop_p),
                      site_seed(h, li, 1), site_seed(h, li, 2), site_seed(h, li, 3), site_seed(h, li, 4), site_seed(h, li, 5)};
}

VitTrainWs vit_train_ws(const VitDims& d, int B, Arena a) {
  const size_t E = d.emb, T = d.window, N = T + 1, din = d.din(), mlp = d.mlp, M = (size_t)B * N, BHN = (size_t)B * d.heads * N;
  VitTrainWs w{};
  w.Mp = (int)align_up(M, 64);
  w.MTp = (int)align_up((size_t)B * T, 64);
  w.xb = a.put((size_t)B * T * din * 2); w.enc = a.put((size_t)B * T * E * 4); w.x = a.put(M * E * 4);
  w.L.resize(d.layers);
  for (auto& l : w.L) {
    l.keep = true;
    l.x_in = a.put(M * E * 4); l.st1 = a.put(M * 8); l.xn1 = a.put(M * E * 2);
    l.q = a.put(M * E * 2); l.k = a.put(M * E * 2); l.vn = a.put(M * E * 2);
    l.lse = a.put(BHN * 4); l.ao = a.put(M * E * 2);
    l.x_mid = a.put(M * E * 4); l.st2 = a.put(M * 8); l.xn2 = a.put(M * E * 2);
    l.u = a.put(M * mlp * 4); l.f = a.put(M * mlp * 2);
  }
  w.dx = a.put(M * E * 4); w.dxm = a.put(M * E * 4); w.dxb = a.put(M * E * 2); w.tmp = a.put(M * std::max(E, mlp) * 4);
  w.du = a.put(M * mlp * 4); w.dub = a.put(M * mlp * 2); w.dO = a.put(M * E * 2); w.dqkv = a.put(M * 3 * E * 2);
  w.delta = a.put(BHN * 4);
  w.dencb = a.put((size_t)B * T * E * 2);        // a k-major wgrad operand: read in its B*T rows only (kernels.h, launch_gemm_bf16_tn)
  w.part = a.put(std::max((M / 64 + 2) * std::max(mlp, E), (M / 4 + 2) * 2 * E) * 4);
  w.head = a.put((size_t)3 * B * E * 4); w.denc = a.put((size_t)B * T * E * 4); w.vec = a.put(4 * std::max(E, mlp) * 4);
  w.total = a.off;
  return w;
}
extern "C" size_t prego_vit_train_workspace_bytes(const prego_vit* h, int batch) {
  return (h && batch > 0) ? vit_train_ws(*h, batch).total : 0;
}

extern "C" int prego_vit_forward_train(prego_vit* h, int batch, const float* rgb, const float* flow, float* out_logits, int flags,
                                       void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (h && refuse_non_bf16("prego_vit_forward_train", h->f16, h->f32)) return PREGO_EINVAL;
  if (!h || !out_logits || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  const VitTrainWs w = vit_train_ws(*h, batch);
  if (int rc = vit_check_call(h, "training workspace", batch, rgb, flow, w.total, workspace_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int B = batch, T = h->window, N = T + 1, E = h->emb, din = h->din();
  const int causal = (flags & 1) ? 1 : 0;
  float* x = (float*)(ws + w.x);
  launch_cat_convert(rgb, flow, B * T, h->d_rgb, h->d_flow, ws + w.xb, s);
  launch_gemm_bf16_nt(ws + w.xb, din, h->enc_w, din, h->enc_b, (float*)(ws + w.enc), E, B * T, E, din, s);      // the eval forward's kernel: the keeping forward is the same arithmetic, bit for bit (test G5b)
  launch_vit_tokens((const float*)(ws + w.enc), h->cls, h->pe, B, T, E, x, s, drop_thresh(h->drop_p), drop_scale(h->drop_p), site_seed(h, 0, 0));
  for (int li = 0; li < h->layers; ++li) {
    const int rc = encoder_block_run(h, h->L[li], x, ws, w.L[li], block_drop(h, li), B, N, causal, s);
    if (rc) return rc > 0 ? prego_fail_(PREGO_EINVAL, "attention launch failed") : rc;
  }
  launch_vit_head(x, B, N, E, h->lnf_w, h->lnf_b, h->head_w, h->head_b, h->ncls, out_logits, s);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// Weight gradient C[Mo, No] = A^T . B over the rows (the reduction dimension of every weight gradient is the row index) and, when
// bias_out is given, the bias gradient colsum(A): the k-major GEMM of csrc/gemm_tn.hip reads A_rows [R, Mo] and B_rows [R, No] (bf16) as
// they lie in memory.  Rp = R padded to 64 (only the R rows are read).
int wgrad(const void* a_rows, int Mo, const void* b_rows, int No, int R, int Rp, float* out, float* bias_out, hipStream_t s) {
  return launch_gemm_bf16_tn(true, true, a_rows, Mo, b_rows, No, nullptr, out, No, Mo, No, Rp, R, bias_out, s);
}
// Input gradient C[R, No] = A [R, Ko] . W [Ko, No]: the weight as nn.Linear stores it IS the [K][N] operand (no transposed copy)
int dgrad(const void* a_rows, int Ko, const void* w, int No, int R, float* out, hipStream_t s, void* out16) {
  return launch_gemm_bf16_tn(false, true, a_rows, Ko, w, No, nullptr, out, No, R, No, Ko, Ko, nullptr, s, out16);
}

extern "C" int prego_vit_backward(prego_vit* h, int batch, const float* dlogits, float* const* grads, int n_tensors, int flags,
                                  void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (h && refuse_non_bf16("prego_vit_backward", h->f16, h->f32)) return PREGO_EINVAL;
  if (!h || !dlogits || !grads || !workspace) return prego_fail_(PREGO_EINVAL, "NULL argument");
  if (n_tensors != prego_vit_num_tensors(h)) return prego_fail_(PREGO_EINVAL, "expected %d gradient tensors, got %d", prego_vit_num_tensors(h), n_tensors);
  for (int i = 0; i < n_tensors; ++i) if (!grads[i]) return prego_fail_(PREGO_EINVAL, "gradient tensor %d is NULL", i);
  const VitTrainWs w = vit_train_ws(*h, batch);
  if (workspace_bytes < w.total) return prego_fail_(PREGO_EWORKSPACE, "training workspace %zu < %zu", workspace_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int B = batch, T = h->window, N = T + 1, E = h->emb, din = h->din(), M = B * N, dh = E / h->heads, mlp = h->mlp;
  const int causal = (flags & 1) ? 1 : 0;
  const int Mp = w.Mp;
  float* dx = (float*)(ws + w.dx);
  float* tmp = (float*)(ws + w.tmp);
  float* part = (float*)(ws + w.part);
  float* vec = (float*)(ws + w.vec);
  // gradient tensors in the order of the handle's tensor table (vit_handle.h)
  float* const* gf = grads;
  float* const* gt = grads + kVitFront + kVitLayerSlots * h->layers;

  // ---- head + final LayerNorm (token 0 only, ViT.py:134-138)
  HIPCHK(hipMemsetAsync(dx, 0, (size_t)M * E * 4, s));
  launch_vit_head_bwd((const float*)(ws + w.x), dlogits, B, N, E, h->ncls, h->lnf_w, h->lnf_b, h->head_w, dx, (float*)(ws + w.head),
                      gt[G_LNF_W], gt[G_LNF_B], gt[G_HEAD_W], gt[G_HEAD_B], s);

  for (int li = h->layers - 1; li >= 0; --li) {
    const VitLayer& l = h->L[li];
    const VitBlockBufs& k = w.L[li];
    const VitBlockDrop dp = block_drop(h, li);
    float* const* g = grads + kVitFront + kVitLayerSlots * li;
    // ---- FFN: x += drop(W2 drop(gelu(W1 LN2(x) + b1)) + b2)   (Transformer.py:35-47)
    // gradient entering a branch = dx through that branch's output dropout (same stateless mask as the forward), as bf16 in w.dxb
    if (dp.thr) launch_mask_convert(dx, (size_t)M * E, (float*)(ws + w.dxm), ws + w.dxb, dp.thr, dp.sc, dp.seed_ffn, s);
    else launch_f32_to_bf16(dx, ws + w.dxb, (size_t)M * E, s);
    if (wgrad(ws + w.dxb, E, ws + k.f, mlp, M, Mp, g[G_FF2_W], g[G_FF2_B], s) ||             // d W2 [E, mlp], d b2
        dgrad(ws + w.dxb, E, l.ff2_w, mlp, M, tmp, s)) return prego_fail_(PREGO_EINVAL, "backward: FFN-2 GEMM shape");   // d f = dx . W2
    launch_gelu_bwd(tmp, (const float*)(ws + k.u), (size_t)M * mlp, (float*)(ws + w.du), ws + w.dub, s, dp.thr, dp.sc, dp.seed_gelu);
    if (wgrad(ws + w.dub, mlp, ws + k.xn2, E, M, Mp, g[G_FF1_W], g[G_FF1_B], s) ||           // d W1 [mlp, E], d b1
        dgrad(ws + w.dub, mlp, l.ff1_w, E, M, tmp, s)) return prego_fail_(PREGO_EINVAL, "backward: FFN-1 GEMM shape");   // d LN2 out = du . W1
    int nb = launch_ln_relu_bwd(tmp, (const float*)(ws + k.x_mid), (const float*)(ws + k.st2), l.ln2_w, l.ln2_b, M, E, 0.f, 0, 0, dx,
                                part, s, 0, 1);                                              // dx += LN2 backward
    launch_colsum_stage2(part, nb, 2 * E, vec, s);
    HIPCHK(hipMemcpyAsync(g[G_LN2_W], vec, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(g[G_LN2_B], vec + E, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
    // ---- attention: x += drop(proj(attn(LN1(x))))   (Attention.py:21-41, Transformer.py:24-32)
    if (dp.thr || dp.athr)
      launch_mask_convert(dx, (size_t)M * E, (float*)(ws + w.dxm), ws + w.dxb, dp.thr, dp.sc, dp.seed_branch, s, dp.athr, dp.asc, dp.seed_proj);
    else launch_f32_to_bf16(dx, ws + w.dxb, (size_t)M * E, s);
    if (wgrad(ws + w.dxb, E, ws + k.ao, E, M, Mp, g[G_PROJ_W], g[G_PROJ_B], s) ||            // d Wproj [E, E], d proj bias
        dgrad(ws + w.dxb, E, l.proj_w, E, M, nullptr, s, ws + w.dO))                         // d o = dx . Wp (bf16, [B,N,h*dh])
      return prego_fail_(PREGO_EINVAL, "backward: projection GEMM shape");
    if (launch_attention_bwd(ws + k.q, ws + k.k, ws + k.vn, ws + k.ao, ws + w.dO, (const float*)(ws + k.lse), (float*)(ws + w.delta),
                             ws + w.dqkv, B, N, h->heads, dh, causal, 1.0f / sqrtf((float)dh), s, dp.athr, dp.asc, dp.seed_probs))
      return prego_fail_(PREGO_EINVAL, "attention backward launch failed");
    if (wgrad(ws + w.dqkv, 3 * E, ws + k.xn1, E, M, Mp, g[G_QKV_W], nullptr, s) ||           // d Wqkv [3E, E] (no bias, Attention.py:16)
        dgrad(ws + w.dqkv, 3 * E, l.qkv_w, E, M, tmp, s)) return prego_fail_(PREGO_EINVAL, "backward: qkv GEMM shape");   // d LN1 out
    nb = launch_ln_relu_bwd(tmp, (const float*)(ws + k.x_in), (const float*)(ws + k.st1), l.ln1_w, l.ln1_b, M, E, 0.f, 0, 0, dx, part,
                            s, 0, 1);                                                        // dx += LN1 backward
    launch_colsum_stage2(part, nb, 2 * E, vec, s);
    HIPCHK(hipMemcpyAsync(g[G_LN1_W], vec, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(g[G_LN1_B], vec + E, (size_t)E * 4, hipMemcpyDeviceToDevice, s));
  }
  // ---- tokens: positional table, cls token, encoding Linear (ViT.py:125-129)
  float* denc = (float*)(ws + w.denc);
  launch_vit_tokens_bwd(dx, B, T, E, denc, gf[G_PE], gf[G_CLS], s, drop_thresh(h->drop_p), drop_scale(h->drop_p), site_seed(h, 0, 0));
  launch_f32_to_bf16(denc, ws + w.dencb, (size_t)B * T * E, s);                              // the wgrad's A operand in bf16 (rows = frames)
  if (wgrad(ws + w.dencb, E, ws + w.xb, din, B * T, w.MTp, gf[G_ENC_W], gf[G_ENC_B], s)) return prego_fail_(PREGO_EINVAL, "backward: encoding GEMM shape");   // d W_enc [E, din], d b_enc
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// optimizer.step() on the handle's tensors: fused AdamW that also rewrites the handle's operand copies (csrc/optim.hip).  Matrices (bf16
// copies) and vectors (fp32 copies) go in two launches, one copy element type each, both in table order
namespace {
struct AdamwList {
  std::vector<float*> p, m, v; std::vector<const float*> g; std::vector<void*> copy; std::vector<long long> n;
  int launch(bool bf16, int64_t step, float lr, float b1, float b2, float eps, float wd, hipStream_t s) {
    return launch_adamw((int)p.size(), p.data(), g.data(), m.data(), v.data(), copy.data(), n.data(), bf16, step, lr, b1, b2, eps, wd, s);
  }
};
}  // namespace
extern "C" int prego_vit_adamw_step(prego_vit* h, float* const* params, const float* const* grads, float* const* exp_avg,
                                    float* const* exp_avg_sq, int n_tensors, int64_t step, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, prego_stream_t stream) {
  if (h && refuse_non_bf16("prego_vit_adamw_step", h->f16, h->f32)) return PREGO_EINVAL;
  if (!h || !params || !grads || !exp_avg || !exp_avg_sq) return prego_fail_(PREGO_EINVAL, "vit adamw: NULL argument");
  if (!h->have_weights) return prego_fail_(PREGO_EINVAL, "vit adamw step before set_weights");
  if (n_tensors != prego_vit_num_tensors(h)) return prego_fail_(PREGO_EINVAL, "expected %d tensors, got %d", prego_vit_num_tensors(h), n_tensors);
  for (int i = 0; i < n_tensors; ++i) if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]) return prego_fail_(PREGO_EINVAL, "vit adamw: tensor %d is NULL", i);
  AdamwList mats, vecs;
  for (int i = 0; i < n_tensors; ++i) {
    const VitTensor& t = h->tensors[i];
    AdamwList& a = t.matrix ? mats : vecs;
    a.p.push_back(params[i]); a.g.push_back(grads[i]); a.m.push_back(exp_avg[i]); a.v.push_back(exp_avg_sq[i]);
    a.copy.push_back(t.matrix ? *t.op : (void*)*t.f32); a.n.push_back((long long)t.n);
  }
  hipStream_t s = (hipStream_t)stream;
  if (mats.launch(true, step, lr, beta1, beta2, eps, weight_decay, s) || vecs.launch(false, step, lr, beta1, beta2, eps, weight_decay, s))
    return prego_fail_(PREGO_EINVAL, "vit adamw: bad step %lld", (long long)step);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
