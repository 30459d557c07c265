// Private to the Transformer host files: the ViTEnc handle and its tensor table, the workspace layouts, the encoder-block runners and the
// small helpers that more than one of the files uses.  Which file defines what:
//   vit_host.cpp         create / destroy, the tensor table, weight setters, the inference layouts (vit_ws, vit_ws32, vit_step_ws), the
//                        block runners (encoder_block_run, encoder_block_token0, vit_forward_f32), blocks_and_head, forward, forward_frames
//   vit_train.cpp        vit_train_ws, prego_vit_forward_train / _backward / _adamw_step, wgrad / dgrad
//   attention_layer.cpp  the AttentionLayer op: stateless, handle, training; its layouts; the two prego_debug_attention_* entries
//   vit_stream.cpp       the Transformer stream pool: prego_vit_stream_pool_*, prego_vit_step_pool(_bursts) (kernels: vit_stream.hip)
#pragma once
#include "host_common.h"

#include <cmath>
#include <vector>

// the model's dimensions: all a layout needs, so that a layout can be computed without a handle (and without a device)
struct VitDims {
  int d_rgb, d_flow, emb, mlp, heads, layers, window, ncls;
  int din() const { return d_rgb + d_flow; }
};
struct VitLayer {
  float *ln1_w, *ln1_b, *proj_b, *ln2_w, *ln2_b, *ff1_b, *ff2_b;
  void *qkv_w, *proj_w, *ff1_w, *ff2_w;    // bf16
  float *qkv_w32 = nullptr, *proj_w32 = nullptr, *ff1_w32 = nullptr, *ff2_w32 = nullptr;   // PREGO_F32 handles only
};
// One tensor of the handle.  A matrix has a 16-bit operand copy (*op) and, on PREGO_F32 handles, an fp32 copy (*f32); a vector has its
// fp32 copy (*f32) only.  The pointers are the addresses of the handle's own members
struct VitTensor {
  size_t n;              // elements
  int rows, cols;        // of a matrix as nn.Linear stores it; a vector: 1 x n
  bool matrix;
  void** op;
  float** f32;
};
// THE order of the handle's tensors (prego_vit_set_weights, the gradient and optimizer lists; _tensor_order in transformer.py): VitFront,
// then VitLayerSlot per layer, then VitTail.  vit_tensors() fills the table by these names, so the two cannot disagree
enum VitFront { G_ENC_W, G_ENC_B, G_CLS, G_PE, kVitFront };
enum VitLayerSlot { G_LN1_W, G_LN1_B, G_QKV_W, G_PROJ_W, G_PROJ_B, G_LN2_W, G_LN2_B, G_FF1_W, G_FF1_B, G_FF2_W, G_FF2_B, kVitLayerSlots };
enum VitTail { G_LNF_W, G_LNF_B, G_HEAD_W, G_HEAD_B, kVitTail };
struct prego_vit : VitDims {
  void* enc_w = nullptr; float* enc_b = nullptr; float* cls = nullptr; float* pe = nullptr;
  std::vector<VitLayer> L;
  float *lnf_w = nullptr, *lnf_b = nullptr, *head_w = nullptr, *head_b = nullptr;
  std::vector<VitTensor> tensors;  // vit_tensors(this), built once by create
  std::vector<void*> allocs;
  bool have_weights = false;
  bool f16 = false;                // IEEE fp16 operands / 16-bit activations instead of bf16 (prego_vit_set_compute_dtype; inference only)
  bool f32 = false;                // fp32 operands everywhere (parity mode, prego_vit_forward only): the matrices are kept in fp32
  float* enc_w32 = nullptr;
  // training-mode dropout (cfg['dropout']; ViT.py:130 pe_dropout, Transformer.py:31 PreNormDrop, Transformer.py:41,46 FeedForward)
  float drop_p = 0.f;
  float attn_drop_p = 0.f;         // cfg['attn_dropout_rate']: attention probabilities (Attention.py:17,36) and proj_drop (Attention.py:19,40)
  unsigned long long drop_seed = 0;
};
// the table of h's tensors in ABI order; h->L must have its `layers` entries
std::vector<VitTensor> vit_tensors(prego_vit* h);

// ---- workspace layouts (each takes an Arena only so that prego_debug_vit_layout can log the blocks) --------------------------------
// the per-batch arena of the 16-bit inference paths (prego_vit_forward, prego_vit_forward_frames, prego_vit_step_pool(_bursts)): B windows
struct VitWs { size_t xb, enc, x, xn, q, k, vn, ao, f, x0, q0, ao0, xn0, f0, total; };
VitWs vit_ws(const VitDims& d, int B, Arena a = {});
// fp32-operand mode: fp32 rows everywhere, every block on every token
struct VitWs32 { size_t xc, enc, x, xn, qkv, ao, tmp, total; };
VitWs32 vit_ws32(const VitDims& d, int B, Arena a = {});
// n frames in front of a per-batch arena of wb windows: xb [n][din] 16-bit | enc [n][E] fp32 | argmax [n] int32 (the stream pool's step;
// prego_vit_forward_frames has none) | vit_ws(d, wb)
struct VitStepWs { size_t xb, enc, am, win; VitWs w; size_t total; };
VitStepWs vit_step_ws(const VitDims& d, int n, int wb, bool argmax, Arena a = {});
// training: what the forward keeps per layer, then the backward's scratch
struct VitBlockBufs { size_t xn1, q, k, vn, ao, xn2, f; bool keep; size_t x_in, st1, lse, x_mid, st2, u; };   // the last six: keep only
struct VitTrainWs {
  size_t xb, enc, x;                     // inputs as bf16, encoding GEMM output, residual stream (final value after forward)
  std::vector<VitBlockBufs> L;
  size_t dx, dxm, dxb, tmp, du, dub, dO, dqkv, delta, dencb, part, head, denc, vec;      // backward scratch; dencb: denc in bf16
  size_t total;
  int Mp, MTp;                           // rows of the layers' / of the encoding's weight gradients, padded to 64
};
VitTrainWs vit_train_ws(const VitDims& d, int B, Arena a = {});
// the AttentionLayer op: five activation buffers of M*D 16-bit elements (x, q, k, v, attention output) ...
struct AttnAct { size_t xb, q, k, vn, ao; };
struct AttnWs { AttnAct act; size_t qkv32, ao32, total; };               // handle: act, or (PREGO_F32) q | k | v rows [M, 3D] and the output
AttnWs attn_ws(int d_model, int batch, int len, bool f32, Arena a = {});
struct AttnTrainWs { AttnAct act; size_t lse, dyb, dO, dqkv, delta, dW, vec, total; int Mp; };
AttnTrainWs attn_train_ws(int d_model, int heads, int batch, int len, Arena a = {});
struct AttnOpWs { size_t wqkv, bqkv, wo; AttnAct act; size_t total; };   // stateless: the converted weights in front
AttnOpWs attn_op_ws(int d_model, int batch, int len, Arena a = {});

// ---- what the block runners and attention_layer_run fill a GemmEpi with ------------------------------------------------------------
static inline GemmEpi epi_qkv(bool f16, void* q, void* k, void* vn, int n_tok, int heads, int dh, int emb) {
  GemmEpi e{}; e.f16 = f16 ? 1 : 0;
  e.mode = EPI_QKV; e.q = q; e.k = k; e.vn = vn; e.n_tok = n_tok; e.heads = heads; e.dh = dh; e.emb = emb;
  e.q_scale = 1.0f / sqrtf((float)dh);                                   // Attention.py:14 (dh^-0.5), attn.py:44
  return e;
}
static inline GemmEpi epi_residual(bool f16) { GemmEpi r{}; r.f16 = f16 ? 1 : 0; r.mode = EPI_RESIDUAL; return r; }
static inline GemmEpi epi_gelu(bool f16, void* out_b) { GemmEpi g{}; g.f16 = f16 ? 1 : 0; g.mode = EPI_GELU_BF16; g.out_b = out_b; return g; }

// nn.Dropout(p) as the kernels take it: keep when hash >= thresh, scale the kept by 1 / (1 - p); p = 0: thresh 0 (no mask), scale 1
static inline unsigned drop_thresh(float p) { return p > 0.f ? (unsigned)((double)p * 4294967296.0) : 0u; }
static inline float drop_scale(float p) { return p > 0.f ? 1.f / (1.f - p) : 1.f; }
// one block's dropout: thr / sc = cfg['dropout'] (attention branch, after GELU, FFN output), athr / asc = cfg['attn_dropout_rate']
// (attention probabilities, proj_drop), a seed per site.  All zero: inference
struct VitBlockDrop { unsigned thr, athr; float sc, asc; unsigned long long seed_branch, seed_gelu, seed_ffn, seed_probs, seed_proj; };

// One pre-norm encoder block on the fp32 residual stream x [M = B*N, E] (Transformer.py:60-77): LN1, QKV GEMM, attention, x += proj,
// LN2, FF1 + GELU, x += FF2.  b.keep (training): x before each branch, the LayerNorm statistics, lse and the GELU pre-activation are
// kept as well.  0, 1 = the attention launch refused the head dim, or PREGO_EHIP with its message
int encoder_block_run(const prego_vit* h, const VitLayer& l, float* x, char* ws, const VitBlockBufs& b, const VitBlockDrop& dp, int B, int N,
                      int causal, hipStream_t s);
// the LAST block when only token 0 of its output is read; have_xn: the caller already wrote LayerNorm1(x) to w.xn and token 0 of every
// window to w.x0 (the token kernels do both), x is not read at all.  Leaves the block's token-0 output in w.x0 [B, E]
int encoder_block_token0(const prego_vit* h, const VitLayer& l, const float* x, char* ws, const VitWs& w, int B, int N, int causal,
                         hipStream_t s, bool have_xn = false);
// the encoder blocks on B windows whose tokens are written (fused: LayerNorm1(x) in w.xn and x0 instead of x), the last one on token 0
// only, then the head with its argmax (nullable).  who (nullable) prefixes the message
int blocks_and_head(const prego_vit* h, const char* who, char* ws, const VitWs& w, int B, int causal, bool fused, float* out_logits,
                    int32_t* am, hipStream_t s);

// what prego_vit_forward, _forward_frames and _forward_train refuse after their NULL checks, in this order: missing weights, batch,
// missing input, a workspace (`who`: how the entry's message calls it) of `have` < `need` bytes
int vit_check_call(const prego_vit* h, const char* who, int batch, const float* rgb, const float* flow, size_t need, size_t have);
// "training runs on bf16 handles": PREGO_EINVAL with that sentence for an fp16- / fp32-operand handle, else 0
static inline int refuse_non_bf16(const char* who, bool f16, bool f32) {
  return (f16 || f32) ? prego_fail_(PREGO_EINVAL, "%s on an fp16- / fp32-operand handle: training runs on bf16 handles", who) : 0;
}
// what the training entries share with the attention layer's (vit_train.cpp): the two k-major training GEMMs
int wgrad(const void* a_rows, int Mo, const void* b_rows, int No, int R, int Rp, float* out, float* bias_out, hipStream_t s);
int dgrad(const void* a_rows, int Ko, const void* w, int No, int R, float* out, hipStream_t s, void* out16 = nullptr);
