// Private to the ViTEnc host files (vit_host.cpp, vit_stream.cpp): the handle, the per-batch workspace layout of the inference entry
// points and the two encoder-block runners that cross files.  Which file defines what:
//   vit_host.cpp      create / destroy, weight setters, vit_ws, encoder_block, encoder_block_token0, forward, forward_frames, training
//   vit_stream.cpp    the Transformer stream pool: prego_vit_stream_pool_*, prego_vit_step_pool(_bursts) (kernels: vit_stream.hip)
#pragma once
#include "host_common.h"

#include <vector>

struct VitLayer {
  float *ln1_w, *ln1_b, *proj_b, *ln2_w, *ln2_b, *ff1_b, *ff2_b;
  void *qkv_w, *proj_w, *ff1_w, *ff2_w;    // bf16
  float *qkv_w32 = nullptr, *proj_w32 = nullptr, *ff1_w32 = nullptr, *ff2_w32 = nullptr;   // PREGO_F32 handles only
};
struct prego_vit {
  int d_rgb, d_flow, emb, mlp, heads, layers, window, ncls;
  void* enc_w = nullptr; float* enc_b = nullptr; float* cls = nullptr; float* pe = nullptr;
  std::vector<VitLayer> L;
  float *lnf_w = nullptr, *lnf_b = nullptr, *head_w = nullptr, *head_b = nullptr;
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

// the per-batch arena of the 16-bit inference paths (prego_vit_forward, prego_vit_forward_frames, prego_vit_step_pool(_bursts)): B windows
struct VitWs { size_t xb, enc, x, xn, q, k, vn, ao, f, x0, q0, ao0, xn0, f0, total; };
VitWs vit_ws(const prego_vit* h, int B);

// one pre-norm encoder block on the fp32 residual stream x [M = B*N, E] (Transformer.py:60-77)
int encoder_block(const prego_vit* h, const VitLayer& l, float* x, char* ws, const VitWs& w, int B, int N, int causal, hipStream_t s);
// the LAST block when only token 0 of its output is read; have_xn: the caller already wrote LayerNorm1(x) to w.xn and token 0 of every
// window to w.x0 (the token kernels do both), x is not read at all.  Leaves the block's token-0 output in w.x0 [B, E]
int encoder_block_token0(const prego_vit* h, const VitLayer& l, const float* x, char* ws, const VitWs& w, int B, int N, int causal,
                         hipStream_t s, bool have_xn = false);
