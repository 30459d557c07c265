// Unit-test entry points of the row-wise training kernels (include/prego_amd_debug.h, tests/test_gpu_rows.py): every entry checks the shape
// the kernel is written for, then calls the launch_* function of kernels.h exactly as the training steps do - the launcher's own choice of
// instantiation runs.  Debug library only.
#ifdef PREGO_DEBUG_ABI
#include "vit_handle.h"      // drop_thresh / drop_scale: the one conversion of a dropout probability the Transformer host files use

#define ROWS_BAD(...) return prego_fail_(PREGO_EINVAL, __VA_ARGS__)
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int prego_debug_ln_relu(int in_type, int out_type, const void* Y, const float* gamma, const float* beta, int nrows, int E, float eps,
                                   void* out, float* stats, float drop_p, uint64_t seed, int row0_abs, int relu, int arm_bf16, int arm_hid,
                                   int arm_G, void* arm_hx, uint32_t* arm_sync, prego_stream_t stream) {
  if (!Y || !gamma || !beta || !out) ROWS_BAD("debug ln_relu: NULL argument");
  if (nrows <= 0 || E <= 0 || E % 512 || E > 4096) ROWS_BAD("debug ln_relu: nrows %d, E %d (a multiple of 512 up to 4096)", nrows, E);
  if (!(drop_p >= 0.f && drop_p < 1.f)) ROWS_BAD("debug ln_relu: drop_p %g", (double)drop_p);
  // the type pairs launch_ln_relu reaches: fp32 -> fp32 / bf16 / fp16, bf16 -> bf16, fp16 -> fp16
  const bool ok = (in_type == 0 && out_type >= 0 && out_type <= 2) || (in_type == 1 && out_type == 1) || (in_type == 2 && out_type == 2);
  if (!ok) ROWS_BAD("debug ln_relu: in_type %d -> out_type %d is no instantiation", in_type, out_type);
  if (!al16(Y) || !al16(out) || !al16(gamma) || !al16(beta)) ROWS_BAD("debug ln_relu: 16-byte aligned rows");
  GruArm arm{nullptr, 0ull, 0u, nullptr};
  if (arm_hx) {
    if (!gru_hidden_supported(arm_bf16 != 0, arm_hid) || arm_G <= 0 || !al16(arm_hx)) ROWS_BAD("debug ln_relu: arm hid %d, G %d", arm_hid, arm_G);
    arm = gru_arm_desc(arm_bf16 != 0, arm_hid, arm_G, arm_hx, arm_sync);
  }
  launch_ln_relu(out_type != 0, Y, gamma, beta, nrows, E, eps, out, stats, drop_p, seed, row0_abs, (hipStream_t)stream, relu, in_type != 0,
                 out_type == 2, arm_hx ? &arm : nullptr);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_ln_relu_x2(const float* Y, const float* gamma, const float* beta, int nrows, int E, float eps, void* out,
                                      prego_stream_t stream) {
  if (!Y || !gamma || !beta || !out) ROWS_BAD("debug ln_relu_x2: NULL argument");
  if (nrows <= 0 || E <= 0 || E % 512 || E > 4096) ROWS_BAD("debug ln_relu_x2: nrows %d, E %d (a multiple of 512 up to 4096)", nrows, E);
  if (!al16(Y) || !al16(out) || !al16(gamma) || !al16(beta)) ROWS_BAD("debug ln_relu_x2: 16-byte aligned rows");
  launch_ln_relu_x2(Y, gamma, beta, nrows, E, eps, out, (hipStream_t)stream, nullptr);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_ln_relu_bwd(const float* dE, const float* Y, const float* stats, const float* gamma, const float* beta, int nrows,
                                       int E, float drop_p, uint64_t seed, int row0_abs, float* dY, void* dYb, float* part, float* dgb,
                                       int relu, int accumulate, prego_stream_t stream) {
  if (!dE || !Y || !stats || !gamma || !beta || !dY || !part || !dgb) ROWS_BAD("debug ln_relu_bwd: NULL argument");
  if (nrows <= 0 || E <= 0 || E % 256 || E > 4096) ROWS_BAD("debug ln_relu_bwd: nrows %d, E %d (a multiple of 256 up to 4096)", nrows, E);
  if (!(drop_p >= 0.f && drop_p < 1.f)) ROWS_BAD("debug ln_relu_bwd: drop_p %g", (double)drop_p);
  if (!al16(dE) || !al16(Y) || !al16(gamma) || !al16(beta) || !al16(dY) || ((uintptr_t)dYb & 7)) ROWS_BAD("debug ln_relu_bwd: aligned rows");
  const int nb = launch_ln_relu_bwd(dE, Y, stats, gamma, beta, nrows, E, drop_p, seed, row0_abs, dY, part, (hipStream_t)stream, relu, accumulate,
                                    dYb);
  launch_colsum_stage2(part, nb, 2 * E, dgb, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_colsum(int bf16, const void* src, int M, int N, float* part, float* out, prego_stream_t stream) {
  if (!src || !part || !out) ROWS_BAD("debug colsum: NULL argument");
  if (M <= 0 || N <= 0 || (M + 63) / 64 > 65535) ROWS_BAD("debug colsum: M %d, N %d", M, N);
  if (bf16) launch_colsum_bf16(src, M, N, part, out, (hipStream_t)stream);
  else launch_colsum((const float*)src, M, N, part, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_colsum_stage2(const float* part, int nb, int N, float* out, prego_stream_t stream) {
  if (!part || !out) ROWS_BAD("debug colsum_stage2: NULL argument");
  if (nb <= 0 || N <= 0) ROWS_BAD("debug colsum_stage2: nb %d, N %d", nb, N);
  launch_colsum_stage2(part, nb, N, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_transpose_convert(int in_bf16, int out_bf16, const void* src, int M, int N, int ld_src, void* dst, int Mpad,
                                             prego_stream_t stream) {
  if (!src || !dst) ROWS_BAD("debug transpose_convert: NULL argument");
  if (M <= 0 || N <= 0 || ld_src < N || Mpad < M || (Mpad + 31) / 32 > 65535) ROWS_BAD("debug transpose_convert: M %d, N %d, ld_src %d, Mpad %d", M, N, ld_src, Mpad);
  launch_transpose_convert(in_bf16 != 0, out_bf16 != 0, src, M, N, ld_src, dst, Mpad, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_gather_dlogits(int bf16, const float* const* dl_ptrs, const int32_t* rowoff, const int32_t* sorted_clip, int t_max,
                                          int nrows, int C, int Cpad, void* out, prego_stream_t stream) {
  if (!dl_ptrs || !rowoff || !sorted_clip || !out) ROWS_BAD("debug gather_dlogits: NULL argument");
  if (t_max <= 0 || nrows <= 0 || C <= 0 || Cpad < C) ROWS_BAD("debug gather_dlogits: t_max %d, nrows %d, C %d, Cpad %d", t_max, nrows, C, Cpad);
  launch_gather_dlogits(bf16 != 0, dl_ptrs, rowoff, sorted_clip, t_max, nrows, C, Cpad, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_build_hprev(int bf16, const float* Hraw, const int32_t* rowoff, int t_max, int nrows, int H, void* out,
                                       prego_stream_t stream) {
  if (!Hraw || !rowoff || !out) ROWS_BAD("debug build_hprev: NULL argument");
  if (t_max <= 0 || nrows <= 0 || H <= 0) ROWS_BAD("debug build_hprev: t_max %d, nrows %d, H %d", t_max, nrows, H);
  launch_build_hprev(bf16 != 0, Hraw, rowoff, t_max, nrows, H, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_relu_mask(const float* dHrelu, const float* Hraw, uint64_t n, float* out, prego_stream_t stream) {
  if (!dHrelu || !Hraw || !out) ROWS_BAD("debug relu_mask: NULL argument");
  if (n == 0) ROWS_BAD("debug relu_mask: n 0");
  launch_relu_mask(dHrelu, Hraw, (size_t)n, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_gru_bwd_step(int bf16, int t, int na, int na_next, int row_t, int row_tm1, int H, const float* dHout,
                                        const float* carry_in, const float* dhpart, const float* R, const float* Z, const float* Nn,
                                        const float* GHN, const float* Hraw, float* carry_out, float* dGI, float* dGH, void* dGIop, void* dGHop,
                                        prego_stream_t stream) {
  if (!dHout || !R || !Z || !Nn || !GHN || !carry_out || !dGI || !dGH || !dGIop || !dGHop) ROWS_BAD("debug gru_bwd_step: NULL argument");
  if (na <= 0 || H <= 0 || t < 0 || na_next < 0 || na_next > na || row_t < 0) ROWS_BAD("debug gru_bwd_step: t %d, na %d, na_next %d, H %d", t, na, na_next, H);
  if (na_next > 0 && (!carry_in || !dhpart)) ROWS_BAD("debug gru_bwd_step: carry_in / dhpart NULL with na_next %d", na_next);
  if (t > 0 && (!Hraw || row_tm1 < 0)) ROWS_BAD("debug gru_bwd_step: Hraw NULL with t %d", t);
  launch_gru_bwd_step(bf16 != 0, t, na, na_next, row_t, row_tm1, H, dHout, carry_in, dhpart, R, Z, Nn, GHN, Hraw, carry_out, dGI, dGH, dGIop,
                      dGHop, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_pad_convert(int out_type, const float* src, int rows_src, int cols_src, int ld_src, void* dst, int rows_dst,
                                       int cols_dst, prego_stream_t stream) {
  if (!src || !dst) ROWS_BAD("debug pad_convert: NULL argument");
  if (out_type < 0 || out_type > 2 || rows_src <= 0 || cols_src <= 0 || ld_src < cols_src || rows_dst < rows_src || cols_dst < cols_src)
    ROWS_BAD("debug pad_convert: type %d, src %d x %d (ld %d), dst %d x %d", out_type, rows_src, cols_src, ld_src, rows_dst, cols_dst);
  launch_pad_convert(out_type != 0, src, rows_src, cols_src, ld_src, dst, rows_dst, cols_dst, (hipStream_t)stream, out_type == 2);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_f32_to_bf16(const float* src, void* dst, uint64_t n, prego_stream_t stream) {
  if (!src || !dst) ROWS_BAD("debug f32_to_bf16: NULL argument");
  if (n == 0) ROWS_BAD("debug f32_to_bf16: n 0");
  launch_f32_to_bf16(src, dst, (size_t)n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_gelu_bwd(const float* df, const float* u, uint64_t n, float* du, void* du_bf16, float drop_p, uint64_t seed,
                                    prego_stream_t stream) {
  if (!df || !u || !du || !du_bf16) ROWS_BAD("debug gelu_bwd: NULL argument");
  if (n == 0 || n % 4) ROWS_BAD("debug gelu_bwd: n %llu (a multiple of 4)", (unsigned long long)n);
  if (!(drop_p >= 0.f && drop_p < 1.f)) ROWS_BAD("debug gelu_bwd: drop_p %g", (double)drop_p);
  if (!al16(df) || !al16(u) || !al16(du) || ((uintptr_t)du_bf16 & 7)) ROWS_BAD("debug gelu_bwd: aligned arrays");
  launch_gelu_bwd(df, u, (size_t)n, du, du_bf16, (hipStream_t)stream, drop_thresh(drop_p), drop_scale(drop_p), seed);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_mask_convert(const float* src, uint64_t n, float* out_f32, void* out_bf16, float drop_p, uint64_t seed, float drop2_p,
                                        uint64_t seed2, prego_stream_t stream) {
  if (!src || !out_bf16) ROWS_BAD("debug mask_convert: NULL argument");
  if (n == 0 || n % 4) ROWS_BAD("debug mask_convert: n %llu (a multiple of 4)", (unsigned long long)n);
  if (!(drop_p >= 0.f && drop_p < 1.f) || !(drop2_p >= 0.f && drop2_p < 1.f)) ROWS_BAD("debug mask_convert: drop_p %g, %g", (double)drop_p, (double)drop2_p);
  if (!al16(src) || !al16(out_f32) || ((uintptr_t)out_bf16 & 7)) ROWS_BAD("debug mask_convert: aligned arrays");
  launch_mask_convert(src, (size_t)n, out_f32, out_bf16, drop_thresh(drop_p), drop_scale(drop_p), seed, (hipStream_t)stream, drop_thresh(drop2_p),
                      drop_scale(drop2_p), seed2);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// the head kernels keep (E + 8 + C) / C floats in dynamic LDS: what a launch may ask for without an attribute is 64 KiB
static inline bool head_shape_ok(int B, int N, int E, int C) {
  return B > 0 && N > 0 && E > 0 && E % 4 == 0 && C > 0 && C < 65535 && (size_t)(E + 8 + C) * sizeof(float) <= 65536;
}

extern "C" int prego_debug_vit_head(const float* x, int B, int N, int E, const float* lnw, const float* lnb, const float* hw, const float* hb,
                                    int C, float* out, int32_t* argmax, prego_stream_t stream) {
  if (!x || !lnw || !lnb || !hw || !hb || !out) ROWS_BAD("debug vit_head: NULL argument");
  if (!head_shape_ok(B, N, E, C) || !al16(hw)) ROWS_BAD("debug vit_head: B %d, N %d, E %d, C %d", B, N, E, C);
  launch_vit_head(x, B, N, E, lnw, lnb, hw, hb, C, out, (hipStream_t)stream, argmax);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_vit_head_bwd(const float* x, const float* dlogits, int B, int N, int E, int C, const float* lnw, const float* lnb,
                                        const float* hw, float* dx, float* scratch, float* g_lnw, float* g_lnb, float* g_hw, float* g_hb,
                                        prego_stream_t stream) {
  if (!x || !dlogits || !lnw || !lnb || !hw || !dx || !scratch || !g_lnw || !g_lnb || !g_hw || !g_hb) ROWS_BAD("debug vit_head_bwd: NULL argument");
  if (!head_shape_ok(B, N, E, C)) ROWS_BAD("debug vit_head_bwd: B %d, N %d, E %d, C %d", B, N, E, C);
  launch_vit_head_bwd(x, dlogits, B, N, E, C, lnw, lnb, hw, dx, scratch, g_lnw, g_lnb, g_hw, g_hb, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_vit_tokens(const float* enc, const float* cls, const float* pe, int B, int T, int E, float* x, float drop_p,
                                      uint64_t seed, prego_stream_t stream) {
  if (!enc || !cls || !pe || !x) ROWS_BAD("debug vit_tokens: NULL argument");
  if (B <= 0 || T <= 0 || E <= 0 || !(drop_p >= 0.f && drop_p < 1.f)) ROWS_BAD("debug vit_tokens: B %d, T %d, E %d, drop_p %g", B, T, E, (double)drop_p);
  launch_vit_tokens(enc, cls, pe, B, T, E, x, (hipStream_t)stream, drop_thresh(drop_p), drop_scale(drop_p), seed);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_debug_vit_tokens_bwd(const float* dx, int B, int T, int E, float* denc, float* g_pe, float* g_cls, float drop_p, uint64_t seed,
                                          prego_stream_t stream) {
  if (!dx || !denc || !g_pe || !g_cls) ROWS_BAD("debug vit_tokens_bwd: NULL argument");
  if (B <= 0 || T <= 0 || E <= 0 || (E + 255) / 256 > 65535 || !(drop_p >= 0.f && drop_p < 1.f))
    ROWS_BAD("debug vit_tokens_bwd: B %d, T %d, E %d, drop_p %g", B, T, E, (double)drop_p);
  launch_vit_tokens_bwd(dx, B, T, E, denc, g_pe, g_cls, (hipStream_t)stream, drop_thresh(drop_p), drop_scale(drop_p), seed);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// launch_oad_loss on the caller's DEVICE tables: prego_oad_loss_reduce stages at most 4096 clips, so the kernel's serial path (more clips
// than its LDS table holds) is reachable from here alone
extern "C" int prego_debug_oad_loss(const float* const* logit_ptrs, const float* const* target_ptrs, const int32_t* lens, int n_clips, int C,
                                    int sum, float* loss_out, float* const* dlogit_ptrs, float grad_scale, prego_stream_t stream) {
  if (!logit_ptrs || !target_ptrs || !lens || !loss_out) ROWS_BAD("debug oad_loss: NULL argument");
  if (n_clips <= 0 || C <= 0 || C > 128) ROWS_BAD("debug oad_loss: %d clips, %d classes (1..128)", n_clips, C);
  launch_oad_loss(logit_ptrs, target_ptrs, lens, n_clips, C, loss_out, dlogit_ptrs, grad_scale, (hipStream_t)stream, sum != 0);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
#endif  // PREGO_DEBUG_ABI
