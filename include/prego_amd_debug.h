/* Probe / unit-test entry points of the MI355X PREGO library - NOT part of the product ABI (include/prego_amd.h).
 * They exist only in libprego_amd_debug.so = the same sources built with -DPREGO_DEBUG_ABI (python -m prego_amd.build builds both),
 * and serve the kernel-level GPU tests (tests/test_gpu_gemm.py, tests/test_gpu_gemm_tn.py, the attention kernel tests) and the measurement scripts under
 * scripts/.  Nothing under prego_amd/ calls them. */
#ifndef PREGO_AMD_DEBUG_H
#define PREGO_AMD_DEBUG_H
#include "prego_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Debug / probe: only the head kernel over n_slots equal slots x n_steps steps of caller-supplied relu(h) rows (16-bit, the handle's
 * operand type, time-major packed [n_steps][n_slots][hidden]); out [n_slots][n_steps][n_classes], argmax [n_slots][n_steps]. */
int prego_debug_head_only(prego_miniroad* h, int n_slots, int n_steps, const void* h_relu, float* out, int32_t* argmax,
                          const void* rowmap /* nullable: int32 (clip, frame) per row, as the pack kernel writes it */, prego_stream_t stream);

/* Debug only (env PREGO_GRU_STAMPS=1 at create): per-phase shader-cycle sums of workgroup 0 / wave 0 of the
 * recurrence kernel: out8[0..4] = rest of gather + mfma, step top -> first gather segment valid, reduce+barrier, gates+publish, outputs; [5] = gather retry rounds;
 * [6] = time steps.  Synchronises the device. */
int prego_miniroad_debug_stamps(prego_miniroad* h, unsigned long long* out8);

/* Probes of DESIGN.md section 5c (scripts/probes/xcd_overlap_probe.py), not product entry points: ONLY the recurrence kernel over
 * n_steps steps of n_slots equal slots dealt to gd groups (0 = all; gi: device 16-bit [n_steps * n_slots][3 H], h_relu: device 16-bit
 * [rows][H]); and the projection GEMM as a persistent worker that leaves XCDs below xcd_lo at once and claims 256 x 256 tiles from
 * *counter (device word, zero at launch). */
int prego_debug_recurrence_only(prego_miniroad* h, int n_slots, int n_steps, int gd, const void* gi, void* h_relu, prego_stream_t stream);
int prego_debug_gemm_worker(const void* A, const void* B, const float* bias, float* C, int M, int N, int K, int xcd_lo,
                            unsigned* counter, int grid, prego_stream_t stream);

/* The split pass's start handshake (DESIGN 5b "fail-safe") under test, and the replay entries counter collection needs.  One shot: applies
 * to the NEXT split pass of the handle.
 *   mode 1: the recurrence launch is withheld - the feed-forward launch's handshake wait runs out, it leaves without having written anything
 *           and prego_miniroad_forward re-runs the call as a chunked pass (tests/test_gpu_split.py)
 *   mode 2: the feed-forward launch is withheld (the recurrence's leader gives up; same outcome)
 *   mode 3: ONLY the feed-forward launch, handshake pre-decided and the recurrence's chunk counters pre-armed: the launch runs alone at full
 *           length (rocprofv3 --pmc serialises dispatches, so the pair can never be profiled together).  No head, outputs untouched
 *   mode 4: ONLY the recurrence launch on whatever (finite) rows an earlier pass left in the GI ring; no head, outputs untouched
 * split_state: fallbacks = calls re-run chunked behind a failed handshake, fails = failed handshakes (3 = chunked for good),
 * skip = eligible calls still to be kept chunked by the back-off, split_env = the handle's PREGO_SPLIT_PASS state (-1 auto, 0 never, R). */
int prego_debug_split_fault(prego_miniroad* h, int mode);
int prego_debug_split_state(const prego_miniroad* h, int64_t* fallbacks, int32_t* fails, int64_t* skip, int32_t* split_env);
/* unit-test hook: sets the handle's timeout word on the device (stream-ordered), as a recurrence / BPTT kernel that gave up would:
 * prego_miniroad_check then reports PREGO_ETIMEOUT and clears it; until then prego_miniroad_adamw_step changes nothing. */
int prego_debug_set_abort(prego_miniroad* h, unsigned value, prego_stream_t stream);
/* unit-test hook: how many hipMalloc calls / host-side stream or event waits the MiniROAD host code of this library has made so far in
 * this process (prego_miniroad_check's own synchronisation counts).  A test calls it around a hot call to hold "forward() allocates
 * nothing and waits for nothing" to zero (include/prego_amd.h, conventions). */
int prego_debug_alloc_count(int64_t* device_mallocs, int64_t* host_waits);
/* A/B switch: on != 0 makes every following MiniROADA backward of this library run the anticipation head's backward over every packed row
 * instead of the device-side span of rows with gradient (prego_miniroad_set_anticipation_grads).  Process-wide. */
int prego_debug_ant_full_span(int on);
/* probe: a synthetic neighbour on XCDs >= xcd_lo for `ms` milliseconds - kind 1: back-to-back MFMAs on registers, no
 * memory traffic; kind 2: streaming reads of read_buf (+ one write per eight reads into write_buf), no matrix work; kind 3: both.
 * Launched on its own stream beside a replayed recurrence launch (prego_debug_split_fault mode 4) it separates what that launch loses to
 * power / clocks from what it loses to the fabric.  bytes: size of each of the two buffers (>= 1 MiB).  sink: one device float. */
int prego_debug_hog(int kind, int xcd_lo, int ms, const void* read_buf, void* write_buf, size_t bytes, float* sink, prego_stream_t stream);

/* Debug / microbenchmark only: C[M,N] fp32 = A[M,K] bf16 . B[N,K]^T bf16 + bias with a chosen kernel variant
 * (0 = 128x128, 1 = 256x128 three-stage, 9 = 256x256 two-stage, 12 = the ping-pong kernel = the production kernel of the projections,
 * 30 = the eight-wave split-K workgroup; scripts/gemm_bench.py).  N % 128 == 0, K % 64 == 0.  A variant forces its kernel: on a shape
 * that kernel does not take (N % 256 or K < 128 for 9 / 12, more than 256 tiles for 30) nothing is launched and 0 is returned.
 * PREGO_EINVAL for any other variant. */
int prego_debug_gemm_bf16(int variant, const void* A, const void* B, const float* bias, float* C, int M, int N, int K,
                          prego_stream_t stream);

/* Unit test only (tests/test_gemm_dispatch_cpu.py): which kernel an NT product runs on - the answer of the one chooser behind
 * launch_gemm_bf16_nt, launch_gemm_bf16_nt_epi and the MiniROAD projections, without touching a device.  entry: 0 = launch_gemm_bf16_nt,
 * 1 = launch_gemm_bf16_nt_epi, 2 = the MiniROAD forward's projection with fp16 operands or a 16-bit C.  mode: the epilogue (0 store fp32,
 * 1 residual, 2 gelu 16-bit, 3 store 16-bit, 4 qkv, 5 tokens); dh, emb: the qkv epilogue's head and embedding widths.  knobs: bit 0
 * PREGO_GEMM_NO_BIG, bit 1 PREGO_GEMM_NO_SPLITK, bit 2 PREGO_GEMM_NO_PINGPONG.  Returns -1 nothing launched (M <= 0), 0 the 128x128
 * kernel, 1 256x128 three-stage, 2 256x256 two-stage, 3 ping-pong, 4 the eight-wave split-K workgroup. */
int prego_debug_gemm_nt_choice(int entry, int M, int N, int K, int lda, int ldb, int has_bias, int f16, int train_splitk, int mode, int dh,
                               int emb, int knobs);

/* Unit test only (tests/test_gru_choice_cpu.py): which recurrence kernel a launch would run, without touching a device (gru_choose,
 * csrc/gru_recurrence.hip).  entry: 0 = launch_gru_recurrence, 1 = launch_gru_recurrence_x2, 2 = launch_gru_recurrence_pass.  operand:
 * 0 bf16, 1 fp16, 2 fp32 (ignored by entry 1).  train: the launch keeps gate activations / raw state.  stamps: a stamp buffer is
 * given.  mt_spec: the value of PREGO_GRU_MT_SPEC (-1 = unset; an argument here because the environment is read once per process).
 * ready: entry 1: the scale pointer is given; entry 2: chunk counters and rendezvous words are given.  Returns -1 = refused, -2 = a
 * choice the launch table has no kernel for (a bug: the chooser's range is the table), otherwise
 * family (0 classic, 1 multi-tile, 2 fp16x2, 3 pass) | operand << 2 | UT << 4 | NCT << 6 | TRAIN << 9 | GI16 << 10 | SPEC << 11 |
 * hid << 12; *grid and *lds (nullable) receive the launch's workgroups and dynamic LDS bytes. */
int prego_debug_gru_choice(int entry, int operand, int hid, int nct, int G, int gi_bf16, int train, int no_mt, int stamps, int rows,
                           int mt_spec, int Gd, int ready, int* grid, int* lds);
/* Unit test only: the recurrence's exchange layout and sizes (csrc/gru_tile.h), the functions the kernels and the host both use.
 * what 0: byte offset of (clip column a, contraction index b, tile c) in a group's plane laid out for `tiles` tiles of `wb`-byte
 * elements; 1: the contraction index held at (fragment a, lane b, byte c); 2: the clip column of lane b; 3: bytes of one plane for
 * hidden size a.  what 10 .. 14: gru_hx_bytes(bf16 = wb == 2, hid = a, G = b), gru_x2_hx_bytes(a, b), gru_group_size(wb == 2, a),
 * gru_hidden_supported(wb == 2, a), slots a handle of b groups plans for (c != 0: an fp16x2 handle). */
long long prego_debug_gru_hx_offset(int what, int wb, int tiles, int a, int b, int c);

/* Unit test only (tests/test_gpu_gemm_tn.py): the training GEMMs on k-major operands exactly as the training steps launch them
 * (launch_gemm_bf16_tn chooses between the split-K and the plain kernel itself).  C[M,N] = op(A) . op(B) (+ bias[n]); ta: A is stored
 * [K][M] with lda elements per k row, else [M][K]; tb: B is stored [K][N], else [N][K]; 16-bit operands are bf16.  k_valid <= K: the
 * contraction rows of a k-major operand that exist.  C16 (nullable): device bf16 [M][ldc], written INSTEAD of the fp32 C.  colsum_out
 * (nullable, ta only): fp32 [M] column sums of A over k.  PREGO_EINVAL, nothing launched, for a shape the launcher refuses. */
int prego_debug_gemm_tn(int ta, int tb, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, void* C16, int ldc,
                        int M, int N, int K, int k_valid, float* colsum_out, prego_stream_t stream);

/* Unit test only (tests/test_gpu_gemm.py): the production dispatcher of the projections, launch_gemm_bf16_nt: C[M,N] fp32 = A[M,K] .
 * B[N,K]^T + bias, operands bf16 or (f16 != 0) IEEE fp16; train_splitk: the keeping training forward's flag.  N % 128 == 0, K % 64 == 0,
 * M > 0, lda, ldb >= K, ldc >= N. */
int prego_debug_gemm_nt(int f16, int train_splitk, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc,
                        int M, int N, int K, prego_stream_t stream);

/* Debug / unit test only: the attention backward kernels alone.  qs (= q * dh^-0.5), k, v: device bf16 [batch, heads, len, dh];
 * o, dout: device bf16 [batch, len, heads*dh]; lse: device fp32 [batch, heads, len] log-sum-exp of the scaled scores;
 * dqkv: device bf16 [batch*len, 3*heads*dh] (dq | dk | dv, dq wrt the unscaled q).  Synchronises the stream. */
int prego_debug_attention_bwd(int batch, int len, int heads, int dh, int causal, const void* qs, const void* k, const void* v,
                              const void* o, const void* dout, const float* lse, void* dqkv, prego_stream_t stream);

/* Debug / unit test only: the attention forward kernel alone (every head-dim / shape variant is reachable from here).
 * qs (= q * dh^-0.5): device bf16 [batch, heads, n_query, dh], queries at sequence positions 0 .. n_query-1; k, v: device bf16
 * [batch, heads, len, dh]; out: device bf16 [batch, n_query, heads*dh]; lse: device fp32 [batch, heads, n_query] or NULL.
 * Synchronises the stream. */
int prego_debug_attention_fwd(int batch, int n_query, int len, int heads, int dh, int causal, const void* qs, const void* k,
                              const void* v, void* out, float* lse, prego_stream_t stream);

/* Unit test only (tests/test_gpu_vit_stream_pool.py): the Transformer stream pool's token kernel alone, on the pool as it stands (no
 * frame is committed): x_out device fp32 [n][window_size + 1][embedding_dim] = the residual-stream rows of the windows of `slots` (HOST
 * int32 [n], as prego_vit_step_pool takes them); neither the fused LayerNorm output nor the token-0 copy is written. */
int prego_debug_vit_ring_tokens(prego_vit_stream_pool* p, int n, const int32_t* slots, float* x_out, prego_stream_t stream);

/* Unit test only (tests/test_gpu_vit_bursts.py): the two burst kernels of the Transformer stream pool alone.  slots / counts: HOST int32
 * [n] as prego_vit_step_pool_bursts takes them; enc: device fp32 [sum(counts)][embedding_dim], the caller's rows in place of the
 * encoding GEMM's.  _tokens: x_out device fp32 [sum(counts)][window_size + 1][embedding_dim], one window per packed row out of the rings
 * as they stand and enc; nothing is committed.  _commit: the rows go into the rings and the ring words advance; nothing else runs. */
int prego_debug_vit_burst_tokens(prego_vit_stream_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* enc,
                                 float* x_out, prego_stream_t stream);
int prego_debug_vit_burst_commit(prego_vit_stream_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* enc,
                                 prego_stream_t stream);

/* Unit test only (tests/test_stream_image_cpu.py), no device: the slot images' validity rule (csrc/pool_image.h: pool_image_fault) on HOST
 * words, so that the Python model `image_fault` is held against the function the restore kernel evaluates.  geometry6: kind | dim |
 * window_size | n_classes | vote window | max_events; tag: the image's 16 tag words; rec: the first 4 + n_classes (rounded up to 4) words
 * of its record.  Returns the clause bits, -1 for a NULL argument. */
int prego_debug_pool_image_fault(const int32_t* geometry6, const int32_t* tag, const int32_t* rec);

/* Unit test only (tests/test_vit_tensor_table_cpu.py), no device: entry i of the ViTEnc handle's tensor table, the one enumeration that
 * prego_vit_set_weights, the gradient list and the AdamW step walk.  dims: HOST int32 [8] = d_rgb, d_flow, embedding_dim, hidden_dim (mlp),
 * num_heads, num_layers, window_size, n_classes.  rows x cols as nn.Linear stores a matrix, 1 x n for a vector; is_matrix: the handle keeps
 * a 16-bit operand copy.  Returns the number of entries (i outside the table writes nothing), -1 for a NULL argument. */
int prego_debug_vit_tensor(const int32_t* dims, int i, int32_t* rows, int32_t* cols, int32_t* is_matrix);

/* Unit test only (tests/test_vit_layout_cpu.py), no device: the blocks of a Transformer workspace layout, in order.  dims as above
 * (the attention layer's kinds read embedding_dim as d_model and num_heads).  kind 0: prego_vit_forward in 16 bits, a = batch; 1: the same
 * on a PREGO_F32 handle; 2: prego_vit_forward_frames, a = n_frames, b = windows_per_batch; 3: prego_vit_step_pool, a = n_active; 4: ViTEnc
 * training, a = batch; 5 / 6: the attention handle's forward in 16 bits / PREGO_F32, a = batch, b = len; 7: the attention handle's
 * training; 8: the stateless attention op.  offsets: HOST uint64 [cap]: offset and bytes asked for of block i at [2i], [2i + 1], then the
 * total.  Returns the number of blocks; -1: a NULL argument, an unknown kind, or cap below 2 * blocks + 1. */
int prego_debug_vit_layout(int kind, const int32_t* dims, int a, int b, uint64_t* offsets, int cap);

/* ---- Unit test only (tests/test_gpu_rows.py): the element-wise and small-reduction kernels of the training steps, each alone, through the
 * launch_* function of csrc/kernels.h the training steps call (the launcher picks the instantiation).  Every pointer is a device pointer.
 * Each entry returns PREGO_EINVAL and launches nothing for a NULL it needs or a shape its kernel is not written for; "reads" / "writes" below
 * is the contract the tests hold the kernels to: nothing outside what is named is read (NaN there must not reach an output) or written.
 * A dropout probability p becomes the kernels' threshold (unsigned)((double)p 2^32) and scale 1.f / (1.f - p); the mask of element i is
 * hash(seed, i) >= threshold (csrc/common.h: dropout_keep_).  Types: 0 fp32, 1 bf16, 2 IEEE fp16; fp16 stores saturate at +-65504. */

/* LayerNorm (biased variance, eps inside the root) [+ ReLU if relu] [+ dropout(drop_p) on element index (row0_abs + r) E + c] of nrows rows
 * of E values.  E a multiple of 512, <= 4096; (in_type, out_type) one of (0,0) (0,1) (0,2) (1,1) (2,2).  Reads Y [nrows][E], gamma, beta
 * [E].  Writes out [nrows][E] and, when stats is given, stats [nrows][2] = (mean, 1 / sqrt(var + eps)) per row.  arm_hx non-NULL: also
 * re-arms a recurrence's exchange buffers as gru_arm_desc(arm_bf16, arm_hid, arm_G) describes them: with W = gru_hx_bytes / 8 words per
 * buffer, words [0, W) of arm_hx := 0x40004000 (16-bit operands) or 0x40000000 (fp32), words [W, 2 W) := 0, arm_sync [0, 16) := 0. */
int prego_debug_ln_relu(int in_type, int out_type, const void* Y, const float* gamma, const float* beta, int nrows, int E, float eps, void* out,
                        float* stats, float drop_p, uint64_t seed, int row0_abs, int relu, int arm_bf16, int arm_hid, int arm_G, void* arm_hx,
                        uint32_t* arm_sync, prego_stream_t stream);
/* LayerNorm + ReLU of fp32 rows into split rows: out [nrows][2 E] fp16 = [hi | lo], hi = fp16_sat(v), lo = fp16_sat(v - hi).  Shapes and reads
 * as above; no dropout, no statistics. */
int prego_debug_ln_relu_x2(const float* Y, const float* gamma, const float* beta, int nrows, int E, float eps, void* out, prego_stream_t stream);
/* Dropout / ReLU / LayerNorm backward + the column sums of its partials, as both training steps run them.  With xhat = (Y - mu) rstd from
 * stats [nrows][2], pre = xhat gamma + beta, d = dE [pre > 0 if relu] [dropout mask and scale as the forward, same (seed, row0_abs)],
 * dxh = d gamma:  dY (+)= rstd (dxh - mean_E(dxh) - xhat mean_E(dxh xhat)) (accumulate: added to what dY holds), dYb (nullable) = bf16 of
 * the stored dY, dgb [2 E] = (sum_rows d xhat | sum_rows d).  E a multiple of 256, <= 4096.  Reads dE, Y [nrows][E], stats, gamma, beta,
 * and dY when accumulate.  Writes dY, dYb [nrows][E], dgb, and part [ceil(nrows / 4)][2][E] (scratch). */
int prego_debug_ln_relu_bwd(const float* dE, const float* Y, const float* stats, const float* gamma, const float* beta, int nrows, int E,
                            float drop_p, uint64_t seed, int row0_abs, float* dY, void* dYb, float* part, float* dgb, int relu, int accumulate,
                            prego_stream_t stream);
/* out [N] = column sums of src [M][N] (fp32, or bf16 with fp32 accumulation) in a fixed order; part: scratch [ceil(M / 64)][N], written.
 * _stage2: out [N] = sum over b < nb of part [b][N] (16 contiguous slices of ceil(nb / 16) partials, slice sums added in order). */
int prego_debug_colsum(int bf16, const void* src, int M, int N, float* part, float* out, prego_stream_t stream);
int prego_debug_colsum_stage2(const float* part, int nb, int N, float* out, prego_stream_t stream);
/* dst [N][Mpad] = src [M][ld_src]^T converted (bf16 stores round to nearest even); columns M .. Mpad-1 of dst are ZERO.  Reads rows
 * [0, M) and columns [0, N) of src only; writes exactly dst [N][Mpad]. */
int prego_debug_transpose_convert(int in_bf16, int out_bf16, const void* src, int M, int N, int ld_src, void* dst, int Mpad,
                                  prego_stream_t stream);
/* Packed time-major rows: rowoff [t_max + 1] the prefix sums of the live clips per step (clips sorted by length, descending), row
 * rowoff[t] + i = step t of sorted clip i.  gather_dlogits: out [nrows][Cpad] (fp32 or bf16) = dl_ptrs[sorted_clip[i]][t][0 .. C), zeros in
 * columns C .. Cpad-1.  build_hprev: out [nrows][H] = Hraw [rowoff[t - 1] + i][H] (the same clip one step earlier), zeros at t = 0. */
int prego_debug_gather_dlogits(int bf16, const float* const* dl_ptrs, const int32_t* rowoff, const int32_t* sorted_clip, int t_max, int nrows,
                               int C, int Cpad, void* out, prego_stream_t stream);
int prego_debug_build_hprev(int bf16, const float* Hraw, const int32_t* rowoff, int t_max, int nrows, int H, void* out, prego_stream_t stream);
/* out [n] = Hraw > 0 ? dHrelu : 0 */
int prego_debug_relu_mask(const float* dHrelu, const float* Hraw, uint64_t n, float* out, prego_stream_t stream);
/* One reverse step of BPTT, element-wise part, for clips b < na and units j < H (formulas: csrc/train.hip).  Reads rows row_t .. row_t + na-1
 * of dHout, R, Z, Nn, GHN [rows][H]; carry_in, dhpart [na_next][H] (rows b >= na_next are NOT read: dh = dHout there); rows row_tm1 ..
 * of Hraw only when t > 0 (t = 0: hprev = 0, Hraw is not read).  Writes carry_out [na][H], rows row_t .. of dGI, dGH [rows][3 H] fp32 and
 * of dGIop, dGHop (bf16, or fp32 when !bf16) - nothing else. */
int prego_debug_gru_bwd_step(int bf16, int t, int na, int na_next, int row_t, int row_tm1, int H, const float* dHout, const float* carry_in,
                             const float* dhpart, const float* R, const float* Z, const float* Nn, const float* GHN, const float* Hraw,
                             float* carry_out, float* dGI, float* dGH, void* dGIop, void* dGHop, prego_stream_t stream);
/* dst [rows_dst][cols_dst] (out_type) = src [rows_src][ld_src] in its rows_src x cols_src corner, zeros elsewhere.  Reads that corner only. */
int prego_debug_pad_convert(int out_type, const float* src, int rows_src, int cols_src, int ld_src, void* dst, int rows_dst, int cols_dst,
                            prego_stream_t stream);
/* dst [n] bf16 = src [n], round to nearest even */
int prego_debug_f32_to_bf16(const float* src, void* dst, uint64_t n, prego_stream_t stream);
/* du [n] = mask_scale(df) (Phi(u) + u phi(u)), exact-erf GELU's derivative; du_bf16 [n] = bf16(du).  n a multiple of 4. */
int prego_debug_gelu_bwd(const float* df, const float* u, uint64_t n, float* du, void* du_bf16, float drop_p, uint64_t seed,
                         prego_stream_t stream);
/* out_f32 (nullable) / out_bf16 [n] = src masked and scaled by (drop_p, seed), then by (drop2_p, seed2).  n a multiple of 4. */
int prego_debug_mask_convert(const float* src, uint64_t n, float* out_f32, void* out_bf16, float drop_p, uint64_t seed, float drop2_p,
                             uint64_t seed2, prego_stream_t stream);
/* The Transformer head on token 0 of each of B windows of N tokens: out [B][C] = LN(x[b, 0, :]; lnw, lnb, eps 1e-5) hw^T + hb, argmax
 * (nullable) [B] = the first maximum.  Reads row 0 of every window only.  (E + 8 + C) floats must fit 64 KiB; E a multiple of 4. */
int prego_debug_vit_head(const float* x, int B, int N, int E, const float* lnw, const float* lnb, const float* hw, const float* hb, int C,
                         float* out, int32_t* argmax, prego_stream_t stream);
/* Its backward, any C the forward takes: dx [b, 0, :] = LayerNorm backward of dlogits[b] hw (rows 1 .. N-1 of dx are NOT written),
 * g_lnw, g_lnb [E], g_hw [C][E], g_hb [C] summed over the windows in window order; scratch [3][B][E] is written. */
int prego_debug_vit_head_bwd(const float* x, const float* dlogits, int B, int N, int E, int C, const float* lnw, const float* lnb,
                             const float* hw, float* dx, float* scratch, float* g_lnw, float* g_lnb, float* g_hw, float* g_hb,
                             prego_stream_t stream);
/* x [B][T + 1][E] = mask_scale((n < T ? enc [b][n] : cls) + pe [n]), mask index = the element's index in x.  _bwd, the same mask on dx:
 * denc [B][T][E] = the masked dx rows n < T, g_pe [T + 1][E] = their sum over b in order, g_cls [E] = g_pe [T]. */
int prego_debug_vit_tokens(const float* enc, const float* cls, const float* pe, int B, int T, int E, float* x, float drop_p, uint64_t seed,
                           prego_stream_t stream);
int prego_debug_vit_tokens_bwd(const float* dx, int B, int T, int E, float* denc, float* g_pe, float* g_cls, float drop_p, uint64_t seed,
                               prego_stream_t stream);
/* The loss kernel on DEVICE tables (logit_ptrs, target_ptrs, dlogit_ptrs [n_clips] device pointers, lens [n_clips] int32), any number of
 * clips: the product entry stages at most 4096, so the kernel's one-wave path for more clips than that is reached from here alone.  Reads
 * the LAST row of each clip's logits and target [lens][C]; writes loss_out [1] and, when dlogit_ptrs is given, all lens x C values of each
 * clip's dlogits (zeros in front of the last row).  C in 1..128. */
int prego_debug_oad_loss(const float* const* logit_ptrs, const float* const* target_ptrs, const int32_t* lens, int n_clips, int C, int sum,
                         float* loss_out, float* const* dlogit_ptrs, float grad_scale, prego_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PREGO_AMD_DEBUG_H */
