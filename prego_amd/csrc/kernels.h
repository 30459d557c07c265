// Host-visible declarations of the kernel launchers (implemented in the .hip files).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <mutex>

// Tuning / A-B / diagnostic environment knobs (PREGO_SPLIT_LAG*, PREGO_PLAN_SLOTS, PREGO_GRU_STAMPS, PREGO_ATTN_NW, ...): only the
// DEBUG library (libprego_amd_debug.so, -DPREGO_DEBUG_ABI) reads them; in the product library this returns nullptr and every one of
// them stays at its default.  The product library reads exactly four switches between code paths that are both held by the driver-run
// tests: PREGO_SPLIT_PASS, PREGO_NO_XCD_OVERLAP, PREGO_GRU_NO_LOCAL, PREGO_GRU_NO_MT (include/prego_amd.h).  Defined in miniroad.cpp.
const char* prego_tune_env(const char* name);

// One-time per-DEVICE setup at a launch site (hipFuncSetAttribute, symbol addresses): function attributes and __device__
// symbols belong to the device that was current when they were set / resolved, so a process that drives several GPUs
// needs them once per device, and the first calls may race between host threads.
struct DeviceOnce {
  std::mutex mu;
  bool done[64] = {};
  template <class F> int run(F&& f) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) { f(); return 0; }
    std::lock_guard<std::mutex> g(mu);
    if (!done[dev]) { f(); done[dev] = true; }
    return dev;
  }
};

// host-visible copy of the slot schedule descriptor (layout identical to common.h's SlotPlan)
#ifndef PREGO_HAVE_SLOTPLAN
struct SlotPlan {
  const int* rowoff; const int* nact; const int* seg_off; const int* seg_clip; const int* seg_start; const int* blk_step;
  int s_max; int n_slots;
};
#define PREGO_HAVE_SLOTPLAN 1
#endif

// Start handshake of a split pass (DESIGN 5b "fail-safe"): both persistent launches must be resident TOGETHER, or neither may touch
// memory.  `word` (device, zeroed per pass) is decided ONCE by compare-and-swap: 1 = GO (the recurrence's leader has seen P workgroups on
// each of its XCDs and at least one feed-forward workgroup on each of the others), 2 = FAIL (somebody's bounded wait ran out: a
// dispatch-serialising profiler, another tenant on the XCDs).  Whoever decides also writes (seq << 2) | state to the pinned host word
// the calling thread polls: on FAIL both launches leave without having written anything and the host runs the chunked pass instead.
struct PassHandshake {
  unsigned* word;               // device: 0 undecided, 1 GO, 2 FAIL
  unsigned* ff_here;            // device [8]: feed-forward workgroups that have started, per XCD
  unsigned* host;               // pinned host memory, nullable
  unsigned seq;
  unsigned ticks_lead;          // s_memrealtime ticks (100 MHz) the recurrence's leader waits for the other launch
  unsigned ticks_all;           // ... everyone waits for a decision before voting FAIL
};
#define PREGO_HS_GO 1u
#define PREGO_HS_FAIL 2u

struct GruArgs {
  const void* whh;       // [3H][H] bf16 or f32, reference layout of gru.weight_hh_l0 (rows r|z|n)
  const float* b_hn;     // [H]  = gru.bias_hh_l0[2H:3H]
  const void* gi;        // [rows][3H] fp32 (or bf16 when gi_bf16), chunk-relative packed rows
  void* h_relu_out;      // [rows][H] WT  relu(h_t)  (operand of the classification GEMM), nullable
  float* h_raw_out;      // [rows][H] fp32 h_t (kept for BPTT), nullable
  float* h_state;        // [n_clips][H] fp32, indexed by SORTED clip position; in: h_{t0-1}, out: h_{t1-1}
  void* hx;              // exchange buffers [G][2][16*NCT][H] WT
  unsigned* flags;       // [G*P] one word per producer workgroup, zeroed before every launch
  unsigned* abort_word;  // set to 1 on spin timeout
  const int* rowoff;     // absolute packed row offsets, [t_max+1]
  const int* nact;       // [t_max]
  int t0, t1;            // time steps [t0, t1) handled by this launch
  int row_base;          // rowoff[t0]: chunk-relative row = rowoff[t] - row_base + sorted_index
  int n_clips;                 // number of SLOTS (one or more clips each)
  int G;
  const int* seg_off; const int* seg_start;   // slot schedule: where each slot's next clip starts (h := 0 there)
  float* keep_r; float* keep_z; float* keep_n; float* keep_ghn;   // [rows][H] gate activations for BPTT, nullable
  unsigned* sync;              // [16] placement rendezvous words (8 per-XCD tickets + total), zeroed per launch; nullable
  unsigned long long* stamps;  // debug: per-phase cycle sums of block 0 / wave 0 (nullable)
  int gi_bf16;                 // gi rows are bf16 (inference path with bf16 intermediates)
  int f16;                     // 16-bit operands / intermediates are IEEE fp16 instead of bf16 (launch_gru_recurrence picks the instantiation)
  int Gd;                      // groups the slots are dealt to (0 = G); one-tile kernel only
  int rows;                    // packed rows this launch covers (rowoff[t1] - row_base); 0 = unknown
  int armed;                   // 1: hx / sync were re-armed by an earlier kernel of this stream (launch_ln_relu with a GruArm): no arm launch
  int no_mt;                   // 1: never the software-pipelined multi-tile kernel (handle created under PREGO_GRU_NO_MT=1: A/B and the bit-identity test)
  // split pass (PASS instantiation, launch_gru_recurrence_pass): gi is a ring of (gi_row_mask + 1) rows indexed by absolute packed row,
  // filled by ff_pass.hip while this launch runs; h_relu_out is indexed by absolute packed row
  const unsigned* gi_cnt;      // [n_chunks] completed 256-row units of chunk c (chunk = rows >> chunk_shift)
  unsigned* rec_cnt;           // [n_chunks] += 1 per wave that has consumed the chunk
  int chunk_shift, n_chunks;
  int units_per_chunk, units_last;   // what gi_cnt[c] must reach (last chunk: units_last)
  unsigned gi_row_mask;
  PassHandshake hs;            // pass mode only
  float out_floor;             // h_relu_out = max(h_t, out_floor): 0 = relu(h_t) (the classifier's operand), -inf = h_t (next GRU layer's input)
};
// ---- split pass (ff_pass.hip + the PASS instantiation of gru_recurrence.hip): the feed-forward of a whole pass as one persistent
// kernel on XCDs xcd_lo .. 7 beside one persistent recurrence launch on XCDs 0 .. xcd_lo - 1
struct FfPassArgs {
  const float* const* rgb_ptrs; const float* const* flow_ptrs;   // per-clip feature arrays (device pointer tables), flow nullable
  SlotPlan plan;
  void* rowmap;                 // int2 [total_rows]: (clip, frame) of every packed row (written by the PACK jobs, read by the head); nullable
  int d_rgb, d_flow;            // d_flow = 0: no flow half
  int in16;                     // feature arrays hold the 16-bit operand type already
  int kx;                       // K of layer1 = d_rgb + d_flow
  const unsigned short* w1; int ld_w1; const float* b1;          // [E][ld_w1]
  const float* ln_g; const float* ln_b; float ln_eps;
  const unsigned short* w_ih; const float* bias2;                // [3H][E]
  int E, n3;                    // embedding width, 3 H
  unsigned short* X; unsigned short* Y; unsigned short* Eb;      // rings of ring_units x 256 rows
  unsigned short* GI;           // ring of gi_ring_units x 256 rows x n3
  int ring_units, gi_ring_units;
  int total_rows, n_units;      // n_units = ceil(total_rows / 256)
  int xcd_lo;                   // XCDs below belong to the recurrence
  int chunk_unit_shift;         // log2(units per chunk): chunk of unit u = u >> shift
  int rec_expect;               // recurrence waves that signal a chunk (groups x P x 4)
  int nt1, nt2;                 // tiles per unit of the two GEMMs (E / 256, 3H / 256)
  int sg;                       // units per super-round of an XCD's ticket order
  int max_wg;                   // debug library (PREGO_SPLIT_FF_CUS): workgroups per feed-forward XCD that take jobs (0 = all 32); the others leave after the handshake
  int lag1, lag2, lag3;         // super-rounds between PACK and L1 / LN / WIH of a unit
  int dbg;                      // timing experiments only (PREGO_SPLIT_DBG; wrong results): 1 skip the pack copies, 2 skip the LayerNorm rows, 4 / 8 skip the layer1 / W_ih tiles
  unsigned long long* stats;    // debug, nullable: [8] 10 ns tick sums (pack, l1, ln, wih, waits, ticket), [6] shader-clock cycles and [7] ticks of the workgroups' lifetime
  int f16;
  unsigned* tick;               // [8] per-XCD job tickets
  unsigned* pack_done; unsigned* l1_cnt; unsigned* ln_done; unsigned* wih_cnt;   // [n_units]
  unsigned* gi_cnt;             // [n_chunks] completed units per chunk (read by the recurrence)
  const unsigned* rec_cnt;      // [n_chunks] recurrence waves done with the chunk
  unsigned* abort_word;
  PassHandshake hs;
};
int launch_ff_pass(const FfPassArgs& a, hipStream_t s);
// the recurrence of a whole pass as one launch on XCDs 0 .. a.Gd - 1 (GruArgs pass fields); 16-bit operands, 16-bit GI ring, one tile
int launch_gru_recurrence_pass(int hid, GruArgs a, hipStream_t s);
int gru_group_size(bool bf16, int hid);            // workgroups per recurrence group
bool gru_hidden_supported(bool bf16, int hid);     // 1024; 512; 2048 with 16-bit operands

// what a recurrence launch needs re-armed before it starts (gru_recurrence.hip: buffer 0 := tag 1 everywhere, buffer 1 := 0,
// sync[0..15] := 0).  A LayerNorm launch that runs between two recurrence launches of a stream can do it on the side (one launch
// and one launch gap fewer per chunk)
struct GruArm { unsigned* hx; unsigned long long words_per_buf; unsigned pattern; unsigned* sync; };
GruArm gru_arm_desc(bool bf16, int hid, int G, void* hx, unsigned* sync);
// the arm as a launch of its own (what the recurrence launchers do for a.armed == 0).  Split pass: it must sit EARLIER in the stream than
// the feed-forward launch of the pass (gru_recurrence.hip, at the function)
void launch_gru_arm(const GruArm& arm, hipStream_t s);

// ---- which recurrence kernel a launch runs: ONE pure host function behind the three entry points (gru_recurrence.hip: gru_choose) ----
enum GruEntry { GRU_ENTRY_MAIN = 0, GRU_ENTRY_X2 = 1, GRU_ENTRY_PASS = 2 };       // launch_gru_recurrence / _x2 / _pass
enum GruFamily { GRU_CLASSIC = 0, GRU_MULTI_TILE = 1, GRU_X2 = 2, GRU_PASS = 3 };
enum GruOperand { GRU_OP_BF16 = 0, GRU_OP_F16 = 1, GRU_OP_F32 = 2, GRU_OP_X2 = 3 };
struct GruQuery {
  int entry;
  bool op16, f16;               // the entry's `bf16` argument (16-bit operands) and GruArgs::f16; ignored by the x2 entry
  int hid, nct, G;
  bool gi_bf16, train;          // train: the launch keeps gate activations / raw state (a.keep_r or a.h_raw_out)
  bool no_mt, stamps;           // GruArgs::no_mt, a.stamps != nullptr
  int rows;
  int mt_spec;                  // PREGO_GRU_MT_SPEC: -1 unset, 0 tag check before the multiply, otherwise inside it
  int Gd;                       // pass entry
  bool ready;                   // x2 entry: inv_scale given; pass entry: gi_cnt, rec_cnt and sync given
};
constexpr int gru_choice_key(int family, int op, int ut, int nct, bool train, bool gi16, bool spec, int hid) {
  return family | op << 2 | ut << 4 | nct << 6 | (int)train << 9 | (int)gi16 << 10 | (int)spec << 11 | hid << 12;
}
struct GruChoice {
  bool ok;                      // false: refused (the entry returns -1 and launches nothing)
  int family, op, hid, ut, nct; // nct: the instantiation's tile count (1, 2 or 4), not the query's
  bool train, gi16, spec;
  int grid;
  size_t lds;
  int packed() const {          // what prego_debug_gru_choice returns (-1: refused)
    return ok ? gru_choice_key(family, op, ut, nct, train, gi16, spec, hid) : -1;
  }
};
GruChoice gru_choose(const GruQuery& q);
bool gru_choice_has_kernel(const GruChoice& c);

// persistent reverse-time recurrence of BPTT (gru_bptt.hip); all row indices are absolute packed rows of the kept forward
struct BpttArgs {
  const void* whhT;            // [H][3H] operand dtype: W_hh transposed (the contraction runs over the 3H gate rows)
  const float* dHout;          // [rows][H] dL/dh_t from the head (after the relu mask)
  const float* R; const float* Z; const float* N; const float* GHN;   // [rows][H] kept gate activations of the forward
  const float* Hraw;           // [rows][H] h_t of the forward
  float* dGI; float* dGH;      // [rows][3H] fp32 gradients of the two pre-activation terms
  void* dGIop; void* dGHop;    // the same in the operand dtype (wgrad GEMM operands)
  void* hx;                    // exchange buffers, gru_bptt_hx_bytes()
  unsigned* sync;              // [1024] placement words + one epoch word per producer workgroup (zeroed by the launcher)
  unsigned* abort_word;
  const int* rowoff; const int* nact;
  int t_max, n_clips, G;
  int force_sc1;               // test knob: skip the XCD-local fast path
};
size_t gru_bptt_hx_bytes(bool bf16, int hid, int G);
int launch_gru_bptt(bool bf16, int hid, int nct, BpttArgs a, hipStream_t s);

// GEMM epilogues (bf16 kernel): what happens to acc + bias
enum { EPI_STORE = 0, EPI_RESIDUAL = 1, EPI_GELU_BF16 = 2, EPI_STORE_BF16 = 3, EPI_QKV = 4, EPI_TOKENS = 5 };
struct GemmEpi {
  int mode;
  void* out_b;                 // bf16 output (EPI_GELU_BF16 / EPI_STORE_BF16), leading dim = ldc
  void* q; void* k;            // EPI_QKV destinations [B,h,n_tok,dh]
  int n_tok, heads, dh, emb;
  float q_scale;               // softmax scale folded into Q
  void* vn;                    // EPI_QKV: V [B,h,n_tok,dh] (row-major; the attention kernels read it transposed from LDS)
  int which0;                  // EPI_QKV: index of the first output block (0 = q|k|v; 1 = the GEMM computes k|v only)
  // training-mode nn.Dropout on the epilogue's result (EPI_RESIDUAL: on acc + bias before the residual add, Transformer.py:31,46;
  // EPI_GELU_BF16: on gelu(.), Transformer.py:41): stateless hash mask of (seed, m * ldc + n); thresh = 0 -> no dropout
  unsigned drop_thresh; float drop_scale; unsigned long long drop_seed;
  unsigned drop2_thresh; float drop2_scale; unsigned long long drop2_seed;   // a second, independent mask on the same value (proj_drop, Attention.py:19,40)
  float* pre_f32;              // EPI_GELU_BF16, training: the pre-activation W1 x + b1 in fp32 (gelu'), leading dim = ldc; nullable
  // EPI_TOKENS (ViT.py:125-129 in the encoding GEMM's epilogue): GEMM row m = b n_tok + t goes to row m + b of C (one cls row per
  // window is left for the caller) with the learned positional row pe[t] added: x[b, t] = W_enc f + b_enc + pe[t]
  const float* pe;
  int f16;                     // operands (and every 16-bit output) are IEEE fp16 instead of bf16
  int xcd_lo; unsigned* counter;   // WORKER instantiation (probe): XCDs below xcd_lo leave at once; tiles are claimed from *counter
  int split_a_lo, split_b_lo;      // SPLIT instantiation (fp16x2 operands): element column of the lo half in the A / B rows
  const float* acc_scale;          // SPLIT: device pointer to 1 / (power-of-two scale of the weights); NULL = 1
};

// ---- which kernel an NT product C[M,N] = epilogue(A[M,K] . B[N,K]^T + bias) runs on (gemm.hip): ONE chooser, ONE launcher ----
enum GemmNtKernel {
  GEMM_NT_NONE = -1,           // nothing to launch (M <= 0)
  GEMM_NT_128 = 0,             // 128 x 128 two-stage (gemm.hip): every epilogue, both operand types, any shape
  GEMM_NT_256X128 = 1,         // 256 x 128 three-stage counted-vmcnt (gemm.hip): bf16, fp32 C
  GEMM_NT_256SQ = 2,           // 256 x 256 two-stage (gemm.hip): bf16, fp32 C, N % 256 == 0
  GEMM_NT_PINGPONG = 3,        // 256 x 256 ping-pong (gemm_pp.hip): every epilogue, both operand types, gemm_pingpong_takes
  GEMM_NT_SPLITK = 4           // eight-wave split-K workgroup (gemm_tn.hip): bf16, fp32 C, at most 256 tiles
};
// who asks: the three call paths differ in what they try (the differences are historical and kept; see gemm_nt_choose)
enum GemmNtEntry {
  GEMM_NT_PLAIN = 0,           // launch_gemm_bf16_nt: a projection with fp32 C and no epilogue
  GEMM_NT_EPI = 1,             // launch_gemm_bf16_nt_epi: any epilogue
  GEMM_NT_PROJ16 = 2           // the MiniROAD forward's projection with fp16 operands or a 16-bit C
};
struct GemmNtKnobs { bool no_big, no_splitk, no_pingpong; };   // PREGO_GEMM_NO_BIG / _NO_SPLITK / _NO_PINGPONG (debug library only)
struct GemmNtQuery {
  int entry, M, N, K, lda, ldb;
  bool has_bias, f16, train_splitk;
  int mode, dh, emb;           // epilogue mode; EPI_QKV: head width and embedding width
};
// pure: no device, no global
GemmNtKernel gemm_nt_choose(const GemmNtQuery& q, GemmNtKnobs knobs);
bool gemm_pingpong_takes(int M, int N, int K, bool has_bias, int mode, int dh, int emb);    // gemm_pp.hip
// runs `kind`; -1 = that kernel does not take the shape or the epilogue (nothing launched).  C: fp32 destination (EPI_STORE,
// EPI_RESIDUAL, EPI_TOKENS); the 16-bit destinations are in epi
int launch_gemm_nt_kernel(GemmNtKernel kind, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M,
                          int N, int K, GemmEpi epi, hipStream_t s);
// choose, then launch
void launch_gemm_nt(int entry, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M, int N, int K,
                    GemmEpi epi, bool train_splitk, hipStream_t s);
inline void launch_gemm_bf16_nt_epi(const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M,
                                    int N, int K, GemmEpi epi, hipStream_t s) {
  launch_gemm_nt(GEMM_NT_EPI, A, lda, B, ldb, bias, C, ldc, M, N, K, epi, false, s);
}

void launch_pack_rows(bool bf16, const float* const* rgb_ptrs, const float* const* flow_ptrs, const SlotPlan& plan,
                      int row0, int nrows, int d_rgb, int d_flow, void* X, hipStream_t s, int grid_limit = 0,
                      void* rowmap = nullptr /* int2 [nrows]: (clip, frame) of every packed row, for the head kernel */,
                      bool f16 = false /* with bf16 = true: the 16-bit operand type is IEEE fp16 */,
                      bool in16 = false /* the feature arrays hold the 16-bit operand type already (PREGO_FWD_IN16) */);
void launch_ln_relu(bool bf16, const void* Y, const float* gamma, const float* beta, int nrows, int E, float eps,
                    void* out, float* stats, float drop_p, unsigned long long seed, int row0_abs, hipStream_t s, int relu = 1,
                    bool in_bf16 = false, bool f16 = false, const GruArm* arm = nullptr);
void launch_f32_to_bf16(const float* src, void* dst, size_t n, hipStream_t s);
void launch_pad_convert(bool bf16, const float* src, int rows_src, int cols_src, int ld_src, void* dst, int rows_dst,
                        int cols_dst, hipStream_t s, bool f16 = false);
// 256x256x64 ping-pong (8-phase) kernel, csrc/gemm_pp.hip; -1 = shape not supported (gemm_pingpong_takes)
int launch_gemm_bf16_pingpong_epi(const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc, int M, int N,
                                  int K, GemmEpi epi, hipStream_t s);
int launch_gemm_bf16_pingpong_worker(const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc, int M, int N,
                                     int K, int xcd_lo, unsigned* counter, int grid, hipStream_t s, bool out16 = false, bool f16 = false);
int launch_gemm_x2_pingpong(const void* A, int lda, int a_lo, const void* B, int ldb, int b_lo, const float* inv_scale, const float* bias,
                            float* C, int ldc, int M, int N, int K, hipStream_t s);
void launch_x2_weight_split(const float* src, int rows, int cols, void* dst, float* scale2 /* device [2]: scale, 1 / scale */, hipStream_t s);
void launch_pack_rows_x2(const float* const* rgb_ptrs, const float* const* flow_ptrs, const SlotPlan& plan, int row0, int nrows,
                         int d_rgb, int d_flow, void* X, hipStream_t s, int grid_limit = 0, void* rowmap = nullptr);
void launch_ln_relu_x2(const float* Y, const float* gamma, const float* beta, int nrows, int E, float eps, void* out, hipStream_t s,
                       const GruArm* arm = nullptr);
// split-operand recurrence (gru_recurrence_x2.hip): a.whh = [3H][2H] split rows of W_hh * scale, a.gi fp32, a.h_relu_out fp32
int launch_gru_recurrence_x2(int hid, int nct, GruArgs a, const float* inv_scale, hipStream_t s);
size_t gru_x2_hx_bytes(int hid, int G);
GruArm gru_x2_arm_desc(int hid, int G, void* hx, unsigned* sync);
inline void launch_gemm_bf16_nt(const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M,
                                int N, int K, hipStream_t s, bool f16 = false,
                                bool train_splitk = false /* bf16, at most 256 tiles of 128 x 128: the eight-wave split-K workgroup of gemm_tn.hip
                                                             (another summation order over k than every other NT kernel: training forward only) */) {
  GemmEpi epi{};
  epi.mode = EPI_STORE; epi.f16 = f16 ? 1 : 0;
  launch_gemm_nt(GEMM_NT_PLAIN, A, lda, B, ldb, bias, C, ldc, M, N, K, epi, train_splitk, s);
}
void launch_gemm_f32_nt(const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, int M,
                        int N, int K, hipStream_t s);
int launch_gru_recurrence(bool bf16, int hid, int nct, GruArgs a, hipStream_t s);
size_t gru_hx_bytes(bool bf16, int hid, int G);
int gru_max_slots(int G, bool x2);       // slots a handle of G groups plans for: 16 per tile and group
int launch_head_softmax(bool bf16, const void* Hrelu, const void* Wc, const float* bc, const SlotPlan& plan,
                        int row0, int nrows, int hid, int C, int apply_softmax,
                        float* const* out_ptrs, int* const* argmax_ptrs, hipStream_t s, const void* rowmap = nullptr, bool f16 = false);
// anticipation head of MiniROADA (ant_head.hip): per row, for l < L, softmax / logits of relu(relu(h) W_a[l]^T + b_a[l]) W_c^T + b_c into
// out_ptrs[clip] [T][L][C] and argmax_ptrs[clip] [T][L]; rows and destinations as launch_head_softmax.  -1 = unsupported shape
int launch_ant_head(bool bf16, bool f16, const void* Hrelu, const void* Wa, const float* ba, const void* Wc, const float* bc,
                    const SlotPlan& plan, int row0, int nrows, int hid, int L, int C, int apply_softmax, float* const* out_ptrs,
                    int* const* argmax_ptrs, const void* rowmap, hipStream_t s);
// training (ant_head.hip): A_l of the packed rows [span[0], span[1]) (device-side span) into a_out [nrows][L * hid], operand type, the forward's bits
int launch_ant_head_store_a(bool bf16, const void* Hrelu, const void* Wa, const float* ba, int nrows, int hid, int L, void* a_out,
                            const int* span, hipStream_t s);
// the anticipation head's backward (ant_head_bwd.hip): d_ant -> packed G [R][L * C] + row flags + the device-side row span, then the
// gradient terms of f_classification, anticipation_layer and d relu(h) over that span
void launch_ant_gather(const float* const* d_ant, const int* rowoff, const int* sorted_clip, int t_max, int nrows, int LC, float* G, int* flags,
                       int* span, int force_full, hipStream_t s);
void launch_ant_head_wgrad(bool bf16, const float* G, const void* HR, const void* Wc, int R, int H, int L, int C, const int* span,
                           const void* Abuf, void* dZ, float* g_fc_w, float* g_fc_b, float* g_w_a, float* g_b_a, hipStream_t s);
void launch_ant_head_dgrad(bool bf16, const void* Wa, int R, int H, int L, const int* span, const void* dZ, float* part, float* dHR, hipStream_t s);
void launch_permute_rows(const float* src, float* dst, const int* sorted_clip, int n, int width, int to_sorted,
                         hipStream_t s);
void launch_add_vec(const float* a, const float* b, float* out, int n, int n_add, hipStream_t s);

// training path (train.hip)
void launch_oad_loss(const float* const* logit_ptrs, const float* const* target_ptrs, const int* lens, int n_clips, int C,
                     float* loss_out, float* const* dlogit_ptrs, float grad_scale, hipStream_t s, bool sum = false);
void launch_gather_dlogits(bool bf16, const float* const* dl_ptrs, const int* rowoff, const int* sorted_clip, int t_max,
                           int nrows, int C, int Cpad, void* out, hipStream_t s);
void launch_transpose_convert(bool in_bf16, bool out_bf16, const void* src, int M, int N, int ld_src, void* dst, int Mpad,
                              hipStream_t s);
void launch_colsum(const float* src, int M, int N, float* part, float* out, hipStream_t s);
void launch_colsum_bf16(const void* src, int M, int N, float* part, float* out, hipStream_t s);
void launch_colsum_stage2(const float* part, int nb, int N, float* out, hipStream_t s);
void launch_gru_bwd_step(bool bf16, int t, int na, int na_next, int row_t, int row_tm1, int H, const float* dHout,
                         const float* carry_in, const float* dhpart, const float* R, const float* Z, const float* Nn,
                         const float* GHN, const float* Hraw, float* carry_out, float* dGI, float* dGH, void* dGIop,
                         void* dGHop, hipStream_t s);
void launch_relu_mask(const float* dHrelu, const float* Hraw, size_t n, float* out, hipStream_t s);
void launch_build_hprev(bool bf16, const float* Hraw, const int* rowoff, int t_max, int nrows, int H, void* out,
                        hipStream_t s);
// relu = 0: plain LayerNorm backward (Transformer path); accumulate = 1: dY += result (residual stream)
int launch_ln_relu_bwd(const float* dE, const float* Y, const float* stats, const float* gamma, const float* beta, int nrows,
                       int E, float drop_p, unsigned long long seed, int row0_abs, float* dY, float* part, hipStream_t s,
                       int relu = 1, int accumulate = 0, void* dYb = nullptr /* bf16 copy of dY (wgrad operand), nullable */);
// training GEMMs on k-major operands (gemm_tn.hip): C[M,N] fp32 = op(A) . op(B) + bias; ta: A stored [K][M]; tb (required): B stored [K][N];
// colsum_out (ta only): [M] column sums of A = the bias gradient of a wgrad; k_valid: contraction rows present in memory
// Caller contract (tests/test_gpu_gemm_tn.py holds the kernel to it with NaN-filled surroundings):
//   * a k-major operand (A with ta, B with tb) is read in rows [0, k_valid) only; rows k_valid .. K-1 need not exist.  Its columns past
//     M (A) / N (B) up to the leading dimension are read but reach only output rows / columns that are never stored
//   * a ROW-MAJOR A (!ta: the dgrads) is read in rows [0, M) and in ALL K columns: with k_valid < K its columns k_valid .. K-1 are
//     multiplied by zero-filled B rows, so the CALLER must keep them finite (the head dgrad's dlogits hold zeros in their pad
//     columns) - a NaN or Inf there would reach every output of its row
//   * lda, ldb multiples of 8, K a multiple of 64; -1 (nothing launched) for anything else, for !tb with ta / K < 128 / more than 256
//     tiles / k_valid != K, and for operands whose byte offsets do not fit 31 bits (K * max(lda, ldb) * 2, M * lda * 2)
//   * exactly the M x N block of C (or C16) and colsum_out[0, M) are written
int launch_gemm_bf16_tn(bool ta, bool tb, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M, int N,
                        int K, int k_valid, float* colsum_out, hipStream_t s, void* C16 = nullptr /* bf16 C instead of fp32 */);

// post-processing (postproc.hip)
int launch_window_vote(const int* pred, long long n_frames, int window, int n_classes, int* votes, hipStream_t s);

// per-frame average precision (metrics.hip): segmented radix sort + scan, one segment per class
int launch_format_ids(const int* ids, long long n, unsigned* text, int* bad, hipStream_t s);
size_t perframe_ap_workspace_bytes(long long n_frames, int n_classes);
int launch_perframe_ap(const float* scores, const float* target, const int* labels, long long n_frames, int n_classes, double* ap, long long* n_pos,
                       double* score_sum, void* workspace, hipStream_t s);
// per-stage average precision (metrics.hip): the per-frame ranks + one counter per (stage, positive); ap / n_pos [10][n_classes]
size_t perstage_ap_workspace_bytes(long long n_frames, int n_classes);
int launch_perstage_ap(const float* scores, const int* labels, long long n_frames, int n_classes, double* ap, long long* n_pos, void* workspace,
                       hipStream_t s);
// calibrated average precision (metrics.hip): the same pipeline over (score key, frame) composites: ties in frame order
size_t perframe_cap_workspace_bytes(long long n_frames, int n_classes);
int launch_perframe_cap(const float* scores, const float* target, const int* labels, long long n_frames, int n_classes, double* ap, long long* n_pos,
                        double* score_sum, void* workspace, hipStream_t s);
size_t perstage_cap_workspace_bytes(long long n_frames, int n_classes);
int launch_perstage_cap(const float* scores, const int* labels, long long n_frames, int n_classes, double* ap, long long* n_pos, void* workspace,
                        hipStream_t s);

// segmental metrics (segmental.hip): MoF, edit distance and F1 at three overlaps per video; one launch, one workgroup per video.
// records [n_videos][8]; bg: four mask words; num / den: three overlaps; -1 = refused, nothing launched.  ws: the query's bytes
constexpr int kSegmentalLdsSegments = 2047;     // PREGO_SEGMENTAL_LDS_SEGMENTS of the public header
constexpr int kSegmentalChunk = 1024;           // frames per scan step of a workgroup
size_t segmental_workspace_bytes(long long n_frames, int n_videos);
int launch_segmental(const int* pred, const int* gt, const int* offsets, int n_videos, long long n_frames, const unsigned* bg, const int* num,
                     const int* den, int* records, void* workspace, hipStream_t s);

// Viterbi decoding (decode.hip): labels [n_frames] and records [n_videos][2] (total cost | end state) from probabilities (fp32 words,
// quantised on load) or emission costs (int32 words, clamped on load: `costs`) [n_frames][ld]; one launch, one workgroup per video.
// -1 = refused, nothing launched.  ws: the query's bytes (n_frames == 0: not touched)
constexpr int kDecodeCap = 32767;               // PREGO_DECODE_CAP of the public header
constexpr int kDecodeMaxClasses = 128;          // PREGO_DECODE_MAX_CLASSES
constexpr int kDecodeBlock = 64;                // PREGO_DECODE_BLOCK: frames per block of the backtrace
constexpr int kDecodePrefetch = 8;              // PREGO_DECODE_PREFETCH: frames the emission rows are requested ahead of the step
size_t viterbi_workspace_bytes(long long n_frames, int n_videos, int n_classes);
int launch_viterbi(bool costs, const void* src, long long ld, const int* offsets, int n_videos, long long n_frames, int n_classes,
                   const int* trans, const int* init, int* labels, long long* records, void* workspace, hipStream_t s);
// probabilities [n_frames][ld] -> emission costs [n_frames][n_classes] with the decode kernel's quantiser; -1 = refused
int launch_emission_costs(const float* probs, long long ld, long long n_frames, int n_classes, int* costs, hipStream_t s);

// THUMOS post-processing (thumos_post.hip): 5-frame max, column merge, stable removal of the ambiguous rows; count, scan, scatter
constexpr int kThumosTileRows = 128;     // rows per scatter tile (PREGO_THUMOS_TILE_ROWS of the public header)
constexpr int kThumosChunkCols = 96;     // columns of a tile staged in LDS at a time
size_t thumos_postprocess_workspace_bytes(long long n_frames, int n_classes);
// target XOR labels; sw_to < 0: no switch; amb < 0: every row kept; -1 = refused, nothing launched.  ws: the query's bytes, n > 0
int launch_thumos_postprocess(const float* scores, long long ld_scores, const float* target, long long ld_target, const int* labels,
                              long long n_frames, int n_classes, bool smooth, int sw_from, int sw_to, int amb, float* scores_out,
                              float* target_out, int* labels_out, long long* n_valid, void* workspace, hipStream_t s);

// Evaluate's feature cache (feature_cache.hip): n fp32 values -> bf16 / fp16 (f16) with the pack kernels' conversion; n % 8 == 0, n > 0
void launch_cast_features(bool f16, const float* src, void* dst, long long n, int n_cu, hipStream_t s);

// training windows cut from the resident training set (train_cache.hip); the fields are prego_gather_windows' arguments (prego_amd.h)
struct GatherWindows {
  const float *rgb_rows, *flow_rows;       // [n_rows][d_rgb], [n_rows][d_flow]; NULL with a NULL output
  const int* labels;                       // [n_rows] class id, -1 for an all-zero row - or
  const float* dense_targets;              // [n_rows][n_classes]
  const long long* vid_row0;               // [n_videos]
  const int *vid_len, *table, *order;      // [n_videos], [n_windows][2], [>= first + n]
  long long n_rows, first;
  int n_videos, n_windows, n, window, n_classes, ant_len, d_rgb, d_flow;
  float *rgb_out, *flow_out, *target_out, *ant_out;      // nullable
};
// the caller has checked: n >= 1, window >= 1, n * window, n * window * n_classes and n * ant_len * n_classes below 2^31, d % 4 == 0,
// 16-byte aligned feature and output pointers, first + n within order
void launch_gather_windows(const GatherWindows& a, int n_cu, hipStream_t s);

// stream pool (stream_pool.hip): slot-addressed GRU state rows and per-slot vote records in the caller's device block
constexpr int kPoolMaxActive = 256;      // slots one call may name
constexpr int kPoolRecHeader = 4;        // record words in front of the counts: frames, last vote + 1, n_events, overflow
constexpr int kPoolOverflowFull = 1, kPoolOverflowBadId = 2;      // bits of the overflow word
struct PoolGeom {
  float* h;                              // [capacity][hid] fp32
  int* rec;                              // [capacity][rec_words]: header | counts[ncls_pad] | event_id[max_events] | event_start[max_events]
  int hid, ncls, ncls_pad, window, max_events, rec_words, capacity;
};
struct PoolSlots { int s[kPoolMaxActive]; };      // the slot list of one call, by value in the kernel arguments
// slots: HOST, n in 1..256, every slot in [0, capacity) and named once (the caller checks duplicates); -1 = refused, nothing launched
int launch_pool_gather(const PoolGeom& g, const int* slots, int n, float* h_ws, hipStream_t s);
// the commit of K frames per slot (1..32, n K <= 256; K = 1: the one-frame call): the state row once, then argmax[i K + t], t = 0 .. K - 1,
// voted in frame order by the slot's lane
int launch_pool_commit(const PoolGeom& g, const int* slots, int n, int K, const float* h_ws, const int* argmax, hipStream_t s);
int launch_pool_vote(const PoolGeom& g, const int* slots, int n, const int* ids, hipStream_t s);
int launch_pool_flush(const PoolGeom& g, const int* slots, int n, hipStream_t s);
int launch_pool_reset(const PoolGeom& g, const int* slots, int n, hipStream_t s);

// event feed of a stream pool (stream_feed.hip): the events appended to the slots' records since the previous drain, in one report
constexpr int kFeedWg = 256;             // slots one workgroup of the drain handles (one trip, one lane per slot)
struct FeedGeom {
  int* cursor;                           // [capacity]: events delivered (bits 0..29) | overflow bits reported (bits 30..31)
  int* seq;                              // drains so far
  int* wg_due;                           // [ceil(capacity / kFeedWg)]: entries due per workgroup of the drain in flight
  int max_out;                           // entries a report holds
};
// report: device, 16-byte aligned, (1 + f.max_out) x 16 bytes.  Reads g's records, writes f's words and the report; -1 = nothing launched
int launch_feed_drain(const PoolGeom& g, const FeedGeom& f, int* report, hipStream_t s);
// cursor[slots[i]] <- 0; slots: HOST, n in 1..256, each in [0, capacity); -1 = nothing launched
int launch_feed_forget(const FeedGeom& f, int capacity, const int* slots, int n, hipStream_t s);

// procedure model (procedure.hip): a grouped corpus of step transcripts in the caller's device block, judged as a back-off n-gram model
constexpr int kProcMaxOrder = 8, kProcMaxClasses = 128, kProcMaxDen = 32768;
constexpr int kProcStart = 0xff;         // the virtual first symbol of every transcript in `sym`
constexpr int kProcNoMatch = 0xfe;       // a queried symbol outside [0, ncls): equal to nothing in `sym`
constexpr int kProcJudged = 1, kProcMistake = 2, kProcUnknown = 4, kProcSkipped = 8, kProcJstarShift = 8;      // a verdict's flags word
constexpr int kProcVerdictWords = 8;
constexpr int kProcWaves = 4;            // judged items per workgroup trip: one wave each
constexpr int kProcMaxGrid = 1024;       // workgroups of a judging launch; they stride over the items
struct ProcGeom {
  const int* goff;                       // [n_groups + 1]: group g's examples are ex[goff[g] .. goff[g + 1])
  const int* ex;                         // [n_examples]: the position in sym of each example's next symbol, sorted by group
  const unsigned char* sym;              // per transcript kProcStart, s_0 .. s_{n-1}; sym[0] is a START, so a backward compare ends inside
  int ncls, order, n_groups, n_examples, n_sym, num, den;       // n_sym: bytes of sym
};
// offsets [n_seq + 1], symbols [n_pos], groups [n_seq]: device; verdicts: device, 16-byte aligned, n_pos x 32 bytes; -1 = nothing launched
int launch_procedure_judge(const ProcGeom& m, int n_seq, int n_pos, const int* offsets, const int* symbols, const int* groups, int* verdicts,
                           hipStream_t s);
// report: what launch_feed_drain wrote (its count is read on the device); slot_groups [g.capacity]: device; verdicts: device, 16-byte
// aligned, max_out x 32 bytes, entry k's verdict at k.  Reads g's records, writes the verdicts alone; -1 = nothing launched
int launch_feed_judge(const ProcGeom& m, const PoolGeom& g, int max_out, const int* report, const int* slot_groups, int* verdicts, hipStream_t s);
// next-step forecast: the histogram row a verdict is read from, ranked (count descending, equal counts by ascending class id)
constexpr int kProcMade = kProcJudged;   // a forecast's flags word: MADE | UNKNOWN | SKIPPED, j* as a verdict, ranked entries in bits 16..19
constexpr int kProcRankedShift = 16, kProcRanks = 8;
constexpr int kProcForecastWords = 24;   // flags | n_cand | tot | group | mask [4] | id [8] | cnt [8]
// offsets [n_seq + 1], symbols [max(n_pos, 1)], groups [n_seq]: device; forecasts: device, 16-byte aligned, (n_pos + n_seq) x 96 bytes, the
// forecast after the first p symbols of sequence s at row offsets[s] + s + p; n_pos 0: every sequence is empty; -1 = nothing launched
int launch_procedure_forecast(const ProcGeom& m, int n_seq, int n_pos, const int* offsets, const int* symbols, const int* groups,
                              int* forecasts, hipStream_t s);
// as launch_feed_judge; forecast k says what follows entry k: the history is the slot's events in front of it and its own step id
int launch_feed_forecast(const ProcGeom& m, const PoolGeom& g, int max_out, const int* report, const int* slot_groups, int* forecasts,
                         hipStream_t s);
// slots [n] (1 <= n <= g.capacity, any words), slot_groups [g.capacity]: device; forecast i says what follows every event slot slots[i]'s
// record holds, a slot outside the pool is SKIPPED; forecasts: device, 16-byte aligned, n x 96 bytes; -1 = nothing launched
int launch_pool_forecast(const ProcGeom& m, const PoolGeom& g, int n, const int* slots, const int* slot_groups, int* forecasts, hipStream_t s);

// Transformer stream pool (vit_stream.hip): a ring of encoded frames per slot in the caller's device block.  ring [capacity][T][E] fp32,
// row f mod T = linear_encoding(frame f); hf [capacity][4] int32 = head (next row to write) | fill (rows that hold a frame) | 0 | 0
struct VitRing {
  float* ring;
  int* hf;
  int T, E, capacity;
};
constexpr int kVitRingStateWords = 4;
// slots: as the pool launchers above (HOST, 1..256, inside the pool, named once); -1 = refused, nothing launched
// ring[slots[i]][head] <- enc[i], then head and fill advance
int launch_vit_ring_commit(const VitRing& r, const int* slots, int n, const float* enc, hipStream_t s);
// launch_vit_sliding_tokens with the rings as the source: window i = the last T frames of slots[i], bias rows where fill does not reach
int launch_vit_ring_tokens(const VitRing& r, const int* slots, int n, const float* enc_b, const float* cls, const float* pe, float* x,
                           const float* ln_w, const float* ln_b, void* xn, float* x0, hipStream_t s, bool f16 = false);
// out [T][E] <- the slot's logical window, oldest to newest (bias rows in front), *fill_out <- fill
int launch_vit_ring_window(const VitRing& r, int slot, const float* enc_b, float* out, int* fill_out, hipStream_t s);

// slot images of either pool type (stream_image.hip; layout and validity rule: pool_image.h).  ImageRing::ring == nullptr: the GRU pool,
// a slot's state is its row of g.h; else the Transformer pool, g.h holds the ring words [capacity][4] and the state is the slot's ring
struct PoolImageDims;                    // pool_image.h
struct ImageRing {
  float* ring;                           // [capacity][T][E] fp32 or nullptr
  int T, E;
};
constexpr int kImageChunkVecs = 4096;    // 16-byte vectors of an image one workgroup moves (64 KB): grid = chunks x n
// slots: as the pool launchers (HOST, 1..256, inside the pool, named once); images: device, 16-byte aligned, n x d.image_words words;
// cursor: the feed's cursor words [capacity] or nullptr; -1 = refused, nothing launched
// images[i] <- slot slots[i] (the pool and the cursors are only read)
int launch_pool_snapshot(const PoolGeom& g, const ImageRing& r, const PoolImageDims& d, const int* cursor, const int* slots, int n,
                         int* images, hipStream_t s);
// slot slots[i] <- images[i] where pool_image_fault says 0, else nothing of that slot; status (nullable) [n] <- the fault words
int launch_pool_restore(const PoolGeom& g, const ImageRing& r, const PoolImageDims& d, int* cursor, const int* slots, int n,
                        const int* images, int* status, hipStream_t s);

// split pass (round 6): rows gate * H + u of a 16-bit [3H][E] matrix and an fp32 [3H] vector -> rows (u / 2) * 6 + 2 * gate + u % 2 (rowwise.hip)
void launch_permute_gi_rows(const void* w, const float* bias, void* w_perm, float* bias_perm, int H, int E, hipStream_t s);

// fused multi-tensor AdamW (optim.hip)
int launch_adamw(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 void* const* copies, const long long* numel, bool copy_bf16, long long step, float lr, float b1, float b2, float eps,
                 float wd, hipStream_t s, unsigned* guard = nullptr /* device word: non-zero = change nothing */,
                 const float* peer = nullptr /* device float: non-zero = change nothing and raise *guard (data-parallel runs) */);

// Transformer path (attention.hip, vit.hip)
// attention forward (attention.hip): query on the lane, V row-major [B,h,N,dh], Nq queries against N keys
int launch_flash_attention_v2(const void* Q, const void* K, const void* V, void* out, int B, int Nq, int N, int heads, int dh,
                              int causal, hipStream_t s, float* lse = nullptr, unsigned drop_thresh = 0, float drop_scale = 1.f,
                              unsigned long long drop_seed = 0, bool f16 = false /* Q, K, V, P and the output are IEEE fp16 */);
// attention backward (attention_bwd.hip): dqkv [B*N, 3*heads*dh] bf16; delta: scratch fp32 [B*heads*N]
int launch_attention_bwd(const void* Qs, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                         float* delta, void* dqkv, int B, int N, int heads, int dh, int causal, float q_scale, hipStream_t s,
                         unsigned drop_thresh = 0, float drop_scale = 1.f, unsigned long long drop_seed = 0);
// ViTEnc training glue (vit_train.hip)
// dropout arguments (thresh = p * 2^32, scale = 1 / (1 - p), seed): thresh = 0 means none
void launch_gelu_bwd(const float* df, const float* u, size_t n, float* du, void* du_bf16, hipStream_t s, unsigned drop_thresh = 0,
                     float drop_scale = 1.f, unsigned long long drop_seed = 0);
// out_f32 (nullable) / out_bf16 := src * dropout mask(seed, element index) * scale
void launch_mask_convert(const float* src, size_t n, float* out_f32, void* out_bf16, unsigned drop_thresh, float drop_scale,
                         unsigned long long drop_seed, hipStream_t s, unsigned drop2_thresh = 0, float drop2_scale = 1.f,
                         unsigned long long drop2_seed = 0);
// any C launch_vit_head takes: its copy of a window's dlogits in LDS is sized by C, and g_hb is written for C > E as well
void launch_vit_head_bwd(const float* x, const float* dlogits, int B, int N, int E, int C, const float* lnw, const float* lnb,
                         const float* hw, float* dx, float* scratch /*[3][B][E]*/, float* g_lnw, float* g_lnb, float* g_hw,
                         float* g_hb, hipStream_t s);
void launch_vit_tokens_bwd(const float* dx, int B, int T, int E, float* denc, float* g_pe, float* g_cls, hipStream_t s,
                           unsigned drop_thresh = 0, float drop_scale = 1.f, unsigned long long drop_seed = 0);
void launch_cat_convert(const float* rgb, const float* flow, int rows, int d_rgb, int d_flow, void* out_bf16, hipStream_t s, bool f16 = false);
void launch_vit_tokens(const float* enc, const float* cls, const float* pe, int B, int T, int E, float* x, hipStream_t s,
                       unsigned drop_thresh = 0, float drop_scale = 1.f, unsigned long long drop_seed = 0);
void launch_vit_cls_rows(const float* cls, const float* pe, int B, int T, int E, float* x, hipStream_t s);
void launch_vit_head(const float* x, int B, int N, int E, const float* lnw, const float* lnb, const float* hw,
                     const float* hb, int C, float* out, hipStream_t s, int* argmax = nullptr);
// sliding windows over one video: token rows of windows ending at frames t0 .. t0 + B - 1 from the per-frame encoding (vit.hip)
void launch_vit_sliding_tokens(const float* enc, const float* enc_b, const float* cls, const float* pe, int t0, int B, int T, int E,
                               float* x, const float* ln_w, const float* ln_b, void* xn, float* x0, hipStream_t s, bool f16 = false);
void launch_add_bias_rows(float* x, const float* bias, int rows, int n, hipStream_t s);
// fp32-operand mode of the Transformer path (vit_f32.hip): attention over fp32 rows (q / k / v at column offsets of one [B*N, ld]
// array, Nq <= N queries per sequence), exact-erf GELU in place, x += y, [rgb | flow] rows
int launch_attention_f32(const float* qkv, int ld, int q_off, int k_off, int v_off, float* out, int B, int N, int Nq, int heads,
                         int dh, int causal, float scale, hipStream_t s);
void launch_gelu_f32(float* u, size_t n, hipStream_t s);
void launch_add_rows(float* x, const float* y, size_t n, hipStream_t s);
void launch_cat_rows_f32(const float* rgb, const float* flow, int rows, int d_rgb, int d_flow, float* out, hipStream_t s);

// streaming step (stream_step.hip): skinny products for n <= 16 rows, one frame per stream
struct StreamGemv {
  const void* W;        // [Nout][K] bf16
  const void* X;        // input columns [0, kx1): [n][ldx], fp32 or bf16 (x_bf16)
  const void* X2;       // input columns [kx1, K): [n][ldx2]; nullptr = zeros
  const float* bias;    // nullable
  float* Y;             // [n][Nout]
  int Nout, K, kx1, ldx, ldx2, x_bf16;
  const float* ln_g = nullptr;   // non-null (with ln_b): X is the fp32 pre-LayerNorm row, normalised + ReLU inside the kernel (n <= 4, K % 2048 == 0)
  const float* ln_b = nullptr;
  float ln_eps = 1e-5f;
};
int launch_stream_gemv(int nprob, const StreamGemv* pr, int n, hipStream_t s, bool f16 = false);
int launch_stream_gates_head(const float* gi, const float* gh, const float* b_hn, float* h_state, const void* wc, const float* bc, int n,
                              int H, int C, int softmax, float* out, int* argmax, hipStream_t s, bool f16 = false);

// MiniROADA streaming (stream_ant.hip): the anticipation head behind the streaming step, two launches for n <= 16 streams.  H == 1024.
// A [n][L * H] 16-bit = op16(relu(op16(relu(h_state)) W_a^T + b_a)) from the fp32 state the step has just written
int launch_stream_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16 = false);
// ant_out [n][L][C] / ant_argmax [n][L] (each nullable) = softmax or logits / first argmax of A_l W_c^T + b_c
int launch_stream_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                           int* ant_argmax, hipStream_t s, bool f16 = false);

// wide streaming step (stream_wide.hip): the same arithmetic per output element for n <= 256 streams, weights read once per call.
// xb [n][d_rgb + d_flow] / hb [n][H] = the fp32 frame (a NULL rgb / flow half: zeros) and state in the operand type (pack2_sat)
int launch_wide_cast(const float* rgb, const float* flow, const float* h_state, void* xb, void* hb, int n, int d_rgb, int d_flow, int H,
                     hipStream_t s, bool f16 = false);
// launch_stream_gemv over ceil(n / 16) stream tiles; every problem takes 16-bit input rows in one piece (x_bf16, kx1 == K), no LayerNorm fusion
int launch_wide_gemv(int nprob, const StreamGemv* pr, int n, hipStream_t s, bool f16 = false);
// launch_stream_ant_hidden over the stream tiles / launch_stream_ant_head with 16 rows of the [n L] row list per workgroup
int launch_wide_ant_hidden(const void* wa, const float* ba, const float* h_state, void* A, int n, int H, int L, hipStream_t s, bool f16 = false);
int launch_wide_ant_head(const void* A, const void* wc, const float* bc, int n, int H, int L, int C, int softmax, float* ant_out,
                         int* ant_argmax, hipStream_t s, bool f16 = false);

// multi-frame streaming step (stream_frames.hip): K <= 32 frames for each of n streams, rows = n K <= 256, row s K + t = frame t of stream s.
// xb [rows][d_rgb + d_flow] = the fp32 frames in the operand type (pack2_sat, a NULL half: zeros); h0 [n][H] = a copy of h_state
int launch_frames_cast(const float* rgb, const float* flow, const float* h_state, void* xb, float* h0, int rows, int n, int d_rgb, int d_flow,
                       int H, hipStream_t s, bool f16 = false);
// frame t: gh = op16(h_{t-1}) W_hh^T and the GRU gates in one launch; h_{t-1} = h0 (t == 0) or hist row s K + t - 1; writes hist and hr
// (relu(h_t), 16-bit) row s K + t, and h_state [n][H] when it is non-null (the last frame).  H == 1024
int launch_frames_recur(const void* whh, const float* gi, const float* b_hn, const float* h0, float* hist, void* hr, float* h_state, int n,
                        int K, int t, int H, hipStream_t s, bool f16 = false);

// ragged streaming step (stream_frames.hip, stream_pool.hip): n <= 256 streams with 1..32 frames each, packed rows, stream s owns rows
// off[s] .. off[s] + count[s]).  One entry per stream, by value in the kernel arguments (1 KB): off | stream << 16 | count << 24
constexpr int kRaggedMaxStreams = 256;
struct RaggedMap { unsigned e[kRaggedMaxStreams]; };
__host__ __device__ inline unsigned ragged_entry(unsigned off, unsigned stream, unsigned count) { return off | (stream << 16) | (count << 24); }
__host__ __device__ inline unsigned ragged_off(unsigned e) { return e & 0xffffu; }
__host__ __device__ inline unsigned ragged_stream(unsigned e) { return (e >> 16) & 0xffu; }
__host__ __device__ inline unsigned ragged_count(unsigned e) { return e >> 24; }
// frame t of a ragged call of n streams / `rows` rows: positions [0, n_t) of `walk` - the streams in descending order of count, so those
// with more than t frames come first - advance; h_{t-1} = h0[stream] (t == 0) or hist row off + t - 1; writes hist and hr row off + t and
// h_state[stream] in the stream's own last frame.  single_frame: the call's largest count is 1 (W_hh read once: non-temporal)
int launch_frames_recur_ragged(const void* whh, const float* gi, const float* b_hn, const float* h0, float* hist, void* hr, float* h_state,
                               const RaggedMap& walk, int n, int rows, int n_t, int t, bool single_frame, int H, hipStream_t s,
                               bool f16 = false);
// stream_pool.hip, a ragged burst: entry i of `rows` (the caller's order: slots[i]) gives the slot's ids, [off, off + count) of the packed
// rows, voted in frame order by the slot's lane - after the state row (commit) or alone (vote); off + count <= n_rows <= 256 for every
// entry, or nothing is launched
int launch_pool_commit_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const float* h_ws,
                              const int* argmax, hipStream_t s);
int launch_pool_vote_ragged(const PoolGeom& g, const int* slots, int n, const RaggedMap& rows, int n_rows, const int* ids, hipStream_t s);

// Transformer stream pool, bursts (vit_stream.hip): slot slots[i] takes count[i] frames (1..min(32, T)), its encoded rows enc[off[i] ..
// off[i] + count[i]) of the call's packed enc [n_rows][E], n_rows <= 256.  by_slot.e[i] = off[i] | i << 16 | count[i] << 24 for i < n;
// by_row.e[b] = the entry of the slot that owns packed row b, for b < n_rows.  The launchers check both tables against each other and
// against n_rows and T; -1 = refused, nothing launched.
// one window per packed row (the window ending at that frame) out of the rings AS THEY STAND - before the commit - and enc
int launch_vit_burst_tokens(const VitRing& r, const int* slots, int n, const RaggedMap& by_slot, const RaggedMap& by_row, int n_rows,
                            const float* enc, const float* enc_b, const float* cls, const float* pe, float* x, const float* ln_w,
                            const float* ln_b, void* xn, float* x0, hipStream_t s, bool f16 = false);
// ring[slots[i]][(head + k) mod T] <- enc[off[i] + k], k < count[i]; then head and fill advance by count[i]
int launch_vit_ring_commit_burst(const VitRing& r, const int* slots, int n, const RaggedMap& by_slot, int n_rows, const float* enc,
                                 hipStream_t s);

// decode pool (decode_pool.hip): online fixed-lag Viterbi, one slot of the caller's device block per live stream.  A slot is
//   header [kDecodePoolHeaderWords] int32: frames | committed | status | end state | total cost (int64, words 4..5) | 0 | 0
//   keys   [ncls_pad] int64: d_{frames-1}(j) << 7 | j, "no path" 2^62 (not read while frames == 0)
//   ring   [ring_rows][row_bytes] bytes: the back-pointer row of frame f at row f mod ring_rows, ring_rows = lag + kDecodePoolBurst
// and an all-zero slot is an empty stream.  The model sits in front of the slots, clamped and in the order the step reads it:
//   model  init [128] int32 (-1 forbidden, -1 for the states >= C) | trans^T [C][2 len] int32: word (j, i) = trans[i][j], -1 for i >= C
constexpr int kDecodePoolMaxLag = 256;        // PREGO_DECODE_POOL_MAX_LAG
constexpr int kDecodePoolBurst = 32;          // frames a slot takes per call at most
constexpr int kDecodePending = -2;            // PREGO_DECODE_PENDING
constexpr int kDecodePoolHeaderWords = 8;
constexpr int kDecodeDead = 1, kDecodeFlushed = 2, kDecodePushedAfterFlush = 4;      // bits of the status word
struct DecodePoolGeom {
  PoolGeom rec;                          // the records (h is NULL, hid 0; window = the vote window)
  int* model;
  char* state;                           // [capacity][slot_bytes]
  int lag, ring_rows, row_bytes, len, ring_off, slot_bytes;      // len: the step's slice (8, 16, 32, 48 or 64; 2 len >= C)
};
int decode_pool_len(int n_classes);
// trans [C][C], init [C] or NULL: device int32, read by the launch and free to go behind it
int launch_decode_pool_model(const DecodePoolGeom& g, const int* trans, const int* init, hipStream_t s);
// slots: HOST, n in 1..256, inside the pool, named once; rows.e[i]: slot i's packed rows (off, count 1..32, off + count <= n_rows <= 256) of
// src [n_rows][ld] (fp32 probabilities, or int32 costs with `costs`); labels [n_rows], commit [n][2], now [n_rows]: device, nullable.
// -1 = refused, nothing launched
int launch_decode_pool_push(const DecodePoolGeom& g, bool costs, const int* slots, int n, const RaggedMap& rows, int n_rows, const void* src,
                            long long ld, int* labels, int* commit, int* now, hipStream_t s);
// labels [n][lag], commit [n][2]: device, nullable
int launch_decode_pool_flush(const DecodePoolGeom& g, const int* slots, int n, int* labels, int* commit, hipStream_t s);
int launch_decode_pool_reset(const DecodePoolGeom& g, const int* slots, int n, hipStream_t s);
