// The primitives of the NT GEMM family (gemm.hip, gemm_pp.hip, gemm_tn.hip, ff_pass.hip): the workgroup remap, the two LDS chunk keys,
// the counted wait, the ONE place where the 8-phase ping-pong K loop is written (pp_tile_loop: the ping-pong GEMM in every instantiation
// and the split pass's feed-forward tiles), what each epilogue mode does with acc + bias (gemm_epilogue, at the end), and the host's one
// switch over (epilogue mode, operand type).
//
// PING-PONG schedule (the 8-phase structure of cdna_hip_programming.md section 5), 256x256x64 tiles:
// 8 waves = two groups of four (group = wave >> 2: the two waves that share a SIMD are in different groups).  The K loop
// is cut into phases of 16 MFMAs per wave (one 64x32 quadrant of the wave's 128x64 output over the 64-wide K tile), and
// every phase is {memory part; s_barrier; MFMA part; s_barrier}.  Group 1 runs ONE BARRIER BEHIND group 0, so in every
// barrier interval one wave of each SIMD is in its MFMA part (256 cycles of matrix pipe) while the other issues its
// ds_reads and LDS-DMA: the matrix pipe always has a wave feeding it, and the memory instructions never sit in front of
// MFMAs of the same wave.
//
// LDS: two K-tile buffers x four half-tiles [A0 | A1 | B0 | B1] of 16 KB (128 rows x 64 k), image = lane-linear LDS-DMA
// pieces (8 rows x 128 B) with the 16-byte-chunk XOR swizzle on the SOURCE address and on the ds_read.  A wave's 128
// rows are 64 from A0 and 64 from A1, its 64 columns 32 from B0 and 32 from B1, so every wave consumes the half-tiles
// in the same order and a slot is dead for all waves at the same phase:
//     phase        ds_read (into)        MFMA quadrant     LDS-DMA issued (one half-tile = 2 pieces per lane)
//     1 of tile t  B0(t)   -> b0 (4)     (a0, b0)          A1(t+1)
//     2            B1(t)   -> b1 (4)     (a0, b1)          A0(t+2)
//     3            A1(t)   -> a1 (8)     (a1, b1)          B0(t+2)
//     4            A0(t+1) -> a0 (8)     (a1, b0)          B1(t+2)
// Every half-tile is issued 6 phases before it is read and waited for 5 phases after its issue, which is ONE counted
// wait per phase: s_waitcnt vmcnt(10) (the five younger half-tiles stay in flight across the barriers; never 0 in the
// steady state).  The wait sits in the memory part of the phase BEFORE the one that reads the half-tile, so both groups
// have passed it (and a barrier) before either reads; a slot is re-staged two phases after its last ds_read, when the
// later group's lgkmcnt(0) has retired those reads too.
#pragma once
#include "common.h"
#include "kernels.h"
#include <type_traits>

// host side: the ONE switch over (epilogue mode, operand type).  f(integral_constant<int, EPI>, OT tag value) runs for the pair; the
// launchers instantiate their kernel from the two types and set its attribute once per device there
template <typename F>
inline void gemm_epi_dispatch(int mode, bool f16, F&& f) {
  auto by_type = [&](auto e) { if (f16) f(e, f16_t{}); else f(e, bf16_t{}); };
  switch (mode) {
    case EPI_STORE: by_type(std::integral_constant<int, EPI_STORE>{}); break;
    case EPI_STORE_BF16: by_type(std::integral_constant<int, EPI_STORE_BF16>{}); break;
    case EPI_RESIDUAL: by_type(std::integral_constant<int, EPI_RESIDUAL>{}); break;
    case EPI_GELU_BF16: by_type(std::integral_constant<int, EPI_GELU_BF16>{}); break;
    case EPI_TOKENS: by_type(std::integral_constant<int, EPI_TOKENS>{}); break;
    default: by_type(std::integral_constant<int, EPI_QKV>{}); break;
  }
}

// bijective XCD-aware remap (cdna_hip_programming.md, T1): blocks b and b+8 share an XCD, so one XCD's L2 sees consecutive tiles
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// 16-byte-chunk XOR key of row r of a [rows][64 k] LDS image (128-byte rows), on the DMA source address and on the ds_read
__device__ __forceinline__ int tile_key_a(int r) { return (r >> 1) & 7; }
// the ping-pong loop reads its B half-tiles with their rows permuted (read_b below), so their key is a different function of the row:
// distinct over the 16 rows one fragment read touches, {8a + 4j + b : a, b = 0..3}
__device__ __forceinline__ int tile_key_b_perm(int r) { return ((r >> 1) & 1) | (((r >> 3) & 3) << 1); }

#define GEMM_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// LDS pointers are typed as such: the loop below is simplified on its own before it is inlined, and on generic pointers it came out
// with other scalar code than the kernels' own copies had
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;
constexpr int kPpBM = 256, kPpBN = 256, kPpBK = 64;
constexpr int kPpHalf = 16384;          // one half-tile: 128 rows x 64 k
constexpr int kPpBuf = 65536;           // one K-tile buffer [A0 | A1 | B0 | B1]; the loop uses two

// LDS-DMA lane offsets of the ping-pong loop: this lane's two pieces (8 rows x 128 B) of every half-tile, relative to the half-tile's
// first row.  SPLIT (fp16x2 operands): chunks 0-3 of an LDS row are k .. k + 31 of the hi half, chunks 4-7 the same k of the lo half,
// which starts at element column a_lo / b_lo of the source row
template <bool SPLIT>
__device__ __forceinline__ void pp_lane_offsets(int wave, int lane, int lda, int ldb, int a_lo, int b_lo, int (&a_off)[2], int (&b_off)[2]) {
  const int sr = lane >> 3, scp = lane & 7;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wave * 2 + i) * 8 + sr;                      // row inside the half-tile, 0..127
    const int c = scp ^ tile_key_a(r);
    const int cb = scp ^ tile_key_b_perm(r);
    if constexpr (SPLIT) {
      a_off[i] = r * lda * 2 + (c < 4 ? c * 16 : a_lo * 2 + (c - 4) * 16);
      b_off[i] = r * ldb * 2 + (cb < 4 ? cb * 16 : b_lo * 2 + (cb - 4) * 16);
    } else {
      a_off[i] = r * lda * 2 + c * 16;
      b_off[i] = r * ldb * 2 + cb * 16;
    }
  }
}

// acc += A[256 rows, nk K tiles] . B[256 rows, same]^T for one 256 x 256 tile, all eight waves of the workgroup.  rs_a / rs_b: buffer
// resources whose base is the tile's first A / B row (rows past num_records read as zeros); smem: 2 * kPpBuf bytes; nk >= 2.
// OT = operand type tag (common.h): the MFMA opcode.  SPLIT: a K tile covers 32 values of k, the k-step-0 fragments are the hi operands
// and the k-step-1 fragments the lo operands, and a phase multiplies a_hi.b_lo, a_lo.b_hi, a_hi.b_hi (small terms first).
// acc[A half][B half][row tile][col tile]: the products are taken as (B-fragment) x (A-fragment), i.e. transposed 16x16 tiles, and the B
// rows are permuted on the way in, so lane (fq, fr) holds for row tile i of quadrant (x, y) row x*128 + grp*64 + i*16 + fr and the EIGHT
// CONSECUTIVE columns y*128 + wc*32 + fq*8 + j*4 + e (j = col tile, e = register).
// On return every LDS read of the tile has retired in both groups: the caller may stage the next tile.
template <typename OT, bool SPLIT>
__device__ __forceinline__ void pp_tile_loop(lds_char* smem, __amdgpu_buffer_rsrc_t rs_a, __amdgpu_buffer_rsrc_t rs_b, const int (&a_off)[2],
                                             const int (&b_off)[2], int lda, int ldb, int nk, int wave, int lane, f32x4 (&acc)[2][2][4][2]) {
  const int grp = wave >> 2, wc = wave & 3;                     // group (= M position), N position
  // slot X of buffer b: A0 = 0, A1 = 1, B0 = 2, B1 = 3; the half-tile / K-tile displacement goes into the scalar offset
  auto stage_a = [&](int hf, int kt) {
    lds_char* dst = smem + (kt & 1) * kPpBuf + hf * kPpHalf + wave * 2048;
    const int so = hf * 128 * lda * 2 + kt * (SPLIT ? kPpBK : kPpBK * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, a_off[i], so, 0, 0);
  };
  auto stage_b = [&](int hf, int kt) {
    lds_char* dst = smem + (kt & 1) * kPpBuf + (2 + hf) * kPpHalf + wave * 2048;
    const int so = hf * 128 * ldb * 2 + kt * (SPLIT ? kPpBK : kPpBK * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, b_off[i], so, 0, 0);
  };

  const int fr = lane & 15, fq = lane >> 4;
  bf16x8 a0[2][4], a1[2][4], b0[2][2], b1[2][2];                // [k-step][tile]
  auto read_a = [&](bf16x8 (&af)[2][4], int slot, int kt) {
    const lds_char* base = smem + (kt & 1) * kPpBuf + slot * kPpHalf;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // row r + i * 16: the key does not see i * 16, so the row tile is a constant on the ADDRESS (the ds_read's immediate offset;
        // written into r, the shared function kept one more address register than the kernels' own copies of this loop had)
        const int r = grp * 64 + fr;
        af[ks][i] = *(const lds_bf16x8*)(base + r * 128 + (((ks * 4 + fq) ^ tile_key_a(r)) << 4) + i * 2048);
      }
  };
  auto read_b = [&](bf16x8 (&bf)[2][2], int slot, int kt) {
    const lds_char* base = smem + (kt & 1) * kPpBuf + slot * kPpHalf;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // MFMA row fr of tile j <- column 8*(fr >> 2) + 4*j + (fr & 3) of the wave's 32: the transposed accumulators of the two
        // tiles then hold EIGHT CONSECUTIVE columns per lane (4*fq' .. : j = 0 | j = 1), one 16-byte store in bf16, 32 B in fp32
        const int r = wc * 32 + (fr >> 2) * 8 + j * 4 + (fr & 3);
        bf[ks][j] = *(const lds_bf16x8*)(base + r * 128 + (((ks * 4 + fq) ^ tile_key_b_perm(r)) << 4));
      }
  };
  auto mma = [&](f32x4 (&c)[4][2], const bf16x8 (&af)[2][4], const bf16x8 (&bf)[2][2]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    if constexpr (SPLIT) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          c[i][j] = op16<OT>::mfma(bf[1][j], af[0][i], c[i][j]);
          c[i][j] = op16<OT>::mfma(bf[0][j], af[1][i], c[i][j]);
        }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) c[i][j] = op16<OT>::mfma(bf[0][j], af[0][i], c[i][j]);
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) c[i][j] = op16<OT>::mfma(bf[ks][j], af[ks][i], c[i][j]);   // D^T
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto bar = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- prologue: the stream up to (not including) phase 1 of tile 0's issue
  stage_a(0, 0); stage_b(0, 0); stage_b(1, 0); stage_a(1, 0);     // A0 B0 B1 A1 of K tile 0
  stage_a(0, 1); stage_b(0, 1); stage_b(1, 1);                    // A0 B0 B1 of K tile 1 (nk >= 2)
  GEMM_VMCNT(10);
  bar();
  read_a(a0, 0, 0);
  if (grp == 1) bar();                                           // group 1 runs one barrier behind
  for (int kt = 0; kt < nk; ++kt) {
    const bool full = kt + 2 < nk;                               // every issue of this tile's phases is real
    // phase 1
    read_b(b0, 2, kt);
    if (kt + 1 < nk) stage_a(1, kt + 1);
    if (full) GEMM_VMCNT(10); else GEMM_VMCNT(0);
    bar();
    mma(acc[0][0], a0, b0);
    bar();
    // phase 2
    read_b(b1, 3, kt);
    if (full) { stage_a(0, kt + 2); GEMM_VMCNT(10); } else GEMM_VMCNT(0);
    bar();
    mma(acc[0][1], a0, b1);
    bar();
    // phase 3
    read_a(a1, 1, kt);
    if (full) { stage_b(0, kt + 2); GEMM_VMCNT(10); } else GEMM_VMCNT(0);
    bar();
    mma(acc[1][1], a1, b1);
    bar();
    // phase 4
    if (kt + 1 < nk) read_a(a0, 0, kt + 1);
    if (full) { stage_b(1, kt + 2); GEMM_VMCNT(10); } else GEMM_VMCNT(0);
    bar();
    mma(acc[1][0], a1, b0);
    bar();
  }
  if (grp == 0) bar();                                           // pairs with group 1's last barrier: every LDS read of this tile has retired
}

// ---- what an epilogue mode (kernels.h: EPI_*) does with acc + bias, once for both lane shapes: W = 1 (the 128 x 128 kernel: one element
// per lane and register) and W = 8 consecutive columns of a row (the ping-pong kernel: 16-byte accesses).  Only the memory accesses and
// the 16-bit conversion differ with W; the masks, gelu, the pre-activation keep, the q scale, the pe row and the index arithmetic do not.
template <int W> __device__ __forceinline__ void epi_load_f32(const float* p, float (&v)[W]) {
  if constexpr (W == 8) {
    const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    v[0] = *p;
  }
}
template <int W> __device__ __forceinline__ void epi_store_f32(float* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    ((float4*)p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4*)p)[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    *p = v[0];
  }
}
template <typename OT, int W> __device__ __forceinline__ void epi_store_16(bf16_t* p, const float (&v)[W]) {     // saturating
  if constexpr (W == 8) {
    uint4 pk;
    pk.x = op16<OT>::pack2_sat(v[0], v[1]); pk.y = op16<OT>::pack2_sat(v[2], v[3]); pk.z = op16<OT>::pack2_sat(v[4], v[5]); pk.w = op16<OT>::pack2_sat(v[6], v[7]);
    *(uint4*)p = pk;
  } else {
    *p = op16<OT>::cvt_sat(v[0]);
  }
}
template <int W> __device__ __forceinline__ void epi_dropout(float (&o)[W], unsigned long long seed, size_t at, unsigned thresh, float scale) {
  if (thresh) {
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = dropout_keep_(seed, at + e, thresh) ? o[e] * scale : 0.f;
  }
}
// o = acc + bias of row m, columns n .. n + W - 1.  C: the fp32 destination (EPI_STORE, EPI_RESIDUAL, EPI_TOKENS); out16: the 16-bit one
// (EPI_STORE_BF16, EPI_GELU_BF16); both with leading dimension ldc.  EPI_QKV with W = 8 needs dh % 8 == 0 and emb % 8 == 0.
template <int EPI, typename OT, int W>
__device__ __forceinline__ void gemm_epilogue(float (&o)[W], int m, int n, int ldc, float* C, bf16_t* out16, const GemmEpi& epi) {
  const size_t at = (size_t)m * ldc + n;                          // also the element index of the dropout masks
  if constexpr (EPI == EPI_STORE) {
    epi_store_f32<W>(C + at, o);
  } else if constexpr (EPI == EPI_STORE_BF16) {
    epi_store_16<OT, W>(out16 + at, o);
  } else if constexpr (EPI == EPI_GELU_BF16) {                    // FFN-1: 16-bit(drop(gelu(.)))
    if (epi.pre_f32) epi_store_f32<W>(epi.pre_f32 + at, o);       // training: keep the pre-activation for gelu'
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = gelu_erf_(o[e]);
    epi_dropout<W>(o, epi.drop_seed, at, epi.drop_thresh, epi.drop_scale);
    epi_store_16<OT, W>(out16 + at, o);
  } else if constexpr (EPI == EPI_RESIDUAL) {                     // x += drop2(drop(.)): the fp32 residual stream, in place
    epi_dropout<W>(o, epi.drop_seed, at, epi.drop_thresh, epi.drop_scale);
    epi_dropout<W>(o, epi.drop2_seed, at, epi.drop2_thresh, epi.drop2_scale);
    float r[W];
    epi_load_f32<W>(C + at, r);
#pragma unroll
    for (int e = 0; e < W; ++e) r[e] = r[e] + o[e];
    epi_store_f32<W>(C + at, r);
  } else if constexpr (EPI == EPI_TOKENS) {                       // x[b, t] = . + pe[t]: row m = b n_tok + t goes to row m + b
    const int b = m / epi.n_tok, t = m - b * epi.n_tok;
    float pe[W];
    epi_load_f32<W>(epi.pe + (size_t)t * ldc + n, pe);
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = o[e] + pe[e];
    epi_store_f32<W>(C + (size_t)(m + b) * ldc + n, o);
  } else {                                                        // EPI_QKV: head split into Q (scaled), K, V [B,h,n_tok,dh]
    const int b = m / epi.n_tok, t = m - b * epi.n_tok;
    const int blk = n / epi.emb, r = n - blk * epi.emb, which = blk + epi.which0;
    const int hd = r / epi.dh, d = r - hd * epi.dh;
    const size_t bh = (size_t)b * epi.heads + hd;
    const float sc = which == 0 ? epi.q_scale : 1.f;
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = o[e] * sc;
    bf16_t* dst = which == 0 ? (bf16_t*)epi.q : which == 1 ? (bf16_t*)epi.k : (bf16_t*)epi.vn;
    epi_store_16<OT, W>(dst + (bh * epi.n_tok + t) * epi.dh + d, o);
  }
}
