// Dense "NT" GEMMs of the MiniROAD path:  C[M,N] = A[M,K] . B[N,K]^T + bias[N]
// (nn.Linear semantics: both operands K-contiguous).  Call sites replaced:
//   layer1[0]  Linear(4096,2048)      model/rnn/rnn.py:40     M = packed rows, N = 2048, K = 4096
//   GRU input projection W_ih          model/rnn/rnn.py:38,61  M = packed rows, N = 3072, K = 2048
//
// bf16 kernel (the product path): 128x128x64 tiles, 4 waves (2x2, 64x64 each), 16x16x32 bf16 MFMA,
// fp32 accumulate.  Operands go HBM -> LDS with 16-byte LDS-DMA (global_load_lds_dwordx4); the LDS image
// is lane-linear per wave-instruction (8 rows x 128 B), the 16-byte chunk XOR-swizzle sits on the SOURCE
// address and on the ds_read address (cdna_hip_programming.md rule 21) so the ds_read_b128 fragments are
// bank-conflict free.  Two LDS buffers, one barrier per K tile.  Block ids are remapped so that one XCD's
// L2 sees consecutive N tiles of the same M tile (A rows are re-used from L2).
// Two larger bf16 kernels with the plain bias epilogue follow it (256x128 three-stage, 256x256 two-stage).
//
// fp32 kernel (parity mode): exact-fp32 MFMA 16x16x4 (bit-for-bit an fmaf chain), register staged.
//
// At the end of the file: gemm_nt_choose, the ONE place that decides which kernel an NT product runs on (these, the ping-pong kernel
// of gemm_pp.hip, the split-K workgroup of gemm_tn.hip), and launch_gemm_nt_kernel, the ONE launcher.
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"

#define BM 128
#define BN 128
#define BK 64

template <typename OutT, int EPI, typename OT = bf16_t>
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_kernel(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, const float* __restrict__ bias,
    OutT* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc, GemmEpi epi) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][A 16 KB | B 16 KB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = N / BN;
  const int ntm = (M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;

  // per-lane staging source (row within the 8-row group of a wave-instruction, swizzled chunk)
  const int sr = lane >> 3;          // 0..7
  const int scp = lane & 7;          // chunk position in LDS
  const bf16_t* a_src[4];
  const bf16_t* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + sr;                 // tile row 0..127
    const int c = scp ^ tile_key_a(r);                    // source chunk that lands at position scp
    int ar = m0 + r; if (ar > M - 1) ar = M - 1;           // clamp: rows past M are never stored
    a_src[i] = A + (size_t)ar * lda + c * 8;
    b_src[i] = B + (size_t)(n0 + r) * ldb + c * 8;
  }
  auto stage = [&](int buf, int kt) {
    char* la = smem + buf * 32768;
    char* lb = la + 16384;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = (wave * 4 + i) * 1024;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (size_t)kt * BK),
                                       (__attribute__((address_space(3))) void*)(la + off), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + (size_t)kt * BK),
                                       (__attribute__((address_space(3))) void*)(lb + off), 16, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment read offsets: row = w*64 + i*16 + (lane&15); chunk = ks*4 + (lane>>4), swizzled
  const int fr = lane & 15, fq = lane >> 4;
  auto compute = [&](int buf) {
    const char* la = smem + buf * 32768;
    const char* lb = la + 16384;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ra = wm * 64 + i * 16 + fr;
        af[i] = *(const bf16x8*)(la + ra * 128 + (((ks * 4 + fq) ^ tile_key_a(ra)) << 4));
        const int rb = wn * 64 + i * 16 + fr;
        bfr[i] = *(const bf16x8*)(lb + rb * 128 + (((ks * 4 + fq) ^ tile_key_a(rb)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = op16<OT>::mfma(af[i], bfr[j], acc[i][j]);
    }
  };

  const int nk = K / BK;
  stage(0, 0);
  __syncthreads();                      // emits vmcnt(0): tile 0 landed
  int cur = 0;
  for (int kt = 0; kt < nk - 1; ++kt) {
    stage(cur ^ 1, kt + 1);
    compute(cur);
    __syncthreads();                    // vmcnt(0) + barrier: next tile landed, everyone done reading cur
    cur ^= 1;
  }
  compute(cur);

  // epilogue: D layout col = lane&15, row = (lane>>4)*4 + j
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fr;
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm * 64 + i * 16 + fq * 4 + e;
        if (m < M) {
          float v[1] = {acc[i][j][e] + bv};
          gemm_epilogue<EPI, OT, 1>(v, m, n, ldc, (float*)C, (bf16_t*)epi.out_b, epi);      // one element per lane: scalar accesses
        }
      }
    }
}


// ------------------------------------------------------------------------------------------------------
// Large-M variant for the two eval-path projections: 256x128x64 tiles, 8 waves (4 x 2, 64x64 each = two waves per
// SIMD), THREE LDS stages (144 KB, one workgroup per CU) with the prefetch two K tiles ahead: the loop waits with a
// COUNTED vmcnt (the newest tile stays in flight across the barrier) and uses a raw s_barrier, so the LDS-DMA of tile
// kt+2 and kt+1 overlap the MFMAs of tile kt (cdna_hip_programming.md "Pipelining across barriers", 3-buffer span).
// One barrier per K tile: passing barrier(kt) proves every wave finished computing tile kt-1, whose buffer is the one
// stage(kt+2) overwrites.  Same lane-linear LDS image + source/read XOR swizzle as the 128x128 kernel.
// ------------------------------------------------------------------------------------------------------
#define GBM 256
#define GSTAGE 49152          // A 32 KB + B 16 KB
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_big_kernel(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, const float* __restrict__ bias,
    float* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [3][A 32 KB | B 16 KB]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;                      // 4 x 2
  const int ntn = N / BN;
  const int ntm = (M + GBM - 1) / GBM;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * GBM, n0 = (tile % ntn) * BN;

  const int sr = lane >> 3, scp = lane & 7;
  // A: 32 wave-instructions per stage (4 per wave), B: 16 (2 per wave)
  const bf16_t* a_src[4];
  const bf16_t* b_src[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + sr;                 // 0..255
    const int c = scp ^ tile_key_a(r);
    int ar = m0 + r; if (ar > M - 1) ar = M - 1;
    a_src[i] = A + (size_t)ar * lda + c * 8;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wave * 2 + i) * 8 + sr;                 // 0..127
    const int c = scp ^ tile_key_a(r);
    b_src[i] = B + (size_t)(n0 + r) * ldb + c * 8;
  }
  auto stage = [&](int buf, int kt) {
    char* la = smem + buf * GSTAGE;
    char* lb = la + 32768;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (size_t)kt * BK),
                                       (__attribute__((address_space(3))) void*)(la + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + (size_t)kt * BK),
                                       (__attribute__((address_space(3))) void*)(lb + (wave * 2 + i) * 1024), 16, 0, 0);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  auto compute = [&](int buf) {
    const char* la = smem + buf * GSTAGE;
    const char* lb = la + 32768;
    // all 16 fragments of the K tile are requested up front (64 VGPRs): the MFMAs of k-step 0 run under the LDS
    // latency of k-step 1's fragments instead of each group of 8 MFMAs waiting for its own reads
    bf16x8 af[2][4], bfr[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ra = wm * 64 + i * 16 + fr;
        af[ks][i] = *(const bf16x8*)(la + ra * 128 + (((ks * 4 + fq) ^ tile_key_a(ra)) << 4));
        const int rb = wn * 64 + i * 16 + fr;
        bfr[ks][i] = *(const bf16x8*)(lb + rb * 128 + (((ks * 4 + fq) ^ tile_key_a(rb)) << 4));
      }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bfr[ks][j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  const int nk = K / BK;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt landed (6 LDS-DMA per wave per tile; leave the newer tile in flight), then meet
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");                      // no LDS access may be scheduled above the barrier
    // (staggering waves 4-7 - prefetch after their MFMAs - measured 8 % slower here: 828 vs 905 TFLOP/s)
    if (kt + 2 < nk) stage((kt + 2) % 3, kt + 2);
    compute(kt % 3);
  }

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fr;
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm * 64 + i * 16 + fq * 4 + e;
        if (m < M) C[(size_t)m * ldc + n] = acc[i][j][e] + bv;
      }
    }
}

// The production kernel before the ping-pong kernel, and its fallback for the shapes that one does not take (no bias vector, K < 128):
// 256x256x64 tile, 8 waves as 2 (M) x 4 (N), wave tile 128x64 = 8x4 MFMA tiles (128 accumulator registers), two LDS stages
// of 64 KB (A 32 KB + B 32 KB), ONE barrier per K tile.  Per K tile a wave issues 8 LDS-DMA pieces, 24 ds_read_b128 and 64
// MFMAs; the fragment reads of phase p+1 are issued before the MFMAs of phase p (register double buffer) and the next tile's
// 8 DMA pieces go out in the first two phases (4 + 4), each group right behind a phase's fragment reads, so that one wave's
// DMA issue (80-190 cycles per piece, measured) runs beside its SIMD partner's MFMAs.
#define XBM 256
#define XBN 256
#define XBK 64
#define XSTAGE 65536
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_256sq_kernel(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, const float* __restrict__ bias,
    float* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][A 32 KB | B 32 KB]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;                      // 2 x 4
  const int ntn = N / XBN;
  const int ntm = (M + XBM - 1) / XBM;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * XBM, n0 = (tile % ntn) * XBN;
  const int sr = lane >> 3, scp = lane & 7;
  const bf16_t* a_src[4];
  const bf16_t* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + sr;                 // 0..255
    const int c = scp ^ tile_key_a(r);
    int ar = m0 + r; if (ar > M - 1) ar = M - 1;
    a_src[i] = A + (size_t)ar * lda + c * 8;
    b_src[i] = B + (size_t)(n0 + r) * ldb + c * 8;
  }
  auto stage = [&](int buf, int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      char* la = smem + buf * XSTAGE;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (size_t)kt * XBK),
                                       (__attribute__((address_space(3))) void*)(la + (wave * 4 + i) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + (size_t)kt * XBK),
                                       (__attribute__((address_space(3))) void*)(la + 32768 + (wave * 4 + i) * 1024), 16, 0, 0);
    }
  };
  auto stage_piece = [&](int buf, int kt, int i) {
    char* la = smem + buf * XSTAGE;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (size_t)kt * XBK),
                                     (__attribute__((address_space(3))) void*)(la + (wave * 4 + i) * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + (size_t)kt * XBK),
                                     (__attribute__((address_space(3))) void*)(la + 32768 + (wave * 4 + i) * 1024), 16, 0, 0);
  };
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  auto lda_frag = [&](const char* la, int ks, int h, bf16x8 (&af)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ra = wm * 128 + h * 64 + i * 16 + fr;
      af[i] = *(const bf16x8*)(la + ra * 128 + (((ks * 4 + fq) ^ tile_key_a(ra)) << 4));
    }
  };
  auto ldb_frag = [&](const char* lb, int ks, bf16x8 (&bfr)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rb = wn * 64 + j * 16 + fr;
      bfr[j] = *(const bf16x8*)(lb + rb * 128 + (((ks * 4 + fq) ^ tile_key_a(rb)) << 4));
    }
  };
  auto mma = [&](int h, const bf16x8 (&af)[4], const bf16x8 (&bfr)[4]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[h * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[h * 4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  const int nk = K / XBK;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tile kt landed (nothing newer is in flight yet)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");                      // no LDS access may be scheduled above the barrier
    const char* la = smem + (kt & 1) * XSTAGE;
    const char* lb = la + 32768;
    const int nbuf = (kt + 1) & 1;
    const bool pre = kt + 1 < nk;
    bf16x8 a0[4], a1[4], b0[4], b1[4];
    ldb_frag(lb, 0, b0); lda_frag(la, 0, 0, a0);
    lda_frag(la, 0, 1, a1);
    if (pre) { stage_piece(nbuf, kt + 1, 0); stage_piece(nbuf, kt + 1, 1); }
    mma(0, a0, b0);
    ldb_frag(lb, 1, b1); lda_frag(la, 1, 0, a0);
    if (pre) { stage_piece(nbuf, kt + 1, 2); stage_piece(nbuf, kt + 1, 3); }
    mma(1, a1, b0);
    lda_frag(la, 1, 1, a1);
    mma(0, a0, b1);
    mma(1, a1, b1);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fr;
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm * 128 + i * 16 + fq * 4 + e;
        if (m < M) C[(size_t)m * ldc + n] = acc[i][j][e] + bv;
      }
    }
}

// ------------------------------------------------------------------------------------------
// exact fp32 GEMM: 128x128x16 tiles, v_mfma_f32_16x16x4_f32.  Each lane reads 4 consecutive k
// (one ds_read_b128) and feeds element j to the j-th MFMA; A and B use the same k permutation,
// so the sum is over the same 16 k values.
// ------------------------------------------------------------------------------------------
#define FK 16
#define FLD 20
template <int DUMMY>
__global__ __launch_bounds__(256) void gemm_f32_nt_kernel(
    const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ bias,
    float* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc) {
  __shared__ __attribute__((aligned(16))) float sa[BM * FLD];
  __shared__ __attribute__((aligned(16))) float sb[BN * FLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (N + BN - 1) / BN;
  const int ntm = (M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += FK) {
    float4 ra[2], rb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256;          // 512 float4 per operand tile
      const int r = idx >> 2, c4 = idx & 3;
      int ar = m0 + r; if (ar > M - 1) ar = M - 1;
      int br = n0 + r; if (br > N - 1) br = N - 1;
      ra[i] = *(const float4*)(A + (size_t)ar * lda + k0 + c4 * 4);
      rb[i] = *(const float4*)(B + (size_t)br * ldb + k0 + c4 * 4);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 2, c4 = idx & 3;
      *(float4*)(sa + r * FLD + c4 * 4) = ra[i];
      *(float4*)(sb + r * FLD + c4 * 4) = rb[i];
    }
    __syncthreads();
    float4 af[4], bfv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = *(const float4*)(sa + (wm * 64 + i * 16 + fr) * FLD + fq * 4);
      bfv[i] = *(const float4*)(sb + (wn * 64 + i * 16 + fr) * FLD + fq * 4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bfv[j].x, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bfv[j].y, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bfv[j].z, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bfv[j].w, acc[i][j], 0, 0, 0);
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fr;
      if (n < N) {
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + wm * 64 + i * 16 + fq * 4 + e;
          if (m < M) C[(size_t)m * ldc + n] = acc[i][j][e] + bv;
        }
      }
    }
}

// fp32: K % 16 == 0; M, N arbitrary
void launch_gemm_f32_nt(const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, int M,
                        int N, int K, hipStream_t s) {
  if (M <= 0) return;
  const int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN;
  gemm_f32_nt_kernel<0><<<ntm * ntn, 256, 0, s>>>(A, B, bias, C, M, N, K, lda, ldb, ldc);
}

// ------------------------------------------------------------------------------------------------------
// Which kernel an NT product runs on.  The table (DESIGN.md section 4a has it in full); the numbered steps are tried in order:
//   fp16 operands, any entry      ping-pong at M >= 4096 where it takes the shape, else 128 x 128; never the three bf16-only kernels
//   plain projection, bf16        1. split-K   train_splitk, <= 256 tiles of 128 x 128, K >= 1024, launch_gemm_bf16_tn's own conditions
//                                 2. M >= 4096 and N % 256 == 0: ping-pong, or 256 x 256 where ping-pong refuses
//                                 3. M >= 2048: 256 x 128
//                                 4. the epilogue path
//   epilogue path                 ping-pong at M >= 4096 where it takes the shape, else 128 x 128
// A line marked "odd" is kept as it was found, not as it would be written today.
// ------------------------------------------------------------------------------------------------------
// launch_gemm_bf16_tn's acceptance of nn.Linear's form (ta = tb = false, all of K present): its refusals above its first launch
static bool splitk_takes(int M, int N, int K, int lda, int ldb) {
  if (K % 64 || K <= 0 || M <= 0 || N <= 0 || lda % 8 || ldb % 8 || lda <= 0 || ldb <= 0) return false;
  const long long ldmax = lda > ldb ? lda : ldb;
  if ((long long)K * ldmax * 2 > 0x7fffffffll || (long long)M * lda * 2 > 0x7fffffffll || 129ll * ldmax * 2 + (long long)K * 2 > 0x7fffffffll)
    return false;
  return (long long)((M + 127) / 128) * ((N + 127) / 128) <= 256 && K >= 128;
}

GemmNtKernel gemm_nt_choose(const GemmNtQuery& q, GemmNtKnobs knobs) {
  if (q.M <= 0) return GEMM_NT_NONE;
  const bool pp = gemm_pingpong_takes(q.M, q.N, q.K, q.has_bias, q.mode, q.dh, q.emb);
  if (q.entry == GEMM_NT_PLAIN && !q.f16) {     // odd: fp16 operands skip this block whole, train_splitk included
    if (q.train_splitk && !knobs.no_splitk && q.K >= 1024 && splitk_takes(q.M, q.N, q.K, q.lda, q.ldb)) return GEMM_NT_SPLITK;
    if (q.M >= 4096 && q.N % 256 == 0 && !knobs.no_big)   // odd: a NULL bias refuses ping-pong here at every N, not only above 8192
      return !knobs.no_pingpong && q.has_bias && pp ? GEMM_NT_PINGPONG : GEMM_NT_256SQ;
    if (q.M >= 2048 && !knobs.no_big) return GEMM_NT_256X128;
  }
  // odd: the MiniROAD 16-bit projection takes ping-pong without looking at NO_PINGPONG; the knob holds only for its bias-less calls
  if (q.entry == GEMM_NT_PROJ16 && q.M >= 4096 && q.has_bias && pp) return GEMM_NT_PINGPONG;
  // the epilogue path.  odd: with NO_BIG alone a plain projection of M >= 4096 still lands on ping-pong here
  if (q.M >= 4096 && !knobs.no_pingpong && pp) return GEMM_NT_PINGPONG;
  return GEMM_NT_128;
}

// one instantiation's launch, its dynamic-LDS attribute set once per device
template <typename... P, typename... Args>
static void launch_with_lds(void (*kern)(P...), DeviceOnce& once, int grid, int block, int lds, hipStream_t s, Args... args) {
  once.run([&] { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
  kern<<<grid, block, lds, s>>>(args...);
}

// bf16: requires N % 128 == 0, K % 64 == 0 (checked by the caller); M arbitrary (> 0)
int launch_gemm_nt_kernel(GemmNtKernel kind, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M,
                          int N, int K, GemmEpi epi, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)A; const bf16_t* b = (const bf16_t*)B;
  const bool plain = epi.mode == EPI_STORE && !epi.f16;      // all that the three bf16-only kernels carry: bias, fp32 C
  switch (kind) {
    case GEMM_NT_NONE: return 0;
    case GEMM_NT_PINGPONG:                                     // the destination is epi.out_b for EPI_STORE_BF16, and C otherwise
      return launch_gemm_bf16_pingpong_epi(A, lda, B, ldb, bias, epi.mode == EPI_STORE_BF16 ? epi.out_b : (void*)C, ldc, M, N, K, epi, s);
    case GEMM_NT_SPLITK:
      return plain ? launch_gemm_bf16_tn(false, false, A, lda, B, ldb, bias, C, ldc, M, N, K, K, nullptr, s) : -1;
    case GEMM_NT_256X128: {
      if (!plain) return -1;
      static DeviceOnce once;
      launch_with_lds(gemm_bf16_nt_big_kernel, once, ((M + GBM - 1) / GBM) * (N / BN), 512, 3 * GSTAGE, s, a, b, bias, C, M, N, K, lda, ldb, ldc);
      return 0;
    }
    case GEMM_NT_256SQ: {
      if (!plain || N % XBN) return -1;
      static DeviceOnce once;
      launch_with_lds(gemm_bf16_nt_256sq_kernel, once, ((M + XBM - 1) / XBM) * (N / XBN), 512, 2 * XSTAGE, s, a, b, bias, C, M, N, K, lda, ldb, ldc);
      return 0;
    }
    case GEMM_NT_128:
      gemm_epi_dispatch(epi.mode, epi.f16 != 0, [&](auto e, auto ot) {
        static DeviceOnce once;                                  // one per (mode, operand type): the lambda is instantiated per pair
        launch_with_lds(gemm_bf16_nt_kernel<float, decltype(e)::value, decltype(ot)>, once, ((M + BM - 1) / BM) * (N / BN), 256, 65536, s, a, b,
                        bias, C, M, N, K, lda, ldb, ldc, epi);
      });
      return 0;
  }
  return -1;
}

void launch_gemm_nt(int entry, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, int ldc, int M, int N, int K,
                    GemmEpi epi, bool train_splitk, hipStream_t s) {
  static const GemmNtKnobs knobs = {prego_tune_env("PREGO_GEMM_NO_BIG") != nullptr, prego_tune_env("PREGO_GEMM_NO_SPLITK") != nullptr,
                                    prego_tune_env("PREGO_GEMM_NO_PINGPONG") != nullptr};
  GemmNtQuery q = {entry, M, N, K, lda, ldb, bias != nullptr, epi.f16 != 0, train_splitk, epi.mode, epi.dh, epi.emb};
  if (launch_gemm_nt_kernel(gemm_nt_choose(q, knobs), A, lda, B, ldb, bias, C, ldc, M, N, K, epi, s) != 0 && q.train_splitk) {
    q.train_splitk = false;      // splitk_takes and gemm_tn.hip disagree: the product still runs, on the kernel it had without the flag
    (void)launch_gemm_nt_kernel(gemm_nt_choose(q, knobs), A, lda, B, ldb, bias, C, ldc, M, N, K, epi, s);
  }
}
