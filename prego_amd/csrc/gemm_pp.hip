// bf16 NT GEMM, 256x256x64 tiles, ping-pong schedule (gemm_tile.h: pp_tile_loop, where the schedule is described):
//   C[M,N] (fp32) = A[M,K] (bf16) * B[N,K]^T (bf16) + bias      layer1 / W_ih projections, model/rnn/rnn.py:38-42,61
// This file: the tile selection, the persistent WORKER form, the eight-columns-per-lane epilogues, and the launchers.
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"

// EPI = what happens to acc + bias (kernels.h): EPI_STORE (fp32 C), EPI_STORE_BF16 (bf16 C: the inference path keeps the
// layer1 and W_ih projections in bf16 between the kernels), and the Transformer path's fused epilogues EPI_RESIDUAL (fp32
// x += .), EPI_GELU_BF16 (bf16(gelu(.))), EPI_QKV (head split into Q, K [B,h,N,dh] and V^T [B,h,dh,Npad]).  A lane holds 8
// consecutive columns of a row, so every epilogue is 16-byte vector accesses: gemm_epilogue<EPI, OT, 8> (gemm_tile.h; the 128 x 128
// kernel calls the same function with one element per lane).
// OT = operand type tag (common.h: bf16_t or f16_t): selects the MFMA opcode and the 16-bit output conversion only.
// WORKER (probe of DESIGN 5c, prego_debug_gemm_worker): a persistent workgroup that leaves at once on XCDs below epi.xcd_lo and
// otherwise claims tiles from the atomic counter epi.counter until none is left (m-major order: consecutive tiles share A rows).
// SPLIT (fp16x2 operands, common.h): A rows are [K hi | .. | K lo at column epi.split_a_lo], B rows likewise at epi.split_b_lo.  A K
// tile then covers 32 values of k and its 128-byte LDS row holds [32 hi | 32 lo]: the 16-byte chunks 0-3 of a row come from the hi
// half, chunks 4-7 from the lo half of the same k range (a per-lane constant in the DMA source offset, nothing else changes in the
// staging, the LDS ring or the wait counts), so the k-step-0 fragments ARE the hi operands and the k-step-1 fragments the lo
// operands, and a phase multiplies a_hi.b_lo, a_lo.b_hi, a_hi.b_hi (small terms first): 24 MFMAs behind the same 12 fragment
// reads and 2 DMA pieces that serve 16 in the 16-bit kernel - a third less LDS traffic and DMA per product than walking three K
// segments through the unchanged loop (the first fp16x2 form: 165 -> 136 ms per pass of the bench workload, 1.49 PFLOP/s of executed MFMA work).  The epilogue multiplies the
// weights' power-of-two scale out (epi.acc_scale: device pointer to 1 / scale) before the bias.
template <int EPI, typename OT = bf16_t, bool WORKER = false, bool SPLIT = false>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt_pingpong_kernel(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, const float* __restrict__ bias,
    void* __restrict__ Cv, int M, int N, int K, int lda, int ldb, int ldc, GemmEpi epi) {
  float* C = (float*)Cv;
  constexpr bool OUT_BF16 = EPI == EPI_STORE_BF16;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 buffers][A0 | A1 | B0 | B1]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, wc = wave & 3;                     // group (= M position wr), N position
  const int ntn = N / kPpBN;
  const int ntm = (M + kPpBM - 1) / kPpBM;
  const int ntiles = ntm * ntn;
  const int nk = SPLIT ? K / (kPpBK / 2) : K / kPpBK;           // SPLIT: a K tile = 32 values of k (hi and lo halves side by side)
  int idx = blockIdx.x;
  int tile = WORKER ? 0 : xcd_remap(idx, ntiles);
  int m0 = (tile / ntn) * kPpBM, n0 = (tile % ntn) * kPpBN;
  __shared__ int s_tile;
  if constexpr (WORKER) {
    const int xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7;           // HW_REG_XCC_ID
    if (xcc < epi.xcd_lo) return;
  }

  // ---- LDS-DMA sources: one buffer resource per operand and tile (base = the tile's first row, num_records = its valid rows: rows
  // past M read as zeros, no clamp), a 32-bit lane offset per piece (gemm_tile.h): 4 VGPRs of addressing in all
  int a_off[2], b_off[2];
  pp_lane_offsets<SPLIT>(wave, lane, lda, ldb, epi.split_a_lo, epi.split_b_lo, a_off, b_off);
  __amdgpu_buffer_rsrc_t rs_a, rs_b;
  auto set_sources = [&](int tm0, int tn0) {
    const int rows = M - tm0 < kPpBM ? M - tm0 : kPpBM;
    rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)tm0 * lda), 0, rows * lda * 2, 0x00020000);
    rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)tn0 * ldb), 0, kPpBN * ldb * 2, 0x00020000);
  };
  if constexpr (!WORKER) set_sources(m0, n0);
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[2][2][4][2];                                         // [A half][B half][row tile][col tile]
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[x][y][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (;;) {                                                     // one pass unless WORKER
  if constexpr (WORKER) {
    if (tid == 0) s_tile = (int)atomicAdd(epi.counter, 1u);
    __syncthreads();
    tile = s_tile;
    __syncthreads();
    if (tile >= ntiles) break;
    m0 = (tile / ntn) * kPpBM; n0 = (tile % ntn) * kPpBN;
    set_sources(m0, n0);
  }
  pp_tile_loop<OT, SPLIT>((lds_char*)smem, rs_a, rs_b, a_off, b_off, lda, ldb, nk, wave, lane, acc);

  const int cm0 = m0, cn0 = n0;
  // lane (fq, fr) holds, for row tile i of quadrant (x, y): row fr, columns y*128 + wc*32 + fq*8 + j*4 + e  (j = tile, e = register)
  float4 bv[2][2];
#pragma unroll
  for (int y = 0; y < 2; ++y)
#pragma unroll
    for (int j = 0; j < 2; ++j) bv[y][j] = *(const float4*)(bias + cn0 + y * 128 + wc * 32 + fq * 8 + j * 4);
  // ---- epilogue: the products were taken as (B-fragment) x (A-fragment), i.e. transposed 16x16 tiles, and the B rows were
  // permuted on the way in, so a lane holds EIGHT CONSECUTIVE COLUMNS of one row of C: one 16-byte store per row in bf16,
  // two in fp32 (the store tail of a tile is bound by the number of store instructions first, by bytes second)
  const bool whole = cm0 + kPpBM <= M;                             // wave-uniform: all the stores of this wave are issued
  float inv_scale = 1.f;
  if constexpr (SPLIT) { if (epi.acc_scale) inv_scale = *epi.acc_scale; }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int n = cn0 + y * 128 + wc * 32 + fq * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = cm0 + x * 128 + grp * 64 + i * 16 + fr;
        f32x4 v0 = acc[x][y][i][0], v1 = acc[x][y][i][1];
        if constexpr (SPLIT) { v0 *= inv_scale; v1 *= inv_scale; }
        if (whole || m < M) {
          float o[8] = {v0[0] + bv[y][0].x, v0[1] + bv[y][0].y, v0[2] + bv[y][0].z, v0[3] + bv[y][0].w,
                        v1[0] + bv[y][1].x, v1[1] + bv[y][1].y, v1[2] + bv[y][1].z, v1[3] + bv[y][1].w};
          gemm_epilogue<EPI, OT, 8>(o, m, n, ldc, C, EPI == EPI_GELU_BF16 ? (bf16_t*)epi.out_b : (bf16_t*)Cv, epi);
        }
        acc[x][y][i][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[x][y][i][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
  if constexpr (!WORKER) break;
  }
}

constexpr int kPpLds = 2 * kPpBuf;
// the launch of one instantiation, with its dynamic-LDS attribute set once per device
template <int EPI, typename OT, bool WORKER = false, bool SPLIT = false>
static void pp_launch(int grid, hipStream_t s, const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int lda, int ldb,
                      int ldc, const GemmEpi& epi) {
  auto* kern = gemm_bf16_nt_pingpong_kernel<EPI, OT, WORKER, SPLIT>;
  static DeviceOnce once;
  once.run([&] { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kPpLds); });
  kern<<<grid, 512, kPpLds, s>>>((const bf16_t*)A, (const bf16_t*)B, bias, C, M, N, K, lda, ldb, ldc, epi);
}
static int pp_tiles(int M, int N) { return ((M + kPpBM - 1) / kPpBM) * (N / kPpBN); }

__device__ float g_pp_zero_bias[8192];        // stands in for a NULL bias (the kernel's bias loads are unconditional)

// the shapes the kernel takes with the epilogue of `mode` (a pure function: gemm_nt_choose asks it, the launcher below enforces it)
bool gemm_pingpong_takes(int M, int N, int K, bool has_bias, int mode, int dh, int emb) {
  (void)M;
  if (N % kPpBN || K % kPpBK || K < 2 * kPpBK || (!has_bias && N > 8192)) return false;
  return !(mode == EPI_QKV && (dh % 8 || emb % 8));        // 8 consecutive columns must lie in one head of one of q / k / v
}

// C[M,N] = epilogue(A[M,K] . B[N,K]^T + bias) with the epilogue of epi.mode; bias may be NULL.  -1 = shape not supported.
int launch_gemm_bf16_pingpong_epi(const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc, int M, int N,
                                  int K, GemmEpi epi, hipStream_t s) {
  if (!gemm_pingpong_takes(M, N, K, bias != nullptr, epi.mode, epi.dh, epi.emb)) return -1;
  if (!bias) {
    static DeviceOnce once;
    static float* zero_bias[64] = {nullptr};
    const int dev = once.run([&] {
      int d = 0;
      (void)hipGetDevice(&d);
      if (d >= 0 && d < 64) (void)hipGetSymbolAddress((void**)&zero_bias[d], HIP_SYMBOL(g_pp_zero_bias));
    });
    bias = zero_bias[dev];
    if (!bias) return -1;
  }
  gemm_epi_dispatch(epi.mode, epi.f16 != 0, [&](auto e, auto ot) {
    pp_launch<decltype(e)::value, decltype(ot)>(pp_tiles(M, N), s, A, B, bias, C, M, N, K, lda, ldb, ldc, epi);
  });
  return 0;
}

// split-operand (fp16x2) projection: C[M,N] fp32 = (A_hi + A_lo)[M,K] . (B_hi + B_lo)[N,K]^T * inv_scale + bias, three fp16 products.
// A rows [.. lda fp16 ..] hold hi at column 0 and lo at column a_lo; B rows hi at 0 and lo at b_lo; any M (rows past M read as zeros).
int launch_gemm_x2_pingpong(const void* A, int lda, int a_lo, const void* B, int ldb, int b_lo, const float* inv_scale, const float* bias,
                            float* C, int ldc, int M, int N, int K, hipStream_t s) {
  if (N % kPpBN || K % (kPpBK / 2) || K < kPpBK || !bias || M <= 0) return -1;
  GemmEpi epi{};
  epi.mode = EPI_STORE; epi.f16 = 1; epi.split_a_lo = a_lo; epi.split_b_lo = b_lo; epi.acc_scale = inv_scale;
  pp_launch<EPI_STORE, f16_t, false, true>(pp_tiles(M, N), s, A, B, bias, C, M, N, K, lda, ldb, ldc, epi);
  return 0;
}

// The ping-pong kernel as a persistent worker: `grid` workgroups claim tiles from *counter (zero at launch) in m-major order; those that
// land on XCDs below xcd_lo leave at once.  out16: 16-bit C of the operand type (the inference projections), else fp32 C.
int launch_gemm_bf16_pingpong_worker(const void* A, int lda, const void* B, int ldb, const float* bias, void* C, int ldc, int M, int N,
                                     int K, int xcd_lo, unsigned* counter, int grid, hipStream_t s, bool out16, bool f16) {
  if (N % kPpBN || K % kPpBK || K < 2 * kPpBK || !bias || !counter) return -1;
  GemmEpi epi{};
  epi.mode = out16 ? EPI_STORE_BF16 : EPI_STORE; epi.xcd_lo = xcd_lo; epi.counter = counter; epi.f16 = f16 ? 1 : 0;
  if (!out16) pp_launch<EPI_STORE, bf16_t, true>(grid, s, A, B, bias, C, M, N, K, lda, ldb, ldc, epi);      // fp32 C: bf16 operands whatever f16 says
  else if (f16) pp_launch<EPI_STORE_BF16, f16_t, true>(grid, s, A, B, bias, C, M, N, K, lda, ldb, ldc, epi);
  else pp_launch<EPI_STORE_BF16, bf16_t, true>(grid, s, A, B, bias, C, M, N, K, lda, ldb, ldc, epi);
  return 0;
}
