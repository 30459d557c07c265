// Backward of MiniROADA's anticipation head (model/rnn/rnn.py:113-130 in training mode, criterions/loss.py:40-79), for packed row r and
// step l < L, with A_l = relu(Z_l), Z_l = relu(h) W_a[l]^T + b_a[l], Y_l = A_l W_c^T + b_c and G_l = dLoss / dY_l:
//   dW_c += sum G_l^T A_l      db_c += sum G_l      dZ_l = (G_l W_c) * [A_l > 0]   (operand type)
//   dW_a[l] = sum_r dZ_l^T relu(h)      db_a[l] = sum_r dZ_l      d relu(h) += sum_l dZ_l W_a[l]
// OadAntLoss puts gradient on the LAST frame of each window only (B of R packed rows; time-major packing makes them the last B rows), so
// the gather below also marks the rows that hold any non-zero gradient and one workgroup turns the marks into a row span [lo, hi),
// rounded out to kSpanTile.  Every later launch of the head's backward reads the span from device memory and touches only those rows:
// the host never learns it, nothing is synchronised.  Rows outside the span have G = 0, so they contribute exact zeros.
// The products are register-tiled fp32-FMA GEMMs (64 x 64 tiles, 4 x 4 per thread, k in order: deterministic).  Under OadAntLoss they
// are small (span = 64 rows); a dense gradient (every frame) runs the same kernels over the whole range.
#include "common.h"
#include "kernels.h"

namespace {
constexpr int kSpanTile = 64;
constexpr int kTM = 64, kTN = 64, kTK = 16;

template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }
}  // namespace

// d_ant[clip] [T][L][C] -> G [R][L * C] packed time-major (the trunk's row order), and flags[r] = any non-zero value in row r
__global__ __launch_bounds__(256) void ant_gather_kernel(const float* const* __restrict__ d_ant, const int* __restrict__ rowoff,
                                                         const int* __restrict__ sorted_clip, int t_max, int nrows, int LC,
                                                         float* __restrict__ G, int* __restrict__ flags) {
  const int r = blockIdx.x;
  if (r >= nrows) return;
  const int t = plan_time_of_row(rowoff, t_max, r);
  const int clip = sorted_clip[r - rowoff[t]];
  const float* src = d_ant[clip] + (size_t)t * LC;
  int nz = 0;
  for (int i = threadIdx.x; i < LC; i += blockDim.x) {
    const float v = src[i];
    nz |= v != 0.f;
    G[(size_t)r * LC + i] = v;
  }
  nz = __syncthreads_or(nz);
  if (threadIdx.x == 0) flags[r] = nz;
}

// span[0..1] = [lo, hi): the smallest row range holding every flagged row, rounded out to kSpanTile; [0, 0) when none; [0, nrows) forced
__global__ __launch_bounds__(1024) void ant_span_kernel(const int* __restrict__ flags, int nrows, int force_full, int* __restrict__ span) {
  __shared__ int s_lo[1024], s_hi[1024];
  int lo = nrows, hi = 0;
  for (int r = threadIdx.x; r < nrows; r += 1024)
    if (flags[r]) { lo = min(lo, r); hi = max(hi, r + 1); }
  s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_lo[threadIdx.x] = min(s_lo[threadIdx.x], s_lo[threadIdx.x + o]);
      s_hi[threadIdx.x] = max(s_hi[threadIdx.x], s_hi[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    lo = s_lo[0]; hi = s_hi[0];
    if (force_full) { lo = 0; hi = nrows; }
    else if (hi <= lo) { lo = 0; hi = 0; }
    else { lo = lo / kSpanTile * kSpanTile; hi = min(nrows, (hi + kSpanTile - 1) / kSpanTile * kSpanTile); }
    span[0] = lo; span[1] = hi;
  }
}

// C[m][n] (EPI) = sum_k A[k sak + m sam] B[k sbk + n sbn], fp32 accumulation in k order.
// range: 0 = k in [0, K) and every m; 1 = k in [span0 mult, span1 mult); 2 = every k, only m in [span0 mult, span1 mult).
// Split-K (grid.z = S > 1): slice z takes k in [z kchunk, (z + 1) kchunk) of the range and writes its partial sum to
// part + z * M * N ([m][n], dense); ant_splitk_add_kernel adds the slices in z order.  EPI (S == 1): 0 store, 1 add, 2 operand type masked
// by mask[m][n] > 0 (dZ).
template <typename TA, typename TB, typename TC, int EPI>
__global__ __launch_bounds__(256) void ant_gemm_kernel(const TA* __restrict__ A, int sak, int sam, const TB* __restrict__ B, int sbk, int sbn,
                                                       TC* __restrict__ Cm, int ldc, const TC* __restrict__ mask, float* __restrict__ part,
                                                       int M, int N, int K, int kchunk, const int* __restrict__ span, int range, int mult) {
  __shared__ float sA[kTK][kTM + 4], sB[kTK][kTN + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN;
  int klo = 0, khi = K, mlo = 0, mhi = M;
  if (range == 1) { klo = span[0] * mult; khi = span[1] * mult; }
  if (range == 2) { mlo = span[0] * mult; mhi = span[1] * mult; }
  if (m0 >= mhi || m0 + kTM <= mlo) return;                  // whole workgroup
  if (gridDim.z > 1) { klo += blockIdx.z * kchunk; khi = min(khi, klo + kchunk); }
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = klo; k0 < khi; k0 += kTK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = tid + 256 * q;
      // contiguous direction first: along m when A is k-major (sam == 1), along k otherwise
      const int kk = sam == 1 ? i / kTM : i % kTK, mm = sam == 1 ? i % kTM : i / kTK;
      const int k = k0 + kk, m = m0 + mm;
      sA[kk][mm] = (k < khi && m < M) ? ldf<TA>(A + (size_t)k * sak + (size_t)m * sam) : 0.f;
      const int kb = sbn == 1 ? i / kTN : i % kTK, nb = sbn == 1 ? i % kTN : i / kTK;
      const int k2 = k0 + kb, n = n0 + nb;
      sB[kb][nb] = (k2 < khi && n < N) ? ldf<TB>(B + (size_t)k2 * sbk + (size_t)n * sbn) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kTK; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = sA[kk][ty + 16 * i]; b[i] = sB[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 16 * i;
    if (m >= M || m < mlo || m >= mhi) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx + 16 * j;
      if (n >= N) continue;
      if (gridDim.z > 1) { part[((size_t)blockIdx.z * M + m) * N + n] = acc[i][j]; continue; }
      TC* c = Cm + (size_t)m * ldc + n;
      if constexpr (EPI == 0) stf<TC>(c, acc[i][j]);
      else if constexpr (EPI == 1) stf<TC>(c, ldf<TC>(c) + acc[i][j]);
      else stf<TC>(c, ldf<TC>(mask + (size_t)m * ldc + n) > 0.f ? acc[i][j] : 0.f);
    }
  }
}

// C[m][n] += sum_z part[z][m][n] (z in order) for m in the row range of ant_gemm_kernel's `range` 2 (or every m)
__global__ __launch_bounds__(256) void ant_splitk_add_kernel(const float* __restrict__ part, int S, int M, int N, float* __restrict__ Cm, int ldc,
                                                             const int* __restrict__ span, int range, int mult) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  if (range == 2 && (m < span[0] * mult || m >= span[1] * mult)) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[((size_t)z * M + m) * N + n];
  Cm[(size_t)m * ldc + n] += s;
}

// out[n] (= or +=) sum_{k in [span0 mult, span1 mult)} A[k][n], k in order
template <typename T>
__global__ __launch_bounds__(256) void ant_colsum_kernel(const T* __restrict__ A, int lda, int N, const int* __restrict__ span, int mult,
                                                         int accumulate, float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int k1 = span[1] * mult;
  float s = 0.f;
  for (int k = span[0] * mult; k < k1; ++k) s += ldf<T>(A + (size_t)k * lda + n);
  out[n] = accumulate ? out[n] + s : s;
}

static dim3 ant_grid(int M, int N, int S) { return dim3((N + kTN - 1) / kTN, (M + kTM - 1) / kTM, S); }

void launch_ant_gather(const float* const* d_ant, const int* rowoff, const int* sorted_clip, int t_max, int nrows, int LC, float* G, int* flags,
                       int* span, int force_full, hipStream_t s) {
  if (nrows <= 0) return;
  ant_gather_kernel<<<nrows, 256, 0, s>>>(d_ant, rowoff, sorted_clip, t_max, nrows, LC, G, flags);
  ant_span_kernel<<<1, 1024, 0, s>>>(flags, nrows, force_full, span);
}

template <typename T>
static void ant_head_wgrad_t(const float* G, const T* HR, const T* Wc, int R, int H, int L, int C, const int* span, const T* Abuf, T* dZ,
                             float* g_fc_w, float* g_fc_b, float* g_w_a, float* g_b_a, hipStream_t s) {
  const int LH = L * H, RL = R * L;
  // dZ [(r, l)][H] = G_l [(r, l)][C] . W_c [C][H], masked by A_l > 0, operand type (rows of the span only)
  ant_gemm_kernel<float, T, T, 2><<<ant_grid(RL, H, 1), 256, 0, s>>>(G, 1, C, Wc, H, 1, dZ, H, Abuf, nullptr, RL, H, C, 0, span, 2, L);
  // dW_c [C][H] += G^T . A over the span's (r, l) pairs; db_c += column sums of G
  ant_gemm_kernel<float, T, float, 1><<<ant_grid(C, H, 1), 256, 0, s>>>(G, C, 1, Abuf, H, 1, g_fc_w, H, nullptr, nullptr, C, H, RL, 0, span, 1, L);
  ant_colsum_kernel<float><<<(C + 255) / 256, 256, 0, s>>>(G, C, C, span, L, 1, g_fc_b);
  // dW_a [L H][H] = dZ^T . relu(h) over the span's rows (written whole: zeros where the span is empty); db_a = column sums of dZ
  ant_gemm_kernel<T, T, float, 0><<<ant_grid(LH, H, 1), 256, 0, s>>>(dZ, LH, 1, HR, H, 1, g_w_a, H, nullptr, nullptr, LH, H, R, 0, span, 1, 1);
  ant_colsum_kernel<T><<<(LH + 255) / 256, 256, 0, s>>>(dZ, LH, LH, span, 1, 0, g_b_a);
}

template <typename T>
static void ant_head_dgrad_t(const T* Wa, int R, int H, int L, const int* span, const T* dZ, float* part, float* dHR, hipStream_t s) {
  const int LH = L * H;
  // d relu(h) [R][H] += dZ [R][L H] . W_a [L H][H] over the span's rows: split over the L steps (K = H each), slices added in l order
  if (L == 1) {
    ant_gemm_kernel<T, T, float, 1><<<ant_grid(R, H, 1), 256, 0, s>>>(dZ, 1, LH, Wa, H, 1, dHR, H, nullptr, nullptr, R, H, LH, 0, span, 2, 1);
  } else {
    ant_gemm_kernel<T, T, float, 0><<<ant_grid(R, H, L), 256, 0, s>>>(dZ, 1, LH, Wa, H, 1, nullptr, H, nullptr, part, R, H, LH, H, span, 2, 1);
    ant_splitk_add_kernel<<<(unsigned)(((long long)R * H + 255) / 256), 256, 0, s>>>(part, L, R, H, dHR, H, span, 2, 1);
  }
}

// the weight-gradient terms of the head after launch_ant_gather (span, G) and launch_ant_head_store_a (Abuf): dZ, dW_c / db_c (added),
// dW_a / db_a (written)
void launch_ant_head_wgrad(bool bf16, const float* G, const void* HR, const void* Wc, int R, int H, int L, int C, const int* span,
                           const void* Abuf, void* dZ, float* g_fc_w, float* g_fc_b, float* g_w_a, float* g_b_a, hipStream_t s) {
  if (bf16) ant_head_wgrad_t<bf16_t>(G, (const bf16_t*)HR, (const bf16_t*)Wc, R, H, L, C, span, (const bf16_t*)Abuf, (bf16_t*)dZ, g_fc_w, g_fc_b, g_w_a, g_b_a, s);
  else ant_head_wgrad_t<float>(G, (const float*)HR, (const float*)Wc, R, H, L, C, span, (const float*)Abuf, (float*)dZ, g_fc_w, g_fc_b, g_w_a, g_b_a, s);
}

// d relu(h) += sum_l dZ_l W_a[l] over the span's rows (part: [L][R][H] fp32 scratch, L > 1)
void launch_ant_head_dgrad(bool bf16, const void* Wa, int R, int H, int L, const int* span, const void* dZ, float* part, float* dHR, hipStream_t s) {
  if (bf16) ant_head_dgrad_t<bf16_t>((const bf16_t*)Wa, R, H, L, span, (const bf16_t*)dZ, part, dHR, s);
  else ant_head_dgrad_t<float>((const float*)Wa, R, H, L, span, (const float*)dZ, part, dHR, s);
}
