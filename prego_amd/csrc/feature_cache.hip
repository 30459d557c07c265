// Feature cache of Evaluate (prego_amd/evaluate.py: cfg['eval_cache_device']): fp32 feature rows -> the 16-bit MFMA operand type, once,
// so that an eval set stays in HBM between Evaluate calls in the form the next forward reads (PREGO_FWD_IN16: half the bytes, and
// pack_rows_kernel copies instead of converting).  The conversion is op16<OT>::pack2_sat - what pack_rows_kernel and ffp_pack_rows apply to
// an fp32 row -, so a forward on the cast rows multiplies bit for bit the operands of the forward on the fp32 rows.
// Pure streaming, as rowwise.hip: per lane two 16-byte non-temporal loads and ONE 16-byte store, grid-stride, no LDS.
#include "common.h"
#include "kernels.h"

// n8 = groups of 8 elements.  64-bit indexing: a whole eval set is ~10^10 elements.
template <typename OT>
__global__ __launch_bounds__(256) void cast_features_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long long n8) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n8; g += stride) {
    const float4 a = nt_load4(src + g * 8);
    const float4 b = nt_load4(src + g * 8 + 4);
    uint4 o;
    o.x = op16<OT>::pack2_sat(a.x, a.y); o.y = op16<OT>::pack2_sat(a.z, a.w);
    o.z = op16<OT>::pack2_sat(b.x, b.y); o.w = op16<OT>::pack2_sat(b.z, b.w);
    *(uint4*)(dst + g * 8) = o;
  }
}

// n % 8 == 0, n > 0 (host_misc.cpp checks).  The grid follows the CUs, not n: 8 workgroups per CU, each walking the rows at the grid's stride.
void launch_cast_features(bool f16, const float* src, void* dst, long long n, int n_cu, hipStream_t s) {
  const long long n8 = n / 8, want = (n8 + 255) / 256, cap = (long long)(n_cu > 0 ? n_cu : 256) * 8;
  const int grid = (int)(want < cap ? want : cap);
  if (f16) cast_features_kernel<f16_t><<<grid, 256, 0, s>>>(src, (bf16_t*)dst, n8);
  else cast_features_kernel<bf16_t><<<grid, 256, 0, s>>>(src, (bf16_t*)dst, n8);
}
