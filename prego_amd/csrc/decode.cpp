// prego_viterbi_decode, prego_viterbi_decode_costs, prego_emission_costs (include/prego_amd.h): the argument checks around decode.hip's
// launches.  Every refusal is decided before the launch; nothing is allocated and nothing waits.
#include "host_common.h"
#ifdef PREGO_DEBUG_ABI
#include "miniroad_handle.h"      // the allocation / wait counters of prego_debug_alloc_count cover these entries as well
#endif

static_assert(kDecodeCap == PREGO_DECODE_CAP && kDecodeMaxClasses == PREGO_DECODE_MAX_CLASSES && kDecodeBlock == PREGO_DECODE_BLOCK &&
              kDecodePrefetch == PREGO_DECODE_PREFETCH, "the header documents the kernel's constants");

// do the byte ranges [a, a + na) and [b, b + nb) share a byte (an empty range shares none)
static bool dec_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

extern "C" size_t prego_viterbi_workspace_bytes(int64_t n_frames, int n_videos, int n_classes) {
  if (n_frames <= 0 || n_frames >= (1ll << 31) || n_videos < 1 || n_classes < 1 || n_classes > kDecodeMaxClasses) return 0;
  return viterbi_workspace_bytes(n_frames, n_videos, n_classes);
}

static int decode_entry(const char* what, bool costs, const void* src, int64_t ld, const int32_t* offsets, int n_videos, int64_t n_frames,
                        int C, const int32_t* trans, const int32_t* init, int32_t* labels, int64_t* records, void* workspace,
                        size_t workspace_bytes, prego_stream_t stream) {
  if (!src || !offsets || !trans || !labels || !records || (!workspace && n_frames > 0)) return prego_fail_(PREGO_EINVAL, "%s: NULL argument", what);
  if (n_videos < 1 || n_frames < 0 || n_frames >= (1ll << 31))
    return prego_fail_(PREGO_EINVAL, "%s: n_videos %d (>= 1), n_frames %lld (0 .. 2^31 - 1)", what, n_videos, (long long)n_frames);
  if (C < 1 || C > kDecodeMaxClasses || ld < C)
    return prego_fail_(PREGO_EINVAL, "%s: n_classes %d (1 .. %d), ld %lld (>= n_classes)", what, C, kDecodeMaxClasses, (long long)ld);
  if ((uintptr_t)records % 16) return prego_fail_(PREGO_EINVAL, "%s: records must be 16-byte aligned", what);
  const size_t need = n_frames > 0 ? viterbi_workspace_bytes(n_frames, n_videos, C) : 0;
  // an output that shares a byte with an input (or with another output) cannot hold what the definitions say
  const struct { const void* p; size_t n; } in[4] = {{src, n_frames > 0 ? ((size_t)(n_frames - 1) * (size_t)ld + (size_t)C) * 4 : 0},
                                                     {offsets, ((size_t)n_videos + 1) * 4}, {trans, (size_t)C * C * 4}, {init, init ? (size_t)C * 4 : 0}};
  const struct { const void* p; size_t n; } out[3] = {{labels, (size_t)n_frames * 4}, {records, (size_t)n_videos * 16}, {workspace, workspace ? need : 0}};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 4; ++i)
      if (dec_overlap(out[o].p, out[o].n, in[i].p, in[i].n))
        return prego_fail_(PREGO_EINVAL, "%s: labels, records and workspace must not overlap an input", what);
    for (int q = o + 1; q < 3; ++q)
      if (dec_overlap(out[o].p, out[o].n, out[q].p, out[q].n))
        return prego_fail_(PREGO_EINVAL, "%s: labels, records and workspace must not overlap each other", what);
  }
  if (workspace_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "%s: workspace %zu < %zu (prego_viterbi_workspace_bytes)", what, workspace_bytes, need);
  // n_frames == 0: every offset clamps to 0, every video is empty, the kernel writes 0 | -1 and touches neither src nor the workspace
  if (launch_viterbi(costs, src, ld, (const int*)offsets, n_videos, n_frames, C, (const int*)trans, (const int*)init, (int*)labels,
                     (long long*)records, workspace, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", what);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_viterbi_decode(const float* probs, int64_t ld, const int32_t* offsets, int n_videos, int64_t n_frames, int n_classes,
                                    const int32_t* trans, const int32_t* init, int32_t* labels, int64_t* records, void* workspace,
                                    size_t workspace_bytes, prego_stream_t stream) {
  return decode_entry("viterbi_decode", false, probs, ld, offsets, n_videos, n_frames, n_classes, trans, init, labels, records, workspace,
                      workspace_bytes, stream);
}

extern "C" int prego_viterbi_decode_costs(const int32_t* costs, int64_t ld, const int32_t* offsets, int n_videos, int64_t n_frames, int n_classes,
                                          const int32_t* trans, const int32_t* init, int32_t* labels, int64_t* records, void* workspace,
                                          size_t workspace_bytes, prego_stream_t stream) {
  return decode_entry("viterbi_decode_costs", true, costs, ld, offsets, n_videos, n_frames, n_classes, trans, init, labels, records, workspace,
                      workspace_bytes, stream);
}

extern "C" int prego_emission_costs(const float* probs, int64_t ld, int64_t n_frames, int n_classes, int32_t* costs, prego_stream_t stream) {
  if (!probs || !costs) return prego_fail_(PREGO_EINVAL, "emission_costs: NULL argument");
  if (n_frames < 0 || n_frames >= (1ll << 31) || n_classes < 1 || ld < n_classes)
    return prego_fail_(PREGO_EINVAL, "emission_costs: n_frames %lld (0 .. 2^31 - 1), n_classes %d (>= 1), ld %lld (>= n_classes)",
                       (long long)n_frames, n_classes, (long long)ld);
  if (n_frames == 0) return PREGO_OK;
  if (dec_overlap(costs, (size_t)n_frames * n_classes * 4, probs, ((size_t)(n_frames - 1) * (size_t)ld + (size_t)n_classes) * 4))
    return prego_fail_(PREGO_EINVAL, "emission_costs: costs must not overlap probs");
  if (launch_emission_costs(probs, ld, n_frames, n_classes, (int*)costs, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "emission_costs: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
