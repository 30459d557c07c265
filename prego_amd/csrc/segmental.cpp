// prego_segmental_scores (include/prego_amd.h): the argument checks around segmental.hip's one launch.  Every refusal is decided
// before the launch; nothing is allocated and nothing waits.
#include "host_common.h"
#ifdef PREGO_DEBUG_ABI
#include "miniroad_handle.h"      // the allocation / wait counters of prego_debug_alloc_count cover this entry as well
#endif

static_assert(kSegmentalLdsSegments == PREGO_SEGMENTAL_LDS_SEGMENTS, "the header documents where the diagonals leave LDS");

extern "C" size_t prego_segmental_workspace_bytes(int64_t n_frames, int n_videos) {
  if (n_frames <= 0 || n_frames >= (1ll << 31) || n_videos < 1) return 0;
  return segmental_workspace_bytes(n_frames, n_videos);
}

extern "C" int prego_segmental_scores(const int32_t* pred, const int32_t* gt, const int32_t* offsets, int n_videos, int64_t n_frames,
                                      const uint32_t bg_mask[4], const int32_t overlap_num[3], const int32_t overlap_den[3], int32_t* records,
                                      void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!pred || !gt || !offsets || !records || (!workspace && n_frames > 0)) return prego_fail_(PREGO_EINVAL, "segmental_scores: NULL argument");
  if (n_videos < 1 || n_frames < 0 || n_frames >= (1ll << 31))
    return prego_fail_(PREGO_EINVAL, "segmental_scores: n_videos %d (>= 1), n_frames %lld (0 .. 2^31 - 1)", n_videos, (long long)n_frames);
  if ((uintptr_t)records % 16) return prego_fail_(PREGO_EINVAL, "segmental_scores: records must be 16-byte aligned");
  if ((overlap_num == nullptr) != (overlap_den == nullptr))
    return prego_fail_(PREGO_EINVAL, "segmental_scores: overlap_num and overlap_den go together (both NULL: 1/10, 1/4, 1/2)");
  static const int32_t def_num[3] = {1, 1, 1}, def_den[3] = {10, 4, 2};
  const int32_t* num = overlap_num ? overlap_num : def_num;
  const int32_t* den = overlap_den ? overlap_den : def_den;
  for (int k = 0; k < 3; ++k)
    if (!(0 < num[k] && num[k] <= den[k] && den[k] <= 32768))
      return prego_fail_(PREGO_EINVAL, "segmental_scores: overlap %d is %d/%d (0 < num <= den <= 32768)", k, num[k], den[k]);
  const size_t need = n_frames > 0 ? segmental_workspace_bytes(n_frames, n_videos) : 0;
  if (workspace_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "segmental_scores: workspace %zu < %zu (prego_segmental_workspace_bytes)", workspace_bytes, need);
  if (n_frames == 0) {                                    // every video is empty: 0 0 0 0 0 0 0 0
    HIPCHK(hipMemsetAsync(records, 0, (size_t)n_videos * 32, (hipStream_t)stream));
    return PREGO_OK;
  }
  static const uint32_t no_bg[4] = {0u, 0u, 0u, 0u};
  if (launch_segmental((const int*)pred, (const int*)gt, (const int*)offsets, n_videos, n_frames, bg_mask ? bg_mask : no_bg, num, den,
                       (int*)records, workspace, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "segmental_scores: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
