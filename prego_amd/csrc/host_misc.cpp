// Handle-free entry points of the C ABI (include/prego_amd.h): post-processing, metrics and label preparation around the models.
#include "host_common.h"
#include "gru_tile.h"
#ifdef PREGO_DEBUG_ABI
#include "miniroad_handle.h"      // the allocation / wait counters of prego_debug_alloc_count cover this file's entries as well
#endif

#include <algorithm>
#include <thread>
#include <vector>

// ================================================================================================
// post-processing: utils/aggregate.py:55-72 (the 200-frame majority vote) on the device
// ================================================================================================
extern "C" int prego_window_vote(const int32_t* argmax, int64_t n_frames, int window, int n_classes, int32_t* votes,
                                 prego_stream_t stream) {
  if (!argmax || !votes) return prego_fail_(PREGO_EINVAL, "window_vote: NULL argument");
  if (launch_window_vote(argmax, n_frames, window, n_classes, votes, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "window_vote: n_frames %lld, window %d, n_classes %d (1..128)", (long long)n_frames, window, n_classes);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_format_ids(const int32_t* ids, int64_t n, uint32_t* text, int32_t* bad, prego_stream_t stream) {
  if (!ids || !text) return prego_fail_(PREGO_EINVAL, "format_ids: NULL argument");
  if (launch_format_ids(ids, n, text, bad, (hipStream_t)stream)) return prego_fail_(PREGO_EINVAL, "format_ids: n %lld", (long long)n);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// ================================================================================================
// Evaluate's feature cache: fp32 feature rows -> the handle's 16-bit operand type, once (feature_cache.hip)
// ================================================================================================
extern "C" int prego_cast_features(const float* src, void* dst, int64_t n, int dtype, prego_stream_t stream) {
  if (!src || !dst) return prego_fail_(PREGO_EINVAL, "cast_features: NULL argument");
  if (dtype != PREGO_BF16 && dtype != PREGO_F16) return prego_fail_(PREGO_EINVAL, "cast_features: dtype %d (PREGO_BF16 or PREGO_F16)", dtype);
  if (n < 0 || n % 8) return prego_fail_(PREGO_EINVAL, "cast_features: n %lld (>= 0, a multiple of 8)", (long long)n);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  if (s0 % 16 || d0 % 16) return prego_fail_(PREGO_EINVAL, "cast_features: src and dst must be 16-byte aligned");
  if (s0 < d0 + (uintptr_t)n * 2 && d0 < s0 + (uintptr_t)n * 4) return prego_fail_(PREGO_EINVAL, "cast_features: src and dst overlap");
  if (n == 0) return PREGO_OK;
  int dev = 0, n_cu = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  launch_cast_features(dtype == PREGO_F16, src, dst, n, n_cu, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// ================================================================================================
// the training set in device memory: one batch of windows per launch (train_cache.hip)
// ================================================================================================
extern "C" int prego_gather_windows(const float* rgb_rows, const float* flow_rows, int64_t n_rows, int d_rgb, int d_flow, const int32_t* labels,
                                    const float* dense_targets, const int64_t* vid_row0, const int32_t* vid_len, int n_videos,
                                    const int32_t* table, int n_windows, const int32_t* order, int64_t n_order, int64_t first, int n,
                                    int window_size, int n_classes, int ant_len, float* rgb_out, float* flow_out, float* target_out,
                                    float* ant_target_out, prego_stream_t stream) {
  if (n < 1) return prego_fail_(PREGO_EINVAL, "gather_windows: n %d (>= 1)", n);
  if (window_size < 1) return prego_fail_(PREGO_EINVAL, "gather_windows: window_size %d (>= 1)", window_size);
  if (ant_len < 0) return prego_fail_(PREGO_EINVAL, "gather_windows: ant_len %d (>= 0)", ant_len);
  if (ant_target_out && ant_len == 0) return prego_fail_(PREGO_EINVAL, "gather_windows: ant_target_out with ant_len 0");
  if ((labels != nullptr) == (dense_targets != nullptr))
    return prego_fail_(PREGO_EINVAL, "gather_windows: exactly one of labels and dense_targets");
  if (d_rgb < 0 || d_rgb % 4 || d_flow < 0 || d_flow % 4)
    return prego_fail_(PREGO_EINVAL, "gather_windows: d_rgb %d, d_flow %d (multiples of 4)", d_rgb, d_flow);
  if ((rgb_out && (!rgb_rows || d_rgb == 0)) || (flow_out && (!flow_rows || d_flow == 0)))
    return prego_fail_(PREGO_EINVAL, "gather_windows: an output without its resident rows");
  if (!vid_row0 || !vid_len || !table || !order || n_videos < 0 || n_windows < 0 || n_rows < 0)
    return prego_fail_(PREGO_EINVAL, "gather_windows: NULL table, or a negative count");
  if (n_classes < 1) return prego_fail_(PREGO_EINVAL, "gather_windows: n_classes %d (>= 1)", n_classes);
  if (first < 0 || n_order < 0 || first > n_order - n)
    return prego_fail_(PREGO_EINVAL, "gather_windows: entries [%lld, %lld + %d) of an order of %lld", (long long)first, (long long)first, n,
                       (long long)n_order);
  const int64_t lim = (int64_t)1 << 31, rows = (int64_t)n * window_size;
  if (rows >= lim || rows * n_classes >= lim || (int64_t)n * ant_len * n_classes >= lim)
    return prego_fail_(PREGO_EINVAL, "gather_windows: a batch of %d windows of %d rows, %d classes, ant_len %d has 2^31 elements or more", n,
                       window_size, n_classes, ant_len);
  if (((uintptr_t)rgb_rows | (uintptr_t)flow_rows | (uintptr_t)rgb_out | (uintptr_t)flow_out | (uintptr_t)target_out |
       (uintptr_t)ant_target_out) % 16)
    return prego_fail_(PREGO_EINVAL, "gather_windows: feature rows and outputs must be 16-byte aligned");
  if (((uintptr_t)labels | (uintptr_t)dense_targets | (uintptr_t)vid_len | (uintptr_t)table | (uintptr_t)order) % 4 || (uintptr_t)vid_row0 % 8)
    return prego_fail_(PREGO_EINVAL, "gather_windows: a table is not aligned to its element");
  if (!rgb_out && !flow_out && !target_out && !ant_target_out) return PREGO_OK;
  int dev = 0, n_cu = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  GatherWindows a;
  a.rgb_rows = rgb_rows; a.flow_rows = flow_rows; a.labels = (const int*)labels; a.dense_targets = dense_targets;
  a.vid_row0 = (const long long*)vid_row0; a.vid_len = (const int*)vid_len; a.table = (const int*)table; a.order = (const int*)order;
  a.n_rows = n_rows; a.first = first; a.n_videos = n_videos; a.n_windows = n_windows; a.n = n; a.window = window_size;
  a.n_classes = n_classes; a.ant_len = ant_len; a.d_rgb = d_rgb; a.d_flow = d_flow;
  a.rgb_out = rgb_out; a.flow_out = flow_out; a.target_out = target_out; a.ant_out = ant_target_out;
  launch_gather_windows(a, n_cu, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// ================================================================================================
// metrics on the device (metrics.hip): utils/metrics.py:25-62 (per-class average precision of the per-frame scores), :64-130 (the same
// metric by tenth of each action instance; ap / n_pos [10][n_classes]) and :10-22 (calibrated average precision, ties in frame order)
// ================================================================================================
static size_t metric_workspace(size_t (*need)(long long, int), int64_t n_frames, int n_classes) {
  return n_frames <= 0 || n_classes <= 0 ? 0 : need(n_frames, n_classes);
}
extern "C" size_t prego_perframe_ap_workspace_bytes(int64_t n, int c) { return metric_workspace(perframe_ap_workspace_bytes, n, c); }
extern "C" size_t prego_perstage_ap_workspace_bytes(int64_t n, int c) { return metric_workspace(perstage_ap_workspace_bytes, n, c); }
extern "C" size_t prego_perframe_cap_workspace_bytes(int64_t n, int c) { return metric_workspace(perframe_cap_workspace_bytes, n, c); }
extern "C" size_t prego_perstage_cap_workspace_bytes(int64_t n, int c) { return metric_workspace(perstage_cap_workspace_bytes, n, c); }

// What the six metric entries do around their launch.  name: in every message; have_args: the entry's own pointers are there;
// zero_ok: n_frames == 0 is accepted and needs no workspace - every entry but prego_perframe_ap(_labels), which refuses it, wants its
// workspace whatever n_frames is, and words the range and the workspace message shorter.
template <typename LAUNCH>
static int metric_entry(const char* name, bool zero_ok, bool have_args, int64_t n_frames, int n_classes, const void* workspace,
                        size_t workspace_bytes, size_t (*need)(long long, int), LAUNCH launch) {
  if (!have_args || (!workspace && (!zero_ok || n_frames > 0))) return prego_fail_(PREGO_EINVAL, "%s: NULL argument", name);
  if (n_frames < (zero_ok ? 0 : 1) || n_frames >= (1ll << 31) || n_classes < 1 || n_classes > 65535)
    return zero_ok ? prego_fail_(PREGO_EINVAL, "%s: n_frames %lld (0 .. 2^31 - 1), n_classes %d (1 .. 65535)", name, (long long)n_frames, n_classes)
                   : prego_fail_(PREGO_EINVAL, "%s: n_frames %lld, n_classes %d", name, (long long)n_frames, n_classes);
  if (n_frames > 0 && workspace_bytes < need(n_frames, n_classes))
    return zero_ok ? prego_fail_(PREGO_EWORKSPACE, "%s: workspace %zu < %zu (prego_%s_workspace_bytes)", name, workspace_bytes,
                                 need(n_frames, n_classes), name)
                   : prego_fail_(PREGO_EWORKSPACE, "%s: workspace %zu < %zu", name, workspace_bytes, need(n_frames, n_classes));
  if (launch()) return prego_fail_(PREGO_EINVAL, "%s: bad arguments", name);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

static int perframe_common(bool cal, const float* scores, const float* target, const int32_t* labels, int64_t n_frames, int n_classes,
                           double* ap, int64_t* n_pos, double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return metric_entry(cal ? "perframe_cap" : "perframe_ap", cal, scores && (target || labels) && ap, n_frames, n_classes, workspace,
                      workspace_bytes, cal ? perframe_cap_workspace_bytes : perframe_ap_workspace_bytes, [&] {
                        return (cal ? launch_perframe_cap : launch_perframe_ap)(scores, target, (const int*)labels, n_frames, n_classes, ap,
                                                                                 (long long*)n_pos, score_sum, workspace, (hipStream_t)stream);
                      });
}
extern "C" int prego_perframe_ap(const float* scores, const float* target, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                 double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perframe_common(false, scores, target, nullptr, n_frames, n_classes, ap, n_pos, score_sum, workspace, workspace_bytes, stream);
}
extern "C" int prego_perframe_ap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                        double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perframe_common(false, scores, nullptr, labels, n_frames, n_classes, ap, n_pos, score_sum, workspace, workspace_bytes, stream);
}
extern "C" int prego_perframe_cap(const float* scores, const float* target, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                  double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perframe_common(true, scores, target, nullptr, n_frames, n_classes, ap, n_pos, score_sum, workspace, workspace_bytes, stream);
}
extern "C" int prego_perframe_cap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                         double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perframe_common(true, scores, nullptr, labels, n_frames, n_classes, ap, n_pos, score_sum, workspace, workspace_bytes, stream);
}

static int perstage_common(bool cal, const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                           void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return metric_entry(cal ? "perstage_cap" : "perstage_ap", true, scores && labels && ap, n_frames, n_classes, workspace, workspace_bytes,
                      cal ? perstage_cap_workspace_bytes : perstage_ap_workspace_bytes, [&] {
                        return (cal ? launch_perstage_cap : launch_perstage_ap)(scores, (const int*)labels, n_frames, n_classes, ap,
                                                                                 (long long*)n_pos, workspace, (hipStream_t)stream);
                      });
}
extern "C" int prego_perstage_ap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                        void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perstage_common(false, scores, labels, n_frames, n_classes, ap, n_pos, workspace, workspace_bytes, stream);
}
extern "C" int prego_perstage_cap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                                         void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  return perstage_common(true, scores, labels, n_frames, n_classes, ap, n_pos, workspace, workspace_bytes, stream);
}

// ================================================================================================
// utils/postprocessing.py:4-29 (THUMOS: 5-frame max, CliffDiving -> Diving, ambiguous frames removed) on the device (thumos_post.hip)
// ================================================================================================
extern "C" size_t prego_thumos_postprocess_workspace_bytes(int64_t n_frames, int n_classes) {
  if (n_frames <= 0 || n_frames >= (1ll << 31) || n_classes <= 0) return 0;
  return thumos_postprocess_workspace_bytes(n_frames, n_classes);
}
static_assert(kThumosTileRows == PREGO_THUMOS_TILE_ROWS, "the header documents the scatter tile");
static bool thumos_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
static int thumos_common(const float* scores, int64_t ld_scores, const float* target, int64_t ld_target, const int32_t* labels, int64_t n_frames,
                         int n_classes, int flags, int switch_from, int switch_to, int ambiguous, float* scores_out, float* target_out,
                         int32_t* labels_out, int64_t* n_valid, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  const bool ids = target == nullptr && target_out == nullptr && (labels || labels_out);
  if (!scores || !scores_out || !n_valid || (ids ? (!labels || !labels_out) : (!target || !target_out)) || (!workspace && n_frames > 0))
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: NULL argument");
  if (n_frames < 0 || n_frames >= (1ll << 31) || n_classes < 1 || n_classes > 65535)
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: n_frames %lld (0 .. 2^31 - 1), n_classes %d (1 .. 65535)", (long long)n_frames, n_classes);
  if (flags & ~(PREGO_THUMOS_SMOOTH | PREGO_THUMOS_SWITCH)) return prego_fail_(PREGO_EINVAL, "thumos_postprocess: flags 0x%x", flags);
  if (ld_scores < n_classes || (!ids && ld_target < n_classes))
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: ld_scores %lld, ld_target %lld below n_classes %d", (long long)ld_scores,
                       (long long)ld_target, n_classes);
  if (ambiguous < -1 || ambiguous >= n_classes)
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: ambiguous %d (-1 .. %d)", ambiguous, n_classes - 1);
  const bool sw = flags & PREGO_THUMOS_SWITCH;
  if (sw && (switch_from < 0 || switch_from >= n_classes || switch_to < 0 || switch_to >= n_classes || switch_from == switch_to))
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: switch columns %d -> %d (two different columns of [0, %d))", switch_from, switch_to,
                       n_classes);
  if (((uintptr_t)scores | (uintptr_t)scores_out | (uintptr_t)target | (uintptr_t)target_out | (uintptr_t)labels | (uintptr_t)labels_out) % 4 ||
      (uintptr_t)n_valid % 8)
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: a pointer is not aligned to its element");
  const size_t n = (size_t)n_frames, C = (size_t)n_classes;
  const size_t in_s = n ? ((n - 1) * (size_t)ld_scores + C) * 4 : 0;
  const size_t in_t = n ? (ids ? n * 4 : ((n - 1) * (size_t)ld_target + C) * 4) : 0;
  const void* in_tp = ids ? (const void*)labels : (const void*)target;
  const size_t need = n ? thumos_postprocess_workspace_bytes(n_frames, n_classes) : 0;
  const void* outs[4] = {scores_out, ids ? (void*)labels_out : (void*)target_out, n_valid, workspace};
  const size_t out_b[4] = {n * C * 4, ids ? n * 4 : n * C * 4, 8, need};
  for (int k = 0; k < 4; ++k)
    if (thumos_overlap(outs[k], out_b[k], scores, in_s) || thumos_overlap(outs[k], out_b[k], in_tp, in_t))
      return prego_fail_(PREGO_EINVAL, "thumos_postprocess: an output or the workspace overlaps an input");
  if (workspace_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "thumos_postprocess: workspace %zu < %zu (prego_thumos_postprocess_workspace_bytes)", workspace_bytes, need);
  if (n_frames == 0) {
    HIPCHK(hipMemsetAsync(n_valid, 0, 8, (hipStream_t)stream));
    return PREGO_OK;
  }
  if (launch_thumos_postprocess(scores, ld_scores, target, ld_target, (const int*)labels, n_frames, n_classes, flags & PREGO_THUMOS_SMOOTH,
                                sw ? switch_from : -1, sw ? switch_to : -1, ambiguous, scores_out, target_out, (int*)labels_out,
                                (long long*)n_valid, workspace, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "thumos_postprocess: bad arguments");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
extern "C" int prego_thumos_postprocess(const float* scores, int64_t ld_scores, const float* target, int64_t ld_target, int64_t n_frames,
                                        int n_classes, int flags, int switch_from, int switch_to, int ambiguous, float* scores_out,
                                        float* target_out, int64_t* n_valid, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!target || !target_out) return prego_fail_(PREGO_EINVAL, "thumos_postprocess: NULL argument");
  return thumos_common(scores, ld_scores, target, ld_target, nullptr, n_frames, n_classes, flags, switch_from, switch_to, ambiguous, scores_out,
                       target_out, nullptr, n_valid, workspace, workspace_bytes, stream);
}
extern "C" int prego_thumos_postprocess_labels(const float* scores, int64_t ld_scores, const int32_t* labels, int64_t n_frames, int n_classes,
                                               int flags, int switch_from, int switch_to, int ambiguous, float* scores_out, int32_t* labels_out,
                                               int64_t* n_valid, void* workspace, size_t workspace_bytes, prego_stream_t stream) {
  if (!labels || !labels_out) return prego_fail_(PREGO_EINVAL, "thumos_postprocess_labels: NULL argument");
  return thumos_common(scores, ld_scores, nullptr, 0, labels, n_frames, n_classes, flags, switch_from, switch_to, ambiguous, scores_out, nullptr,
                       labels_out, n_valid, workspace, workspace_bytes, stream);
}

// The feeder's side of the class-id entries: one-hot target rows (what the reference's dataset yields, dataset.py / eval.py:55 np.argmax(target)) reduced
// to their class id on the host, in the loader's own memory, by a few threads - while the GPU is busy with the features.  HOST function.
extern "C" int prego_onehot_labels(int n_videos, const float* const* targets, const int64_t* n_frames, int n_classes, int32_t* labels,
                                   int32_t* onehot) {
  if (n_videos < 0 || (n_videos && (!targets || !n_frames || !labels || !onehot)) || n_classes <= 0)
    return prego_fail_(PREGO_EINVAL, "onehot_labels: bad argument");
  std::vector<int64_t> off((size_t)n_videos + 1, 0);
  for (int v = 0; v < n_videos; ++v) {
    if (n_frames[v] < 0 || (n_frames[v] && !targets[v])) return prego_fail_(PREGO_EINVAL, "onehot_labels: video %d", v);
    off[(size_t)v + 1] = off[(size_t)v] + n_frames[v];
    onehot[v] = 1;
  }
  const int64_t total = off[(size_t)n_videos];
  const unsigned hw = std::thread::hardware_concurrency();
  const int nt = (int)std::min<int64_t>(std::max<int64_t>(1, total / 16384), std::min(16u, hw ? hw : 1u));
  auto work = [&](int t) {
    const int64_t a = total * t / nt, b = total * (t + 1) / nt;
    int v = (int)(std::upper_bound(off.begin(), off.end(), a) - off.begin()) - 1;
    for (int64_t i = a; i < b; ++i) {
      while (i >= off[(size_t)v + 1]) ++v;
      const float* row = targets[v] + (size_t)(i - off[(size_t)v]) * n_classes;
      int nz = 0, pos = 0;
      for (int c = 0; c < n_classes; ++c) { nz += row[c] != 0.f; pos += row[c] > 0.f; }
      int best = 0;                                            // np.argmax: the first maximum
      if (nz == 1 && pos == 1) { while (!(row[best] > 0.f)) ++best; }
      else {
        __atomic_store_n(&onehot[v], 0, __ATOMIC_RELAXED);
        for (int c = 1; c < n_classes; ++c) if (row[c] > row[best]) best = c;
      }
      labels[i] = best;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
  if (total > 0) work(0);
  for (auto& x : th) x.join();
  return PREGO_OK;
}
#ifdef PREGO_DEBUG_ABI
// probe: the ping-pong GEMM as a persistent worker that only runs on XCDs >= xcd_lo and claims tiles from `counter`
// (device word, zeroed by the caller in stream order); grid = workgroups launched (256 = one per CU)
extern "C" int prego_debug_gemm_worker(const void* A, const void* B, const float* bias, float* C, int M, int N, int K, int xcd_lo,
                                       unsigned* counter, int grid, prego_stream_t stream) {
  if (!A || !B || !bias || !C || !counter || M <= 0 || grid <= 0) return prego_fail_(PREGO_EINVAL, "debug gemm worker: bad arguments");
  if (launch_gemm_bf16_pingpong_worker(A, K, B, K, bias, C, N, M, N, K, xcd_lo, counter, grid, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "debug gemm worker: unsupported shape");
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// debug / microbenchmark: C[M,N] (fp32) = A[M,K] . B[N,K]^T + bias with a chosen bf16 kernel variant
// (0 = 128x128 two-stage, 1 = 256x128 three-stage counted-vmcnt, 9 = 256x256 two-stage, 12 = ping-pong, 30 = the eight-wave split-K
// workgroup), scripts/gemm_bench.py.  A variant forces its kernel; on a shape that kernel does not take nothing is launched and the
// call still returns 0 (tests/test_gpu_gemm.py sees it by its canary)
extern "C" int prego_debug_gemm_bf16(int variant, const void* A, const void* B, const float* bias, float* C, int M, int N, int K,
                                     prego_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N % 128 || K % 64) return prego_fail_(PREGO_EINVAL, "debug gemm: bad arguments");
  GemmNtKernel kind;
  switch (variant) {
    case 0: kind = GEMM_NT_128; break;
    case 1: kind = GEMM_NT_256X128; break;
    case 9: kind = GEMM_NT_256SQ; break;
    case 12: kind = GEMM_NT_PINGPONG; break;
    case 30: kind = GEMM_NT_SPLITK; break;
    default: return prego_fail_(PREGO_EINVAL, "debug gemm: unknown variant %d", variant);
  }
  GemmEpi epi{};
  epi.mode = EPI_STORE;
  if (!(variant == 12 && !bias))     // odd: this hook's ping-pong variant has never taken a NULL bias
    (void)launch_gemm_nt_kernel(kind, A, K, B, K, bias, C, N, M, N, K, epi, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// unit test (tests/test_gemm_dispatch_cpu.py): gemm_nt_choose's answer (GemmNtKernel as an int) - no device is touched.  entry: GemmNtEntry;
// knobs: bit 0 PREGO_GEMM_NO_BIG, bit 1 _NO_SPLITK, bit 2 _NO_PINGPONG, as arguments here because the environment is read once per process
extern "C" int prego_debug_gemm_nt_choice(int entry, int M, int N, int K, int lda, int ldb, int has_bias, int f16, int train_splitk, int mode,
                                          int dh, int emb, int knobs) {
  const GemmNtQuery q = {entry, M, N, K, lda, ldb, has_bias != 0, f16 != 0, train_splitk != 0, mode, dh, emb};
  return (int)gemm_nt_choose(q, GemmNtKnobs{(knobs & 1) != 0, (knobs & 2) != 0, (knobs & 4) != 0});
}

// unit test (tests/test_gru_choice_cpu.py): gru_choose's answer packed (GruChoice::packed) - no device is touched
extern "C" int prego_debug_gru_choice(int entry, int operand, int hid, int nct, int G, int gi_bf16, int train, int no_mt, int stamps, int rows,
                                      int mt_spec, int Gd, int ready, int* grid, int* lds) {
  const GruChoice c = gru_choose(GruQuery{entry, operand != GRU_OP_F32, operand == GRU_OP_F16, hid, nct, G, gi_bf16 != 0, train != 0, no_mt != 0,
                                          stamps != 0, rows, mt_spec, Gd, ready != 0});
  if (grid) *grid = c.ok ? c.grid : 0;
  if (lds) *lds = c.ok ? (int)c.lds : 0;
  return c.ok && !gru_choice_has_kernel(c) ? -2 : c.packed();
}
// unit test: the exchange layout functions and the sizes the host derives from them (gru_tile.h)
extern "C" long long prego_debug_gru_hx_offset(int what, int wb, int tiles, int a, int b, int c) {
  switch (what) {
    case 0: return gru_hx_offset(wb, tiles, a, b, c);
    case 1: return gru_hx_k_at(wb, a, b, c);
    case 2: return gru_hx_col_at(b);
    case 3: return gru_plane_bytes(wb, a, tiles);
    case 10: return (long long)gru_hx_bytes(wb == 2, a, b);
    case 11: return (long long)gru_x2_hx_bytes(a, b);
    case 12: return gru_group_size(wb == 2, a);
    case 13: return gru_hidden_supported(wb == 2, a) ? 1 : 0;
    case 14: return gru_max_slots(b, c != 0);
    default: return -1;
  }
}

// unit test (tests/test_gpu_gemm_tn.py): launch_gemm_bf16_tn as the training steps call it - the launcher's own choice of kernel runs
extern "C" int prego_debug_gemm_tn(int ta, int tb, const void* A, int lda, const void* B, int ldb, const float* bias, float* C, void* C16,
                                   int ldc, int M, int N, int K, int k_valid, float* colsum_out, prego_stream_t stream) {
  if (!A || !B || (!C && !C16)) return prego_fail_(PREGO_EINVAL, "debug gemm tn: NULL argument");
  if (launch_gemm_bf16_tn(ta != 0, tb != 0, A, lda, B, ldb, bias, C, ldc, M, N, K, k_valid, colsum_out, (hipStream_t)stream, C16))
    return prego_fail_(PREGO_EINVAL, "debug gemm tn: unsupported shape (ta %d, tb %d, M %d, N %d, K %d, k_valid %d, lda %d, ldb %d)", ta, tb, M,
                       N, K, k_valid, lda, ldb);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

// unit test (tests/test_gpu_gemm.py): the production dispatcher of the NT projections, with the argument checks its callers guarantee
extern "C" int prego_debug_gemm_nt(int f16, int train_splitk, const void* A, int lda, const void* B, int ldb, const float* bias, float* C,
                                   int ldc, int M, int N, int K, prego_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || N % 128 || K <= 0 || K % 64 || lda < K || ldb < K || ldc < N)
    return prego_fail_(PREGO_EINVAL, "debug gemm nt: bad arguments (M %d, N %d, K %d, lda %d, ldb %d, ldc %d)", M, N, K, lda, ldb, ldc);
  launch_gemm_bf16_nt(A, lda, B, ldb, bias, C, ldc, M, N, K, (hipStream_t)stream, f16 != 0, train_splitk != 0);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
#endif  // PREGO_DEBUG_ABI
