// Training windows cut on the device (prego_amd/train_cache.py: cfg['train_cache_device']): the training set's UNPADDED feature rows stay
// in HBM, and one launch writes a whole batch - rgb / flow / target / ant_target of n windows - as the loader's default_collate would have
// stacked it from datasets/dataset.py:96-132 (StepRecognitionDataset) or :138-231 (AnticipationDataset).  The W - 1 zero rows those
// datasets put in front of every video are synthesised here, one-hot target rows are built from a 4-byte class id.
// Pure streaming, as feature_cache.hip and rowwise.hip: 16 bytes per lane and trip, 256 lanes, grid-stride, no LDS.  Resident rows are read
// with non-temporal loads (a row is read again by later windows of the epoch, but far away in time); the outputs are written with ordinary
// stores, the forward reads them next.
#include "common.h"
#include "kernels.h"

// The resident frame (row of rgb_rows / flow_rows / labels / dense_targets) behind padded row s + p_off of window i of the batch, or -1 for
// a row of zeros: the front pad, a row past the video's end, a window or video index outside its table, a row outside the resident arrays.
// pad: the entry carries bit 31 of the video word (EpochWindowSampler's PAD entry: the features of the window, all-zero targets).
// Everything here is uniform across the workgroup when i and p_off are.
__device__ __forceinline__ long long gw_resident_row(const GatherWindows& a, unsigned i, unsigned p_off, bool& pad) {
  pad = false;
  const int idx = a.order[a.first + i];
  if ((unsigned)idx >= (unsigned)a.n_windows) return -1;
  const int vw = a.table[2 * (long long)idx], s = a.table[2 * (long long)idx + 1];
  pad = vw < 0;
  const int v = vw & 0x7fffffff;
  if (v >= a.n_videos) return -1;
  const long long q = (long long)s + p_off - (a.window - 1);       // frame of the unpadded video
  if (q < 0 || q >= a.vid_len[v]) return -1;
  const long long row = a.vid_row0[v] + q;
  return row >= 0 && row < a.n_rows ? row : -1;
}

// One element of a target row: `frame_row` counts rows over the batch ([n][rows_per] flattened), p_base is the padded offset of a
// window's first such row (0 for target, W for ant_target).
struct GwTargetRow { long long row; bool pad; int label; };
__device__ __forceinline__ GwTargetRow gw_target_row(const GatherWindows& a, unsigned frame_row, unsigned rows_per, unsigned p_base) {
  const unsigned i = frame_row / rows_per, r = frame_row - i * rows_per;
  GwTargetRow t;
  t.row = gw_resident_row(a, i, p_base + r, t.pad);
  if (t.pad) t.row = -1;
  t.label = (t.row >= 0 && a.labels) ? a.labels[t.row] : -1;
  return t;
}

// out [n][rows_per][C] flattened, 4 consecutive elements per lane; C is not a multiple of 4 in general, so a lane's four elements may sit
// in two rows (in more for C < 4) and the last lane may hold fewer than four.
__device__ __forceinline__ void gw_target_chunk(const GatherWindows& a, float* __restrict__ out, unsigned chunk, unsigned rows_per,
                                                unsigned p_base) {
  const unsigned C = a.n_classes, total = (unsigned)a.n * rows_per * C;
  const unsigned e0 = (chunk * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  unsigned fr = e0 / C, c = e0 - fr * C;
  GwTargetRow t = gw_target_row(a, fr, rows_per, p_base);
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0.f;
    if (e0 + k < total) {
      if (t.row >= 0) v[k] = a.labels ? ((int)c == t.label ? 1.f : 0.f) : a.dense_targets[t.row * C + c];
      if (++c == C && e0 + k + 1 < total) {
        c = 0;
        t = gw_target_row(a, ++fr, rows_per, p_base);
      }
    }
  }
  if (e0 + 4 <= total) *(float4*)(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
  else
    for (unsigned k = 0; e0 + k < total; ++k) out[e0 + k] = v[k];
}

// Units of work, walked at the grid's stride: one feature row of rgb_out, then of flow_out (a workgroup per row: the row arithmetic is
// scalar), then chunks of 1024 target elements, then of ant_target elements.
__global__ __launch_bounds__(256) void gather_windows_kernel(const GatherWindows a) {
  const unsigned W = a.window, rows = (unsigned)a.n * W;                      // host: n * W, n * W * C, n * L * C below 2^31
  const unsigned n_rgb = a.rgb_out ? rows : 0, n_flow = a.flow_out ? rows : 0;
  const unsigned t_chunks = a.target_out ? (rows * a.n_classes + 1023) / 1024 : 0;
  const unsigned a_chunks = a.ant_out ? ((unsigned)a.n * a.ant_len * a.n_classes + 1023) / 1024 : 0;
  const unsigned long long n_feat = (unsigned long long)n_rgb + n_flow, total = n_feat + t_chunks + a_chunks;
  for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
    if (u < n_feat) {
      const bool fl = u >= n_rgb;
      const unsigned row = (unsigned)(fl ? u - n_rgb : u);
      const unsigned i = row / W, r = row - i * W;
      bool pad;
      const long long src_row = gw_resident_row(a, i, r, pad);
      const int d = fl ? a.d_flow : a.d_rgb;
      const float* src = src_row < 0 ? nullptr : (fl ? a.flow_rows : a.rgb_rows) + src_row * d;
      float* dst = (fl ? a.flow_out : a.rgb_out) + (long long)row * d;
      for (int c = threadIdx.x * 4; c < d; c += 256 * 4)
        *(float4*)(dst + c) = src ? nt_load4(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (u < n_feat + t_chunks) {
      gw_target_chunk(a, a.target_out, (unsigned)(u - n_feat), W, 0);
    } else {
      gw_target_chunk(a, a.ant_out, (unsigned)(u - n_feat - t_chunks), (unsigned)a.ant_len, W);
    }
  }
}

// Arguments checked by prego_gather_windows (host_misc.cpp).  The grid follows the CUs: 8 workgroups per CU at the most.
void launch_gather_windows(const GatherWindows& a, int n_cu, hipStream_t s) {
  const unsigned long long rows = (unsigned long long)a.n * a.window;
  const unsigned long long want = (a.rgb_out ? rows : 0) + (a.flow_out ? rows : 0) + (a.target_out ? (rows * a.n_classes + 1023) / 1024 : 0) +
                                  (a.ant_out ? ((unsigned long long)a.n * a.ant_len * a.n_classes + 1023) / 1024 : 0);
  const unsigned long long cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * 8;
  if (want == 0) return;
  gather_windows_kernel<<<(int)(want < cap ? want : cap), 256, 0, s>>>(a);
}
