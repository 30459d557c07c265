// Segmental metrics on the device (include/prego_amd.h, prego_segmental_scores): frame accuracy, segmental edit distance and segmental
// F1 at three overlaps of V videos, from one predicted and one true class id per frame.  ONE launch, one workgroup per video (the grid
// strides over the videos when there are more of them than workgroups); no workgroup waits for another, integers only.
//
// A workgroup, for its video [a, b) (both words of `offsets` clamped into [0, n_frames], a descending pair = an empty video):
//   1. streams the frames in chunks of SEG_CHUNK (four consecutive frames per thread, one 16-byte load per array where the chunk grid
//      - aligned to four frames of the whole axis - and the arrays' alignment allow it), counts pred == gt, and flags the HEADS
//      (first frame of a maximal run of equal ids inside the video) and TAILS (last frame) of both sequences; runs of a masked id are
//      dropped here.  One wg_scan_step per chunk ranks the kept heads of both sequences (two counts in the halves of one 64-bit sum,
//      carried from chunk to chunk): a head writes (label, start) of its segment, a tail its end - the kept tails are as many as the
//      kept heads and in the same order - into the video's slice of the workspace (segment j of the video at a + j: a video has at
//      most b - a segments).
//   2. F1: a thread per pred segment bisects the true segments (sorted, disjoint) for the first that ends behind its start and walks
//      while they start before its end; among those of its label it keeps the largest inter / union (64-bit cross products, the
//      earliest on a tie) and ORs one bit per overlap it reaches into that true segment's flag word.  tp_k = the flag words with bit k.
//   3. Levenshtein distance of the two label lists by anti-diagonals: cell (i, j) of diagonal d = i + j needs (i - 1, j), (i, j - 1)
//      of d - 1 and (i - 1, j - 1) of d - 2, so three diagonals of min(m, n) + 1 cells rotate, every cell of one in parallel, one
//      barrier per diagonal.  They live in LDS up to PREGO_SEGMENTAL_LDS_SEGMENTS on the short side and in the workspace above it
//      (adversarial input only: slow, every diagonal is a round trip through the cache hierarchy).
//   4. lane 0 writes the record correct | frames | m | n | dist | tp_0 | tp_1 | tp_2 as two 16-byte stores.
#include "common.h"
#include "kernels.h"
#include "wg_scan.h"

#define SEG_CHUNK 1024        // frames per scan step: 256 threads x 4 (kSegmentalChunk in kernels.h)
#define SEG_GRID 1024         // workgroups of a launch at most: four per CU; more videos than that are strided over
static_assert(SEG_CHUNK == kSegmentalChunk, "the tests place video boundaries around the chunk size");

struct SegArgs {
  const int *pred, *gt, *offsets;
  int n_videos;
  long long n_frames;
  unsigned bg[4];
  int num[3], den[3];
  int* records;
  // workspace, each [n_frames] unless noted: the segments of both sequences, the true segments' flag words, the diagonals [3 (n_frames + n_videos)]
  int *p_lab, *p_st, *p_en, *g_lab, *g_st, *g_en;
  unsigned* g_hit;
  int* diag;
  int vec;                    // pred and gt are 16-byte aligned
};

size_t segmental_workspace_bytes(long long n, int V) { return ((size_t)10 * (size_t)n + (size_t)3 * (size_t)V) * 4; }

__device__ __forceinline__ bool seg_masked(const unsigned (&bg)[4], int lab) {      // selects, not an indexed read of the kernel arguments
  const unsigned w = (unsigned)lab >> 5;
  const unsigned word = w == 0u ? bg[0] : w == 1u ? bg[1] : w == 2u ? bg[2] : w == 3u ? bg[3] : 0u;
  return (word >> ((unsigned)lab & 31u)) & 1u;
}

// the labels around a thread's four frames i0 .. i0 + 3 of the video [a, b): lab[e + 1] = frame i0 + e; lab[0] / lab[5] = the frames in
// front and behind.  i0 is a multiple of 4.  Only the entries of frames inside the video mean anything (the 16-byte load brings
// whatever lies beside them, the scalar path 0): the caller reads no other.
__device__ __forceinline__ void seg_load(const int* __restrict__ x, long long a, long long b, long long n_frames, long long i0, bool vec,
                                         int lane, int (&lab)[6]) {
  if (vec && i0 >= 0 && i0 + 4 <= n_frames && i0 + 3 >= a && i0 < b) {
    const int4 q = *(const int4*)(x + i0);
    lab[1] = q.x; lab[2] = q.y; lab[3] = q.z; lab[4] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const long long i = i0 + e; lab[e + 1] = (i >= a && i < b) ? x[i] : 0; }
  }
  const int up = __shfl_up(lab[4], 1, 64), down = __shfl_down(lab[1], 1, 64);
  lab[0] = up;
  lab[5] = down;
  if (lane == 0) lab[0] = (i0 - 1 >= a && i0 - 1 < b) ? x[i0 - 1] : 0;
  if (lane == 63) lab[5] = (i0 + 4 >= a && i0 + 4 < b) ? x[i0 + 4] : 0;
}

// Levenshtein distance of s[0 .. ns) and l[0 .. nl), ns <= nl; d3: three diagonals of `stride` >= ns + 1 ints (LDS or global).
// Every thread of the workgroup calls it; the result is valid in every thread.
__device__ __forceinline__ int seg_edit_distance(const int* s, int ns, const int* l, int nl, int* d3, int stride) {
  const int tid = threadIdx.x;
  int cur = 0, prev = stride, prev2 = 2 * stride;
  for (int d = 0; d <= ns + nl; ++d) {
    const int lo = d > nl ? d - nl : 0, hi = d < ns ? d : ns;
    for (int i = lo + tid; i <= hi; i += 256) {
      const int j = d - i;
      int v;
      if (i == 0 || j == 0) {
        v = d;
      } else {
        const int del = d3[prev + i - 1] + 1, ins = d3[prev + i] + 1, sub = d3[prev2 + i - 1] + (s[i - 1] != l[j - 1] ? 1 : 0);
        v = min(min(del, ins), sub);
      }
      d3[cur + i] = v;
    }
    __syncthreads();                                        // diagonal d is written; nobody still reads d - 2, which d + 1 overwrites
    const int t = prev2; prev2 = prev; prev = cur; cur = t;
  }
  return d3[prev + ns];                                     // after the last rotation `prev` is the diagonal ns + nl: its one cell
}

__global__ __launch_bounds__(256) void segmental_kernel(const SegArgs A) {
  __shared__ int lds_diag[3 * (kSegmentalLdsSegments + 1)];
  __shared__ long long wsum[2][4];
  __shared__ int red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nf = A.n_frames;
  for (int v = blockIdx.x; v < A.n_videos; v += gridDim.x) {
    long long a = (long long)A.offsets[v], b = (long long)A.offsets[v + 1];
    a = a < 0 ? 0 : (a > nf ? nf : a);
    b = b < 0 ? 0 : (b > nf ? nf : b);
    if (b < a) b = a;
    int *p_lab = A.p_lab + a, *p_st = A.p_st + a, *p_en = A.p_en + a, *g_lab = A.g_lab + a, *g_st = A.g_st + a, *g_en = A.g_en + a;
    unsigned* g_hit = A.g_hit + a;
    // ---- 1. frames: correct, heads and tails, compaction ----
    int correct = 0;
    long long carry = 0;                                    // kept heads so far: pred in the low half, gt in the high half
    int parity = 0;
    for (long long base = a & ~3ll; base < b; base += SEG_CHUNK, parity ^= 1) {
      const long long i0 = base + (long long)tid * 4;
      int lp[6], lg[6];
      seg_load(A.pred, a, b, nf, i0, A.vec != 0, lane, lp);
      seg_load(A.gt, a, b, nf, i0, A.vec != 0, lane, lg);
      bool hp[4], hg[4], tp[4], tg[4];
      long long mine = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long i = i0 + e;
        const bool in = i >= a && i < b;
        const bool kp = in && !seg_masked(A.bg, lp[e + 1]), kg = in && !seg_masked(A.bg, lg[e + 1]);
        hp[e] = kp && (i == a || lp[e + 1] != lp[e]);
        tp[e] = kp && (i == b - 1 || lp[e + 1] != lp[e + 2]);
        hg[e] = kg && (i == a || lg[e + 1] != lg[e]);
        tg[e] = kg && (i == b - 1 || lg[e + 1] != lg[e + 2]);
        if (in && lp[e + 1] == lg[e + 1]) ++correct;
        mine += (hp[e] ? 1ll : 0ll) + (hg[e] ? 1ll << 32 : 0ll);
      }
      long long run = wg_scan_step<ScanSum>(mine, carry, wsum, parity);      // the kept heads in front of my first frame
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int np = (int)(run & 0xFFFFFFFFll), ng = (int)(run >> 32);
        if (hp[e]) { p_lab[np] = lp[e + 1]; p_st[np] = (int)(i0 + e); ++np; }
        if (hg[e]) { g_lab[ng] = lg[e + 1]; g_st[ng] = (int)(i0 + e); g_hit[ng] = 0u; ++ng; }
        if (tp[e]) p_en[np - 1] = (int)(i0 + e + 1);        // a kept tail closes the segment of the last kept head at or before it
        if (tg[e]) g_en[ng - 1] = (int)(i0 + e + 1);
        run = (long long)np | ((long long)ng << 32);
      }
    }
    const int m = (int)(carry & 0xFFFFFFFFll), n = (int)(carry >> 32);
    __syncthreads();                                        // the segment lists are the workgroup's
    // ---- 2. F1: the best true segment of every pred segment ----
    for (int p = tid; p < m; p += 256) {
      const int lab = p_lab[p], ps = p_st[p], pe = p_en[p];
      int lo = 0, cnt = n;                                  // the first true segment that ends behind ps
      while (cnt > 0) {
        const int half = cnt >> 1;
        if (g_en[lo + half] <= ps) { lo += half + 1; cnt -= half + 1; } else cnt = half;
      }
      int best = -1;
      long long bi = 0, bu = 1;
      for (int g = lo; g < n; ++g) {
        const int gs = g_st[g];
        if (gs >= pe) break;
        if (g_lab[g] != lab) continue;
        const int ge = g_en[g];
        const long long inter = (long long)(min(pe, ge) - max(ps, gs)), uni = (long long)(max(pe, ge) - min(ps, gs));
        if (best < 0 || inter * bu > bi * uni) { best = g; bi = inter; bu = uni; }
      }
      if (best >= 0) {
        unsigned bits = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) if (bi * (long long)A.den[k] >= bu * (long long)A.num[k]) bits |= 1u << k;
        if (bits) atomicOr(&g_hit[best], bits);
      }
    }
    __syncthreads();
    int t0 = 0, t1 = 0, t2 = 0;
    for (int g = tid; g < n; g += 256) { const unsigned h = g_hit[g]; t0 += h & 1u; t1 += (h >> 1) & 1u; t2 += (h >> 2) & 1u; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      correct += __shfl_xor(correct, o, 64); t0 += __shfl_xor(t0, o, 64); t1 += __shfl_xor(t1, o, 64); t2 += __shfl_xor(t2, o, 64);
    }
    if (lane == 0) { red[wave][0] = correct; red[wave][1] = t0; red[wave][2] = t1; red[wave][3] = t2; }
    // ---- 3. edit distance of the label lists ----
    const bool p_short = m <= n;
    const int ns = p_short ? m : n, nl = p_short ? n : m;
    const int *s_lab = p_short ? p_lab : g_lab, *l_lab = p_short ? g_lab : p_lab;
    int dist;
    if (ns == 0) dist = nl;
    else if (ns <= kSegmentalLdsSegments) dist = seg_edit_distance(s_lab, ns, l_lab, nl, lds_diag, ns + 1);
    else dist = seg_edit_distance(s_lab, ns, l_lab, nl, A.diag + 3 * (a + v), ns + 1);
    __syncthreads();                                        // red is written (ns == 0 passes no barrier above); everyone has read its dist
    // ---- 4. the record ----
    if (tid == 0) {
      int r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
      int4* out = (int4*)(A.records + (size_t)v * 8);
      out[0] = make_int4(r[0], (int)(b - a), m, n);
      out[1] = make_int4(dist, r[1], r[2], r[3]);
    }
    __syncthreads();                                        // red and the diagonals are free for the next video
  }
}

// Returns 0, or -1 on a bad argument (nothing launched).  ws must hold segmental_workspace_bytes(n_frames, n_videos) bytes.
int launch_segmental(const int* pred, const int* gt, const int* offsets, int n_videos, long long n_frames, const unsigned* bg, const int* num,
                     const int* den, int* records, void* ws, hipStream_t s) {
  if (n_videos < 1 || n_frames < 0 || n_frames >= (1ll << 31)) return -1;
  SegArgs A;
  A.pred = pred; A.gt = gt; A.offsets = offsets; A.n_videos = n_videos; A.n_frames = n_frames; A.records = records;
  for (int k = 0; k < 4; ++k) A.bg[k] = bg[k];
  for (int k = 0; k < 3; ++k) { A.num[k] = num[k]; A.den[k] = den[k]; }
  int* w = (int*)ws;
  const size_t n = (size_t)n_frames;
  A.p_lab = w; A.p_st = w + n; A.p_en = w + 2 * n; A.g_lab = w + 3 * n; A.g_st = w + 4 * n; A.g_en = w + 5 * n;
  A.g_hit = (unsigned*)(w + 6 * n);
  A.diag = w + 7 * n;
  A.vec = (((uintptr_t)pred | (uintptr_t)gt) % 16) == 0;
  segmental_kernel<<<n_videos < SEG_GRID ? n_videos : SEG_GRID, 256, 0, s>>>(A);
  return 0;
}
