// Geometry and exchange layout of the persistent GRU recurrences (gru_recurrence.hip: classic / multi-tile, gru_recurrence_x2.hip,
// gru_bptt.hip), stated once for the kernels AND the host: buffer sizes, group sizes and LDS sizes come from the expressions the
// kernels index with, and the statement blocks the forward kernels share.  Nothing here is a function call inside a kernel: hipcc's
// register allocation of these kernels moves with any helper call in them (profiles/gru_ab/codegen.md), so the kernels take
// constants and macros, and compile to the code they were.
#pragma once
#include "common.h"

// Clip tiles per group an exchange buffer is LAID OUT for against tiles a launch may RUN.  The 16-bit / fp32 layout keeps room for 8
// (128 slots per group: the fragment stride the kernels were tuned at - a 1 KiB fragment of tile ct sits 8 KiB from its k-neighbour);
// kernels exist for 1, 2 and 4 live tiles (8 spills registers).  The split-operand layout is built for 4 and runs 2 (2 x 96 weight registers)
#define GRU_MAX_TILES 8
#define GRU_RUN_TILES 4
#define GRU_X2_TILES 4
#define GRU_X2_RUN_TILES 2

constexpr int gru_kf(int wb) { return wb == 2 ? 32 : 16; }      // k per MFMA B-fragment (wb = operand bytes)
constexpr int gru_epl(int wb) { return wb == 2 ? 8 : 4; }       // elements per lane and fragment (16 bytes)
constexpr int gru_ut(int wb, int hid) { return wb == 2 && hid <= 1024 ? 2 : 1; }   // 16-row unit tiles a workgroup owns
constexpr int gru_plane_bytes(int wb, int k, int tiles) { return (k / gru_kf(wb)) * tiles * 1024; }   // [fragment k / KF][tile][lane 0..63][16 B]
constexpr int gru_red_bytes(int ngate, int ut) { return 2 * 4 * ngate * ut * 64 * 16; }   // [2 parities][4 waves][gates][UT][64 lanes] f32x4
// the multi-tile kernel's LDS behind the reduction buffers: two gather images per wave of nks fragments, the gi rows of two steps
constexpr int gru_mt_gather_bytes(int nks) { return 2 * 4 * nks * 1024; }
constexpr int gru_mt_gi_bytes(int nct) { return 2 * nct * 3 * 1024; }

// WB operand bytes, UT unit tiles, TILES the layout's tiles, PLANES x REGIONS copies of a plane per group (fp16x2: hi | lo, L | R)
template <int WB, int HID, int UT, int TILES, int PLANES = 1, int REGIONS = 1>
struct GruGeom {
  static constexpr int UNITS = 16 * UT, P = HID / UNITS, KQ = HID / 4, KF = gru_kf(WB), EPL = gru_epl(WB), NKS = KQ / KF;
  static constexpr unsigned TAGM = WB == 2 ? 0x40004000u : 0x40000000u;         // the free top exponent bit of every element (|h| < 2)
  static constexpr int PLANE_BYTES = gru_plane_bytes(WB, HID, TILES), REGION_BYTES = PLANES * PLANE_BYTES, GROUP_BYTES = REGIONS * REGION_BYTES;
  static constexpr int RED_STRIDE = 4 * 3 * UT * 64, RED_BYTES = gru_red_bytes(3, UT);
};

// Exchange layout = MFMA B-fragment order, so that a consumer's fragment load is ONE contiguous 1 KiB (rows at a 2 KiB stride all
// fell on the same L2 channel and ran at 10 B/clk/CU).  Element (clip column col of tile ct, contraction index k): fragment k / KF,
// lane ((k % KF) / EPL) * 16 + col, byte (k % EPL) * WB.  GRU_HX_FRAG: where the 1 KiB of (fragment, tile) starts; lane l of a consumer
// reads 16 bytes at + 16 l.  Macros, so that publisher and gather of every kernel share ONE text and compile to what they were.
#define GRU_HX_FRAG(TILES, frag, ct) (((frag) * TILES + ct) * 1024)
#define GRU_HX_OFFSET(KF, EPL, WB, TILES, col, k, ct) \
  (((k / KF) * TILES + ct) * 1024 + ((((k % KF) / EPL) << 4) + col) * 16 + (k % EPL) * WB)
constexpr int gru_hx_offset(int wb, int tiles, int col, int k, int ct) { return GRU_HX_OFFSET(gru_kf(wb), gru_epl(wb), wb, tiles, col, (k), ct); }
// the inverse: what byte `byte` of lane `lane`'s 16 bytes of fragment `frag` holds - the B operand the MFMA wants there
constexpr int gru_hx_k_at(int wb, int frag, int lane, int byte) { return frag * gru_kf(wb) + (lane >> 4) * gru_epl(wb) + byte / wb; }
constexpr int gru_hx_col_at(int lane) { return lane & 15; }

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- statement blocks the forward kernels (classic, multi-tile, fp16x2) share.  Macros over the kernel's own names (a, sidx, hreg,
// redw, ...), not functions, for the reason at the top: as functions each of them moved registers, spills or scratch somewhere.
// Continuous batching: a slot runs several clips back to back; h restarts from 0 where the next clip begins.  nstart: the step at
// which the slot's next clip starts, segp / sege: its segment and the slot's last + 1.  ZERO_H zeroes the lane's state of tile ct
// (a clip starts on this launch's first step)
#define GRU_SEG_INIT(ct, ZERO_H)                                                        \
  nstart[ct] = 0x7fffffff; segp[ct] = 0; sege[ct] = 0;                                  \
  if (a.seg_start != nullptr && sidx[ct] < a.n_clips) {                                 \
    int k = a.seg_off[sidx[ct]];                                                        \
    sege[ct] = a.seg_off[sidx[ct] + 1];                                                 \
    while (k < sege[ct] && a.seg_start[k] < a.t0) ++k;                                  \
    if (k < sege[ct] && a.seg_start[k] == a.t0 && a.t0 > 0) { ZERO_H }                  \
    while (k < sege[ct] && a.seg_start[k] <= a.t0) ++k;                                 \
    segp[ct] = k;                                                                       \
    nstart[ct] = k < sege[ct] ? a.seg_start[k] : 0x7fffffff;                            \
  }
// after a restart: on to the slot's next clip.  The pin takes the (rare) load's wait here, not as a vmcnt(0) in every step
#define GRU_SEG_ADVANCE(ct)                                                             \
  ++segp[ct];                                                                           \
  nstart[ct] = segp[ct] < sege[ct] ? a.seg_start[segp[ct]] : 0x7fffffff;                \
  asm volatile("" : "+v"(nstart[ct]));
// Plan look-ahead.  The plan tables are read-only for the whole launch: constant address space = scalar (s_load) path, so the
// look-ahead never touches the vector-memory queue (a vector load here drags a vmcnt wait through every step).  The scalars run one
// step ahead of their use (s_load latency off the critical path); rowoff is carried RAW and row_base subtracted where it is used: a
// subtraction next to the look-ahead s_load makes hipcc wait for that load at the top of every step
#define GRU_PLAN_INIT                                                                   \
  typedef const __attribute__((address_space(4))) int* cint_p;                          \
  cint_p nact_c = (cint_p)a.nact;                                                       \
  cint_p rowoff_c = (cint_p)a.rowoff;                                                   \
  const int nsteps = a.t1 - a.t0;                                                       \
  int na_c = nact_c[a.t0], rb_c = rowoff_c[a.t0];                                       \
  int na_n = nsteps > 1 ? nact_c[a.t0 + 1] : 0, rb_n = nsteps > 1 ? rowoff_c[a.t0 + 1] : 0;
#define GRU_PLAN_PEEK                                                                   \
  const int t2 = (tl + 2 < nsteps) ? t + 2 : t;                                         \
  const int na_2 = nact_c[t2], rb_2 = rowoff_c[t2];
#define GRU_PLAN_SHIFT na_c = na_n; rb_c = rb_n; na_n = na_2; rb_n = rb_2;
// K-quarter sums of a lane that owns registers {own_r0, own_r0 + 1} of its tile: 8-byte LDS reads at immediate offsets, and the two
// elements go through the gate math as one f32x2 (v_pk_add/mul/fma_f32): the step runs one wave per SIMD, so every VALU instruction
// is ~4 cycles of its critical path.  The pin keeps all twelve reads in flight before the first add (left alone, hipcc recycles
// registers and serialises the LDS round trips: read 2, wait, add, read 2, wait, ...)
#define GRU_RED_READ2                                                                                                            \
  const f32x2* rp = (const f32x2*)((const float*)&redw[own_ut * 64 + lane] + own_r0);                                            \
  f32x2 part[3][4];                                                                                                              \
  _Pragma("unroll") for (int gate = 0; gate < 3; ++gate)                                                                         \
    _Pragma("unroll") for (int qq = 0; qq < 4; ++qq) part[gate][qq] = rp[((qq * 3 + gate) * UT) * 64 * 2];                       \
  asm volatile("" : "+v"(part[0][0]), "+v"(part[0][1]), "+v"(part[0][2]), "+v"(part[0][3]), "+v"(part[1][0]), "+v"(part[1][1]),  \
                    "+v"(part[1][2]), "+v"(part[1][3]), "+v"(part[2][0]), "+v"(part[2][1]), "+v"(part[2][2]), "+v"(part[2][3])); \
  f32x2 gh[3];                                                                                                                   \
  _Pragma("unroll") for (int gate = 0; gate < 3; ++gate) gh[gate] = (part[gate][0] + part[gate][1]) + (part[gate][2] + part[gate][3]);
// packed gate math of tile ct: r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r (gh_n + b_hn)), h' = (1 - z) n + z h
#define GRU_GATES2(ct)                                                                  \
  const f32x2 hp = {hreg[ct][0], hreg[ct][1]}, bh = {bhn[0], bhn[1]};                   \
  const f32x2 xr = gr + gh[0], xz = gz + gh[1];                                         \
  f32x2 r, z, n;                                                                        \
  r[0] = sigmoidf_(xr[0]); r[1] = sigmoidf_(xr[1]);                                     \
  z[0] = sigmoidf_(xz[0]); z[1] = sigmoidf_(xz[1]);                                     \
  const f32x2 ghn = gh[2] + bh;                                                         \
  const f32x2 xn = gn + r * ghn;                                                        \
  n[0] = tanhf_(xn[0]); n[1] = tanhf_(xn[1]);                                           \
  const f32x2 hn = (one - z) * n + z * hp;                                              \
  hreg[ct][0] = hn[0]; hreg[ct][1] = hn[1];
