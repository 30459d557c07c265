// Host side of the procedure model (include/prego_amd.h: prego_procedure_*, prego_stream_pool_feed_judge, the _forecast entries at the
// end of this file; kernels: procedure.hip).  Create
// validates the corpus, sorts it by group and lays it out for the caller's device block; the model object keeps the host image alive for
// the copy and the geometry for the launches.  Every entry point decides all its refusals before its first copy or launch, so a refused
// call has written nothing.
//   block: goff [n_groups + 1] int32 | ex [n_examples] int32 | sym [n_symbols + n_transcripts] bytes, each part 256-byte aligned
// Caps, from the word widths: a position in sym is one int32 word, so n_sym <= 2^30; tot and cnt are int32 words of the verdict and of
// the LDS counters, so n_examples <= 2^24 - and cnt * den <= 2^24 * 2^15 = 2^39 fits the 64-bit product; goff is indexed by an int32
// group, n_groups <= 2^20 keeps the table at 4 MB.  A symbol is one byte: ncls <= 128 leaves 0xff for START and 0xfe for "no match".
#include "pool_slot_check.h"

#include <cstdint>
#include <vector>

namespace {
constexpr int kProcMaxGroups = 1 << 20;
constexpr long long kProcMaxExamples = 1ll << 24, kProcMaxSymbols = 1ll << 30;

struct ProcLayout { size_t goff, ex, sym, total; };
ProcLayout proc_layout(long long n_groups, long long n_sym, long long n_examples) {
  ProcLayout l{};
  l.goff = 0;
  l.ex = l.goff + align_up((size_t)(n_groups + 1) * 4, 256);
  l.sym = l.ex + align_up((size_t)n_examples * 4, 256);
  l.total = l.sym + align_up((size_t)n_sym, 256);
  return l;
}
bool proc_sizes_ok(long long n_groups, long long n_transcripts, long long n_symbols, long long n_examples) {
  return n_groups >= 0 && n_groups <= kProcMaxGroups && n_transcripts >= 0 && n_symbols >= 0 && n_symbols + n_transcripts <= kProcMaxSymbols &&
         n_examples >= 0 && n_examples <= kProcMaxExamples && n_examples <= n_symbols;
}
size_t verdict_bytes_for(long long n) { return (size_t)n * kProcVerdictWords * 4; }
}  // namespace

struct prego_procedure_model {
  ProcGeom g;
  size_t bytes;                          // of the block, as laid out
  std::vector<char> image;               // what create copies into the block; alive until destroy, so the copy may run late
};

extern "C" size_t prego_procedure_model_bytes(int n_groups, int64_t n_transcripts, int64_t n_symbols, int64_t n_examples) {
  if (!proc_sizes_ok(n_groups, n_transcripts, n_symbols, n_examples)) return 0;
  return proc_layout(n_groups, n_symbols + n_transcripts, n_examples).total;
}

extern "C" int prego_procedure_model_create(prego_procedure_model** out, int n_classes, int order, int thr_num, int thr_den, int n_transcripts,
                                            const int32_t* groups, const int64_t* offsets, const int32_t* symbols, const uint8_t* targets,
                                            void* device_block, size_t bytes, prego_stream_t stream) {
  const char* who = "procedure_model_create";
  if (!out) return prego_fail_(PREGO_EINVAL, "%s: out is NULL", who);
  *out = nullptr;
  if (n_classes < 1 || n_classes > kProcMaxClasses) return prego_fail_(PREGO_EINVAL, "%s: n_classes %d (1..%d)", who, n_classes, kProcMaxClasses);
  if (order < 1 || order > kProcMaxOrder) return prego_fail_(PREGO_EINVAL, "%s: order %d (1..%d)", who, order, kProcMaxOrder);
  if (thr_num < 0 || thr_den < 1 || thr_num > thr_den || thr_den > kProcMaxDen)
    return prego_fail_(PREGO_EINVAL, "%s: threshold %d/%d (0 <= num <= den, 1 <= den <= %d)", who, thr_num, thr_den, kProcMaxDen);
  if (n_transcripts < 0) return prego_fail_(PREGO_EINVAL, "%s: %d transcripts", who, n_transcripts);
  if (!offsets) return prego_fail_(PREGO_EINVAL, "%s: offsets is NULL", who);
  if (n_transcripts > 0 && !groups) return prego_fail_(PREGO_EINVAL, "%s: groups is NULL", who);
  if (offsets[0] != 0) return prego_fail_(PREGO_EINVAL, "%s: offsets[0] = %lld (0)", who, (long long)offsets[0]);
  int n_groups = 0;
  for (int t = 0; t < n_transcripts; ++t) {
    if (offsets[t + 1] < offsets[t]) return prego_fail_(PREGO_EINVAL, "%s: offsets[%d] = %lld is below offsets[%d]", who, t + 1, (long long)offsets[t + 1], t);
    if (offsets[t + 1] > kProcMaxSymbols) return prego_fail_(PREGO_EINVAL, "%s: %lld symbols (at most %lld)", who, (long long)offsets[t + 1], kProcMaxSymbols);
    if (groups[t] < 0 || groups[t] >= kProcMaxGroups)
      return prego_fail_(PREGO_EINVAL, "%s: groups[%d] = %d (0..%d)", who, t, groups[t], kProcMaxGroups - 1);
    if (groups[t] >= n_groups) n_groups = groups[t] + 1;
  }
  const long long n_symbols = offsets[n_transcripts];
  if (n_symbols > 0 && !symbols) return prego_fail_(PREGO_EINVAL, "%s: symbols is NULL", who);
  long long n_examples = 0;
  for (long long i = 0; i < n_symbols; ++i) {
    if (symbols[i] < 0 || symbols[i] >= n_classes)
      return prego_fail_(PREGO_EINVAL, "%s: symbols[%lld] = %d is outside [0, %d)", who, i, symbols[i], n_classes);
    n_examples += !targets || targets[i];
  }
  if (!proc_sizes_ok(n_groups, n_transcripts, n_symbols, n_examples))
    return prego_fail_(PREGO_EINVAL, "%s: %lld symbols with %d STARTs (at most %lld), %lld examples (at most %lld)", who, n_symbols, n_transcripts,
                       kProcMaxSymbols, n_examples, kProcMaxExamples);
  const long long n_sym = n_symbols + n_transcripts;
  const ProcLayout l = proc_layout(n_groups, n_sym, n_examples);
  if (!device_block) return prego_fail_(PREGO_EINVAL, "%s: block is NULL", who);
  if ((uintptr_t)device_block & 255) return prego_fail_(PREGO_EINVAL, "%s: the block must be 256-byte aligned", who);
  if (bytes < l.total)
    return prego_fail_(PREGO_EWORKSPACE, "%s: block with %zu bytes, %d groups, %lld symbols in %d transcripts and %lld examples need %zu "
                       "(prego_procedure_model_bytes)", who, bytes, n_groups, n_symbols, n_transcripts, n_examples, l.total);

  prego_procedure_model* m = new prego_procedure_model();
  m->image.assign(l.total, 0);
  int* goff = (int*)(m->image.data() + l.goff);
  int* ex = (int*)(m->image.data() + l.ex);
  unsigned char* sym = (unsigned char*)(m->image.data() + l.sym);
  // a stable counting sort of the transcripts by group: where each group's examples and each transcript's symbols begin
  std::vector<long long> sym_at((size_t)n_groups + 1, 0), ex_at((size_t)n_groups + 1, 0);
  for (int t = 0; t < n_transcripts; ++t) {
    sym_at[(size_t)groups[t] + 1] += offsets[t + 1] - offsets[t] + 1;
    for (long long i = offsets[t]; i < offsets[t + 1]; ++i) ex_at[(size_t)groups[t] + 1] += !targets || targets[i];
  }
  for (int g = 0; g < n_groups; ++g) {
    sym_at[(size_t)g + 1] += sym_at[g];
    ex_at[(size_t)g + 1] += ex_at[g];
  }
  for (int g = 0; g <= n_groups; ++g) goff[g] = (int)ex_at[g];
  for (int t = 0; t < n_transcripts; ++t) {
    long long at = sym_at[groups[t]], e = ex_at[groups[t]];
    sym[at++] = (unsigned char)kProcStart;
    for (long long i = offsets[t]; i < offsets[t + 1]; ++i, ++at) {
      sym[at] = (unsigned char)symbols[i];
      if (!targets || targets[i]) ex[e++] = (int)at;
    }
    sym_at[groups[t]] = at;
    ex_at[groups[t]] = e;
  }
  char* base = (char*)device_block;
  m->g = ProcGeom{(const int*)(base + l.goff), (const int*)(base + l.ex), (const unsigned char*)(base + l.sym), n_classes, order, n_groups,
                  (int)n_examples, (int)n_sym, thr_num, thr_den};
  m->bytes = l.total;
  const hipError_t e = hipMemcpyAsync(device_block, m->image.data(), l.total, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) {
    delete m;
    return prego_fail_(PREGO_EHIP, "%s: hipMemcpyAsync failed: %s", who, hipGetErrorString(e));
  }
  *out = m;
  return PREGO_OK;
}

extern "C" void prego_procedure_model_destroy(prego_procedure_model* m) { delete m; }

extern "C" int prego_procedure_judge(const prego_procedure_model* m, int n_sequences, int n_positions, const int32_t* offsets,
                                     const int32_t* symbols, const int32_t* groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream) {
  const char* who = "procedure_judge";
  if (!m) return prego_fail_(PREGO_EINVAL, "%s: model is NULL", who);
  if (n_sequences < 1 || n_positions < 1 || n_positions > kProcMaxSymbols || n_sequences > n_positions)
    return prego_fail_(PREGO_EINVAL, "%s: %d sequences with %d positions (1 <= sequences <= positions <= %lld)", who, n_sequences, n_positions,
                       kProcMaxSymbols);
  if (!offsets) return prego_fail_(PREGO_EINVAL, "%s: offsets is NULL", who);
  if (!symbols) return prego_fail_(PREGO_EINVAL, "%s: symbols is NULL", who);
  if (!groups) return prego_fail_(PREGO_EINVAL, "%s: groups is NULL", who);
  if (!verdicts) return prego_fail_(PREGO_EINVAL, "%s: verdicts is NULL", who);
  if ((uintptr_t)verdicts & 255) return prego_fail_(PREGO_EINVAL, "%s: the verdicts must be 256-byte aligned", who);
  const size_t need = verdict_bytes_for(n_positions);
  if (verdict_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "%s: verdicts with %zu bytes, %d positions need %zu (32 each)", who, verdict_bytes, n_positions, need);
  if (launch_procedure_judge(m->g, n_sequences, n_positions, offsets, symbols, groups, (int*)verdicts, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

namespace {
int feed_judge(const char* who, const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
               const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream) {
  if (!f) return prego_fail_(PREGO_EINVAL, "%s: feed is NULL", who);
  if (!m) return prego_fail_(PREGO_EINVAL, "%s: model is NULL", who);
  if (!report) return prego_fail_(PREGO_EINVAL, "%s: report is NULL", who);
  if ((uintptr_t)report & 255) return prego_fail_(PREGO_EINVAL, "%s: the report must be 256-byte aligned", who);
  const int max_out = stream_pool_feed_geom(f)->max_out;
  const size_t need_report = prego_stream_pool_feed_report_bytes(max_out);
  if (report_bytes < need_report)
    return prego_fail_(PREGO_EWORKSPACE, "%s: report with %zu bytes, %d entries need %zu (prego_stream_pool_feed_report_bytes)", who, report_bytes,
                       max_out, need_report);
  if (!slot_groups) return prego_fail_(PREGO_EINVAL, "%s: slot_groups is NULL", who);
  if (!verdicts) return prego_fail_(PREGO_EINVAL, "%s: verdicts is NULL", who);
  if ((uintptr_t)verdicts & 255) return prego_fail_(PREGO_EINVAL, "%s: the verdicts must be 256-byte aligned", who);
  const size_t need = verdict_bytes_for(max_out);
  if (verdict_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "%s: verdicts with %zu bytes, %d entries need %zu (32 each)", who, verdict_bytes, max_out, need);
  if (launch_feed_judge(m->g, *stream_pool_feed_pool(f), max_out, (const int*)report, slot_groups, (int*)verdicts, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" int prego_stream_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                            const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream) {
  return feed_judge("stream_pool_feed_judge", f, m, report, report_bytes, slot_groups, verdicts, verdict_bytes, stream);
}

extern "C" int prego_vit_stream_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report,
                                                size_t report_bytes, const int32_t* slot_groups, void* verdicts, size_t verdict_bytes,
                                                prego_stream_t stream) {
  return feed_judge("vit_stream_pool_feed_judge", f, m, report, report_bytes, slot_groups, verdicts, verdict_bytes, stream);
}

// the decode pool's feed: its step ids are the decoder's classes, so a model of another class count cannot judge them
static int decode_model_refusal(const char* who, const PoolGeom* g, const prego_procedure_model* m) {
  if (g && m && m->g.ncls != g->ncls)
    return prego_fail_(PREGO_EINVAL, "%s: the procedure model has %d classes, the decode pool %d", who, m->g.ncls, g->ncls);
  return 0;
}

extern "C" int prego_decode_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                            const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream) {
  if (int rc = decode_model_refusal("decode_pool_feed_judge", f ? stream_pool_feed_pool(f) : nullptr, m)) return rc;
  return feed_judge("decode_pool_feed_judge", f, m, report, report_bytes, slot_groups, verdicts, verdict_bytes, stream);
}

// ---- next-step forecast: the same refusals in the same order for the five entries, decided before the launch ------------------------------
namespace {
size_t forecast_bytes_for(long long n) { return (size_t)n * kProcForecastWords * 4; }

// the forecast buffer of `rows` rows (`what` names them in the message); 0 = fine
int forecast_buffer_ok(const char* who, const void* forecasts, size_t forecast_bytes, long long rows, const char* what) {
  if (!forecasts) return prego_fail_(PREGO_EINVAL, "%s: forecasts is NULL", who);
  if ((uintptr_t)forecasts & 15) return prego_fail_(PREGO_EINVAL, "%s: the forecasts must be 16-byte aligned", who);
  const size_t need = forecast_bytes_for(rows);
  if (forecast_bytes < need)
    return prego_fail_(PREGO_EWORKSPACE, "%s: forecasts with %zu bytes, %lld %s need %zu (96 each)", who, forecast_bytes, rows, what, need);
  return 0;
}

int feed_forecast(const char* who, const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                  const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream) {
  if (!f) return prego_fail_(PREGO_EINVAL, "%s: feed is NULL", who);
  if (!m) return prego_fail_(PREGO_EINVAL, "%s: model is NULL", who);
  if (!report) return prego_fail_(PREGO_EINVAL, "%s: report is NULL", who);
  if ((uintptr_t)report & 255) return prego_fail_(PREGO_EINVAL, "%s: the report must be 256-byte aligned", who);
  const int max_out = stream_pool_feed_geom(f)->max_out;
  const size_t need_report = prego_stream_pool_feed_report_bytes(max_out);
  if (report_bytes < need_report)
    return prego_fail_(PREGO_EWORKSPACE, "%s: report with %zu bytes, %d entries need %zu (prego_stream_pool_feed_report_bytes)", who, report_bytes,
                       max_out, need_report);
  if (!slot_groups) return prego_fail_(PREGO_EINVAL, "%s: slot_groups is NULL", who);
  if (int rc = forecast_buffer_ok(who, forecasts, forecast_bytes, max_out, "entries")) return rc;
  if (launch_feed_forecast(m->g, *stream_pool_feed_pool(f), max_out, (const int*)report, slot_groups, (int*)forecasts, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

int pool_forecast(const char* who, const PoolGeom* g, const prego_procedure_model* m, const int32_t* slots, int n, const int32_t* slot_groups,
                  void* forecasts, size_t forecast_bytes, prego_stream_t stream) {
  if (!g) return prego_fail_(PREGO_EINVAL, "%s: pool is NULL", who);
  if (!m) return prego_fail_(PREGO_EINVAL, "%s: model is NULL", who);
  if (n < 1 || n > g->capacity) return prego_fail_(PREGO_EINVAL, "%s: %d slots (1..%d, the pool's capacity)", who, n, g->capacity);
  if (!slots) return prego_fail_(PREGO_EINVAL, "%s: slots is NULL", who);
  if (!slot_groups) return prego_fail_(PREGO_EINVAL, "%s: slot_groups is NULL", who);
  if (int rc = forecast_buffer_ok(who, forecasts, forecast_bytes, n, "slots")) return rc;
  if (launch_pool_forecast(m->g, *g, n, slots, slot_groups, (int*)forecasts, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}
}  // namespace

extern "C" int prego_procedure_forecast(const prego_procedure_model* m, int n_sequences, int n_positions, const int32_t* offsets,
                                        const int32_t* symbols, const int32_t* groups, void* forecasts, size_t forecast_bytes,
                                        prego_stream_t stream) {
  const char* who = "procedure_forecast";
  if (!m) return prego_fail_(PREGO_EINVAL, "%s: model is NULL", who);
  if (n_sequences < 1 || n_positions < 0 || (long long)n_positions + n_sequences > kProcMaxSymbols)
    return prego_fail_(PREGO_EINVAL, "%s: %d sequences with %d positions (1 <= sequences, 0 <= positions, together at most %lld)", who, n_sequences,
                       n_positions, kProcMaxSymbols);
  if (!offsets) return prego_fail_(PREGO_EINVAL, "%s: offsets is NULL", who);
  if (!symbols) return prego_fail_(PREGO_EINVAL, "%s: symbols is NULL", who);
  if (!groups) return prego_fail_(PREGO_EINVAL, "%s: groups is NULL", who);
  if (int rc = forecast_buffer_ok(who, forecasts, forecast_bytes, (long long)n_positions + n_sequences, "rows")) return rc;
  if (launch_procedure_forecast(m->g, n_sequences, n_positions, offsets, symbols, groups, (int*)forecasts, (hipStream_t)stream))
    return prego_fail_(PREGO_EINVAL, "%s: bad arguments", who);
  HIPCHK(hipGetLastError());
  return PREGO_OK;
}

extern "C" int prego_stream_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report,
                                               size_t report_bytes, const int32_t* slot_groups, void* forecasts, size_t forecast_bytes,
                                               prego_stream_t stream) {
  return feed_forecast("stream_pool_feed_forecast", f, m, report, report_bytes, slot_groups, forecasts, forecast_bytes, stream);
}

extern "C" int prego_vit_stream_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report,
                                                   size_t report_bytes, const int32_t* slot_groups, void* forecasts, size_t forecast_bytes,
                                                   prego_stream_t stream) {
  return feed_forecast("vit_stream_pool_feed_forecast", f, m, report, report_bytes, slot_groups, forecasts, forecast_bytes, stream);
}

extern "C" int prego_stream_pool_forecast(const prego_stream_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                                          const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream) {
  return pool_forecast("stream_pool_forecast", p ? stream_pool_geom(p) : nullptr, m, slots, n, slot_groups, forecasts, forecast_bytes, stream);
}

extern "C" int prego_vit_stream_pool_forecast(const prego_vit_stream_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                                              const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream) {
  return pool_forecast("vit_stream_pool_forecast", p ? vit_stream_pool_geom(p) : nullptr, m, slots, n, slot_groups, forecasts, forecast_bytes,
                       stream);
}

extern "C" int prego_decode_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report,
                                               size_t report_bytes, const int32_t* slot_groups, void* forecasts, size_t forecast_bytes,
                                               prego_stream_t stream) {
  if (int rc = decode_model_refusal("decode_pool_feed_forecast", f ? stream_pool_feed_pool(f) : nullptr, m)) return rc;
  return feed_forecast("decode_pool_feed_forecast", f, m, report, report_bytes, slot_groups, forecasts, forecast_bytes, stream);
}

extern "C" int prego_decode_pool_forecast(const prego_decode_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                                          const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream) {
  if (int rc = decode_model_refusal("decode_pool_forecast", p ? decode_pool_geom(p) : nullptr, m)) return rc;
  return pool_forecast("decode_pool_forecast", p ? decode_pool_geom(p) : nullptr, m, slots, n, slot_groups, forecasts, forecast_bytes, stream);
}
