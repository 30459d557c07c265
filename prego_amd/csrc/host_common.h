// Shared by every host translation unit (*.cpp) of the library: error plumbing and two small helpers.
#pragma once
#include "../../include/prego_amd.h"
#ifdef PREGO_DEBUG_ABI
#include "../../include/prego_amd_debug.h"
#endif
#include "kernels.h"      // declares prego_tune_env (defined in miniroad.cpp: getenv in the debug library, NULL in the product library)

#include <cstddef>

// Records the message for prego_last_error() and, when an entry point of a MiniROAD handle is running on this thread (HandleScope,
// miniroad_handle.h), for prego_miniroad_last_error(h) as well; returns `code`.  Defined in miniroad.cpp beside the error state.
int prego_fail_(int code, const char* fmt, ...);
#define HIPCHK(x)                                                                                          \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) return prego_fail_(PREGO_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));      \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator over a caller's workspace: put() returns the block's offset, every block starts on a 256-byte boundary, off is the
// total so far.  log (prego_debug_vit_layout only): (offset, bytes asked for) of every block, in order
struct ArenaLog { size_t* v; int cap, n; };
struct Arena {
  size_t off = 0;
  ArenaLog* log = nullptr;
  size_t put(size_t bytes) {
    const size_t o = off;
    off += align_up(bytes, 256);
    if (log) {
      if (log->n < log->cap) { log->v[2 * log->n] = o; log->v[2 * log->n + 1] = bytes; }
      ++log->n;
    }
    return o;
  }
};
