// Host-side error plumbing of the C ABI (include/statecatcher.h).
#include <stdarg.h>
#include <stdio.h>

#include "sc_common.h"

namespace sc {

static thread_local char g_err[512];

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void clear_error() { g_err[0] = 0; }

int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace sc

extern "C" int sc_abi_version(void) { return SC_ABI_VERSION; }
extern "C" const char* sc_last_error(void) { return sc::g_err; }

// The struct layouts the Python binding derives from the header (ctypes computes the same numbers;
// tests/test_capi.py pins them on that side).
#define SC_LAYOUT(T, size, last, off)                                        \
  static_assert(sizeof(T) == size, #T ": sizeof changed (ABI)");             \
  static_assert(offsetof(T, last) == off, #T ": field offsets changed (ABI)")
SC_LAYOUT(sc_adam_tensor, 40, n, 32);
SC_LAYOUT(sc_image_job, 80, row_shift, 72);
SC_LAYOUT(sc_ln_fold_job, 80, D, 72);
SC_LAYOUT(sc_frame_gemm_job, 144, mask, 136);
SC_LAYOUT(sc_frame_cell_job, 120, D, 116);
SC_LAYOUT(sc_tframe_job, 136, mask, 128);
#undef SC_LAYOUT
