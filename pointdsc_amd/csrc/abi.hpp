// abi.hpp -- what every extern "C" entry point of libpdsc uses (host only): the
// status / last-error convention of include/pdsc.h and the workspace check.
//
// A row's entry points live in the row's file; api.hip is the forward.  Each
// entry is one function: check the arguments, size and carve the workspace,
// launch on the caller's stream.  No allocation, no synchronisation.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pdsc.h"
#include "workspace.hpp"

namespace pdsc {

// Formats the calling thread's pdsc_last_error() string and returns `code`
// (api.hip: the one definition, beside the string it writes).
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// The checks the forwards and the encoder row's entries share (api.hip): the
// config's supported ranges; then B, N and what the config makes of N: the seeds
// S = int(N * ratio) and k = min(cfg k, N - 1), the one place that computes them.
int check_cfg(const pdsc_config *cfg);
int check_shape(const pdsc_config *cfg, int B, int N, int &S, int &k);

inline hipStream_t S_(pdsc_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int need_ws(size_t have, size_t need) {
    if (have < need) return fail(PDSC_ERR_ARG, "workspace too small: %zu < %zu bytes", have, need);
    return PDSC_OK;
}

}  // namespace pdsc

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return pdsc::fail(PDSC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

#define RET_IF(x)                     \
    do {                              \
        int r_ = (x);                 \
        if (r_ != PDSC_OK) return r_; \
    } while (0)
