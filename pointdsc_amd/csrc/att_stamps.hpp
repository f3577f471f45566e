// att_stamps.hpp -- the -DATT_STAMPS build's timestamp buffer and macros (empty
// otherwise).  g_att_stamps is static: every translation unit that includes
// this has a buffer of its own, read by the pdsc_diag_*_stamps entry compiled
// in that unit (DESIGN.md "Diagnostic builds").
#pragma once
#include "pdsc_common.hpp"

namespace pdsc {

// Diagnostic build only (-DATT_STAMPS, tools/att_stamps.py): s_memtime stamps of
// the waves of every 16th workgroup (the first 64 of them) -- per key tile: top,
// S and M ready, softmax done, PV issued, barrier passed; then the chain phase.
// Stamps go to a buffer of their own that nothing in the kernel reads.
#ifdef ATT_STAMPS
constexpr int ST_PER_WAVE = 256, ST_WGS = 64;  // (192 + 3 c .. : the fused chain's chunk c, w2_layer)
static __device__ unsigned long long g_att_stamps[ST_WGS * 4 * ST_PER_WAVE];
PDSC_DEV unsigned long long *att_stamp_ptr(int wave) {
    return (blockIdx.x % 16 == 0 && blockIdx.x / 16 < ST_WGS && wave < 4 && blockIdx.z == 0)
               ? g_att_stamps + ((blockIdx.x / 16) * 4 + wave) * ST_PER_WAVE
               : nullptr;
}
#define ATT_STAMP(stp, i)                                                       \
    do {                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                      \
        if (stp) {                                                              \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();         \
            if (lane == 0) stp[i] = t_;                                         \
        }                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                      \
    } while (0)
#define ATT_RSTAMP(stp, i)                                                      \
    do {                                                                        \
        if (stp) {                                                              \
            const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();     \
            if (lane == 0) stp[i] = t_;                                         \
        }                                                                       \
    } while (0)
#define CH_STAMP(i)                                       \
    do {                                                  \
        unsigned long long *stc_ = att_stamp_ptr(wave);   \
        ATT_STAMP(stc_, i);                               \
    } while (0)
#else
#define CH_STAMP(i) \
    do {            \
    } while (0)
#define ATT_STAMP(stp, i) \
    do {                  \
    } while (0)
#define ATT_RSTAMP(stp, i) \
    do {                   \
    } while (0)
#endif

}  // namespace pdsc
