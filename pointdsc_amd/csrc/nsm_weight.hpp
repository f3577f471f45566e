// nsm_weight.hpp -- a8's last step, shared by the two kernels that run it:
// nsm_finish_kernel (nsm.hip) and kabsch_sums_kernel<.., FIN> (hypotheses.hip),
// which finishes the weights inside the hypotheses' first launch.
#pragma once
#include "pdsc_common.hpp"

namespace pdsc {

// w = v_{t*} / (sum v_{t*} + 1e-6)  (models/PointDSC.py:280-282)
// The first iterate t* (1-based; T when none) at which every one of the nq
// seeds' allclose bits from q0 on is set: torch.allclose over the iterate the
// reference compares at once (:354).  Wave-uniform.
PDSC_DEV int nsm_tstar(const unsigned *__restrict__ seed_flags, size_t q0, size_t nq, int T, int lane) {
    unsigned all = 0xffffffffu;
    if (T > 0)
        for (size_t q = lane; q < nq; q += 64) all &= seed_flags[q0 + q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) all &= (unsigned)__shfl_xor((int)all, o);
    const unsigned m = all & ((T >= 32) ? 0xffffffffu : ((1u << T) - 1u));
    return m ? (__ffs(m)) : T;
}
// This lane's normalised weight of seed row `row` (= b * S + s) from its
// iterate t* (lanes >= k: 0).
PDSC_DEV float nsm_weight(const float *__restrict__ hist, size_t row, int tstar, int k, int T, int lane) {
    float v = 1.0f;
    if (tstar > 0 && lane < k) v = hist[(row * T + (tstar - 1)) * k + lane];
    if (lane >= k) v = 0.0f;
    const float sum = wave_sum(v);
    return lane < k ? v / (sum + 1e-6f) : 0.0f;
}

}  // namespace pdsc
