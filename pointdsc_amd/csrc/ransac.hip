// ransac.hip -- f6: RANSAC on correspondences on the GPU, the reference drivers'
// registration_ransac_based_on_correspondence (baseline_scripts/baseline_3DMatch.py:80-98,
// evaluation/test_3DMatch.py:59-77, algorithms/FR.py:122-150) restated with the
// choices open3d leaves open fixed (include/pdsc.h, f6): a counter-based
// sampler, fp64 everywhere, a total order on hypotheses, the confidence stop
// at round granularity.  Hypotheses are processed in rounds of RANSAC_ROUND:
//
//   hypotheses   one lane per hypothesis draws its sample (integer arithmetic
//                only), rejects repeated indices and, with the edge-length
//                checker on, samples whose edges disagree.  The survivors of a
//                workgroup are compacted by ballot + prefix in lane order (so
//                the order does not depend on timing, and the slot keeps its
//                h), and the first `survivors` lanes solve the unit-weight
//                Kabsch of one survivor each: full waves there too.
//   score        a lane holds one surviving hypothesis's 12 fp64 coefficients;
//                the grid is (64 hypotheses) x (RANSAC_PCHUNK points).  The
//                chunk's points sit in LDS as fp64 and every lane reads the
//                same address (a broadcast).  Per (hypothesis, chunk): the
//                inlier count and sum d^2 in point order.  Survivors of all the
//                round's workgroups are addressed through the prefix of the
//                workgroups' counts, so the waves are full whatever the
//                checker's rejection rate.
//   round        one workgroup adds each hypothesis's chunk rows in chunk
//                order, reduces the round under (count desc, sumsq asc, h asc)
//                -- a total order, so the reduction tree cannot change the
//                winner -- folds it into the state block and applies the stop
//                rule.
//   finish       labels, the optional refit (fp64 Kabsch over the winner's
//                inliers, centred, fixed order) and the result.
//
// Everything is enqueued up front; once the state's `done` word is set the
// remaining rounds' kernels return at entry (as icp.hip).  No float atomics:
// two calls are bitwise equal.
#include "ransac_shared.hpp"

namespace pdsc {

// ------------------------------------------------------------------------ init
// The state block, and the debug rows' "never drawn" status (the rounds after an
// early stop return at entry and cannot write it).
__global__ __launch_bounds__(256) void ransac_init_kernel(RansacState *st, int H, int *dbg_count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (dbg_count && i < (size_t)H) dbg_count[i] = -3;
    if (i == 0) {
        for (int k = 0; k < 12; ++k) st->c[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        st->sumsq = 0.0;
        st->count = -1;
        st->best = -1;
        st->iterations = 0;
        st->n_validated = 0;
        st->done = 0;
        st->pad = 0;
    }
}

// ----------------------------------------------------------------------- round
struct RansacCand {
    double ss;
    int cnt, h, slot;
};
// (count desc, sumsq asc, h asc): a total order over distinct h
PDSC_DEV bool ransac_better(const RansacCand &a, const RansacCand &b) {
    return a.cnt > b.cnt || (a.cnt == b.cnt && (a.ss < b.ss || (a.ss == b.ss && a.h < b.h)));
}

__global__ __launch_bounds__(RANSAC_FIN) void ransac_round_kernel(int N, int nwg, int nchunks, int round, int H,
                                                                  int ns, double confidence, RansacBufs B,
                                                                  pdsc_ransac_debug dbg) {
    __shared__ RansacCand wbest[RANSAC_FIN / 64];
    RansacState *st = B.st;
    if (st->done) return;  // workgroup-uniform
    const int tid = threadIdx.x;
    int total = 0;
    for (int k = 0; k < nwg; ++k) total += B.wgcount[k];
    RansacCand best = {0.0, -1, 0x7fffffff, 0};
    for (int g = tid; g < total; g += RANSAC_FIN) {
        RansacCand x = {0.0, 0, 0, B.gslot[g]};
        for (int ch = 0; ch < nchunks; ++ch) {  // chunk order
            x.cnt += B.pcount[(size_t)ch * RANSAC_ROUND + g];
            x.ss += B.psum[(size_t)ch * RANSAC_ROUND + g];
        }
        x.h = B.hidx[x.slot];
        if (dbg.count) dbg.count[x.h] = x.cnt;
        if (dbg.sumsq) dbg.sumsq[x.h] = x.ss;
        if (ransac_better(x, best)) best = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RansacCand y;
        y.ss = __shfl_xor(best.ss, o);
        y.cnt = __shfl_xor(best.cnt, o);
        y.h = __shfl_xor(best.h, o);
        y.slot = __shfl_xor(best.slot, o);
        if (ransac_better(y, best)) best = y;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < RANSAC_FIN / 64; ++k)
        if (ransac_better(wbest[k], best)) best = wbest[k];
    // an earlier round's winner has the lower h: it keeps an exact tie
    if (best.cnt >= 0 && (best.cnt > st->count || (best.cnt == st->count && best.ss < st->sumsq))) {
        for (int k = 0; k < 12; ++k) st->c[k] = B.coef[(size_t)k * RANSAC_ROUND + best.slot];
        st->sumsq = best.ss;
        st->count = best.cnt;
        st->best = best.h;
    }
    const long long drawn = ((long long)round + 1) * RANSAC_ROUND;
    st->iterations = drawn < (long long)H ? (int)drawn : H;
    st->n_validated += total;
    if (confidence < 1.0 && st->count > 0) {
        bool stop = st->count == N;  // f = 1: the criterion's log(0)
        if (!stop) {
            const double f = (double)st->count / (double)N;
            const double fn = ns == 3 ? f * f * f : (f * f) * (f * f);
            stop = (double)drawn >= log(1.0 - confidence) / log(1.0 - fn);
        }
        if (stop) st->done = 1;
    }
}

// ---------------------------------------------------------------------- finish

__global__ __launch_bounds__(RANSAC_FIN) void ransac_finish_kernel(const float *__restrict__ src,
                                                                   const float *__restrict__ tgt, int N, double r2,
                                                                   int refit, const RansacState *st, float *trans_f32,
                                                                   float *labels, pdsc_ransac_result *res) {
    __shared__ double red[RANSAC_FIN / 64];
    const int tid = threadIdx.x;
    const int count = st->count;  // -1: no valid hypothesis (c is the identity)
    double c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = st->c[k];
    const bool refit_now = refit && count > 0;  // workgroup-uniform
    double n = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    for (int i = tid; i < N; i += RANSAC_FIN) {
        const D3 a = load3(src, i), b = load3(tgt, i);
        const bool in = count >= 0 && ransac_d2(c, a.x, a.y, a.z, b.x, b.y, b.z) < r2;
        if (labels) labels[i] = in ? 1.0f : 0.0f;
        if (in) {
            n += 1.0;
            sa[0] += a.x, sa[1] += a.y, sa[2] += a.z;
            sb[0] += b.x, sb[1] += b.y, sb[2] += b.z;
        }
    }
    if (refit_now) {
        n = block_sum(n, red, tid);
        refit_kabsch(src, tgt, N, r2, n, sa, sb, c, red, tid);
    }
    if (tid != 0) return;
    double T[16];
    T[0] = c[0], T[1] = c[1], T[2] = c[2], T[3] = c[9];
    T[4] = c[3], T[5] = c[4], T[6] = c[5], T[7] = c[10];
    T[8] = c[6], T[9] = c[7], T[10] = c[8], T[11] = c[11];
    T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
    if (res) {
        for (int i = 0; i < 16; ++i) res->trans[i] = T[i];
        res->fitness = count > 0 ? (double)count / (double)N : 0.0;
        res->inlier_rmse = count > 0 ? sqrt(st->sumsq / (double)count) : 0.0;
        res->n_inliers = count > 0 ? count : 0;
        res->iterations = st->iterations;
        res->best = st->best;
        res->n_validated = st->n_validated;
    }
    if (trans_f32)
        for (int i = 0; i < 16; ++i) trans_f32[i] = (float)T[i];
}

// ---------------------------------------------------------------- refit_inliers
// pdsc_refit_inliers (f7): ransac_finish_kernel's refit over a point set of the
// caller's choice under a pose of the caller's (FR.py:101-114 refits over the
// unfiltered pairs, RANSAC scored the filtered ones).  With fewer than 3 inliers
// the pose is returned unchanged.
__global__ __launch_bounds__(RANSAC_FIN) void refit_inliers_kernel(const double *pose,  // trans may alias it
                                                                   const float *__restrict__ src,
                                                                   const float *__restrict__ tgt, int N, double r2,
                                                                   double *trans, float *trans_f32, int *count,
                                                                   float *labels) {
    __shared__ double red[RANSAC_FIN / 64];
    const int tid = threadIdx.x;
    double T[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = pose[k];
    double c[12] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10], T[3], T[7], T[11]};
    double n = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    for (int i = tid; i < N; i += RANSAC_FIN) {
        const D3 a = load3(src, i), b = load3(tgt, i);
        const bool in = ransac_d2(c, a.x, a.y, a.z, b.x, b.y, b.z) < r2;
        if (labels) labels[i] = in ? 1.0f : 0.0f;
        if (in) {
            n += 1.0;
            sa[0] += a.x, sa[1] += a.y, sa[2] += a.z;
            sb[0] += b.x, sb[1] += b.y, sb[2] += b.z;
        }
    }
    n = block_sum(n, red, tid);  // workgroup-uniform
    if (n >= 3.0) {
        refit_kabsch(src, tgt, N, r2, n, sa, sb, c, red, tid);
        T[0] = c[0], T[1] = c[1], T[2] = c[2], T[3] = c[9];
        T[4] = c[3], T[5] = c[4], T[6] = c[5], T[7] = c[10];
        T[8] = c[6], T[9] = c[7], T[10] = c[8], T[11] = c[11];
        T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
    }
    if (tid != 0) return;
    for (int i = 0; i < 16; ++i) trans[i] = T[i];
    if (trans_f32)
        for (int i = 0; i < 16; ++i) trans_f32[i] = (float)T[i];
    if (count) count[0] = (int)n;
}

hipError_t launch_refit_inliers(const double *pose, const float *src, const float *tgt, int N, double radius,
                                double *trans, float *trans_f32, int *count, float *labels, hipStream_t s) {
    hipLaunchKernelGGL(refit_inliers_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, pose, src, tgt, N, radius * radius, trans,
                       trans_f32, count, labels);
    return hipGetLastError();
}

// ------------------------------------------------------------------- launchers
size_t ransac_workspace_bytes(int N) {
    const size_t R = RANSAC_ROUND;
    return align_bytes(sizeof(RansacState)) + align_bytes(RANSAC_NWG * sizeof(int)) + 2 * align_bytes(R * sizeof(int)) +
           align_bytes(12 * R * sizeof(double)) + align_bytes(ransac_chunks(N) * R * sizeof(int)) +
           align_bytes(ransac_chunks(N) * R * sizeof(double));
}

hipError_t launch_ransac(const float *src, const float *tgt, int N, double max_distance, int ransac_n, double sim,
                         int H, double confidence, unsigned long long seed, int refit, float *trans_f32, float *labels,
                         pdsc_ransac_result *res, const pdsc_ransac_debug *debug, void *ws, hipStream_t s) {
    const size_t R = RANSAC_ROUND;
    const int nchunks = (int)ransac_chunks(N);
    RansacBufs B;
    ransac_bind(static_cast<char *>(ws), N, B);
    pdsc_ransac_debug dbg = {nullptr, nullptr, nullptr, nullptr};
    if (debug) dbg = *debug;
    const double r2 = max_distance * max_distance;
    const int init_blocks = dbg.count ? (int)(((size_t)H + 255) / 256) : 1;
    hipLaunchKernelGGL(ransac_init_kernel, dim3(init_blocks), dim3(256), 0, s, B.st, H, dbg.count);
    const int rounds = (int)(((size_t)H + R - 1) / R);
    for (int r = 0; r < rounds; ++r) {
        const long long base = (long long)r * RANSAC_ROUND;
        const int nh = (int)((long long)H - base < (long long)R ? (long long)H - base : (long long)R);
        const int nwg = (nh + RANSAC_HWG - 1) / RANSAC_HWG;
        if (ransac_n == 3)
            hipLaunchKernelGGL(ransac_hyp_kernel<3>, dim3(nwg), dim3(RANSAC_HWG), 0, s, src, tgt, N, (int)base, H,
                               (u64)seed, sim, B, dbg);
        else
            hipLaunchKernelGGL(ransac_hyp_kernel<4>, dim3(nwg), dim3(RANSAC_HWG), 0, s, src, tgt, N, (int)base, H,
                               (u64)seed, sim, B, dbg);
        hipLaunchKernelGGL(ransac_score_kernel<false>, dim3((nh + 63) / 64, nchunks), dim3(64), 0, s, src, tgt, N, nwg,
                           r2, B);
        hipLaunchKernelGGL(ransac_round_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, N, nwg, nchunks, r, H, ransac_n,
                           confidence, B, dbg);
        HIP_RET(hipGetLastError());
    }
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, src, tgt, N, r2, refit, B.st, trans_f32,
                       labels, res);
    return hipGetLastError();
}

}  // namespace pdsc
