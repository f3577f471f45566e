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
//                winner (ransac_shared.hpp: round_best) -- folds it into the
//                state block and applies the stop rule.
//   finish       labels, the optional refit (fp64 Kabsch over the winner's
//                inliers, centred, fixed order) and the result.
//
// Everything is enqueued up front; once the state's `done` word is set the
// remaining rounds' kernels return at entry (as icp.hip).  No float atomics:
// two calls are bitwise equal.
#include <cmath>

#include "ransac_shared.hpp"

namespace pdsc {

// ------------------------------------------------------------------------ init
// The state block and the debug rows' "never drawn" status.
__global__ __launch_bounds__(256) void ransac_init_kernel(RansacState *st, int H, int *dbg_count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    debug_prefill(dbg_count, H, i);
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
// (count desc, sumsq asc, h asc): a total order over distinct h, so the shape of
// round_best's reduction tree cannot change the winner
struct RansacBetter {
    PDSC_DEV bool operator()(const Cand &a, const Cand &b) const {
        return a.cnt > b.cnt || (a.cnt == b.cnt && (a.s < b.s || (a.s == b.s && a.h < b.h)));
    }
};

__global__ __launch_bounds__(RANSAC_FIN) void ransac_round_kernel(int N, int nwg, int nchunks, int round, int H,
                                                                  int ns, double confidence, RansacBufs B,
                                                                  pdsc_ransac_debug dbg) {
    __shared__ Cand wbest[RANSAC_FIN / 64];
    RansacState *st = B.st;
    if (st->done) return;  // workgroup-uniform
    const int tid = threadIdx.x;
    int total;
    const Cand best = round_best(B, nwg, nchunks, dbg, Cand{0.0, -1, 0x7fffffff, 0}, wbest, tid, total, RansacBetter{});
    if (tid != 0) return;
    // an earlier round's winner has the lower h: it keeps an exact tie
    if (best.cnt >= 0 && (best.cnt > st->count || (best.cnt == st->count && best.s < st->sumsq))) {
        for (int k = 0; k < 12; ++k) st->c[k] = B.coef[(size_t)k * RANSAC_ROUND + best.slot];
        st->sumsq = best.s;
        st->count = best.cnt;
        st->best = best.h;
    }
    const long long drawn = ((long long)round + 1) * RANSAC_ROUND;
    st->iterations = drawn < (long long)H ? (int)drawn : H;
    st->n_validated += total;
    if (confidence_stop(st->count, N, ns, drawn, confidence)) st->done = 1;
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
    label_inliers(src, tgt, N, c, r2, count >= 0, labels, n, sa, sb, tid);
    if (refit_now) {
        n = block_sum(n, red, tid);
        refit_kabsch(src, tgt, N, r2, n, sa, sb, c, red, tid);
    }
    if (tid != 0) return;
    double T[16];
    pose16(c, T);
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
    double T[16], c[12];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = pose[k];
    pose12(T, c);
    double n = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    label_inliers(src, tgt, N, c, r2, true, labels, n, sa, sb, tid);
    n = block_sum(n, red, tid);  // workgroup-uniform
    if (n >= 3.0) {
        refit_kabsch(src, tgt, N, r2, n, sa, sb, c, red, tid);
        pose16(c, T);
    }
    if (tid != 0) return;
    for (int i = 0; i < 16; ++i) trans[i] = T[i];
    if (trans_f32)
        for (int i = 0; i < 16; ++i) trans_f32[i] = (float)T[i];
    if (count) count[0] = (int)n;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

int32_t pdsc_refit_inliers(const double *pose, const float *src, const float *tgt, int32_t N, double radius,
                           double *trans, float *trans_f32, int32_t *count, float *labels, pdsc_stream_t stream) {
    if (N < 1) return fail(PDSC_ERR_ARG, "N=%d (need >= 1)", N);
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(PDSC_ERR_ARG, "radius %g must be > 0 and finite", radius);
    if (!pose || !src || !tgt || !trans) return fail(PDSC_ERR_ARG, "null pointer");
    hipLaunchKernelGGL(refit_inliers_kernel, dim3(1), dim3(RANSAC_FIN), 0, S_(stream), pose, src, tgt, N,
                       radius * radius, trans, trans_f32, count, labels);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

int32_t pdsc_ransac_round(void) { return RANSAC_ROUND; }

size_t pdsc_ransac_workspace_bytes(int32_t N) {
    if (N < 1) return 0;
    Carve c(nullptr);
    RansacBufs B;
    bind_ransac(c, N, B);
    return c.off;
}

// Enqueues every round and the finish.
int32_t pdsc_ransac_correspondence(const float *src, const float *tgt, int32_t N, double max_distance,
                                   int32_t ransac_n, double edge_similarity, int32_t max_iteration,
                                   double confidence, uint64_t seed, int32_t refit, float *trans_f32, float *labels,
                                   pdsc_ransac_result *result, const pdsc_ransac_debug *debug, void *ws,
                                   size_t ws_bytes, pdsc_stream_t stream) {
    if (ransac_n != 3 && ransac_n != 4)
        return fail(PDSC_ERR_UNSUPPORTED, "ransac_n=%d: only 3 and 4 are implemented", ransac_n);
    if (N < ransac_n) return fail(PDSC_ERR_ARG, "N=%d < ransac_n=%d", N, ransac_n);
    if (max_iteration < 1) return fail(PDSC_ERR_ARG, "max_iteration=%d (need >= 1)", max_iteration);
    if (!(max_distance > 0.0) || !std::isfinite(max_distance))
        return fail(PDSC_ERR_ARG, "max_distance %g must be > 0 and finite", max_distance);
    if (!(confidence > 0.0 && confidence <= 1.0)) return fail(PDSC_ERR_ARG, "confidence %g not in (0, 1]", confidence);
    if (!(edge_similarity >= 0.0 && edge_similarity <= 1.0))
        return fail(PDSC_ERR_ARG, "edge_similarity %g not in [0, 1]", edge_similarity);
    if (!src || !tgt || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_ransac_workspace_bytes(N)));
    hipStream_t s = S_(stream);
    const int H = max_iteration, nchunks = (int)ransac_chunks(N);
    Carve c(ws);
    RansacBufs B;
    bind_ransac(c, N, B);
    pdsc_ransac_debug dbg = {nullptr, nullptr, nullptr, nullptr};
    if (debug) dbg = *debug;
    const double r2 = max_distance * max_distance;
    const int init_blocks = dbg.count ? (int)(((size_t)H + 255) / 256) : 1;
    hipLaunchKernelGGL(ransac_init_kernel, dim3(init_blocks), dim3(256), 0, s, B.st, H, dbg.count);
    for (int r = 0, rounds = ransac_rounds(H); r < rounds; ++r) {
        const RoundShape q = ransac_round_shape(H, r);
        if (ransac_n == 3)
            hipLaunchKernelGGL(ransac_hyp_kernel<3>, dim3(q.nwg), dim3(RANSAC_HWG), 0, s, src, tgt, N, q.base, H,
                               (u64)seed, edge_similarity, B, dbg);
        else
            hipLaunchKernelGGL(ransac_hyp_kernel<4>, dim3(q.nwg), dim3(RANSAC_HWG), 0, s, src, tgt, N, q.base, H,
                               (u64)seed, edge_similarity, B, dbg);
        hipLaunchKernelGGL(ransac_score_kernel<false>, dim3((q.nh + 63) / 64, nchunks), dim3(64), 0, s, src, tgt, N,
                           q.nwg, r2, B);
        hipLaunchKernelGGL(ransac_round_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, N, q.nwg, nchunks, r, H, ransac_n,
                           confidence, B, dbg);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, src, tgt, N, r2, refit ? 1 : 0, B.st,
                       trans_f32, labels, result);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
