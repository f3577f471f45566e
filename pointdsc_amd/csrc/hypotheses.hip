// hypotheses.hip -- a9-a11: hypothesis generation and verification, the best
// hypothesis and its post-refinement.
//
//   hypotheses   a9-a10  weighted Kabsch per seed (fp64 3x3 SVD on device) +
//                    inlier count over all N correspondences
//   select_best  a10 first argmax of fitness, labels of the best hypothesis
//   post_refine  a11 <= 20 device-side IRLS refits, one workgroup per pair
#include "abi.hpp"
#ifdef ATT_STAMPS
#include "att_stamps.hpp"  // the stamp buffer (BR_ST)
#endif
#include "launch_plan.hpp"
#include "nsm_weight.hpp"

namespace pdsc {

// ------------------------------------------------------------ a9 Kabsch
// Hypotheses (models/PointDSC.py:287-328) in three SIMD-friendly steps:
//  1. kabsch_sums   one wave per seed: weighted centroids and H (wave reductions)
//  2. kabsch_solve  one LANE per seed: fp64 3x3 rotation + t (64 solves per wave)
//  3. count_inliers one workgroup per HS seeds: every correspondence's residual
//                   under all HS hypotheses (src/tgt read once per HS seeds)
constexpr int HSUM = 15;  // H[9], cA[3], cB[3]
constexpr int HS = 8;     // seeds per count_inliers workgroup

PDSC_DEV void kabsch_finish(const float H[9], const float cA[3], const float cB[3], float *T);

// for (n = tid; n < N; n += NT) body(n, src row n, tgt row n) with RU rows'
// loads issued together: the pair's rows come from L2, and a loop that loads
// and consumes one row per trip waits a full round trip per row (r06 stamps of
// best_refine at N = 5000: 6.7 us per pass of 20 rows per thread).  body runs
// in the same n order, so sums accumulate in the same order: the same bits.
// A/B build knob: -DROWS_RU=1 consumes each row as it is loaded (measurement only)
#ifndef ROWS_RU
#define ROWS_RU 8
#endif
template <int NT, int RU = ROWS_RU, typename F>
PDSC_DEV void for_rows(const float *__restrict__ sb, const float *__restrict__ tb, int N, int tid, F body) {
    for (int n0 = tid; n0 < N; n0 += RU * NT) {
        float a[RU][3], c[RU][3];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int n = min(n0 + u * NT, N - 1);  // (clamped: an in-range row, not consumed)
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                a[u][e] = sb[3 * n + e];
                c[u][e] = tb[3 * n + e];
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u)
            if (n0 + u * NT < N) body(n0 + u * NT, a[u], c[u]);
    }
}

// SOLVE (small batches, TailPlan::kabsch_fused): lane 0 of the seed's wave also finishes
// the Kabsch solve (kabsch_finish on the same 15 sums kabsch_solve_kernel would
// read back: the same bits) and writes trans -- one launch instead of two.
// FIN (the testing forward): the seed's NSM weights are finished here, as
// nsm_finish_kernel computes them (nsm_tstar over the pair's seeds, nsm_weight;
// the same bits), and written to `weights` -- one launch fewer per forward.
// COUNT (with SOLVE, small batches): the seed's wave then counts the inliers of
// its own hypothesis over the pair's correspondences (count_inliers_kernel's
// test, residual_sq < tau2, the same integer) -- one launch fewer.
template <bool SOLVE, bool FIN = false, bool COUNT = false>
__global__ __launch_bounds__(256) void kabsch_sums_kernel(const float *__restrict__ src,
                                                          const float *__restrict__ tgt,
                                                          const int *__restrict__ knn,
                                                          const float *__restrict__ weights, int N,
                                                          int S, int k, float *__restrict__ sums, Ragged rg,
                                                          float *__restrict__ trans, const float *__restrict__ hist = nullptr,
                                                          const unsigned *__restrict__ seed_flags = nullptr, int T = 0,
                                                          float *__restrict__ wout = nullptr, float tau2 = 0.0f,
                                                          int *__restrict__ counts = nullptr) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int Sb = rg.s(b, S);
    if (s >= Sb) return;  // (N, S: the strides; knn entries lie below this pair's count)
    const float *sb = src + (size_t)b * N * 3, *tb = tgt + (size_t)b * N * 3;
    float w = 0, ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0;
    float wf = 0.0f;
    if constexpr (FIN) {
        const int tstar = nsm_tstar(seed_flags, (size_t)b * S, (size_t)Sb, T, lane);
        wf = nsm_weight(hist, (size_t)b * S + s, tstar, k, T, lane);
        if (lane < k) wout[((size_t)b * S + s) * k + lane] = wf;
    }
    if (lane < k) {
        const int j = min(max(knn[((size_t)b * S + s) * k + lane], 0), N - 1);
        w = FIN ? wf : weights[((size_t)b * S + s) * k + lane];
        ax = sb[3 * j];
        ay = sb[3 * j + 1];
        az = sb[3 * j + 2];
        bx = tb[3 * j];
        by = tb[3 * j + 1];
        bz = tb[3 * j + 2];
    }
    // centroid = sum(A * w) / (sum(w) + 1e-6)  (models/common.py:24-25)
    const float den = wave_sum(w) + 1e-6f;
    const float cA0 = wave_sum(ax * w) / den, cA1 = wave_sum(ay * w) / den, cA2 = wave_sum(az * w) / den;
    const float cB0 = wave_sum(bx * w) / den, cB1 = wave_sum(by * w) / den, cB2 = wave_sum(bz * w) / den;
    const float am[3] = {ax - cA0, ay - cA1, az - cA2};
    const float bm[3] = {bx - cB0, by - cB1, bz - cB2};
    float out = 0.0f;  // lane e < 15 keeps sums[e]
    float Hs[9];       // (every lane holds every wave sum)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const float h = wave_sum((am[i] * w) * bm[jj]);  // H = Am^T diag(w) Bm (:33)
            Hs[3 * i + jj] = h;
            if (lane == 3 * i + jj) out = h;
        }
    if constexpr (SOLVE) {
        float T[16];
        if (lane == 0) {
            const float cA[3] = {cA0, cA1, cA2}, cB[3] = {cB0, cB1, cB2};
            kabsch_finish(Hs, cA, cB, T);
#pragma unroll
            for (int e = 0; e < 16; ++e) trans[((size_t)b * S + s) * 16 + e] = T[e];
        }
        if constexpr (COUNT) {
            // lane 0's pose to every lane, then the pair's correspondences 64 at a time
            float Tb[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) Tb[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, T[e])));
            const int n = rg.n(b, N);
            int c = 0;
            for_rows<64>(sb, tb, n, lane, [&](int, const float (&p)[3], const float (&q)[3]) {
                c += residual_sq(Tb, p[0], p[1], p[2], q[0], q[1], q[2]) < tau2;  // L2 < tau (:327-328)
            });
            c = wave_sum(c);
            if (lane == 0) counts[(size_t)b * S + s] = c;
        }
        return;
    }
    if (lane == 9) out = cA0;
    if (lane == 10) out = cA1;
    if (lane == 11) out = cA2;
    if (lane == 12) out = cB0;
    if (lane == 13) out = cB1;
    if (lane == 14) out = cB2;
    if (lane < HSUM) sums[((size_t)b * S + s) * HSUM + lane] = out;
}

// Finish a weighted Kabsch from its sums: t = c_B - R c_A in fp32 as
// models/common.py:42 computes it; T row-major 4x4.
PDSC_DEV void kabsch_finish(const float H[9], const float cA[3], const float cB[3], float *T) {
    double Hd[9], Rd[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hd[i] = H[i];
    kabsch_rotation(Hd, Rd);
    float R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (float)Rd[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        T[4 * r + 0] = R[3 * r + 0];
        T[4 * r + 1] = R[3 * r + 1];
        T[4 * r + 2] = R[3 * r + 2];
        T[4 * r + 3] = cB[r] - ((R[3 * r] * cA[0] + R[3 * r + 1] * cA[1]) + R[3 * r + 2] * cA[2]);
    }
    T[12] = 0.0f;
    T[13] = 0.0f;
    T[14] = 0.0f;
    T[15] = 1.0f;
}

__global__ __launch_bounds__(64) void kabsch_solve_kernel(const float *__restrict__ sums, int n, int S,
                                                          float *__restrict__ trans, Ragged rg) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || i % S >= rg.s(i / S, S)) return;  // (a ragged pair's seeds end early)
    const float *p = sums + (size_t)i * HSUM;
    float H[9], cA[3], cB[3], T[16];
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = p[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        cA[e] = p[9 + e];
        cB[e] = p[12 + e];
    }
    kabsch_finish(H, cA, cB, T);
#pragma unroll
    for (int e = 0; e < 16; ++e) trans[(size_t)i * 16 + e] = T[e];
}

__global__ __launch_bounds__(256) void count_inliers_kernel(const float *__restrict__ src,
                                                            const float *__restrict__ tgt,
                                                            const float *__restrict__ seed_trans,
                                                            int Nstr, int S, float tau2,
                                                            int *__restrict__ counts, Ragged rg) {
    __shared__ float Ts[HS][12];
    __shared__ int wc[4][HS];
    const int b = blockIdx.y, s0 = blockIdx.x * HS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = rg.n(b, Nstr);  // this pair's correspondences; Nstr, S: the strides
    if (s0 >= rg.s(b, S)) return;  // workgroup-uniform
    const int ns = min(HS, rg.s(b, S) - s0);
    if (tid < HS * 12) {
        const int q = tid / 12, e = tid % 12;
        Ts[q][e] = (q < ns) ? seed_trans[((size_t)b * S + s0 + q) * 16 + e] : 0.0f;
    }
    __syncthreads();
    const float *sb = src + (size_t)b * Nstr * 3, *tb = tgt + (size_t)b * Nstr * 3;
    int c[HS];
#pragma unroll
    for (int q = 0; q < HS; ++q) c[q] = 0;
    for (int n = tid; n < N; n += 256) {
        const float x = sb[3 * n], y = sb[3 * n + 1], z = sb[3 * n + 2];
        const float tx = tb[3 * n], ty = tb[3 * n + 1], tz = tb[3 * n + 2];
#pragma unroll
        for (int q = 0; q < HS; ++q) c[q] += residual_sq(Ts[q], x, y, z, tx, ty, tz) < tau2;  // L2 < tau (:327-328)
    }
#pragma unroll
    for (int q = 0; q < HS; ++q) {
        const int v = wave_sum(c[q]);
        if (lane == 0) wc[wave][q] = v;
    }
    __syncthreads();
    if (tid < ns) counts[(size_t)b * S + s0 + tid] = wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
}

hipError_t launch_hypotheses(const TailPlan &tp, const float *src, const float *tgt, const int *knn,
                             const float *weights, int B, int N, int S, int k, float tau, float *seed_trans, int *counts,
                             float *sums, hipStream_t s, Ragged rg, const float *hist, const unsigned *seed_flags,
                             int T, float *wout) {
    const int wpb = tp.wpb;
    const int n = B * S;
    const dim3 grid((S + wpb - 1) / wpb, B), block(64 * wpb);
    const bool fin = hist != nullptr;
    const float tau2 = sqrt_ge_threshold(tau);
    if (tp.kabsch_fused) {
        // the inlier count in the same launch (count_inliers_kernel's integers)
        if (fin)
            hipLaunchKernelGGL((kabsch_sums_kernel<true, true, true>), grid, block, 0, s, src, tgt, knn, weights, N, S,
                               k, sums, rg, seed_trans, hist, seed_flags, T, wout, tau2, counts);
        else
            hipLaunchKernelGGL((kabsch_sums_kernel<true, false, true>), grid, block, 0, s, src, tgt, knn, weights, N, S,
                               k, sums, rg, seed_trans, nullptr, nullptr, 0, nullptr, tau2, counts);
        return hipGetLastError();
    } else {
        if (fin)
            hipLaunchKernelGGL((kabsch_sums_kernel<false, true>), grid, block, 0, s, src, tgt, knn, weights, N, S, k,
                               sums, rg, seed_trans, hist, seed_flags, T, wout);
        else
            hipLaunchKernelGGL((kabsch_sums_kernel<false>), grid, block, 0, s, src, tgt, knn, weights, N, S, k, sums,
                               rg, seed_trans, nullptr, nullptr, 0, nullptr);
        hipLaunchKernelGGL(kabsch_solve_kernel, dim3((n + 63) / 64), dim3(64), 0, s, sums, n, S, seed_trans, rg);
    }
    hipLaunchKernelGGL(count_inliers_kernel, dim3((S + HS - 1) / HS, B), dim3(256), 0, s, src, tgt,
                       seed_trans, N, S, tau2, counts, rg);
    return hipGetLastError();
}

// ------------------------------------------------------------- a10 best
// One 256-thread workgroup per pair: the range guard, the first argmax of the
// inlier counts, the best hypothesis into Ts (LDS) and trans, its labels.
// Returns false for a pair the range guard flagged (workgroup-uniform).
PDSC_DEV bool select_best_wg(const float *__restrict__ src, const float *__restrict__ tgt,
                             const float *__restrict__ seed_trans, const int *__restrict__ counts, int Nstr, int Sstr,
                             float tau, float *__restrict__ fitness, int *__restrict__ best_out,
                             float *__restrict__ trans, float *__restrict__ labels, const Ragged &rg,
                             const float *__restrict__ conf, int *__restrict__ range, int *wbest, int *wcnt, float *Ts) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = rg.n(b, Nstr), S = rg.s(b, Sstr);  // this pair's sizes; Nstr, Sstr: the strides
    if (conf) {
        // the fp16 range guard (pdsc.h, PDSC_ERR_RANGE): an activation that left
        // fp16's range in a 3xfp16 contraction turns into NaN (inf hi, -inf lo),
        // which the encoder's NaN-propagating ReLUs carry into every logit
        int bad = 0;
        const float *cb = conf + (size_t)b * Nstr;
        for (int n0 = tid; n0 < N; n0 += 8 * 256) {  // 8 loads in flight per thread
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = cb[min(n0 + 256 * u, N - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) bad |= !__builtin_isfinite(v[u]);
        }
        bad = __syncthreads_or(bad);
        if (range && tid == 0) range[b] = bad;
        if (bad) {
            if (tid < 16) trans[(size_t)b * 16 + tid] = __builtin_nanf("");
            for (int n = tid; n < Nstr; n += 256) labels[(size_t)b * Nstr + n] = 0.0f;
            return false;  // workgroup-uniform
        }
    }
    int bc = -1, bi = 0x7fffffff;
    for (int s = tid; s < S; s += 256) {
        const int c = counts[(size_t)b * Sstr + s];
        if (fitness) fitness[(size_t)b * Sstr + s] = (float)c / (float)N;  // torch.mean of 0/1
        if (c > bc) { bc = c; bi = s; }  // strided ascending s: first max kept
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o), oi = __shfl_xor(bi, o);
        if (oc > bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (lane == 0) { wcnt[wave] = bc; wbest[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        int c = wcnt[0], i = wbest[0];
        for (int w = 1; w < 4; ++w)
            if (wcnt[w] > c || (wcnt[w] == c && wbest[w] < i)) { c = wcnt[w]; i = wbest[w]; }
        wbest[0] = i;
        if (best_out) best_out[b] = i;
    }
    __syncthreads();
    const int best = wbest[0];
    if (tid < 16) {
        Ts[tid] = seed_trans[((size_t)b * Sstr + best) * 16 + tid];
        trans[(size_t)b * 16 + tid] = Ts[tid];
    }
    __syncthreads();
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = Ts[e];
    const float *sb = src + (size_t)b * Nstr * 3, *tb = tgt + (size_t)b * Nstr * 3;
    for_rows<256>(sb, tb, N, tid, [&](int n, const float (&a)[3], const float (&c)[3]) {
        const float L2 = residual(T, a[0], a[1], a[2], c[0], c[1], c[2]);
        labels[(size_t)b * Nstr + n] = (L2 < tau) ? 1.0f : 0.0f;
    });
    for (int n = N + tid; n < Nstr; n += 256) labels[(size_t)b * Nstr + n] = 0.0f;  // a ragged pair's padding
    return true;
}

__global__ __launch_bounds__(256) void select_best_kernel(const float *__restrict__ src,
                                                          const float *__restrict__ tgt,
                                                          const float *__restrict__ seed_trans,
                                                          const int *__restrict__ counts, int Nstr, int Sstr,
                                                          float tau, float *__restrict__ fitness,
                                                          int *__restrict__ best_out,
                                                          float *__restrict__ trans,
                                                          float *__restrict__ labels, Ragged rg,
                                                          const float *__restrict__ conf, int *__restrict__ range) {
    __shared__ int wbest[4], wcnt[4];
    __shared__ float Ts[16];
    select_best_wg(src, tgt, seed_trans, counts, Nstr, Sstr, tau, fitness, best_out, trans, labels, rg, conf, range,
                   wbest, wcnt, Ts);
}

hipError_t launch_select_best(const float *src, const float *tgt, const float *seed_trans,
                              const int *counts, int B, int N, int S, float tau, float *fitness,
                              int *best, float *trans, float *labels, hipStream_t s, Ragged rg, const float *conf,
                              int *range) {
    hipLaunchKernelGGL(select_best_kernel, dim3(B), dim3(256), 0, s, src, tgt, seed_trans, counts, N, S,
                       tau, fitness, best, trans, labels, rg, conf, range);
    return hipGetLastError();
}

// --------------------------------------------------- block-wide Kabsch
constexpr int RB = 256;  // threads per refinement / rigid workgroup (register room for the fp64 SVD)
constexpr int RW = RB / 64;

template <int NV>
PDSC_DEV void block_sum(float (&v)[NV], float (*red)[NV], int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave][i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float a = 0.0f;
        for (int w = 0; w < RW; ++w) a += red[w][i];
        v[i] = a;
    }
    __syncthreads();
}

template <typename WF>
PDSC_DEV void block_rigid_h(const float *__restrict__ A, const float *__restrict__ Bp, int n, WF wfun,
                            const float (&s7)[7], float *Tout, float (*red)[9], int tid);

// rigid_transform_3d on (A, B, w) rows [0, n) (models/common.py:7-45).
// wfun(i) returns the weight of row i (0 drops it).
template <typename WF>
PDSC_DEV void block_rigid(const float *__restrict__ A, const float *__restrict__ Bp, int n, WF wfun,
                          float *Tout, float (*red)[9], int tid) {
    float s7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += RB) {
        const float w = wfun(i);
        s7[0] += w;
        s7[1] += A[3 * i] * w;
        s7[2] += A[3 * i + 1] * w;
        s7[3] += A[3 * i + 2] * w;
        s7[4] += Bp[3 * i] * w;
        s7[5] += Bp[3 * i + 1] * w;
        s7[6] += Bp[3 * i + 2] * w;
    }
    block_sum<7>(s7, reinterpret_cast<float (*)[7]>(red), tid);
    block_rigid_h(A, Bp, n, wfun, s7, Tout, red, tid);
}

// block_rigid's second half: the centroids from the block-summed weight and
// weighted coordinate sums s7 = (sum w, sum w A, sum w B), then H and the solve.
template <typename WF>
PDSC_DEV void block_rigid_h(const float *__restrict__ A, const float *__restrict__ Bp, int n, WF wfun,
                            const float (&s7)[7], float *Tout, float (*red)[9], int tid) {
    const float den = s7[0] + 1e-6f;
    const float cA[3] = {s7[1] / den, s7[2] / den, s7[3] / den};
    const float cB[3] = {s7[4] / den, s7[5] / den, s7[6] / den};
    float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += RB) {
        const float w = wfun(i);
        if (w == 0.0f) continue;
        const float am[3] = {A[3 * i] - cA[0], A[3 * i + 1] - cA[1], A[3 * i + 2] - cA[2]};
        const float bm[3] = {Bp[3 * i] - cB[0], Bp[3 * i + 1] - cB[1], Bp[3 * i + 2] - cB[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[3 * r + c] += (am[r] * w) * bm[c];
    }
    block_sum<9>(H, red, tid);
    if (tid == 0) kabsch_finish(H, cA, cB, Tout);
    __syncthreads();
}

// ---------------------------------------------------- a11 post-refinement
// Diagnostic build only (-DATT_STAMPS, tools/refine_stamps.py): pair 0's
// workgroup stamps s_memrealtime into the stamp buffer's last wave slot at the
// refinement's phase ends (BR_ST(i): 0 start, 1 select done, 2 + 3 it + {0, 1,
// 2}: iteration it's count pass, H pass, solve; 98 the iterations run, 99 end).
#ifdef ATT_STAMPS
#define BR_ST(i)                                                                                         \
    do {                                                                                                 \
        if (blockIdx.x == 0 && threadIdx.x == 0 && (i) < ST_PER_WAVE)                                   \
            g_att_stamps[(ST_WGS * 4 - 1) * ST_PER_WAVE + (i)] = __builtin_amdgcn_s_memrealtime();        \
    } while (0)
#else
#define BR_ST(i) \
    do {         \
    } while (0)
#endif
// The refinement of pair blockIdx.x from the pose in Ts (LDS, every thread's
// view current), written to trans[b] at the end.
PDSC_DEV void post_refine_wg(float *Ts, float *__restrict__ trans, const float *__restrict__ src,
                             const float *__restrict__ tgt, int Nstr, float thr, const Ragged &rg, float (*red)[9]) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = rg.n(b, Nstr);  // this pair's correspondences; Nstr: the stride
    const float *sb = src + (size_t)b * Nstr * 3, *tb = tgt + (size_t)b * Nstr * 3;
    int prev = 0;
    for (int it = 0; it < 20; ++it) {
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = Ts[e];
        auto weight = [&](const float (&pa)[3], const float (&pb)[3]) -> float {
            const float L2 = residual(T, pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]);
            const float r = L2 / thr;
            const float wv = 1.0f / (1.0f + r * r);  // 1/(1 + (L2/thr)^2) (:435)
            return L2 < thr ? wv : 0.0f;
        };
        // one pass: the inlier count (:423-426) and block_rigid's weighted sums of
        // the same T (the next iterate's weights), in block_rigid's order
        float c8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for_rows<RB>(sb, tb, N, tid, [&](int, const float (&pa)[3], const float (&pb)[3]) {
            const float ax = pa[0], ay = pa[1], az = pa[2];
            const float bx = pb[0], by = pb[1], bz = pb[2];
            const float L2 = residual(T, ax, ay, az, bx, by, bz);
            // branch-free (the weight evaluated for every row, kept where L2 < thr):
            // the rows of a trip are independent chains the scheduler interleaves
            const bool in = L2 < thr;
            const float r = L2 / thr;
            const float wv = 1.0f / (1.0f + r * r);
            const float w = in ? wv : 0.0f;
            c8[7] += in ? 1.0f : 0.0f;
            c8[0] += w;
            c8[1] += ax * w;
            c8[2] += ay * w;
            c8[3] += az * w;
            c8[4] += bx * w;
            c8[5] += by * w;
            c8[6] += bz * w;
        });
        block_sum<8>(c8, reinterpret_cast<float (*)[8]>(red), tid);
        BR_ST(2 + 3 * it);
#ifdef ATT_STAMPS
        if (blockIdx.x == 0 && tid == 0) g_att_stamps[(ST_WGS * 4 - 1) * ST_PER_WAVE + 98] = it + 1;
#endif
        const int cnt = (int)c8[7];
        if (cnt == prev) break;  // abs(int(inlier_num - previous_inlier_num)) < 1 (:426)
        prev = cnt;
        const float s7[7] = {c8[0], c8[1], c8[2], c8[3], c8[4], c8[5], c8[6]};
        float Tn[16];
        {   // block_rigid_h(sb, tb, N, wfun, s7, Tn, red, tid) with the rows loaded RU at a time
            const float den = s7[0] + 1e-6f;
            const float cA[3] = {s7[1] / den, s7[2] / den, s7[3] / den};
            const float cB[3] = {s7[4] / den, s7[5] / den, s7[6] / den};
            float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for_rows<RB>(sb, tb, N, tid, [&](int, const float (&pa)[3], const float (&pb)[3]) {
                // a zero weight adds (am 0) bm = +-0 to H, which leaves it as skipping the
                // row did (H starts at +0 and x + -0 = x, +0 + -0 = +0): branch-free
                const float w = weight(pa, pb);
                const float am[3] = {pa[0] - cA[0], pa[1] - cA[1], pa[2] - cA[2]};
                const float bm[3] = {pb[0] - cB[0], pb[1] - cB[1], pb[2] - cB[2]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) H[3 * r + c] += (am[r] * w) * bm[c];
            });
            block_sum<9>(H, red, tid);
            BR_ST(3 + 3 * it);
            if (tid == 0) kabsch_finish(H, cA, cB, Tn);
            __syncthreads();
        }
        if (tid == 0)
            for (int e = 0; e < 16; ++e) Ts[e] = Tn[e];
        __syncthreads();
        BR_ST(4 + 3 * it);
    }
    BR_ST(99);
    if (tid < 16) trans[(size_t)b * 16 + tid] = Ts[tid];
}

__global__ __launch_bounds__(RB) void post_refine_kernel(float *__restrict__ trans,
                                                         const float *__restrict__ src,
                                                         const float *__restrict__ tgt, int Nstr,
                                                         float thr, Ragged rg, const int *__restrict__ range) {
    __shared__ float red[RW][9];
    __shared__ float Ts[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (range && range[b]) return;  // a pair the range guard flagged keeps its NaN pose (workgroup-uniform)
    if (tid < 16) Ts[tid] = trans[(size_t)b * 16 + tid];
    __syncthreads();
    post_refine_wg(Ts, trans, src, tgt, Nstr, thr, rg, red);
}

// select_best + post_refine of one pair in one launch (the testing forward):
// the same two workgroup bodies back to back, the best pose handed over in LDS.
static_assert(RB == 256, "select_best_wg runs 256 threads");
__global__ __launch_bounds__(RB) void best_refine_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                         const float *__restrict__ seed_trans,
                                                         const int *__restrict__ counts, int Nstr, int Sstr,
                                                         float tau, float thr, float *__restrict__ trans,
                                                         float *__restrict__ labels, Ragged rg,
                                                         const float *__restrict__ conf, int *__restrict__ range) {
    __shared__ int wbest[4], wcnt[4];
    __shared__ float Ts[16];
    __shared__ float red[RW][9];
    BR_ST(0);
    if (!select_best_wg(src, tgt, seed_trans, counts, Nstr, Sstr, tau, nullptr, nullptr, trans, labels, rg, conf, range,
                        wbest, wcnt, Ts))
        return;  // (workgroup-uniform) the range guard's NaN pose stays
    BR_ST(1);
    post_refine_wg(Ts, trans, src, tgt, Nstr, thr, rg, red);
}

hipError_t launch_best_refine(const float *src, const float *tgt, const float *seed_trans, const int *counts, int B,
                              int N, int S, float tau, float thr, float *trans, float *labels, hipStream_t s,
                              Ragged rg, const float *conf, int *range) {
    hipLaunchKernelGGL(best_refine_kernel, dim3(B), dim3(RB), 0, s, src, tgt, seed_trans, counts, N, S, tau, thr, trans,
                       labels, rg, conf, range);
    return hipGetLastError();
}

hipError_t launch_post_refine(float *trans, const float *src, const float *tgt, int B, int N, float thr,
                              hipStream_t s, Ragged rg, const int *range) {
    hipLaunchKernelGGL(post_refine_kernel, dim3(B), dim3(RB), 0, s, trans, src, tgt, N, thr, rg, range);
    return hipGetLastError();
}

__global__ __launch_bounds__(RB) void rigid_kernel(const float *__restrict__ A, const float *__restrict__ Bp,
                                                   const float *__restrict__ w, int n,
                                                   float *__restrict__ trans) {
    __shared__ float red[RW][9];
    __shared__ float Ts[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *Ab = A + (size_t)b * n * 3, *Bb = Bp + (size_t)b * n * 3;
    const float *wb = w ? w + (size_t)b * n : nullptr;
    auto wfun = [&](int i) -> float {
        if (!wb) return 1.0f;
        const float x = wb[i];
        return x < 0.0f ? 0.0f : x;  // weights[weights < weight_threshold(=0)] = 0 (:20)
    };
    float T[16];
    block_rigid(Ab, Bb, n, wfun, T, red, tid);
    if (tid == 0)
        for (int e = 0; e < 16; ++e) Ts[e] = T[e];
    __syncthreads();
    if (tid < 16) trans[(size_t)b * 16 + tid] = Ts[tid];
}

hipError_t launch_rigid(const float *A, const float *Bp, const float *w, int nb, int n, float *trans,
                        hipStream_t s) {
    hipLaunchKernelGGL(rigid_kernel, dim3(nb), dim3(RB), 0, s, A, Bp, w, n, trans);
    return hipGetLastError();
}

#ifdef ATT_STAMPS
// BR_ST's stamps (this file's copy of the stamp buffer; tools/refine_stamps.py)
extern "C" int pdsc_diag_refine_stamps(void *host, size_t bytes) {
    const size_t n = std::min(bytes, sizeof(g_att_stamps));
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_att_stamps), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int pdsc_diag_refine_stamps_clear() {
    static unsigned long long zero[ST_WGS * 4 * ST_PER_WAVE];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_att_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice) == hipSuccess ? 0
                                                                                                             : -1;
}
#endif

static float *bind_hypothesis_sums(Carve &c, int B, int S) { return c.take<float>((size_t)B * S * 15); }

}  // namespace pdsc

using namespace pdsc;

extern "C" {

// -------------------------------------------------------------------- a9
int32_t pdsc_rigid_transform_3d(const float *A, const float *Bp, const float *w, int32_t nb, int32_t n,
                                float *trans, pdsc_stream_t stream) {
    if (!A || !Bp || !trans) return fail(PDSC_ERR_ARG, "null pointer");
    if (nb < 1 || n < 0) return fail(PDSC_ERR_ARG, "nb=%d n=%d", nb, n);
    HIPCHK(launch_rigid(A, Bp, w, nb, n, trans, S_(stream)));
    return PDSC_OK;
}

// ------------------------------------------------------------------- a10
size_t pdsc_seed_hypotheses_workspace_bytes(int32_t B, int32_t S) {
    Carve c(nullptr);
    bind_hypothesis_sums(c, B, S);
    return c.off;
}

int32_t pdsc_seed_hypotheses(const float *src, const float *tgt, const int32_t *knn, const float *weights,
                             int32_t B, int32_t N, int32_t S, int32_t k, float tau, float *seed_trans,
                             float *fitness, int32_t *best, float *trans, float *labels, void *ws,
                             size_t ws_bytes, pdsc_stream_t stream) {
    if (!src || !tgt || !knn || !weights || !trans || !labels || !seed_trans)
        return fail(PDSC_ERR_ARG, "null pointer (seed_trans is required as scratch)");
    if (B < 1 || S < 1 || k < 1 || k > 63 || N < k + 1)
        return fail(PDSC_ERR_ARG, "B=%d N=%d S=%d k=%d (1 <= k <= min(63, N-1))", B, N, S, k);
    hipStream_t s = S_(stream);
    // the integer inlier counts live in the caller's fitness buffer until select_best turns
    // each into count / N (same thread, same element)
    if (!fitness) return fail(PDSC_ERR_ARG, "fitness [B,S] buffer is required (hosts the inlier counts)");
    int *counts = reinterpret_cast<int *>(fitness);
    if (!ws || ws_bytes < pdsc_seed_hypotheses_workspace_bytes(B, S))
        return fail(PDSC_ERR_ARG, "workspace too small");
    Carve c(ws);
    HIPCHK(launch_hypotheses(plan_tail(B, N, S), src, tgt, knn, weights, B, N, S, k, tau, seed_trans, counts,
                             bind_hypothesis_sums(c, B, S), s));
    HIPCHK(launch_select_best(src, tgt, seed_trans, counts, B, N, S, tau, fitness, best, trans, labels, s));
    return PDSC_OK;
}

// ------------------------------------------------------------------- a11
int32_t pdsc_post_refine(float *trans, const float *src, const float *tgt, int32_t B, int32_t N, float thr,
                         pdsc_stream_t stream) {
    if (!trans || !src || !tgt) return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || N < 1) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    HIPCHK(launch_post_refine(trans, src, tgt, B, N, thr, S_(stream)));
    return PDSC_OK;
}

}  // extern "C"
