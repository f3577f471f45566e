// icp.hip -- f5: point-to-point ICP refinement of a predicted pose on the GPU,
// the "+ICP" stage every reference driver runs on the forward's final_trans
// through open3d (test.py:183-189, evaluation/benchmark_utils.py:40-56).
// open3d's RegistrationICP with TransformationEstimationPointToPoint(
// with_scaling=False) restated (open3d is not a dependency; parity with open3d
// itself is unpinned), the choices it leaves open fixed:
//
//   evaluate(T)   q = R p + t per source point in fp64; its correspondence is the
//                 nearest target point in fp64 d^2 with d^2 <= r^2 (ties: the
//                 lower target index), found in a uniform grid of r-sized cells
//                 over the target (build_grid, descriptors.hip) -- the query's
//                 cell coordinates are signed, a query one cell outside the
//                 target's box still meets the border cells
//   sums          17 fp64 quantities per 256-point source chunk (count, sum d^2,
//                 sum a, sum b, sum a b^T with a = q - c, b = target - c, c the
//                 target's centroid: no cancellation at KITTI-scale coordinates),
//                 reduced by wave shuffles and a small LDS stage, the chunks'
//                 rows summed in chunk order by one wave: no float atomics, a
//                 fixed order, so two runs are bitwise equal
//   solve         fitness / rmse of the T just evaluated, open3d's convergence
//                 test against the previous evaluation, else update =
//                 Kabsch(sums) (kabsch_rotation, fp64) and T <- update T
//
// T, the sums and the loop state stay on the device in fp64: the call enqueues
// 1 + max_iteration evaluate / solve pairs and every kernel returns at entry
// once the state's `done` word is set.  For Ns <= ICP_ONE_WG_MAX the whole loop
// runs in one launch of one workgroup instead (the same two device
// functions between __syncthreads, so the results are bitwise the same).
#include <cmath>
#include <cstdlib>

#include "abi.hpp"
#include "pdsc_common.hpp"
#include "chunk_sums.hpp"
#include "pdsc_internal.hpp"

namespace pdsc {

typedef unsigned long long u64;
constexpr int ICP_CHUNK = 256;       // source points per partial row (the fixed summation order)
constexpr int ICP_ONE_WG_MAX = 512;  // Ns up to which the loop runs in one workgroup (the measured crossover)
constexpr long long ICP_KEY_MAX = (1LL << GRID_KEY_BITS) - 1;
constexpr int ICP_NSUM = 17;  // count, sum d^2, sum a [3], sum b [3], sum a b^T [9]

struct IcpState {
    double T[16];          // the current transform, row-major
    double fitness, rmse;  // of the last evaluation
    int iterations, n_corr, done, pad;
};

PDSC_DEV u64 icp_key(long long ix, long long iy, long long iz) {
    return ((u64)ix << (2 * GRID_KEY_BITS)) | ((u64)iy << GRID_KEY_BITS) | (u64)iz;
}

PDSC_DEV int icp_lower_bound(const u64 *__restrict__ ukey, int nr, u64 k) {
    int lo = 0, hi = nr;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ukey[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

PDSC_DEV void icp_init_state(IcpState *st, const double *init) {
    for (int i = 0; i < 16; ++i) st->T[i] = init ? init[i] : (i % 5 == 0 ? 1.0 : 0.0);
    st->fitness = 0.0;
    st->rmse = 0.0;
    st->iterations = 0;
    st->n_corr = 0;
    st->done = 0;
    st->pad = 0;
}

// A source point's correspondence under T: q = R p + t in fp64 and the nearest
// target point with d^2 <= r2 (ties: the lower index), best = -1 without one.
// The 27 cells around the query are 9 (x, y) columns of up to 3 cells
// consecutive in key order: one binary search in ukey per column, then the
// occupied cells' runs.  Shared by evaluate (f5) and the information matrix (f11).
struct IcpHit {
    int best;
    double d2, qx, qy, qz, tx, ty, tz;  // d2 and the target point (fp64) where best >= 0
};
PDSC_DEV IcpHit icp_nearest(const float *__restrict__ src, int i, const float *__restrict__ tgt,
                            const CloudStats *__restrict__ gs, double cell, double r2, const GridView &g,
                            const double *T) {
    const double x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], z = src[3 * (size_t)i + 2];
    const double qx = (T[0] * x + T[1] * y) + T[2] * z + T[3];
    const double qy = (T[4] * x + T[5] * y) + T[6] * z + T[7];
    const double qz = (T[8] * x + T[9] * y) + T[10] * z + T[11];
    // signed cell coordinates (cell_of's formula, not clamped); NaN fails the range test
    const double fx = floor((qx - (double)gs->mn[0]) / cell), fy = floor((qy - (double)gs->mn[1]) / cell),
                 fz = floor((qz - (double)gs->mn[2]) / cell);
    const double top = (double)(ICP_KEY_MAX + 1);
    int best = -1;
    double bd = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    if (fx >= -1.0 && fx <= top && fy >= -1.0 && fy <= top && fz >= -1.0 && fz <= top) {
        const long long cx = (long long)fx, cy = (long long)fy, cz = (long long)fz;
        const long long z0 = cz > 0 ? cz - 1 : 0, z1 = cz < ICP_KEY_MAX ? cz + 1 : ICP_KEY_MAX;
        const int nr = *g.nruns;
        for (int c = 0; c < 9; ++c) {
            const long long ix = cx + c / 3 - 1, iy = cy + c % 3 - 1;
            if (ix < 0 || iy < 0 || ix > ICP_KEY_MAX || iy > ICP_KEY_MAX || z0 > z1) continue;
            const u64 khi = icp_key(ix, iy, z1);
            for (int u = icp_lower_bound(g.ukey, nr, icp_key(ix, iy, z0)); u < nr && g.ukey[u] <= khi; ++u) {
                const int s = g.ustart[u], m = g.ucount[u];
                for (int j = s; j < s + m; ++j) {
                    const int pi = g.sidx[j];
                    const double tx = tgt[3 * (size_t)pi], ty = tgt[3 * (size_t)pi + 1], tz = tgt[3 * (size_t)pi + 2];
                    const double dx = tx - qx, dy = ty - qy, dz = tz - qz;
                    const double d2 = dx * dx + dy * dy + dz * dz;
                    if (d2 <= r2 && (best < 0 || d2 < bd || (d2 == bd && pi < best))) {
                        best = pi;
                        bd = d2;
                        bx = tx;
                        by = ty;
                        bz = tz;
                    }
                }
            }
        }
    }
    return IcpHit{best, bd, qx, qy, qz, bx, by, bz};
}

// evaluate(T) for source chunk `chunk` (points 256 chunk + t, t = 0 .. 255, by
// the 256 threads that call this together with every other thread of the
// workgroup: it holds workgroup barriers).  red: the chunk's [4][17] LDS stage;
// the chunk's 17 sums go to part[17 chunk ..] (chunk < nchunks).
PDSC_DEV void icp_eval_chunk(const float *__restrict__ src, int Ns, const float *__restrict__ tgt,
                             const CloudStats *__restrict__ gs, double cell, double r2, const GridView &g,
                             const double *T, int chunk, int nchunks, int t, double *red, double *part,
                             int *__restrict__ corr) {
    const int i = chunk * ICP_CHUNK + t;
    double v[ICP_NSUM];
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) v[j] = 0.0;
    if (i < Ns) {
        const IcpHit h = icp_nearest(src, i, tgt, gs, cell, r2, g, T);
        if (corr) corr[i] = h.best;
        if (h.best >= 0) {
            const double c0 = gs->centroid[0], c1 = gs->centroid[1], c2 = gs->centroid[2];
            const double ax = h.qx - c0, ay = h.qy - c1, az = h.qz - c2;
            const double bx = h.tx - c0, by = h.ty - c1, bz = h.tz - c2;
            v[0] = 1.0;
            v[1] = h.d2;
            v[2] = ax;
            v[3] = ay;
            v[4] = az;
            v[5] = bx;
            v[6] = by;
            v[7] = bz;
            v[8] = ax * bx;
            v[9] = ax * by;
            v[10] = ax * bz;
            v[11] = ay * bx;
            v[12] = ay * by;
            v[13] = ay * bz;
            v[14] = az * bx;
            v[15] = az * by;
            v[16] = az * bz;
        }
    }
    icp_reduce_chunk<ICP_NSUM>(v, t, chunk, nchunks, red, part);
}

// One wave, after evaluation k (k = 0: of init): the chunks' rows summed in
// chunk order, fitness / rmse, open3d's convergence test against evaluation
// k - 1, and either the outputs (converged, or k == max_iter) or T <- update T.
// Every lane computes the same values; lane 0 stores.
PDSC_DEV void icp_solve(const double *part, int nchunks, int Ns, const CloudStats *__restrict__ gs, IcpState *st,
                        int k, int max_iter, double rel_fitness, double rel_rmse, pdsc_icp_result *res,
                        float *trans_f32, int lane) {
    double acc = 0.0;
    if (lane < ICP_NSUM)
        for (int c = 0; c < nchunks; ++c) acc += part[(size_t)c * ICP_NSUM + lane];
    double S[ICP_NSUM];
#pragma unroll
    for (int j = 0; j < ICP_NSUM; ++j) S[j] = __shfl(acc, j);
    const double n = S[0];
    const double fitness = n / (double)Ns, rmse = n > 0.0 ? sqrt(S[1] / n) : 0.0;
    const bool conv = k > 0 && fabs(st->fitness - fitness) < rel_fitness && fabs(st->rmse - rmse) < rel_rmse;
    const bool done = conv || k == max_iter;
    if (done) {
        if (lane == 0) {
            if (res) {
                for (int i = 0; i < 16; ++i) res->trans[i] = st->T[i];
                res->fitness = fitness;
                res->inlier_rmse = rmse;
                res->iterations = k;
                res->n_corr = (int)n;
            }
            if (trans_f32)
                for (int i = 0; i < 16; ++i) trans_f32[i] = (float)st->T[i];
        }
    } else if (n > 0.0) {  // n == 0: the identity update, T stays bit for bit
        const double inv = 1.0 / n;
        const double ma0 = S[2] * inv, ma1 = S[3] * inv, ma2 = S[4] * inv;
        const double mb0 = S[5] * inv, mb1 = S[6] * inv, mb2 = S[7] * inv;
        double H[9], R[9];
        H[0] = S[8] - S[2] * mb0;
        H[1] = S[9] - S[2] * mb1;
        H[2] = S[10] - S[2] * mb2;
        H[3] = S[11] - S[3] * mb0;
        H[4] = S[12] - S[3] * mb1;
        H[5] = S[13] - S[3] * mb2;
        H[6] = S[14] - S[4] * mb0;
        H[7] = S[15] - S[4] * mb1;
        H[8] = S[16] - S[4] * mb2;
        kabsch_rotation(H, R);
        const double c0 = gs->centroid[0], c1 = gs->centroid[1], c2 = gs->centroid[2];
        const double a0 = c0 + ma0, a1 = c1 + ma1, a2 = c2 + ma2;
        const double t0 = (c0 + mb0) - ((R[0] * a0 + R[1] * a1) + R[2] * a2);
        const double t1 = (c1 + mb1) - ((R[3] * a0 + R[4] * a1) + R[5] * a2);
        const double t2 = (c2 + mb2) - ((R[6] * a0 + R[7] * a1) + R[8] * a2);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // update T: rows 0 .. 2 (update's last row is 0 0 0 1)
                const double u0 = st->T[j], u1 = st->T[4 + j], u2 = st->T[8 + j], u3 = st->T[12 + j];
                st->T[j] = ((R[0] * u0 + R[1] * u1) + R[2] * u2) + t0 * u3;
                st->T[4 + j] = ((R[3] * u0 + R[4] * u1) + R[5] * u2) + t1 * u3;
                st->T[8 + j] = ((R[6] * u0 + R[7] * u1) + R[8] * u2) + t2 * u3;
            }
        }
    }
    if (lane == 0) {
        st->fitness = fitness;
        st->rmse = rmse;
        st->iterations = k;
        st->n_corr = (int)n;
        if (done) st->done = 1;
    }
}

// ------------------------------------------------------- the multi-launch path
__global__ void icp_init_kernel(IcpState *st, const double *init) {
    if (threadIdx.x == 0) icp_init_state(st, init);
}

__global__ __launch_bounds__(ICP_CHUNK) void icp_eval_kernel(const float *__restrict__ src, int Ns,
                                                             const float *__restrict__ tgt, const CloudStats *gs,
                                                             double cell, double r2, GridView g, const IcpState *st,
                                                             int nchunks, double *part, int *corr) {
    __shared__ double red[4 * ICP_NSUM];
    if (st->done) return;  // workgroup-uniform
    icp_eval_chunk(src, Ns, tgt, gs, cell, r2, g, st->T, blockIdx.x, nchunks, threadIdx.x, red, part, corr);
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const double *part, int nchunks, int Ns, const CloudStats *gs,
                                                       IcpState *st, int k, int max_iter, double rel_fitness,
                                                       double rel_rmse, pdsc_icp_result *res, float *trans_f32) {
    if (st->done) return;
    icp_solve(part, nchunks, Ns, gs, st, k, max_iter, rel_fitness, rel_rmse, res, trans_f32, threadIdx.x);
}

// ------------------------------------------------------ the one-workgroup path
// The whole loop in one launch: the workgroup evaluates ICP_WG / ICP_CHUNK chunks
// per pass (all of them at the present ICP_ONE_WG_MAX), wave 0 solves; state and
// the chunks' rows live in LDS.
constexpr int ICP_WG = ICP_ONE_WG_MAX < 1024 ? ICP_ONE_WG_MAX : 1024;
constexpr int ICP_WG_CHUNKS = ICP_ONE_WG_MAX / ICP_CHUNK;

__global__ __launch_bounds__(ICP_WG) void icp_one_wg_kernel(const float *__restrict__ src, int Ns,
                                                            const float *__restrict__ tgt, const CloudStats *gs,
                                                            double cell, double r2, GridView g, const double *init,
                                                            int max_iter, double rel_fitness, double rel_rmse,
                                                            pdsc_icp_result *res, float *trans_f32, int *corr) {
    __shared__ IcpState st;
    __shared__ double red[ICP_WG / 64 * ICP_NSUM];
    __shared__ double part[ICP_WG_CHUNKS * ICP_NSUM];
    const int tid = threadIdx.x, sub = tid / ICP_CHUNK, t = tid % ICP_CHUNK;
    const int nchunks = (Ns + ICP_CHUNK - 1) / ICP_CHUNK;
    if (tid == 0) icp_init_state(&st, init);
    __syncthreads();
    for (int k = 0; k <= max_iter; ++k) {
        for (int c0 = 0; c0 < nchunks; c0 += ICP_WG / ICP_CHUNK)
            icp_eval_chunk(src, Ns, tgt, gs, cell, r2, g, st.T, c0 + sub, nchunks, t, red + sub * 4 * ICP_NSUM, part,
                           corr);
        if (tid < 64) icp_solve(part, nchunks, Ns, gs, &st, k, max_iter, rel_fitness, rel_rmse, res, trans_f32, tid);
        __syncthreads();
        if (st.done) break;  // workgroup-uniform
    }
}

// ------------------------------------------- f11: the information matrix
// open3d's GetInformationMatrixFromPointClouds on evaluate(T)'s correspondences:
// per correspondence the target point (x, y, z) in fp64, not transformed, adds
// G^T G for G's rows (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1),
// which is 10 sums: the count, sum t, and the six entries of sum t t^T
// (INFO_NSUM and info_from_sums, chunk_sums.hpp: f13 builds its matrix from them too).
__global__ __launch_bounds__(ICP_CHUNK) void info_eval_kernel(const float *__restrict__ src, int Ns,
                                                              const float *__restrict__ tgt, const CloudStats *gs,
                                                              double cell, double r2, GridView g, const double *trans,
                                                              int nchunks, double *part, int *corr) {
    __shared__ double red[4 * INFO_NSUM];
    __shared__ double T[16];
    const int t = threadIdx.x;
    if (t < 16) T[t] = trans ? trans[t] : (t % 5 == 0 ? 1.0 : 0.0);
    __syncthreads();
    const int i = blockIdx.x * ICP_CHUNK + t;
    double v[INFO_NSUM];
#pragma unroll
    for (int j = 0; j < INFO_NSUM; ++j) v[j] = 0.0;
    if (i < Ns) {
        const IcpHit h = icp_nearest(src, i, tgt, gs, cell, r2, g, T);
        if (corr) corr[i] = h.best;
        if (h.best >= 0) {
            v[0] = 1.0;
            v[1] = h.tx;
            v[2] = h.ty;
            v[3] = h.tz;
            v[4] = h.tx * h.tx;
            v[5] = h.tx * h.ty;
            v[6] = h.tx * h.tz;
            v[7] = h.ty * h.ty;
            v[8] = h.ty * h.tz;
            v[9] = h.tz * h.tz;
        }
    }
    icp_reduce_chunk<INFO_NSUM>(v, t, blockIdx.x, nchunks, red, part);
}

// One wave: the chunks' rows summed in chunk order, then the 36 entries.
__global__ __launch_bounds__(64) void info_finish_kernel(const double *part, int nchunks,
                                                         pdsc_information_result *res) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    if (lane < INFO_NSUM)
        for (int c = 0; c < nchunks; ++c) acc += part[(size_t)c * INFO_NSUM + lane];
    double S[INFO_NSUM];
#pragma unroll
    for (int j = 0; j < INFO_NSUM; ++j) S[j] = __shfl(acc, j);
    if (lane != 0) return;
    info_from_sums(S, res->info);
    const double n = S[0];
    res->n_corr = (int)n;
    res->pad = 0;
}

// ------------------------------------------------------------------ launchers
static size_t icp_chunks(int Ns) { return ((size_t)Ns + ICP_CHUNK - 1) / ICP_CHUNK; }

// the target's grid, the state block and the partial rows [nchunks][ICP_NSUM]
struct IcpBufs {
    GridBufs grid;
    IcpState *st;
    double *part;
};
static void bind_icp(Carve &c, int Ns, int Nt, IcpBufs &I) {
    bind_grid(c, Nt, I.grid);
    I.st = c.take<IcpState>(1);
    I.part = c.take<double>(icp_chunks(Ns) * ICP_NSUM);
}

// PDSC_ICP_ONE_WG=0: the launch-per-step path at every size (not in Knobs: read at every call, tests toggle it)
static bool icp_one_wg() {
    const char *e = getenv("PDSC_ICP_ONE_WG");
    return !(e && e[0] == '0');
}

// f11's layout: the target's grid and the partial rows [nchunks][INFO_NSUM]
struct InfoBufs {
    GridBufs grid;
    double *part;
};
static void bind_info(Carve &c, int Ns, int Nt, InfoBufs &I) {
    bind_grid(c, Nt, I.grid);
    I.part = c.take<double>(icp_chunks(Ns) * INFO_NSUM);
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_icp_workspace_bytes(int32_t Ns, int32_t Nt) {
    if (Ns < 1 || Nt < 1) return 0;
    Carve c(nullptr);
    IcpBufs I;
    bind_icp(c, Ns, Nt, I);
    return c.off;
}

// Builds the target's grid and enqueues the loop: one workgroup where
// Ns <= ICP_ONE_WG_MAX (unless PDSC_ICP_ONE_WG=0), else a launch pair per step.
int32_t pdsc_icp_point_to_point(const float *source, int32_t Ns, const float *target, int32_t Nt,
                                const double *init_trans, double max_distance, int32_t max_iteration,
                                double relative_fitness, double relative_rmse, float *trans_f32,
                                pdsc_icp_result *result, int32_t *corr, void *ws, size_t ws_bytes,
                                pdsc_stream_t stream) {
    if (Ns < 1 || Nt < 1) return fail(PDSC_ERR_ARG, "Ns=%d Nt=%d (need >= 1)", Ns, Nt);
    if (!(max_distance > 0.0) || !std::isfinite(max_distance))
        return fail(PDSC_ERR_ARG, "max_distance %g must be > 0 and finite", max_distance);
    if (max_iteration < 0) return fail(PDSC_ERR_ARG, "max_iteration=%d", max_iteration);
    if (!source || !target || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_icp_workspace_bytes(Ns, Nt)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    IcpBufs I;
    bind_icp(c, Ns, Nt, I);
    const GridBufs &G = I.grid;
    HIPCHK(build_grid(target, Nt, max_distance, 0.0, G, s));
    const double r2 = max_distance * max_distance;
    const int nchunks = (int)icp_chunks(Ns);
    if (icp_one_wg() && Ns <= ICP_ONE_WG_MAX) {
        hipLaunchKernelGGL(icp_one_wg_kernel, dim3(1), dim3(ICP_WG), 0, s, source, Ns, target, G.st, max_distance, r2,
                           G.view, init_trans, max_iteration, relative_fitness, relative_rmse, result, trans_f32, corr);
    } else {
        hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, s, I.st, init_trans);
        for (int k = 0; k <= max_iteration; ++k) {
            hipLaunchKernelGGL(icp_eval_kernel, dim3(nchunks), dim3(ICP_CHUNK), 0, s, source, Ns, target, G.st,
                               max_distance, r2, G.view, I.st, nchunks, I.part, corr);
            hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(64), 0, s, I.part, nchunks, Ns, G.st, I.st, k,
                               max_iteration, relative_fitness, relative_rmse, result, trans_f32);
        }
    }
    HIPCHK(hipGetLastError());
    return grid_status(G, s);
}

size_t pdsc_information_matrix_workspace_bytes(int32_t Ns, int32_t Nt) {
    if (Ns < 1 || Nt < 1) return 0;
    Carve c(nullptr);
    InfoBufs I;
    bind_info(c, Ns, Nt, I);
    return c.off;
}

// Builds the target's grid (cell = max_distance, as f5), one lane per source point, one finishing wave.
int32_t pdsc_information_matrix(const float *source, int32_t Ns, const float *target, int32_t Nt, const double *trans,
                                double max_distance, pdsc_information_result *result, int32_t *corr, void *ws,
                                size_t ws_bytes, pdsc_stream_t stream) {
    if (Ns < 1 || Nt < 1) return fail(PDSC_ERR_ARG, "Ns=%d Nt=%d (need >= 1)", Ns, Nt);
    if (!(max_distance > 0.0) || !std::isfinite(max_distance))
        return fail(PDSC_ERR_ARG, "max_distance %g must be > 0 and finite", max_distance);
    if (!source || !target || !result || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_information_matrix_workspace_bytes(Ns, Nt)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    InfoBufs I;
    bind_info(c, Ns, Nt, I);
    const GridBufs &G = I.grid;
    HIPCHK(build_grid(target, Nt, max_distance, 0.0, G, s));
    const int nchunks = (int)icp_chunks(Ns);
    hipLaunchKernelGGL(info_eval_kernel, dim3(nchunks), dim3(ICP_CHUNK), 0, s, source, Ns, target, G.st, max_distance,
                       max_distance * max_distance, G.view, trans, nchunks, I.part, corr);
    hipLaunchKernelGGL(info_finish_kernel, dim3(1), dim3(64), 0, s, I.part, nchunks, result);
    HIPCHK(hipGetLastError());
    return grid_status(G, s);
}

}  // extern "C"
