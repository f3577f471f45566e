// rgbd_odometry.hip -- f13: RGB-D odometry with the hybrid term, batched over
// frame pairs: step 1 of the fork's multiway experiment (multiway/
// make_fragments.py:58-61 calls open3d's compute_rgbd_odometry with
// RGBDOdometryJacobianFromHybridTerm on every adjacent frame pair).  open3d
// 0.10's Odometry.cpp restated; the contract is in include/pdsc.h.
//
//   frames   once per call and shared by all pairs: clip + 3x3 Gaussian at level
//            0, two 2x2 downsamples, Sobel dx / dy of intensity and depth per
//            level -- 6 fp32 images per level and frame in the workspace; xyz is
//            recomputed from the depth where it is read
//   a pair   is blockIdx.y of every per-iteration kernel.  Its transform, its two
//            intensity scales and its loop state stay on the device in fp64
//            (OdoState); a kernel returns at entry once the pair is done, so the
//            call enqueues all 35 iterations with no host synchronisation
//   one iteration = 3 launches:
//     odo_corr_kernel   a lane per source pixel, one 64-bit atomicMin per accepted
//                       pixel on key[target pixel] = (fp32 bits of p.z, source index)
//     odo_lin_kernel    a lane per target pixel: the winner's two Jacobian rows,
//                       28 fp64 sums per 256-pixel chunk (chunk_sums.hpp); it
//                       resets the key it read, so the map is empty again
//     odo_solve_kernel  one wave per pair: the chunks' rows in order, 6x6
//                       Cholesky, T <- Exp(x) T (se3.hpp)
#include <cmath>

#include "abi.hpp"
#include "chunk_sums.hpp"
#include "pdsc_common.hpp"
#include "se3.hpp"

namespace pdsc {

typedef unsigned long long u64;
constexpr int ODO_LEVELS = 3;
constexpr int ODO_CHUNK = 256;  // pixels per partial row (the fixed summation order)
constexpr int ODO_NSUM = 28;    // J^T J upper triangle [21], J^T r [6], the count
constexpr int ODO_NNORM = 3;    // the count, sum I_s, sum I_t
constexpr u64 ODO_EMPTY = ~0ull;
constexpr int ODO_MAX_GRID_Y = 65535;
constexpr long long ODO_MAX_PIXELS = 1LL << 26;  // per frame: pixel indices, H W and the grids stay far inside an int
constexpr double ODO_LAMBDA_DEP = 0.968;
constexpr double ODO_SOBEL_SCALE = 0.125;

struct OdoLevel {  // one pyramid level of all F frames: [F][H][W] each
    float *I, *D, *Idx, *Idy, *Ddx, *Ddy;
    int H, W;
    double fx, fy, cx, cy;
};
struct OdoState {
    double T[16];
    double a_s, a_t;  // the pair's intensity scales
    int done, failed, n_corr, iters;
};

// ------------------------------------------------------------ frames, once
PDSC_DEV int clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }
PDSC_DEV float odo_clip(float d, float mn, float mx) { return (d < mn || d > mx || d <= 0.0f) ? NAN : d; }
PDSC_DEV float tap3(float a, float b, float c) { return (0.25f * a + 0.5f * b) + 0.25f * c; }

// separable [1/4, 1/2, 1/4] at (u, v) with clamped reads: the three rows'
// horizontal values in fp32, then the vertical pass over them
template <bool CLIP>
PDSC_DEV float gauss3(const float *__restrict__ img, int H, int W, int u, int v, float mn, float mx) {
    float h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float *row = img + (size_t)clampi(v + r - 1, H - 1) * W;
        float a = row[clampi(u - 1, W - 1)], b = row[u], c = row[clampi(u + 1, W - 1)];
        if (CLIP) {
            a = odo_clip(a, mn, mx);
            b = odo_clip(b, mn, mx);
            c = odo_clip(c, mn, mx);
        }
        h[r] = tap3(a, b, c);
    }
    return tap3(h[0], h[1], h[2]);
}

__global__ __launch_bounds__(256) void odo_prep0_kernel(const float *__restrict__ intensity,
                                                        const float *__restrict__ depth, int H, int W, float mn,
                                                        float mx, float *__restrict__ I0, float *__restrict__ D0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const size_t f = (size_t)blockIdx.y * H * W;
    const int u = i % W, v = i / W;
    I0[f + i] = gauss3<false>(intensity + f, H, W, u, v, 0.0f, 0.0f);
    D0[f + i] = gauss3<true>(depth + f, H, W, u, v, mn, mx);
}

// level l from level l - 1 (Hp x Wp): intensity filtered again, depth not; 2x2 means
__global__ __launch_bounds__(256) void odo_down_kernel(const float *__restrict__ Ip, const float *__restrict__ Dp,
                                                       int Hp, int Wp, float *__restrict__ I, float *__restrict__ D) {
    const int H = Hp / 2, W = Wp / 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const size_t fp = (size_t)blockIdx.y * Hp * Wp, f = (size_t)blockIdx.y * H * W;
    const int u = i % W, v = i / W;
    const float g00 = gauss3<false>(Ip + fp, Hp, Wp, 2 * u, 2 * v, 0.0f, 0.0f);
    const float g01 = gauss3<false>(Ip + fp, Hp, Wp, 2 * u + 1, 2 * v, 0.0f, 0.0f);
    const float g10 = gauss3<false>(Ip + fp, Hp, Wp, 2 * u, 2 * v + 1, 0.0f, 0.0f);
    const float g11 = gauss3<false>(Ip + fp, Hp, Wp, 2 * u + 1, 2 * v + 1, 0.0f, 0.0f);
    I[f + i] = (((g00 + g01) + g10) + g11) * 0.25f;
    const float *d0 = Dp + fp + (size_t)(2 * v) * Wp + 2 * u, *d1 = d0 + Wp;
    D[f + i] = (((d0[0] + d0[1]) + d1[0]) + d1[1]) * 0.25f;
}

// Sobel 3x3 with clamped reads: dx = (h(v-1) + 2 h(v)) + h(v+1), h = img(u+1) - img(u-1); dy transposed
PDSC_DEV void sobel3(const float *__restrict__ img, int H, int W, int u, int v, float &dx, float &dy) {
    const int um = clampi(u - 1, W - 1), up = clampi(u + 1, W - 1);
    const float *r0 = img + (size_t)clampi(v - 1, H - 1) * W, *r1 = img + (size_t)v * W,
                *r2 = img + (size_t)clampi(v + 1, H - 1) * W;
    dx = ((r0[up] - r0[um]) + 2.0f * (r1[up] - r1[um])) + (r2[up] - r2[um]);
    dy = ((r2[um] - r0[um]) + 2.0f * (r2[u] - r0[u])) + (r2[up] - r0[up]);
}

__global__ __launch_bounds__(256) void odo_sobel_kernel(OdoLevel L) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.H * L.W) return;
    const size_t f = (size_t)blockIdx.y * L.H * L.W;
    const int u = i % L.W, v = i / L.W;
    float dx, dy;
    sobel3(L.I + f, L.H, L.W, u, v, dx, dy);
    L.Idx[f + i] = dx;
    L.Idy[f + i] = dy;
    sobel3(L.D + f, L.H, L.W, u, v, dx, dy);
    L.Ddx[f + i] = dx;
    L.Ddy[f + i] = dy;
}

// ------------------------------------------------------------ a pair's state
__global__ void odo_init_kernel(OdoState *st, const double *init, int P) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    OdoState &s = st[p];
    for (int i = 0; i < 16; ++i) s.T[i] = init ? init[16 * (size_t)p + i] : (i % 5 == 0 ? 1.0 : 0.0);
    s.a_s = 1.0;
    s.a_t = 1.0;
    s.done = 0;
    s.failed = 0;
    s.n_corr = 0;
    s.iters = 0;
}

__global__ void odo_fill_keys_kernel(u64 *keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ODO_EMPTY;
}

// Source pixel i of frame Ds under T: p = R X_s + t, its target pixel, and the
// acceptance test against the target's depth.
struct OdoProj {
    double px, py, pz, dt;
    int j;  // target pixel index
};
PDSC_DEV bool odo_project(const OdoLevel &L, const float *__restrict__ Ds, const float *__restrict__ Dt,
                          const double (&T)[12], int i, double max_depth_diff, OdoProj &o) {
    const float d = Ds[i];
    if (!isfinite(d)) return false;
    const int us = i % L.W, vs = i / L.W;
    const double X = (((double)us - L.cx) * (double)d) / L.fx, Y = (((double)vs - L.cy) * (double)d) / L.fy;
    aff_apply(T, X, Y, (double)d, o.px, o.py, o.pz);
    if (!(o.pz > 0.0)) return false;
    const double uf = (L.fx * o.px) / o.pz + L.cx + 0.5, vf = (L.fy * o.py) / o.pz + L.cy + 0.5;
    if (!(uf > -1.0 && uf < (double)L.W && vf > -1.0 && vf < (double)L.H)) return false;  // int() truncates toward 0
    o.j = (int)vf * L.W + (int)uf;
    const float dt = Dt[o.j];
    if (!isfinite(dt)) return false;
    o.dt = (double)dt;
    return fabs(o.pz - o.dt) <= max_depth_diff;
}

__global__ __launch_bounds__(ODO_CHUNK) void odo_corr_kernel(OdoLevel L, const int *__restrict__ pair_src,
                                                             const int *__restrict__ pair_tgt,
                                                             const OdoState *__restrict__ st, double max_depth_diff,
                                                             int honour_done, u64 *__restrict__ keys, size_t key_stride) {
    const int p = blockIdx.y;
    if (honour_done && st[p].done) return;
    const int i = blockIdx.x * ODO_CHUNK + threadIdx.x, HW = L.H * L.W;
    if (i >= HW) return;
    double T[12];
    aff_load(st[p].T, T);
    OdoProj o;
    if (!odo_project(L, L.D + (size_t)pair_src[p] * HW, L.D + (size_t)pair_tgt[p] * HW, T, i, max_depth_diff, o)) return;
    const u64 key = ((u64)__float_as_uint((float)o.pz) << 32) | (u64)(unsigned)i;
    atomicMin(keys + (size_t)p * key_stride + o.j, key);
}

// The winner of target pixel j (or -1), its key reset; recomputes the winner's projection.
PDSC_DEV int odo_take(const OdoLevel &L, const float *Ds, const float *Dt, const double (&T)[12], int j, int HW,
                      double max_depth_diff, u64 *keys, OdoProj &o) {
    if (j >= HW) return -1;
    const u64 k = keys[j];
    if (k == ODO_EMPTY) return -1;
    keys[j] = ODO_EMPTY;
    const int i = (int)(k & 0xffffffffu);
    odo_project(L, Ds, Dt, T, i, max_depth_diff, o);
    return i;
}

// step 2: the sums behind a_s and a_t, over the level-0 correspondences
__global__ __launch_bounds__(ODO_CHUNK) void odo_norm_kernel(OdoLevel L, const int *__restrict__ pair_src,
                                                             const int *__restrict__ pair_tgt,
                                                             const OdoState *__restrict__ st, double max_depth_diff,
                                                             u64 *__restrict__ keys, size_t key_stride, int nchunks,
                                                             double *__restrict__ part, size_t part_stride) {
    __shared__ double red[4 * ODO_NNORM];
    const int p = blockIdx.y, t = threadIdx.x, HW = L.H * L.W, j = blockIdx.x * ODO_CHUNK + t;
    const size_t fs = (size_t)pair_src[p] * HW, ft = (size_t)pair_tgt[p] * HW;
    double T[12];
    aff_load(st[p].T, T);
    double v[ODO_NNORM] = {0.0, 0.0, 0.0};
    OdoProj o;
    const int i = odo_take(L, L.D + fs, L.D + ft, T, j, HW, max_depth_diff, keys + (size_t)p * key_stride, o);
    if (i >= 0) {
        v[0] = 1.0;
        v[1] = (double)L.I[fs + i];
        v[2] = (double)L.I[ft + j];
    }
    icp_reduce_chunk<ODO_NNORM>(v, t, blockIdx.x, nchunks, red, part + (size_t)p * part_stride);
}

__global__ __launch_bounds__(64) void odo_norm_finish_kernel(const double *__restrict__ part, size_t part_stride,
                                                             int nchunks, OdoState *st, double *scales) {
    const int p = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    if (lane < ODO_NNORM)
        for (int c = 0; c < nchunks; ++c) acc += part[(size_t)p * part_stride + (size_t)c * ODO_NNORM + lane];
    const double n = __shfl(acc, 0), ss = __shfl(acc, 1), stt = __shfl(acc, 2);
    if (lane == 0) {
        st[p].a_s = n > 0.0 ? 0.5 / (ss / n) : 1.0;
        st[p].a_t = n > 0.0 ? 0.5 / (stt / n) : 1.0;
        if (scales) {
            scales[2 * p] = st[p].a_s;
            scales[2 * p + 1] = st[p].a_t;
        }
    }
}

PDSC_DEV double nan0(float g) { return isnan(g) ? 0.0 : (double)g; }

// step 4 and 5: the two rows of every correspondence and the chunk's 28 sums
__global__ __launch_bounds__(ODO_CHUNK) void odo_lin_kernel(OdoLevel L, const int *__restrict__ pair_src,
                                                            const int *__restrict__ pair_tgt,
                                                            const OdoState *__restrict__ st, double max_depth_diff,
                                                            int honour_done, u64 *__restrict__ keys, size_t key_stride,
                                                            int nchunks, double *__restrict__ part, size_t part_stride,
                                                            int *__restrict__ corr) {
    __shared__ double red[4 * ODO_NSUM];
    const int p = blockIdx.y;
    if (honour_done && st[p].done) return;  // workgroup-uniform
    const int t = threadIdx.x, HW = L.H * L.W, j = blockIdx.x * ODO_CHUNK + t;
    const size_t fs = (size_t)pair_src[p] * HW, ft = (size_t)pair_tgt[p] * HW;
    double T[12];
    aff_load(st[p].T, T);
    double v[ODO_NSUM];
#pragma unroll
    for (int k = 0; k < ODO_NSUM; ++k) v[k] = 0.0;
    OdoProj o;
    const int i = odo_take(L, L.D + fs, L.D + ft, T, j, HW, max_depth_diff, keys + (size_t)p * key_stride, o);
    if (corr && j < HW) corr[(size_t)p * HW + j] = i;
    if (i >= 0) {
        const double a_s = st[p].a_s, a_t = st[p].a_t;
        const double sq_i = sqrt(1.0 - ODO_LAMBDA_DEP), sq_d = sqrt(ODO_LAMBDA_DEP);
        const double px = o.px, py = o.py, pz = o.pz;
        const double sI = ODO_SOBEL_SCALE * a_t;
        const double c0 = sI * nan0(L.Idx[ft + j]) * L.fx / pz, c1 = sI * nan0(L.Idy[ft + j]) * L.fy / pz;
        const double c2 = -(c0 * px + c1 * py) / pz;
        const double d0 = ODO_SOBEL_SCALE * nan0(L.Ddx[ft + j]) * L.fx / pz,
                     d1 = ODO_SOBEL_SCALE * nan0(L.Ddy[ft + j]) * L.fy / pz;
        const double d2 = -(d0 * px + d1 * py) / pz;
        const double JI[6] = {sq_i * (-pz * c1 + py * c2), sq_i * (pz * c0 - px * c2), sq_i * (-py * c0 + px * c1),
                              sq_i * c0,                   sq_i * c1,                  sq_i * c2};
        const double JD[6] = {sq_d * (-pz * d1 + py * d2 - py), sq_d * (pz * d0 - px * d2 + px),
                              sq_d * (-py * d0 + px * d1),      sq_d * d0,
                              sq_d * d1,                        sq_d * (d2 - 1.0)};
        const double rI = sq_i * (a_t * (double)L.I[ft + j] - a_s * (double)L.I[fs + i]);
        const double rD = sq_d * (o.dt - pz);
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) v[k++] = JI[r] * JI[c] + JD[r] * JD[c];
#pragma unroll
        for (int r = 0; r < 6; ++r) v[21 + r] = JI[r] * rI + JD[r] * rD;
        v[27] = 1.0;
    }
    icp_reduce_chunk<ODO_NSUM>(v, t, blockIdx.x, nchunks, red, part + (size_t)p * part_stride);
}

// One wave per pair: the chunks' rows in order (every lane ends with all 28).
PDSC_DEV void odo_sum_chunks(const double *part, int nchunks, int lane, double (&S)[ODO_NSUM]) {
    double acc = 0.0;
    if (lane < ODO_NSUM)
        for (int c = 0; c < nchunks; ++c) acc += part[(size_t)c * ODO_NSUM + lane];
#pragma unroll
    for (int j = 0; j < ODO_NSUM; ++j) S[j] = __shfl(acc, j);
}

// J^T J x = -J^T r by Cholesky, T <- Exp(x) T; every lane computes the same, lane 0 stores
__global__ __launch_bounds__(64) void odo_solve_kernel(const double *__restrict__ part, size_t part_stride, int nchunks,
                                                       OdoState *st) {
    const int p = blockIdx.x, lane = threadIdx.x;
    OdoState &s = st[p];
    if (s.done) return;
    double S[ODO_NSUM];
    odo_sum_chunks(part + (size_t)p * part_stride, nchunks, lane, S);
    double A[6][6], x[6];
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) A[c][r] = S[k++];  // the lower triangle
    bool ok = S[27] > 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {  // A = L L^T in place
        double d = A[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) d -= A[j][q] * A[j][q];
        if (!(d > 0.0) || !isfinite(d)) ok = false;
        const double l = sqrt(d);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double a = A[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) a -= A[i][q] * A[j][q];
            A[i][j] = a / l;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {  // L z = -J^T r
        double a = -S[21 + i];
#pragma unroll
        for (int q = 0; q < i; ++q) a -= A[i][q] * x[q];
        x[i] = a / A[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L^T x = z
        double a = x[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) a -= A[q][i] * x[q];
        x[i] = a / A[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!isfinite(x[i])) ok = false;
    if (lane != 0) return;
    s.n_corr = (int)S[27];
    if (!ok) {  // trans stays as last accepted
        s.failed = 1;
        s.done = 1;
        return;
    }
    double Ex[12], T[12], Q[12];
    se3_exp(x, Ex);
    aff_load(s.T, T);
    aff_mul(Ex, T, Q);
#pragma unroll
    for (int i = 0; i < 12; ++i) s.T[i] = Q[i];
    s.iters += 1;
}

// the debug entry's finish: the 28 sums as they are
__global__ __launch_bounds__(64) void odo_sums_out_kernel(const double *__restrict__ part, size_t part_stride,
                                                          int nchunks, double *sums) {
    double S[ODO_NSUM];
    odo_sum_chunks(part + (size_t)blockIdx.x * part_stride, nchunks, threadIdx.x, S);
    if (threadIdx.x == 0)
        for (int j = 0; j < ODO_NSUM; ++j) sums[(size_t)blockIdx.x * ODO_NSUM + j] = S[j];
}

// step 6: f11's sums over the back-projected target points of the level-0 correspondences
__global__ __launch_bounds__(ODO_CHUNK) void odo_info_kernel(OdoLevel L, const int *__restrict__ pair_src,
                                                             const int *__restrict__ pair_tgt,
                                                             const OdoState *__restrict__ st, double max_depth_diff,
                                                             u64 *__restrict__ keys, size_t key_stride, int nchunks,
                                                             double *__restrict__ part, size_t part_stride) {
    __shared__ double red[4 * INFO_NSUM];
    const int p = blockIdx.y, t = threadIdx.x, HW = L.H * L.W, j = blockIdx.x * ODO_CHUNK + t;
    const size_t fs = (size_t)pair_src[p] * HW, ft = (size_t)pair_tgt[p] * HW;
    double T[12];
    aff_load(st[p].T, T);
    double v[INFO_NSUM];
#pragma unroll
    for (int k = 0; k < INFO_NSUM; ++k) v[k] = 0.0;
    OdoProj o;
    const int i = odo_take(L, L.D + fs, L.D + ft, T, j, HW, max_depth_diff, keys + (size_t)p * key_stride, o);
    if (i >= 0) {
        const int ut = j % L.W, vt = j / L.W;
        const double z = o.dt, x = (((double)ut - L.cx) * z) / L.fx, y = (((double)vt - L.cy) * z) / L.fy;
        v[0] = 1.0;
        v[1] = x;
        v[2] = y;
        v[3] = z;
        v[4] = x * x;
        v[5] = x * y;
        v[6] = x * z;
        v[7] = y * y;
        v[8] = y * z;
        v[9] = z * z;
    }
    icp_reduce_chunk<INFO_NSUM>(v, t, blockIdx.x, nchunks, red, part + (size_t)p * part_stride);
}

__global__ __launch_bounds__(64) void odo_finish_kernel(const double *__restrict__ part, size_t part_stride,
                                                        int nchunks, const OdoState *__restrict__ st, double *trans,
                                                        double *info, pdsc_rgbd_odometry_status *status) {
    const int p = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    if (lane < INFO_NSUM)
        for (int c = 0; c < nchunks; ++c) acc += part[(size_t)p * part_stride + (size_t)c * INFO_NSUM + lane];
    double S[INFO_NSUM];
#pragma unroll
    for (int j = 0; j < INFO_NSUM; ++j) S[j] = __shfl(acc, j);
    if (lane != 0) return;
    info_from_sums(S, info + 36 * (size_t)p);
    for (int i = 0; i < 12; ++i) trans[16 * (size_t)p + i] = st[p].T[i];
    trans[16 * (size_t)p + 12] = 0.0;
    trans[16 * (size_t)p + 13] = 0.0;
    trans[16 * (size_t)p + 14] = 0.0;
    trans[16 * (size_t)p + 15] = 1.0;
    status[p].success = st[p].failed ? 0 : 1;
    status[p].n_corr_last = st[p].n_corr;
    status[p].iterations_run = st[p].iters;
    status[p].pad = 0;
}

// uint8 colour / uint16 depth -> intensity and metres (open3d's create_from_color_and_depth)
__global__ __launch_bounds__(256) void rgbd_convert_kernel(const uint8_t *__restrict__ color,
                                                           const uint16_t *__restrict__ depth16, size_t n,
                                                           float depth_scale, float depth_trunc,
                                                           float *__restrict__ intensity, float *__restrict__ depth) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = color[3 * i], g = color[3 * i + 1], b = color[3 * i + 2];
    intensity[i] = ((0.299f * r + 0.587f * g) + 0.114f * b) / 255.0f;
    const float d = (float)depth16[i] / depth_scale;
    depth[i] = d > depth_trunc ? 0.0f : d;
}

// ------------------------------------------------------------------ launchers
static size_t odo_chunks(int H, int W, int l) { return ((size_t)(H >> l) * (W >> l) + ODO_CHUNK - 1) / ODO_CHUNK; }

struct OdoBufs {
    OdoLevel lv[ODO_LEVELS];
    u64 *keys;     // [P][H W]
    double *part;  // [P][chunks of level 0][28]
    OdoState *st;  // [P]
    int *pair_src, *pair_tgt;
};
static void bind_odo(Carve &c, int F, int H, int W, int P, OdoBufs &B) {
    for (int l = 0; l < ODO_LEVELS; ++l) {
        OdoLevel &L = B.lv[l];
        L.H = H >> l;
        L.W = W >> l;
        const size_t n = (size_t)F * L.H * L.W;
        L.I = c.take<float>(n);
        L.D = c.take<float>(n);
        L.Idx = c.take<float>(n);
        L.Idy = c.take<float>(n);
        L.Ddx = c.take<float>(n);
        L.Ddy = c.take<float>(n);
    }
    B.keys = c.take<u64>((size_t)P * H * W);
    B.part = c.take<double>((size_t)P * odo_chunks(H, W, 0) * ODO_NSUM);
    B.st = c.take<OdoState>(P);
    B.pair_src = c.take<int>(P);
    B.pair_tgt = c.take<int>(P);
}

// One predicate for every entry.  frames_only (the pyramid entry: step 1 has no
// pairs) leaves out the checks of the pair list, the intrinsics, max_depth_diff
// and the iteration counts; the frame checks and their order are the same.
static int odo_check(const void *intensity, const void *depth, int F, int H, int W, double fx, double fy, double cx,
                     double cy, const int32_t *pair_src, const int32_t *pair_tgt, int P,
                     const pdsc_rgbd_odometry_options *opt, const void *ws, bool frames_only = false) {
    if (!intensity || !depth || (!frames_only && (!pair_src || !pair_tgt)) || !opt || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    if (F < 1 || P < 1) return fail(PDSC_ERR_ARG, "F=%d P=%d (need F >= 1, P >= 1)", F, P);
    if (H < 8 || W < 8 || H % 4 || W % 4)
        return fail(PDSC_ERR_ARG, "H=%d W=%d (need >= 8 and divisible by 4: three pyramid levels)", H, W);
    if (F > ODO_MAX_GRID_Y || P > ODO_MAX_GRID_Y)
        return fail(PDSC_ERR_UNSUPPORTED, "F=%d P=%d (at most %d each)", F, P, ODO_MAX_GRID_Y);
    if ((long long)H * W > ODO_MAX_PIXELS)
        return fail(PDSC_ERR_UNSUPPORTED, "H=%d W=%d (at most 2^26 pixels per frame)", H, W);
    const double k[4] = {fx, fy, cx, cy};
    for (double v : k)
        if (!frames_only && (!(v > 0.0) || !std::isfinite(v)))
            return fail(PDSC_ERR_ARG, "intrinsics fx=%g fy=%g cx=%g cy=%g must be > 0 and finite", fx, fy, cx, cy);
    if (!frames_only && (!(opt->max_depth_diff > 0.0) || !std::isfinite(opt->max_depth_diff)))
        return fail(PDSC_ERR_ARG, "max_depth_diff %g must be > 0 and finite", opt->max_depth_diff);
    if (!(opt->min_depth >= 0.0) || !(opt->max_depth > opt->min_depth) || !std::isfinite(opt->max_depth))
        return fail(PDSC_ERR_ARG, "min_depth %g / max_depth %g (need 0 <= min < max, finite)", opt->min_depth,
                    opt->max_depth);
    if (frames_only) return PDSC_OK;
    for (int l = 0; l < ODO_LEVELS; ++l)
        if (opt->iterations[l] < 0 || opt->iterations[l] > 1000)
            return fail(PDSC_ERR_ARG, "iterations[%d]=%d (need 0 .. 1000)", l, opt->iterations[l]);
    for (int p = 0; p < P; ++p)
        if (pair_src[p] < 0 || pair_src[p] >= F || pair_tgt[p] < 0 || pair_tgt[p] >= F || pair_src[p] == pair_tgt[p])
            return fail(PDSC_ERR_ARG, "pair %d = (%d, %d): need two different frames in [0, %d)", p, pair_src[p],
                        pair_tgt[p], F);
    return PDSC_OK;
}

// step 1: every frame's three levels, 6 images each
static void odo_frames(const float *intensity, const float *depth, int F, int H, int W,
                       const pdsc_rgbd_odometry_options *opt, OdoBufs &B, hipStream_t s) {
    hipLaunchKernelGGL(odo_prep0_kernel, dim3((unsigned)odo_chunks(H, W, 0), F), dim3(256), 0, s, intensity, depth, H, W,
                       (float)opt->min_depth, (float)opt->max_depth, B.lv[0].I, B.lv[0].D);
    for (int l = 1; l < ODO_LEVELS; ++l)
        hipLaunchKernelGGL(odo_down_kernel, dim3((unsigned)odo_chunks(H, W, l), F), dim3(256), 0, s, B.lv[l - 1].I,
                           B.lv[l - 1].D, B.lv[l - 1].H, B.lv[l - 1].W, B.lv[l].I, B.lv[l].D);
    for (int l = 0; l < ODO_LEVELS; ++l)
        hipLaunchKernelGGL(odo_sobel_kernel, dim3((unsigned)odo_chunks(H, W, l), F), dim3(256), 0, s, B.lv[l]);
}

// the frames' pyramids, the pair list and the pairs' states; then a_s, a_t (step 2)
static int odo_setup(const float *intensity, const float *depth, int F, int H, int W, double fx, double fy, double cx,
                     double cy, const int32_t *pair_src, const int32_t *pair_tgt, int P, const double *init,
                     const pdsc_rgbd_odometry_options *opt, OdoBufs &B, double *scales, hipStream_t s) {
    for (int l = 0; l < ODO_LEVELS; ++l) {
        const double sc = 1.0 / (double)(1 << l);
        B.lv[l].fx = fx * sc;
        B.lv[l].fy = fy * sc;
        B.lv[l].cx = cx * sc;
        B.lv[l].cy = cy * sc;
    }
    HIPCHK(hipMemcpyAsync(B.pair_src, pair_src, sizeof(int) * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(B.pair_tgt, pair_tgt, sizeof(int) * P, hipMemcpyHostToDevice, s));
    odo_frames(intensity, depth, F, H, W, opt, B, s);
    hipLaunchKernelGGL(odo_init_kernel, dim3((P + 63) / 64), dim3(64), 0, s, B.st, init, P);
    const size_t nk = (size_t)P * H * W;
    hipLaunchKernelGGL(odo_fill_keys_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, B.keys, nk);
    const size_t ks = (size_t)H * W, ps = odo_chunks(H, W, 0) * ODO_NSUM;
    const int nc = (int)odo_chunks(H, W, 0);
    hipLaunchKernelGGL(odo_corr_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[0], B.pair_src, B.pair_tgt, B.st,
                       opt->max_depth_diff, 0, B.keys, ks);
    hipLaunchKernelGGL(odo_norm_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[0], B.pair_src, B.pair_tgt, B.st,
                       opt->max_depth_diff, B.keys, ks, nc, B.part, ps);
    hipLaunchKernelGGL(odo_norm_finish_kernel, dim3(P), dim3(64), 0, s, B.part, ps, nc, B.st, scales);
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_rgbd_odometry_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t P) {
    if (F < 1 || P < 1 || H < 8 || W < 8 || H % 4 || W % 4 || F > ODO_MAX_GRID_Y || P > ODO_MAX_GRID_Y ||
        (long long)H * W > ODO_MAX_PIXELS)
        return 0;
    Carve c(nullptr);
    OdoBufs B;
    bind_odo(c, F, H, W, P, B);
    return c.off;
}

int32_t pdsc_rgbd_odometry(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W, double fx,
                           double fy, double cx, double cy, const int32_t *pair_src, const int32_t *pair_tgt, int32_t P,
                           const double *init, const pdsc_rgbd_odometry_options *options, double *trans, double *info,
                           pdsc_rgbd_odometry_status *status, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(odo_check(intensity, depth, F, H, W, fx, fy, cx, cy, pair_src, pair_tgt, P, options, ws));
    if (!trans || !info || !status) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_rgbd_odometry_workspace_bytes(F, H, W, P)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    OdoBufs B;
    bind_odo(c, F, H, W, P, B);
    RET_IF(odo_setup(intensity, depth, F, H, W, fx, fy, cx, cy, pair_src, pair_tgt, P, init, options, B, nullptr, s));
    const size_t ks = (size_t)H * W, ps = odo_chunks(H, W, 0) * ODO_NSUM;
    const double mdd = options->max_depth_diff;
    for (int k = 0; k < ODO_LEVELS; ++k) {  // coarsest level first
        const int l = ODO_LEVELS - 1 - k, nc = (int)odo_chunks(H, W, l);
        for (int it = 0; it < options->iterations[k]; ++it) {
            hipLaunchKernelGGL(odo_corr_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[l], B.pair_src, B.pair_tgt,
                               B.st, mdd, 1, B.keys, ks);
            hipLaunchKernelGGL(odo_lin_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[l], B.pair_src, B.pair_tgt, B.st,
                               mdd, 1, B.keys, ks, nc, B.part, ps, (int *)nullptr);
            hipLaunchKernelGGL(odo_solve_kernel, dim3(P), dim3(64), 0, s, B.part, ps, nc, B.st);
        }
    }
    const int nc = (int)odo_chunks(H, W, 0);
    hipLaunchKernelGGL(odo_corr_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[0], B.pair_src, B.pair_tgt, B.st, mdd,
                       0, B.keys, ks);
    hipLaunchKernelGGL(odo_info_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[0], B.pair_src, B.pair_tgt, B.st, mdd,
                       B.keys, ks, nc, B.part, ps);
    hipLaunchKernelGGL(odo_finish_kernel, dim3(P), dim3(64), 0, s, B.part, ps, nc, B.st, trans, info, status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return PDSC_OK;
}

int32_t pdsc_rgbd_odometry_linearize(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W,
                                     double fx, double fy, double cx, double cy, const int32_t *pair_src,
                                     const int32_t *pair_tgt, int32_t P, const double *trans,
                                     const pdsc_rgbd_odometry_options *options, int32_t level, int32_t *corr,
                                     double *sums, double *scales, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(odo_check(intensity, depth, F, H, W, fx, fy, cx, cy, pair_src, pair_tgt, P, options, ws));
    if (!sums) return fail(PDSC_ERR_ARG, "null pointer");
    if (level < 0 || level >= ODO_LEVELS) return fail(PDSC_ERR_ARG, "level=%d (need 0 .. %d)", level, ODO_LEVELS - 1);
    RET_IF(need_ws(ws_bytes, pdsc_rgbd_odometry_workspace_bytes(F, H, W, P)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    OdoBufs B;
    bind_odo(c, F, H, W, P, B);
    RET_IF(odo_setup(intensity, depth, F, H, W, fx, fy, cx, cy, pair_src, pair_tgt, P, trans, options, B, scales, s));
    const size_t ks = (size_t)H * W, ps = odo_chunks(H, W, 0) * ODO_NSUM;
    const int nc = (int)odo_chunks(H, W, level);
    hipLaunchKernelGGL(odo_corr_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[level], B.pair_src, B.pair_tgt, B.st,
                       options->max_depth_diff, 0, B.keys, ks);
    hipLaunchKernelGGL(odo_lin_kernel, dim3(nc, P), dim3(ODO_CHUNK), 0, s, B.lv[level], B.pair_src, B.pair_tgt, B.st,
                       options->max_depth_diff, 0, B.keys, ks, nc, B.part, ps, corr);
    hipLaunchKernelGGL(odo_sums_out_kernel, dim3(P), dim3(64), 0, s, B.part, ps, nc, sums);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return PDSC_OK;
}

int32_t pdsc_rgbd_odometry_pyramid(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W,
                                   double min_depth, double max_depth, int32_t level, float *I, float *D, float *Idx,
                                   float *Idy, float *Ddx, float *Ddy, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    pdsc_rgbd_odometry_options opt = {};
    opt.min_depth = min_depth;
    opt.max_depth = max_depth;
    RET_IF(odo_check(intensity, depth, F, H, W, 0.0, 0.0, 0.0, 0.0, nullptr, nullptr, 1, &opt, ws, true));
    if (level < 0 || level >= ODO_LEVELS) return fail(PDSC_ERR_ARG, "level=%d (need 0 .. %d)", level, ODO_LEVELS - 1);
    RET_IF(need_ws(ws_bytes, pdsc_rgbd_odometry_workspace_bytes(F, H, W, 1)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    OdoBufs B;
    bind_odo(c, F, H, W, 1, B);
    odo_frames(intensity, depth, F, H, W, &opt, B, s);
    const OdoLevel &L = B.lv[level];
    const size_t bytes = sizeof(float) * (size_t)F * L.H * L.W;
    float *const out[6] = {I, D, Idx, Idy, Ddx, Ddy};
    const float *const img[6] = {L.I, L.D, L.Idx, L.Idy, L.Ddx, L.Ddy};
    for (int k = 0; k < 6; ++k)
        if (out[k]) HIPCHK(hipMemcpyAsync(out[k], img[k], bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return PDSC_OK;
}

int32_t pdsc_rgbd_from_color_and_depth(const uint8_t *color, const uint16_t *depth16, int32_t F, int32_t H, int32_t W,
                                       double depth_scale, double depth_trunc, float *intensity, float *depth,
                                       pdsc_stream_t stream) {
    if (!color || !depth16 || !intensity || !depth) return fail(PDSC_ERR_ARG, "null pointer");
    if (F < 1 || H < 1 || W < 1) return fail(PDSC_ERR_ARG, "F=%d H=%d W=%d (need >= 1)", F, H, W);
    if (!(depth_scale > 0.0) || !std::isfinite(depth_scale) || !(depth_trunc > 0.0))
        return fail(PDSC_ERR_ARG, "depth_scale %g / depth_trunc %g must be > 0", depth_scale, depth_trunc);
    const size_t n = (size_t)F * H * W;
    hipLaunchKernelGGL(rgbd_convert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S_(stream), color, depth16,
                       n, (float)depth_scale, (float)depth_trunc, intensity, depth);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
