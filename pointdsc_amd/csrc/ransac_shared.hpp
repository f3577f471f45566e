// ransac_shared.hpp -- what ransac.hip (f6) and gc_ransac.hip (f10) share:
//   host    the round workspace's layout (bind_ransac) and a round's launch shape
//           (ransac_round_shape);
//   sample  the counter-based sampler, the fp64 Kabsch of a sample (compensated H,
//           Jacobi SVD, one Newton step), d^2, the c[12] <-> T[16] pose conversions;
//   round   the hypothesis and scoring kernels (templates: each translation unit
//           instantiates its own), the "never drawn" debug prefill, the round's
//           reduction under a caller's total order (round_best) and the
//           confidence stop rule;
//   finish  the label-and-sum loop over d^2 < r2 (label_inliers) and the refit
//           over a row predicate.
// Everything here is fp64 without contraction in a fixed order, so a caller
// gets the same bits from either translation unit.
#pragma once
#include "abi.hpp"
#include "pdsc_common.hpp"
#include "pdsc_internal.hpp"

namespace pdsc {

typedef unsigned long long u64;
constexpr int RANSAC_ROUND = 16384;                    // hypotheses per round: part of the result's definition (pdsc_ransac_round)
constexpr int RANSAC_HWG = 256;                        // hypotheses per workgroup of the hypothesis kernel
constexpr int RANSAC_NWG = RANSAC_ROUND / RANSAC_HWG;  // its workgroups per full round
constexpr int RANSAC_PCHUNK = 256;                     // points per scoring chunk (the fixed summation order)
constexpr int RANSAC_FIN = 256;                        // threads of the round / finish kernels
static_assert(RANSAC_NWG <= 64, "the score kernel scans the workgroup counts in one wave");
static_assert(RANSAC_ROUND % RANSAC_HWG == 0, "whole workgroups per round");

struct RansacState {
    double c[12];  // the best hypothesis: R row-major [9], t [3]
    double sumsq;
    int count, best, iterations, n_validated, done, pad;
};

struct RansacBufs {
    RansacState *st;
    int *wgcount;  // [RANSAC_NWG] survivors per hypothesis workgroup
    int *hidx;     // [ROUND] slot -> h (slot = workgroup * RANSAC_HWG + rank)
    int *gslot;    // [ROUND] compact index -> slot
    double *coef;  // [12][ROUND] by slot
    int *pcount;   // [nchunks][ROUND] by compact index
    double *psum;  // [nchunks][ROUND]
};

// the workspace of a round over N rows
inline size_t ransac_chunks(int N) { return ((size_t)N + RANSAC_PCHUNK - 1) / RANSAC_PCHUNK; }
inline void bind_ransac(Carve &c, int N, RansacBufs &B) {
    const size_t R = RANSAC_ROUND, nchunks = ransac_chunks(N);
    B.st = c.take<RansacState>(1);
    B.wgcount = c.take<int>(RANSAC_NWG);
    B.hidx = c.take<int>(R);
    B.gslot = c.take<int>(R);
    B.coef = c.take<double>(12 * R);
    B.pcount = c.take<int>(nchunks * R);
    B.psum = c.take<double>(nchunks * R);
}

// Round r of H hypotheses: the first hypothesis, how many it draws, their workgroups.
struct RoundShape {
    int base, nh, nwg;
};
inline int ransac_rounds(int H) { return (int)(((size_t)H + RANSAC_ROUND - 1) / RANSAC_ROUND); }
inline RoundShape ransac_round_shape(int H, int r) {
    const long long base = (long long)r * RANSAC_ROUND, left = (long long)H - base;
    const int nh = (int)(left < (long long)RANSAC_ROUND ? left : (long long)RANSAC_ROUND);
    return {(int)base, nh, (nh + RANSAC_HWG - 1) / RANSAC_HWG};
}

PDSC_DEV u64 mix64(u64 z) {  // the splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
PDSC_DEV int ransac_draw(u64 seed, int h, int j, int N) {
    const u64 u = mix64(seed + (8ull * (u64)h + (u64)j) * 0x9E3779B97F4A7C15ull);
    return (int)(((u >> 32) * (u64)N) >> 32);
}

PDSC_DEV D3 load3(const float *__restrict__ p, int i) {
    return d3((double)p[3 * (size_t)i], (double)p[3 * (size_t)i + 1], (double)p[3 * (size_t)i + 2]);
}
PDSC_DEV D3 sub3(const D3 &a, const D3 &b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }

// ---------------------------------------------------------------------------
// kabsch_rotation's R = V diag(1, 1, det(V U^T)) U^T by a one-sided Jacobi SVD
// of H itself.  kabsch_rotation (pdsc_common.hpp) diagonalises H^T H, which
// squares the condition number: for a sample whose sigma_2 / sigma_1 is 1e-4
// (three nearly collinear points; one in a few thousand draws) its rotation is
// off by 1e-8, more than this stage's 1e-9 bound against LAPACK.  Rotating the
// columns of G = H V until they are orthogonal keeps the error at about
// eps sigma_1 / sigma_2 (kabsch_newton takes it from there).  Named scalars only (no scratch), one H per lane.
// ---------------------------------------------------------------------------
PDSC_DEV void hrot(D3 &gp, D3 &gq, D3 &vp, D3 &vq, bool &rotated) {
    const double alpha = dot3(gp, gp), beta = dot3(gq, gq), gamma = dot3(gp, gq);
    if (alpha == 0.0 || beta == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) return;
    rotated = true;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const D3 g0 = gp, g1 = gq, v0 = vp, v1 = vq;
    gp = d3(c * g0.x - s * g1.x, c * g0.y - s * g1.y, c * g0.z - s * g1.z);
    gq = d3(s * g0.x + c * g1.x, s * g0.y + c * g1.y, s * g0.z + c * g1.z);
    vp = d3(c * v0.x - s * v1.x, c * v0.y - s * v1.y, c * v0.z - s * v1.z);
    vq = d3(s * v0.x + c * v1.x, s * v0.y + c * v1.y, s * v0.z + c * v1.z);
}

// H row-major (H[i][j] = sum Am_i Bm_j) -> R row-major.
PDSC_DEV void kabsch_rotation_svd(const double H[9], double R[9]) {
    D3 g0 = d3(H[0], H[3], H[6]), g1 = d3(H[1], H[4], H[7]), g2 = d3(H[2], H[5], H[8]);  // columns of H V
    D3 v0 = d3(1, 0, 0), v1 = d3(0, 1, 0), v2 = d3(0, 0, 1);                             // columns of V
    for (int sweep = 0; sweep < 12; ++sweep) {
        bool rotated = false;
        hrot(g0, g1, v0, v1, rotated);
        hrot(g0, g2, v0, v2, rotated);
        hrot(g1, g2, v1, v2, rotated);
        if (!rotated) break;
    }
    double s0 = dot3(g0, g0), s1 = dot3(g1, g1), s2 = dot3(g2, g2);  // sigma^2, then by descending sigma
    if (s0 < s1) {
        const double ts = s0; s0 = s1; s1 = ts;
        const D3 tg = g0; g0 = g1; g1 = tg;
        const D3 tv = v0; v0 = v1; v1 = tv;
    }
    if (s0 < s2) {
        const double ts = s0; s0 = s2; s2 = ts;
        const D3 tg = g0; g0 = g2; g2 = tg;
        const D3 tv = v0; v0 = v2; v2 = tv;
    }
    if (s1 < s2) {
        const double ts = s1; s1 = s2; s2 = ts;
        const D3 tg = g1; g1 = g2; g2 = tg;
        const D3 tv = v1; v1 = v2; v2 = tv;
    }
    if (!(s0 > 0)) {  // H == 0: LAPACK returns U = V = I -> R = I
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    D3 u0 = g0, u1 = g1;
    const double n0 = normalize3(u0);
    const double d01 = dot3(u1, u0);
    u1 = d3(u1.x - d01 * u0.x, u1.y - d01 * u0.y, u1.z - d01 * u0.z);
    const double n1 = normalize3(u1);
    if (!(n1 > 1e-290) || !(n1 > 1e-15 * n0)) u1 = orthogonal3(u0);  // rank 1: any completion (no exactness claim)
    const D3 u2 = cross3(u0, u1);
    const double d = dot3(v0, cross3(v1, v2)) < 0 ? -1.0 : 1.0;  // det(V); det(U) = +1
    R[0] = v0.x * u0.x + v1.x * u1.x + d * v2.x * u2.x;
    R[1] = v0.x * u0.y + v1.x * u1.y + d * v2.x * u2.y;
    R[2] = v0.x * u0.z + v1.x * u1.z + d * v2.x * u2.z;
    R[3] = v0.y * u0.x + v1.y * u1.x + d * v2.y * u2.x;
    R[4] = v0.y * u0.y + v1.y * u1.y + d * v2.y * u2.y;
    R[5] = v0.y * u0.z + v1.y * u1.z + d * v2.y * u2.z;
    R[6] = v0.z * u0.x + v1.z * u1.x + d * v2.z * u2.x;
    R[7] = v0.z * u0.y + v1.z * u1.y + d * v2.z * u2.y;
    R[8] = v0.z * u0.z + v1.z * u1.z + d * v2.z * u2.z;
}

// R, t of the unit-weight Kabsch of n centred sums: ca, cb the centroids,
// H[i][j] = sum (a - ca)_i (b - cb)_j; c = R row-major [9], t = cb - R ca [3].
PDSC_DEV void kabsch_pose(const double R[9], const D3 &ca, const D3 &cb, double c[12]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = R[i];
    c[9] = cb.x - ((R[0] * ca.x + R[1] * ca.y) + R[2] * ca.z);
    c[10] = cb.y - ((R[3] * ca.x + R[4] * ca.y) + R[5] * ca.z);
    c[11] = cb.z - ((R[6] * ca.x + R[7] * ca.y) + R[8] * ca.z);
}

// c = R row-major [9], t [3]  <->  T = the row-major 4x4 (its last row 0 0 0 1)
PDSC_DEV void pose16(const double c[12], double T[16]) {
    T[0] = c[0], T[1] = c[1], T[2] = c[2], T[3] = c[9];
    T[4] = c[3], T[5] = c[4], T[6] = c[5], T[7] = c[10];
    T[8] = c[6], T[9] = c[7], T[10] = c[8], T[11] = c[11];
    T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
}
PDSC_DEV void pose12(const double T[16], double c[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[3 * i] = T[4 * i], c[3 * i + 1] = T[4 * i + 1], c[3 * i + 2] = T[4 * i + 2];
        c[9 + i] = T[4 * i + 3];
    }
}

// ---------------------------------------------------------------------------
// The sample's pose to fp64 rounding.  Any fp64 SVD of an fp64 H is only good
// to eps sigma_1 / sigma_2 (the roundings of H itself are amplified as much), a
// few 1e-14 for one sample in a hundred, which reaches 1e-12 of that
// hypothesis's sum d^2.  So H is accumulated as an unevaluated sum hi + lo
// (error-free products by fma, compensated sums) from quantities that are exact
// in fp64 for fp32 inputs -- the differences to the first pair, times n, minus
// their sum -- and the Jacobi rotation R0 gets one Newton step on SO(3): the
// optimum makes M = R H symmetric, the step is w = (tr(P) I - P)^-1 g with P =
// sym(M) and g the axial vector of M - M^T evaluated in hi + lo, after taking
// out R0's own orthogonality defect D = R0 R0^T - I (also hi + lo; left in, it
// would be amplified like any other 1e-16 of M).  (tr(P) I - P) has the
// eigenvalues sigma_i + sigma_j: the step is skipped where it is singular (rank-1
// samples) or would be large.
// ---------------------------------------------------------------------------
struct DD {
    double h, l;
};
PDSC_DEV void dd_add_prod(DD &acc, double a, double b) {  // acc += a b, the product error-free
    const double p = a * b, e = __builtin_fma(a, b, -p);
    const double s = acc.h + p, bb = s - acc.h;
    const double x = (acc.h - (s - bb)) + (p - bb);
    acc.h = s;
    acc.l += x + e;
}

PDSC_DEV void kabsch_newton(const double Hh[9], const double Hl[9], double R[9]) {
    double D[9], M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            DD a = {i == j ? -1.0 : 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k) dd_add_prod(a, R[3 * i + k], R[3 * j + k]);
            D[3 * i + j] = D[3 * j + i] = a.h + a.l;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = (R[3 * i] * Hh[j] + R[3 * i + 1] * Hh[3 + j]) + R[3 * i + 2] * Hh[6 + j];
    double g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // g_a = M[i][j] - M[j][i], (i, j) = (1,2), (2,0), (0,1)
        const int i = (a + 1) % 3, j = (a + 2) % 3;
        DD acc = {0.0, 0.0};
        double lo = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dd_add_prod(acc, R[3 * i + k], Hh[3 * k + j]);
            dd_add_prod(acc, -R[3 * j + k], Hh[3 * k + i]);
            lo += R[3 * i + k] * Hl[3 * k + j] - R[3 * j + k] * Hl[3 * k + i];
        }
        // (I - D / 2) M in place of M: minus half the same difference of D M
        double dm = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) dm += D[3 * i + k] * M[3 * k + j] - D[3 * j + k] * M[3 * k + i];
        g[a] = (acc.h + (acc.l + lo)) - 0.5 * dm;
    }
    const double tr = M[0] + M[4] + M[8];
    const double a = tr - M[0], d = tr - M[4], f = tr - M[8];
    const double b = -0.5 * (M[1] + M[3]), c = -0.5 * (M[2] + M[6]), e = -0.5 * (M[5] + M[7]);
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double det = (a * c00 + b * c01) + c * c02;
    const double sc = fabs(tr);
    if (!(fabs(det) > 1e-12 * sc * sc * sc)) return;
    const double inv = 1.0 / det;
    const double w0 = ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) * inv;
    const double w1 = ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) * inv;
    const double w2 = ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) * inv;
    if (!((w0 * w0 + w1 * w1) + w2 * w2 < 1e-12)) return;
    double R1[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R1[3 * i + j] = R[3 * i + j] -
                            0.5 * ((D[3 * i] * R[j] + D[3 * i + 1] * R[3 + j]) + D[3 * i + 2] * R[6 + j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // column j: r + w x r + (w x (w x r)) / 2
        const D3 r = d3(R1[j], R1[3 + j], R1[6 + j]), w = d3(w0, w1, w2);
        const D3 wr = cross3(w, r), wwr = cross3(w, wr);
        R[j] = r.x + (wr.x + 0.5 * wwr.x);
        R[3 + j] = r.y + (wr.y + 0.5 * wwr.y);
        R[6 + j] = r.z + (wr.z + 0.5 * wwr.z);
    }
}

// The unit-weight Kabsch of the NS sampled pairs (s_j, t_j) -> c.
template <int NS> PDSC_DEV void kabsch_sample(const D3 (&s)[NS], const D3 (&t)[NS], double c[12]) {
    D3 da[NS], db[NS];
    D3 sa = d3(0, 0, 0), sb = d3(0, 0, 0);
#pragma unroll
    for (int j = 0; j < NS; ++j) {  // exact: fp32 inputs
        da[j] = sub3(s[j], s[0]);
        db[j] = sub3(t[j], t[0]);
        sa = d3(sa.x + da[j].x, sa.y + da[j].y, sa.z + da[j].z);
        sb = d3(sb.x + db[j].x, sb.y + db[j].y, sb.z + db[j].z);
    }
    DD H[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = DD{0.0, 0.0};
    const double n = (double)NS;
#pragma unroll
    for (int j = 0; j < NS; ++j) {  // n^2 H = sum (n a_j - sum a)(n b_j - sum b)^T: the scale does not matter
        const D3 a = d3(n * da[j].x - sa.x, n * da[j].y - sa.y, n * da[j].z - sa.z);
        const D3 b = d3(n * db[j].x - sb.x, n * db[j].y - sb.y, n * db[j].z - sb.z);
        dd_add_prod(H[0], a.x, b.x);
        dd_add_prod(H[1], a.x, b.y);
        dd_add_prod(H[2], a.x, b.z);
        dd_add_prod(H[3], a.y, b.x);
        dd_add_prod(H[4], a.y, b.y);
        dd_add_prod(H[5], a.y, b.z);
        dd_add_prod(H[6], a.z, b.x);
        dd_add_prod(H[7], a.z, b.y);
        dd_add_prod(H[8], a.z, b.z);
    }
    double Hh[9], Hl[9], R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Hh[i] = H[i].h + H[i].l;
        Hl[i] = H[i].l - (Hh[i] - H[i].h);
    }
    kabsch_rotation_svd(Hh, R);
    kabsch_newton(Hh, Hl, R);
    const double inv = 1.0 / n;
    const D3 ca = d3(s[0].x + sa.x * inv, s[0].y + sa.y * inv, s[0].z + sa.z * inv);
    const D3 cb = d3(t[0].x + sb.x * inv, t[0].y + sb.y * inv, t[0].z + sb.z * inv);
    kabsch_pose(R, ca, cb, c);
}

// d^2 = |R s + t - b|^2, 15 fp64 FMA-class operations
PDSC_DEV double ransac_d2(const double c[12], double sx, double sy, double sz, double bx, double by, double bz) {
    const double dx = __builtin_fma(c[0], sx, __builtin_fma(c[1], sy, __builtin_fma(c[2], sz, c[9]))) - bx;
    const double dy = __builtin_fma(c[3], sx, __builtin_fma(c[4], sy, __builtin_fma(c[5], sz, c[10]))) - by;
    const double dz = __builtin_fma(c[6], sx, __builtin_fma(c[7], sy, __builtin_fma(c[8], sz, c[11]))) - bz;
    return __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
}

// ------------------------------------------------------------------ hypotheses
template <int NS>
__global__ __launch_bounds__(RANSAC_HWG) void ransac_hyp_kernel(const float *__restrict__ src,
                                                                const float *__restrict__ tgt, int N, int base,
                                                                int H, u64 seed, double sim, RansacBufs B,
                                                                pdsc_ransac_debug dbg) {
    __shared__ int wtot[RANSAC_HWG / 64];
    __shared__ int list[RANSAC_HWG];
    if (B.st->done) return;  // workgroup-uniform
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long hl = (long long)base + blockIdx.x * RANSAC_HWG + tid;
    const bool drawn = hl < (long long)H;
    const int h = (int)hl;  // < H <= INT_MAX for every drawn lane
    bool ok = drawn;
    if (drawn) {
        int idx[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) idx[j] = ransac_draw(seed, h, j, N);
        if (dbg.samples) {
#pragma unroll
            for (int j = 0; j < NS; ++j) dbg.samples[(size_t)h * NS + j] = idx[j];
        }
        int status = 0;
#pragma unroll
        for (int a = 0; a < NS; ++a)
#pragma unroll
            for (int b = a + 1; b < NS; ++b)
                if (idx[a] == idx[b]) status = -1;
        if (status == 0 && sim > 0.0) {
            D3 s[NS], t[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                s[j] = load3(src, idx[j]);
                t[j] = load3(tgt, idx[j]);
            }
#pragma unroll
            for (int a = 0; a < NS; ++a)
#pragma unroll
                for (int b = a + 1; b < NS; ++b) {
                    const D3 es = sub3(s[a], s[b]), et = sub3(t[a], t[b]);
                    const double ds = sqrt(dot3(es, es)), dt = sqrt(dot3(et, et));
                    if (!(ds >= sim * dt && dt >= sim * ds)) status = -2;
                }
        }
        if (status != 0 && dbg.count) dbg.count[h] = status;
        ok = status == 0;
    }
    // survivors in lane order: rank = (survivors of the lower waves) + (of the lower lanes)
    const u64 mask = __ballot(ok);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < RANSAC_HWG / 64; ++k) {
        off += k < w ? wtot[k] : 0;
        total += wtot[k];
    }
    if (ok) list[off + pre] = tid;
    __syncthreads();
    if (tid == 0) B.wgcount[blockIdx.x] = total;
    if (tid >= total) return;
    const int hh = base + blockIdx.x * RANSAC_HWG + list[tid];
    D3 s[NS], t[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = ransac_draw(seed, hh, j, N);
        s[j] = load3(src, i);
        t[j] = load3(tgt, i);
    }
    double c[12];
    kabsch_sample<NS>(s, t, c);
    const int slot = blockIdx.x * RANSAC_HWG + tid;
    B.hidx[slot] = hh;
#pragma unroll
    for (int k = 0; k < 12; ++k) B.coef[(size_t)k * RANSAC_ROUND + slot] = c[k];
    if (dbg.trans) pose16(c, dbg.trans + (size_t)hh * 16);
}

// ----------------------------------------------------------------------- score
// blockIdx.x: 64 compact hypothesis indices, blockIdx.y: the point chunk.
// MSAC (f10): psum holds sum (1 - d^2 / r2) over the inliers instead of sum d^2.
template <bool MSAC>
__global__ __launch_bounds__(64) void ransac_score_kernel(const float *__restrict__ src,
                                                          const float *__restrict__ tgt, int N, int nwg, double r2,
                                                          RansacBufs B) {
    __shared__ int pre[RANSAC_NWG + 1];
    __shared__ double pts[RANSAC_PCHUNK * 6];
    if (B.st->done) return;  // workgroup-uniform
    const int lane = threadIdx.x;
    {  // inclusive scan of the workgroups' survivor counts
        int v = lane < nwg ? B.wgcount[lane] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 0) pre[0] = 0;
        if (lane < RANSAC_NWG) pre[lane + 1] = v;
    }
    __syncthreads();
    const int total = pre[nwg];
    if ((int)blockIdx.x * 64 >= total) return;  // workgroup-uniform
    const int g = blockIdx.x * 64 + lane;
    const bool active = g < total;
    int slot = 0;
    double c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = 0.0;
    if (active) {
        int lo = 0, hi = nwg;  // the workgroup wg with pre[wg] <= g < pre[wg + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= g)
                lo = mid;
            else
                hi = mid;
        }
        slot = lo * RANSAC_HWG + (g - pre[lo]);
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k] = B.coef[(size_t)k * RANSAC_ROUND + slot];
    }
    const int p0 = blockIdx.y * RANSAC_PCHUNK;
    const int np = N - p0 < RANSAC_PCHUNK ? N - p0 : RANSAC_PCHUNK;
    for (int p = lane; p < np; p += 64) {
        const D3 a = load3(src, p0 + p), b = load3(tgt, p0 + p);
        pts[6 * p] = a.x, pts[6 * p + 1] = a.y, pts[6 * p + 2] = a.z;
        pts[6 * p + 3] = b.x, pts[6 * p + 4] = b.y, pts[6 * p + 5] = b.z;
    }
    __syncthreads();
    int cnt = 0;
    double ss = 0.0;
#pragma unroll 4
    for (int p = 0; p < np; ++p) {
        const double d2 = ransac_d2(c, pts[6 * p], pts[6 * p + 1], pts[6 * p + 2], pts[6 * p + 3], pts[6 * p + 4],
                                    pts[6 * p + 5]);
        const bool in = d2 < r2;
        cnt += in ? 1 : 0;
        if (MSAC) {
            if (in) ss += 1.0 - d2 / r2;
        } else {
            ss += in ? d2 : 0.0;
        }
    }
    if (active) {
        B.pcount[(size_t)blockIdx.y * RANSAC_ROUND + g] = cnt;
        B.psum[(size_t)blockIdx.y * RANSAC_ROUND + g] = ss;
        if (blockIdx.y == 0) B.gslot[g] = slot;
    }
}

// ----------------------------------------------------------------------- round
// The debug rows' "never drawn" status, by the init kernels' 256-thread
// workgroups (the rounds after an early stop return at entry and cannot write it).
PDSC_DEV void debug_prefill(int *dbg_count, int H, size_t i) {
    if (dbg_count && i < (size_t)H) dbg_count[i] = -3;
}

struct Cand {  // a scored hypothesis: its score (sum d^2, or the MSAC sum), inlier count, h and coefficient slot
    double s;
    int cnt, h, slot;
};

// The round's winner under `better`, returned to thread 0 (the other threads'
// return value is their wave's): the survivors' chunk rows added in chunk order
// (and written to the debug rows), a strided scan, the xor butterfly, then the
// waves through wbest [RANSAC_FIN / 64].  `better` must be a total order over
// distinct h, so that neither the stride nor the tree's shape can change the
// winner; `identity` loses to every candidate.  Sets total = the survivors.
template <typename Better>
PDSC_DEV Cand round_best(const RansacBufs &B, int nwg, int nchunks, const pdsc_ransac_debug &dbg, Cand identity,
                         Cand *wbest, int tid, int &total, Better better) {
    total = 0;
    for (int k = 0; k < nwg; ++k) total += B.wgcount[k];
    Cand best = identity;
    for (int g = tid; g < total; g += RANSAC_FIN) {
        Cand x = {0.0, 0, 0, B.gslot[g]};
        for (int ch = 0; ch < nchunks; ++ch) {  // chunk order
            x.cnt += B.pcount[(size_t)ch * RANSAC_ROUND + g];
            x.s += B.psum[(size_t)ch * RANSAC_ROUND + g];
        }
        x.h = B.hidx[x.slot];
        if (dbg.count) dbg.count[x.h] = x.cnt;
        if (dbg.sumsq) dbg.sumsq[x.h] = x.s;
        if (better(x, best)) best = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand y;
        y.s = __shfl_xor(best.s, o);
        y.cnt = __shfl_xor(best.cnt, o);
        y.h = __shfl_xor(best.h, o);
        y.slot = __shfl_xor(best.slot, o);
        if (better(y, best)) best = y;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return best;
    for (int k = 1; k < RANSAC_FIN / 64; ++k)
        if (better(wbest[k], best)) best = wbest[k];
    return best;
}

// The confidence stop after `drawn` hypotheses of ns points with `count` of N rows inliers of the best.
PDSC_DEV bool confidence_stop(int count, int N, int ns, long long drawn, double confidence) {
    if (!(confidence < 1.0 && count > 0)) return false;
    if (count == N) return true;  // f = 1: the criterion's log(0)
    const double f = (double)count / (double)N;
    const double fn = ns == 3 ? f * f * f : (f * f) * (f * f);
    return (double)drawn >= log(1.0 - confidence) / log(1.0 - fn);
}

// ---------------------------------------------------------------------- finish
// labels[i] = d^2 < r2 under c (all 0 unless valid; labels may be null), and this
// thread's inlier count and coordinate sums over its rows tid, tid + RANSAC_FIN, ...
PDSC_DEV void label_inliers(const float *__restrict__ src, const float *__restrict__ tgt, int N, const double c[12],
                            double r2, bool valid, float *labels, double &n, double sa[3], double sb[3], int tid) {
    for (int i = tid; i < N; i += RANSAC_FIN) {
        const D3 a = load3(src, i), b = load3(tgt, i);
        const bool in = valid && ransac_d2(c, a.x, a.y, a.z, b.x, b.y, b.z) < r2;
        if (labels) labels[i] = in ? 1.0f : 0.0f;
        if (in) {
            n += 1.0;
            sa[0] += a.x, sa[1] += a.y, sa[2] += a.z;
            sb[0] += b.x, sb[1] += b.y, sb[2] += b.z;
        }
    }
}

// Sum of v over the workgroup in a fixed order (xor butterfly, then the waves in
// order); every thread returns the same bits.  red: [RANSAC_FIN / 64].
PDSC_DEV double block_sum(double v, double *red, int tid) {
    v = wave_sum(v);
    __syncthreads();  // red is free
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < RANSAC_FIN / 64; ++k) s += red[k];
    return s;
}

// The refit (algorithms/FR.py:101-114): one unit-weight fp64 Kabsch over the
// rows with d^2 < r2 under c, centred, in a fixed order; c <- the new pose, the
// same bits in every thread.  n: the inlier count (already summed over the
// workgroup), sa / sb: this thread's partial coordinate sums over its inliers.
// refit_kabsch_rows: the same over the rows a predicate selects (f10's labelled
// rows); sel(i, a, b) must give what it gave when n, sa and sb were summed.
template <typename Sel>
PDSC_DEV void refit_kabsch_rows(const float *__restrict__ src, const float *__restrict__ tgt, int N, double n,
                                double sa[3], double sb[3], double c[12], double *red, int tid, const Sel &sel) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sa[k] = block_sum(sa[k], red, tid);
        sb[k] = block_sum(sb[k], red, tid);
    }
    const double inv = 1.0 / n;
    const D3 ca = d3(sa[0] * inv, sa[1] * inv, sa[2] * inv), cb = d3(sb[0] * inv, sb[1] * inv, sb[2] * inv);
    double Hm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hm[k] = 0.0;
    for (int i = tid; i < N; i += RANSAC_FIN) {
        const D3 a0 = load3(src, i), b0 = load3(tgt, i);
        if (sel(i, a0, b0)) {
            const D3 a = sub3(a0, ca), b = sub3(b0, cb);
            Hm[0] += a.x * b.x;
            Hm[1] += a.x * b.y;
            Hm[2] += a.x * b.z;
            Hm[3] += a.y * b.x;
            Hm[4] += a.y * b.y;
            Hm[5] += a.y * b.z;
            Hm[6] += a.z * b.x;
            Hm[7] += a.z * b.y;
            Hm[8] += a.z * b.z;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Hm[k] = block_sum(Hm[k], red, tid);
    double Rf[9];
    kabsch_rotation_svd(Hm, Rf);
    kabsch_pose(Rf, ca, cb, c);  // every thread: the same bits
}

PDSC_DEV void refit_kabsch(const float *__restrict__ src, const float *__restrict__ tgt, int N, double r2, double n,
                           double sa[3], double sb[3], double c[12], double *red, int tid) {
    double c0[12];  // the pose the inliers are taken under (c is overwritten at the end)
#pragma unroll
    for (int k = 0; k < 12; ++k) c0[k] = c[k];
    refit_kabsch_rows(src, tgt, N, n, sa, sb, c, red, tid, [&c0, r2](int, const D3 &a, const D3 &b) {
        return ransac_d2(c0, a.x, a.y, a.z, b.x, b.y, b.z) < r2;
    });
}

}  // namespace pdsc
