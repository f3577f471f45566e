// posegraph.hip -- f12: pose-graph optimisation on the GPU, the step of multiway
// registration that throws out false loop closures (multiway/test_multi_ate.py:
// 166-174, 217-224: open3d's global_optimization with
// GlobalOptimizationLevenbergMarquardt and a line process).  open3d's algorithm
// restated (open3d is not a dependency; parity with open3d itself is unpinned),
// the choices it leaves open fixed in include/pdsc.h.
//
// The whole two-pass optimisation is ONE launch of ONE workgroup (the precedent
// of icp_one_wg_kernel): a scene has tens of nodes, the system is a few hundred
// unknowns, and every convergence decision would otherwise cost a host round
// trip.  All arithmetic is fp64, there is no float atomic and every sum has a
// fixed order, so two calls are bitwise equal.
//
//   edges     one lane per edge: e = vec6(X^-1 Tt^-1 Ts), Js (Jt = -Js bit for
//             bit: negation commutes with every operation of lin6), and the
//             edge's B = Js^T L Js (r <= c computed, mirrored), g = Js^T L e,
//             q = e^T L e to the workspace
//   assemble  dense H and b: entry (r, c) of node i's row block walks the node's
//             incident-edge list (built once per pass, ascending edge index):
//             H_ii += l B, H_i,other -= l B, b_i -+= l g.  One thread owns an
//             entry, so nothing is atomic and H is symmetric bit for bit
//   solve     blocked right-looking Cholesky of H + lambda I on 6x6 blocks: the
//             diagonal block by one lane, the panel below it one row per lane and
//             staged in LDS (its first PG_PANEL_ROWS rows; the rest is read back
//             from L, L2-resident), the trailing update from the staged panel
//   loop      open3d's Levenberg-Marquardt schedule, every lane carrying the same
//             scalars (the reductions return the same bits to every lane)
#include <cmath>

#include "abi.hpp"
#include "pdsc_common.hpp"
#include "pdsc_internal.hpp"
#include "se3.hpp"

namespace pdsc {

constexpr int PG_MAX_N = 256;          // nodes (one lane per node where a node is the unit of work)
constexpr int PG_MAX_E = 32768;        // edges
constexpr int PG_WG = 256;             // the workgroup
constexpr int PG_PANEL_ROWS = 1024;    // panel rows staged in LDS: 48 KiB of the 64 KiB a static allocation may take
static_assert(PG_MAX_N <= PG_WG, "one lane per node");

struct PgEdges {
    const int *src, *tgt;
    const double *trans, *info;
    const int *unc;
    int E;
};
struct PgBufs {
    double *res, *B, *g, *q, *l;  // per edge: e [6], B [36], g [6], q, the line process
    int *active, *inc_off, *inc;  // per edge: in this pass; per node: its incident edges [inc_off[i], inc_off[i+1])
    double *H, *L, *b, *trial;    // [6n,6n] x 2, [6n], trial poses [n,16]
    int *err;
};
struct PgParams {
    int n, reference, max_iter, max_iter_lm;
    double min_rel_inc, min_rel_res_inc, min_right, min_res;
    double mu_scale;  // preference_loop_closure * max_correspondence_distance^2
    double prune;
};

static void bind_pg(Carve &c, int n, int E, PgBufs &W) {
    const size_t e = (size_t)(E > 0 ? E : 1), n6 = 6 * (size_t)n;
    W.res = c.take<double>(6 * e);
    W.B = c.take<double>(36 * e);
    W.g = c.take<double>(6 * e);
    W.q = c.take<double>(e);
    W.l = c.take<double>(e);
    W.active = c.take<int>(e);
    W.inc_off = c.take<int>((size_t)n + 1);
    W.inc = c.take<int>(2 * e);
    W.H = c.take<double>(n6 * n6);
    W.L = c.take<double>(n6 * n6);
    W.b = c.take<double>(n6);
    W.trial = c.take<double>(16 * (size_t)n);
    W.err = c.take<int>(1);
}

// open3d's TransformMatrix4dToVector6d, with its singular branch
PDSC_DEV void vec6(const double (&M)[12], double (&v)[6]) {
    const double sy = sqrt(M[0] * M[0] + M[4] * M[4]);
    if (!(sy < 1e-6)) {
        v[0] = atan2(M[9], M[10]);
        v[1] = atan2(-M[8], sy);
        v[2] = atan2(M[4], M[0]);
    } else {
        v[0] = atan2(-M[6], M[5]);
        v[1] = atan2(-M[8], sy);
        v[2] = 0.0;
    }
    v[3] = M[3];
    v[4] = M[7];
    v[5] = M[11];
}

// The workgroup's sum / maximum of one value per lane, the same bits in every
// lane: xor shuffles inside the waves, the four waves in order through red [4].
PDSC_DEV double pg_sum(double v, double *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
PDSC_DEV double pg_max(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// One edge at `poses`: returns q = e^T L e; FULL also stores e, B, g and q.
template <bool FULL>
PDSC_DEV double pg_edge(const PgEdges &G, const PgBufs &W, const double *poses, int e) {
    double Ts[12], Tt[12], X[12], Xi[12], Ti[12], A[12], M[12], r[6], we[6];
    aff_load(poses + 16 * (size_t)G.src[e], Ts);
    aff_load(poses + 16 * (size_t)G.tgt[e], Tt);
    aff_load(G.trans + 16 * (size_t)e, X);
    aff_inv(X, Xi);
    aff_inv(Tt, Ti);
    aff_mul(Xi, Ti, A);
    aff_mul(A, Ts, M);
    vec6(M, r);
    const double *__restrict__ Lm = G.info + 36 * (size_t)e;
    double q = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += Lm[6 * p + k] * r[k];
        we[p] = s;
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) q += r[p] * we[p];
    if (!FULL) return q;
    // Js: column i = lin6(A D_i Ts); D_i Ts is a selection of Ts's rows
    double J[36];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double Gm[12], Mi[12];
        const int a = (i + 1) % 3, b = (i + 2) % 3;  // D_i: row b <- row a, row a <- -row b
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            Gm[4 * i + c] = 0.0;
            Gm[4 * a + c] = -Ts[4 * b + c];
            Gm[4 * b + c] = Ts[4 * a + c];
        }
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                Mi[4 * rr + c] = (A[4 * rr] * Gm[c] + A[4 * rr + 1] * Gm[4 + c]) + A[4 * rr + 2] * Gm[8 + c];
        J[i] = (Mi[9] - Mi[6]) / 2.0;
        J[6 + i] = (Mi[2] - Mi[8]) / 2.0;
        J[12 + i] = (Mi[4] - Mi[1]) / 2.0;
        J[18 + i] = Mi[3];
        J[24 + i] = Mi[7];
        J[30 + i] = Mi[11];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // translations: A D_(3+i) Ts has only column 3 = A's column i
        J[3 + i] = 0.0;
        J[9 + i] = 0.0;
        J[15 + i] = 0.0;
        J[21 + i] = A[i];
        J[27 + i] = A[4 + i];
        J[33 + i] = A[8 + i];
    }
    double *__restrict__ Bo = W.B + 36 * (size_t)e;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double w[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += Lm[6 * p + k] * J[6 * k + c];
            w[p] = s;
        }
#pragma unroll
        for (int rr = 0; rr <= c; ++rr) {
            double s = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p) s += J[6 * p + rr] * w[p];
            Bo[6 * rr + c] = s;
            Bo[6 * c + rr] = s;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) s += J[6 * p + rr] * we[p];
        W.g[6 * (size_t)e + rr] = s;
        W.res[6 * (size_t)e + rr] = r[rr];
    }
    W.q[e] = q;
    return q;
}

// Validates the edge ids (workgroup-uniform result), marks every edge active.
PDSC_DEV bool pg_bad_edges(const PgEdges &G, int n) {
    int bad = 0;
    for (int e = threadIdx.x; e < G.E; e += PG_WG) {
        const int s = G.src[e], t = G.tgt[e];
        bad |= (s < 0 || s >= n || t < 0 || t >= n || s == t);
    }
    return __syncthreads_or(bad) != 0;
}

// The incident-edge lists of the active edges: lane i walks the edges in
// ascending order for node i (count, one lane's scan, fill).
PDSC_DEV void pg_incidence(const PgEdges &G, const PgBufs &W, int n) {
    const int i = threadIdx.x;
    int cnt = 0;
    if (i < n)
        for (int e = 0; e < G.E; ++e) cnt += W.active[e] && (G.src[e] == i || G.tgt[e] == i);
    if (i < n) W.inc_off[i + 1] = cnt;
    __syncthreads();
    if (i == 0) {
        W.inc_off[0] = 0;
        for (int k = 0; k < n; ++k) W.inc_off[k + 1] += W.inc_off[k];
    }
    __syncthreads();
    if (i < n) {
        int o = W.inc_off[i];
        for (int e = 0; e < G.E; ++e)
            if (W.active[e] && (G.src[e] == i || G.tgt[e] == i)) W.inc[o++] = e;
    }
    __syncthreads();
}

PDSC_DEV void pg_edges_full(const PgEdges &G, const PgBufs &W, const double *poses) {
    for (int e = threadIdx.x; e < G.E; e += PG_WG)
        if (W.active[e]) pg_edge<true>(G, W, poses, e);
    __syncthreads();
}

// l from the stored q: 1 for certain edges, (mu / (mu + q))^2 for uncertain ones (1 where mu + q is not positive)
PDSC_DEV void pg_line_process(const PgEdges &G, const PgBufs &W, double mu) {
    for (int e = threadIdx.x; e < G.E; e += PG_WG)
        if (W.active[e]) {
            double l = 1.0;
            if (G.unc[e]) {
                const double den = mu + W.q[e];
                const double f = den > 0.0 ? mu / den : 1.0;
                l = f * f;
            }
            W.l[e] = l;
        }
    __syncthreads();
}

// F = sum l q + mu sum over uncertain edges (sqrt(l) - 1)^2; q from the store, or of `poses` when given
PDSC_DEV double pg_objective(const PgEdges &G, const PgBufs &W, const double *l, double mu, const double *poses,
                             double *red) {
    double acc = 0.0;
    for (int e = threadIdx.x; e < G.E; e += PG_WG)
        if (W.active[e]) {
            const double le = l ? l[e] : 1.0;
            const double q = poses ? pg_edge<false>(G, W, poses, e) : W.q[e];
            acc += le * q;
            if (G.unc[e]) {
                const double d = sqrt(le) - 1.0;
                acc += mu * (d * d);
            }
        }
    return pg_sum(acc, red);
}

// Dense H [6n,6n] and b [6n] from the stored B and g under l; the reference node's rows and columns the identity's.
PDSC_DEV void pg_assemble(const PgEdges &G, const PgBufs &W, const double *l, int n, int ref, double *H, double *b) {
    const int n6 = 6 * n;
    for (size_t k = threadIdx.x; k < (size_t)n6 * n6; k += PG_WG) H[k] = 0.0;
    __syncthreads();
    for (int w = threadIdx.x; w < 42 * n; w += PG_WG) {
        const int i = w / 42, k = w % 42;
        const int lo = W.inc_off[i], hi = W.inc_off[i + 1];
        if (k < 36) {
            const int r = k / 6, c = k % 6;
            double *row = H + (size_t)(6 * i + r) * n6;
            double diag = 0.0;
            for (int u = lo; u < hi; ++u) {
                const int e = W.inc[u];
                const int s = G.src[e], other = s == i ? G.tgt[e] : s;
                const double v = (l ? l[e] : 1.0) * W.B[36 * (size_t)e + k];
                diag += v;
                row[6 * other + c] -= v;
            }
            row[6 * i + c] = diag;
        } else {
            const int r = k - 36;
            double acc = 0.0;
            for (int u = lo; u < hi; ++u) {
                const int e = W.inc[u];
                const double v = (l ? l[e] : 1.0) * W.g[6 * (size_t)e + r];
                if (G.src[e] == i)
                    acc -= v;
                else
                    acc += v;
            }
            b[6 * i + r] = acc;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 6 * n6; k += PG_WG) {
        const int r = 6 * ref + k / n6, c = k % n6;
        H[(size_t)r * n6 + c] = r == c ? 1.0 : 0.0;
        H[(size_t)c * n6 + r] = r == c ? 1.0 : 0.0;
    }
    if (threadIdx.x < 6) b[6 * ref + threadIdx.x] = 0.0;
    __syncthreads();
}

// (H + lam I) y = b by the blocked Cholesky; y [6n] in LDS holds the solution.
// Returns false (workgroup-uniform) on a pivot that is not positive and finite.
PDSC_DEV bool pg_solve(const PgBufs &W, int n, double lam, double *panel, double *y, double *Ldd, int *flag) {
    const int n6 = 6 * n, tid = threadIdx.x;
    double *L = W.L;
    for (size_t k = tid; k < (size_t)n6 * n6; k += PG_WG) {
        const int i = (int)(k / n6), j = (int)(k % n6);
        if (j <= i) L[k] = i == j ? W.H[k] + lam : W.H[k];
    }
    for (int k = tid; k < n6; k += PG_WG) y[k] = W.b[k];
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int kb = 0; kb < n; ++kb) {
        const int c0 = 6 * kb;
        if (tid == 0) {  // the diagonal block, unblocked, in LDS
            bool ok = true;
            for (int j = 0; j < 6; ++j) {
                double d = L[(size_t)(c0 + j) * n6 + c0 + j];
                for (int m = 0; m < j; ++m) d -= Ldd[6 * j + m] * Ldd[6 * j + m];
                if (!(d > 0.0) || !(d <= 1.79769313486231570e308)) ok = false;
                const double p = sqrt(d);
                Ldd[6 * j + j] = p;
                for (int i = j + 1; i < 6; ++i) {
                    double s = L[(size_t)(c0 + i) * n6 + c0 + j];
                    for (int m = 0; m < j; ++m) s -= Ldd[6 * i + m] * Ldd[6 * j + m];
                    Ldd[6 * i + j] = s / p;
                }
            }
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j <= i; ++j) L[(size_t)(c0 + i) * n6 + c0 + j] = Ldd[6 * i + j];
            if (!ok) *flag = 1;
        }
        __syncthreads();
        if (*flag) return false;
        const int m = n6 - c0 - 6;  // rows below the block
        for (int rr = tid; rr < m; rr += PG_WG) {  // the panel: row (c0 + 6 + rr) times Ldd^-T
            double *row = L + (size_t)(c0 + 6 + rr) * n6 + c0;
            double x[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double s = row[j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= x[k] * Ldd[6 * j + k];
                x[j] = s / Ldd[6 * j + j];
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                row[j] = x[j];
                if (rr < PG_PANEL_ROWS) panel[6 * rr + j] = x[j];
            }
        }
        __syncthreads();
        const int mb = m / 6;  // the trailing update: row i of block column bj, 6 entries
        for (int w = tid; w < m * mb; w += PG_WG) {
            const int i = w / mb, bj = w % mb;
            if (bj > i / 6) continue;
            const double *pi = i < PG_PANEL_ROWS ? panel + 6 * i : L + (size_t)(c0 + 6 + i) * n6 + c0;
            double a[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] = pi[k];
            double *out = L + (size_t)(c0 + 6 + i) * n6 + c0 + 6 + 6 * bj;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                const int j = 6 * bj + jj;
                if (j > i) break;
                const double *pj = j < PG_PANEL_ROWS ? panel + 6 * j : L + (size_t)(c0 + 6 + j) * n6 + c0;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) s += a[k] * pj[k];
                out[jj] -= s;
            }
        }
        __syncthreads();
    }
    for (int kb = 0; kb < n; ++kb) {  // L z = b
        const int c0 = 6 * kb;
        if (tid == 0)
            for (int j = 0; j < 6; ++j) {
                double s = y[c0 + j];
                for (int k = 0; k < j; ++k) s -= L[(size_t)(c0 + j) * n6 + c0 + k] * y[c0 + k];
                y[c0 + j] = s / L[(size_t)(c0 + j) * n6 + c0 + j];
            }
        __syncthreads();
        for (int r = c0 + 6 + tid; r < n6; r += PG_WG) {
            const double *row = L + (size_t)r * n6 + c0;
            double s = y[r];
#pragma unroll
            for (int j = 0; j < 6; ++j) s -= row[j] * y[c0 + j];
            y[r] = s;
        }
        __syncthreads();
    }
    for (int kb = n - 1; kb >= 0; --kb) {  // L^T y = z
        const int c0 = 6 * kb;
        if (tid == 0)
            for (int j = 5; j >= 0; --j) {
                double s = y[c0 + j];
                for (int k = j + 1; k < 6; ++k) s -= L[(size_t)(c0 + k) * n6 + c0 + j] * y[c0 + k];
                y[c0 + j] = s / L[(size_t)(c0 + j) * n6 + c0 + j];
            }
        __syncthreads();
        for (int r = tid; r < c0; r += PG_WG) {
            double s = y[r];
#pragma unroll
            for (int j = 0; j < 6; ++j) s -= L[(size_t)(c0 + j) * n6 + r] * y[c0 + j];
            y[r] = s;
        }
        __syncthreads();
    }
    return true;
}

// trial_i = Exp(delta_i) pose_i, Exp(d) = Rz(d2) Ry(d1) Rx(d0) with translation d3..5 (lane i, node i)
PDSC_DEV void pg_trial(const double *poses, const double *delta, double *trial, int n) {
    const int i = threadIdx.x;
    if (i < n) {
        const double *d = delta + 6 * i;
        double Ex[12], P[12], Q[12];
        se3_exp(d, Ex);
        aff_load(poses + 16 * (size_t)i, P);
        aff_mul(Ex, P, Q);
#pragma unroll
        for (int k = 0; k < 12; ++k) trial[16 * (size_t)i + k] = Q[k];
        trial[16 * (size_t)i + 12] = 0.0;
        trial[16 * (size_t)i + 13] = 0.0;
        trial[16 * (size_t)i + 14] = 0.0;
        trial[16 * (size_t)i + 15] = 1.0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PG_WG) void pg_optimize_kernel(double *poses, PgEdges G, PgBufs W, PgParams P,
                                                            double *confidence, int *keep,
                                                            pdsc_pose_graph_result *res) {
    __shared__ double panel[6 * PG_PANEL_ROWS];
    __shared__ double y[6 * PG_MAX_N];
    __shared__ double red[4];
    __shared__ double Ldd[36];
    __shared__ int flag;
    const int tid = threadIdx.x, n = P.n, n6 = 6 * n;
    if (tid == 0) {
        for (int p = 0; p < 2; ++p) {
            res->objective[p] = 0.0;
            res->mu[p] = 0.0;
            res->iterations[p] = 0;
        }
        res->edges_kept = 0;
        res->solver_failed = 0;
        *W.err = 0;
    }
    if (pg_bad_edges(G, n)) {
        if (tid == 0) *W.err = 1;
        return;
    }
    int failed = 0;
    for (int pass = 0; pass < 2 && !failed; ++pass) {
        for (int e = tid; e < G.E; e += PG_WG) W.active[e] = pass == 0 ? 1 : keep[e];
        __syncthreads();
        pg_incidence(G, W, n);
        double s55 = 0.0, cnt = 0.0;
        for (int e = tid; e < G.E; e += PG_WG)
            if (W.active[e] && G.unc[e]) {
                s55 += G.info[36 * (size_t)e + 35];
                cnt += 1.0;
            }
        s55 = pg_sum(s55, red);
        cnt = pg_sum(cnt, red);
        const double mu = cnt > 0.0 ? P.mu_scale * (s55 / cnt) : 0.0;
        pg_edges_full(G, W, poses);
        pg_line_process(G, W, mu);
        double F = pg_objective(G, W, W.l, mu, nullptr, red);
        pg_assemble(G, W, W.l, n, P.reference, W.H, W.b);
        double maxd = 0.0, maxb = -1.79769313486231570e308;
        for (int k = tid; k < n6; k += PG_WG) {
            maxd = fmax(maxd, W.H[(size_t)k * n6 + k]);
            maxb = fmax(maxb, W.b[k]);
        }
        maxd = pg_max(maxd, red);
        maxb = pg_max(maxb, red);
        double lam = 1e-5 * maxd, nu = 2.0;
        bool stop = maxb < P.min_right || F < P.min_res;
        int iter = 0;
        while (!stop && iter < P.max_iter) {
            int lm = 0;
            double rho = 0.0;
            do {
                if (!pg_solve(W, n, lam, panel, y, Ldd, &flag)) {
                    failed = 1;
                    stop = true;
                    break;
                }
                double dn = 0.0, xn = 0.0;
                for (int k = tid; k < n6; k += PG_WG) dn += y[k] * y[k];
                if (tid < n) {
                    double T[12], v[6];
                    aff_load(poses + 16 * (size_t)tid, T);
                    vec6(T, v);
#pragma unroll
                    for (int k = 0; k < 6; ++k) xn += v[k] * v[k];
                }
                dn = sqrt(pg_sum(dn, red));
                xn = sqrt(pg_sum(xn, red));
                if (dn < P.min_rel_inc * (xn + P.min_rel_inc)) {
                    stop = true;
                } else {
                    pg_trial(poses, y, W.trial, n);
                    const double Fn = pg_objective(G, W, W.l, mu, W.trial, red);
                    double den = 0.0;
                    for (int k = tid; k < n6; k += PG_WG) den += y[k] * (lam * y[k] + W.b[k]);
                    den = pg_sum(den, red) + 1e-3;
                    rho = (F - Fn) / den;
                    if (rho > 0.0) {
                        if (F - Fn < P.min_rel_res_inc * F) {
                            stop = true;
                        } else {
                            for (int k = tid; k < 16 * n; k += PG_WG) poses[k] = W.trial[k];
                            __syncthreads();
                            pg_edges_full(G, W, poses);
                            pg_line_process(G, W, mu);
                            F = pg_objective(G, W, W.l, mu, nullptr, red);
                            pg_assemble(G, W, W.l, n, P.reference, W.H, W.b);
                            const double a = 2.0 * rho - 1.0;
                            lam *= fmax(1.0 / 3.0, 1.0 - a * a * a);
                            nu = 2.0;
                            double mb = -1.79769313486231570e308;
                            for (int k = tid; k < n6; k += PG_WG) mb = fmax(mb, W.b[k]);
                            if (pg_max(mb, red) < P.min_right) stop = true;
                        }
                    } else {
                        lam *= nu;
                        nu *= 2.0;
                    }
                }
                if (++lm > P.max_iter_lm) stop = true;
            } while (!(rho > 0.0 || stop));
            ++iter;
            if (F < P.min_res) stop = true;
        }
        int kept = 0;
        for (int e = tid; e < G.E; e += PG_WG)
            if (W.active[e]) {
                confidence[e] = W.l[e];
                if (pass == 0) keep[e] = !G.unc[e] || W.l[e] > P.prune;
                kept += keep[e];
            }
        const double nk = pg_sum((double)kept, red);
        if (tid == 0) {
            res->objective[pass] = F;
            res->mu[pass] = mu;
            res->iterations[pass] = iter;
            res->edges_kept = (int)nk;
            res->solver_failed = failed;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PG_WG) void pg_linearize_kernel(const double *poses, PgEdges G, PgBufs W, int n, int ref,
                                                             const double *l, double mu, double *residual,
                                                             double *objective, double *H, double *b) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    if (tid == 0) *W.err = 0;
    if (pg_bad_edges(G, n)) {
        if (tid == 0) *W.err = 1;
        return;
    }
    for (int e = tid; e < G.E; e += PG_WG) W.active[e] = 1;
    __syncthreads();
    pg_incidence(G, W, n);
    pg_edges_full(G, W, poses);
    const double F = pg_objective(G, W, l, mu, nullptr, red);
    pg_assemble(G, W, l, n, ref, H, b);
    for (int k = tid; k < 6 * G.E; k += PG_WG) residual[k] = W.res[k];
    if (tid == 0) *objective = F;
}

static int pg_check(int n, int E, int ref, const void *poses, const void *es, const void *et, const void *tr,
                    const void *info, const void *unc) {
    if (n < 1 || E < 0) return fail(PDSC_ERR_ARG, "n=%d E=%d (need n >= 1, E >= 0)", n, E);
    if (n > PG_MAX_N || E > PG_MAX_E)
        return fail(PDSC_ERR_UNSUPPORTED, "n=%d E=%d above the caps %d nodes, %d edges", n, E, PG_MAX_N, PG_MAX_E);
    if (ref < 0 || ref >= n) return fail(PDSC_ERR_ARG, "reference_node=%d outside [0, %d)", ref, n);
    if (!poses || (E > 0 && (!es || !et || !tr || !info || !unc))) return fail(PDSC_ERR_ARG, "null pointer");
    return PDSC_OK;
}

static int pg_status(const PgBufs &W, hipStream_t s) {
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, W.err, sizeof e, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (e) return fail(PDSC_ERR_ARG, "an edge with source == target or a node id outside [0, n)");
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_pose_graph_workspace_bytes(int32_t n, int32_t E) {
    if (n < 1 || E < 0 || n > PG_MAX_N || E > PG_MAX_E) return 0;
    Carve c(nullptr);
    PgBufs W;
    bind_pg(c, n, E, W);
    return c.off;
}

int32_t pdsc_pose_graph_optimize(double *poses, int32_t n, const int32_t *edge_src, const int32_t *edge_tgt,
                                 const double *edge_trans, const double *edge_info, const int32_t *edge_uncertain,
                                 int32_t E, const pdsc_pose_graph_options *options,
                                 const pdsc_pose_graph_criteria *criteria, double *confidence, int32_t *edge_keep,
                                 pdsc_pose_graph_result *result, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (!options) return fail(PDSC_ERR_ARG, "null pointer (options)");
    RET_IF(pg_check(n, E, options->reference_node, poses, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain));
    if (!result || !ws || (E > 0 && (!confidence || !edge_keep))) return fail(PDSC_ERR_ARG, "null pointer");
    const double d = options->max_correspondence_distance, pref = options->preference_loop_closure;
    if (!(d > 0.0) || !std::isfinite(d))
        return fail(PDSC_ERR_ARG, "max_correspondence_distance %g must be > 0 and finite", d);
    if (!(pref >= 0.0) || !std::isfinite(pref))
        return fail(PDSC_ERR_ARG, "preference_loop_closure %g must be >= 0 and finite", pref);
    if (!std::isfinite(options->edge_prune_threshold))
        return fail(PDSC_ERR_ARG, "edge_prune_threshold must be finite");
    pdsc_pose_graph_criteria cr = {PDSC_PG_MAX_ITERATION,           PDSC_PG_MAX_ITERATION_LM,
                                   PDSC_PG_MIN_RELATIVE_INCREMENT,  PDSC_PG_MIN_RELATIVE_RESIDUAL_INCREMENT,
                                   PDSC_PG_MIN_RIGHT_TERM,          PDSC_PG_MIN_RESIDUAL};
    if (criteria) cr = *criteria;
    if (cr.max_iteration < 0 || cr.max_iteration_lm < 0)
        return fail(PDSC_ERR_ARG, "max_iteration=%d max_iteration_lm=%d", cr.max_iteration, cr.max_iteration_lm);
    RET_IF(need_ws(ws_bytes, pdsc_pose_graph_workspace_bytes(n, E)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    PgBufs W;
    bind_pg(c, n, E, W);
    const PgEdges G = {edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain, E};
    const PgParams P = {n,
                        options->reference_node,
                        cr.max_iteration,
                        cr.max_iteration_lm,
                        cr.min_relative_increment,
                        cr.min_relative_residual_increment,
                        cr.min_right_term,
                        cr.min_residual,
                        pref * d * d,
                        options->edge_prune_threshold};
    hipLaunchKernelGGL(pg_optimize_kernel, dim3(1), dim3(PG_WG), 0, s, poses, G, W, P, confidence, edge_keep, result);
    HIPCHK(hipGetLastError());
    return pg_status(W, s);
}

int32_t pdsc_pose_graph_linearize(const double *poses, int32_t n, const int32_t *edge_src, const int32_t *edge_tgt,
                                  const double *edge_trans, const double *edge_info, const int32_t *edge_uncertain,
                                  int32_t E, const double *line_process, double mu, int32_t reference_node,
                                  double *residual, double *objective, double *H, double *b, void *ws, size_t ws_bytes,
                                  pdsc_stream_t stream) {
    RET_IF(pg_check(n, E, reference_node, poses, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain));
    if (!objective || !H || !b || !ws || (E > 0 && !residual)) return fail(PDSC_ERR_ARG, "null pointer");
    if (!(mu >= 0.0) || !std::isfinite(mu)) return fail(PDSC_ERR_ARG, "mu %g must be >= 0 and finite", mu);
    RET_IF(need_ws(ws_bytes, pdsc_pose_graph_workspace_bytes(n, E)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    PgBufs W;
    bind_pg(c, n, E, W);
    const PgEdges G = {edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain, E};
    hipLaunchKernelGGL(pg_linearize_kernel, dim3(1), dim3(PG_WG), 0, s, poses, G, W, n, reference_node, line_process,
                       mu, residual, objective, H, b);
    HIPCHK(hipGetLastError());
    return pg_status(W, s);
}

}  // extern "C"
