// gc_ransac.hip -- f10: GC-RANSAC (Barath & Matas, CVPR 2018) on correspondences
// in the configuration the fork runs (algorithms/GC_RANSAC.py:8-50,
// baseline_scripts/baseline_3DMatch.py:101-123): neighborhood 0, the grid graph.
// Two rows are neighbours iff they share a cell of the 6-D grid, so the graph is
// a disjoint union of cliques, every edge of a clique carries the same pairwise
// weight, and the minimum cut is exact per cell: sort the cell's rows by residual,
// one prefix sum, an argmin over the number of inliers (include/pdsc.h, f10).
//
//   grid     one workgroup: column extrema, the 64-bit cell keys, a bitonic sort
//            of (key, row) -- in LDS up to GC_GRID_LDS rows, in global memory
//            above -- and a scan of the key changes.  Once per solve.
//   label    the hot kernel.  A workgroup of 4 waves owns 4 consecutive cells.
//            Cells of up to GC_WAVE_CELL = 64 rows: one wave each, a row per lane,
//            the sort by shuffles in registers.  Larger cells: the whole
//            workgroup, one after the other, in LDS up to GC_LDS_CELL = 1024 rows
//            and in a global scratch segment (the cell's own rows of three [N]
//            arrays) above.  The prefix sum is sequential in the sorted order
//            (the definition); the n + 1 energies and their argmin are parallel.
//   solver   f6's hypothesis kernel (ransac_n 3) and its scoring kernel in the
//            MSAC form, a round kernel, ten enqueued LO steps (label, then one
//            workgroup: Kabsch over the labelled rows, score, accept) that return
//            at entry unless the round's best beat the so-far-best, and a fold
//            kernel with the stop rule.  Nothing synchronises; integer atomics
//            only: two calls are bitwise equal.
#include <cmath>

#include "ransac_shared.hpp"

namespace pdsc {

constexpr int GC_MAX_ROWS = 1 << 18;  // as pdsc_gpf_select's limit; also the LDS chunk rows of the one-pose scorer
constexpr int GC_MAX_GRID = 1024;     // cells per axis: 6 axes of 10 bits in the 64-bit key
constexpr int GC_WAVE_CELL = 64;      // cells up to this many rows: one wave, a row per lane
constexpr int GC_LDS_CELL = 1024;     // up to this many: one workgroup in LDS; above: its global scratch
constexpr int GC_GRID_WG = 1024;   // threads of the grid kernel
constexpr int GC_GRID_LDS = 2048;  // rows up to which the grid's sort runs in LDS
constexpr int GC_LABEL_WG = 256;   // threads of the label kernel
constexpr int GC_CELLS_PER_WG = GC_LABEL_WG / 64;
constexpr int GC_LO_STEPS = 10;
constexpr int GC_MAX_CHUNKS = GC_MAX_ROWS / RANSAC_PCHUNK;  // chunk rows of the one-pose scorer (LDS)
static_assert(GC_WAVE_CELL == 64, "a row per lane");
static_assert(RANSAC_FIN == GC_LABEL_WG, "block_sum's workgroup");

PDSC_DEV bool pair_less(u64 ka, int va, u64 kb, int vb) { return ka < kb || (ka == kb && va < vb); }

// Bitonic sort of n (key, val) pairs, any n, by one workgroup of NT threads (n
// workgroup-uniform).  The all-ascending form of the network: the first step of
// a merge of width k pairs i with i ^ (k - 1), the later ones i with i + j.
// Every exchange moves the smaller pair down, so rows past n -- which would hold
// +infinity -- never move and are simply skipped.  key / val: LDS or global.
template <int NT> PDSC_DEV void sort_pairs(u64 *key, int *val, int n, int tid) {
    for (unsigned k = 2; (k >> 1) < (unsigned)n; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = tid;; t += NT) {
                const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // the t-th index with bit j clear
                if (i >= (unsigned)n) break;
                const unsigned l = j == (k >> 1) ? i ^ (k - 1) : i + j;
                if (l < (unsigned)n) {
                    const u64 ki = key[i], kl = key[l];
                    const int vi = val[i], vl = val[l];
                    if (pair_less(kl, vl, ki, vi)) {
                        key[i] = kl, val[i] = vl;
                        key[l] = ki, val[l] = vi;
                    }
                }
            }
            __syncthreads();
        }
}

// The same network on one wave, a pair per lane (lanes past n hold the maximum).
PDSC_DEV void wave_sort(u64 &key, int &val, int lane, int n) {
    for (int k = 2; (k >> 1) < n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int l = j == (k >> 1) ? lane ^ (k - 1) : lane ^ j;
            const u64 ok = __shfl(key, l);
            const int ov = __shfl(val, l);
            const bool take = lane < l ? pair_less(ok, ov, key, val) : pair_less(key, val, ok, ov);
            if (take) key = ok, val = ov;
        }
}

// ------------------------------------------------------------------------ grid
PDSC_DEV u64 gc_axis(float x, float m, float M, int G) {
    if (M == m) return 0;
    const double q = floor(((double)G * ((double)x - (double)m)) / ((double)M - (double)m));
    long long c = (long long)q;
    if (c > G - 1) c = G - 1;
    if (c < 0) c = 0;
    return (u64)c;
}

__global__ __launch_bounds__(GC_GRID_WG) void gc_grid_kernel(const float *__restrict__ src,
                                                             const float *__restrict__ tgt, int N, int G, u64 *gkey,
                                                             int *order, int *cell_start, int *cell_of, int *n_cells) {
    constexpr int NW = GC_GRID_WG / 64;
    __shared__ float smin[6][NW], smax[6][NW];
    __shared__ u64 lkey[GC_GRID_LDS];
    __shared__ int lval[GC_GRID_LDS];
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float mn[6], mx[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) mn[a] = INFINITY, mx[a] = -INFINITY;
    for (int i = tid; i < N; i += GC_GRID_WG)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = src[3 * (size_t)i + a], y = tgt[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], x), mx[a] = fmaxf(mx[a], x);
            mn[3 + a] = fminf(mn[3 + a], y), mx[3 + a] = fmaxf(mx[3 + a], y);
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
        }
        if (lane == 0) smin[a][w] = mn[a], smax[a][w] = mx[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        mn[a] = smin[a][0], mx[a] = smax[a][0];
#pragma unroll
        for (int k = 1; k < NW; ++k) mn[a] = fminf(mn[a], smin[a][k]), mx[a] = fmaxf(mx[a], smax[a][k]);
    }
    const bool in_lds = N <= GC_GRID_LDS;  // workgroup-uniform
    u64 *key = in_lds ? lkey : gkey;
    int *val = in_lds ? lval : order;
    for (int i = tid; i < N; i += GC_GRID_WG) {
        u64 k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) k = k * (u64)G + gc_axis(src[3 * (size_t)i + a], mn[a], mx[a], G);
#pragma unroll
        for (int a = 0; a < 3; ++a) k = k * (u64)G + gc_axis(tgt[3 * (size_t)i + a], mn[3 + a], mx[3 + a], G);
        key[i] = k, val[i] = i;
    }
    __syncthreads();
    sort_pairs<GC_GRID_WG>(key, val, N, tid);
    // cells: the sorted positions where the key changes; a contiguous stripe per thread
    const int per = (N + GC_GRID_WG - 1) / GC_GRID_WG;
    const int lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
    int v = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int before = v - mine, total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        before += k < w ? wsum[k] : 0;
        total += wsum[k];
    }
    int c = before;  // cells that start before this stripe
    for (int i = lo; i < hi; ++i) {
        if (i == 0 || key[i] != key[i - 1]) cell_start[c++] = i;
        const int row = val[i];
        cell_of[row] = c - 1;
        if (in_lds) order[i] = row;
    }
    if (tid == 0) {
        cell_start[total] = N;
        n_cells[0] = total;
    }
}

// ----------------------------------------------------------------------- label
struct GcLabelArgs {
    const double *pose;  // row-major 4x4
    const float *src, *tgt;
    const int *order, *cell_start, *n_cells;
    double den, lambda;  // den = 2 eps^2
    float *labels;
    int *count;  // += the rows labelled 1 (zeroed by the caller)
    pdsc_gc_label_debug dbg;
    u64 *skey;  // [N] the global scratch of cells above GC_LDS_CELL rows
    int *srow;  // [N]
    double *sP;  // [N]
    const int *gate, *done;  // run iff (*gate != 0 or null) and (*done == 0 or null)
};

// E(m) of a cell of n rows: P = the sum of K over the m lowest residuals, S over all
PDSC_DEV double gc_energy(int m, int n, double P, double S, double lam) {
    const double dm = (double)m, dn = (double)n;
    const double u = (dm - 2.0 * P) + S;
    const double a = dm * (dn - dm);
    const double b = (((dn - dm) - 1.0) * 0.5) * (S - P);
    const double c = (dm * (dm - 1.0)) * 0.5;
    const double d = ((dm - 1.0) * 0.5) * P;
    return (1.0 - lam) * u + lam * (((a + b) + c) - d);
}

struct GcMin {  // the lowest energy, its m (ties: the lower m), the second-lowest energy
    double e1;
    int m1;
    double e2;
};
PDSC_DEV void gc_merge(GcMin &a, const GcMin &b) {
    GcMin lo = a, hi = b;
    if (b.e1 < a.e1 || (b.e1 == a.e1 && b.m1 < a.m1)) lo = b, hi = a;
    a.e1 = lo.e1, a.m1 = lo.m1;
    a.e2 = lo.e2 < hi.e1 ? lo.e2 : hi.e1;
}
PDSC_DEV GcMin gc_wave_min(GcMin g) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        GcMin y;
        y.e1 = __shfl_xor(g.e1, o);
        y.m1 = __shfl_xor(g.m1, o);
        y.e2 = __shfl_xor(g.e2, o);
        gc_merge(g, y);
    }
    return g;
}

PDSC_DEV double gc_row_d2(const double c[12], const float *__restrict__ src, const float *__restrict__ tgt, int row) {
    const D3 a = load3(src, row), b = load3(tgt, row);
    return ransac_d2(c, a.x, a.y, a.z, b.x, b.y, b.z);
}

PDSC_DEV void gc_cell_out(const GcLabelArgs &A, int cell, const GcMin &g) {
    atomicAdd(A.count, g.m1);
    if (A.dbg.m_star) A.dbg.m_star[cell] = g.m1;
    if (A.dbg.energy) A.dbg.energy[cell] = g.e1;
    if (A.dbg.energy_gap) A.dbg.energy_gap[cell] = g.e2 - g.e1;
}

__global__ __launch_bounds__(GC_LABEL_WG) void gc_label_kernel(GcLabelArgs A) {
    __shared__ u64 lkey[GC_LDS_CELL];
    __shared__ int lval[GC_LDS_CELL];
    __shared__ double lP[GC_LDS_CELL];
    __shared__ GcMin wmin[GC_CELLS_PER_WG];
    if (A.done && *A.done) return;  // workgroup-uniform
    if (A.gate && !*A.gate) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ncell = *A.n_cells;
    const int cell0 = blockIdx.x * GC_CELLS_PER_WG;
    if (cell0 >= ncell) return;
    double c[12];
    pose12(A.pose, c);
    const double inf = INFINITY;
    // cells of up to 64 rows: a wave each, a row per lane
    if (cell0 + w < ncell) {
        const int cell = cell0 + w, start = A.cell_start[cell], n = A.cell_start[cell + 1] - start;  // wave-uniform
        if (n <= GC_WAVE_CELL) {
            int row = 0x7fffffff;
            u64 key = ~0ull;
            if (lane < n) {
                row = A.order[start + lane];
                const double d2 = gc_row_d2(c, A.src, A.tgt, row);
                key = (u64)__double_as_longlong(d2);  // d2 >= +0: the bits order as the values
                if (A.dbg.d2) A.dbg.d2[row] = d2;
            }
            wave_sort(key, row, lane, n);
            const double K = lane < n ? exp(-(__longlong_as_double((long long)key) / A.den)) : 0.0;
            double acc = 0.0, P = 0.0;
            for (int i = 0; i < n; ++i) {  // sequential in the sorted order
                if (lane == i) P = acc;
                acc += __shfl(K, i);
            }
            const double S = acc;
            if (lane >= n) P = S;
            GcMin g = {inf, 0x7fffffff, inf};
            if (lane <= n) g.e1 = gc_energy(lane, n, P, S, A.lambda), g.m1 = lane;
            if (n == 64 && lane == 0) gc_merge(g, GcMin{gc_energy(64, 64, S, S, A.lambda), 64, inf});
            g = gc_wave_min(g);
            if (lane < n) A.labels[row] = lane < g.m1 ? 1.0f : 0.0f;
            if (lane == 0) gc_cell_out(A, cell, g);
        }
    }
    // larger cells: the workgroup, one cell after the other
    for (int q = 0; q < GC_CELLS_PER_WG && cell0 + q < ncell; ++q) {
        const int cell = cell0 + q, start = A.cell_start[cell], n = A.cell_start[cell + 1] - start;  // uniform
        if (n <= GC_WAVE_CELL) continue;
        const bool in_lds = n <= GC_LDS_CELL;
        u64 *key = in_lds ? lkey : A.skey + start;
        int *val = in_lds ? lval : A.srow + start;
        double *P = in_lds ? lP : A.sP + start;
        __syncthreads();  // the previous cell is done with the LDS
        for (int i = tid; i < n; i += GC_LABEL_WG) {
            const int row = A.order[start + i];
            const double d2 = gc_row_d2(c, A.src, A.tgt, row);
            key[i] = (u64)__double_as_longlong(d2), val[i] = row;
            if (A.dbg.d2) A.dbg.d2[row] = d2;
        }
        __syncthreads();
        sort_pairs<GC_LABEL_WG>(key, val, n, tid);
        for (int i = tid; i < n; i += GC_LABEL_WG) P[i] = exp(-(__longlong_as_double((long long)key[i]) / A.den));
        __syncthreads();
        if (tid == 0) {  // P[i] <- K_0 + .. + K_i, sequential in the sorted order
            double acc = 0.0;
            for (int i = 0; i < n; ++i) {
                acc += P[i];
                P[i] = acc;
            }
        }
        __syncthreads();
        const double S = P[n - 1];
        GcMin g = {inf, 0x7fffffff, inf};
        for (int m = tid; m <= n; m += GC_LABEL_WG)
            gc_merge(g, GcMin{gc_energy(m, n, m ? P[m - 1] : 0.0, S, A.lambda), m, inf});
        g = gc_wave_min(g);
        if (lane == 0) wmin[w] = g;
        __syncthreads();
        g = wmin[0];
#pragma unroll
        for (int k = 1; k < GC_CELLS_PER_WG; ++k) gc_merge(g, wmin[k]);
        for (int i = tid; i < n; i += GC_LABEL_WG) A.labels[val[i]] = i < g.m1 ? 1.0f : 0.0f;
        if (tid == 0) gc_cell_out(A, cell, g);
    }
}

// ---------------------------------------------------------------------- solver
struct GcState {
    double c[12];  // the so-far-best model: R row-major [9], t [3]
    double score;
    int count, best;
    double rc[12];  // the round's best, then the LO's current model
    double rscore;
    int rcount, rbest;
    double T[16];  // rc as the row-major 4x4 the label kernel reads
    int rvalid, lo_active, iterations, lo_runs, lo_steps, n_lab;
};

__global__ __launch_bounds__(256) void gc_init_kernel(GcState *st, RansacState *rs, int H, int *dbg_count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    debug_prefill(dbg_count, H, i);
    if (i == 0) {
        for (int k = 0; k < 12; ++k) st->c[k] = st->rc[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        pose16(st->c, st->T);
        st->score = st->rscore = -1.0;
        st->count = st->rcount = -1;
        st->best = st->rbest = -1;
        st->rvalid = st->lo_active = st->iterations = st->lo_runs = st->lo_steps = st->n_lab = 0;
        rs->done = 0;
    }
}

// (score desc, h asc): a total order over distinct h, so the shape of
// round_best's reduction tree cannot change the winner
struct GcBetter {
    PDSC_DEV bool operator()(const Cand &a, const Cand &b) const { return a.s > b.s || (a.s == b.s && a.h < b.h); }
};

__global__ __launch_bounds__(RANSAC_FIN) void gc_round_kernel(int nwg, int nchunks, int round, int H, int lo,
                                                              RansacBufs B, GcState *st, pdsc_ransac_debug dbg) {
    __shared__ Cand wbest[RANSAC_FIN / 64];
    if (B.st->done) return;  // workgroup-uniform
    const int tid = threadIdx.x;
    int total;
    const Cand best = round_best(B, nwg, nchunks, dbg, Cand{-1.0, -1, 0x7fffffff, 0}, wbest, tid, total, GcBetter{});
    if (tid != 0) return;
    st->rvalid = 0;
    st->lo_active = 0;
    st->n_lab = 0;
    if (best.cnt >= 0 && best.s > st->score) {
        for (int k = 0; k < 12; ++k) st->rc[k] = B.coef[(size_t)k * RANSAC_ROUND + best.slot];
        pose16(st->rc, st->T);
        st->rscore = best.s;
        st->rcount = best.cnt;
        st->rbest = best.h;
        st->rvalid = 1;
        if (lo) {
            st->lo_active = 1;
            st->lo_runs += 1;
        }
    }
    const long long drawn = ((long long)round + 1) * RANSAC_ROUND;
    st->iterations = drawn < (long long)H ? (int)drawn : H;
}

// One LO step after its labelling: Kabsch over the labelled rows, the MSAC score
// of the new pose in the scoring kernel's order (chunks of RANSAC_PCHUNK rows,
// each summed in row order, then the chunks in order), accept iff it is higher.
__global__ __launch_bounds__(RANSAC_FIN) void gc_lo_kernel(const float *__restrict__ src,
                                                           const float *__restrict__ tgt, int N, double r2,
                                                           const float *__restrict__ labels, const RansacState *rs,
                                                           GcState *st) {
    __shared__ double red[RANSAC_FIN / 64];
    __shared__ double csum[GC_MAX_CHUNKS];
    __shared__ int ccnt[GC_MAX_CHUNKS];
    if (rs->done) return;  // workgroup-uniform
    if (!st->lo_active) return;
    const int tid = threadIdx.x;
    const int n_lab = st->n_lab;
    __syncthreads();  // every thread has read the state
    if (tid == 0) {
        st->n_lab = 0;
        st->lo_steps += 1;
        if (n_lab < 3) st->lo_active = 0;
    }
    if (n_lab < 3) return;
    double n = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    for (int i = tid; i < N; i += RANSAC_FIN)
        if (labels[i] > 0.5f) {
            const D3 a = load3(src, i), b = load3(tgt, i);
            n += 1.0;
            sa[0] += a.x, sa[1] += a.y, sa[2] += a.z;
            sb[0] += b.x, sb[1] += b.y, sb[2] += b.z;
        }
    n = block_sum(n, red, tid);
    double c[12];
    refit_kabsch_rows(src, tgt, N, n, sa, sb, c, red, tid,
                      [labels](int i, const D3 &, const D3 &) { return labels[i] > 0.5f; });
    const int nchunks = (N + RANSAC_PCHUNK - 1) / RANSAC_PCHUNK;
    for (int ch = tid; ch < nchunks; ch += RANSAC_FIN) {
        const int p0 = ch * RANSAC_PCHUNK, p1 = p0 + RANSAC_PCHUNK < N ? p0 + RANSAC_PCHUNK : N;
        int cnt = 0;
        double ss = 0.0;
        for (int p = p0; p < p1; ++p) {
            const double d2 = gc_row_d2(c, src, tgt, p);
            if (d2 < r2) {
                cnt += 1;
                ss += 1.0 - d2 / r2;
            }
        }
        csum[ch] = ss, ccnt[ch] = cnt;
    }
    __syncthreads();
    if (tid != 0) return;
    int cnt = 0;
    double sc = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) cnt += ccnt[ch], sc += csum[ch];
    if (sc > st->rscore) {
        for (int k = 0; k < 12; ++k) st->rc[k] = c[k];
        pose16(c, st->T);
        st->rscore = sc;
        st->rcount = cnt;
    } else {
        st->lo_active = 0;
    }
}

// The end of a round: the round's best (after its LO) becomes the so-far-best; the stop rule.
__global__ void gc_fold_kernel(int N, int round, double confidence, RansacState *rs, GcState *st) {
    if (rs->done || threadIdx.x != 0) return;
    if (st->rvalid) {
        for (int k = 0; k < 12; ++k) st->c[k] = st->rc[k];
        st->score = st->rscore;
        st->count = st->rcount;
        st->best = st->rbest;
    }
    st->rvalid = 0;
    st->lo_active = 0;
    if (confidence_stop(st->count, N, 3, ((long long)round + 1) * RANSAC_ROUND, confidence)) rs->done = 1;
}

// labels and count of the so-far-best under d^2 < r2, then pdsc_refit_inliers' fit over them
__global__ __launch_bounds__(RANSAC_FIN) void gc_finish_kernel(const float *__restrict__ src,
                                                               const float *__restrict__ tgt, int N, double r2,
                                                               const GcState *st, const int *n_cells,
                                                               float *trans_f32, float *labels,
                                                               pdsc_gc_ransac_result *res) {
    __shared__ double red[RANSAC_FIN / 64];
    const int tid = threadIdx.x;
    const int count = st->count;  // -1: no valid hypothesis (c is the identity)
    double c[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = st->c[k];
    double n = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    label_inliers(src, tgt, N, c, r2, count >= 0, labels, n, sa, sb, tid);
    n = block_sum(n, red, tid);  // workgroup-uniform
    if (n >= 3.0) refit_kabsch(src, tgt, N, r2, n, sa, sb, c, red, tid);
    if (tid != 0) return;
    double T[16];
    pose16(c, T);
    if (res) {
        for (int i = 0; i < 16; ++i) res->trans[i] = T[i];
        res->score = count >= 0 ? st->score : 0.0;
        res->n_inliers = count > 0 ? count : 0;
        res->iterations = st->iterations;
        res->best = st->best;
        res->lo_runs = st->lo_runs;
        res->lo_steps = st->lo_steps;
        res->n_cells = n_cells ? n_cells[0] : 0;
    }
    if (trans_f32)
        for (int i = 0; i < 16; ++i) trans_f32[i] = (float)T[i];
}

// ------------------------------------------------------------------- launchers
// the grid kernel's scratch: the keys of the in-global-memory sort
static u64 *bind_gc_grid(Carve &c, int N) { return c.take<u64>((size_t)N); }

static hipError_t gc_grid_enqueue(const float *src, const float *tgt, int N, int G, u64 *gkey, int *order,
                                  int *cell_start, int *cell_of, int *n_cells, hipStream_t s) {
    hipLaunchKernelGGL(gc_grid_kernel, dim3(1), dim3(GC_GRID_WG), 0, s, src, tgt, N, G, gkey, order, cell_start,
                       cell_of, n_cells);
    return hipGetLastError();
}

// the label kernel's scratch for cells above GC_LDS_CELL rows
static void bind_gc_label(Carve &c, int N, GcLabelArgs &A) {
    A.skey = c.take<u64>((size_t)N);
    A.srow = c.take<int>((size_t)N);
    A.sP = c.take<double>((size_t)N);
}

static hipError_t gc_label_enqueue(const GcLabelArgs &A, int N, hipStream_t s) {
    hipLaunchKernelGGL(gc_label_kernel, dim3((N + GC_CELLS_PER_WG - 1) / GC_CELLS_PER_WG), dim3(GC_LABEL_WG), 0, s, A);
    return hipGetLastError();
}

// The solver's workspace: the round buffers, its state, the grid (scratch and outputs) and the LO's labelling.
struct GcBufs {
    RansacBufs B;
    GcState *st;
    u64 *gkey;
    int *order, *cell_of, *cell_start, *n_cells;
    GcLabelArgs A;  // its three scratch arrays
    float *lab;
};
static void bind_gc_ransac(Carve &c, int N, GcBufs &W) {
    bind_ransac(c, N, W.B);
    W.st = c.take<GcState>(1);
    W.gkey = bind_gc_grid(c, N);
    W.order = c.take<int>((size_t)N);
    W.cell_of = c.take<int>((size_t)N);
    W.cell_start = c.take<int>((size_t)N + 1);
    W.n_cells = c.take<int>(1);
    bind_gc_label(c, N, W.A);
    W.lab = c.take<float>((size_t)N);
}

static int32_t check_gc_rows(int32_t N, int32_t least) {
    if (N < least) return fail(PDSC_ERR_ARG, "N=%d (need >= %d)", N, least);
    if (N > GC_MAX_ROWS) return fail(PDSC_ERR_UNSUPPORTED, "N=%d > %d", N, GC_MAX_ROWS);
    return PDSC_OK;
}

static int32_t check_gc_grid_size(int32_t G) {
    if (G < 1 || G > GC_MAX_GRID) return fail(PDSC_ERR_ARG, "neighborhood_size G=%d not in [1, %d]", G, GC_MAX_GRID);
    return PDSC_OK;
}

static int32_t check_gc_model(double threshold, double lambda) {
    if (!(threshold > 0.0) || !std::isfinite(threshold))
        return fail(PDSC_ERR_ARG, "threshold %g must be > 0 and finite", threshold);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(PDSC_ERR_ARG, "spatial_coherence_weight %g not in [0, 1]", lambda);
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

int32_t pdsc_gc_cell_bound(int32_t which) { return which == 0 ? GC_WAVE_CELL : which == 1 ? GC_LDS_CELL : 0; }

int32_t pdsc_gc_ransac_round(void) { return RANSAC_ROUND; }

size_t pdsc_gc_grid_workspace_bytes(int32_t N) {
    if (N < 1 || N > GC_MAX_ROWS) return 0;
    Carve c(nullptr);
    bind_gc_grid(c, N);
    return c.off;
}

int32_t pdsc_gc_grid(const float *src, const float *tgt, int32_t N, int32_t G, int32_t *order, int32_t *cell_start,
                     int32_t *cell_of, int32_t *n_cells, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_gc_rows(N, 1));
    RET_IF(check_gc_grid_size(G));
    if (!src || !tgt || !order || !cell_start || !cell_of || !n_cells || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_gc_grid_workspace_bytes(N)));
    Carve c(ws);
    HIPCHK(gc_grid_enqueue(src, tgt, N, G, bind_gc_grid(c, N), order, cell_start, cell_of, n_cells, S_(stream)));
    return PDSC_OK;
}

size_t pdsc_gc_label_workspace_bytes(int32_t N) {
    if (N < 1 || N > GC_MAX_ROWS) return 0;
    Carve c(nullptr);
    GcLabelArgs A;
    bind_gc_label(c, N, A);
    return c.off;
}

int32_t pdsc_gc_label(const double *pose, const float *src, const float *tgt, int32_t N, const int32_t *order,
                      const int32_t *cell_start, const int32_t *n_cells, double threshold, double lambda, float *labels,
                      int32_t *count, const pdsc_gc_label_debug *debug, void *ws, size_t ws_bytes,
                      pdsc_stream_t stream) {
    RET_IF(check_gc_rows(N, 1));
    RET_IF(check_gc_model(threshold, lambda));
    if (!pose || !src || !tgt || !order || !cell_start || !n_cells || !labels || !count || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_gc_label_workspace_bytes(N)));
    hipStream_t s = S_(stream);
    GcLabelArgs A;
    A.pose = pose, A.src = src, A.tgt = tgt, A.order = order, A.cell_start = cell_start, A.n_cells = n_cells;
    A.den = 2.0 * (threshold * threshold), A.lambda = lambda;
    A.labels = labels, A.count = count;
    A.dbg = pdsc_gc_label_debug{nullptr, nullptr, nullptr, nullptr};
    if (debug) A.dbg = *debug;
    A.gate = nullptr, A.done = nullptr;
    Carve c(ws);
    bind_gc_label(c, N, A);
    HIPCHK(hipMemsetAsync(count, 0, sizeof(int), s));
    HIPCHK(gc_label_enqueue(A, N, s));
    return PDSC_OK;
}

size_t pdsc_gc_ransac_workspace_bytes(int32_t N) {
    if (N < 3 || N > GC_MAX_ROWS) return 0;
    Carve c(nullptr);
    GcBufs W;
    bind_gc_ransac(c, N, W);
    return c.off;
}

// Enqueues the grid (local_optimization != 0), every round with its LO steps and the finish.
int32_t pdsc_gc_ransac(const float *src, const float *tgt, int32_t N, double threshold, double lambda, int32_t G,
                       int32_t max_iteration, double confidence, uint64_t seed, int32_t local_optimization,
                       float *trans_f32, float *labels, pdsc_gc_ransac_result *result,
                       const pdsc_gc_ransac_debug *debug, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_gc_rows(N, 3));
    if (max_iteration < 1) return fail(PDSC_ERR_ARG, "max_iteration=%d (need >= 1)", max_iteration);
    RET_IF(check_gc_model(threshold, lambda));
    if (!(confidence > 0.0 && confidence <= 1.0)) return fail(PDSC_ERR_ARG, "confidence %g not in (0, 1]", confidence);
    RET_IF(check_gc_grid_size(G));
    if (!src || !tgt || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_gc_ransac_workspace_bytes(N)));
    hipStream_t s = S_(stream);
    const int H = max_iteration, lo = local_optimization ? 1 : 0, nchunks = (int)ransac_chunks(N);
    Carve c(ws);
    GcBufs W;
    bind_gc_ransac(c, N, W);
    const RansacBufs &B = W.B;
    GcState *st = W.st;
    GcLabelArgs &A = W.A;
    pdsc_ransac_debug dbg = {nullptr, nullptr, nullptr, nullptr};
    if (debug) dbg = pdsc_ransac_debug{debug->samples, debug->count, debug->score, debug->trans};
    const double r2 = threshold * threshold;
    const int init_blocks = dbg.count ? (int)(((size_t)H + 255) / 256) : 1;
    hipLaunchKernelGGL(gc_init_kernel, dim3(init_blocks), dim3(256), 0, s, st, B.st, H, dbg.count);
    if (lo) {
        HIPCHK(gc_grid_enqueue(src, tgt, N, G, W.gkey, W.order, W.cell_start, W.cell_of, W.n_cells, s));
        A.pose = st->T, A.src = src, A.tgt = tgt, A.order = W.order, A.cell_start = W.cell_start, A.n_cells = W.n_cells;
        A.den = 2.0 * r2, A.lambda = lambda;
        A.labels = W.lab, A.count = &st->n_lab;
        A.dbg = pdsc_gc_label_debug{nullptr, nullptr, nullptr, nullptr};
        A.gate = &st->lo_active, A.done = &B.st->done;
    }
    for (int r = 0, rounds = ransac_rounds(H); r < rounds; ++r) {
        const RoundShape q = ransac_round_shape(H, r);
        hipLaunchKernelGGL(ransac_hyp_kernel<3>, dim3(q.nwg), dim3(RANSAC_HWG), 0, s, src, tgt, N, q.base, H, (u64)seed,
                           0.0, B, dbg);
        hipLaunchKernelGGL(ransac_score_kernel<true>, dim3((q.nh + 63) / 64, nchunks), dim3(64), 0, s, src, tgt, N,
                           q.nwg, r2, B);
        hipLaunchKernelGGL(gc_round_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, q.nwg, nchunks, r, H, lo, B, st, dbg);
        for (int step = 0; lo && step < GC_LO_STEPS; ++step) {
            HIPCHK(gc_label_enqueue(A, N, s));
            hipLaunchKernelGGL(gc_lo_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, src, tgt, N, r2, W.lab, B.st, st);
        }
        hipLaunchKernelGGL(gc_fold_kernel, dim3(1), dim3(64), 0, s, N, r, confidence, B.st, st);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(gc_finish_kernel, dim3(1), dim3(RANSAC_FIN), 0, s, src, tgt, N, r2, st, lo ? W.n_cells : nullptr,
                       trans_f32, labels, result);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
