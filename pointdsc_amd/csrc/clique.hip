// clique.hip -- the PMC baseline's two pieces (include/pdsc.h f8): the pairwise
// length-consistency graph over N correspondences as bitsets, and an exact
// maximum clique of such a graph (baseline_scripts/baseline_3DMatch.py:56-77;
// the reference's utils/max_clique.py calls a prebuilt x86 libpmc.so).
//
// A graph is N rows of W = ceil(N / 64) 64-bit words.  Wherever one wavefront
// holds a row, lane l holds word l (and word l + 64 when W > 64: WPL = 2 words
// per lane), so an intersection is one AND per lane, a cardinality one popcount
// and a wave sum, and "the lowest / highest member" a ballot and a shuffle.
//
// Everything is integer work except the graph's fp32 predicate, which follows
// the reference's operation order with no contraction (the library's
// -ffp-contract=off, restated for this file below).  No floating-point atomics,
// no integer atomics on global memory either: every output word has one writer,
// so two calls are bitwise equal.  DESIGN.md §7 "PMC baseline" has the algorithm.
#include <cmath>

#include "abi.hpp"
#include "pdsc_internal.hpp"

#pragma clang fp contract(off)

namespace pdsc {

typedef unsigned long long u64;

namespace {

// ---------------------------------------------------------------- the graph --
// One workgroup = 4 waves = one word column wj of GRAPH_ROWS rows; lane l of
// every wave keeps column point j = 64 wj + l in registers, the row point is a
// wave-uniform load, and the 64 predicates of a row become one word by ballot.
constexpr int GRAPH_ROWS = 64;

template <bool LENGTH>
__global__ __launch_bounds__(256) void graph_kernel(const float *__restrict__ corr, int N, int W, double thr,
                                                    u64 *__restrict__ adj) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wj = blockIdx.x, j = wj * 64 + lane;
    const int jc = j < N ? j : N - 1;
    const float sx = corr[6 * jc], sy = corr[6 * jc + 1], sz = corr[6 * jc + 2];
    const float tx = corr[6 * jc + 3], ty = corr[6 * jc + 4], tz = corr[6 * jc + 5];
    const int i0 = blockIdx.y * GRAPH_ROWS + wave * (GRAPH_ROWS / 4);
    for (int r = 0; r < GRAPH_ROWS / 4; ++r) {
        const int i = i0 + r;  // wave-uniform
        if (i >= N) break;
        const float *ci = corr + 6 * (size_t)i;
        const float dx = ci[0] - sx, dy = ci[1] - sy, dz = ci[2] - sz;
        const float ex = ci[3] - tx, ey = ci[4] - ty, ez = ci[5] - tz;
        // np.sum(d ** 2) over three fp32 values: ((dx^2 + dy^2) + dz^2), each product and sum rounded
        float a = (dx * dx + dy * dy) + dz * dz;
        float b = (ex * ex + ey * ey) + ez * ez;
        if (LENGTH) {
            a = sqrtf(a);
            b = sqrtf(b);
        }
        const float diff = a - b;
        const bool edge = j < N && j != i && (double)fabsf(diff) < thr;
        const u64 word = __ballot(edge);
        if (lane == 0) adj[(size_t)i * W + wj] = word;
    }
}

// degree[i] = the members of row i; one wave per row.
__global__ __launch_bounds__(256) void degree_kernel(const u64 *__restrict__ adj, int N, int W, int *__restrict__ degree) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(adj[(size_t)i * W + w]);
    c = wave_sum(c);
    if (lane == 0) degree[i] = c;
}

// ------------------------------------------------------- wave-wide bitsets --
template <int WPL> struct Bits {
    u64 w[WPL];
};

template <int WPL> PDSC_DEV Bits<WPL> load_row(const u64 *__restrict__ g, int v, int W, int lane) {
    Bits<WPL> r;
#pragma unroll
    for (int s = 0; s < WPL; ++s) {
        const int wi = s * 64 + lane;
        r.w[s] = wi < W ? g[(size_t)v * W + wi] : 0ull;
    }
    return r;
}
template <int WPL> PDSC_DEV void store_row(u64 *__restrict__ g, int W, int lane, const Bits<WPL> &r) {
#pragma unroll
    for (int s = 0; s < WPL; ++s) {
        const int wi = s * 64 + lane;
        if (wi < W) g[wi] = r.w[s];
    }
}
template <int WPL> PDSC_DEV int count(const Bits<WPL> &a) {
    int c = 0;
#pragma unroll
    for (int s = 0; s < WPL; ++s) c += __popcll(a.w[s]);
    return wave_sum(c);
}
template <int WPL> PDSC_DEV bool empty(const Bits<WPL> &a) {
    u64 o = 0;
#pragma unroll
    for (int s = 0; s < WPL; ++s) o |= a.w[s];
    return __ballot(o != 0) == 0;
}
PDSC_DEV u64 shfl64(u64 v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
// the highest / lowest member, -1 for the empty set (wave-uniform)
template <int WPL> PDSC_DEV int highest(const Bits<WPL> &a) {
#pragma unroll
    for (int s = WPL - 1; s >= 0; --s) {
        const u64 m = __ballot(a.w[s] != 0);
        if (m) {
            const int l = 63 - __clzll(m);
            return ((s * 64 + l) << 6) + 63 - __clzll(shfl64(a.w[s], l));
        }
    }
    return -1;
}
template <int WPL> PDSC_DEV int lowest(const Bits<WPL> &a) {
#pragma unroll
    for (int s = 0; s < WPL; ++s) {
        const u64 m = __ballot(a.w[s] != 0);
        if (m) {
            const int l = __ffsll(m) - 1;
            return ((s * 64 + l) << 6) + __ffsll(shfl64(a.w[s], l)) - 1;
        }
    }
    return -1;
}
template <int WPL> PDSC_DEV void set_bit(Bits<WPL> &a, int v, int lane, bool on) {
    const int wi = v >> 6;
    const u64 bit = 1ull << (v & 63);
#pragma unroll
    for (int s = 0; s < WPL; ++s)
        if (wi == s * 64 + lane) a.w[s] = on ? (a.w[s] | bit) : (a.w[s] & ~bit);
}
// the members above v
template <int WPL> PDSC_DEV Bits<WPL> above(const Bits<WPL> &a, int v, int lane) {
    Bits<WPL> r;
    const int wv = v >> 6;
#pragma unroll
    for (int s = 0; s < WPL; ++s) {
        const int wi = s * 64 + lane;
        const u64 keep = wi > wv ? ~0ull : (wi == wv ? ((v & 63) == 63 ? 0ull : (~0ull << ((v & 63) + 1))) : 0ull);
        r.w[s] = a.w[s] & keep;
    }
    return r;
}

// ---------------------------------------------------------- the lower bound --
// Greedy clique from start vertex v: the candidates are v's neighbours; take
// the candidate of the highest degree (ties: the lower index), intersect, repeat.
// Returns the size; C receives the clique.
template <int WPL>
PDSC_DEV int greedy_from(const u64 *__restrict__ adj, const int *__restrict__ degree, int N, int W, int v, int lane,
                         Bits<WPL> &C) {
    Bits<WPL> P = load_row<WPL>(adj, v, W, lane);
#pragma unroll
    for (int s = 0; s < WPL; ++s) {  // a caller's stray bits past N never become indices
        const int rem = N - ((s * 64 + lane) << 6);
        P.w[s] &= rem >= 64 ? ~0ull : (rem > 0 ? (1ull << rem) - 1ull : 0ull);
        C.w[s] = 0;
    }
    set_bit(P, v, lane, false);
    set_bit(C, v, lane, true);
    int size = 1;
    for (;;) {
        // key = degree (13 bits: N <= 8192 so degree <= 8191) above the complemented index
        uint32_t key = 0;
#pragma unroll
        for (int s = 0; s < WPL; ++s) {
            u64 w = P.w[s];
            const int base = (s * 64 + lane) << 6;
            while (w) {
                const int u = base + __ffsll(w) - 1;
                w &= w - 1;
                const uint32_t k = ((uint32_t)degree[u] << 13) | (uint32_t)(8191 - u);
                key = k > key ? k : key;
            }
        }
        const bool any = __ballot(key != 0) != 0;  // a candidate has degree >= 1 (it neighbours v): key != 0
        if (!any) break;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
            key = other > key ? other : key;
        }
        const int u = 8191 - (int)(key & 8191u);
        const Bits<WPL> R = load_row<WPL>(adj, u, W, lane);
#pragma unroll
        for (int s = 0; s < WPL; ++s) P.w[s] &= R.w[s];
        set_bit(P, u, lane, false);  // the diagonal is 0 by contract; this keeps the loop finite without it
        set_bit(C, u, lane, true);
        ++size;
    }
    return size;
}

template <int WPL>
__global__ __launch_bounds__(256) void greedy_kernel(const u64 *__restrict__ adj, const int *__restrict__ degree, int N,
                                                     int W, int *__restrict__ hsize) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    Bits<WPL> C;
    const int size = greedy_from<WPL>(adj, degree, N, W, v, lane, C);
    if (lane == 0) hsize[v] = size;
}

// the scalars of a call, in the workspace
struct CliqueState {
    int inc;         // the incumbent's size (best_orig holds its members, original indices)
    int hsize;       // the lower bound's size
    int n_alive;     // survivors of the reduction = rows of the relabelled graph
    int incomplete;  // roots stopped by the budget or the stack depth
    long long nodes;
};

// The best start by (size, lower start vertex), its clique rebuilt (the same
// deterministic greedy) as the first incumbent.  One workgroup.
template <int WPL>
__global__ __launch_bounds__(1024) void greedy_pick_kernel(const u64 *__restrict__ adj, const int *__restrict__ degree,
                                                           const int *__restrict__ hsize, int N, int W,
                                                           CliqueState *__restrict__ st, u64 *__restrict__ best_orig) {
    __shared__ uint32_t part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t key = 0;
    for (int v = threadIdx.x; v < N; v += 1024) {
        const uint32_t k = ((uint32_t)hsize[v] << 13) | (uint32_t)(8191 - v);  // size <= 8192: 14 bits
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
        key = other > key ? other : key;
    }
    if (lane == 0) part[wave] = key;
    __syncthreads();
    if (wave != 0) return;
    key = part[lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, o);
        key = other > key ? other : key;
    }
    const int v = 8191 - (int)(key & 8191u);
    Bits<WPL> C;
    const int size = greedy_from<WPL>(adj, degree, N, W, v, lane, C);
    store_row<WPL>(best_orig, W, lane, C);
    if (lane == 0) {
        st->inc = size;
        st->hsize = size;
        st->n_alive = 0;
        st->incomplete = 0;
        st->nodes = 0;
    }
}

// ------------------------------------------------------------- the reduction --
__global__ __launch_bounds__(128) void alive_init_kernel(int N, int W, u64 *__restrict__ alive) {
    const int w = threadIdx.x;
    if (w >= W) return;
    const int rem = N - w * 64;
    alive[w] = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

// One round: a vertex stays when it has at least st->inc neighbours among the
// vertices alive before the round (a clique larger than the incumbent needs
// that many).  Workgroup wj decides the 64 vertices of word wj, 16 per wave,
// and writes that one word; rdeg[v] = the degree counted.
__global__ __launch_bounds__(256) void peel_kernel(const u64 *__restrict__ adj, int N, int W,
                                                   const CliqueState *__restrict__ st, const u64 *__restrict__ alive_in,
                                                   u64 *__restrict__ alive_out, int *__restrict__ rdeg) {
    __shared__ int keep[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wj = blockIdx.x;
    const int need = st->inc;
    const u64 mine = alive_in[wj];
    for (int r = 0; r < 16; ++r) {
        const int b = wave * 16 + r, v = wj * 64 + b;
        int k = 0;
        if (v < N && ((mine >> b) & 1ull)) {
            int c = 0;
            for (int w = lane; w < W; w += 64) c += __popcll(adj[(size_t)v * W + w] & alive_in[w]);
            c = wave_sum(c);
            k = c >= need;
            if (lane == 0) rdeg[v] = c;
        }
        if (lane == 0) keep[b] = k;
    }
    __syncthreads();
    if (wave == 0) {
        const u64 word = __ballot(keep[lane] != 0);
        if (lane == 0) alive_out[wj] = word;
    }
}

// The survivors' order: ascending (remaining degree, index).  order[rank] = v;
// ranks by counting (N^2 compares of uniform loads).
__global__ __launch_bounds__(256) void order_kernel(const u64 *__restrict__ alive, const int *__restrict__ rdeg, int N,
                                                    int W, int *__restrict__ order, CliqueState *__restrict__ st) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        int c = 0;
        for (int w = threadIdx.x; w < W; w += 64) c += __popcll(alive[w]);
        c = wave_sum(c);
        if (threadIdx.x == 0) st->n_alive = c;
    }
    if (v >= N || !((alive[v >> 6] >> (v & 63)) & 1ull)) return;
    const uint32_t key = ((uint32_t)rdeg[v] << 13) | (uint32_t)v;
    int rank = 0;
    for (int w = 0; w < W; ++w) {
        u64 m = alive[w];
        while (m) {
            const int u = (w << 6) + __ffsll(m) - 1;
            m &= m - 1;
            rank += ((((uint32_t)rdeg[u] << 13) | (uint32_t)u) < key) ? 1 : 0;
        }
    }
    order[rank] = v;
}

// adj2: the survivors' graph in that order (row r = vertex order[r]); rows and
// bits past n_alive are 0.  One wave per new row.
__global__ __launch_bounds__(256) void relabel_kernel(const u64 *__restrict__ adj, int N, int W,
                                                      const int *__restrict__ order, const CliqueState *__restrict__ st,
                                                      u64 *__restrict__ adj2) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    const int n = st->n_alive;
    const u64 *row = r < n ? adj + (size_t)order[r] * W : nullptr;
    for (int w = lane; w < W; w += 64) {
        u64 out = 0;
        if (row)
            for (int b = 0; b < 64; ++b) {
                const int r2 = (w << 6) + b;
                if (r2 >= n) break;
                const int u = order[r2];
                out |= ((row[u >> 6] >> (u & 63)) & 1ull) << b;
            }
        adj2[(size_t)r * W + w] = out;
    }
}

// ---------------------------------------------------------- the exact search --
// One wave per root; wave g of the launch takes roots lo + g, lo + g + G, ...
// below min(hi, n_alive) (a fixed assignment).  A root r searches the cliques
// whose lowest member is r: C = {r}, candidates P = r's later neighbours.
// Node (C, P), with `best` the size to beat: a larger clique needs more than
// k = best - |C| members of P.  |P| <= k prunes.  Otherwise colour P greedily
// (highest index first) with k colour classes: what k classes cover holds no
// clique above k, so every improving clique has a member in the rest Q.  Q
// empty prunes; else branch on the lowest member v of Q -- child (C + v, P & adj[v])
// -- and take v out of P; on return the node is coloured again (with the
// smaller P and maybe a larger best).  Each colouring is one expanded node.
// The stack holds one candidate bitset per level; the clique's vertices sit in LDS.
struct SearchOut {
    int *wsize;        // [G] the wave's best size found in this launch, 0: none above the launch's incumbent
    int *wroot;        // [G] its root
    int *wincomp;      // [G] roots this wave left incomplete
    long long *wnodes; // [G]
    u64 *wbest;        // [G][W] the clique, relabelled indices
};

constexpr int CLIQUE_DEPTH = 256;  // stack levels per root (pdsc_max_clique_depth)

template <int WPL>
__global__ __launch_bounds__(64) void search_kernel(const u64 *__restrict__ adj2, int W, int lo, int hi, int depth,
                                                    long long budget, const CliqueState *__restrict__ st,
                                                    u64 *__restrict__ stack, SearchOut out) {
    __shared__ int cst[CLIQUE_DEPTH];
    const int lane = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    const int n = st->n_alive;
    const int inc0 = st->inc;
    if (hi > n) hi = n;
    int best = inc0, broot = -1, incomplete = 0;
    long long total = 0;
    u64 *stk = stack + (size_t)g * depth * W;
    for (int r = lo + g; r < hi; r += G) {
        Bits<WPL> P = above<WPL>(load_row<WPL>(adj2, r, W, lane), r, lane);
        Bits<WPL> C;
#pragma unroll
        for (int s = 0; s < WPL; ++s) C.w[s] = 0;
        set_bit(C, r, lane, true);
        int d = 0;  // |C| = d + 1
        long long nodes = 0;
        bool stop = false;
        for (;;) {
            const int k = best - (d + 1);
            bool pop = count(P) <= (k > 0 ? k : 0);  // also the empty P
            if (!pop) {
                if (nodes >= budget) {
                    stop = true;
                    break;
                }
                ++nodes;
                Bits<WPL> Q = P;
                for (int c = 0; c < k; ++c) {
                    Bits<WPL> Qc = Q;
                    for (;;) {
                        const int v = highest(Qc);
                        if (v < 0) break;
                        const Bits<WPL> R = load_row<WPL>(adj2, v, W, lane);
#pragma unroll
                        for (int s = 0; s < WPL; ++s) Qc.w[s] &= ~R.w[s];
                        set_bit(Qc, v, lane, false);
                        set_bit(Q, v, lane, false);
                    }
                    if (empty(Q)) break;
                }
                const int v = lowest(Q);
                if (v < 0) {
                    pop = true;
                } else {
                    set_bit(P, v, lane, false);
                    const Bits<WPL> R = load_row<WPL>(adj2, v, W, lane);
                    Bits<WPL> Pn;
#pragma unroll
                    for (int s = 0; s < WPL; ++s) Pn.w[s] = P.w[s] & R.w[s];
                    if (d + 2 > best) {  // C + v beats the best
                        best = d + 2;
                        broot = r;
                        set_bit(C, v, lane, true);
                        store_row<WPL>(out.wbest + (size_t)g * W, W, lane, C);
                        set_bit(C, v, lane, false);
                    }
                    if (!empty(Pn)) {
                        if (d >= depth) {  // no level left for this node's candidates
                            stop = true;
                            break;
                        }
                        store_row<WPL>(stk + (size_t)d * W, W, lane, P);
                        cst[d] = v;  // every lane, the same value: each reads back its own store
                        set_bit(C, v, lane, true);
                        P = Pn;
                        ++d;
                    }
                }
            }
            if (pop) {
                if (d == 0) break;
                --d;
                const int v = cst[d];
                set_bit(C, v, lane, false);
                P = load_row<WPL>(stk + (size_t)d * W, 0, W, lane);
            }
        }
        incomplete += stop ? 1 : 0;
        total += nodes;
    }
    if (lane == 0) {
        out.wsize[g] = best > inc0 ? best : 0;
        out.wroot[g] = broot;
        out.wincomp[g] = incomplete;
        out.wnodes[g] = total;
    }
}

// After a launch: sums the counters and adopts the launch's winner by (size,
// lower root) as the incumbent, mapped back to original indices.  One workgroup.
__global__ __launch_bounds__(256) void adopt_kernel(int G, int W, SearchOut out, const int *__restrict__ order,
                                                    CliqueState *__restrict__ st, u64 *__restrict__ best_orig) {
    __shared__ uint32_t pkey[4];
    __shared__ int pg[4], pinc[4];
    __shared__ long long pnodes[4];
    __shared__ u64 bits[128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t key = 0;
    int kg = -1, inc = 0;
    long long nodes = 0;
    for (int g = threadIdx.x; g < G; g += 256) {
        inc += out.wincomp[g];
        nodes += out.wnodes[g];
        const int sz = out.wsize[g];
        if (sz > 0) {
            const uint32_t k = ((uint32_t)sz << 13) | (uint32_t)(8191 - out.wroot[g]);  // roots are distinct per wave
            if (k > key) key = k, kg = g;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)key, o);
        const int og = __shfl_xor(kg, o);
        if (ok > key) key = ok, kg = og;
    }
    inc = wave_sum(inc);
    nodes = wave_sum(nodes);
    if (lane == 0) pkey[wave] = key, pg[wave] = kg, pinc[wave] = inc, pnodes[wave] = nodes;
    if (threadIdx.x < 128) bits[threadIdx.x] = 0;
    __syncthreads();
    key = 0, kg = -1;
    for (int w = 0; w < 4; ++w)
        if (pkey[w] > key) key = pkey[w], kg = pg[w];
    if (threadIdx.x == 0) {
        st->incomplete += pinc[0] + pinc[1] + pinc[2] + pinc[3];
        st->nodes += pnodes[0] + pnodes[1] + pnodes[2] + pnodes[3];
    }
    if (key == 0) return;  // uniform: no wave beat the incumbent
    const u64 *src = out.wbest + (size_t)kg * W;
    for (int w = threadIdx.x; w < W; w += 256) {
        u64 m = src[w];
        while (m) {
            const int u = order[(w << 6) + __ffsll(m) - 1];
            m &= m - 1;
            atomicOr(&bits[u >> 6], 1ull << (u & 63));  // LDS, commutative: the word does not depend on the order
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += 256) best_orig[w] = bits[w];
    if (threadIdx.x == 0) st->inc = (int)(key >> 13);
}

// members ascending (-1 past the size), labels, the result struct.  One workgroup.
__global__ __launch_bounds__(256) void finish_kernel(const u64 *__restrict__ best_orig, int N, int W,
                                                     const CliqueState *__restrict__ st, int exact_search,
                                                     int *__restrict__ members, float *__restrict__ labels,
                                                     pdsc_clique_result *__restrict__ res) {
    for (int w = threadIdx.x; w < W; w += 256) {
        int at = 0;
        for (int p = 0; p < w; ++p) at += __popcll(best_orig[p]);
        u64 m = best_orig[w];
        while (m) {
            members[at++] = (w << 6) + __ffsll(m) - 1;
            m &= m - 1;
        }
    }
    const int size = st->inc;
    for (int i = threadIdx.x; i < N; i += 256) {
        if (i >= size) members[i] = -1;
        if (labels) labels[i] = ((best_orig[i >> 6] >> (i & 63)) & 1ull) ? 1.0f : 0.0f;
    }
    if (threadIdx.x == 0 && res) {
        res->size = size;
        res->exact = exact_search && st->incomplete == 0 ? 1 : 0;
        res->heuristic_size = st->hsize;
        res->roots_incomplete = st->incomplete;
        res->nodes = st->nodes;
    }
}

// --------------------------------------------------------------- workspace --
constexpr int PEEL_ROUNDS = 16;         // reduction rounds (each sound on its own; a fixed number of launches)
constexpr int SEARCH_LAUNCHES = 4;      // root ranges, each starting from the previous one's winner
constexpr size_t STACK_BYTES_MAX = size_t(128) << 20;

struct CliqueWs {
    int *deg0, *hsize, *rdeg, *order;
    u64 *alive[2], *best_orig, *adj2, *stack;
    CliqueState *st;
    SearchOut out;
    int G, depth;
};

CliqueWs carve_clique(Carve &k, int N) {
    const int W = (N + 63) / 64;
    CliqueWs c;
    c.depth = N < CLIQUE_DEPTH ? N : CLIQUE_DEPTH;
    const size_t level = (size_t)c.depth * W * sizeof(u64);
    size_t stack_bytes = (size_t)N * level;  // monotone in N; capped
    if (stack_bytes > STACK_BYTES_MAX) stack_bytes = STACK_BYTES_MAX;
    c.G = (int)(stack_bytes / level);  // >= 1: one level set is at most 256 KiB
    c.st = k.take<CliqueState>(1);
    c.deg0 = k.take<int>((size_t)N);
    c.hsize = k.take<int>((size_t)N);
    c.rdeg = k.take<int>((size_t)N);
    c.order = k.take<int>((size_t)N);
    c.alive[0] = k.take<u64>((size_t)W);
    c.alive[1] = k.take<u64>((size_t)W);
    c.best_orig = k.take<u64>((size_t)W);
    c.adj2 = k.take<u64>((size_t)N * W);
    // the per-wave slots are sized for N waves (G <= N), so that the total is monotone in N
    c.out.wsize = k.take<int>((size_t)N);
    c.out.wroot = k.take<int>((size_t)N);
    c.out.wincomp = k.take<int>((size_t)N);
    c.out.wnodes = k.take<long long>((size_t)N);
    c.out.wbest = k.take<u64>((size_t)N * W);
    c.stack = reinterpret_cast<u64 *>(k.take_bytes(stack_bytes));
    return c;
}

template <int WPL>
hipError_t run_clique(const u64 *adj, int N, long long budget, bool exact, int *members, pdsc_clique_result *res,
                      float *labels, void *ws, hipStream_t s) {
    const int W = (N + 63) / 64;
    Carve k(ws);
    const CliqueWs c = carve_clique(k, N);
    const int rows4 = (N + 3) / 4;
    hipLaunchKernelGGL(degree_kernel, dim3(rows4), dim3(256), 0, s, adj, N, W, c.deg0);
    hipLaunchKernelGGL(greedy_kernel<WPL>, dim3(rows4), dim3(256), 0, s, adj, c.deg0, N, W, c.hsize);
    hipLaunchKernelGGL(greedy_pick_kernel<WPL>, dim3(1), dim3(1024), 0, s, adj, c.deg0, c.hsize, N, W, c.st, c.best_orig);
    if (exact) {
        hipLaunchKernelGGL(alive_init_kernel, dim3(1), dim3(128), 0, s, N, W, c.alive[0]);
        for (int r = 0; r < PEEL_ROUNDS; ++r)
            hipLaunchKernelGGL(peel_kernel, dim3(W), dim3(256), 0, s, adj, N, W, c.st, c.alive[r & 1], c.alive[(r + 1) & 1],
                               c.rdeg);
        const u64 *alive = c.alive[PEEL_ROUNDS & 1];
        hipLaunchKernelGGL(order_kernel, dim3((N + 255) / 256), dim3(256), 0, s, alive, c.rdeg, N, W, c.order, c.st);
        hipLaunchKernelGGL(relabel_kernel, dim3(rows4), dim3(256), 0, s, adj, N, W, c.order, c.st, c.adj2);
        const int per = (N + SEARCH_LAUNCHES - 1) / SEARCH_LAUNCHES;
        for (int lo = 0; lo < N; lo += per) {
            const int hi = lo + per < N ? lo + per : N;
            const int G = hi - lo < c.G ? hi - lo : c.G;
            hipLaunchKernelGGL(search_kernel<WPL>, dim3(G), dim3(64), 0, s, c.adj2, W, lo, hi, c.depth, budget, c.st,
                               c.stack, c.out);
            hipLaunchKernelGGL(adopt_kernel, dim3(1), dim3(256), 0, s, G, W, c.out, c.order, c.st, c.best_orig);
        }
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, s, c.best_orig, N, W, c.st, exact ? 1 : 0, members, labels,
                       res);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_consistency_graph(const float *corr_pos, int N, double thr, bool length, u64 *adj, int *degree,
                                    hipStream_t s) {
    const int W = (N + 63) / 64;
    const dim3 grid(W, (N + GRAPH_ROWS - 1) / GRAPH_ROWS);
    if (length)
        hipLaunchKernelGGL(graph_kernel<true>, grid, dim3(256), 0, s, corr_pos, N, W, thr, adj);
    else
        hipLaunchKernelGGL(graph_kernel<false>, grid, dim3(256), 0, s, corr_pos, N, W, thr, adj);
    if (degree) hipLaunchKernelGGL(degree_kernel, dim3((N + 3) / 4), dim3(256), 0, s, adj, N, W, degree);
    return hipGetLastError();
}

void *reserve_clique(Carve &k, int N) {
    void *ws = k.take_bytes(0);  // where the next slice starts
    carve_clique(k, N);
    return ws;
}

hipError_t launch_max_clique(const u64 *adj, int N, long long budget, bool exact, int *members, pdsc_clique_result *res,
                             float *labels, void *ws, hipStream_t s) {
    return N > 4096 ? run_clique<2>(adj, N, budget, exact, members, res, labels, ws, s)
                    : run_clique<1>(adj, N, budget, exact, members, res, labels, ws, s);
}

static int32_t clique_call(const uint64_t *adj, int32_t N, int64_t node_budget, bool exact, int32_t *members,
                           pdsc_clique_result *result, float *labels, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (N < 1) return fail(PDSC_ERR_ARG, "N=%d (need >= 1)", N);
    if (N > CLIQUE_MAX_N) return fail(PDSC_ERR_UNSUPPORTED, "N=%d > %d", N, CLIQUE_MAX_N);
    if (node_budget < 0) return fail(PDSC_ERR_ARG, "node_budget=%lld (need >= 0; 0: the default)", (long long)node_budget);
    if (!adj || !members || !result || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_max_clique_workspace_bytes(N)));
    HIPCHK(launch_max_clique(reinterpret_cast<const u64 *>(adj), N,
                             node_budget ? (long long)node_budget : CLIQUE_DEFAULT_BUDGET, exact, members, result, labels,
                             ws, S_(stream)));
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

int32_t pdsc_consistency_graph(const float *corr_pos, int32_t N, double threshold, int32_t mode, uint64_t *adj,
                               int32_t *degree, pdsc_stream_t stream) {
    if (N < 1) return fail(PDSC_ERR_ARG, "N=%d (need >= 1)", N);
    if (N > CLIQUE_MAX_N) return fail(PDSC_ERR_UNSUPPORTED, "N=%d > %d", N, CLIQUE_MAX_N);
    if (!(threshold > 0.0) || !std::isfinite(threshold))
        return fail(PDSC_ERR_ARG, "threshold %g must be > 0 and finite", threshold);
    if (mode != PDSC_EDGE_SQUARED && mode != PDSC_EDGE_LENGTH)
        return fail(PDSC_ERR_ARG, "mode=%d (PDSC_EDGE_SQUARED or PDSC_EDGE_LENGTH)", mode);
    if (!corr_pos || !adj) return fail(PDSC_ERR_ARG, "null pointer");
    HIPCHK(launch_consistency_graph(corr_pos, N, threshold, mode == PDSC_EDGE_LENGTH, reinterpret_cast<u64 *>(adj), degree,
                                    S_(stream)));
    return PDSC_OK;
}

int32_t pdsc_max_clique_depth(void) { return CLIQUE_DEPTH; }
int64_t pdsc_max_clique_default_budget(void) { return CLIQUE_DEFAULT_BUDGET; }

size_t pdsc_max_clique_workspace_bytes(int32_t N) {
    if (N < 1 || N > CLIQUE_MAX_N) return 0;
    Carve k(nullptr);
    carve_clique(k, N);
    return k.off;
}

int32_t pdsc_max_clique(const uint64_t *adj, int32_t N, int64_t node_budget, int32_t *members,
                        pdsc_clique_result *result, float *labels, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    return clique_call(adj, N, node_budget, true, members, result, labels, ws, ws_bytes, stream);
}

int32_t pdsc_greedy_clique(const uint64_t *adj, int32_t N, int32_t *members, pdsc_clique_result *result, float *labels,
                           void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    return clique_call(adj, N, 0, false, members, result, labels, ws, ws_bytes, stream);
}

}  // extern "C"
