// match_filter.hip -- f7: the filter stage of the fork's "fast RANSAC" pipeline
// (algorithms/matching.py, algorithms/FR.py:36-58) between descriptor matching
// and RANSAC: second nearest neighbours in feature space, the best-buddy mark,
// the 1st / 2nd distance ratio and the Grid-Prioritized Filter.  The choices the
// reference leaves open (ties, summation order, the unstable argsort, max == min)
// are fixed in include/pdsc.h (f7).  The refit over the unfiltered pairs
// (FR.py:101-114, pdsc_refit_inliers) shares ransac_finish_kernel's scoring and
// Kabsch and therefore lives beside it in ransac.hip.
//
//   nn2          dist = sqrt(max(|a|^2 + |b|^2 - 2 a.b, 1e-30)) in 64 x 64 tiles
//                (fp32 FMA chains from LDS, as nn_argmin_kernel); the N0 x N1
//                matrix never reaches HBM.  A workgroup owns a stripe of 64 rows
//                and walks a contiguous range of column tiles with the rows'
//                two best (key, index) words in registers; the column minima go
//                out by 64-bit atomicMin per tile as in nn_argmin_kernel.  The
//                column tiles are split over `nsplit` workgroups per stripe
//                (79 stripes at N0 = 5000 would leave two thirds of 256 CUs
//                idle; at N0 = 20000 the 313 stripes still get a split of 4)
//                and nn2_merge folds the partial pairs in split order.  The
//                words are distinct (they carry the index), so the two
//                smallest of a union do not depend on how it was split.
//   match_ratio  one thread per row: the two length-D sums, the ratio and the
//                best-buddy mark; then one workgroup: min / max, num_bb, norm.
//   gpf          cells + counts + water-filling (one workgroup, the bisection in
//                one thread, fp64), a scatter of (key, index) words into per-cell
//                lists, rank counting inside the cell, and an ordered
//                compaction in ascending row (the corr_select_kernel pattern).
//
// Integer atomics only: two calls are bitwise equal.
#include <cmath>

#include "abi.hpp"
#include "pdsc_internal.hpp"

namespace pdsc {

typedef unsigned long long u64;
constexpr int N2_T = 64;      // tile edge
constexpr int N2_DMAX = 64;   // descriptor width limit (as pdsc_mutual_nn)
constexpr u64 KEY_NONE = ~0ull;
constexpr int NN2_MAX_SPLIT = 16;  // column splits per row stripe the workspace is sized for

// Ordered pairs (k1 < k2 unless both are KEY_NONE) are updated by value with
// min / max selects only: no branch, no store through a reference, so the
// pairs stay in registers.
PDSC_DEV u64 umax64(u64 a, u64 b) { return a < b ? b : a; }
// the second of the two smallest of {k1, k2, k} (the first is umin64(k1, k))
PDSC_DEV u64 top2_second(u64 k1, u64 k2, u64 k) { return umin64(k2, umax64(k1, k)); }
// the second of the two smallest of two ordered pairs (the first is umin64(a1, b1))
PDSC_DEV u64 top2_merge_second(u64 a1, u64 a2, u64 b1, u64 b2) { return umin64(umax64(a1, b1), umin64(a2, b2)); }

// grid: (nsplit, row stripes).  rowpart: [nsplit][Na][2].
__global__ __launch_bounds__(256) void nn2_kernel(const float *__restrict__ A, const float *__restrict__ Bd, int Na,
                                                  int Nb, int D, int nsplit, u64 *__restrict__ rowpart,
                                                  u64 *__restrict__ colkey) {
    __shared__ __attribute__((aligned(16))) float sa[N2_DMAX][N2_T + 4];  // sa[k][row]
    __shared__ __attribute__((aligned(16))) float sb[N2_DMAX][N2_T + 4];  // sb[k][col]
    __shared__ __attribute__((aligned(16))) float na[N2_T], nb[N2_T];     // squared norms
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;  // columns 4tx..+3, rows 4ty..+3
    const int i0 = blockIdx.y * N2_T;
    const int ntile = (Nb + N2_T - 1) / N2_T;
    const int t0 = (int)((long long)blockIdx.x * ntile / nsplit), t1 = (int)((long long)(blockIdx.x + 1) * ntile / nsplit);
    for (int e = tid; e < N2_T * D; e += 256) {
        const int r = e / D, k = e % D;
        sa[k][r] = (i0 + r < Na) ? A[(size_t)(i0 + r) * D + k] : 0.0f;
    }
    u64 r1[4], r2[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r1[q] = r2[q] = KEY_NONE;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * N2_T;
        __syncthreads();  // the previous tile's reads of sb / nb are done
        for (int e = tid; e < N2_T * D; e += 256) {
            const int r = e / D, k = e % D;
            sb[k][r] = (j0 + r < Nb) ? Bd[(size_t)(j0 + r) * D + k] : 0.0f;
        }
        __syncthreads();
        if (tid < N2_T) {  // |b|^2: ascending-k fmaf chain
            float s = 0.0f;
            for (int k = 0; k < D; ++k) s = __builtin_fmaf(sb[k][tid], sb[k][tid], s);
            nb[tid] = s;
        } else if (tid < 2 * N2_T && t == t0) {
            float s = 0.0f;
            for (int k = 0; k < D; ++k) s = __builtin_fmaf(sa[k][tid - N2_T], sa[k][tid - N2_T], s);
            na[tid - N2_T] = s;
        }
        float acc[4][4] = {};
#pragma unroll 4
        for (int k = 0; k < D; ++k) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&sa[k][4 * ty]);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(&sb[k][4 * tx]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_fmaf(a[r], b[c], acc[r][c]);
        }
        __syncthreads();  // na / nb
        u64 cbest[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cbest[q] = KEY_NONE;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * ty + r;
            const float an = na[4 * ty + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = j0 + 4 * tx + c;
                if (i < Na && j < Nb) {
                    const float d2 = (an + nb[4 * tx + c]) - 2.0f * acc[r][c];
                    const float d = sqrtf(d2 < 1e-30f ? 1e-30f : d2);  // clamp_min: a NaN stays a NaN
                    const u64 key = (u64)nn_key(d) << 32;
                    const u64 kj = key | (uint32_t)j;
                    r2[r] = top2_second(r1[r], r2[r], kj);
                    r1[r] = umin64(r1[r], kj);
                    cbest[c] = umin64(cbest[c], key | (uint32_t)i);
                }
            }
        }
        // columns: lanes tx, tx+16, tx+32, tx+48 of a wave share tx
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            cbest[c] = umin64(cbest[c], shfl_xor64(cbest[c], 16));
            cbest[c] = umin64(cbest[c], shfl_xor64(cbest[c], 32));
            const int j = j0 + 4 * tx + c;
            if ((tid & 63) < 16 && j < Nb && cbest[c] != KEY_NONE) atomicMin(colkey + j, cbest[c]);
        }
    }
    // rows: the 16 threads sharing ty are 16 consecutive lanes
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) {
            const u64 b1 = shfl_xor64(r1[r], m), b2 = shfl_xor64(r2[r], m);
            r2[r] = top2_merge_second(r1[r], r2[r], b1, b2);
            r1[r] = umin64(r1[r], b1);
        }
        const int i = i0 + 4 * ty + r;
        if (tx == 0 && i < Na) {
            u64 *p = rowpart + ((size_t)blockIdx.x * Na + i) * 2;
            p[0] = r1[r];
            p[1] = r2[r];
        }
    }
}

__global__ __launch_bounds__(256) void nn2_merge_kernel(const u64 *__restrict__ rowpart, const u64 *__restrict__ colkey,
                                                        int Na, int Nb, int nsplit, int *__restrict__ nn1,
                                                        int *__restrict__ nn2, int *__restrict__ rev) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Na) {
        u64 k1 = KEY_NONE, k2 = KEY_NONE;
        for (int s = 0; s < nsplit; ++s) {
            const u64 *p = rowpart + ((size_t)s * Na + i) * 2;
            const u64 b1 = p[0], b2 = p[1];
            k2 = top2_merge_second(k1, k2, b1, b2);
            k1 = umin64(k1, b1);
        }
        nn1[i] = (int)(uint32_t)k1;
        nn2[i] = (int)(uint32_t)k2;
    }
    if (i < Nb) rev[i] = (int)(uint32_t)colkey[i];
}

static int nn2_default_split(int Na, int Nb) {
    const int stripes = (Na + N2_T - 1) / N2_T, ntile = (Nb + N2_T - 1) / N2_T;
    int s = (1024 + stripes - 1) / stripes;  // four 35 KiB workgroups per CU on 256 CUs
    if (s > NN2_MAX_SPLIT) s = NN2_MAX_SPLIT;
    if (s > ntile) s = ntile;
    return s < 1 ? 1 : s;
}

struct Nn2Bufs {
    u64 *rowpart;  // [NN2_MAX_SPLIT][Na][2] the splits' two best keys per row
    u64 *colkey;   // [Nb] the best key per column
};
static void bind_nn2(Carve &c, int Na, int Nb, Nn2Bufs &W) {
    W.rowpart = c.take<u64>((size_t)NN2_MAX_SPLIT * Na * 2);
    W.colkey = c.take<u64>((size_t)Nb);
}

static int32_t check_desc_args(int32_t N0, int32_t N1, int32_t D) {
    if (N0 < 1 || N1 < 2 || D < 1) return fail(PDSC_ERR_ARG, "N0=%d N1=%d D=%d (need N0 >= 1, N1 >= 2, D >= 1)", N0, N1, D);
    if (D > N2_DMAX) return fail(PDSC_ERR_UNSUPPORTED, "D=%d > %d", D, N2_DMAX);
    return PDSC_OK;
}

// split: column splits per row stripe, 0 = nn2_default_split (clamped to the column tiles and NN2_MAX_SPLIT)
static int32_t nn2_call(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, int split, int32_t *nn1,
                        int32_t *nn2, int32_t *rev, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_desc_args(N0, N1, D));
    if (!f0 || !f1 || !nn1 || !nn2 || !rev || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_nn2_workspace_bytes(N0, N1)));
    hipStream_t s = S_(stream);
    const int ntile = (N1 + N2_T - 1) / N2_T;
    int nsplit = split > 0 ? split : nn2_default_split(N0, N1);
    if (nsplit > NN2_MAX_SPLIT) nsplit = NN2_MAX_SPLIT;
    if (nsplit > ntile) nsplit = ntile;
    Carve c(ws);
    Nn2Bufs W;
    bind_nn2(c, N0, N1, W);
    HIPCHK(hipMemsetAsync(W.colkey, 0xff, (size_t)N1 * sizeof(u64), s));
    hipLaunchKernelGGL(nn2_kernel, dim3(nsplit, (N0 + N2_T - 1) / N2_T), dim3(256), 0, s, f0, f1, N0, N1, D, nsplit,
                       W.rowpart, W.colkey);
    HIPCHK(hipGetLastError());
    const int n = N0 > N1 ? N0 : N1;
    hipLaunchKernelGGL(nn2_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, s, W.rowpart, W.colkey, N0, N1, nsplit,
                       nn1, nn2, rev);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

// ---------------------------------------------------------------- match_ratio
// sqrt(sum_k (a_k - b_k)^2), the sum an ascending-k fmaf chain of the squared differences
PDSC_DEV float diff_norm(const float *__restrict__ a, const float *__restrict__ b, int D) {
    float s = 0.0f;
    for (int k = 0; k < D; ++k) {
        const float d = a[k] - b[k];
        s = __builtin_fmaf(d, d, s);
    }
    return sqrtf(s);
}

__global__ __launch_bounds__(256) void ratio_rows_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                         int N0, int N1, int D, const int *__restrict__ nn1,
                                                         const int *__restrict__ nn2, const int *__restrict__ rev,
                                                         int *__restrict__ is_bb, float *__restrict__ feat_dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N0) return;
    const int j1 = nn1[i], j2 = nn2[i];
    const bool ok = (unsigned)j1 < (unsigned)N1 && (unsigned)j2 < (unsigned)N1;  // foreign indices: NaN, no gather
    float fd = __builtin_nanf("");
    if (ok) {
        const float *a = f0 + (size_t)i * D;
        fd = diff_norm(a, f1 + (size_t)j1 * D, D) / (diff_norm(a, f1 + (size_t)j2 * D, D) + 1e-6f);
    }
    feat_dist[i] = fd;
    if (rev) is_bb[i] = ok && rev[j1] == i ? 1 : 0;
}

// one workgroup: min / max of feat_dist, num_bb, norm = (fd - min) / (max - min) [- 1 on best buddies]
__global__ __launch_bounds__(1024) void ratio_norm_kernel(const float *__restrict__ feat_dist,
                                                          const int *__restrict__ is_bb, int N0,
                                                          float *__restrict__ norm, int *__restrict__ num_bb) {
    __shared__ float smin[16], smax[16];
    __shared__ int scnt[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int cnt = 0;
    for (int i = tid; i < N0; i += 1024) {
        const float v = feat_dist[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        cnt += is_bb[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) smin[wave] = mn, smax[wave] = mx, scnt[wave] = cnt;
    __syncthreads();
    mn = smin[0], mx = smax[0], cnt = scnt[0];
    for (int w = 1; w < 16; ++w) {
        mn = smin[w] < mn ? smin[w] : mn;
        mx = smax[w] > mx ? smax[w] : mx;
        cnt += scnt[w];
    }
    const float span = mx - mn;
    for (int i = tid; i < N0; i += 1024) {
        float v = span == 0.0f ? 0.0f : (feat_dist[i] - mn) / span;  // max == min: zeros (the reference divides by 0)
        if (is_bb[i]) v -= 1.0f;
        norm[i] = v;
    }
    if (tid == 0) num_bb[0] = cnt;
}

// ------------------------------------------------------------------------ gpf
struct GpfBufs {
    int *cell;     // [N0] cell of each row, -1: outside the grid (the reference's loops never visit it)
    int *cnt;      // [G2] max_per_quad
    int *start;    // [G2] first slot of the cell's list
    int *cursor;   // [G2]
    int *quota;    // [G2] rows to keep
    u64 *list;     // [N0] (key(norm), row) words grouped by cell
    int *keep;     // [N0]
};

PDSC_DEV float wg_min(float v, float *red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(v, o);
        v = a < v ? a : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int w = 1; w < 16; ++w) v = red[w] < v ? red[w] : v;
    return v;
}

// to_quads (matching.py:139-145) in its own operation order, fp32, no contraction
PDSC_DEV int to_quad(float x, float m, float M, int G) {
    const float x_ = (x - m) / ((M - m) + 1e-3f);
    const float q = floorf((float)G * x_);
    return (q >= 0.0f && q < (float)G) ? (int)q : -1;
}

__global__ __launch_bounds__(1024) void gpf_cells_kernel(const float *__restrict__ xyz, int N0, int G,
                                                         const int *__restrict__ num_bb, double factor, GpfBufs B,
                                                         pdsc_gpf_debug dbg) {
    __shared__ float red[16];
    __shared__ int scnt[64 * 64];
    const int tid = threadIdx.x, G2 = G * G;
    float mnx = __builtin_inff(), mxx = __builtin_inff(), mny = __builtin_inff(), mxy = __builtin_inff();
    for (int i = tid; i < N0; i += 1024) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1];
        mnx = x < mnx ? x : mnx;
        mxx = -x < mxx ? -x : mxx;  // max as -min(-x): exact
        mny = y < mny ? y : mny;
        mxy = -y < mxy ? -y : mxy;
    }
    mnx = wg_min(mnx, red, tid);
    mxx = -wg_min(mxx, red, tid);
    mny = wg_min(mny, red, tid);
    mxy = -wg_min(mxy, red, tid);
    for (int c = tid; c < G2; c += 1024) scnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < N0; i += 1024) {
        const int qi = to_quad(xyz[3 * (size_t)i], mnx, mxx, G), qj = to_quad(xyz[3 * (size_t)i + 1], mny, mxy, G);
        const int c = (qi < 0 || qj < 0) ? -1 : qi * G + qj;
        B.cell[i] = c;
        if (dbg.cell) dbg.cell[i] = c;
        if (c >= 0) atomicAdd(&scnt[c], 1);
    }
    __syncthreads();
    for (int c = tid; c < G2; c += 1024) {
        B.cnt[c] = scnt[c];
        B.cursor[c] = 0;
        if (dbg.max_per_quad) dbg.max_per_quad[c] = scnt[c];
    }
    if (tid != 0) return;
    // the water-filling bisection (matching.py:157-182) as written, fp64, cells in index order
    const double total = factor * (double)num_bb[0];
    double max_h = total, min_h = 0.0, cur = (max_h + min_h) / 2;
    while (fabs(max_h - min_h) > 2) {
        double sum = 0.0;
        for (int c = 0; c < G2; ++c) {
            const double m = (double)scnt[c];
            sum += m < cur ? m : cur;
        }
        if (sum == total) break;
        if (sum < total)
            min_h = cur;
        else if (sum > total)
            max_h = cur;
        cur = (max_h + min_h) / 2;
    }
    const double h = rint(cur);  // np.round: half to even
    int run = 0;
    for (int c = 0; c < G2; ++c) {
        const double m = (double)scnt[c];
        const double pq = m < h ? m : h;
        B.start[c] = run;
        run += scnt[c];
        B.quota[c] = pq == m ? scnt[c] : (pq > 0.0 ? (int)pq : 0);  // pq < m <= INT_MAX on the second branch
        if (dbg.per_quad) dbg.per_quad[c] = pq;
    }
    if (dbg.height) dbg.height[0] = cur;
}

__global__ __launch_bounds__(256) void gpf_scatter_kernel(const float *__restrict__ norm, int N0, GpfBufs B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N0) return;
    const int c = B.cell[i];
    if (c < 0) return;
    const int pos = B.start[c] + atomicAdd(&B.cursor[c], 1);  // the order inside a list does not matter
    B.list[pos] = ((u64)nn_key(norm[i]) << 32) | (uint32_t)i;
}

// keep[i] = the row is among the quota lowest (norm, row) of its cell
__global__ __launch_bounds__(256) void gpf_rank_kernel(const float *__restrict__ norm, int N0, GpfBufs B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N0) return;
    const int c = B.cell[i];
    int keep = 0;
    if (c >= 0) {
        const int n = B.cnt[c], q = B.quota[c];
        if (q >= n) {
            keep = 1;
        } else if (q > 0) {
            const u64 me = ((u64)nn_key(norm[i]) << 32) | (uint32_t)i;
            const u64 *l = B.list + B.start[c];
            int rank = 0;
            for (int k = 0; k < n; ++k) rank += l[k] < me ? 1 : 0;
            keep = rank < q;
        }
    }
    B.keep[i] = keep;
}

// One 1024-thread workgroup: ordered compaction in ascending row (as corr_select_kernel).
__global__ __launch_bounds__(1024) void gpf_compact_kernel(const int *__restrict__ keepf, const float *__restrict__ norm,
                                                           int N0, int *__restrict__ kept, int *__restrict__ count,
                                                           float *__restrict__ kept_norm) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int running = 0;
    for (int base = 0; base < N0; base += 1024) {
        const int i = base + tid;
        const bool keep = i < N0 && keepf[i] != 0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        if (keep) {
            const int pos = running + before + __popcll(m & ((1ull << lane) - 1ull));
            kept[pos] = i;
            if (kept_norm) kept_norm[pos] = norm[i];
        }
        running += total;
        __syncthreads();
    }
    if (tid == 0) count[0] = running;
}

static void bind_gpf(Carve &c, int N0, int G, GpfBufs &B) {
    const size_t G2 = (size_t)G * G;
    B.cell = c.take<int>((size_t)N0);
    B.keep = c.take<int>((size_t)N0);
    B.cnt = c.take<int>(G2);
    B.start = c.take<int>(G2);
    B.cursor = c.take<int>(G2);
    B.quota = c.take<int>(G2);
    B.list = c.take<u64>((size_t)N0);
}

// Rows pdsc_gpf_select accepts: a truncated cell of n rows costs n^2 word compares (gpf_rank_kernel), so one
// cell holding every row costs N0^2 -- 6.9e10 at this limit, well under a second on 256 CUs.
constexpr int GPF_MAX_ROWS = 1 << 18;

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_nn2_workspace_bytes(int32_t N0, int32_t N1) {
    if (N0 < 1 || N1 < 2) return 0;
    Carve c(nullptr);
    Nn2Bufs W;
    bind_nn2(c, N0, N1, W);
    return c.off;
}

int32_t pdsc_nn2(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, int32_t *nn1, int32_t *nn2,
                 int32_t *rev, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    return nn2_call(f0, f1, N0, N1, D, 0, nn1, nn2, rev, ws, ws_bytes, stream);
}

int32_t pdsc_nn2_split(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, int32_t split,
                       int32_t *nn1, int32_t *nn2, int32_t *rev, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (split < 1) return fail(PDSC_ERR_ARG, "split=%d (need >= 1)", split);
    return nn2_call(f0, f1, N0, N1, D, split, nn1, nn2, rev, ws, ws_bytes, stream);
}

// rev == nullptr: only feat_dist
int32_t pdsc_match_ratio(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, const int32_t *nn1,
                         const int32_t *nn2, const int32_t *rev, int32_t *is_bb, float *feat_dist, float *norm,
                         int32_t *num_bb, pdsc_stream_t stream) {
    RET_IF(check_desc_args(N0, N1, D));
    if (!f0 || !f1 || !nn1 || !nn2 || !feat_dist) return fail(PDSC_ERR_ARG, "null pointer");
    if (rev && (!is_bb || !norm || !num_bb)) return fail(PDSC_ERR_ARG, "null pointer (is_bb, norm, num_bb go with rev)");
    hipStream_t s = S_(stream);
    hipLaunchKernelGGL(ratio_rows_kernel, dim3((N0 + 255) / 256), dim3(256), 0, s, f0, f1, N0, N1, D, nn1, nn2, rev,
                       is_bb, feat_dist);
    HIPCHK(hipGetLastError());
    if (rev) hipLaunchKernelGGL(ratio_norm_kernel, dim3(1), dim3(1024), 0, s, feat_dist, is_bb, N0, norm, num_bb);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

size_t pdsc_gpf_select_workspace_bytes(int32_t N0, int32_t grid_wid) {
    if (N0 < 1 || N0 > GPF_MAX_ROWS || grid_wid < 1 || grid_wid > 64) return 0;
    Carve c(nullptr);
    GpfBufs B;
    bind_gpf(c, N0, grid_wid, B);
    return c.off;
}

int32_t pdsc_gpf_select(const float *xyz0, const float *norm, const int32_t *num_bb, int32_t N0, int32_t grid_wid,
                        double gpf_factor, int32_t *kept, int32_t *count, float *kept_norm,
                        const pdsc_gpf_debug *debug, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (N0 < 1 || grid_wid < 1) return fail(PDSC_ERR_ARG, "N0=%d grid_wid=%d (need >= 1)", N0, grid_wid);
    if (grid_wid > 64) return fail(PDSC_ERR_UNSUPPORTED, "grid_wid=%d > 64", grid_wid);
    if (N0 > GPF_MAX_ROWS) return fail(PDSC_ERR_UNSUPPORTED, "N0=%d > %d (rank counting inside a cell)", N0, GPF_MAX_ROWS);
    if (!(gpf_factor >= 0.0) || !std::isfinite(gpf_factor))
        return fail(PDSC_ERR_ARG, "gpf_factor %g must be >= 0 and finite", gpf_factor);
    if (!xyz0 || !norm || !num_bb || !kept || !count || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_gpf_select_workspace_bytes(N0, grid_wid)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    GpfBufs B;
    bind_gpf(c, N0, grid_wid, B);
    pdsc_gpf_debug dbg = {nullptr, nullptr, nullptr, nullptr};
    if (debug) dbg = *debug;
    hipLaunchKernelGGL(gpf_cells_kernel, dim3(1), dim3(1024), 0, s, xyz0, N0, grid_wid, num_bb, gpf_factor, B, dbg);
    hipLaunchKernelGGL(gpf_scatter_kernel, dim3((N0 + 255) / 256), dim3(256), 0, s, norm, N0, B);
    hipLaunchKernelGGL(gpf_rank_kernel, dim3((N0 + 255) / 256), dim3(256), 0, s, norm, N0, B);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(gpf_compact_kernel, dim3(1), dim3(1024), 0, s, B.keep, norm, N0, kept, count, kept_norm);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
