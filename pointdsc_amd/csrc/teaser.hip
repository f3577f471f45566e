// teaser.hip -- TEASER++ after the inlier selection (include/pdsc.h f9): the
// GNC-TLS rotation estimate over translation-invariant measurements (TIMs), the
// component-wise TLS translation estimate by adaptive voting, and the pieces
// that chain them behind f8's graph and clique (algorithms/TEASER_plus_plus.py:
// 78-93).  The reference calls the x86 teaserpp_python; the algorithm is
// restated in include/pdsc.h, and parity with that library is unpinned.
//
// Both solvers are small-data loops, so each runs as device-side code with no
// host round trip: the rotation as ONE workgroup that keeps the TIMs in
// registers across all GNC iterations, the translation as one workgroup per
// axis around an LDS bitonic sort.  fp64 throughout; every sum goes through a
// fixed tree (per-thread in slot order, xor butterfly inside a wave, the wave
// partials in wave order), no atomics: two calls are bitwise equal.
// DESIGN.md §7 "TEASER++" has the shapes and the numbers.
#include <cmath>

#include "abi.hpp"
#include "pdsc_internal.hpp"

#pragma clang fp contract(off)

namespace pdsc {

namespace {

constexpr int TB = 1024;       // threads of a solver workgroup
constexpr int TW = TB / WAVE;  // its waves

PDSC_DEV double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// ------------------------------------------------------------------ rotation --
// Thread t owns TIMs t + 256 s.  Slots s < REG stay in registers across all
// passes; slots REG <= s < REG + MEM are read again from memory (L2) in every
// pass.  At one wave per SIMD a lane has 512 registers (VGPRs and AGPRs): 24
// slots of 6 doubles are 288 of them and leave room for the Jacobi solve
// without scratch, 32 slots (384) do not; at 1024 threads a lane has 128
// registers and not even 8 slots (96) fit beside the solve.  The work per SIMD
// is the same either way (4 waves x 8 slots or 1 wave x 32), the independent
// slots give the one wave its instruction-level parallelism, and a reduction
// crosses 4 waves, not 16.  The weights sit in LDS, each thread reading and
// writing its own words only.  <4, 0>, <16, 0>, <24, 0> serve K <= 1024, 4096,
// 6144 from registers alone; <24, 8> serves K <= 8192.
constexpr int GB = 256;       // threads of the rotation workgroup
constexpr int GW = GB / WAVE;

template <int NV> PDSC_DEV void gnc_reduce(double (&x)[NV], bool last_is_max, double (*part)[12], int lane, int wave) {
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = (last_is_max && i == NV - 1) ? wave_max_d(x[i]) : wave_sum(x[i]);
    __syncthreads();  // the previous reduction's readers are done with part
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) part[wave][i] = x[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double a = part[0][i];
#pragma unroll
        for (int w = 1; w < GW; ++w) a = (last_is_max && i == NV - 1) ? fmax(a, part[w][i]) : a + part[w][i];
        x[i] = a;  // every thread: the same values in the same order
    }
}

PDSC_DEV double gnc_weight(double r, double th1, double th2, double nb2, double mu) {
    if (r >= th1) return 0.0;
    if (r <= th2) return 1.0;
    return sqrt(nb2 * mu * (mu + 1.0) / r) - mu;
}

PDSC_DEV double gnc_residual(const double R[9], double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = bx - ((R[0] * ax + R[1] * ay) + R[2] * az);
    const double dy = by - ((R[3] * ax + R[4] * ay) + R[5] * az);
    const double dz = bz - ((R[6] * ax + R[7] * ay) + R[8] * az);
    return (dx * dx + dy * dy) + dz * dz;
}

template <int REG, int MEM>
__global__ __launch_bounds__(GB) void gnc_kernel(const double *__restrict__ A, const double *__restrict__ B, int Kin,
                                                 const int *__restrict__ Kdev, double nb2, double factor, int max_iter,
                                                 double cost_thr, double *__restrict__ Rout, double *__restrict__ wout,
                                                 int *__restrict__ inl, pdsc_gnc_info *__restrict__ info) {
    __shared__ double part[GW][12];
    __shared__ double wl[(REG + MEM) * GB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = Kdev ? *Kdev : Kin;  // uniform
    if (K < 1) return;                 // pdsc_teaser_solve's "clique too small"
    double ax[REG], ay[REG], az[REG], bx[REG], by[REG], bz[REG];
#pragma unroll
    for (int s = 0; s < REG; ++s) {
        const int j = tid + s * GB;
        const bool in = j < K;
        const size_t o = 3 * (size_t)(in ? j : 0);
        ax[s] = in ? A[o] : 0.0, ay[s] = in ? A[o + 1] : 0.0, az[s] = in ? A[o + 2] : 0.0;
        bx[s] = in ? B[o] : 0.0, by[s] = in ? B[o + 1] : 0.0, bz[s] = in ? B[o + 2] : 0.0;
        wl[s * GB + tid] = in ? 1.0 : 0.0;  // a slot past K: zero TIM, zero weight, residual 0
    }
#pragma unroll
    for (int s = REG; s < REG + MEM; ++s) wl[s * GB + tid] = tid + s * GB < K ? 1.0 : 0.0;
    double R[9], mu = 0.0, prev = __builtin_inf(), cost = 0.0;
    int it = 0, reason = 0;
    for (;;) {
        // 1. H = sum w a b^T, R = V U^T
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = 0.0;
#pragma unroll
        for (int s = 0; s < REG; ++s) {
            const double w = wl[s * GB + tid];
            const double wx = w * ax[s], wy = w * ay[s], wz = w * az[s];
            h[0] += wx * bx[s], h[1] += wx * by[s], h[2] += wx * bz[s];
            h[3] += wy * bx[s], h[4] += wy * by[s], h[5] += wy * bz[s];
            h[6] += wz * bx[s], h[7] += wz * by[s], h[8] += wz * bz[s];
        }
#pragma unroll
        for (int s = REG; s < REG + MEM; ++s) {
            const int j = tid + s * GB;
            if (j < K) {
                const double *a = A + 3 * (size_t)j, *b = B + 3 * (size_t)j;
                const double w = wl[s * GB + tid];
                const double wx = w * a[0], wy = w * a[1], wz = w * a[2];
                h[0] += wx * b[0], h[1] += wx * b[1], h[2] += wx * b[2];
                h[3] += wy * b[0], h[4] += wy * b[1], h[5] += wy * b[2];
                h[6] += wz * b[0], h[7] += wz * b[1], h[8] += wz * b[2];
            }
        }
        gnc_reduce<9>(h, false, part, lane, wave);
        kabsch_rotation(h, R);  // every thread on the same bits: R is uniform
        ++it;
        // 2. residuals under R, 4. the cost with the old weights; the maximum for pass 0
        double cm[2] = {0.0, 0.0};
#pragma unroll
        for (int s = 0; s < REG; ++s) {
            const double r = gnc_residual(R, ax[s], ay[s], az[s], bx[s], by[s], bz[s]);
            cm[0] += wl[s * GB + tid] * r;
            cm[1] = fmax(cm[1], r);
        }
#pragma unroll
        for (int s = REG; s < REG + MEM; ++s) {
            const int j = tid + s * GB;
            if (j < K) {
                const double *a = A + 3 * (size_t)j, *b = B + 3 * (size_t)j;
                const double r = gnc_residual(R, a[0], a[1], a[2], b[0], b[1], b[2]);
                cm[0] += wl[s * GB + tid] * r;
                cm[1] = fmax(cm[1], r);
            }
        }
        gnc_reduce<2>(cm, true, part, lane, wave);
        cost = cm[0];
        if (it == 1) {  // 3. the first mu from the largest residual
            const double d = 2.0 * cm[1] / nb2 - 1.0;
            if (d <= 0.0) {
                reason = 1;  // every residual inside the bound: weights stay 1
                break;
            }
            mu = 1.0 / d;
        }
        const double th1 = (mu + 1.0) / mu * nb2, th2 = mu / (mu + 1.0) * nb2;
#pragma unroll
        for (int s = 0; s < REG; ++s)  // the residual again (the same bits) rather than REG more live registers
            if (tid + s * GB < K)
                wl[s * GB + tid] = gnc_weight(gnc_residual(R, ax[s], ay[s], az[s], bx[s], by[s], bz[s]), th1, th2, nb2, mu);
#pragma unroll
        for (int s = REG; s < REG + MEM; ++s) {
            const int j = tid + s * GB;
            if (j < K) {
                const double *a = A + 3 * (size_t)j, *b = B + 3 * (size_t)j;
                wl[s * GB + tid] = gnc_weight(gnc_residual(R, a[0], a[1], a[2], b[0], b[1], b[2]), th1, th2, nb2, mu);
            }
        }
        // 5. all uniform values: every thread takes the same branch
        const double diff = fabs(cost - prev);
        mu *= factor;
        prev = cost;
        if (diff < cost_thr) {
            reason = 2;
            break;
        }
        if (it >= max_iter) break;
    }
#pragma unroll
    for (int s = 0; s < REG + MEM; ++s) {
        const int j = tid + s * GB;
        if (j < K) {
            const double w = wl[s * GB + tid];
            if (wout) wout[j] = w;
            if (inl) inl[j] = w >= 0.5 ? 1 : 0;
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Rout[i] = R[i];
        if (info) {
            info->iterations = it;
            info->stop_reason = reason;
            info->cost = cost;
            info->mu = mu;
        }
    }
}

// --------------------------------------------------------------- translation --
// One workgroup per axis.  With one range beta for every measurement the
// consensus set after an event is a window [lo, hi) of the sorted x:
//   the i-th enter (x_(i) - beta):  hi = i + 1, lo = #{k : x_(k) + beta <= x_(i) - beta}
//   the k-th leave (x_(k) + beta):  lo = k + 1, hi = #{i : x_(i) - beta <  x_(k) + beta}
// (a leave sorts before an enter of the same value: its tag is negative), and
// the event's place in the merged sequence is i + lo resp. k + hi.  The sums of
// a window come from prefix sums of (x - x_med) and its square.
constexpr int TLS_MAX = 8192;

struct TlsBest {
    double cost;
    int event;
    int lo, hi;
};
PDSC_DEV bool tls_better(double c, int e, double bc, int be) { return c < bc || (c == bc && e < be); }

__global__ __launch_bounds__(TB) void tls_axis_kernel(const double *__restrict__ src, const double *__restrict__ dst,
                                                      int Kin, const int *__restrict__ Kdev, double beta,
                                                      double *__restrict__ pre, int cap, double *__restrict__ tout) {
    __shared__ double xs[TLS_MAX];
    __shared__ double wtot[2][TW];
    __shared__ double bcost[TW];
    __shared__ int bev[TW], blo[TW], bhi[TW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x;
    const int K = Kdev ? *Kdev : Kin;
    if (K < 1) return;
    int P = 1;
    while (P < K) P <<= 1;
    for (int i = tid; i < P; i += TB) xs[i] = i < K ? dst[3 * (size_t)i + c] - src[3 * (size_t)i + c] : __builtin_inf();
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (P >> 1); p += TB) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;  // i < l < P
                const bool up = (i & k) == 0;
                const double a = xs[i], b = xs[l];
                if ((a > b) == up) xs[i] = b, xs[l] = a;
            }
            __syncthreads();
        }
    // prefix sums, centred on the median: P1[i] = sum_{k < i} (x_(k) - m), P2 of the squares
    double *P1 = pre + (size_t)c * 2 * (cap + 1), *P2 = P1 + (cap + 1);
    const double m = xs[K >> 1];
    const int C = P >= TB ? P / TB : 1;  // elements per thread, contiguous
    const int e0 = tid * C;
    double s1 = 0.0, s2 = 0.0;
    for (int e = 0; e < C; ++e)
        if (e0 + e < K) {
            const double d = xs[e0 + e] - m;
            s1 += d;
            s2 += d * d;
        }
    double i1 = s1, i2 = s2;  // inclusive scan over the wave's threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u1 = __shfl_up(i1, o), u2 = __shfl_up(i2, o);
        if (lane >= o) i1 += u1, i2 += u2;
    }
    if (lane == 63) wtot[0][wave] = i1, wtot[1][wave] = i2;
    __syncthreads();
    double b1 = 0.0, b2 = 0.0;
    for (int w = 0; w < wave; ++w) b1 += wtot[0][w], b2 += wtot[1][w];
    b1 += i1 - s1, b2 += i2 - s2;  // the exclusive prefix at e0
    for (int e = 0; e < C; ++e)
        if (e0 + e < K) {
            P1[e0 + e] = b1, P2[e0 + e] = b2;
            const double d = xs[e0 + e] - m;
            b1 += d;
            b2 += d * d;
            if (e0 + e == K - 1) P1[K] = b1, P2[K] = b2;
        }
    __syncthreads();  // the workgroup's own global stores, read back below
    TlsBest best{__builtin_inf(), 0x7fffffff, 0, 0};
    for (int q = tid; q < 2 * K; q += TB) {
        const bool enter = q < K;
        const int i = enter ? q : q - K;
        int lo, hi;
        if (enter) {
            const double v = xs[i] - beta;
            int a = 0, b = i;  // leaves at or below v lie before i (beta > 0)
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (xs[mid] + beta <= v) a = mid + 1; else b = mid;
            }
            lo = a, hi = i + 1;
        } else {
            const double v = xs[i] + beta;
            int a = i + 1, b = K;  // enters below v include 0 .. i
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (xs[mid] - beta < v) a = mid + 1; else b = mid;
            }
            lo = i + 1, hi = a;
        }
        const int n = hi - lo;
        if (n <= 0) continue;  // an event that leaves the set empty
        const double S1 = P1[hi] - P1[lo], S2 = P2[hi] - P2[lo];
        const double cost = (S2 - S1 * S1 / (double)n) + beta * (double)(K - n);
        const int ev = enter ? i + lo : i + hi;
        if (tls_better(cost, ev, best.cost, best.event)) best = TlsBest{cost, ev, lo, hi};
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(best.cost, o);
        const int oe = __shfl_xor(best.event, o), ol = __shfl_xor(best.lo, o), oh = __shfl_xor(best.hi, o);
        if (tls_better(oc, oe, best.cost, best.event)) best = TlsBest{oc, oe, ol, oh};
    }
    if (lane == 0) bcost[wave] = best.cost, bev[wave] = best.event, blo[wave] = best.lo, bhi[wave] = best.hi;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < TW; ++w)
            if (tls_better(bcost[w], bev[w], best.cost, best.event)) best = TlsBest{bcost[w], bev[w], blo[w], bhi[w]};
        // the first enter always leaves a set of one: a best event exists
        tout[c] = m + (P1[best.hi] - P1[best.lo]) / (double)(best.hi - best.lo);
    }
}

__global__ __launch_bounds__(256) void tls_inlier_kernel(const double *__restrict__ src, const double *__restrict__ dst,
                                                         int Kin, const int *__restrict__ Kdev, double beta,
                                                         const double *__restrict__ t, int *__restrict__ inl) {
    const int K = Kdev ? *Kdev : Kin, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    bool in = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) in = in && fabs((dst[3 * (size_t)j + c] - src[3 * (size_t)j + c]) - t[c]) <= beta;
    inl[j] = in ? 1 : 0;
}

// ------------------------------------------------------------- the solve's glue --
__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ src, const float *__restrict__ tgt, int N,
                                                   float *__restrict__ corr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) corr[6 * (size_t)i + c] = src[3 * (size_t)i + c], corr[6 * (size_t)i + 3 + c] = tgt[3 * (size_t)i + c];
}

// CHAIN TIMs over the clique's members c_0 < ... < c_{Kc-1}; *kdev = Kc, or 0 for Kc <= 1.
__global__ __launch_bounds__(256) void tim_kernel(const float *__restrict__ src, const float *__restrict__ tgt, int N,
                                                  const int *__restrict__ members, const pdsc_clique_result *__restrict__ cr,
                                                  double *__restrict__ A, double *__restrict__ B, int *__restrict__ kdev) {
    int Kc = cr->size;
    Kc = Kc > N ? N : Kc;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *kdev = Kc >= 2 ? Kc : 0;
    if (Kc < 2 || i >= Kc) return;
    const int p = members[i], q = members[i + 1 == Kc ? 0 : i + 1];
    if (p < 0 || p >= N || q < 0 || q >= N) {  // never for f8's members; nothing is read out of range
        for (int c = 0; c < 3; ++c) A[3 * (size_t)i + c] = 0.0, B[3 * (size_t)i + c] = 0.0;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[3 * (size_t)i + c] = (double)src[3 * (size_t)q + c] - (double)src[3 * (size_t)p + c];
        B[3 * (size_t)i + c] = (double)tgt[3 * (size_t)q + c] - (double)tgt[3 * (size_t)p + c];
    }
}

// the clique's source points under R, its target points, both fp64
__global__ __launch_bounds__(256) void rotate_kernel(const float *__restrict__ src, const float *__restrict__ tgt, int N,
                                                     const int *__restrict__ members, const int *__restrict__ kdev,
                                                     const double *__restrict__ R, double *__restrict__ S,
                                                     double *__restrict__ D) {
    const int K = *kdev, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    int p = members[i];
    p = p < 0 ? 0 : (p >= N ? N - 1 : p);
    const double x = src[3 * (size_t)p], y = src[3 * (size_t)p + 1], z = src[3 * (size_t)p + 2];
    S[3 * (size_t)i] = (R[0] * x + R[1] * y) + R[2] * z;
    S[3 * (size_t)i + 1] = (R[3] * x + R[4] * y) + R[5] * z;
    S[3 * (size_t)i + 2] = (R[6] * x + R[7] * y) + R[8] * z;
#pragma unroll
    for (int c = 0; c < 3; ++c) D[3 * (size_t)i + c] = (double)tgt[3 * (size_t)p + c];
}

// One workgroup: the result struct, trans_f32, labels.  Integer counts only.
__global__ __launch_bounds__(256) void teaser_finish_kernel(int N, const int *__restrict__ members,
                                                            const pdsc_clique_result *__restrict__ cr,
                                                            const int *__restrict__ kdev, const double *__restrict__ R,
                                                            const double *__restrict__ t,
                                                            const pdsc_gnc_info *__restrict__ info,
                                                            const int *__restrict__ rinl, const int *__restrict__ tinl,
                                                            pdsc_teaser_result *__restrict__ res,
                                                            float *__restrict__ trans_f32, float *__restrict__ labels) {
    __shared__ int cnt[2][4];
    const int tid = threadIdx.x, K = *kdev;
    if (labels)
        for (int i = tid; i < N; i += 256) labels[i] = 0.0f;
    __syncthreads();
    int nr = 0, nt = 0;
    for (int i = tid; i < K; i += 256) {
        nr += rinl[i];
        nt += tinl[i];
        const int p = members[i];
        if (labels && tinl[i] && p >= 0 && p < N) labels[p] = 1.0f;  // members are distinct: one writer per label
    }
    nr = wave_sum(nr), nt = wave_sum(nt);
    if ((tid & 63) == 0) cnt[0][tid >> 6] = nr, cnt[1][tid >> 6] = nt;
    __syncthreads();
    if (tid != 0) return;
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (K >= 2)
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
            T[4 * r + 3] = t[r];
        }
    for (int i = 0; i < 16; ++i) {
        res->trans[i] = T[i];
        if (trans_f32) trans_f32[i] = (float)T[i];
    }
    res->valid = K >= 2 ? 1 : 0;
    res->clique_size = cr->size;
    res->clique_exact = cr->exact;
    res->roots_incomplete = cr->roots_incomplete;
    res->gnc_iterations = K >= 2 ? info->iterations : 0;
    res->n_rotation_inliers = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3];
    res->n_translation_inliers = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
    res->reserved = 0;
}

struct TeaserWs {
    float *corr;
    unsigned long long *adj;
    int *members, *kdev, *rinl, *tinl;
    pdsc_clique_result *cr;
    pdsc_gnc_info *info;
    double *A, *B, *S, *D, *R, *t, *pre;
    void *clique;
};

double *carve_tls(Carve &c, int K) { return c.take<double>((size_t)3 * 2 * ((size_t)K + 1)); }

TeaserWs carve_teaser(Carve &k, int N) {
    const int W = (N + 63) / 64;
    TeaserWs c;
    c.corr = k.take<float>((size_t)N * 6);
    c.adj = k.take<unsigned long long>((size_t)N * W);
    c.members = k.take<int>((size_t)N);
    c.kdev = k.take<int>(1);
    c.rinl = k.take<int>((size_t)N);
    c.tinl = k.take<int>((size_t)N);
    c.cr = k.take<pdsc_clique_result>(1);
    c.info = k.take<pdsc_gnc_info>(1);
    c.A = k.take<double>((size_t)N * 3);
    c.B = k.take<double>((size_t)N * 3);
    c.S = k.take<double>((size_t)N * 3);
    c.D = k.take<double>((size_t)N * 3);
    c.R = k.take<double>(9);
    c.t = k.take<double>(3);
    c.pre = carve_tls(k, N);
    c.clique = reserve_clique(k, N);
    return c;
}

// Kdev != nullptr (the solve): the count is read on the device (0: return at entry) and K is the capacity the
// launch is shaped for.
hipError_t launch_gnc_rotation(const double *A, const double *B, int K, const int *Kdev, double noise_bound,
                               double factor, int max_iter, double cost_thr, double *R, double *weights, int *inliers,
                               pdsc_gnc_info *info, hipStream_t s) {
    const double nb2 = noise_bound * noise_bound;
#define PDSC_GNC(REG, MEM)                                                                                      \
    hipLaunchKernelGGL((gnc_kernel<REG, MEM>), dim3(1), dim3(GB), 0, s, A, B, K, Kdev, nb2, factor, max_iter, cost_thr, \
                       R, weights, inliers, info)
    if (K > 24 * GB)
        PDSC_GNC(24, 8);
    else if (K > 16 * GB)
        PDSC_GNC(24, 0);
    else if (K > 4 * GB)
        PDSC_GNC(16, 0);
    else
        PDSC_GNC(4, 0);
#undef PDSC_GNC
    return hipGetLastError();
}

// pre: carve_tls(K)'s slice
hipError_t launch_tls_translation(const double *src, const double *dst, int K, const int *Kdev, double noise_bound,
                                  double *t, int *inliers, double *pre, hipStream_t s) {
    hipLaunchKernelGGL(tls_axis_kernel, dim3(3), dim3(TB), 0, s, src, dst, K, Kdev, noise_bound, pre, K, t);
    if (inliers)
        hipLaunchKernelGGL(tls_inlier_kernel, dim3((K + 255) / 256), dim3(256), 0, s, src, dst, K, Kdev, noise_bound, t,
                           inliers);
    return hipGetLastError();
}

constexpr int TEASER_MAX_N = CLIQUE_MAX_N;  // TIMs per thread of the one-workgroup rotation loop, LDS of the sort

int32_t check_teaser_count(const char *what, int32_t n) {
    if (n < 1) return fail(PDSC_ERR_ARG, "%s=%d (need >= 1)", what, n);
    if (n > TEASER_MAX_N) return fail(PDSC_ERR_UNSUPPORTED, "%s=%d > %d", what, n, TEASER_MAX_N);
    return PDSC_OK;
}

int32_t check_noise_bound(double noise_bound) {
    if (!(noise_bound > 0.0) || !std::isfinite(noise_bound))
        return fail(PDSC_ERR_ARG, "noise_bound %g must be > 0 and finite", noise_bound);
    return PDSC_OK;
}

int32_t check_gnc(double gnc_factor, int32_t max_iterations, double cost_threshold) {
    if (!(gnc_factor > 1.0) || !std::isfinite(gnc_factor))
        return fail(PDSC_ERR_ARG, "gnc_factor %g must be > 1 and finite", gnc_factor);
    if (max_iterations < 1) return fail(PDSC_ERR_ARG, "max_iterations=%d (need >= 1)", max_iterations);
    if (cost_threshold != cost_threshold) return fail(PDSC_ERR_ARG, "cost_threshold is NaN");
    return PDSC_OK;
}

}  // namespace
}  // namespace pdsc

using namespace pdsc;

extern "C" {

int32_t pdsc_gnc_tls_rotation(const double *src_tims, const double *dst_tims, int32_t K, double noise_bound,
                              double gnc_factor, int32_t max_iterations, double cost_threshold, double *R,
                              double *weights, int32_t *inliers, pdsc_gnc_info *info, pdsc_stream_t stream) {
    RET_IF(check_teaser_count("K", K));
    RET_IF(check_noise_bound(noise_bound));
    RET_IF(check_gnc(gnc_factor, max_iterations, cost_threshold));
    if (!src_tims || !dst_tims || !R) return fail(PDSC_ERR_ARG, "null pointer");
    HIPCHK(launch_gnc_rotation(src_tims, dst_tims, K, nullptr, noise_bound, gnc_factor, max_iterations, cost_threshold,
                               R, weights, inliers, info, S_(stream)));
    return PDSC_OK;
}

size_t pdsc_tls_translation_workspace_bytes(int32_t K) {
    if (K < 1 || K > TEASER_MAX_N) return 0;
    Carve c(nullptr);
    carve_tls(c, K);
    return c.off;
}

int32_t pdsc_tls_translation(const double *src, const double *dst, int32_t K, double noise_bound, double *t,
                             int32_t *inliers, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_teaser_count("K", K));
    RET_IF(check_noise_bound(noise_bound));
    if (!src || !dst || !t || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_tls_translation_workspace_bytes(K)));
    Carve c(ws);
    HIPCHK(launch_tls_translation(src, dst, K, nullptr, noise_bound, t, inliers, carve_tls(c, K), S_(stream)));
    return PDSC_OK;
}

size_t pdsc_teaser_solve_workspace_bytes(int32_t N) {
    if (N < 1 || N > TEASER_MAX_N) return 0;
    Carve k(nullptr);
    carve_teaser(k, N);
    return k.off;
}

int32_t pdsc_teaser_solve(const float *src, const float *tgt, int32_t N, double noise_bound, double gnc_factor,
                          int32_t max_iterations, double cost_threshold, int64_t node_budget,
                          pdsc_teaser_result *result, float *trans_f32, float *labels, void *ws, size_t ws_bytes,
                          pdsc_stream_t stream) {
    RET_IF(check_teaser_count("N", N));
    RET_IF(check_noise_bound(noise_bound));
    RET_IF(check_gnc(gnc_factor, max_iterations, cost_threshold));
    if (node_budget < 0) return fail(PDSC_ERR_ARG, "node_budget=%lld (need >= 0; 0: the default)", (long long)node_budget);
    if (!src || !tgt || !result || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_teaser_solve_workspace_bytes(N)));
    hipStream_t s = S_(stream);
    const long long budget = node_budget ? (long long)node_budget : CLIQUE_DEFAULT_BUDGET;
    Carve k(ws);
    const TeaserWs c = carve_teaser(k, N);
    const dim3 rows((N + 255) / 256), b256(256);
    hipLaunchKernelGGL(pack_kernel, rows, b256, 0, s, src, tgt, N, c.corr);
    HIPCHK(launch_consistency_graph(c.corr, N, 2.0 * noise_bound, true, c.adj, nullptr, s));
    HIPCHK(launch_max_clique(c.adj, N, budget, true, c.members, c.cr, nullptr, c.clique, s));
    hipLaunchKernelGGL(tim_kernel, rows, b256, 0, s, src, tgt, N, c.members, c.cr, c.A, c.B, c.kdev);
    HIPCHK(launch_gnc_rotation(c.A, c.B, N, c.kdev, noise_bound, gnc_factor, max_iterations, cost_threshold, c.R, nullptr,
                               c.rinl, c.info, s));
    hipLaunchKernelGGL(rotate_kernel, rows, b256, 0, s, src, tgt, N, c.members, c.kdev, c.R, c.S, c.D);
    HIPCHK(launch_tls_translation(c.S, c.D, N, c.kdev, noise_bound, c.t, c.tinl, c.pre, s));
    hipLaunchKernelGGL(teaser_finish_kernel, dim3(1), b256, 0, s, N, c.members, c.cr, c.kdev, c.R, c.t, c.info, c.rinl,
                       c.tinl, result, trans_f32, labels);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
