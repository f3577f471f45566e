// knn.hip -- a6: the seed rows' feature-space kNN.
//
//   knn_dist     a6  seed rows of 2 - 2 F F^T (3-product fp16 MFMA), [B][S][N]
//   knn_select   a6  topk(k+1, smallest)[1:] per seed row (one wave per seed,
//                    row in registers): lane-minimum threshold + compaction +
//                    (key, index) ranking; radix-select fallback
#include "abi.hpp"
#include "h3.hpp"
#include "launch_plan.hpp"

namespace pdsc {

// ------------------------------------------------------------------ a6 kNN
// dist[b][s][j] = 2 - 2 * <normed[seed_s], normed[j]>   (models/common.py:58-60)
// on the fp16 matrix cores with the 3-product split of h3.hpp
// (|error| <= 2^-21 on a distance in [0, 4], i.e. fp32-equivalent): ns is the
// split copy of normed, [B][N][2][128] fp16 in qk_pos order (pw_last writes it).
// A workgroup = 4 waves = 4 tiles of 32 seeds (lane <-> seed fragment, held in
// registers for the whole launch) sweeping KNN_KPB tiles of 32 keys; each key
// tile (32 rows x 512 B of split features, contiguous in HBM) is copied once
// into LDS (16-B chunks XOR-swizzled by row: conflict-free fragment reads) and
// feeds all four waves, so a wave-tile of 24 MFMAs costs ~4 KB of L2 traffic
// instead of 24 KB.  lane <-> key in the accumulator (register r is seed row
// acc_row(r, h)): each store instruction writes 128 contiguous bytes.
constexpr int KNN_KPB = 5;

// order-preserving float -> uint key (+0 and -0 share a key, like float ==).
// The kNN distance rows are stored as these keys (knn_select ranks keys; the
// distances themselves are never read back).
PDSC_DEV uint32_t fkey(float f) {
    if (f == 0.0f) f = 0.0f;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256, 4) void knn_dist_kernel(const _Float16 *__restrict__ ns,
                                                       const int *__restrict__ seeds, int Nstr, int Sstr,
                                                       int kpb, float *__restrict__ dist, Ragged rg) {
    __shared__ f16x8 Bt[32 * 32];
    uint32_t *dkey = reinterpret_cast<uint32_t *>(dist);
    const int b = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int h = lane >> 5, l32 = lane & 31;
    // this pair's keys and seeds; Nstr, Sstr: the batch's strides (rows [b][s] of
    // dist are Nstr long)
    const int N = rg.n(b, Nstr), S = rg.s(b, Sstr);
    if (blockIdx.y * 128 >= S || blockIdx.x * kpb * 32 >= N) return;  // workgroup-uniform
    const int s0 = (blockIdx.y * 4 + wave) * 32;
    const bool active = s0 < S;  // wave-uniform; every wave joins the barriers
    const _Float16 *F = ns + (size_t)b * Nstr * 2 * CH;
    const int sidx = s0 + l32;
    f16x8 ah[8], al[8];
    if (active) {
        const int seed = (sidx < S) ? seeds[(size_t)b * Sstr + sidx] : 0;
        const char *row = reinterpret_cast<const char *>(F + (size_t)min(max(seed, 0), N - 1) * 2 * CH);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ah[j] = *reinterpret_cast<const f16x8 *>(row + 16 * (2 * j + h));
            al[j] = *reinterpret_cast<const f16x8 *>(row + 2 * CH + 16 * (2 * j + h));
        }
    }
    const int nkt = (N + 31) / 32;
    const int t0 = blockIdx.x * kpb, t1 = min(t0 + kpb, nkt);
    // the wave's 32 seed rows through a buffer resource: rows past S fall outside
    // it (their stores are dropped), row r's offset is an SGPR operand
    const uint32_t rowb = (uint32_t)Nstr * 4u;
    const __amdgpu_buffer_rsrc_t rd =
        h3_rsrc(dkey + ((size_t)b * Sstr + min(s0, S)) * Nstr, (uint32_t)max(min(32, S - s0), 0) * rowb);
    // key tile t+1 is loaded into registers while tile t computes and stores
    f16x8 stage[4];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, r = e >> 5, c = e & 31;
            stage[q] = reinterpret_cast<const f16x8 *>(F + (size_t)min(t * 32 + r, N - 1) * 2 * CH)[c];
        }
    };
    if (t0 < t1) load_tile(t0);
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * 32;
        __syncthreads();  // the previous tile's readers are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, r = e >> 5, c = e & 31;
            Bt[r * 32 + (c & 16) + ((c & 15) ^ (r & 15))] = stage[q];
        }
        __syncthreads();
        if (t + 1 < t1) load_tile(t + 1);
        if (!active) continue;
        const int j = j0 + l32;
        f32x16 acc = zero16();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cc = (2 * i + h) ^ (l32 & 15);
            acc = mfma_h3(ah[i], al[i], Bt[l32 * 32 + cc], Bt[l32 * 32 + 16 + cc], acc);
        }
        if (j < N) {
            const uint32_t vo = 4u * j + (uint32_t)(4 * h) * rowb;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                __builtin_amdgcn_raw_buffer_store_b32(fkey(2.0f - 2.0f * acc[r]), rd, vo,
                                                      (uint32_t)((r & 3) + 8 * (r >> 2)) * rowb, 0);
        }
    }
}

static hipError_t launch_knn_dist(const _Float16 *ns, const int *seeds, int B, int N, int S, float *dist,
                           hipStream_t s, Ragged rg) {
    const int nkt = (N + 31) / 32;
    // key tiles per workgroup: KNN_KPB, or 1 when that leaves fewer than 256
    // workgroups (a single N = 1000 pair: 32 instead of 7)
    const long wg5 = (long)((nkt + KNN_KPB - 1) / KNN_KPB) * ((S + 127) / 128) * B;
    const int kpb = wg5 >= 256 ? KNN_KPB : 1;
    hipLaunchKernelGGL(knn_dist_kernel, dim3((nkt + kpb - 1) / kpb, (S + 127) / 128, B), dim3(256), 0, s,
                       ns, seeds, N, S, kpb, dist, rg);
    return hipGetLastError();
}

// PDSC_PRECISION_F32: the same seed rows of 2 - 2 F F^T on exact fp32 MFMA
// (32x32x2), straight from the fp32 normed rows [B][N][128].  A wave owns 32
// seeds (its 64 fp32 fragment values per lane held for the launch) and sweeps
// KNN_KPB key tiles, each key fragment read from L2 as 16-B pieces; k-step
// 4j + e of lane (h, .) is channel 8j + 4h + e for both operands.
__global__ __launch_bounds__(256) void knn_dist_f32_kernel(const float *__restrict__ normed,
                                                           const int *__restrict__ seeds, int Nstr, int Sstr,
                                                           float *__restrict__ dist, Ragged rg) {
    uint32_t *dkey = reinterpret_cast<uint32_t *>(dist);
    const int b = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int h = lane >> 5, l32 = lane & 31;
    const int N = rg.n(b, Nstr), S = rg.s(b, Sstr);  // this pair's keys and seeds
    const int s0 = (blockIdx.y * 4 + wave) * 32;
    if (s0 >= S) return;  // wave-uniform; no barriers
    const float *F = normed + (size_t)b * Nstr * CH;
    const int sidx = s0 + l32;
    const int seed = (sidx < S) ? seeds[(size_t)b * Sstr + sidx] : 0;
    const float *srow = F + (size_t)min(max(seed, 0), N - 1) * CH + 4 * h;
    f32x4 a[CH / 8];
#pragma unroll
    for (int j = 0; j < CH / 8; ++j) a[j] = *reinterpret_cast<const f32x4 *>(srow + 8 * j);
    const int nkt = (N + 31) / 32;
    const int t0 = blockIdx.x * KNN_KPB, t1 = min(t0 + KNN_KPB, nkt);
    for (int t = t0; t < t1; ++t) {
        const int j = t * 32 + l32;
        const float *krow = F + (size_t)min(j, N - 1) * CH + 4 * h;
        f32x16 acc = zero16();
#pragma unroll
        for (int jj = 0; jj < CH / 8; ++jj) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(krow + 8 * jj);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma32(a[jj][e], bv[e], acc);
        }
        if (j < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int sr = s0 + acc_row(r, h);
                if (sr < S) dkey[((size_t)b * Sstr + sr) * Nstr + j] = fkey(2.0f - 2.0f * acc[r]);
            }
        }
    }
}

static hipError_t launch_knn_dist_f32(const float *normed, const int *seeds, int B, int N, int S, float *dist,
                               hipStream_t s, Ragged rg) {
    const int nkt = (N + 31) / 32;
    hipLaunchKernelGGL(knn_dist_f32_kernel, dim3((nkt + KNN_KPB - 1) / KNN_KPB, (S + 127) / 128, B), dim3(256), 0,
                       s, normed, seeds, N, S, dist, rg);
    return hipGetLastError();
}

// fp32 rows [rows][128] -> [rows][2][128] fp16 hi/lo in qk_pos order (standalone API)
__global__ void split_rows_kernel(const float *__restrict__ x, size_t rows, _Float16 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * CH) return;
    const size_t row = i / CH;
    const int c = (int)(i % CH);
    _Float16 hi, lo;
    split_h(x[i], hi, lo);
    out[(size_t)row * 2 * CH + qk_pos(c)] = hi;
    out[(size_t)row * 2 * CH + CH + qk_pos(c)] = lo;
}

hipError_t launch_split_rows(const float *x, size_t rows, _Float16 *out, hipStream_t s) {
    const size_t n = rows * CH;
    hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, rows, out);
    return hipGetLastError();
}

// topk(k+1, smallest) of one seed row, one WAVE per seed (4 per workgroup).
// The row's keys live in registers (R per lane, R*64 >= N; R = 0: re-read
// from memory each pass, any N).  Radix select on the order-preserving keys:
// starting at the highest bit where the row's min and max keys differ (the
// common prefix carries no information -- distances in [0, 4] share their top
// byte, and an 8-bit digit there would put every key in one histogram bin),
// 8-bit digits are histogrammed in LDS until the bin holding the (k+1)-th
// smallest key is taken whole, holds <= KNN_BINCAP keys, or the key is
// resolved.  One ordered pass then collects every key below that bin (ballot
// + popcount compaction) and either the bin's keys (ranked by (key, index) to
// pick the `need` smallest -- usually after ONE histogram pass) or its first
// `need` keys in index order; the k+1 candidates are ranked by (key, index)
// and the first is dropped positionally (models/common.py:68).
// Rows to R = 80 keep 4 waves per SIMD (<= 128 VGPRs; the register fallback
// alone would take 142 at R = 80, and 8 x 5000's 4000 row waves would need two
// rounds of 3: r06, profiles/r06_ab_knn_wpe.log).
constexpr int KNN_BINCAP = 64;
constexpr int KNN_FASTCAP = 128;

#ifdef KNN_DIAG
// Diagnostic build only (-DKNN_DIAG): per launch, how many seed rows took each
// path: [0] bitonic fast path, [1] readlane ranking, [2] radix fallback,
// [3] fallback histogram passes, [4] fallback rows resolved through a small bin.
static __device__ unsigned g_knn_paths[8];
#define KNN_COUNT(i, v) do { if (lane == 0) atomicAdd(&g_knn_paths[i], (unsigned)(v)); } while (0)
extern "C" int pdsc_diag_knn_paths(unsigned *host, int reset) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_knn_paths), sizeof(g_knn_paths), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    static const unsigned zero[8] = {};
    return reset && hipMemcpyToSymbol(HIP_SYMBOL(g_knn_paths), zero, sizeof(zero), 0, hipMemcpyHostToDevice) != hipSuccess
               ? -1 : 0;
}
#else
#define KNN_COUNT(i, v) do { } while (0)
#endif

template <int R>
__global__ __launch_bounds__(256, R <= 80 ? 4 : 1) void knn_select_kernel(const float *__restrict__ dist, int Nstr, int Sstr,
                                                         int k, int *__restrict__ knn, Ragged rg, int bitonic) {
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t ckey[4][64];
    __shared__ int cidx[4][64];
    __shared__ uint32_t bkey[4][KNN_BINCAP];
    __shared__ int bidx[4][KNN_BINCAP];
    __shared__ uint32_t fkeyb[4][KNN_FASTCAP];
    __shared__ int fidxb[4][KNN_FASTCAP];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * (blockDim.x >> 6) + wave;
    // this pair's keys and seeds; Nstr, Sstr: the batch's strides
    const int N = rg.n(b, Nstr), S = rg.s(b, Sstr);
    if (s >= S) return;  // wave-uniform; no workgroup barriers below
    const uint32_t *row = reinterpret_cast<const uint32_t *>(dist) + ((size_t)b * Sstr + s) * Nstr;  // fkey keys
    const uint32_t want = k + 1;
    // Fast path (no atomics): tau0 = the want-th smallest of the 64 per-lane
    // minima bounds the want-th smallest key from above (at least `want` keys are
    // <= tau0), so every key of the answer is <= tau0.  For iid keys about
    // 1.3 * want keys qualify; they are compacted (in any order) and ranked by
    // (key, index).  R > 0: the row is held in registers, lane l owning keys
    // 256 i + 4 l + e (16-B loads); R = 0: re-read from memory.  More than
    // KNN_FASTCAP qualifying keys (heavy ties, adversarial orders) falls through
    // to the radix select below.
    constexpr int NR = R > 0 ? R : 1;
    uint32_t key[NR];  // R > 0: the row in registers (fast path and radix fallback)
    {
        if constexpr (R > 0) {
            if ((Nstr & 3) == 0) {  // rows 16-B aligned (wave-uniform)
                // buffer loads over the row's first round_up(N, 4) keys (lane offset
                // in one VGPR, the key block's offset in the SGPR operand; blocks
                // past them return 0 without a fetch), branch-free, so all R/4
                // loads are in flight together and no per-load 64-bit addresses
                // stay live (97 vs 178 VGPRs at R = 80); keys past N selected away
                const __amdgpu_buffer_rsrc_t rr = h3_rsrc(row, (uint32_t)((N + 3) & ~3) * 4u);
#pragma unroll
                for (int i4 = 0; i4 < R / 4; ++i4) {
                    const u32x4 v = __builtin_bit_cast(
                        u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, 16u * lane, 1024u * i4, 0));
#pragma unroll
                    for (int e = 0; e < 4; ++e) key[4 * i4 + e] = 256 * i4 + 4 * lane + e < N ? v[e] : 0xffffffffu;
                }
            } else {
                // exec-masked dword loads (measured faster here than branch-free
                // buffer or clamped loads: 134 vs 150 / 145 us at 128 x 1289)
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int j = 256 * (i >> 2) + 4 * lane + (i & 3);
                    key[i] = j < N ? row[j] : 0xffffffffu;
                }
            }
        }
    }
    if (want <= 64) {
        const int NI = R > 0 ? R : (N + 63) / 64;
        // index of this lane's i-th key
        auto J = [&](int i) -> int { return R > 0 ? 256 * (i >> 2) + 4 * lane + (i & 3) : lane + 64 * i; };
        auto K = [&](int i) -> uint32_t {
            if constexpr (R > 0) {
                return key[i];
            } else {
                const int j = lane + 64 * i;
                return j < N ? row[j] : 0xffffffffu;
            }
        };
        // Long rows (R >= 32: N > 2048) also keep each lane's second-smallest key:
        // the threshold then comes from 128 values, about half as many keys pass it
        // (clustered rows of a trained network: fewer rows overflow the fast path
        // into the radix select; r06).  Still at least `want` keys <= tau0 (a lane's
        // two values are two of its keys), so the same rows result.
        constexpr bool TWO = R >= 32;
        uint32_t lmin = 0xffffffffu, lmin2 = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (R > 0 || J(i) < N) {  // R > 0: keys past N are ~0u
                const uint32_t x = K(i);
                if constexpr (TWO) lmin2 = min(lmin2, max(lmin, x));
                lmin = min(lmin, x);
            }
        // tau0 = the want-th smallest lane minimum (TWO: of the 128 lane minima and
        // second minima): the smallest value v with #{lanes: lmin <= v} (+ #{lanes:
        // lmin2 <= v}) >= want, built bit by bit from the top (one compare + ballot
        // + scalar popcount per bit instead of 64 readlanes)
        uint32_t tau0 = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t probe = tau0 | ((1u << bit) - 1u);  // this bit 0, all lower bits 1
            uint32_t cnt = (uint32_t)__popcll(__ballot(lmin <= probe));
            if constexpr (TWO) cnt += (uint32_t)__popcll(__ballot(lmin2 <= probe));
            if (cnt < want) tau0 |= 1u << bit;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        // the key indices recomputed from an opaque base: otherwise the compiler
        // keeps the R load-time indices live across the threshold search
        int lb = R > 0 ? 4 * lane : lane;
        asm volatile("" : "+v"(lb));
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = R > 0 ? 256 * (i >> 2) + lb + (i & 3) : lb + 64 * i;
            const uint32_t u = K(i);
            const bool q = j < N && u <= tau0;
            const unsigned long long m = __ballot(q);
            if (m) {
                if (q) {
                    const uint32_t pos = c + __popcll(m & below);
                    if (pos < KNN_FASTCAP) {
                        fkeyb[wave][pos] = u;
                        fidxb[wave][pos] = j;
                    }
                }
                c += __popcll(m);
            }
        }
        if (bitonic && c <= 64) {  // wave-uniform
            // the c <= 64 candidates sorted by (key, index) across the wave (a
            // 21-stage bitonic network of lane-pair exchanges): lane r then holds
            // rank r, the same order the compare ranking below computes
            __builtin_amdgcn_wave_barrier();
            uint32_t kk = lane < (int)c ? fkeyb[wave][lane] : 0xffffffffu;
            int ii = lane < (int)c ? fidxb[wave][lane] : 0x7fffffff;
#pragma unroll
            for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    const uint32_t ok = (uint32_t)__shfl_xor((int)kk, stride);
                    const int oi = __shfl_xor(ii, stride);
                    const bool other_less = (ok < kk) | ((ok == kk) & (oi < ii));
                    // the lower lane of an ascending pair (or the upper of a descending one) keeps the smaller
                    const bool keep_small = ((lane & stride) == 0) == ((lane & size) == 0);
                    if (keep_small == other_less) {
                        kk = ok;
                        ii = oi;
                    }
                }
            int *out = knn + ((size_t)b * Sstr + s) * k;
            if (lane > 0 && lane < (int)want && lane < (int)c) out[lane - 1] = ii;  // drop position 0 (:68)
            KNN_COUNT(0, 1);
            return;
        }
        if (c <= KNN_FASTCAP) {
            __builtin_amdgcn_wave_barrier();
            const int e0 = lane, e1 = lane + 64;
            const uint32_t k0 = e0 < (int)c ? fkeyb[wave][e0] : 0xffffffffu;
            const int i0 = e0 < (int)c ? fidxb[wave][e0] : 0x7fffffff;
            const uint32_t k1 = e1 < (int)c ? fkeyb[wave][e1] : 0xffffffffu;
            const int i1 = e1 < (int)c ? fidxb[wave][e1] : 0x7fffffff;
            // ranks by (key, index): candidate m broadcast from lane m % 64 by
            // v_readlane (no LDS round trip per candidate)
            uint32_t r0 = 0, r1 = 0;
            for (int m = 0; m < min((int)c, 64); ++m) {
                const uint32_t mu = __builtin_amdgcn_readlane(k0, m);
                const int mi = __builtin_amdgcn_readlane(i0, m);
                r0 += (mu < k0) || (mu == k0 && mi < i0);
                r1 += (mu < k1) || (mu == k1 && mi < i1);
            }
            for (int m = 64; m < (int)c; ++m) {
                const uint32_t mu = __builtin_amdgcn_readlane(k1, m - 64);
                const int mi = __builtin_amdgcn_readlane(i1, m - 64);
                r0 += (mu < k0) || (mu == k0 && mi < i0);
                r1 += (mu < k1) || (mu == k1 && mi < i1);
            }
            int *out = knn + ((size_t)b * Sstr + s) * k;
            if (e0 < (int)c && r0 > 0 && r0 < want) out[r0 - 1] = i0;  // drop position 0 (:68)
            if (e1 < (int)c && r1 > 0 && r1 < want) out[r1 - 1] = i1;
            KNN_COUNT(1, 1);
            return;
        }
    }
    KNN_COUNT(2, 1);
    if constexpr (R > 0) {
        // Radix fallback on the row held in registers (r06: the memory form below
        // re-reads the row from L2 in every histogram pass, one dependent load per
        // atomic; the single N = 5000 pair's clustered rows took 90 us in it).
        // Lane l holds keys 256 b + 4 l + e (block b = i / 4, e = i % 4, ~0u past N):
        // counting passes do not care about order, and the collection pass ranks
        // a block's keys in index order from its four ballots.  The same selection
        // as the memory form, so the same kNN rows.
        uint32_t kmin = 0xffffffffu, kmax = 0u;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool valid = 256 * (i >> 2) + 4 * lane + (i & 3) < N;
            if (valid) {
                kmin = min(kmin, key[i]);
                kmax = max(kmax, key[i]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
            kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
        }
        uint32_t *hb = hist[wave];
        uint32_t need = want, prefix = kmin, mask = 0xffffffffu, bin_cnt = want;
        bool small_bin = false;
        if (kmin != kmax) {
            const int top = 31 - __clz((int)(kmin ^ kmax));
            mask = top == 31 ? 0u : ~((2u << top) - 1u);
            prefix = kmin & mask;
            for (int hi = top; hi >= 0; hi -= 8) {
                const int lo = max(hi - 7, 0);
                const uint32_t dm = (2u << (hi - lo)) - 1u;
                KNN_COUNT(3, 1);
#pragma unroll
                for (int e = 0; e < 4; ++e) hb[lane + 64 * e] = 0;
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const uint32_t u = key[i];
                    if (256 * (i >> 2) + 4 * lane + (i & 3) < N && (u & mask) == prefix)
                        atomicAdd(&hb[(u >> lo) & dm], 1u);
                    if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_wave_barrier();
                uint32_t c[4], tot = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    c[e] = hb[4 * lane + e];
                    tot += c[e];
                }
                uint32_t incl = tot;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                const uint32_t base = incl - tot;
                uint32_t my_bin = 0, my_need = 0, my_cnt = 0;
                const bool hit = base < need && need <= incl;
                if (hit) {
                    uint32_t cum = base;
                    bool done = false;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!done && cum + c[e] >= need) {
                            my_bin = 4 * lane + e;
                            my_need = need - cum;
                            my_cnt = c[e];
                            done = true;
                        }
                        cum += c[e];
                    }
                }
                const int src_lane = __ffsll((unsigned long long)__ballot(hit)) - 1;
                const uint32_t bin = __shfl(my_bin, src_lane);
                const uint32_t cnt = __shfl(my_cnt, src_lane);
                need = __shfl(my_need, src_lane);
                prefix |= bin << lo;
                mask |= dm << lo;
                bin_cnt = cnt;
                if (cnt == need) break;
                if (cnt <= KNN_BINCAP) {
                    small_bin = true;
                    break;
                }
            }
        }
        const uint32_t nless = want - need;
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t pl = 0, pe = 0;
#pragma unroll
        for (int i4 = 0; i4 < R / 4; ++i4) {
            bool less[4], eq[4];
            unsigned long long lm[4], em[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t u = key[4 * i4 + e], um = u & mask;
                const bool valid = 256 * i4 + 4 * lane + e < N;
                less[e] = valid && um < prefix;
                eq[e] = valid && um == prefix;
                lm[e] = __ballot(less[e]);
                em[e] = __ballot(eq[e]);
            }
            // index-order rank inside the block: every key of the lanes below, then
            // this lane's keys before e
            uint32_t lb = 0, eb = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lb += __popcll(lm[e] & below);
                eb += __popcll(em[e] & below);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 256 * i4 + 4 * lane + e;
                const uint32_t u = key[4 * i4 + e];
                if (less[e]) {
                    const uint32_t pos = pl + lb;
                    if (pos < want) {
                        ckey[wave][pos] = u;
                        cidx[wave][pos] = j;
                    }
                }
                if (eq[e]) {
                    const uint32_t r = pe + eb;
                    if (small_bin) {
                        bkey[wave][r] = u;
                        bidx[wave][r] = j;
                    } else if (r < need) {
                        ckey[wave][nless + r] = u;
                        cidx[wave][nless + r] = j;
                    }
                }
                lb += less[e];
                eb += eq[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pl += __popcll(lm[e]);
                pe += __popcll(em[e]);
            }
            __builtin_amdgcn_sched_barrier(0);  // one block's ballots live at a time
        }
        __builtin_amdgcn_wave_barrier();
        if (small_bin) KNN_COUNT(4, 1);
        if (small_bin) {
            for (int e = lane; e < (int)bin_cnt; e += 64) {
                const uint32_t ku = bkey[wave][e];
                const int ki = bidx[wave][e];
                uint32_t rank = 0;
                for (int m = 0; m < (int)bin_cnt; ++m) {
                    const uint32_t mu = bkey[wave][m];
                    rank += (mu < ku) || (mu == ku && bidx[wave][m] < ki);
                }
                if (rank < need) {
                    ckey[wave][nless + rank] = ku;
                    cidx[wave][nless + rank] = ki;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (lane < (int)want) {
            const uint32_t ku = ckey[wave][lane];
            const int ki = cidx[wave][lane];
            int rank = 0;
            for (int m = 0; m < (int)want; ++m) {
                const uint32_t mu = ckey[wave][m];
                rank += (mu < ku) || (mu == ku && cidx[wave][m] < ki);
            }
            if (rank > 0) knn[((size_t)b * Sstr + s) * k + rank - 1] = ki;  // drop position 0 (:68)
        }
        return;
    }
    // Radix fallback, keys re-read from memory (lane l owns keys l + 64 i, so a
    // ballot over lanes visits keys in index order).
    const int NI = (N + 63) / 64;
    auto K = [&](int i) -> uint32_t {
        const int j = lane + 64 * i;
        return j < N ? row[j] : 0xffffffffu;
    };
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    for (int i = 0; i < NI; ++i) {
        if (lane + 64 * i < N) {
            const uint32_t u = K(i);
            kmin = min(kmin, u);
            kmax = max(kmax, u);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
    }
    uint32_t *hb = hist[wave];
    uint32_t need = want, prefix = kmin, mask = 0xffffffffu, bin_cnt = want;
    bool small_bin = false;  // the bin holding the (k+1)-th key has <= KNN_BINCAP keys: rank them directly
    if (kmin != kmax) {
        const int top = 31 - __clz((int)(kmin ^ kmax));  // highest differing bit
        mask = top == 31 ? 0u : ~((2u << top) - 1u);
        prefix = kmin & mask;
        for (int hi = top; hi >= 0; hi -= 8) {
            const int lo = max(hi - 7, 0);
            const uint32_t dm = (2u << (hi - lo)) - 1u;  // digit = bits [lo, hi]
            KNN_COUNT(3, 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) hb[lane + 64 * e] = 0;
            __builtin_amdgcn_wave_barrier();
            for (int i = 0; i < NI; ++i) {
                const uint32_t u = K(i);
                if (lane + 64 * i < N && (u & mask) == prefix) atomicAdd(&hb[(u >> lo) & dm], 1u);
            }
            __builtin_amdgcn_wave_barrier();
            uint32_t c[4], tot = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = hb[4 * lane + e];
                tot += c[e];
            }
            uint32_t incl = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            const uint32_t base = incl - tot;
            uint32_t my_bin = 0, my_need = 0, my_cnt = 0;
            const bool hit = base < need && need <= incl;
            if (hit) {
                uint32_t cum = base;
                bool done = false;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (!done && cum + c[e] >= need) {
                        my_bin = 4 * lane + e;
                        my_need = need - cum;
                        my_cnt = c[e];
                        done = true;
                    }
                    cum += c[e];
                }
            }
            const int src_lane = __ffsll((unsigned long long)__ballot(hit)) - 1;
            const uint32_t bin = __shfl(my_bin, src_lane);
            const uint32_t cnt = __shfl(my_cnt, src_lane);
            need = __shfl(my_need, src_lane);
            prefix |= bin << lo;
            mask |= dm << lo;
            bin_cnt = cnt;
            if (cnt == need) break;  // the whole bin is taken: no need to resolve further
            if (cnt <= KNN_BINCAP) {
                small_bin = true;
                break;
            }
        }
    }
    // take every key with (u & mask) < prefix and the first `need` keys with (u & mask) == prefix
    const uint32_t nless = want - need;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t pl = 0, pe = 0;
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        const uint32_t u = K(i);
        const uint32_t um = u & mask;
        const bool valid = j < N;
        const bool less = valid && um < prefix, eq = valid && um == prefix;
        const unsigned long long lm = __ballot(less), em = __ballot(eq);
        if (less) {
            const uint32_t pos = pl + __popcll(lm & below);
            if (pos < want) {
                ckey[wave][pos] = u;
                cidx[wave][pos] = j;
            }
        }
        if (eq) {
            const uint32_t r = pe + __popcll(em & below);
            if (small_bin) {  // every key of the bin, ranked below
                bkey[wave][r] = u;
                bidx[wave][r] = j;
            } else if (r < need) {
                ckey[wave][nless + r] = u;
                cidx[wave][nless + r] = j;
            }
        }
        pl += __popcll(lm);
        pe += __popcll(em);
    }
    __builtin_amdgcn_wave_barrier();
    if (small_bin) KNN_COUNT(4, 1);
    if (small_bin) {  // the `need` smallest (key, index) of the bin's bin_cnt keys
        for (int e = lane; e < (int)bin_cnt; e += 64) {
            const uint32_t ku = bkey[wave][e];
            const int ki = bidx[wave][e];
            uint32_t rank = 0;
            for (int m = 0; m < (int)bin_cnt; ++m) {
                const uint32_t mu = bkey[wave][m];
                rank += (mu < ku) || (mu == ku && bidx[wave][m] < ki);
            }
            if (rank < need) {
                ckey[wave][nless + rank] = ku;
                cidx[wave][nless + rank] = ki;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < (int)want) {
        const uint32_t ku = ckey[wave][lane];
        const int ki = cidx[wave][lane];
        int rank = 0;
        for (int m = 0; m < (int)want; ++m) {
            const uint32_t mu = ckey[wave][m];
            rank += (mu < ku) || (mu == ku && cidx[wave][m] < ki);
        }
        if (rank > 0) knn[((size_t)b * Sstr + s) * k + rank - 1] = ki;  // drop position 0 (:68)
    }
}

static hipError_t launch_knn_select(const TailPlan &tp, const float *dist, int B, int N, int S, int k, int *knn,
                             hipStream_t s, Ragged rg) {
    const int wpb = tp.wpb, bit = tp.knn_bitonic;
    const dim3 grid((S + wpb - 1) / wpb, B), block(64 * wpb);
    const int R = (N + 63) / 64;
    if (R <= 16)
        hipLaunchKernelGGL(knn_select_kernel<16>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 32)
        hipLaunchKernelGGL(knn_select_kernel<32>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 48)
        hipLaunchKernelGGL(knn_select_kernel<48>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 64)
        hipLaunchKernelGGL(knn_select_kernel<64>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 80)
        hipLaunchKernelGGL(knn_select_kernel<80>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 96)
        hipLaunchKernelGGL(knn_select_kernel<96>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else if (R <= 128)
        hipLaunchKernelGGL(knn_select_kernel<128>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    else
        hipLaunchKernelGGL(knn_select_kernel<0>, grid, block, 0, s, dist, N, S, k, knn, rg, bit);
    return hipGetLastError();
}

// a6 (:250-252) for the forwards: knn [B][S][k]; dist [B][S][N] scratch
int run_seed_knn(const TailPlan &tp, const float *normed, const _Float16 *normed_s, bool f32, const int *seeds, int B,
                 int N, int S, int k, float *dist, int *knn, hipStream_t s, Ragged rg) {
    // (no zero fill of knn: knn_select writes all k entries of every seed row it
    // owns -- ranks 1 .. k of k + 1 distinct (key, index) candidates -- and the
    // rows past a ragged pair's own seeds are never read; readers clamp indices)
    if (f32) {
        HIPCHK(launch_knn_dist_f32(normed, seeds, B, N, S, dist, s, rg));
    } else {
        HIPCHK(launch_knn_dist(normed_s, seeds, B, N, S, dist, s, rg));
    }
    HIPCHK(launch_knn_select(tp, dist, B, N, S, k, knn, s, rg));
    return PDSC_OK;
}

// the seed rows' distances [B][S][N] and the split normed copy [B][N][2][CH]
struct SeedKnnBufs {
    float *dist;
    _Float16 *ns;
};
static void bind_seed_knn(Carve &c, int B, int N, int S, SeedKnnBufs &W) {
    W.dist = c.take<float>((size_t)B * S * N);
    W.ns = c.take<_Float16>((size_t)B * N * 2 * CH);
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_seed_knn_workspace_bytes(int32_t B, int32_t N, int32_t S) {
    Carve c(nullptr);
    SeedKnnBufs W;
    bind_seed_knn(c, B, N, S, W);
    return c.off;
}

int32_t pdsc_seed_knn(const float *normed, const int32_t *seeds, int32_t B, int32_t N, int32_t C,
                      int32_t S, int32_t k, int32_t precision, int32_t *knn, void *ws, size_t ws_bytes,
                      pdsc_stream_t stream) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision=%d", precision);
    if (C != CH) return fail(PDSC_ERR_UNSUPPORTED, "C=%d (only %d)", C, CH);
    if (!normed || !seeds || !knn || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || S < 1 || k < 1 || k + 1 > N || k > 63) return fail(PDSC_ERR_ARG, "B=%d N=%d S=%d k=%d", B, N, S, k);
    RET_IF(need_ws(ws_bytes, pdsc_seed_knn_workspace_bytes(B, N, S)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    SeedKnnBufs W;
    bind_seed_knn(c, B, N, S, W);
    const bool f32 = precision == PDSC_PRECISION_F32;
    if (!f32) HIPCHK(launch_split_rows(normed, (size_t)B * N, W.ns, s));
    return run_seed_knn(plan_tail(B, N, S), normed, W.ns, f32, seeds, B, N, S, k, W.dist, knn, s);
}

}  // extern "C"
