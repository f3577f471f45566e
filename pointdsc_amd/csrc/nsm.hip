// nsm.hip -- a7-a8: Neural Spectral Matching.
//
//   nsm_seed     a7-a8  one wave per seed: k x k feature Gram on the fp16
//                    matrix cores (3-product split), T = F o S in LDS, then all
//                    num_iterations power iterates + per-iterate allclose flags
//   nsm_finish   a8  pair- or batch-global early exit t* = first iterate where every seed
//                    is allclose (torch.allclose over the whole batch, :354)
#include "abi.hpp"
#include "att_stamps.hpp"
#include "h3.hpp"
#include "launch_plan.hpp"
#include "nsm_weight.hpp"

namespace pdsc {

// NSM A/B build knob: 1 (default) the T build on packed fp32 (source, target)
// pairs and the power iterate's norm through the wave-uniform cr_sqrt; 0 the
// scalar T build and sqrtf (the same bits either way)
#ifndef NSM_PK_TBUILD
#define NSM_PK_TBUILD 1
#endif

// -------------------------------------------------------------- a7-a8 NSM
constexpr int KMAX = 64;

// Power iteration of one seed's k x k matrix (models/PointDSC.py:347-358), one
// wave: lane a holds row a of T in registers, v is broadcast from LDS 4 entries
// at a time.  hist[t][a] = iterate t+1; returns bit t = allclose(v_{t+1}, v_t).
// KC: k rounded up to a multiple of 16 (columns past k are zero, their FMAs
// exact no-ops), so k = 40 runs 48-long rows instead of KMAX = 64.
// T's rows in LDS: stride tstride (a multiple of 4), columns k .. KC-1 zero, so
// every row is KC / 4 unconditional 16-B reads (rows past k read as zero rows).
template <int KC>
PDSC_DEV unsigned power_iterate(const float *trow_lds, int tstride, int k, int T, float *vbuf, float *hb, int a) {
    float trow[KC];
    const float *tr = trow_lds + min(a, k - 1) * tstride;
#pragma unroll
    for (int c = 0; c < KC; c += 4) {
        const f32x4 t4 = *reinterpret_cast<const f32x4 *>(tr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) trow[c + e] = a < k ? t4[e] : 0.0f;
    }
    vbuf[a] = 1.0f;
    float v = (a < k) ? 1.0f : 0.0f;
    unsigned flags = 0;
    __builtin_amdgcn_wave_barrier();
    for (int t = 0; t < T; ++t) {
        // four partial sums as two packed pairs: v_pk_fma_f32, two lanes' worth of
        // fma per instruction, the same arithmetic per component
        f32x2 acc01 = {0.0f, 0.0f}, acc23 = {0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < KC; c += 4) {
            const f32x4 vv = *reinterpret_cast<const f32x4 *>(&vbuf[c]);
            acc01 = __builtin_elementwise_fma(f32x2{trow[c], trow[c + 1]}, f32x2{vv[0], vv[1]}, acc01);
            acc23 = __builtin_elementwise_fma(f32x2{trow[c + 2], trow[c + 3]}, f32x2{vv[2], vv[3]}, acc23);
        }
        float nv = (acc01[0] + acc01[1]) + (acc23[0] + acc23[1]);   // (T v)_a  (bmm, :352)
        // no LDS round trip per iterate; every lane holds the same sum, so the
        // square root branches wave-uniformly: the fma-corrected cr_sqrt (the
        // same correctly rounded value) where it is exact, sqrtf below 2^-96
#if NSM_PK_TBUILD
        const float ss = __builtin_bit_cast(
            float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave_sum_dpp(nv * nv))));
        const float nrm = ss >= 0x1p-96f ? cr_sqrt(ss) : sqrtf(ss);
#else
        const float nrm = sqrtf(wave_sum_dpp(nv * nv));
#endif
        nv = nv / (nrm + 1e-6f);                              // :353
        const bool close = (a >= k) || (fabsf(nv - v) <= 1e-8f + 1e-5f * fabsf(v));  // allclose (:354)
        if (__all(close)) flags |= 1u << t;
        if (a < k) hb[(size_t)t * k + a] = nv;
        v = nv;
        __builtin_amdgcn_wave_barrier();
        vbuf[a] = nv;
        __builtin_amdgcn_wave_barrier();
    }
    return flags;
}

// nsm_seed_kernel: one WAVE per (seed, pair), 4 seeds per workgroup.  The
// k x k feature Gram matrix of the seed's neighbourhood comes from the fp16
// matrix cores with the 3-product split (h3.hpp), its operands read
// straight from the split normed copy ns [B][N][2][128] (the same bytes the
// seed kNN reads) into registers: tiles (0,0), (0,1), (1,1) of 32 x 32 for
// k <= 64.  T = F o S (diag 0, :257-278) goes to the wave's slice of LDS, each
// unordered pair evaluated once and mirrored (T exactly symmetric), then the
// same wave runs the power iteration.  No workgroup barriers: waves are
// independent.
constexpr int NSM_PSTR = 8;  // floats per neighbour in the LDS coordinate table
// cr_sqrt / cr_div (pdsc_common.hpp) on two lanes' worth of operands: the
// fma corrections as v_pk_fma_f32, the same operations per component.
PDSC_DEV f32x2 cr_sqrt2(f32x2 x) {
    const f32x2 s = {__builtin_amdgcn_sqrtf(x[0]), __builtin_amdgcn_sqrtf(x[1])};
    const f32x2 dn = {__uint_as_float(__float_as_uint(s[0]) - 1u), __uint_as_float(__float_as_uint(s[1]) - 1u)};
    const f32x2 up = {__uint_as_float(__float_as_uint(s[0]) + 1u), __uint_as_float(__float_as_uint(s[1]) + 1u)};
    const f32x2 rdn = __builtin_elementwise_fma(-dn, s, x), rup = __builtin_elementwise_fma(-up, s, x);
    f32x2 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float v = rdn[i] <= 0.0f ? dn[i] : s[i];
        v = rup[i] > 0.0f ? up[i] : v;
        r[i] = x[i] == 0.0f ? x[i] : v;
    }
    return r;
}
PDSC_DEV f32x2 cr_div2(f32x2 x, f32x2 d, f32x2 rcp) {
    const f32x2 q = x * rcp;
    const f32x2 r = __builtin_elementwise_fma(-q, d, x);
    return __builtin_elementwise_fma(r, rcp, q);
}
// LDS row stride of T for KC-padded rows: 16-B aligned, 13 (KC + 4) / 4 mod 16
// distinct 16-B banks groups over 16 consecutive rows (conflict-free ds_read_b128)
__host__ __device__ constexpr int nsm_tstride(int kc) { return kc + 4; }
// The unordered pairs a < c < KMAX in c-major order (pair p = c (c - 1) / 2 + a,
// packed a | c << 8): the first k (k - 1) / 2 entries are exactly the pairs of
// a k-neighbourhood, for every k -- one table load per pair instead of a
// square-root index decode.
struct NsmPairs {
    unsigned short v[KMAX * (KMAX - 1) / 2];
};
constexpr NsmPairs make_nsm_pairs() {
    NsmPairs t{};
    int p = 0;
    for (int c = 1; c < KMAX; ++c)
        for (int a = 0; a < c; ++a) t.v[p++] = (unsigned short)(a | (c << 8));
    return t;
}
static __constant__ const NsmPairs g_nsm_pairs = make_nsm_pairs();

#ifdef ATT_STAMPS
// Diagnostic build: stamps of 64 evenly spaced workgroups' waves (tools/nsm_stamps.py).
PDSC_DEV unsigned long long *nsm_stamp_ptr(int wave) {
    const int wg = blockIdx.y * gridDim.x + blockIdx.x, str = max(1, (int)(gridDim.x * gridDim.y) / ST_WGS);
    return (wg % str == 0 && wg / str < ST_WGS && wave < 4) ? g_att_stamps + ((wg / str) * 4 + wave) * ST_PER_WAVE
                                                            : nullptr;
}
#define NSM_STAMP(i) ATT_STAMP(nstp, i)
#else
#define NSM_STAMP(i) \
    do {             \
    } while (0)
#endif

// F32 (PDSC_PRECISION_F32): the Gram tiles on exact fp32 MFMA from the fp32
// normed rows (`feats` = normed [B][N][128]); H3: `feats` = the split copy.
template <bool F32, int KC>
__global__ __launch_bounds__(256, 4) void nsm_seed_kernel(const void *__restrict__ feats,
                                                       const float *__restrict__ src,
                                                       const float *__restrict__ tgt,
                                                       const int *__restrict__ knn, int N, int S, int k, int T,
                                                       const float *__restrict__ sigma_p,
                                                       const float *__restrict__ sigma_d_p,
                                                       float *__restrict__ hist, unsigned *__restrict__ seed_flags,
                                                       Ragged rg) {
    extern __shared__ __attribute__((aligned(16))) float nsm_sdyn[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.y, s = blockIdx.x * (blockDim.x >> 6) + wave;
    if (s >= rg.s(b, S)) return;  // wave-uniform (a ragged pair's own seed count; S, N: the strides)
#ifdef ATT_STAMPS
    unsigned long long *nstp = nsm_stamp_ptr(wave);
    ATT_RSTAMP(nstp, 16);
    NSM_STAMP(0);
#endif
    const int tls = nsm_tstride(KC);
    float *Tl = nsm_sdyn + (size_t)wave * (k * tls + k * NSM_PSTR + 64);
    float *P = Tl + k * tls;  // [k][NSM_PSTR]: src xyz, tgt xyz
    float *vb = P + k * NSM_PSTR;
    const float sig = sigma_p[0], sd = sigma_d_p[0];
    const float sig2 = sig * sig, sd2 = sd * sd;
    const float rsig2 = 1.0f / sig2, rsd2 = 1.0f / sd2;
    const int *kr = knn + ((size_t)b * S + s) * k;
    const int idx = min(max(kr[lane < k ? lane : 0], 0), N - 1);
    NSM_STAMP(1);
    // the neighbour's coordinates: loaded now (every lane's idx is a valid row),
    // written to LDS once the Gram gathers are in flight, so the two gathers'
    // latencies overlap
    const float *ps = src + ((size_t)b * N + idx) * 3, *pt = tgt + ((size_t)b * N + idx) * 3;
    const float p0 = ps[0], p1 = ps[1], p2 = ps[2], p3 = pt[0], p4 = pt[1], p5 = pt[2];
    auto store_p = [&] {
        if (lane < k) {
#if NSM_PK_TBUILD
            // (src, tgt) interleaved per axis: the T build's packed fp32 pairs
            *reinterpret_cast<f32x4 *>(P + lane * NSM_PSTR) = f32x4{p0, p3, p1, p4};
            *reinterpret_cast<f32x4 *>(P + lane * NSM_PSTR + 4) = f32x4{p2, p5, 0.0f, 0.0f};
#else
            *reinterpret_cast<f32x4 *>(P + lane * NSM_PSTR) = f32x4{p0, p1, p2, p3};
            *reinterpret_cast<f32x4 *>(P + lane * NSM_PSTR + 4) = f32x4{p4, p5, 0.0f, 0.0f};
#endif
        }
        NSM_STAMP(2);
    };
    // Gram operands streamed one 16-input k-step at a time (16 VGPRs in
    // flight instead of both whole 32-row fragments): the wave fits in 128
    // VGPRs, 4 waves per SIMD to hide the row gathers.  Accumulation order per
    // tile is unchanged (k-steps ascending).
    const int nt = (k + 31) / 32;
    f32x16 G00 = zero16(), G01 = zero16(), G11 = zero16();
    if constexpr (F32) {
        store_p();
        const float *F = static_cast<const float *>(feats) + (size_t)b * N * CH;
        const float *r0 = F + (size_t)__shfl(idx, l32) * CH + 4 * h;
        const float *r1 = F + (size_t)__shfl(idx, 32 + l32) * CH + 4 * h;
#pragma unroll 4
        for (int j = 0; j < CH / 8; ++j) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(r0 + 8 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) G00 = mfma32(av[e], av[e], G00);
            if (nt > 1) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(r1 + 8 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    G01 = mfma32(av[e], bv[e], G01);
                    G11 = mfma32(bv[e], bv[e], G11);
                }
            }
        }
    } else {
        // rows past k are never read back (the T triangle takes a < c < k): their
        // lanes point outside the buffer resource, so those loads return zero
        // without a gather (k = 40: 40 of 64 rows).  Branch-free buffer loads:
        // every k-step's fragments can be in flight together (exec-masked loads
        // in branches were issued one k-step at a time, 16 serial gathers).
        const __amdgpu_buffer_rsrc_t rF =
            h3_rsrc(static_cast<const _Float16 *>(feats) + (size_t)b * N * 2 * CH, (uint32_t)N * 4u * CH);
        const uint32_t oob = 0x80000000u;
        const uint32_t o0 = l32 < k ? (uint32_t)__shfl(idx, l32) * 4u * CH + 16u * h : oob;
        const uint32_t o1 = 32 + l32 < k ? (uint32_t)__shfl(idx, 32 + l32) * 4u * CH + 16u * h : oob;
        auto ld = [&](uint32_t o, int off) {
            return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rF, o, (uint32_t)off, 0));
        };
        // k-step j's four fragments are issued NSM_GLA steps ahead of its MFMAs
        // (the empty asm keeps the scheduler from sinking them to their uses)
        constexpr int NSM_GLA = 3;
        f16x8 fr[8][4];
        auto issue = [&](int j) {
            fr[j][0] = ld(o0, 32 * j);
            fr[j][1] = ld(o0, 2 * CH + 32 * j);
            if (nt > 1) {
                fr[j][2] = ld(o1, 32 * j);
                fr[j][3] = ld(o1, 2 * CH + 32 * j);
            }
        };
#pragma unroll
        for (int j = 0; j < NSM_GLA; ++j) issue(j);
        store_p();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j + NSM_GLA < 8) issue(j + NSM_GLA);
            asm volatile("" ::: "memory");
            G00 = mfma_h3(fr[j][0], fr[j][1], fr[j][0], fr[j][1], G00);
            if (nt > 1) {
                G01 = mfma_h3(fr[j][0], fr[j][1], fr[j][2], fr[j][3], G01);
                G11 = mfma_h3(fr[j][2], fr[j][3], fr[j][2], fr[j][3], G11);
            }
        }
    }
    // The Gram tiles' strict upper triangle (a < c < k) to LDS, then T = F o S
    // evaluated once per unordered pair with the pairs dealt evenly over the
    // 64 lanes (triangular index p -> (a, c)): ceil(k(k-1)/128) passes instead
    // of 16 per Gram tile with most lanes masked off.  Each pair is read and
    // overwritten in place by the one lane that owns it, then mirrored.
    auto gstore = [&](const f32x16 &G, int ta, int tb) {
        const int c = 32 * tb + l32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = 32 * ta + acc_row(r, h);
            if (a < c && c < k) Tl[a * tls + c] = G[r];
        }
    };
    gstore(G00, 0, 0);
    if (nt > 1) {
        gstore(G01, 0, 1);
        gstore(G11, 1, 1);
    }
    NSM_STAMP(3);
    if (lane < k) Tl[lane * tls + lane] = 0.0f;  // diag 0 (:278)
    for (int a0 = 0; a0 < k; a0 += 4) {  // pad columns k .. KC-1 (KC - k < 16): 4 rows x 16 columns per pass
        const int a = a0 + (lane >> 4), c = k + (lane & 15);
        if (a < k && c < KC) Tl[a * tls + c] = 0.0f;
    }
    __builtin_amdgcn_wave_barrier();  // P and the Gram triangle visible to the wave
    const int npair = k * (k - 1) / 2;
    // the pair table entry of the next pass is loaded one pass ahead (a global
    // load per pass otherwise exposes its whole latency, 13 passes at k = 40);
    // k = 1 has no pair: the prefetch still reads inside the table
    unsigned pc_next = g_nsm_pairs.v[max(min(lane, npair - 1), 0)];
    for (int p = lane; p < npair; p += 64) {
        const unsigned pc = pc_next;
        pc_next = g_nsm_pairs.v[min(p + 64, npair - 1)];
        const int a = (int)(pc & 255u), c = (int)(pc >> 8);
        const float g = Tl[a * tls + c];
        const f32x4 pa0 = *reinterpret_cast<const f32x4 *>(P + a * NSM_PSTR);
        const f32x4 pa1 = *reinterpret_cast<const f32x4 *>(P + a * NSM_PSTR + 4);
        const f32x4 pc0 = *reinterpret_cast<const f32x4 *>(P + c * NSM_PSTR);
        const f32x4 pc1 = *reinterpret_cast<const f32x4 *>(P + c * NSM_PSTR + 4);
        // correctly rounded '/' and sqrtf through their fma-corrected forms
        // (pdsc_common.hpp; exact for normal operands, within 1 ulp below 2^-96).
        // (r04: the hardware square root and a reciprocal multiply in the H3 build,
        // -22 VALU per pair, flipped one borderline pair of the recall-parity
        // proxy -- test_recall_parity_synthetic -- so both modes keep these.)
#if NSM_PK_TBUILD
        // the source and target halves as packed fp32 pairs (v_pk_add / mul /
        // fma_f32): per component the same operations in the same order as the
        // scalar form below, so the same bits
        const f32x2 dx = f32x2{pa0[0], pa0[1]} - f32x2{pc0[0], pc0[1]};
        const f32x2 dy = f32x2{pa0[2], pa0[3]} - f32x2{pc0[2], pc0[3]};
        const f32x2 dz = f32x2{pa1[0], pa1[1]} - f32x2{pc1[0], pc1[1]};
        const f32x2 d2 = (dx * dx + dy * dy) + dz * dz;                       // :268 (src, tgt)
        const f32x2 st = cr_sqrt2(d2);
        const float dd = st[0] - st[1];
        // (1 - g) / sigma^2 and dd^2 / sigma_d^2 as one packed correctly rounded division
        const f32x2 qd = cr_div2(f32x2{1.0f - g, dd * dd}, f32x2{sig2, sd2}, f32x2{rsig2, rsd2});
        const f32x2 om = f32x2{1.0f, 1.0f} - qd;
        const float val = fmaxf(om[0], 0.0f) * fmaxf(om[1], 0.0f);            // :259, :270, :277
#else
        const float fm = fmaxf(1.0f - cr_div(1.0f - g, sig2, rsig2), 0.0f);  // :259
        float dx = pa0[0] - pc0[0], dy = pa0[1] - pc0[1], dz = pa0[2] - pc0[2];
        const float ds = cr_sqrt((dx * dx + dy * dy) + dz * dz);    // :268
        dx = pa0[3] - pc0[3];
        dy = pa1[0] - pc1[0];
        dz = pa1[1] - pc1[1];
        const float dt = cr_sqrt((dx * dx + dy * dy) + dz * dz);
        const float dd = ds - dt;
        const float sm = fmaxf(1.0f - cr_div(dd * dd, sd2, rsd2), 0.0f);     // :270
        const float val = fm * sm;                                            // :277
#endif
        Tl[a * tls + c] = val;
        Tl[c * tls + a] = val;
    }
    __builtin_amdgcn_wave_barrier();
    NSM_STAMP(4);
    const unsigned flags = power_iterate<KC>(Tl, tls, k, T, vb, hist + ((size_t)b * S + s) * T * k, lane);
    NSM_STAMP(5);
#ifdef ATT_STAMPS
    ATT_RSTAMP(nstp, 17);
#endif
    // this seed's allclose bits; nsm_finish ANDs a pair's seeds (a per-pair
    // atomicAnd here serialised S atomics per address: 30-60 us of the launch)
    if (lane == 0) seed_flags[(size_t)b * S + s] = flags;
}

size_t nsm_seed_lds_bytes(int k, int wpb) {
    const int kc = (k + 15) / 16 * 16;
    return (size_t)wpb * (k * nsm_tstride(kc) + k * NSM_PSTR + 64) * sizeof(float);
}

hipError_t launch_nsm_seed(const TailPlan &tp, const void *feats, bool f32, const float *src, const float *tgt,
                           const int *knn, int B, int N, int S, int k, int T, const float *sigma, const float *sigma_d,
                           float *hist, unsigned *seed_flags, hipStream_t s, Ragged rg) {
    if (k < 1 || k > KMAX) return hipErrorInvalidValue;
    const int wpb = tp.wpb;
    const dim3 grid((S + wpb - 1) / wpb, B), block(64 * wpb);
    const size_t lds = nsm_seed_lds_bytes(k, wpb);
#define NSM_LAUNCH(F, KC)                                                                                     \
    hipLaunchKernelGGL((nsm_seed_kernel<F, KC>), grid, block, lds, s, feats, src, tgt, knn, N, S, k, T, sigma, \
                       sigma_d, hist, seed_flags, rg)
    const int kc = (k + 15) / 16;
    if (f32) {
        if (kc == 1) NSM_LAUNCH(true, 16); else if (kc == 2) NSM_LAUNCH(true, 32);
        else if (kc == 3) NSM_LAUNCH(true, 48); else NSM_LAUNCH(true, 64);
    } else {
        if (kc == 1) NSM_LAUNCH(false, 16); else if (kc == 2) NSM_LAUNCH(false, 32);
        else if (kc == 3) NSM_LAUNCH(false, 48); else NSM_LAUNCH(false, 64);
    }
#undef NSM_LAUNCH
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void nsm_finish_kernel(const float *__restrict__ hist,
                                                        const unsigned *__restrict__ seed_flags, int S,
                                                        int k, int T, int batch_global, float *__restrict__ weights,
                                                        int *__restrict__ iters_used, Ragged rg) {
    const int b = blockIdx.y, s = blockIdx.x, a = threadIdx.x;
    const int Sb = rg.s(b, S);  // this pair's seeds (a ragged batch); S: the stride
    if (s >= Sb) return;
    // the allclose bits ANDed over the seeds torch.allclose sees at once (:354):
    // the pair's S seeds (a bs = 1 testing forward) or, batch_global, all
    // gridDim.y * S seeds of the call (the training forward's [bs * S, k] iterate)
    // (ragged batches run per pair: pdsc_forward_testing_ragged is B bs = 1 forwards)
    const size_t q0 = batch_global ? 0 : (size_t)b * S, nq = batch_global ? (size_t)gridDim.y * S : (size_t)Sb;
    const int tstar = nsm_tstar(seed_flags, q0, nq, T, a);  // 1-based iterate index
    const float w = nsm_weight(hist, (size_t)b * S + s, tstar, k, T, a);
    if (a < k) weights[((size_t)b * S + s) * k + a] = w;
    if (s == 0 && a == 0 && iters_used) iters_used[b] = tstar;
}

static hipError_t launch_nsm_finish(const float *hist, const unsigned *seed_flags, int B, int S, int k, int T,
                             bool batch_global, float *weights, int *iters_used, hipStream_t s, Ragged rg) {
    if (batch_global && rg.sv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nsm_finish_kernel, dim3(S, B), dim3(64), 0, s, hist, seed_flags, S, k, T, (int)batch_global,
                       weights, iters_used, rg);
    return hipGetLastError();
}

NsmBufs carve_nsm(Carve &c, int B, int S, int k, int T) {
    NsmBufs n;
    n.hist = c.take<float>((size_t)B * S * std::max(T, 1) * k);
    n.mask = c.take<unsigned>((size_t)B * S);  // per-seed allclose bits
    n.weights = c.take<float>((size_t)B * S * k);
    return n;
}

// normed_s: the split normed copy (H3); f32: the Gram reads normed itself
int run_nsm(const TailPlan &tp, const float *normed, const _Float16 *normed_s, bool f32, const float *src,
            const float *tgt, const int *knn, int B, int N, int S, int k, int T, const float *sigma, const float *sigma_d,
            const NsmBufs &nb, float *weights, int *iters, bool batch_global, hipStream_t s, Ragged rg) {
    const void *feats = f32 ? static_cast<const void *>(normed) : static_cast<const void *>(normed_s);
    if (T > 0)
        HIPCHK(launch_nsm_seed(tp, feats, f32, src, tgt, knn, B, N, S, k, T, sigma, sigma_d, nb.hist, nb.mask, s, rg));
    HIPCHK(launch_nsm_finish(nb.hist, nb.mask, B, S, k, T, batch_global, weights, iters, s, rg));
    return PDSC_OK;
}

// the standalone entry's workspace: its own split copy of normed [B][N][2][CH] (the forward
// passes pw_last's), then the stage's buffers
static NsmBufs bind_nsm(Carve &c, int B, int N, int S, int k, int T, _Float16 *&ns) {
    ns = c.take<_Float16>((size_t)B * N * 2 * CH);
    return carve_nsm(c, B, S, k, T);
}

#ifdef ATT_STAMPS
extern "C" int pdsc_diag_nsm_stamps(void *host, size_t bytes) {
    const size_t n = std::min(bytes, sizeof(g_att_stamps));
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_att_stamps), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int pdsc_diag_nsm_stamps_clear() {
    static unsigned long long zero[ST_WGS * 4 * ST_PER_WAVE];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_att_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice) == hipSuccess ? 0
                                                                                                             : -1;
}
#endif

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_nsm_workspace_bytes(int32_t B, int32_t N, int32_t S, int32_t k, int32_t T) {
    Carve c(nullptr);
    _Float16 *ns;
    bind_nsm(c, B, N, S, k, T, ns);
    return c.off;
}

int32_t pdsc_nsm_weights(const float *normed, const float *src, const float *tgt, const int32_t *knn,
                         int32_t B, int32_t N, int32_t C, int32_t S, int32_t k, int32_t T, int32_t precision,
                         const float *sigma, const float *sigma_d, float *weights, int32_t *iters,
                         void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (C != CH) return fail(PDSC_ERR_UNSUPPORTED, "C=%d (only %d)", C, CH);
    if (!normed || !src || !tgt || !knn || !sigma || !sigma_d || !weights || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || S < 1 || k < 1 || k > 63 || N < k + 1 || T < 0 || T > 31)
        return fail(PDSC_ERR_ARG, "B=%d N=%d S=%d k=%d T=%d (1 <= k <= min(63, N-1), 0 <= T <= 31)", B, N, S, k, T);
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision=%d", precision);
    RET_IF(need_ws(ws_bytes, pdsc_nsm_workspace_bytes(B, N, S, k, T)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    _Float16 *ns;
    const NsmBufs nb = bind_nsm(c, B, N, S, k, T, ns);
    const bool f32 = precision == PDSC_PRECISION_F32;
    if (!f32) HIPCHK(launch_split_rows(normed, (size_t)B * N, ns, s));
    return run_nsm(plan_tail(B, N, S), normed, ns, f32, src, tgt, knn, B, N, S, k, T, sigma, sigma_d, nb, weights, iters,
                   true, s);
}

}  // extern "C"
