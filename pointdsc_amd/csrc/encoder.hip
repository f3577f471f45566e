// encoder.hip -- a2-a4: SCNonlocal encoder, F.normalize and the classifier.
//
// Replaces models/PointDSC.py:9-77 (NonLocalBlock / NonLocalNet), :155-156 and
// :171.  Layout in HBM (per pair b, N padded to Npad = round_up(N,128) rows):
//   feat          : [B][Npad][128] fp32, point-major (row = correspondence)
//   Qs, Ks, Vs    : the fp16 hi/lo split layouts of h3.hpp (4 B/element)
//   M             : [B][N][N] fp32 (a1 output; symmetric)
//   opart, ml     : [B][nsplit][Npad][128], [B][nsplit][Npad][2] attention partials
//
// Kernels per forward: pw_first (layer0 + PointCN_0 + QKV_0), then per layer
// attention_l (+ pw_mid_l = combine + fc_message_l + residual + PointCN_{l+1}
// + QKV_{l+1}), and pw_last (combine + fc_message + residual + normalize +
// classifier).  The pointwise products run on v_mfma_f32_32x32x16_f16 with the
// 3-product split of h3.hpp (activations split as read from LDS,
// weights pre-split and power-of-two scaled at pack time); their Q/K/V
// epilogues write the fp16 hi/lo splits that the attention consumes.
//
// Attention (attention_h3.hpp; flash-style, never materialising the N x N
// logits): 3 fp16 MFMAs per fp32 product (hi.hi + hi.lo + lo.hi, 22-bit
// operands, fp32 accumulation) -- fp32-equivalent results at 16/3 x the fp32
// matrix rate; logits = M_ij * s_ij / sqrt(C) with M read column-wise (M
// symmetric => coalesced 128-B rows); incompatible pairs keep logit 0 (not
// -inf) exactly as :41; online softmax with a lazily re-based running max;
// split-K over keys when B*N is too small to fill 256 CUs.
//
// This file: the plan (plan_encoder), the register-chained pointwise chain and
// the fused attention + chain kernels, the launch_pw_* dispatchers, the row's
// run loop (run_encoder, its parts on side streams) and its entry points.
// pack.hip packs the weights, attention.hip launches the split attention,
// pw_lds.hpp holds the LDS-tiled chain.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "abi.hpp"
#include "encoder.hpp"
#include "pw_lds.hpp"

namespace pdsc {

static thread_local int g_diag_qkv_delay = 0;  // pdsc_diag_qkv_delay (tests only)

// pw2 for launches of at least 320 128-point workgroups, 1.25 per CU.  Measured
// encoder ms, pw2 vs pw_mid chains: 8 x N=5000 (320 WGs; 3 key splits) 4.48
// vs 4.61; 40 x 1000 (320, fused) 1.47 vs 1.78; 56 x 1000 (448, fused) 1.68 vs
// 2.12; 32 x 1000 (256) 1.26 vs 1.22 and 1.24 fused; 16 x 1000 (128) 0.95 vs 0.80.
static bool use_pw2(const Knobs &k, int B, int Npad, bool f32) {
    if (f32 || k.pw2 == 0) return false;
    return k.pw2 == 2 || (long)B * ((Npad + PW2_PTS - 1) / PW2_PTS) >= 320;
}

// The encoder's plan (launch_plan.hpp): every rule that picks a kernel and its
// grid for a shape, each with the measurements behind it.
EncoderPlan plan_encoder(int B, int N, bool f32, bool dense_m_caller, bool allow_fused) {
    const Knobs &k = knobs();
    EncoderPlan p{};
    p.B = B;
    p.N = N;
    p.Npad = round_up(N, QB);
    p.f32 = f32;
    p.nw = ATT_NW;
    p.ws = 1;
    const int nst = (N + H3_TILE - 1) / H3_TILE;
    const long blocks = (long)B * ((N + QB - 1) / QB);  // of 128 queries
    auto take = [&p](AttnKind kind, const auto &g) {
        p.kind = kind;
        p.nqb = g.nqb;
        p.sps = g.sps;
        p.nsplit = g.nsplit;
    };

    // attn_pw2 wherever pw2 runs and the attention has one key split
    const AttnGridH3 fg = attention_h3_grid<PW2_W>(B, N, k.target * 4 / PW2_W);
    p.pw2 = use_pw2(k, B, p.Npad, f32);
    const bool fused = allow_fused && k.fuse && p.pw2 && fg.nsplit == 1 && fg.nqb * PW2_PTS == p.Npad;

    // The 64-query-wave attention (attention_w64.hpp, one 4-wave workgroup per CU,
    // symmetric-packed M) for the split path: from 128 blocks of 256 queries
    // (8 x 5000: 160 blocks, 3 key splits).
    const bool w64 = !fused && !f32 && !dense_m_caller && k.w64 != 0 &&
                     (k.w64 == 1 || (long)B * ((N + W64_QPB - 1) / W64_QPB) >= 128);
    if (f32) {
        take(ATT_F32, attention_grid<ATT_NW, ATT_F32_KTS>(B, N, k.target));
    } else if (w64) {
        const int nwg = k.target / 2;
        const AttnGridH3 g = attention_w64_grid(B, N, nwg);
        take(ATT_W64, g);
        // Stream-K (one workgroup per CU) for a uniform batch: when one round of nwg
        // workgroups of ceil(T / nwg) tiles (+ ~2 tiles for a workgroup's second
        // segment) beats the split grid's rounds of sps tiles.
        const long T = (long)B * g.nqb * nst, rounds = ((long)B * g.nqb * g.nsplit + nwg - 1) / nwg;
        if (k.w64_sk && T >= 4L * nwg && (T + nwg - 1) / nwg + 2 < rounds * g.sps) {
            p.kind = ATT_W64_SK;
            p.sk_wgs = nwg;
            p.nsplit = std::max(g.nsplit, w64_sk_nsplit(B, g.nqb, nst, nwg));
        }
    } else {
        // The smallest batches (at most 16 query blocks of 128 and splits of <= 24 key
        // tiles: a single pair to N = 1536, two to 1024, four to 512): 32-query
        // workgroups whose key splits fill ONE round of tiny_slots (128) workgroups (a
        // 1000-key pair: 32 blocks x 4 splits of 8 tiles, run by attention_h3_ws_kernel's
        // 4 waves) instead of 16 blocks x 16 splits of 2 -- a quarter of the split
        // partials, so pw_mid combines them itself (precombine: fewer than 16 splits)
        // and the combine_rows launch goes.
        // The slot target, 128 (ms per forward, wave-split kernel,
        // profiles/r06_ab_tiny_slots.log): 1 x 1000 0.374 at 256 slots -> 0.366 at 128
        // (4 splits of 8 tiles, 2 per wave; half the partials again) -> 0.385 at 96,
        // 0.415 at 64; 2 x 500 0.342 -> 0.316; 1 x 700 0.362 -> 0.345.
        // Splits of at most 24 key tiles (6 per wave of the wave-split kernel): ms per
        // forward, 8 -> 16-block limit (profiles/r06_ab_tiny16.log): 2 x 1000 0.431 ->
        // 0.382, 4 x 500 0.374 -> 0.324, 1 x 1500 (24 tiles) 0.456 -> 0.439, but 1 x 2000
        // (32 tiles) 0.489 -> 0.504, which keeps the two-wave split plan.
        const AttnGridH3 tg = attention_h3_grid<1>(B, N, std::min(k.target, k.tiny_slots));
        if (blocks <= k.tiny && tg.sps <= 24) {
            // The tiles spread over the workgroup's waves where each split has at least
            // 4 tiles (measured, ms per forward, 1 -> 4 waves: 1 x 1000 (4 tiles per
            // split) 0.393 -> 0.377; 1 x 700 (2 tiles) 0.366 -> 0.371, 2 x 500 0.347 ->
            // 0.351, so shorter splits keep the one-wave kernel; profiles/r06_ab_att_ws.log).
            const bool wave_split = k.ws > 1 && tg.sps >= 4;
            take(wave_split ? ATT_H3_WS : ATT_H3, tg);
            p.nw = 1;
            p.ws = wave_split ? k.ws : 1;
        } else {
            // Waves (x 32 queries) per workgroup: 4, except 2 for batches of at most 16
            // blocks of 128 queries (single pairs up to N = 2048), whose launch is
            // latency-bound: twice the query blocks, each workgroup's K/V stream shared
            // by 2 waves.  Measured (ms per forward, two A/B rounds on one box,
            // profiles/r06_ab_att_nw.log): 1 x 1000 0.4235 -> 0.417, 1 x 2000 0.531 ->
            // 0.504, 1 x 5000 (not covered) equal; 1 wave 0.4185 / 0.515.
            p.nw = blocks <= 16 ? k.nw : ATT_NW;
            take(ATT_H3, p.nw == 1   ? attention_h3_grid<1>(B, N, k.target)
                         : p.nw == 2 ? attention_h3_grid<2>(B, N, k.target)
                                     : attention_h3_grid<ATT_NW>(B, N, k.target));
        }
        // long splits: the early-issue loop (attention_h3_core's EARLY; measured there)
        p.early = p.kind == ATT_H3 && p.sps >= 3;
    }

    // The tiniest batches (<= 16 query blocks of 128, >= 16 key splits: a single
    // N = 2000 pair) combine the attention partials in their own launch
    // (combine_rows) rather than in the pointwise kernel's prologue: measured
    // 0.511 -> 0.482 ms per single-pair forward (N = 1000, before the tiny plan),
    // but slower from 4 pairs of N = 1000 on (an extra launch per layer).
    p.precombine = k.precombine && !f32 && !fused && p.nsplit >= 16 && blocks <= 16;
    // M: symmetric-packed for the H3 plans, dense for exact fp32, for a caller's
    // own M, and under PDSC_DENSE_M=1 on the h3 plans other than attention_w64's.
    p.m_layout = w64 || !(f32 || dense_m_caller || k.dense_m) ? M_PACKED : M_DENSE;

    // The V fold goes with the kernels that have its form: the fused plan, or the
    // register-chained chain behind attention_w64 (on zero-padded V') or behind the
    // 4-wave h3 kernel with the in-kernel combine.  (allow_fused = false: the
    // standalone attention, on the caller's 128-channel V.)
    p.vfold = k.vfold && allow_fused && !f32 &&
              (fused || (p.pw2 && !p.precombine &&
                         (p.w64() || (p.kind == ATT_H3 && p.nw == ATT_NW))));
    if (fused) {  // one key split per query block; nsplit stays the split plan's
        p.kind = ATT_FUSED;
        p.nw = PW2_W;
        p.ws = 1;
        p.early = false;
        p.nqb = fg.nqb;
        p.sps = nst;
    }
    if (p.pw2) return p;

    // The LDS-tiled pointwise chain's form.
    // Point-tile size: 64 points (two 32-row MFMA tiles per wave, 2 workgroups per
    // CU) once the launch has >= 2 workgroups per CU, else 32 (twice the
    // workgroups for single pairs and small batches).
    const bool small_tiles = (long)B * (p.Npad / 64) < k.pw_small_limit;
    p.pw_tile = small_tiles ? 32 : 64;
    // 8-wave pw_mid workgroups (32 points each) when the launch has at most one
    // workgroup per CU (a single N = 1000 pair: 32): the chain's output tiles
    // spread over twice the waves.
    p.pw_mid8 = !f32 && k.pw_waves8 && (long)B * (p.Npad / 32) <= 256;
    // Q, K and V in three workgroups per point tile (pcn_qkv8's `only`) while that
    // stays within one workgroup per CU: pw_first on its 32-point tiles, and the
    // 8-wave pw_mid.
    const bool qkv3 = k.pw_qkv_split && 3L * B * (p.Npad / 32) <= 256;
    p.pw_first_qkv3 = !f32 && small_tiles && qkv3;
    p.pw_mid_qkv3 = p.pw_mid8 && qkv3;
    p.pw_prefetch = p.pw_mid8 && k.pw_prefetch;
    return p;
}

// The standalone attention's combine (attention.hip calls it).  It is compiled here, beside the pointwise
// kernels that inline the same combine16: in attention.hip the compiler allocates the kernel's registers
// differently (same resources, another instruction stream), and no kernel's code may move.
template <bool F32>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float *__restrict__ opart,
                                                           const float *__restrict__ ml, int N,
                                                           int Npad, int nsplit,
                                                           float *__restrict__ msg) {
    const int b = blockIdx.y;
    const int row = blockIdx.x * 32 + (threadIdx.x >> 3), d0 = (threadIdx.x & 7) * 16;
    if (row >= N) return;
    float out[16];
    combine16<F32>(opart, ml, b, nsplit, Npad, row, d0, out);
    f32x4 *dst = reinterpret_cast<f32x4 *>(msg + ((size_t)b * N + row) * CH + d0);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = f32x4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
}

hipError_t launch_attn_combine(const float *opart, const float *ml, bool f32, int B, int N, int Npad,
                               int nsplit, float *msg, hipStream_t s) {
    if (f32)
        hipLaunchKernelGGL(attn_combine_kernel<true>, dim3((N + 31) / 32, B), dim3(256), 0, s, opart, ml, N, Npad,
                           nsplit, msg);
    else
        hipLaunchKernelGGL(attn_combine_kernel<false>, dim3((N + 31) / 32, B), dim3(256), 0, s, opart, ml, N, Npad,
                           nsplit, msg);
    return hipGetLastError();
}

// Small batches (many key splits): the split partials combined ahead of the
// pointwise kernel by 32 threads per row (4 channels each), every split's
// loads of a 16-split chunk issued together -- one L2 round trip per chunk
// where combine16 (8 threads per row, 16 channels) needs six for 16 splits --
// and written back as ONE split (m = 0, l = 1) that the pointwise kernel's
// combine16 reads unchanged (w = e^0 = 1, L = 1 l = 1, acc = 1 O, O / 1).  The
// same operations in the same order per channel as combine16: bit-identical.
constexpr int CMB_SB = 16;
__global__ __launch_bounds__(256) void combine_rows_kernel(const float *__restrict__ opart,
                                                           const float *__restrict__ ml, int nsplit, int Npad,
                                                           float *__restrict__ opart1, float *__restrict__ ml1) {
    const int b = blockIdx.y, row = blockIdx.x * 8 + (threadIdx.x >> 5), d0 = 4 * (threadIdx.x & 31);
    if (row >= Npad) return;
    const float *mlb = ml + ((size_t)b * nsplit * Npad + row) * 2;  // split s: mlb[s * Npad * 2 + {0, 1}]
    const size_t oo = h3_opart_off(row, d0);
    float mstar = -INFINITY;
    if (nsplit > CMB_SB) {  // the maxima first when they do not fit one chunk
        for (int s0 = 0; s0 < nsplit; s0 += CMB_SB) {
            float mv[CMB_SB];
#pragma unroll
            for (int j = 0; j < CMB_SB; ++j) mv[j] = s0 + j < nsplit ? mlb[(size_t)(s0 + j) * Npad * 2] : -INFINITY;
#pragma unroll
            for (int j = 0; j < CMB_SB; ++j) mstar = fmaxf(mstar, mv[j]);
        }
    }
    float L = 0.0f;
    f32x4 acc = {};
    for (int s0 = 0; s0 < nsplit; s0 += CMB_SB) {
        f32x2 mlv[CMB_SB];
        f32x4 ov[CMB_SB];
#pragma unroll
        for (int j = 0; j < CMB_SB; ++j) {
            if (s0 + j < nsplit) {
                const size_t base = (size_t)(b * nsplit + s0 + j) * Npad;
                mlv[j] = *reinterpret_cast<const f32x2 *>(ml + (base + row) * 2);
                ov[j] = *reinterpret_cast<const f32x4 *>(opart + base * CH + oo);
            }
        }
        if (nsplit <= CMB_SB) {
#pragma unroll
            for (int j = 0; j < CMB_SB; ++j)
                if (j < nsplit) mstar = fmaxf(mstar, mlv[j][0]);
        }
#pragma unroll
        for (int j = 0; j < CMB_SB; ++j) {
            if (s0 + j < nsplit) {
                const float w = expf(mlv[j][0] - mstar);
                L += w * mlv[j][1];
                acc += w * ov[j];
            }
        }
    }
    const size_t base1 = (size_t)b * Npad;
    *reinterpret_cast<f32x4 *>(opart1 + base1 * CH + oo) = f32x4{acc[0] / L, acc[1] / L, acc[2] / L, acc[3] / L};
    if (d0 == 0) *reinterpret_cast<f32x2 *>(ml1 + (base1 + row) * 2) = f32x2{0.0f, 1.0f};
}

static hipError_t launch_combine_rows(const float *opart, const float *ml, int B, int Npad, int nsplit, float *opart1,
                               float *ml1, hipStream_t s) {
    hipLaunchKernelGGL(combine_rows_kernel, dim3((Npad + 7) / 8, B), dim3(256), 0, s, opart, ml, nsplit, Npad, opart1,
                       ml1);
    return hipGetLastError();
}

// ============================================== pw2: register-chained pointwise chain
// The large-launch form of pw_first / pw_mid / pw_last (H3 precision).  A
// workgroup is PW2_W waves; wave w owns the 32 consecutive points p0 + 32 w ..
// +31 (lane l32 <-> point: one MFMA tile) and carries their whole per-point
// chain in registers.  Dense layers run transposed, Y^T = W X^T (A = weights,
// B = activations): accumulator register r of lane (h, l32) of output tile t is
// channel 32 t + acc_row(r, h) of point l32, and registers 8u .. 8u+7 of tile t
// are exactly the fragment of k-step 2t + u that the next layer's B operand
// takes (inputs in qk_pos order -- the packed weights' order), so layers chain
// with no data movement between lanes.  V runs untransposed (A = activations,
// B = weights) to come out in the attention's V-tile layout.
//
// Weights: the kernel's layers are cut into chunks of <= PW2_CB weight blocks
// (w3_index: one block = 32 outputs x 16 inputs x W_PLANES planes of 1 KiB,
// contiguous per chunk), listed in consumption order by the host (W2Sched).
// Chunks are copied into a 2-slot LDS ring by LDS-DMA and shared by the
// workgroup's waves: right after the barrier that retires chunk c, chunk c + 2
// is queued into the slot c just freed -- before any epilogue work -- so the
// barrier at the end of chunk c + 1 waits only for that DMA (vmcnt counts the
// epilogue's later stores out), and no store is ever waited for.  Per-channel
// epilogue coefficients (bias, BN alpha / beta) sit in LDS for the launch.
// Two workgroups per CU (~55 KiB of LDS and <= 256 VGPRs each) overlap one's
// HBM phases and epilogues with the other's MFMAs.
// (PW2_W waves x 32 = PW2_PTS points per workgroup: attention_plan.hpp, whose fused
// rule depends on them; build knob -DPW2_WAVES.)
// The fused kernels' attention with attention_h3_core's early-issue loop
// (measured, one box: 128 x 1000 forward 3.802 vs 3.831 ms over three A/B
// pairs, attn_pw2 290.3 vs 291.7 us; ragged 4.51 vs 4.58 ms).  A/B build
// -DPW2_EARLY=0: the plain loop.
#ifndef PW2_EARLY
#define PW2_EARLY 1
#endif
constexpr int PW2_OCC = PW2_W >= 8 ? 1 : 2;           // workgroups per CU (<= 256 VGPRs: 2 waves per SIMD)
// 16 two-plane blocks = 32 KiB chunks (r04, A/B: -0.7 % per step at 128 x 1000
// against 8, equal at 8 x 5000 and one pair): half the chunk barriers per chain
#ifndef PW2_CHUNK_BLOCKS
#define PW2_CHUNK_BLOCKS 16
#endif
constexpr int PW2_CB = PW2_CHUNK_BLOCKS;              // blocks per chunk (W_PLANES KiB each)
constexpr int PW2_BLKB = W_PLANES * 1024;             // bytes per block (W_PLANES planes)
constexpr int PW2_SLOT = PW2_CB * PW2_BLKB;
constexpr int PW2_COEF = 1536;                        // floats of epilogue coefficients in LDS
constexpr int PW2_NSLOT = 2;                          // weight-ring slots
constexpr size_t PW2_LDS = PW2_NSLOT * PW2_SLOT + PW2_COEF * sizeof(float);
constexpr int W2_MAXCH = 24;

struct W2Sched {                 // chunk c: np[c] pieces of 1 KiB starting at pk-halfs off[c]
    uint32_t off[W2_MAXCH];
    int32_t np[W2_MAXCH];
    int32_t n;
};

// output tiles per chunk of an IN -> OUT layer
constexpr int w2_nt(int in, int out) {
    return PW2_CB / (in / 16) < 1 ? 1 : (PW2_CB / (in / 16) < out / 32 ? PW2_CB / (in / 16) : out / 32);
}

// Host: append a layer's chunks to the schedule (same cut as w2_layer).
static void w2_sched_add(W2Sched &S, const DenseOff &o, int in, int out) {
    const int nks = in / 16, nt = w2_nt(in, out);
    for (int c = 0; c < out / 32 / nt; ++c) {
        S.off[S.n] = (uint32_t)(2 * o.w + (size_t)c * nt * nks * W3_BLOCK);
        S.np[S.n] = W_PLANES * nt * nks;
        ++S.n;
    }
}

// LDS-DMA of chunk c into `slot` (nothing past the schedule): piece i = 1 KiB =
// one wave instruction, lane-linear on both sides.
PDSC_DEV void w2_stage(const float *pk, const W2Sched &S, int c, char *slot, int wave, int lane) {
    if (c >= S.n) return;
#if ATT_BUFDMA
    // the piece's offset in the SGPR operand: no per-piece address VALU
    const __amdgpu_buffer_rsrc_t r = h3_rsrc(pk, 0xFFFFFFFFu);
    for (int i = wave; i < S.np[c]; i += PW2_W)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)(slot + 1024 * i), 16,
                                                 16 * lane, (int)(2 * S.off[c]) + 1024 * i, 0, 0);
#else
    const _Float16 *src = reinterpret_cast<const _Float16 *>(pk) + S.off[c] + 8 * lane;
    for (int i = wave; i < S.np[c]; i += PW2_W)
        __builtin_amdgcn_global_load_lds(src + 512 * i, slot + 1024 * i, 16, 0, 0);
#endif
}

struct W2Pipe {
    char *base;
    int c;  // chunk being multiplied
    PDSC_DEV char *slot(int k) const { return base + (k % PW2_NSLOT) * PW2_SLOT; }
};

// End of a chunk: this wave's DMA of the next chunk has landed (all but its
// NST youngest vector-memory ops -- the stores issued after that DMA -- are
// done) and its LDS reads have returned, then the barrier.
template <int NST>
PDSC_DEV void w2_sync(bool active) {
    if (NST > 0 && active)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NST) : "memory");
    else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

PDSC_DEV void w2_frag(const char *bp, f16x8 (&w)[3]) {
    w[0] = *reinterpret_cast<const f16x8 *>(bp);
    w[1] = *reinterpret_cast<const f16x8 *>(bp + 1024);
    if constexpr (W_PLANES == 3) w[2] = *reinterpret_cast<const f16x8 *>(bp + 2048);
}

// acc[t0 + t] += W_t X over the chunk's NT tiles x NKS k-steps (TRANS: A = W,
// B = X).  The fragments of block j + 2 are read while block j's MFMAs run (a
// ring of three register sets with compile-time indices); sched_barrier(0)
// pins that order (left alone, the scheduler sinks every read next to its
// MFMA and exposes the LDS latency each time).
template <int NKS, int NT, bool TRANS, int NACC>
PDSC_DEV void w2_mma(const char *slot, const f16x8 *xh, const f16x8 *xl, f32x16 (&acc)[NACC], int t0, int lane) {
    constexpr int NB = NT * NKS;
    const char *bp = slot + 16 * lane;
    f16x8 w[3][3];
    w2_frag(bp, w[0]);
    if (NB > 1) w2_frag(bp + PW2_BLKB, w[1]);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j + 2 < NB) w2_frag(bp + (j + 2) * PW2_BLKB, w[(j + 2) % 3]);
        const int t = j / NKS, ks = j % NKS;
        const f16x8(&f)[3] = w[j % 3];
        const f32x16 c = ks == 0 ? zero16() : acc[t0 + t];  // k-step 0 starts from the inline-constant 0
        acc[t0 + t] = TRANS ? mfma_w3x(f[0], f[1], f[2], xh[ks], xl[ks], c) : mfma_xw3(xh[ks], xl[ks], f[0], f[1], f[2], c);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// One dense layer IN -> OUT.  Per chunk: multiply, sync (NST: the stores the
// caller issued since the previous barrier), queue chunk + 2 into the slot just
// retired.
template <int IN, int OUT, bool TRANS, int NST = 0>
PDSC_DEV void w2_layer(W2Pipe &P, const float *pk, const W2Sched &S, const f16x8 *xh, const f16x8 *xl,
                       f32x16 (&acc)[OUT / 32], bool active, int wave, int lane) {
    constexpr int NKS = IN / 16, NT = w2_nt(IN, OUT), NCH = OUT / 32 / NT;
    static_assert(NCH * NT == OUT / 32, "chunk tiling");
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        CH_STAMP(192 + 3 * min(P.c, 20));  // (diagnostic build: chunk P.c's MFMAs, its sync, tools/att_stamps.py)
        if (active) w2_mma<NKS, NT, TRANS>(P.slot(P.c), xh, xl, acc, c * NT, lane);
        CH_STAMP(193 + 3 * min(P.c, 20));
        if (c == 0)
            w2_sync<NST>(active);
        else
            w2_sync<0>(active);
        CH_STAMP(194 + 3 * min(P.c, 20));
        w2_stage(pk, S, P.c + PW2_NSLOT, P.slot(P.c), wave, lane);
        asm volatile("" ::: "memory");
        ++P.c;
    }
}

// The epilogue coefficients (bias, alpha, beta: 3 * out contiguous floats from
// DenseOff::bias) of one layer into LDS at `dst`.
PDSC_DEV void w2_coef(float *dst, const float *__restrict__ pk, const DenseOff &o, int out, int tid) {
    for (int i = tid; i < 3 * out; i += PW2_W * 64) dst[i] = pk[o.bias + i];
}

// fp32 -> fp16 hi / lo of 8 values
PDSC_DEV void split8v(const float (&v)[8], f16x8 &hi, f16x8 &lo) { split8x(v, hi, lo); }

// Channel of register 8u + e of output tile t for lane half h (transposed layout).
PDSC_DEV int w2_chan(int t, int u, int e, int h) { return 32 * t + 16 * u + 8 * (e >> 2) + 4 * h + (e & 3); }

// Epilogue of a transposed layer: y = epi(acc 2^-s + b) (EPI_BIAS / RELU /
// BN_RELU, as dense_tile_w; EPI_RESID adds resid[t][r]) back into acc, and
// (SPLIT) the hi / lo split of every k-step fragment into xh / xl.  cf = the
// layer's LDS coefficients (bias[out], alpha[out], beta[out]).  SPLIT is a
// compile-time flag: a run-time null test of xh would keep the caller's arrays
// out of registers.
template <int OUT, int EPI, bool SPLIT = true>
PDSC_DEV void w2_epilogue(f32x16 (&acc)[OUT / 32], float inv, const float *cf, const f32x16 *resid, f16x8 *xh,
                          f16x8 *xl, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int t = 0; t < OUT / 32; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c0 = 32 * t + 16 * u + 4 * h;
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(cf + c0), b1 = *reinterpret_cast<const f32x4 *>(cf + c0 + 8);
            f32x4 a0, a1, e0, e1;
            if (EPI == EPI_BN_RELU) {
                a0 = *reinterpret_cast<const f32x4 *>(cf + OUT + c0);
                a1 = *reinterpret_cast<const f32x4 *>(cf + OUT + c0 + 8);
                e0 = *reinterpret_cast<const f32x4 *>(cf + 2 * OUT + c0);
                e1 = *reinterpret_cast<const f32x4 *>(cf + 2 * OUT + c0 + 8);
            }
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int r = 8 * u + e;
                float y = __builtin_fmaf(acc[t][r], inv, e < 4 ? b0[e] : b1[e - 4]);  // exact acc 2^-s, one rounding
                if (EPI == EPI_BN_RELU) y = relu_nan(y * (e < 4 ? a0[e] : a1[e - 4]) + (e < 4 ? e0[e] : e1[e - 4]));
                if (EPI == EPI_RELU) y = relu_nan(y);
                if (EPI == EPI_RESID) y = resid[t][r] + y;  // res = feat + message (:44)
                acc[t][r] = y;
                v[e] = y;
            }
            if constexpr (SPLIT) split8v(v, xh[2 * t + u], xl[2 * t + u]);
        }
}

// Combine the split partials of this lane's point into the k-step fragments of
// the 128 message channels (as combine16: sum_s w_s O_s / sum_s w_s l_s).  The
// partials are in the fragment-block tiling (h3.hpp): k-step ks is
// blocks 2 ks and 2 ks + 1 at this lane, 16 coalesced 1-KiB loads per split.
PDSC_DEV void w2_combine(const float *__restrict__ opart, const float *__restrict__ ml, int b, int nsplit, int Npad,
                         int row, f16x8 *xh, f16x8 *xl, int lane) {
    float mstar = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mstar = fmaxf(mstar, ml[((size_t)(b * nsplit + s) * Npad + row) * 2]);
    float L = 0.0f;
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // (r06: both splits of a pair issued before either is used measured no
    // faster at 8 x 5000, 4.34 vs 4.33 ms per forward: not kept)
    for (int s = 0; s < nsplit; ++s) {
        const size_t base = (size_t)(b * nsplit + s) * Npad + row;
        const float ms = ml[base * 2];
        // an empty split (m = -inf: past a ragged pair's keys, or a stream-K slot past
        // the block's segments, attention_w64.hpp) has w = 0: its O is not read
        // (uniform over the wave's 32 rows, which share one query block)
        if (ms == -INFINITY) continue;
        const float w = expf(ms - mstar);
        L += w * ml[base * 2 + 1];
        const float *src = opart + (base - (row & 31)) * CH + 4 * lane;  // the tile's first block
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += w * *reinterpret_cast<const f32x4 *>(src + 256 * i);
    }
    const float rl = 1.0f / L;  // the softmax denominator once (the reference divides e by its sum first)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = acc[2 * ks][e] * rl;
            v[4 + e] = acc[2 * ks + 1][e] * rl;
        }
        split8v(v, xh[ks], xl[ks]);
    }
}

// VFOLD: w2_combine over the partials' first 64 channels (blocks 0 .. 7 of a
// tile), left as fc0's pre-activation accumulators: block 2 ks + g = registers
// 8 (ks & 1) + 4 g .. +3 of tile ks >> 1 (as attention_h3_kernel stored them).
PDSC_DEV void w2_combine_acc(const float *__restrict__ opart, const float *__restrict__ ml, int b, int nsplit, int Npad,
                             int row, f32x16 (&a)[2], int lane) {
    float mstar = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mstar = fmaxf(mstar, ml[((size_t)(b * nsplit + s) * Npad + row) * 2]);
    float L = 0.0f;
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < nsplit; ++s) {
        const size_t base = (size_t)(b * nsplit + s) * Npad + row;
        const float ms = ml[base * 2];
        if (ms == -INFINITY) continue;  // an empty split (w2_combine)
        const float w = expf(ms - mstar);
        L += w * ml[base * 2 + 1];
        const float *src = opart + (base - (row & 31)) * CH + 4 * lane;  // the tile's first block
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += w * *reinterpret_cast<const f32x4 *>(src + 256 * i);
    }
    const float rl = 1.0f / L;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[i >> 2][4 * (i & 3) + e] = acc[i][e] * rl;
}

// VFOLD: the core's 64-channel O^T -> fc0's pre-activation accumulators (O / l;
// a one-split w2_combine_acc is exactly this)
PDSC_DEV void w2_msg_acc(const f32x16 (&O)[2], float l_run, f32x16 (&a)[2]) {
    const float rl = 1.0f / l_run;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[t][r] = O[t][r] * rl;
}

// The O^T accumulators of the attention core -> the message's k-step fragments
// (msg = O / l; registers 8u .. 8u+7 of tile t = k-step 2t + u).
PDSC_DEV void w2_msg_frags(const f32x16 (&O)[4], float l_run, f16x8 *xh, f16x8 *xl) {
    const float rl = 1.0f / l_run;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = O[ks >> 1][8 * (ks & 1) + e] * rl;
        split8v(v, xh[ks], xl[ks]);
    }
}

// This lane's 64 fp32 values of a 128-channel row.  featL keeps the lane-register
// order of a transposed 128-output layer in the fragment-block tiling of the
// attention partials (per 32-row tile, block 4t + q = registers 4q .. 4q+3 of
// tile t for the 64 lanes): 16 coalesced 1-KiB accesses each way.
PDSC_DEV void w2_load_row(const float *__restrict__ featL, int row, int lane, f32x16 (&y)[4]) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(featL + (size_t)(row >> 5) * (32 * CH)) + lane;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = src[64 * (4 * t + q)];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[t][4 * q + e] = v[e];
        }
}
PDSC_DEV void w2_store_row(float *__restrict__ featL, int row, int lane, const f32x16 (&y)[4]) {
    f32x4 *dst = reinterpret_cast<f32x4 *>(featL + (size_t)(row >> 5) * (32 * CH)) + lane;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[64 * (4 * t + q)] = f32x4{y[t][4 * q], y[t][4 * q + 1], y[t][4 * q + 2], y[t][4 * q + 3]};
}

// Q / K outputs (transposed, bias only) in the attention_h3 fragment-block
// tiling: registers 8u .. 8u+7 of tile t = fragment 2t + u of this lane (qk_pos
// positions 32t + 16u + 8h .. +7 of its point): 16 coalesced 1-KiB stores.
template <bool QSCALE>  // Q: times log2(e)/sqrt(C) (ATT_QFMA: the attention's softmax scale)
PDSC_DEV void w2_store_qk(const f32x16 (&acc)[4], float inv, const float *bias, _Float16 *__restrict__ dst, int row,
                          int lane) {
    const int h = lane >> 5;
    _Float16 *dtile = dst + (size_t)(row >> 5) * H3_TILE_H;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c0 = 32 * t + 16 * u + 4 * h;
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(bias + c0), b1 = *reinterpret_cast<const f32x4 *>(bias + c0 + 8);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] = __builtin_fmaf(acc[t][8 * u + e], inv, e < 4 ? b0[e] : b1[e - 4]);
                if (QSCALE && ATT_QFMA) v[e] *= H3_QSCALE;
            }
            f16x8 hi, lo;
            split8v(v, hi, lo);
            *reinterpret_cast<f16x8 *>(dtile + h3_frag(2 * t + u, 0, lane)) = hi;
            *reinterpret_cast<f16x8 *>(dtile + h3_frag(2 * t + u, 1, lane)) = lo;
        }
}

// V output (untransposed: lane l32 <-> channel 32t + l32, registers 8s .. 8s+7
// <-> the key tile's v_keypos positions 16s + 8h .. +7) = fragment 2t + s of
// this lane in the V tiling, scaled by the tile's 2^vexp (the tile's max |v| is
// wave-local here): 16 coalesced 1-KiB stores.
// NT = 2 (VFOLD): the folded V' = acc 2^-s (its bias went into fc0's), channel
// tiles 0 and 1 of the V tile; pad: channel tiles 2 and 3 written as zeros
// (attention_w64's 128-channel P.V then adds exact zeros to its upper O).
template <int NT>
PDSC_DEV void w2_store_v(f32x16 (&acc)[NT], float inv, const float *bias, _Float16 *__restrict__ Vt,
                         float *__restrict__ vexp_t, int lane, bool pad = false) {
    const int h = lane >> 5, l32 = lane & 31;
    float m = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float bs = NT == 4 ? bias[32 * t + l32] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = __builtin_fmaf(acc[t][r], inv, bs);
            m = fmaxf(m, fabsf(acc[t][r]));
        }
    }
    const int ev = h3_vexp(wave_max(m));
    if (lane == 0) *vexp_t = (float)ev;
    if (NT == 2 && pad) {
        const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 4; i < 8; ++i) {
            *reinterpret_cast<f16x8 *>(Vt + h3_frag(i, 0, lane)) = z;
            *reinterpret_cast<f16x8 *>(Vt + h3_frag(i, 1, lane)) = z;
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = ldexpf(acc[t][8 * s + e], ev);
            f16x8 hi, lo;
            split8v(v, hi, lo);
            *reinterpret_cast<f16x8 *>(Vt + h3_frag(2 * t + s, 0, lane)) = hi;
            *reinterpret_cast<f16x8 *>(Vt + h3_frag(2 * t + s, 1, lane)) = lo;
        }
    }
}

// LDS coefficient table of a PointCN + QKV stage (PW2_COEF floats available).
struct W2CoefQKV {
    static constexpr int pcn = 0, q = 3 * CH, k = 4 * CH, v = 5 * CH, end = 6 * CH;
};
// vfold: d.v is the folded block, whose V' takes no bias (its CH2 coefficients are fc0's)
PDSC_DEV void w2_coef_qkv(float *cf, const float *pk, const PwDense4 &d, int tid, bool vfold) {
    w2_coef(cf + W2CoefQKV::pcn, pk, d.pcn, CH, tid);
    for (int i = tid; i < CH; i += PW2_W * 64) {  // Q / K / V: bias only
        cf[W2CoefQKV::q + i] = pk[d.q.bias + i];
        cf[W2CoefQKV::k + i] = pk[d.k.bias + i];
        if (!vfold) cf[W2CoefQKV::v + i] = pk[d.v.bias + i];
    }
}

// PointCN (BN, ReLU) of the fragments x, then the Q/K/V projections; the
// PointCN rows go to featL.  The pipeline is at the PointCN layer's first chunk.
// VFOLD: d.v is the layer's folded block (LayerOff::vm), V' comes out 64 channels wide.
template <bool VFOLD>
PDSC_DEV void w2_pcn_qkv(W2Pipe &P, const float *__restrict__ pk, const W2Sched &S, const float *cf, const PwDense4 &d,
                         const f16x8 *xh, const f16x8 *xl, float *__restrict__ featL, _Float16 *__restrict__ Q,
                         _Float16 *__restrict__ K, _Float16 *__restrict__ V, float *__restrict__ vexp, int row,
                         bool active, int wave, int lane, bool vpad = false) {
    const int h = lane >> 5;
    f32x16 acc[4];
    f16x8 yh[8], yl[8];
    const float sp = pk[d.pcn.scale], sq = pk[d.q.scale], sk = pk[d.k.scale], sv = pk[d.v.scale];
    w2_layer<CH, CH, true>(P, pk, S, xh, xl, acc, active, wave, lane);
    if (active) {
        w2_epilogue<CH, EPI_BN_RELU>(acc, sp, cf + W2CoefQKV::pcn, nullptr, yh, yl, lane);
        w2_store_row(featL, row, lane, acc);
    }
    CH_STAMP(175);
    w2_layer<CH, CH, true, 16>(P, pk, S, yh, yl, acc, active, wave, lane);
    if (active) w2_store_qk<true>(acc, sq, cf + W2CoefQKV::q, Q, row, lane);
    CH_STAMP(176);
    w2_layer<CH, CH, true, 16>(P, pk, S, yh, yl, acc, active, wave, lane);
    if (active) w2_store_qk<false>(acc, sk, cf + W2CoefQKV::k, K, row, lane);
    CH_STAMP(177);
    if constexpr (VFOLD) {
        f32x16 av[2];
        w2_layer<CH, CH2, false, 16>(P, pk, S, yh, yl, av, active, wave, lane);
        if (active)
            w2_store_v<2>(av, sv, nullptr, V + (size_t)(row >> 5) * H3_TILE_H, vexp + (row >> 5), lane, vpad);
    } else {
        w2_layer<CH, CH, false, 16>(P, pk, S, yh, yl, acc, active, wave, lane);
        if (active)
            w2_store_v<4>(acc, sv, cf + W2CoefQKV::v, V + (size_t)(row >> 5) * H3_TILE_H, vexp + (row >> 5), lane);
    }
    CH_STAMP(178);
}

// Coefficients of combine + fc_message + PointCN + QKV (pw2_mid / attn_pw2).
struct W2CoefMid {
    static constexpr int f0 = W2CoefQKV::end, f3 = f0 + 3 * CH2, f6 = f3 + 3 * CH2, end = f6 + 3 * CH;
};
static_assert(W2CoefMid::end <= PW2_COEF, "coefficient table");
PDSC_DEV void w2_coef_mid(float *cf, const float *__restrict__ pk, const PwMsg &m, const PwDense4 &d, int tid,
                          bool vfold) {
    w2_coef_qkv(cf, pk, d, tid, vfold);
    w2_coef(cf + W2CoefMid::f0, pk, m.fc0, CH2, tid);
    w2_coef(cf + W2CoefMid::f3, pk, m.fc3, CH2, tid);
    w2_coef(cf + W2CoefMid::f6, pk, m.fc6, CH, tid);
}

// fc_message + residual + PointCN + QKV from the message fragments x (after the
// combine); the pipeline is at fc0's first chunk.  featL, Q, K, V, vexp: the pair's.
// VFOLD: a2 holds the folded message (fc0's pre-activation without its bias;
// w2_msg_acc / w2_combine_acc), m.fc0 is the layer's folded block, whose
// coefficients are W0 bv + b0 and fc0's BatchNorm, and the pipeline is at fc3's
// first chunk; x is then scratch.
template <bool VFOLD>
PDSC_DEV void w2_mid_chain(W2Pipe &P, const float *__restrict__ pk, const W2Sched &S, const float *cf, const PwMsg &m,
                           const PwDense4 &d, f16x8 *xh, f16x8 *xl, f32x16 (&a2)[2], const float *featL_in, float *featL,
                           _Float16 *__restrict__ Q, _Float16 *__restrict__ K, _Float16 *__restrict__ V,
                           float *__restrict__ vexp, int row, bool active, int wave, int lane, bool vpad = false) {
    // featL_in: the residual rows; featL: where the PointCN rows go (each lane
    // reads and writes only its own row, so the two may be one buffer)
    f32x16 a4[4], res[4];
    f16x8 yh[8], yl[8];
    if constexpr (VFOLD) {
        if (active) w2_epilogue<CH2, EPI_BN_RELU>(a2, 1.0f, cf + W2CoefMid::f0, nullptr, yh, yl, lane);
    } else {
        w2_layer<CH, CH2, true>(P, pk, S, xh, xl, a2, active, wave, lane);
        if (active) w2_epilogue<CH2, EPI_BN_RELU>(a2, pk[m.fc0.scale], cf + W2CoefMid::f0, nullptr, yh, yl, lane);
    }
    CH_STAMP(172);
    w2_layer<CH2, CH2, true>(P, pk, S, yh, yl, a2, active, wave, lane);
    if (active) {
        w2_epilogue<CH2, EPI_BN_RELU>(a2, pk[m.fc3.scale], cf + W2CoefMid::f3, nullptr, xh, xl, lane);
        w2_load_row(featL_in, row, lane, res);  // the residual: lands during fc6's MFMAs
    }
    CH_STAMP(173);
    w2_layer<CH2, CH, true, 16>(P, pk, S, xh, xl, a4, active, wave, lane);
    if (active) w2_epilogue<CH, EPI_RESID>(a4, pk[m.fc6.scale], cf + W2CoefMid::f6, res, yh, yl, lane);
    CH_STAMP(174);
    w2_pcn_qkv<VFOLD>(P, pk, S, cf, d, yh, yl, featL, Q, K, V, vexp, row, active, wave, lane, vpad);
}

#define PW2_PROLOGUE                                                                              \
    extern __shared__ __attribute__((aligned(16))) char w2smem[];                                 \
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5; \
    const int row = blockIdx.x * PW2_PTS + wave * 32 + (lane & 31);                               \
    const bool active = blockIdx.x * PW2_PTS + wave * 32 < Npad; /* wave-uniform */               \
    const size_t boff = (size_t)b * Npad * CH;                                                    \
    W2Pipe P{w2smem, 0};                                                                          \
    float *cf = reinterpret_cast<float *>(w2smem + PW2_NSLOT * PW2_SLOT);                         \
    for (int c_ = 0; c_ < PW2_NSLOT; ++c_) w2_stage(pk, S, c_, P.slot(c_), wave, lane);

// layer0 (Conv1d in_dim -> 128 on exact fp32 MFMA 32x32x2, k-step j: inputs 2j + h)
// + PointCN_0 + QKV_0.
template <bool VFOLD>
__global__ __launch_bounds__(PW2_W * 64, PW2_OCC) void pw2_first_kernel(const float *__restrict__ pk, W2Sched S, size_t l0w,
                                                                 size_t l0b, PwDense4 d, const float *__restrict__ corr,
                                                                 int in_dim, int N, int Npad, float *__restrict__ featL,
                                                                 _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                                                                 _Float16 *__restrict__ V, float *__restrict__ vexp,
                                                                 const int *__restrict__ nv, int vpad) {
    // ragged batches: a workgroup wholly past its pair's rows has nothing any later
    // kernel reads (the attention's key tiles end at round_up(n, 32) <= its first
    // row; its query blocks past n exit) -- leave before staging any weights
    if (nv && (int)blockIdx.x * PW2_PTS >= nv[blockIdx.y]) return;  // workgroup-uniform
    PW2_PROLOGUE
    const int l32 = lane & 31;
    const int n = nv ? nv[b] : N;  // this pair's rows (ragged batches); N: the row stride
    w2_coef_qkv(cf, pk, d, tid, VFOLD);
    f16x8 xh[8], xl[8];
    if (active) {
        const float *cp = corr + ((size_t)b * N + min(row, n - 1)) * in_dim;
        const bool in = row < n;
        f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
        for (int j = 0; j < (in_dim + 1) / 2; ++j) {
            const int i = 2 * j + h;
            const float x = (in && i < in_dim) ? cp[i] : 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float w = i < in_dim ? pk[l0w + (32 * t + l32) * in_dim + i] : 0.0f;
                acc[t] = mfma32(w, x, acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = acc[t][8 * u + e] + pk[l0b + w2_chan(t, u, e, h)];
                split8v(v, xh[2 * t + u], xl[2 * t + u]);
            }
    }
    __syncthreads();
    w2_pcn_qkv<VFOLD>(P, pk, S, cf, d, xh, xl, featL + boff, Q + 2 * boff, K + 2 * boff, V + 2 * boff,
                      vexp + (size_t)b * (Npad / 32), row, active, wave, lane, vpad != 0);
}

// combine_l + fc_message_l + residual + PointCN_{l+1} + QKV_{l+1}.
// VFOLD: V' padded with zero channels (the attention may be attention_w64's).
template <bool VFOLD>
__global__ __launch_bounds__(PW2_W * 64, PW2_OCC) void pw2_mid_kernel(const float *__restrict__ pk, W2Sched S, PwMsg m,
                                                               PwDense4 d, const float *__restrict__ opart,
                                                               const float *__restrict__ ml, int nsplit, int N,
                                                               int Npad, const float *__restrict__ featL_in,
                                                               float *__restrict__ featL,
                                                               _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                                                               _Float16 *__restrict__ V, float *__restrict__ vexp) {
    PW2_PROLOGUE
    w2_coef_mid(cf, pk, m, d, tid, VFOLD);
    f16x8 xh[8], xl[8];
    f32x16 a2[2];
    if (active) {
        if constexpr (VFOLD)
            w2_combine_acc(opart, ml, b, nsplit, Npad, row, a2, lane);
        else
            w2_combine(opart, ml, b, nsplit, Npad, row, xh, xl, lane);
    }
    __syncthreads();
    w2_mid_chain<VFOLD>(P, pk, S, cf, m, d, xh, xl, a2, featL_in + boff, featL + boff, Q + 2 * boff, K + 2 * boff,
                        V + 2 * boff, vexp + (size_t)b * (Npad / 32), row, active, wave, lane, true);
}

// attention_l + fc_message_l + residual + PointCN_{l+1} + QKV_{l+1} in ONE
// launch (one key split: the workgroup's 128 queries are the 128 points of its
// chain): the O^T accumulators the attention core leaves in registers are the
// message's k-step fragments, so the partials never touch HBM, and workgroups
// in their attention phase overlap others' store-heavy chain phase.  Reads the
// layer-l Q/K/V (Qs, Ks, Vs, vexp_in) and writes the layer-(l+1) ones to other
// buffers (Q, K, V, vexp): other workgroups of the pair still read layer l.
// Bit-identical to attention_h3_kernel + pw2_mid_kernel (a one-split combine
// is O * (1 / l) exactly).  LDS: the K/V ring, then the weight ring.
template <bool PACKED, bool VFOLD>
__global__ __launch_bounds__(PW2_W * 64, PW2_OCC) void attn_pw2_kernel(
    const _Float16 *__restrict__ Qs, const _Float16 *__restrict__ Ks, const _Float16 *__restrict__ Vs,
    const float *__restrict__ vexp_in, const float *__restrict__ M, AttnGridH3 g, const float *__restrict__ pk,
    W2Sched S, PwMsg m, PwDense4 d, float *__restrict__ featL, _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
    _Float16 *__restrict__ V, float *__restrict__ vexp) {
    extern __shared__ __attribute__((aligned(16))) char w2smem[];
    const AttnBlock blk = attention_h3_block(g, true);
    if (blk.qb * PW2_PTS >= g.n(blk.b)) return;  // past a ragged pair's end (workgroup-uniform)
    const int b = blk.b, Npad = g.Npad, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6),
              lane = tid & 63;
    const int row = blk.qb * PW2_PTS + wave * 32 + (lane & 31);
    const bool active = blk.qb * PW2_PTS + wave * 32 < Npad;  // wave-uniform
    const size_t boff = (size_t)b * Npad * CH;
#ifdef ATT_STAMPS
    unsigned long long *stp = att_stamp_ptr(wave);
    ATT_RSTAMP(stp, 188);
    ATT_STAMP(stp, 0);
#endif
    constexpr int CV = VFOLD ? CH2 : CH;
    f32x16 O[CV / 32];
    float m_run, l_run;
    attention_h3_core<PW2_W, PACKED, PW2_EARLY, 0, CV>(Qs, Ks, Vs, vexp_in, M, g, blk, w2smem, wave, lane, O, m_run,
                                                       l_run);
    ATT_STAMP(stp, 170);
    // the K/V ring is free (the core ends on a barrier): weight chunks 0, 1 and the coefficients
    W2Pipe P{w2smem, 0};
    float *cf = reinterpret_cast<float *>(w2smem + PW2_NSLOT * PW2_SLOT);
    for (int c = 0; c < PW2_NSLOT; ++c) w2_stage(pk, S, c, P.slot(c), wave, lane);
    w2_coef_mid(cf, pk, m, d, tid, VFOLD);
    f16x8 xh[8], xl[8];
    f32x16 a2[2];
    if (active) {  // msg = O / l
        if constexpr (VFOLD)
            w2_msg_acc(O, l_run, a2);
        else
            w2_msg_frags(O, l_run, xh, xl);
    }
    __syncthreads();
    ATT_STAMP(stp, 171);
    w2_mid_chain<VFOLD>(P, pk, S, cf, m, d, xh, xl, a2, featL + boff, featL + boff, Q + 2 * boff, K + 2 * boff,
                        V + 2 * boff, vexp + (size_t)b * (Npad / 32), row, active, wave, lane);
    ATT_STAMP(stp, 180);
    ATT_RSTAMP(stp, 189);
}

#ifdef ATT_STAMPS
extern "C" int pdsc_diag_att_stamps(void *host, size_t bytes) {
    const size_t n = std::min(bytes, sizeof(g_att_stamps));
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_att_stamps), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int pdsc_diag_att_stamps_clear() {
    static unsigned long long zero[ST_WGS * 4 * ST_PER_WAVE];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_att_stamps), zero, sizeof(zero), 0, hipMemcpyHostToDevice) == hipSuccess ? 0
                                                                                                             : -1;
}
#endif

// Coefficients of the last layer's fc_message + classifier (pw2_last / attn_pw2_last).
struct W2CoefLast {
    static constexpr int f0 = 0, f3 = f0 + 3 * CH2, f6 = f3 + 3 * CH2, c0 = f6 + 3 * CH, c2 = c0 + 3 * CLS,
                         c4 = c2 + 3 * CLS, end = c4 + CLS;
};
static_assert(W2CoefLast::end <= PW2_COEF, "coefficient table");
PDSC_DEV void w2_coef_last(float *cf, const float *__restrict__ pk, const PwMsg &m, const DenseOff &c0,
                           const DenseOff &c2, size_t c4w, int tid) {
    w2_coef(cf + W2CoefLast::f0, pk, m.fc0, CH2, tid);
    w2_coef(cf + W2CoefLast::f3, pk, m.fc3, CH2, tid);
    w2_coef(cf + W2CoefLast::f6, pk, m.fc6, CH, tid);
    w2_coef(cf + W2CoefLast::c0, pk, c0, CLS, tid);
    w2_coef(cf + W2CoefLast::c2, pk, c2, CLS, tid);
    for (int i = tid; i < CLS; i += PW2_W * 64) cf[W2CoefLast::c4 + i] = pk[c4w + i];
}

// fc_message + residual from the message fragments x, then F.normalize (:156)
// and the classifier (:171); the pipeline is at fc0's first chunk.  featL: the pair's.
// VFOLD: as w2_mid_chain's.
template <bool VFOLD>
PDSC_DEV void w2_last_chain(W2Pipe &P, const float *__restrict__ pk, const W2Sched &S, const float *cf, const PwMsg &m,
                            const DenseOff &c0, const DenseOff &c2, size_t c4b, f16x8 *xh, f16x8 *xl, f32x16 (&a2)[2],
                            const float *__restrict__ featL, float *__restrict__ feat_out, float *__restrict__ normed,
                            _Float16 *__restrict__ normed_s, float *__restrict__ conf, int b, int N, int row,
                            bool active, int wave, int lane) {
    constexpr int CF0 = W2CoefLast::f0, CF3 = W2CoefLast::f3, CF6 = W2CoefLast::f6, CC0 = W2CoefLast::c0,
                  CC2 = W2CoefLast::c2, CC4 = W2CoefLast::c4;
    const int h = lane >> 5;
    f32x16 a1[1], a4[4], res[4];
    f16x8 yh[8], yl[8];
    if constexpr (VFOLD) {
        if (active) w2_epilogue<CH2, EPI_BN_RELU>(a2, 1.0f, cf + CF0, nullptr, yh, yl, lane);
    } else {
        w2_layer<CH, CH2, true>(P, pk, S, xh, xl, a2, active, wave, lane);
        if (active) w2_epilogue<CH2, EPI_BN_RELU>(a2, pk[m.fc0.scale], cf + CF0, nullptr, yh, yl, lane);
    }
    w2_layer<CH2, CH2, true>(P, pk, S, yh, yl, a2, active, wave, lane);
    if (active) {
        w2_epilogue<CH2, EPI_BN_RELU>(a2, pk[m.fc3.scale], cf + CF3, nullptr, xh, xl, lane);
        w2_load_row(featL, row, lane, res);
    }
    w2_layer<CH2, CH, true, 16>(P, pk, S, xh, xl, a4, active, wave, lane);
    const bool in = row < N;
    if (active) {
        w2_epilogue<CH, EPI_RESID>(a4, pk[m.fc6.scale], cf + CF6, res, yh, yl, lane);  // a4 = corr_features (:155)
        float ss = 0.0f;  // F.normalize(p=2, dim=-1, eps=1e-12) (:156)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) ss = __builtin_fmaf(a4[t][r], a4[t][r], ss);
        ss = halves_sum(ss);
        const float den = fmaxf(sqrtf(ss), 1e-12f);
        if (in) {
            float *dst = normed + ((size_t)b * N + row) * CH;
            _Float16 *ds = normed_s ? normed_s + ((size_t)b * N + row) * 2 * CH : nullptr;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = a4[t][8 * u + e] / den;
                    *reinterpret_cast<f32x4 *>(dst + 32 * t + 16 * u + 4 * h) = f32x4{v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4 *>(dst + 32 * t + 16 * u + 8 + 4 * h) = f32x4{v[4], v[5], v[6], v[7]};
                    if (ds) {  // the fp16 hi/lo split copy (qk_pos order) the seed kNN consumes
                        f16x8 hi, lo;
                        split8v(v, hi, lo);
                        const int chk = 4 * t + 2 * u + h;
                        *reinterpret_cast<f16x8 *>(ds + 8 * chk) = hi;
                        *reinterpret_cast<f16x8 *>(ds + CH + 8 * chk) = lo;
                    }
                }
            if (feat_out) {  // natural channel order (the standalone encoder API only)
                float *fo = feat_out + ((size_t)b * N + row) * CH;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<f32x4 *>(fo + 32 * t + 8 * g + 4 * h) =
                            f32x4{a4[t][4 * g], a4[t][4 * g + 1], a4[t][4 * g + 2], a4[t][4 * g + 3]};
            }
        }
    }
    // classification MLP 128 -> 32 -> 32 -> 1 on the unnormalised features (:171)
    w2_layer<CH, CLS, true>(P, pk, S, yh, yl, a1, active, wave, lane);
    if (active) w2_epilogue<CLS, EPI_RELU>(a1, pk[c0.scale], cf + CC0, nullptr, xh, xl, lane);
    w2_layer<CLS, CLS, true>(P, pk, S, xh, xl, a1, active, wave, lane);
    if (active) {
        w2_epilogue<CLS, EPI_RELU, false>(a1, pk[c2.scale], cf + CC2, nullptr, nullptr, nullptr, lane);
        float s = 0.0f;  // this half's 16 channels, then the other half's
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) s = __builtin_fmaf(cf[CC4 + w2_chan(0, u, e, h)], a1[0][8 * u + e], s);
        s = halves_sum(s);
        if (in && h == 0) conf[(size_t)b * N + row] = s + pk[c4b];
    }
}

// combine + fc_message + residual, then F.normalize (:156) and the classifier (:171).
template <bool VFOLD>
__global__ __launch_bounds__(PW2_W * 64, PW2_OCC) void pw2_last_kernel(
    const float *__restrict__ pk, W2Sched S, PwMsg m, DenseOff c0, DenseOff c2, size_t c4w, size_t c4b,
    const float *__restrict__ opart, const float *__restrict__ ml, int nsplit, int N, int Npad,
    const float *__restrict__ featL, float *__restrict__ feat_out, float *__restrict__ normed,
    _Float16 *__restrict__ normed_s, float *__restrict__ conf) {
    PW2_PROLOGUE
    w2_coef_last(cf, pk, m, c0, c2, c4w, tid);
    f16x8 xh[8], xl[8];
    f32x16 a2[2];
    if (active) {
        if constexpr (VFOLD)
            w2_combine_acc(opart, ml, b, nsplit, Npad, row, a2, lane);
        else
            w2_combine(opart, ml, b, nsplit, Npad, row, xh, xl, lane);
    }
    __syncthreads();
    w2_last_chain<VFOLD>(P, pk, S, cf, m, c0, c2, c4b, xh, xl, a2, featL + boff, feat_out, normed, normed_s, conf, b, N,
                         row, active, wave, lane);
}

// attention_{L-1} + fc_message_{L-1} + residual + normalize + classifier in ONE
// launch (as attn_pw2_kernel for the last layer): bit-identical to
// attention_h3_kernel + pw2_last_kernel with one key split.
template <bool PACKED, bool VFOLD>
__global__ __launch_bounds__(PW2_W * 64, PW2_OCC) void attn_pw2_last_kernel(
    const _Float16 *__restrict__ Qs, const _Float16 *__restrict__ Ks, const _Float16 *__restrict__ Vs,
    const float *__restrict__ vexp_in, const float *__restrict__ M, AttnGridH3 g, const float *__restrict__ pk,
    W2Sched S, PwMsg m, DenseOff c0, DenseOff c2, size_t c4w, size_t c4b, const float *__restrict__ featL,
    float *__restrict__ feat_out, float *__restrict__ normed, _Float16 *__restrict__ normed_s,
    float *__restrict__ conf) {
    extern __shared__ __attribute__((aligned(16))) char w2smem[];
    const AttnBlock blk = attention_h3_block(g, true);
    if (blk.qb * PW2_PTS >= g.n(blk.b)) return;  // past a ragged pair's end (workgroup-uniform)
    const int b = blk.b, N = g.N, Npad = g.Npad, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6),
              lane = tid & 63;
    const int row = blk.qb * PW2_PTS + wave * 32 + (lane & 31);
    const bool active = blk.qb * PW2_PTS + wave * 32 < Npad;  // wave-uniform
    constexpr int CV = VFOLD ? CH2 : CH;
    f32x16 O[CV / 32];
    float m_run, l_run;
    attention_h3_core<PW2_W, PACKED, PW2_EARLY, 0, CV>(Qs, Ks, Vs, vexp_in, M, g, blk, w2smem, wave, lane, O, m_run,
                                                       l_run);
    W2Pipe P{w2smem, 0};
    float *cf = reinterpret_cast<float *>(w2smem + PW2_NSLOT * PW2_SLOT);
    for (int c = 0; c < PW2_NSLOT; ++c) w2_stage(pk, S, c, P.slot(c), wave, lane);
    w2_coef_last(cf, pk, m, c0, c2, c4w, tid);
    f16x8 xh[8], xl[8];
    f32x16 a2[2];
    if (active) {
        if constexpr (VFOLD)
            w2_msg_acc(O, l_run, a2);
        else
            w2_msg_frags(O, l_run, xh, xl);
    }
    __syncthreads();
    w2_last_chain<VFOLD>(P, pk, S, cf, m, c0, c2, c4b, xh, xl, a2, featL + (size_t)b * Npad * CH, feat_out, normed,
                         normed_s, conf, b, N, row, active, wave, lane);
}
#undef PW2_PROLOGUE

// vfold: d.v and m.fc0 are the layer's folded block (dense4 / msg3): V' is 128 -> 64,
// and fc0's product is gone from the message chain.
static W2Sched sched_qkv(W2Sched S, const PwDense4 &d, bool vfold) {
    w2_sched_add(S, d.pcn, CH, CH);
    w2_sched_add(S, d.q, CH, CH);
    w2_sched_add(S, d.k, CH, CH);
    w2_sched_add(S, d.v, CH, vfold ? CH2 : CH);
    return S;
}
static W2Sched sched_msg(const PwMsg &m, bool vfold) {
    W2Sched S{};
    if (!vfold) w2_sched_add(S, m.fc0, CH, CH2);
    w2_sched_add(S, m.fc3, CH2, CH2);
    w2_sched_add(S, m.fc6, CH2, CH);
    return S;
}

static PwDense4 dense4(const LayerOff &l, bool vfold = false) { return PwDense4{l.pcn, l.q, l.k, vfold ? l.vm : l.v}; }
static PwMsg msg3(const LayerOff &l, bool vfold = false) { return PwMsg{vfold ? l.vm : l.fc0, l.fc3, l.fc6}; }

// The fused launches (the plan's ATT_FUSED): one key split per query block, a
// workgroup per PW2_PTS queries.
static hipError_t launch_attn_pw2(const EncoderPlan &plan, const float *packed, const PackLayout &lay, int layer,
                           const void *q, const void *k, const void *v, const float *vexp_in, const float *M,
                           float *feat, void *qo, void *ko, void *vo, float *vexp_out, hipStream_t s, Ragged rg) {
    if (!plan.fused() || layer + 1 >= lay.L) return hipErrorInvalidValue;
    const AttnGridH3 g = plan_grid_h3(plan, rg, layer);
    const bool vf = plan.vfold;
    const PwMsg m = msg3(lay.layer[layer], vf);
    const PwDense4 d = dense4(lay.layer[layer + 1], vf);
    const W2Sched S = sched_qkv(sched_msg(m, vf), d, vf);
    const size_t lds = std::max(attention_h3_lds_bytes<PW2_W>(), PW2_LDS);
    const _Float16 *qs = static_cast<const _Float16 *>(q), *ks = static_cast<const _Float16 *>(k),
                   *vs = static_cast<const _Float16 *>(v);
    _Float16 *Q = static_cast<_Float16 *>(qo), *K = static_cast<_Float16 *>(ko), *V = static_cast<_Float16 *>(vo);
    with_bool(plan.m_layout == M_PACKED, [&](auto pk) {
        with_bool(vf, [&](auto vfold) {
            hipLaunchKernelGGL((attn_pw2_kernel<decltype(pk)::value, decltype(vfold)::value>), dim3(plan.workgroups()),
                               dim3(PW2_W * 64), lds, s, qs, ks, vs, vexp_in, M, g, packed, S, m, d, feat, Q, K, V,
                               vexp_out);
        });
    });
    return hipGetLastError();
}

static hipError_t launch_attn_pw2_last(const EncoderPlan &plan, const float *packed, const PackLayout &lay, const void *q,
                                const void *k, const void *v, const float *vexp_in, const float *M, const float *feat,
                                float *feat_out, float *normed, _Float16 *normed_s, float *conf, hipStream_t s,
                                Ragged rg) {
    if (!plan.fused()) return hipErrorInvalidValue;
    const AttnGridH3 g = plan_grid_h3(plan, rg, lay.L - 1);
    const bool vf = plan.vfold;
    const PwMsg m = msg3(lay.layer[lay.L - 1], vf);
    W2Sched S = sched_msg(m, vf);
    w2_sched_add(S, lay.c0, CH, CLS);
    w2_sched_add(S, lay.c2, CLS, CLS);
    const size_t lds = std::max(attention_h3_lds_bytes<PW2_W>(), PW2_LDS);
    const _Float16 *qs = static_cast<const _Float16 *>(q), *ks = static_cast<const _Float16 *>(k),
                   *vs = static_cast<const _Float16 *>(v);
    with_bool(plan.m_layout == M_PACKED, [&](auto pk) {
        with_bool(vf, [&](auto vfold) {
            hipLaunchKernelGGL((attn_pw2_last_kernel<decltype(pk)::value, decltype(vfold)::value>),
                               dim3(plan.workgroups()), dim3(PW2_W * 64), lds, s, qs, ks, vs, vexp_in, M, g, packed, S, m,
                               lay.c0, lay.c2, lay.c4_w, lay.c4_b, feat, feat_out, normed, normed_s, conf);
        });
    });
    return hipGetLastError();
}

// One launch of pointwise kernel K<PTT, F32> with the plan's PTT and F32.
#define PW_LAUNCH(K, rows, ...)                                                                         \
    do {                                                                                                \
        const bool st_ = plan.pw_tile == 32;                                                            \
        const dim3 g_(((rows) + plan.pw_tile - 1) / plan.pw_tile, plan.B);                              \
        if (st_ && plan.f32)                                                                            \
            hipLaunchKernelGGL((K<32, true>), g_, dim3(256), pw_lds<32>(), s, __VA_ARGS__);             \
        else if (st_)                                                                                   \
            hipLaunchKernelGGL((K<32, false>), g_, dim3(256), pw_lds<32>(), s, __VA_ARGS__);            \
        else if (plan.f32)                                                                              \
            hipLaunchKernelGGL((K<64, true>), g_, dim3(256), pw_lds<64>(), s, __VA_ARGS__);             \
        else                                                                                            \
            hipLaunchKernelGGL((K<64, false>), g_, dim3(256), pw_lds<64>(), s, __VA_ARGS__);            \
    } while (0)

static hipError_t launch_pw_first(const EncoderPlan &plan, const float *packed, const PackLayout &lay, const float *corr_pos,
                           float *feat, void *q, void *k, void *v, float *vexp, hipStream_t s, Ragged rg) {
    if (lay.in_dim > IN_LIMIT) return hipErrorInvalidValue;
    const int B = plan.B, N = plan.N, Npad = plan.Npad;
    _Float16 *Q = static_cast<_Float16 *>(q), *K = static_cast<_Float16 *>(k), *V = static_cast<_Float16 *>(v);
    if (plan.pw2) {  // the fused plan's layouts
        const PwDense4 d = dense4(lay.layer[0], plan.vfold);
        const W2Sched S = sched_qkv(W2Sched{}, d, plan.vfold);
        with_bool(plan.vfold, [&](auto vf) {
            hipLaunchKernelGGL(pw2_first_kernel<decltype(vf)::value>, dim3((Npad + PW2_PTS - 1) / PW2_PTS, B),
                               dim3(PW2_W * 64), PW2_LDS, s, packed, S, lay.l0_w, lay.l0_b, d, corr_pos, lay.in_dim, N,
                               Npad, feat, Q, K, V, vexp, rg.nv, (int)!plan.fused());
        });
        return hipGetLastError();
    }
    if (plan.pw_first_qkv3) {  // Q / K / V in three workgroups per tile
        hipLaunchKernelGGL((pw_first_kernel<32, false>), dim3(Npad / 32, B, 3), dim3(256), pw_lds<32>(), s, packed,
                           lay.l0_w, lay.l0_b, dense4(lay.layer[0]), corr_pos, lay.in_dim, N, Npad, feat, Q, K, V, vexp,
                           rg.nv);
        return hipGetLastError();
    }
    PW_LAUNCH(pw_first_kernel, Npad, packed, lay.l0_w, lay.l0_b, dense4(lay.layer[0]), corr_pos, lay.in_dim, N, Npad,
              feat, Q, K, V, vexp, rg.nv);
    return hipGetLastError();
}

static hipError_t launch_pw_mid(const EncoderPlan &plan, const float *packed, const PackLayout &lay, int layer,
                         const float *opart, const float *ml, int nsplit, const float *feat_in, float *feat, void *q,
                         void *k, void *v, float *vexp, hipStream_t s) {
    const int delay = g_diag_qkv_delay;  // tests only (pdsc_diag_qkv_delay): delay the split's K / V workgroups
    const int B = plan.B, N = plan.N, Npad = plan.Npad;
    _Float16 *Q = static_cast<_Float16 *>(q), *K = static_cast<_Float16 *>(k), *V = static_cast<_Float16 *>(v);
    if (plan.pw2) {
        const PwMsg m = msg3(lay.layer[layer], plan.vfold);
        const PwDense4 d = dense4(lay.layer[layer + 1], plan.vfold);
        const W2Sched S = sched_qkv(sched_msg(m, plan.vfold), d, plan.vfold);
        with_bool(plan.vfold, [&](auto vf) {
            hipLaunchKernelGGL(pw2_mid_kernel<decltype(vf)::value>, dim3((Npad + PW2_PTS - 1) / PW2_PTS, B),
                               dim3(PW2_W * 64), PW2_LDS, s, packed, S, m, d, opart, ml, nsplit, N, Npad, feat_in, feat, Q,
                               K, V, vexp);
        });
        return hipGetLastError();
    }
    if (plan.pw_mid8) {
        hipLaunchKernelGGL((pw_mid_kernel<32, false, 8>), dim3(Npad / 32, B, plan.pw_mid_qkv3 ? 3 : 1), dim3(512),
                           pw_lds<32>(), s, packed,
                           msg3(lay.layer[layer]), dense4(lay.layer[layer + 1]), opart, ml, nsplit, N, Npad, feat_in,
                           feat, Q, K, V, vexp, delay, (int)plan.pw_prefetch);
        return hipGetLastError();
    }
    PW_LAUNCH(pw_mid_kernel, Npad, packed, msg3(lay.layer[layer]), dense4(lay.layer[layer + 1]), opart, ml, nsplit,
              N, Npad, feat_in, feat, Q, K, V, vexp, 0, 0);
    return hipGetLastError();
}

static hipError_t launch_pw_last(const EncoderPlan &plan, const float *packed, const PackLayout &lay, const float *opart,
                          const float *ml, int nsplit, const float *feat, float *feat_out, float *normed,
                          _Float16 *normed_s, float *conf, hipStream_t s) {
    const int B = plan.B, N = plan.N, Npad = plan.Npad;
    if (plan.pw2) {
        const PwMsg m = msg3(lay.layer[lay.L - 1], plan.vfold);
        W2Sched S = sched_msg(m, plan.vfold);
        w2_sched_add(S, lay.c0, CH, CLS);
        w2_sched_add(S, lay.c2, CLS, CLS);
        with_bool(plan.vfold, [&](auto vf) {
            hipLaunchKernelGGL(pw2_last_kernel<decltype(vf)::value>, dim3((Npad + PW2_PTS - 1) / PW2_PTS, B),
                               dim3(PW2_W * 64), PW2_LDS, s, packed, S, m, lay.c0, lay.c2, lay.c4_w, lay.c4_b, opart, ml,
                               nsplit, N, Npad, feat, feat_out, normed, normed_s, conf);
        });
        return hipGetLastError();
    }
    PW_LAUNCH(pw_last_kernel, N, packed, msg3(lay.layer[lay.L - 1]), lay.c0, lay.c2, lay.c4_w, lay.c4_b, opart, ml,
              nsplit, N, Npad, feat, feat_out, normed, normed_s, conf);
    return hipGetLastError();
}
#undef PW_LAUNCH

// ================================================ the row's workspace and run loop
// measurement hook (pdsc_attention_timing): events recorded around attention launches
static thread_local hipEvent_t *g_tstart = nullptr, *g_tstop = nullptr;
static thread_local int g_tcap = 0;
static thread_local int32_t *g_tcount = nullptr;

EncBufs carve_encoder(Carve &c, const EncoderPlan &plan) {
    EncBufs e;
    const size_t B = plan.B, Npad = plan.Npad, rows = B * Npad * CH;
    e.feat = c.take<float>(rows);
    e.q = c.take<_Float16>(2 * rows);
    e.k = c.take<_Float16>(2 * rows);
    e.v = c.take<_Float16>(2 * rows);
    e.opart = c.take<float>(rows * plan.nsplit);
    e.ml = c.take<float>(B * Npad * plan.nsplit * 2);
    e.vexp = c.take<float>(B * (Npad / 32));
    e.opart1 = plan.precombine ? c.take<float>(rows) : nullptr;
    e.ml1 = plan.precombine ? c.take<float>(B * Npad * 2) : nullptr;
    e.q2 = e.k2 = e.v2 = nullptr;
    e.vexp2 = nullptr;
    // pw_mid's three Q / K / V workgroups per point tile all read the layer's
    // residual rows while one of them writes the new PointCN rows: the rows
    // ping-pong between feat and feat2 so no workgroup overwrites what another
    // still reads
    e.feat2 = plan.fused() ? nullptr : c.take<float>(rows);
    if (plan.fused()) {
        e.q2 = c.take<_Float16>(2 * rows);
        e.k2 = c.take<_Float16>(2 * rows);
        e.v2 = c.take<_Float16>(2 * rows);
        e.vexp2 = c.take<float>(B * (Npad / 32));
    }
    return e;
}

// M: in the plan's layout (batch.m_layout)
static int run_encoder(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                       const EncoderPlan &batch, const EncBufs &e, float *feat_out, float *normed, _Float16 *normed_s,
                       float *conf, hipStream_t s, Ragged rg = {}) {
    const EncoderPlan plan = batch.for_ragged(rg);
    HIPCHK(launch_pw_first(plan, packed, lay, corr_pos, e.feat, e.q, e.k, e.v, e.vexp, s, rg));
    if (plan.fused()) {  // every layer fused (0 .. L-2 with the next layer's PointCN/QKV, Q/K/V alternating between the two sets)
        _Float16 *q = e.q, *k = e.k, *v = e.v, *q2 = e.q2, *k2 = e.k2, *v2 = e.v2;
        float *vx = e.vexp, *vx2 = e.vexp2;
        for (int l = 0; l + 1 < lay.L; ++l) {
            const bool timed = g_tcap > 0 && g_tcount && *g_tcount < g_tcap;
            if (timed) HIPCHK(hipEventRecord(g_tstart[*g_tcount], s));
            HIPCHK(launch_attn_pw2(plan, packed, lay, l, q, k, v, vx, M, e.feat, q2, k2, v2, vx2, s, rg));
            if (timed) HIPCHK(hipEventRecord(g_tstop[(*g_tcount)++], s));
            std::swap(q, q2);
            std::swap(k, k2);
            std::swap(v, v2);
            std::swap(vx, vx2);
        }
        HIPCHK(launch_attn_pw2_last(plan, packed, lay, q, k, v, vx, M, e.feat, feat_out, normed, normed_s, conf, s, rg));
        return PDSC_OK;
    }
    float *feat = e.feat, *feat_alt = e.feat2;
    for (int l = 0; l < lay.L; ++l) {
        const bool timed = g_tcap > 0 && g_tcount && *g_tcount < g_tcap;
        if (timed) HIPCHK(hipEventRecord(g_tstart[*g_tcount], s));
        HIPCHK(launch_attention(plan, e.q, e.k, e.v, e.vexp, M, e.opart, e.ml, s, rg, l));
        if (timed) HIPCHK(hipEventRecord(g_tstop[(*g_tcount)++], s));
        const float *op = e.opart, *mlp = e.ml;
        int ns = plan.nsplit;
        if (plan.precombine) {
            HIPCHK(launch_combine_rows(e.opart, e.ml, plan.B, plan.Npad, plan.nsplit, e.opart1, e.ml1, s));
            op = e.opart1;
            mlp = e.ml1;
            ns = 1;
        }
        if (l + 1 < lay.L) {
            HIPCHK(launch_pw_mid(plan, packed, lay, l, op, mlp, ns, feat, feat_alt, e.q, e.k, e.v, e.vexp, s));
            std::swap(feat, feat_alt);
        } else {
            HIPCHK(launch_pw_last(plan, packed, lay, op, mlp, ns, feat, feat_out, normed, plan.f32 ? nullptr : normed_s,
                                  conf, s));
        }
    }
    return PDSC_OK;
}

// Ragged batches run the fused encoder as P parts of the batch (contiguous pair
// ranges of equal pair counts), each on its own
// stream -- the caller's and P - 1 per-device side streams, forked and joined
// by events -- so one part's launches fill the others' dispatch tails: a ragged
// batch's attention launches end in a tail of a few long workgroups per XCD
// (DESIGN.md §7).  Pairs are independent through the encoder, so each part is
// the same arithmetic on its own pointer range (bitwise equal results).
// 128 pairs, N in [700, 1300], two halves: 4.54 -> 4.12 ms per forward (three
// parts 4.23, four 4.32 vs two 4.19 on another box); uniform batches (two full
// rounds of workgroups, no tail to fill) measured 3.77 -> 3.83 ms, so they stay
// on one stream.  Knobs: PDSC_ENC_HALVES 0 never, 1 uniform batches too;
// PDSC_ENC_PARTS P in [2, 4] (default 2).  Every part keeps the whole batch's
// plan (the fused launches' one key split, pw2_first's layouts).
bool enc_halves(const EncoderPlan &plan, bool ragged) {
    const Knobs &k = knobs();
    return plan.fused() && plan.B >= 16 * k.enc_parts && (k.enc_halves == 1 || (k.enc_halves != 0 && ragged));
}
// Part boundaries bounds[0 .. P]: bounds[i] = the first pair whose work prefix
// reaches i/P of the total (counts: HOST sizes, or NULL for a uniform batch).
void enc_bounds(const int32_t *counts, int B, int P, int *bounds) {
    std::vector<double> pre(B + 1, 0.0);
    for (int b = 0; b < B; ++b) pre[b + 1] = pre[b] + (counts ? (double)counts[b] * counts[b] : 1.0);
    bounds[0] = 0;
    bounds[P] = B;
    for (int i = 1; i < P; ++i) {
        const double goal = pre[B] * i / P;
        int h = bounds[i - 1] + 1;
        while (h < B - (P - i) && std::abs(pre[h + 1] - goal) < std::abs(pre[h] - goal)) ++h;
        bounds[i] = h;
    }
}

struct SideStream {
    std::mutex mu;  // one fork / join enqueued at a time per device
    hipStream_t s2[ENC_MAX_PARTS - 1] = {};
    hipEvent_t fork = nullptr, join[ENC_MAX_PARTS - 1] = {};
    bool ok = false;
};
// The side streams of the device that stream s runs on (the current device for
// the legacy default stream), created there on first use.
SideStream *side_stream(hipStream_t s) {
    static SideStream ss[64];
    hipDevice_t dev = 0;
    if (!s || hipStreamGetDevice(s, &dev) != hipSuccess)
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (dev < 0 || dev >= 64) return nullptr;
    SideStream &x = ss[dev];
    static std::mutex create_mu;
    std::lock_guard<std::mutex> lock(create_mu);
    if (!x.ok) {  // all or none (a failure leaves the forward on one stream)
        int cur = dev;
        if (hipGetDevice(&cur) != hipSuccess || (cur != dev && hipSetDevice(dev) != hipSuccess)) return nullptr;
        bool ok = x.fork || hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < ENC_MAX_PARTS - 1; ++i) {
            if (!x.s2[i]) ok = hipStreamCreateWithFlags(&x.s2[i], hipStreamNonBlocking) == hipSuccess;
            if (ok && !x.join[i]) ok = hipEventCreateWithFlags(&x.join[i], hipEventDisableTiming) == hipSuccess;
        }
        if (cur != dev) (void)hipSetDevice(cur);
        x.ok = ok;
    }
    return x.ok ? &x : nullptr;
}

// The fused plan's encoder over pairs [b0, b0 + nb): every per-pair pointer
// moved to pair b0 (the pair-major layouts of carve_encoder / carve_forward).
static int run_encoder_part(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                            const EncoderPlan &plan, const EncBufs &e, float *normed, _Float16 *normed_s, float *conf,
                            hipStream_t s, Ragged rg, int b0, int nb) {
    const int N = plan.N, Npad = plan.Npad;
    const size_t rows = (size_t)b0 * Npad * CH;
    EncBufs eh = e;
    eh.feat = e.feat + rows;
    eh.q = e.q + 2 * rows;
    eh.k = e.k + 2 * rows;
    eh.v = e.v + 2 * rows;
    eh.q2 = e.q2 + 2 * rows;
    eh.k2 = e.k2 + 2 * rows;
    eh.v2 = e.v2 + 2 * rows;
    eh.vexp = e.vexp + (size_t)b0 * (Npad / 32);
    eh.vexp2 = e.vexp2 + (size_t)b0 * (Npad / 32);
    const size_t mstr = plan.m_layout == M_PACKED ? mpack_floats(N) : (size_t)N * N;
    Ragged rh = rg;
    if (rg.nv) rh.nv = rg.nv + b0;
    if (rg.sv) rh.sv = rg.sv + b0;
    if (rg.po) rh.po = rg.po + b0;
    // (the batch's plan on nb pairs, not nb pairs' own)
    return run_encoder(lay, packed, corr_pos + (size_t)b0 * N * lay.in_dim, M + (size_t)b0 * mstr, plan.for_pairs(nb), eh,
                       nullptr, normed + (size_t)b0 * N * CH, normed_s + (size_t)b0 * N * 2 * CH, conf + (size_t)b0 * N, s,
                       rh);
}

// run_encoder for the forward: the fused plan as P concurrent parts given side
// streams ss and the part boundaries (enc_halves / enc_bounds; rg.po, when set,
// must then order each part's pairs on its own: launch_ragged_order per part),
// else run_encoder itself.
int run_encoder_fwd(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                    const EncoderPlan &plan, const EncBufs &e, float *normed, _Float16 *normed_s, float *conf,
                    hipStream_t s, Ragged rg, SideStream *ss, const int *bounds, int P) {
    if (!ss) return run_encoder(lay, packed, corr_pos, M, plan, e, nullptr, normed, normed_s, conf, s, rg);
    std::lock_guard<std::mutex> lock(ss->mu);
    // The side streams are shared by every caller stream of the device.  A side
    // stream forked into another thread's graph capture stays in that capture
    // until it ends: enqueueing there from a stream outside that capture would
    // record into (or invalidate) the other graph, so such a call runs on one
    // stream (bitwise the same results).
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone, c2 = hipStreamCaptureStatusNone;
        unsigned long long id = 0, id2 = 0;
        HIPCHK(hipStreamGetCaptureInfo(s, &cs, &id));
        for (int i = 1; i < P; ++i) {
            HIPCHK(hipStreamGetCaptureInfo(ss->s2[i - 1], &c2, &id2));
            if (c2 != hipStreamCaptureStatusNone && (cs != hipStreamCaptureStatusActive || id2 != id))
                return run_encoder(lay, packed, corr_pos, M, plan, e, nullptr, normed, normed_s, conf, s, rg);
        }
    }
    HIPCHK(hipEventRecord(ss->fork, s));
    int forked = 1, r = PDSC_OK;
    for (; forked < P; ++forked)
        if (hipStreamWaitEvent(ss->s2[forked - 1], ss->fork, 0) != hipSuccess) {
            r = fail(PDSC_ERR_HIP, "hipStreamWaitEvent (fork)");
            break;
        }
    for (int i = 0; r == PDSC_OK && i < P; ++i)
        r = run_encoder_part(lay, packed, corr_pos, M, plan, e, normed, normed_s, conf, i ? ss->s2[i - 1] : s, rg,
                             bounds[i], bounds[i + 1] - bounds[i]);
    // join every side stream that was forked, on success AND on error: the
    // caller's stream must not run ahead of work a side stream may still do in
    // the workspace, and a capture must not end with an unjoined fork
    for (int i = 1; i < forked; ++i) {
        const hipError_t a = hipEventRecord(ss->join[i - 1], ss->s2[i - 1]);
        const hipError_t b = a == hipSuccess ? hipStreamWaitEvent(s, ss->join[i - 1], 0) : a;
        if (b != hipSuccess && r == PDSC_OK) r = fail(PDSC_ERR_HIP, "join: %s", hipGetErrorString(b));
    }
    return r;
}

// The standalone encoder's plan: on the caller's dense M (plan_encoder's dense_m_caller).
static int encoder_plan_for(const pdsc_config *cfg, int B, int N, EncoderPlan &plan) {
    RET_IF(check_cfg(cfg));
    int S, k;  // (the forwards' limits hold for the standalone encoder too)
    RET_IF(check_shape(cfg, B, N, S, k));
    plan = plan_encoder(B, N, cfg->precision == PDSC_PRECISION_F32, true);
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

// ---------------------------------------------------------------- a2-a4
size_t pdsc_encoder_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N) {
    EncoderPlan plan;
    if (encoder_plan_for(cfg, B, N, plan) != PDSC_OK) return 0;
    Carve c(nullptr);
    carve_encoder(c, plan);
    return c.off;
}

int32_t pdsc_encoder_f32(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                         const float *M, int32_t B, int32_t N, float *feat, float *normed, float *conf,
                         void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    EncoderPlan plan;
    RET_IF(encoder_plan_for(cfg, B, N, plan));
    if (!packed || !corr_pos || !M || !normed || !conf || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_encoder_workspace_bytes(cfg, B, N)));
    Carve c(ws);
    const EncBufs e = carve_encoder(c, plan);
    const PackLayout lay = make_layout(cfg->num_layers, cfg->in_dim);
    return run_encoder(lay, packed, corr_pos, M, plan, e, feat, normed, nullptr, conf, S_(stream));
}

int32_t pdsc_attention_timing(void *const *start_events, void *const *stop_events, int32_t capacity,
                              int32_t *count) {
    if (capacity > 0 && (!start_events || !stop_events || !count))
        return fail(PDSC_ERR_ARG, "null events/count with capacity %d", capacity);
    g_tstart = reinterpret_cast<hipEvent_t *>(const_cast<void **>(start_events));
    g_tstop = reinterpret_cast<hipEvent_t *>(const_cast<void **>(stop_events));
    g_tcap = capacity;
    g_tcount = count;
    return PDSC_OK;
}

int32_t pdsc_diag_qkv_delay(int32_t loops) {
    if (loops < 0) return fail(PDSC_ERR_ARG, "loops=%d", loops);
    g_diag_qkv_delay = loops;
    return PDSC_OK;
}

int32_t pdsc_attention_layout(int32_t B, int32_t N, int32_t precision, int32_t *Npad, int32_t *nsplit) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !Npad || !nsplit) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    const EncoderPlan plan = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false);
    *Npad = plan.Npad;
    *nsplit = plan.nsplit;
    return PDSC_OK;
}

int32_t pdsc_encoder_plan(int32_t B, int32_t N, int32_t precision, int32_t *fused) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !fused) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    const EncoderPlan plan = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false);
    *fused = plan.fused() ? 1 : (plan.w64() ? 2 : 0);
    return PDSC_OK;
}

int32_t pdsc_encoder_plan_vfold(int32_t B, int32_t N, int32_t precision, int32_t *vfold) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !vfold) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    *vfold = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false).vfold ? 1 : 0;
    return PDSC_OK;
}

}  // extern "C"
