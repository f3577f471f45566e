// encoder_row.hpp -- what the encoder row's files (encoder.hip, attention.hip)
// share, and nobody else: the attention kernels' headers, the plan-to-kernel
// dispatch helpers, launch_attention, and the device code that the attention's
// combine and both pointwise chains use.
#pragma once
#include <type_traits>

#include "attention.hpp"
#include "attention_h3.hpp"
#include "launch_plan.hpp"
#include "attention_w64.hpp"

namespace pdsc {

// Production instantiation of attention_h3.hpp: 4 waves x 32 queries per
// workgroup, XCD-aware block map.  (tools/attn_bench.hip A/B-times it against
// the exact-fp32-MFMA kernel of attention.hpp.)
constexpr int ATT_NW = 4;
// PDSC_PRECISION_F32: attention.hpp's exact-fp32 MFMA kernel, 32-key stages, libm expf
constexpr int ATT_F32_KTS = 32;

// the h3 kernels' grid argument for layer `layer` (stream-K: the uniform batch's form)
static AttnGridH3 plan_grid_h3(const EncoderPlan &plan, const Ragged &rg, int layer) {
    const bool sk = plan.kind == ATT_W64_SK;
    return AttnGridH3{plan.B, plan.N, plan.Npad, plan.nqb, plan.fused() ? 1 : plan.nsplit, plan.sps,
                      sk ? nullptr : rg.nv, sk ? nullptr : rg.po, plan.rev(rg, layer)};
}

// A run-time bool / int of the plan as a kernel template argument: f(std::bool_constant) / f(std::integral_constant).
template <typename F> static void with_bool(bool b, F &&f) { b ? f(std::true_type{}) : f(std::false_type{}); }
template <int V, int... Vs, typename F> static void with_int(int v, F &&f) {
    if (v == V) f(std::integral_constant<int, V>{});
    else if constexpr (sizeof...(Vs) > 0) with_int<Vs...>(v, f);
}

// One layer's split attention as the plan says (attention.hip).
// q, k, v: the fp16 hi/lo split layouts of h3.hpp (4 B per element), or fp32
// [B][Npad][CH] rows for the exact-fp32 plan (attention.hpp).
// M: dense [B][N][N] or symmetric-packed [B][mpack_floats(N)], per plan.m_layout.
// vexp: [B][Npad/32] V-tile exponents of the H3 layout; unused for f32.
// opart [B][nsplit][Npad x CH] (rows for f32, h3_opart_off's tiling for H3), ml [B][nsplit][Npad][2].
hipError_t launch_attention(const EncoderPlan &plan, const void *q, const void *k, const void *v, const float *vexp,
                            const float *M, float *opart, float *ml, hipStream_t s, Ragged rg = {}, int layer = 0);

// Combine partials -> msg [B][N][CH] (the standalone attention; encoder.hip).
hipError_t launch_attn_combine(const float *opart, const float *ml, bool f32, int B, int N, int Npad, int nsplit,
                               float *msg, hipStream_t s);

// Combine the split partials of one row segment: msg = sum_s O_s e^{m_s-m*} / sum_s l_s e^{m_s-m*}.
// Channels d0 .. d0+15 (d0 % 16 == 0) as 4 runs of 4: opart rows [Npad][CH]
// (F32 attention) or the fragment-block tiling (H3, h3.hpp: run a
// of the 16 sits in block 2 (d0/16) + (a >> 1), lane half a & 1).
// Loads are issued in batches (8 maxima, then 4 splits' m, l and 16 channels)
// before any is used: one L2 round trip per batch instead of one per split
// (the split loop's loads otherwise wait for each other: 10.6 of a single
// N = 1000 pair's 25 us pw_mid launch went to the 16-split combine).  Same
// arithmetic, same order as the one-load-per-split loop.
#ifndef PDSC_C16_ONE
#define PDSC_C16_ONE 8  // A/B build knob (-DPDSC_C16_ONE=0: the chunked loads only)
#endif
constexpr int C16_ONE = PDSC_C16_ONE;  // combine16: up to this many splits in one batch of loads (r06)
template <bool F32>
PDSC_DEV void combine16(const float *__restrict__ opart, const float *__restrict__ ml, int b,
                        int nsplit, int Npad, int row, int d0, float out[16]) {
    const float *mlb = ml + ((size_t)b * nsplit * Npad + row) * 2;  // split s: mlb[s * Npad * 2 + {0, 1}]
    if (nsplit <= C16_ONE) {
        // every split's m, l and 16 channels in ONE batch of loads (one round
        // trip to the partials the attention launch just left in other XCDs'
        // caches, instead of three), the maximum from the loaded m's: the same
        // operations in the same order as the chunked loop below
        f32x2 mlv[C16_ONE > 0 ? C16_ONE : 1];
        f32x4 ov[C16_ONE > 0 ? C16_ONE : 1][4];
#pragma unroll
        for (int j = 0; j < C16_ONE; ++j) {
            if (j < nsplit) {
                const size_t base = (size_t)(b * nsplit + j) * Npad + row;
                mlv[j] = *reinterpret_cast<const f32x2 *>(ml + base * 2);
                const float *ob = opart + (base - row) * CH;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const size_t o = F32 ? (size_t)row * CH + d0 + 4 * i : h3_opart_off(row, d0 + 4 * i);
                    ov[j][i] = *reinterpret_cast<const f32x4 *>(ob + o);
                }
            }
        }
        float mstar = -INFINITY;
#pragma unroll
        for (int j = 0; j < C16_ONE; ++j)
            if (j < nsplit) mstar = fmaxf(mstar, mlv[j][0]);
        float L = 0.0f;
        f32x4 acc[4] = {};
#pragma unroll
        for (int j = 0; j < C16_ONE; ++j) {
            if (j < nsplit) {
                const float w = expf(mlv[j][0] - mstar);
                L += w * mlv[j][1];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += w * ov[j][i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) out[4 * i + e] = acc[i][e] / L;
        return;
    }
    float mstar = -INFINITY;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
        float mv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) mv[j] = s0 + j < nsplit ? mlb[(size_t)(s0 + j) * Npad * 2] : -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) mstar = fmaxf(mstar, mv[j]);
    }
    float L = 0.0f;
    f32x4 acc[4] = {};
    constexpr int SB = 4;
    for (int s0 = 0; s0 < nsplit; s0 += SB) {
        f32x2 mlv[SB];
        f32x4 ov[SB][4];
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            if (s0 + j < nsplit) {
                const size_t base = (size_t)(b * nsplit + s0 + j) * Npad + row;
                mlv[j] = *reinterpret_cast<const f32x2 *>(ml + base * 2);
                const float *ob = opart + (base - row) * CH;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const size_t o = F32 ? (size_t)row * CH + d0 + 4 * i : h3_opart_off(row, d0 + 4 * i);
                    ov[j][i] = *reinterpret_cast<const f32x4 *>(ob + o);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            if (s0 + j < nsplit) {
                const float w = expf(mlv[j][0] - mstar);
                L += w * mlv[j][1];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += w * ov[j][i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * i + e] = acc[i][e] / L;
}

// ---- what both pointwise chains use (pw_lds.hpp; encoder.hip: pw2)
enum Epi { EPI_BIAS = 0, EPI_RELU = 1, EPI_BN_RELU = 2, EPI_RESID = 3, EPI_RESID_R = 4 };

// ReLU that keeps NaN (torch.relu(nan) = nan; fmaxf(nan, 0) = 0).  The fp16
// range guard relies on it: a 3xfp16 operand beyond fp16's range (hi = inf,
// lo = -inf) makes its contraction NaN, and this carries the NaN on to the
// logits, where select_best_kernel flags the pair (pdsc.h, PDSC_ERR_RANGE)
// instead of a ReLU silently zeroing it.  Same value as fmaxf(x, 0) for every
// non-NaN x (-0 -> +0).  IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950.
PDSC_DEV float relu_nan(float x) { return __builtin_elementwise_maximum(x, 0.0f); }

constexpr int IN_LIMIT = 128;  // layer0 input width supported (datasets/ThreeDMatch.py:311-315: 70)

struct PwDense4 {  // PointCN + Q/K/V of one layer
    DenseOff pcn, q, k, v;
};
struct PwMsg {  // fc_message of one layer
    DenseOff fc0, fc3, fc6;
};

}  // namespace pdsc
