// pw_lds.hpp -- the LDS-tiled pointwise chain: pw_first / pw_mid / pw_last and
// what only they use.  Kernel templates: encoder.hip instantiates them
// (launch_pw_first / _mid / _last pick between these and the register-chained
// pw2_* per plan).
#pragma once
#include "encoder_row.hpp"

namespace pdsc {

// ============================================================ pointwise chain
// A workgroup (4 waves) owns PT = 64 points (two 32-row MFMA tiles) held in LDS
// and runs the whole per-point chain between two attention launches.
// Dense layer Y = epi(X W^T + b): A operand = X rows (lane -> point), B operand
// = packed W (one coalesced 1-KiB load per 4 MFMAs).  Wide layers (>= 128
// outputs): each wave owns column tiles and computes BOTH row tiles, so every
// weight fragment feeds two MFMAs; narrow layers (32/64 outputs): one
// (row tile, column tile) per wave so all four waves stay busy.
constexpr int S132 = CH + 4, S68 = CH2 + 4, S36 = CLS + 4;
constexpr int IN_MAX = 16;     // layer0 input width held in registers (pw_first)

// The wave's weight panel for output tile ct.  H3: per 16-input k-step, the hi
// and lo fragments (lane (h, n): inputs 16 ks + 8h .. +7 of output 32 ct + n).
// F32: per 8-input chunk j, lane (h, n) holds inputs 8j + 4h .. +3 of output
// 32 ct + n -- the exact-fp32 MFMA's k-step 4j + e uses input 8j + 4h + e (the
// activations are read with the same map, so the products pair up).
template <int IN, bool F32> struct WPanel;
template <int IN> struct WPanel<IN, false> {
    f16x8 h[IN / 16], m[IN / 16], l[W_PLANES == 3 ? IN / 16 : 1];  // (l: the 3-plane build only)
};
template <int IN> struct WPanel<IN, true> {
    f32x4 w[IN / 8];
};

template <int IN, int OUT, bool F32>
PDSC_DEV void load_wpanel(const float *__restrict__ pk, const DenseOff &off, int ct, int lane, WPanel<IN, F32> &p) {
    if constexpr (F32) {
        const float *W = pk + off.w;
        const size_t rowo = (size_t)(ct * 32 + (lane & 31)) * IN + 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < IN / 8; ++j) p.w[j] = *reinterpret_cast<const f32x4 *>(W + rowo + 8 * j);
    } else {
        const _Float16 *W = reinterpret_cast<const _Float16 *>(pk + off.w) + (size_t)ct * (IN / 16) * W3_BLOCK + 8 * lane;
#pragma unroll
        for (int ks = 0; ks < IN / 16; ++ks) {
            p.h[ks] = *reinterpret_cast<const f16x8 *>(W + ks * W3_BLOCK);
            p.m[ks] = *reinterpret_cast<const f16x8 *>(W + ks * W3_BLOCK + 512);
            if constexpr (W_PLANES == 3) p.l[ks] = *reinterpret_cast<const f16x8 *>(W + ks * W3_BLOCK + 1024);
        }
    }
}

// The 8 fp32 activations at positions 8h .. 8h+7 of the k-step starting at x
// (qk_pos order: channels 4h..4h+3 and 8+4h..8+4h+3; LDS, 16-B aligned) ->
// hi / lo fp16 fragments.
PDSC_DEV void split8(const float *x, int h, f16x8 &hi, f16x8 &lo) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(x + 4 * h), b = *reinterpret_cast<const f32x4 *>(x + 8 + 4 * h);
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    split8x(v, hi, lo);
}

// One 32-output tile of Y = epi(X W^T + b) for NRT row tiles.  H3: the fp16
// matrix cores with the 3-product split (h3.hpp), activations split
// as they are read from LDS, weights pre-split and pre-scaled by 2^s (the
// accumulator is scaled back by the exact 2^-s before the bias).  F32: exact
// fp32 MFMA 32x32x2 on the fp32 activations and weights.
template <int IN, int OUT, int EPI, int NRT, bool F32>
PDSC_DEV void dense_tile_w(const float *X, int xstr, const WPanel<IN, F32> &wp, const float *__restrict__ pk,
                           const DenseOff &off, int rt0, int ct, float *Y, int ystr, const float *__restrict__ resid,
                           int lane, const float *rres = nullptr) {
    const int h = lane >> 5, l32 = lane & 31;
    f32x16 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = zero16();
    if constexpr (F32) {
        const float *xp = X + (rt0 * 32 + l32) * xstr + 4 * h;
#pragma unroll
        for (int j = 0; j < IN / 8; ++j) {
#pragma unroll
            for (int i = 0; i < NRT; ++i) {
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xp + i * 32 * xstr + 8 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i] = mfma32(xv[e], wp.w[j][e], acc[i]);
            }
        }
    } else {
        const float *xp = X + (rt0 * 32 + l32) * xstr;
#pragma unroll
        for (int ks = 0; ks < IN / 16; ++ks) {
#pragma unroll
            for (int i = 0; i < NRT; ++i) {
                f16x8 xh, xl;
                split8(xp + i * 32 * xstr + 16 * ks, h, xh, xl);
                acc[i] = mfma_xw3(xh, xl, wp.h[ks], wp.m[ks], wp.l[W_PLANES == 3 ? ks : 0], acc[i]);
            }
        }
    }
    const int j = ct * 32 + l32;
    const float inv = pk[off.scale];
    const float bias = pk[off.bias + j];
    const float al = pk[off.alpha + j], be = pk[off.beta + j];
#pragma unroll
    for (int i = 0; i < NRT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (rt0 + i) * 32 + acc_row(r, h);
            float y = acc[i][r] * inv + bias;
            if (EPI == EPI_BN_RELU) y = relu_nan(y * al + be);  // eval BN as torch folds it, ReLU
            if (EPI == EPI_RELU) y = relu_nan(y);
            if (EPI == EPI_RESID) y = resid[row * CH + j] + y;      // res = feat + message (:44)
            if (EPI == EPI_RESID_R) y = rres[16 * i + r] + y;       // the same, rows loaded ahead (NRT = 1)
            Y[row * ystr + j] = y;
        }
}

template <int IN, int OUT, int EPI, int NRT, bool F32>
PDSC_DEV void dense_tile(const float *X, int xstr, const float *__restrict__ pk, const DenseOff &off,
                         int rt0, int ct, float *Y, int ystr, const float *__restrict__ resid, int lane) {
    WPanel<IN, F32> wp;  // the wave's whole weight panel, issued up front
    load_wpanel<IN, OUT, F32>(pk, off, ct, lane, wp);
    // keep the scheduler from sinking the loads next to their uses (each would
    // then expose a full L2 round trip per k-step); waits stay counted
    asm volatile("" ::: "memory");
    dense_tile_w<IN, OUT, EPI, NRT, F32>(X, xstr, wp, pk, off, rt0, ct, Y, ystr, resid, lane);
}

// Q/K/V projections (Conv1d 128 -> 128 + bias, :36-38) of the PT-point tile,
// written as fp16 hi/lo splits in the attention_h3 layouts.  Wave `ct` owns
// output channels ct*32..+31 of both 32-point row tiles.
//   SPLIT_Q, SPLIT_K: transposed product (accumulator rows = channels, lane =
//     point), so registers 8s..8s+7 are 8 consecutive qk_pos positions: one
//     16-B store of hi and one of lo per (row tile, s); K chunks swizzled.
//   SPLIT_V: lane = channel, registers 8s..8s+7 = 8 consecutive v_keypos
//     positions of the point tile: 16-B stores into the tile's V planes.
enum SplitMode { SPLIT_Q = 0, SPLIT_K = 1, SPLIT_V = 2 };

// The PT x 128 activation tile split once into hi / lo fp16 in LDS (row r:
// 16 hi chunks of 16 B then 16 lo chunks, chunk c stored at c ^ (r & 15) so a
// fragment read -- 32 rows, one chunk each -- is conflict-free).  Shared by the
// Q, K and V products instead of re-splitting per wave and per product.
constexpr int XS_ROWB = 2 * CH * 2;  // bytes per split row
template <int PTT, int NT = 256>
PDSC_DEV void split_tile(const float *X, int xstr, char *Xs, int tid) {
    constexpr int TPR = NT / PTT, CPT = 16 / TPR;  // threads per row, chunks per thread
    const int r = tid / TPR;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int c = (tid % TPR) * CPT + q;  // chunk c = positions 8c .. 8c+7 (qk_pos order)
        f16x8 hi, lo;
        split8(X + r * xstr + 16 * (c >> 1), c & 1, hi, lo);
        const int o = r * XS_ROWB + 16 * (c ^ (r & 15));
        *reinterpret_cast<f16x8 *>(Xs + o) = hi;
        *reinterpret_cast<f16x8 *>(Xs + o + CH * 2) = lo;
    }
}

// SPLIT_V also sets the tile exponents vexp[p0/32 + i] (h3.hpp) from
// the max |v| over the 4 waves' channel tiles, exchanged through `red` (LDS,
// 4 * NRT floats no other wave reads at this point; one barrier).
// active = false (8-wave workgroups, SPLIT_V): the wave only joins the barrier.
template <int MODE, int NRT>
PDSC_DEV void dense_split(const char *Xs, const WPanel<CH, false> &wp, const float *__restrict__ pk,
                          const DenseOff &off, int ct, _Float16 *__restrict__ dst, int p0, int lane,
                          float *red = nullptr, float *__restrict__ vexp = nullptr, bool active = true) {
    const int h = lane >> 5, l32 = lane & 31;
    f32x16 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = zero16();
    if (active)
#pragma unroll
    for (int ks = 0; ks < CH / 16; ++ks) {
#pragma unroll
        for (int i = 0; i < NRT; ++i) {
            const int r = 32 * i + l32;
            const char *xr = Xs + r * XS_ROWB + 16 * ((2 * ks + h) ^ (r & 15));
            const f16x8 xh = *reinterpret_cast<const f16x8 *>(xr);
            const f16x8 xl = *reinterpret_cast<const f16x8 *>(xr + CH * 2);
            acc[i] = MODE == SPLIT_V ? mfma_xw3(xh, xl, wp.h[ks], wp.m[ks], wp.l[W_PLANES == 3 ? ks : 0], acc[i])
                                     : mfma_w3x(wp.h[ks], wp.m[ks], wp.l[W_PLANES == 3 ? ks : 0], xh, xl, acc[i]);
        }
    }
    const float inv = pk[off.scale];
    if constexpr (MODE == SPLIT_V) {
        const int c = ct * 32 + l32;
        const float bias = pk[off.bias + c];
        int ev[NRT];
        if (active)
#pragma unroll
        for (int i = 0; i < NRT; ++i) {
            float m = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][r] = acc[i][r] * inv + bias;
                m = fmaxf(m, fabsf(acc[i][r]));
            }
            m = wave_max(m);
            if (lane == 0) red[4 * i + ct] = m;
        }
        __syncthreads();
        if (!active) return;
#pragma unroll
        for (int i = 0; i < NRT; ++i) {
            ev[i] = h3_vexp(fmaxf(fmaxf(red[4 * i], red[4 * i + 1]), fmaxf(red[4 * i + 2], red[4 * i + 3])));
            if (ct == 0 && lane == 0) vexp[(p0 >> 5) + i] = (float)ev[i];
        }
#pragma unroll
        for (int i = 0; i < NRT; ++i) {
            _Float16 *tile = dst + (size_t)((p0 >> 5) + i) * H3_TILE_H;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    _Float16 a, b;
                    split_h(ldexpf(acc[i][8 * s + e], ev[i]), a, b);
                    hi[e] = a;
                    lo[e] = b;
                }
                *reinterpret_cast<f16x8 *>(tile + h3_frag(2 * ct + s, 0, lane)) = hi;
                *reinterpret_cast<f16x8 *>(tile + h3_frag(2 * ct + s, 1, lane)) = lo;
            }
        }
    } else {
        float bias[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[r] = pk[off.bias + ct * 32 + acc_row(r, h)];
#pragma unroll
        for (int i = 0; i < NRT; ++i) {
            _Float16 *tile = dst + (size_t)((p0 >> 5) + i) * H3_TILE_H;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    _Float16 a, b;
                    const float y = acc[i][8 * s + e] * inv + bias[8 * s + e];
                    split_h(MODE == SPLIT_Q && ATT_QFMA ? y * H3_QSCALE : y, a, b);
                    hi[e] = a;
                    lo[e] = b;
                }
                *reinterpret_cast<f16x8 *>(tile + h3_frag(2 * ct + s, 0, lane)) = hi;
                *reinterpret_cast<f16x8 *>(tile + h3_frag(2 * ct + s, 1, lane)) = lo;
            }
        }
    }
}

// Y = epi(X W^T + b) over a PTT-point tile (PTT/32 row tiles) by 4 waves.
template <int IN, int OUT, int EPI, int PTT, bool F32, int NWV = 4>
PDSC_DEV void dense64(const float *X, int xstr, const float *__restrict__ pk, const DenseOff &off, float *Y,
                      int ystr, const float *__restrict__ resid, int wave, int lane) {
    constexpr int NCT = OUT / 32, NRT = PTT / 32;
    static_assert(NWV == 4 || NRT == 1, "8-wave workgroups take 32-point tiles");
    if constexpr (NCT >= 4) {
        for (int ct = wave; ct < NCT; ct += NWV)
            dense_tile<IN, OUT, EPI, NRT, F32>(X, xstr, pk, off, 0, ct, Y, ystr, resid, lane);
    } else if constexpr (NRT == 2) {
        const int rt = wave & 1, ct = wave >> 1;
        if (ct < NCT) dense_tile<IN, OUT, EPI, 1, F32>(X, xstr, pk, off, rt, ct, Y, ystr, resid, lane);
    } else {
        if (wave < NCT) dense_tile<IN, OUT, EPI, 1, F32>(X, xstr, pk, off, 0, wave, Y, ystr, resid, lane);
    }
}

// Copy a [PT][CH] LDS tile (stride xstr) to global rows [p0, p0 + nrows) (row stride CH).
template <int PTT, int NT = 256>
PDSC_DEV void store_rows(const float *X, int xstr, float *__restrict__ dst, int p0, int nrows, int tid) {
    for (int e = tid; e < PTT * (CH / 4); e += NT) {
        const int p = e / (CH / 4), c4 = e % (CH / 4);
        if (p < nrows)
            *reinterpret_cast<f32x4 *>(dst + (size_t)(p0 + p) * CH + 4 * c4) =
                *reinterpret_cast<const f32x4 *>(X + p * xstr + 4 * c4);
    }
}

// LDS: A, B = [PT][S132] (67,584 B -> 2 workgroups per CU).  The fc_message
// hidden tile C [PT][S68] and pw_first's corr_pos tile live in B, which is free
// until the residual add writes it.
template <int PTT> constexpr size_t pw_lds() { return (size_t)(2 * PTT * S132) * sizeof(float); }

// PointCN_l (Xin -> Xout) then Q/K/V_l (Xout -> the attention's input layouts);
// Xout rows -> feat.  Q, K, V point at the pair's buffers: the fp16 hi/lo split
// layouts (H3) or fp32 [Npad][CH] rows (F32, same bytes).
// only = 0 / 1 / 2 (H3): this workgroup writes Q / K / V alone (feat only with
// Q), as pcn_qkv8's `only` (pw_first_kernel's z dimension).
template <int PTT, bool F32>
PDSC_DEV void pcn_qkv(const float *Xin, float *Xout, const float *__restrict__ pk, const PwDense4 &d,
                      float *__restrict__ feat, _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                      _Float16 *__restrict__ V, float *__restrict__ vexp, int p0, int tid, int wave, int lane,
                      int only = -1) {
    // four 128 -> 128 products with the same wave -> output-tile map (ct = wave):
    // each one's weight panel is fetched while the previous one computes
    WPanel<CH, F32> pa, pb;
    if constexpr (!F32) {
        if (only >= 0) {  // workgroup-uniform
            load_wpanel<CH, CH, F32>(pk, d.pcn, wave, lane, pa);
            load_wpanel<CH, CH, F32>(pk, only == 0 ? d.q : (only == 1 ? d.k : d.v), wave, lane, pb);
            asm volatile("" ::: "memory");
            dense_tile_w<CH, CH, EPI_BN_RELU, PTT / 32, F32>(Xin, S132, pa, pk, d.pcn, 0, wave, Xout, S132, nullptr,
                                                             lane);
            __syncthreads();  // Xout complete; Xin is dead (it now holds the split copy of Xout)
            char *Xs = reinterpret_cast<char *>(const_cast<float *>(Xin));
            split_tile<PTT>(Xout, S132, Xs, tid);
            if (only == 0) store_rows<PTT>(Xout, S132, feat, p0, PTT, tid);
            __syncthreads();
            if (only == 0)
                dense_split<SPLIT_Q, PTT / 32>(Xs, pb, pk, d.q, wave, Q, p0, lane);
            else if (only == 1)
                dense_split<SPLIT_K, PTT / 32>(Xs, pb, pk, d.k, wave, K, p0, lane);
            else
                dense_split<SPLIT_V, PTT / 32>(Xs, pb, pk, d.v, wave, V, p0, lane, Xout, vexp);  // Xout is dead
            return;
        }
    }
    load_wpanel<CH, CH, F32>(pk, d.pcn, wave, lane, pa);
    load_wpanel<CH, CH, F32>(pk, d.q, wave, lane, pb);
    asm volatile("" ::: "memory");
    dense_tile_w<CH, CH, EPI_BN_RELU, PTT / 32, F32>(Xin, S132, pa, pk, d.pcn, 0, wave, Xout, S132, nullptr, lane);
    __syncthreads();  // Xout complete; Xin is dead (H3: it now holds the split copy of Xout)
    CH_STAMP(155);
    if constexpr (F32) {
        float *Qf = reinterpret_cast<float *>(Q) + (size_t)p0 * CH, *Kf = reinterpret_cast<float *>(K) + (size_t)p0 * CH,
              *Vf = reinterpret_cast<float *>(V) + (size_t)p0 * CH;
        load_wpanel<CH, CH, F32>(pk, d.k, wave, lane, pa);
        asm volatile("" ::: "memory");
        store_rows<PTT>(Xout, S132, feat, p0, PTT, tid);
        dense_tile_w<CH, CH, EPI_BIAS, PTT / 32, F32>(Xout, S132, pb, pk, d.q, 0, wave, Qf, CH, nullptr, lane);
        load_wpanel<CH, CH, F32>(pk, d.v, wave, lane, pb);
        asm volatile("" ::: "memory");
        dense_tile_w<CH, CH, EPI_BIAS, PTT / 32, F32>(Xout, S132, pa, pk, d.k, 0, wave, Kf, CH, nullptr, lane);
        dense_tile_w<CH, CH, EPI_BIAS, PTT / 32, F32>(Xout, S132, pb, pk, d.v, 0, wave, Vf, CH, nullptr, lane);
    } else {
        char *Xs = reinterpret_cast<char *>(const_cast<float *>(Xin));
        split_tile<PTT>(Xout, S132, Xs, tid);
        load_wpanel<CH, CH, F32>(pk, d.k, wave, lane, pa);
        asm volatile("" ::: "memory");
        store_rows<PTT>(Xout, S132, feat, p0, PTT, tid);
        __syncthreads();
        CH_STAMP(156);
        dense_split<SPLIT_Q, PTT / 32>(Xs, pb, pk, d.q, wave, Q, p0, lane);
        load_wpanel<CH, CH, F32>(pk, d.v, wave, lane, pb);
        asm volatile("" ::: "memory");
        CH_STAMP(157);
        dense_split<SPLIT_K, PTT / 32>(Xs, pa, pk, d.k, wave, K, p0, lane);
        CH_STAMP(158);
        dense_split<SPLIT_V, PTT / 32>(Xs, pb, pk, d.v, wave, V, p0, lane, Xout, vexp);  // Xout is dead
        CH_STAMP(159);
    }
}

// pcn_qkv for 8-wave workgroups (H3, 32-point tiles; small batches): PointCN on
// waves 0-3, then Q (waves 0-3) and K (waves 4-7) at once, then V (waves 0-3).
// Every output tile is the same dense_tile_w / dense_split code as the 4-wave
// form, so the same bits.  only = 0 / 1 / 2: this workgroup writes Q / K / V
// alone (and feat only for Q): three workgroups per point tile share the
// projections (pw_mid_kernel's z dimension), each streaming 4 of the chain's
// 7 weight panels instead of all 7 -- the single pair's chain is bound by
// each CU streaming its panels.
template <int PTT>
PDSC_DEV void pcn_qkv8(const float *Xin, float *Xout, const float *__restrict__ pk, const PwDense4 &d,
                       float *__restrict__ feat, _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                       _Float16 *__restrict__ V, float *__restrict__ vexp, int p0, int tid, int wave, int lane,
                       int only = -1) {
    static_assert(PTT == 32, "8-wave chain: 32-point tiles");
    const int w4 = wave & 3;
    const bool lo = wave < 4;
    WPanel<CH, false> pa, pb;
    if (only >= 0) {  // workgroup-uniform
        if (lo) {
            load_wpanel<CH, CH, false>(pk, d.pcn, w4, lane, pa);
            load_wpanel<CH, CH, false>(pk, only == 0 ? d.q : (only == 1 ? d.k : d.v), w4, lane, pb);
        }
        asm volatile("" ::: "memory");
        if (lo) dense_tile_w<CH, CH, EPI_BN_RELU, 1, false>(Xin, S132, pa, pk, d.pcn, 0, w4, Xout, S132, nullptr, lane);
        __syncthreads();  // Xout complete; Xin is dead (it now holds the split copy of Xout)
        CH_STAMP(155);
        char *Xs = reinterpret_cast<char *>(const_cast<float *>(Xin));
        split_tile<PTT, 512>(Xout, S132, Xs, tid);
        if (only == 0) store_rows<PTT, 512>(Xout, S132, feat, p0, PTT, tid);
        __syncthreads();
        CH_STAMP(156);
        CH_STAMP(157);
        CH_STAMP(158);
        if (only == 0) {
            if (lo) dense_split<SPLIT_Q, 1>(Xs, pb, pk, d.q, w4, Q, p0, lane);
        } else if (only == 1) {
            if (lo) dense_split<SPLIT_K, 1>(Xs, pb, pk, d.k, w4, K, p0, lane);
        } else {
            dense_split<SPLIT_V, 1>(Xs, pb, pk, d.v, w4, V, p0, lane, Xout, vexp, lo);  // Xout is dead
        }
        CH_STAMP(159);
        return;
    }
    if (lo) {
        load_wpanel<CH, CH, false>(pk, d.pcn, w4, lane, pa);
        load_wpanel<CH, CH, false>(pk, d.q, w4, lane, pb);
    } else {
        load_wpanel<CH, CH, false>(pk, d.k, w4, lane, pb);
    }
    asm volatile("" ::: "memory");
    if (lo) dense_tile_w<CH, CH, EPI_BN_RELU, 1, false>(Xin, S132, pa, pk, d.pcn, 0, w4, Xout, S132, nullptr, lane);
    __syncthreads();  // Xout complete; Xin is dead (it now holds the split copy of Xout)
    CH_STAMP(155);
    char *Xs = reinterpret_cast<char *>(const_cast<float *>(Xin));
    split_tile<PTT, 512>(Xout, S132, Xs, tid);
    if (lo) load_wpanel<CH, CH, false>(pk, d.v, w4, lane, pa);
    asm volatile("" ::: "memory");
    store_rows<PTT, 512>(Xout, S132, feat, p0, PTT, tid);
    __syncthreads();
    CH_STAMP(156);
    CH_STAMP(157);  // (Q and K run at once: the "k" phase of tools/pw_stamps.py)
    if (lo)
        dense_split<SPLIT_Q, 1>(Xs, pb, pk, d.q, w4, Q, p0, lane);
    else
        dense_split<SPLIT_K, 1>(Xs, pb, pk, d.k, w4, K, p0, lane);
    CH_STAMP(158);
    dense_split<SPLIT_V, 1>(Xs, pa, pk, d.v, w4, V, p0, lane, Xout, vexp, lo);  // Xout is dead
    CH_STAMP(159);
}

// layer0 (Conv1d in_dim -> 128, :54, :73) + PointCN_0 + QKV_0.
template <int PTT, bool F32>
__global__ __launch_bounds__(256, 2) void pw_first_kernel(const float *__restrict__ pk, size_t l0w,
                                                       size_t l0b, PwDense4 d,
                                                       const float *__restrict__ corr, int in_dim,
                                                       int N, int Npad, float *__restrict__ feat,
                                                       _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                                                       _Float16 *__restrict__ V, float *__restrict__ vexp,
                                                       const int *__restrict__ nv) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *XA = sm, *XB = sm + PTT * S132, *cp = XB;  // cp: [PTT][in_dim], consumed before XB is written
    const int b = blockIdx.y, p0 = blockIdx.x * PTT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t boff = (size_t)b * Npad * CH;
    const int n = nv ? nv[b] : N;  // this pair's rows (ragged batches); N: the row stride
    for (int e = tid; e < PTT * in_dim; e += 256) {
        const int p = e / in_dim;
        cp[e] = (p0 + p < n) ? corr[((size_t)b * N + p0) * in_dim + e] : 0.0f;
    }
    // thread -> output channel j (both halves of the block cover rows of opposite parity)
    const int j = tid & (CH - 1), p_off = tid >> 7;
    const float bj = pk[l0b + j];
    if (in_dim <= IN_MAX) {  // the weights in registers
        float w[IN_MAX];
#pragma unroll
        for (int c = 0; c < IN_MAX; ++c) w[c] = (c < in_dim) ? pk[l0w + j * in_dim + c] : 0.0f;
        __syncthreads();
        for (int p = p_off; p < PTT; p += 2) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < IN_MAX; ++c)
                if (c < in_dim) s = __builtin_fmaf(w[c], cp[p * in_dim + c], s);
            XA[p * S132 + j] = s + bj;
        }
    } else {  // wide inputs (in_dim <= IN_LIMIT): the same ascending fma chain, weights from L1
        __syncthreads();
        const float *wj = pk + l0w + (size_t)j * in_dim;
        for (int p = p_off; p < PTT; p += 2) {
            float s = 0.0f;
            for (int c = 0; c < in_dim; ++c) s = __builtin_fmaf(wj[c], cp[p * in_dim + c], s);
            XA[p * S132 + j] = s + bj;
        }
    }
    __syncthreads();
    pcn_qkv<PTT, F32>(XA, XB, pk, d, feat + boff, Q + 2 * boff, K + 2 * boff, V + 2 * boff,
                      vexp + (size_t)b * (Npad / 32), p0, tid, wave, lane, gridDim.z == 3 ? (int)blockIdx.z : -1);
}

// Combine the split partials of rows p0..p0+63 into X (stride S132); 4 threads per row.
template <int PTT, bool F32>
PDSC_DEV void combine_tile(const float *__restrict__ opart, const float *__restrict__ ml, int b,
                           int nsplit, int Npad, int p0, float *X, int tid) {
    constexpr int TPR = 256 / PTT, NH = 8 / TPR;  // threads per row, 16-channel pieces per thread
    const int p = tid / TPR;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
        const int d0 = (tid % TPR) * (16 * NH) + half * 16;
        float out[16];
        combine16<F32>(opart, ml, b, nsplit, Npad, p0 + p, d0, out);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<f32x4 *>(X + p * S132 + d0 + 4 * i) =
                f32x4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
    }
}

// fc_message + residual (:43-44): X = msg (A) -> C -> A (stride S68) -> R (B);
// C may alias R: it is dead once fc3 has read it (barrier before fc6).
template <int PTT, bool F32, int NWV = 4>
PDSC_DEV void message_resid(float *A, float *C, float *R, const float *__restrict__ pk, const PwMsg &m,
                            const float *__restrict__ feat_rows, int wave, int lane) {
    dense64<CH, CH2, EPI_BN_RELU, PTT, F32, NWV>(A, S132, pk, m.fc0, C, S68, nullptr, wave, lane);
    __syncthreads();
    CH_STAMP(152);
    dense64<CH2, CH2, EPI_BN_RELU, PTT, F32, NWV>(C, S68, pk, m.fc3, A, S68, nullptr, wave, lane);
    __syncthreads();
    CH_STAMP(153);
    dense64<CH2, CH, EPI_RESID, PTT, F32, NWV>(A, S68, pk, m.fc6, R, S132, feat_rows, wave, lane);
    __syncthreads();
    CH_STAMP(154);
}

// pw_mid's chain for the 8-wave workgroups of a Q / K / V split (three
// workgroups per 32-point tile, `only` = blockIdx.z), each wave's weight panel
// loaded a phase ahead of its layer instead of at its start (the single pair's
// chain is a sequence of L2 round trips: every layer of the message chain paid
// one before its MFMAs).  Roles: fc0 on waves 4-5 and fc3 on waves 6-7 (panels
// loaded before the combine), fc6 on waves 0-3 (panel and residual rows loaded
// before the combine), PointCN on waves 4-7 (panel loaded once fc0 / fc3 are
// done, during fc6), the projection on waves 0-3 (panel loaded after fc6,
// during PointCN).  Every output tile is the same dense_tile_w / dense_split
// arithmetic as message_resid + pcn_qkv8: the same bits.
PDSC_DEV void mid_split8(float *XA, float *XB, const float *__restrict__ pk, const PwMsg &m, const PwDense4 &d,
                         const float *__restrict__ opart, const float *__restrict__ ml, int b, int nsplit, int Npad,
                         int p0, const float *__restrict__ feat_rows, float *__restrict__ feat,
                         _Float16 *__restrict__ Q, _Float16 *__restrict__ K, _Float16 *__restrict__ V,
                         float *__restrict__ vexp, int only, int tid, int wave, int lane) {
    constexpr int PTT = 32;
    float *XC = XB;
    const int w4 = wave & 3, h = lane >> 5, l32 = lane & 31;
    WPanel<CH, false> pa;   // fc0 (waves 4-5), then PointCN (waves 4-7) / the projection (waves 0-3)
    WPanel<CH2, false> pb;  // fc3 (waves 6-7) / fc6 (waves 0-3)
    float res[16];          // fc6's residual rows (waves 0-3)
    if (wave >= 6)
        load_wpanel<CH2, CH2, false>(pk, m.fc3, wave - 6, lane, pb);
    else if (wave >= 4)
        load_wpanel<CH, CH2, false>(pk, m.fc0, wave - 4, lane, pa);
    asm volatile("" ::: "memory");
    if (tid < 256) {
        combine_tile<PTT, false>(opart, ml, b, nsplit, Npad, p0, XA, tid);
        // (after the combine: its loads and these do not share the register file)
        load_wpanel<CH2, CH, false>(pk, m.fc6, wave, lane, pb);
#pragma unroll
        for (int r = 0; r < 16; ++r) res[r] = feat_rows[acc_row(r, h) * CH + wave * 32 + l32];
    }
    asm volatile("" ::: "memory");
    __syncthreads();
    CH_STAMP(151);
    if (wave == 4 || wave == 5)  // fc0: XA -> XC
        dense_tile_w<CH, CH2, EPI_BN_RELU, 1, false>(XA, S132, pa, pk, m.fc0, 0, wave - 4, XC, S68, nullptr, lane);
    __syncthreads();
    CH_STAMP(152);
    if (wave >= 4) load_wpanel<CH, CH, false>(pk, d.pcn, w4, lane, pa);  // (waves 4-5 are done with fc0's)
    asm volatile("" ::: "memory");
    if (wave >= 6)  // fc3: XC -> XA
        dense_tile_w<CH2, CH2, EPI_BN_RELU, 1, false>(XC, S68, pb, pk, m.fc3, 0, wave - 6, XA, S68, nullptr, lane);
    __syncthreads();
    CH_STAMP(153);
    if (wave < 4)  // fc6 + residual: XA -> XB
        dense_tile_w<CH2, CH, EPI_RESID_R, 1, false>(XA, S68, pb, pk, m.fc6, 0, wave, XB, S132, nullptr, lane, res);
    __syncthreads();
    CH_STAMP(154);
    if (wave < 4) load_wpanel<CH, CH, false>(pk, only == 0 ? d.q : (only == 1 ? d.k : d.v), wave, lane, pa);
    asm volatile("" ::: "memory");
    if (wave >= 4)  // PointCN: XB -> XA
        dense_tile_w<CH, CH, EPI_BN_RELU, 1, false>(XB, S132, pa, pk, d.pcn, 0, w4, XA, S132, nullptr, lane);
    __syncthreads();  // XA complete; XB is dead (it now holds the split copy of XA)
    CH_STAMP(155);
    char *Xs = reinterpret_cast<char *>(XB);
    split_tile<PTT, 512>(XA, S132, Xs, tid);
    if (only == 0) store_rows<PTT, 512>(XA, S132, feat, p0, PTT, tid);
    __syncthreads();
    CH_STAMP(156);
    CH_STAMP(157);
    CH_STAMP(158);
    if (only == 0) {
        if (wave < 4) dense_split<SPLIT_Q, 1>(Xs, pa, pk, d.q, wave, Q, p0, lane);
    } else if (only == 1) {
        if (wave < 4) dense_split<SPLIT_K, 1>(Xs, pa, pk, d.k, wave, K, p0, lane);
    } else {
        dense_split<SPLIT_V, 1>(Xs, pa, pk, d.v, w4, V, p0, lane, XA, vexp, wave < 4);  // XA is dead
    }
    CH_STAMP(159);
}

template <int PTT, bool F32, int NWV = 4>
__global__ __launch_bounds__(NWV * 64, NWV == 4 ? 2 : 1) void pw_mid_kernel(const float *__restrict__ pk, PwMsg m, PwDense4 d,
                                                     const float *__restrict__ opart,
                                                     const float *__restrict__ ml, int nsplit, int N,
                                                     int Npad, const float *__restrict__ feat_in,
                                                     float *__restrict__ feat,
                                                     _Float16 *__restrict__ Q, _Float16 *__restrict__ K,
                                                     _Float16 *__restrict__ V, float *__restrict__ vexp,
                                                     int diag_delay, int prefetch) {
    // feat_in != feat: with gridDim.z == 3 the three workgroups of a point tile
    // read feat_in's rows as fc6's residual while the z = 0 one writes feat
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *XA = sm, *XB = sm + PTT * S132, *XC = XB;
    const int b = blockIdx.y, p0 = blockIdx.x * PTT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // diagnostic (PDSC_DIAG_QKV_DELAY, tests only): the K / V workgroups start
    // late, after the Q one has stored its PointCN rows
    if (diag_delay > 0 && blockIdx.z != 0)
        for (int i = 0; i < diag_delay; ++i) __builtin_amdgcn_s_sleep(127);
    const size_t boff = (size_t)b * Npad * CH;
#ifdef ATT_STAMPS
    unsigned long long *stp = att_stamp_ptr(wave);
    ATT_RSTAMP(stp, 186);
    ATT_STAMP(stp, 150);
#endif
    if constexpr (NWV == 8 && PTT == 32 && !F32) {
        if (prefetch && gridDim.z == 3) {  // workgroup-uniform
            mid_split8(XA, XB, pk, m, d, opart, ml, b, nsplit, Npad, p0, feat_in + boff + (size_t)p0 * CH, feat + boff,
                       Q + 2 * boff, K + 2 * boff, V + 2 * boff, vexp + (size_t)b * (Npad / 32), (int)blockIdx.z, tid,
                       wave, lane);
            ATT_RSTAMP(stp, 187);
            return;
        }
    }
    if (tid < 256) combine_tile<PTT, F32>(opart, ml, b, nsplit, Npad, p0, XA, tid);
    __syncthreads();
    ATT_STAMP(stp, 151);
    message_resid<PTT, F32, NWV>(XA, XC, XB, pk, m, feat_in + boff + (size_t)p0 * CH, wave, lane);
    if constexpr (NWV == 8)
        pcn_qkv8<PTT>(XB, XA, pk, d, feat + boff, Q + 2 * boff, K + 2 * boff, V + 2 * boff,
                      vexp + (size_t)b * (Npad / 32), p0, tid, wave, lane, gridDim.z == 3 ? (int)blockIdx.z : -1);
    else
        pcn_qkv<PTT, F32>(XB, XA, pk, d, feat + boff, Q + 2 * boff, K + 2 * boff, V + 2 * boff,
                          vexp + (size_t)b * (Npad / 32), p0, tid, wave, lane);
    ATT_RSTAMP(stp, 187);
}

template <int PTT, bool F32>
__global__ __launch_bounds__(256, 2) void pw_last_kernel(
    const float *__restrict__ pk, PwMsg m, DenseOff c0, DenseOff c2, size_t c4w, size_t c4b,
    const float *__restrict__ opart, const float *__restrict__ ml, int nsplit, int N, int Npad,
    const float *__restrict__ feat, float *__restrict__ feat_out, float *__restrict__ normed,
    _Float16 *__restrict__ normed_s, float *__restrict__ conf) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *XA = sm, *XB = sm + PTT * S132, *XC = XB;
    float *C1 = XA, *C2 = XA + PTT * S36;  // classifier hidden layers reuse A
    const int b = blockIdx.y, p0 = blockIdx.x * PTT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t boff = (size_t)b * Npad * CH;
    const int nrows = min(PTT, N - p0);
    combine_tile<PTT, F32>(opart, ml, b, nsplit, Npad, p0, XA, tid);
    __syncthreads();
    message_resid<PTT, F32>(XA, XC, XB, pk, m, feat + boff + (size_t)p0 * CH, wave, lane);
    // XB = corr_features rows
    if (feat_out) store_rows<PTT>(XB, S132, feat_out + (size_t)b * N * CH, p0, nrows, tid);
    {   // F.normalize(p=2, dim=-1, eps=1e-12) (:156); LPP lanes per point
        constexpr int LPP = 256 / PTT, CPL = CH / LPP;  // lanes per point, channels per lane
        const int p = tid / LPP, d0 = (tid % LPP) * CPL;
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const float x = XB[p * S132 + d0 + i];
            ss = __builtin_fmaf(x, x, ss);
        }
#pragma unroll
        for (int o = 1; o < LPP; o <<= 1) ss += __shfl_xor(ss, o);
        const float den = fmaxf(sqrtf(ss), 1e-12f);
        if (p < nrows) {
            float *dst = normed + ((size_t)b * N + p0 + p) * CH + d0;
#pragma unroll
            for (int i = 0; i < CPL / 4; ++i)
                *reinterpret_cast<f32x4 *>(dst + 4 * i) =
                    f32x4{XB[p * S132 + d0 + 4 * i] / den, XB[p * S132 + d0 + 4 * i + 1] / den,
                          XB[p * S132 + d0 + 4 * i + 2] / den, XB[p * S132 + d0 + 4 * i + 3] / den};
            if (!F32 && normed_s) {  // the fp16 hi/lo split copy (qk_pos order) the H3 seed kNN consumes
                _Float16 *ds = normed_s + ((size_t)b * N + p0 + p) * 2 * CH;
#pragma unroll
                for (int q = 0; q < CPL / 8; ++q) {
                    f16x8 hi, lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        _Float16 a, c;
                        split_h(XB[p * S132 + qk_pos(d0 + 8 * q + e)] / den, a, c);
                        hi[e] = a;
                        lo[e] = c;
                    }
                    *reinterpret_cast<f16x8 *>(ds + d0 + 8 * q) = hi;
                    *reinterpret_cast<f16x8 *>(ds + CH + d0 + 8 * q) = lo;
                }
            }
        }
    }
    // classification MLP 128 -> 32 -> 32 -> 1 on the unnormalised features (:171)
    dense64<CH, CLS, EPI_RELU, PTT, F32>(XB, S132, pk, c0, C1, S36, nullptr, wave, lane);
    __syncthreads();
    dense64<CLS, CLS, EPI_RELU, PTT, F32>(C1, S36, pk, c2, C2, S36, nullptr, wave, lane);
    __syncthreads();
    if (tid < nrows) {
        float s = 0.0f;
        for (int c = 0; c < CLS; ++c) s = __builtin_fmaf(pk[c4w + c], C2[tid * S36 + c], s);
        conf[(size_t)b * N + p0 + tid] = s + pk[c4b];
    }
}

}  // namespace pdsc
