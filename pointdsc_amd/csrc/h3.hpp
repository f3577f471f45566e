// h3.hpp -- the 3xf16 operand format (attention_h3.hpp has the why): the fp16
// hi/lo HBM layouts, the split and the MFMA products on them.  What the kNN,
// the NSM and the feature similarity share with the attention and the
// pointwise chains; no kernel.
//
// HBM layouts (written by the pointwise kernels' epilogues, encoder.hip, or
// by split_qkv_kernel, attention.hip, for the standalone API), per pair, in 32-row tiles of
// 16 KiB made of 16 "fragment blocks" of 1 KiB: block (f, plane) holds, for
// each lane (h, n) of a wave in lane order, the 16 B (8 fp16) that lane feeds
// the MFMA as operand fragment f -- so a producer's store of one fragment and
// a consumer's load of it (or LDS-DMA + ds_read) are one contiguous 1 KiB:
//   Qs, Ks  fragment j (k-step, 0..7), lane (h, n): row n of the tile,
//           positions 16 j + 8h .. +7 of the row in qk_pos order (bits 2 and 3
//           of the channel index swapped); plane 0 = hi, 1 = lo
//   Vs      fragment i = 2t + s, lane (h, n): channel 32 t + n, the tile's
//           keys at v_keypos positions 16 s + 8h .. +7
// Each layout equals the fp32 tensor's size (4 B per element).
// The partial outputs (opart) use the same tiling for fp32: per 32-query tile
// 16 blocks (2 ks + g) of 64 lanes x 4 floats, lane (h, n) = query n,
// qk_pos positions 16 ks + 8h + 4g .. +3 (h3_opart_off) -- the k-step
// fragments of the message layer that consumes them.
#pragma once
#include "pdsc_internal.hpp"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace pdsc {

constexpr int H3_ROWB = 2 * CH * 2;          // bytes per Qs/Ks row (hi + lo)
constexpr int H3_TILE = 32;                  // keys per LDS tile
constexpr int H3_KTB = H3_TILE * H3_ROWB;    // K tile bytes (16 KiB)
constexpr int H3_VTB = 2 * CH * H3_TILE * 2; // V tile bytes (16 KiB)
constexpr int H3_PSHIFT = 7;                 // p = 2^(x - m + PSHIFT)
constexpr float H3_DEFER = 8.0f;             // re-base the max when it grows by > 2^8
#ifndef ATT_SOFTMAX_PRIO
#define ATT_SOFTMAX_PRIO 1  // s_setprio of the softmax section (build knob; 0 = off)
#endif
#ifndef ATT_QFMA
#define ATT_QFMA 1  // Q pre-scaled by log2(e)/sqrt(C) at production; logits minus the running base by one fma
#endif
#ifndef ATT_BUFDMA
#define ATT_BUFDMA 1  // K/V (and pw2 weight) LDS-DMA by buffer_load ... lds (no per-piece 64-bit address VALU)
#endif
constexpr float H3_QSCALE = 0.12751743082459868f;  // log2(e) / sqrt(128): the softmax's scale, in base 2
constexpr int H3_VEXP_MAX = 8;               // V tile pre-scale 2^e, 0 <= e <= 8
constexpr int H3_VEXP_TARGET = 5;            // ... lifting the tile's max |v| below 2^5

// The V-tile exponent for a tile whose max |v| is vmax: the largest e <= 8 with
// vmax 2^e < 2^H3_VEXP_TARGET (0 for vmax >= 2^4, vmax == 0 or non-finite vmax).
PDSC_DEV int h3_vexp(float vmax) {
    if (!(vmax > 0.0f) || !(vmax < 8192.0f)) return 0;
    int ex;
    frexpf(vmax, &ex);  // vmax < 2^ex
    return max(0, min(H3_VEXP_MAX, H3_VEXP_TARGET - ex));
}

// channel -> position in a Qs/Ks row: swap bits 2 and 3
PDSC_DEV constexpr int qk_pos(int c) { return (c & ~12) | ((c & 4) << 1) | ((c & 8) >> 1); }
// key (0..31 within a tile) -> position in a Vs plane row: swap bits 2 and 3
PDSC_DEV constexpr int v_keypos(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }
// Fragment-block tiling (above): 32 rows x 128 channels x (hi, lo) per tile;
// element offset of (fragment f, plane, lane) in fp16 units within the tile.
constexpr int H3_TILE_H = 2 * CH * H3_TILE;  // fp16 per tile (8192)
PDSC_DEV constexpr int h3_frag(int f, int plane, int lane) { return ((2 * f + plane) * 64 + lane) * 8; }

// element offsets (in fp16 units) inside one pair's buffers
PDSC_DEV size_t qs_off(int row, int half, int c) {
    const int p = qk_pos(c);
    return (size_t)(row >> 5) * H3_TILE_H + h3_frag(p >> 4, half, 32 * ((p >> 3) & 1) + (row & 31)) + (p & 7);
}
PDSC_DEV size_t ks_off(int row, int half, int c) { return qs_off(row, half, c); }
PDSC_DEV size_t vs_off(int key, int half, int c) {
    const int kp = v_keypos(key & 31);
    return (size_t)(key >> 5) * H3_TILE_H + h3_frag(2 * (c >> 5) + (kp >> 4), half, 32 * ((kp >> 3) & 1) + (c & 31)) +
           (kp & 7);
}
// fp32 offset of (row, channel c) in one (pair, split)'s opart of Npad rows
PDSC_DEV size_t h3_opart_off(int row, int c) {
    const int p = qk_pos(c);
    return (size_t)(row >> 5) * (H3_TILE * CH) + ((2 * (p >> 4) + ((p >> 2) & 1)) * 64 + 32 * ((p >> 3) & 1) + (row & 31)) * 4 +
           (p & 3);
}

// x = hi + lo (fp16 pair).  The empty asm pins x as the rounded fp32 value:
// without it the compiler folds a producing multiply into the hi conversion
// (v_fma_mixlo_f16: one rounding of the exact product) while lo is formed from the
// fp32-rounded product, so where that product rounds onto an fp16 tie, hi and
// lo disagree by one fp16 ulp (measured: 1 channel in ~10^4, 1e-4 errors).
PDSC_DEV void split_h(float x, _Float16 &hi, _Float16 &lo) {
    asm("" : "+v"(x));
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// Two values at once: hi = {f16(x0), f16(x1)} (one v_cvt_pk_f16_f32) and lo =
// {f16(x0 - hi0), f16(x1 - hi1)} by v_fma_mixlo / v_fma_mixhi, which form the
// exact difference of the fp32 value and the fp16 hi operand and round once --
// bit-identical to split_h (x - hi is exact in fp32), 1.5 instead of ~2.5 VALU
// per value.  Inline asm: the inputs are the rounded fp32 values by
// construction, and every use sees the same hi register.  ONE asm statement:
// the closing s_nop 1 gives both hi and lo the 2 wait states a VALU write needs
// before an MFMA reads the register as A/B (hipcc pads nothing inside asm, and
// its hazard recognizer does not see asm-written VGPRs); as separate statements
// the scheduler could move the hi.hi MFMA right after the cvt.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
PDSC_DEV void split2(float x0, float x1, uint32_t &hi, uint32_t &lo) {
    asm("v_cvt_pk_f16_f32 %0, %2, %3\n\t"
        "v_fma_mixlo_f16 %1, %2, 1.0, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(hi), "=&v"(lo)
        : "v"(x0), "v"(x1));
}
// 8 values (v[e] -> element e of the fragments)
PDSC_DEV void split8x(const float (&v)[8], f16x8 &hi, f16x8 &lo) {
    u32x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t a, b;
        split2(v[2 * e], v[2 * e + 1], a, b);
        h[e] = a;
        l[e] = b;
    }
    hi = __builtin_bit_cast(f16x8, h);
    lo = __builtin_bit_cast(f16x8, l);
}

// x (op) x of the lane 32 apart, on every lane, by v_permlane32_swap (no LDS
// round trip, unlike __shfl_xor's ds_bpermute); bit-identical to the shuffle
// form since max and + commute.
PDSC_DEV float halves_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
PDSC_DEV float halves_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

PDSC_DEV f32x16 mfma_h(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// a.b with a = ah + al, b = bh + bl: small terms first
PDSC_DEV f32x16 mfma_h3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16 c) {
    c = mfma_h(al, bh, c);
    c = mfma_h(ah, bl, c);
    return mfma_h(ah, bh, c);
}

// Products with a W_PLANES-plane weight w = wh + wm (+ wl) (pack.hip:
// pack_dense_kernel) and a two-plane activation x = xh + xl:
// x.w ~= xh.(wh + wm (+ wl)) + xl.wh, small terms first.  The dropped xl.wm is
// 2^-22 relative, as is a 2-plane weight's representation error (r01-r03 kept
// the lo plane: every fp32 weight exactly, one more product; r04 measured the
// two forms inside the same fp32 noise, tools/emulate_conv.py).
// mfma_xw3: A = activations (rows = points), B = weights; mfma_w3x: transposed.
PDSC_DEV f32x16 mfma_xw3(f16x8 xh, f16x8 xl, f16x8 wh, f16x8 wm, f16x8 wl, f32x16 c) {
    if constexpr (W_PLANES == 3) c = mfma_h(xh, wl, c);
    c = mfma_h(xh, wm, c);
    c = mfma_h(xl, wh, c);
    return mfma_h(xh, wh, c);
}
PDSC_DEV f32x16 mfma_w3x(f16x8 wh, f16x8 wm, f16x8 wl, f16x8 xh, f16x8 xl, f32x16 c) {
    if constexpr (W_PLANES == 3) c = mfma_h(wl, xh, c);
    c = mfma_h(wm, xh, c);
    c = mfma_h(wh, xl, c);
    return mfma_h(wh, xh, c);
}

PDSC_DEV __amdgpu_buffer_rsrc_t h3_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}

}  // namespace pdsc
