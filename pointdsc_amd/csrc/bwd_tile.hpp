// bwd_tile.hpp -- the tile loop the training kernels share (attention_bwd.hip,
// sm_loss_fused.hip): a workgroup = 4 waves x 32 stationary rows kept in
// registers, 32-row tiles of the other operand streamed through LDS, both
// products on v_mfma_f32_32x32x2_f32; and how a pair's streamed tiles are split
// over workgroups to fill the chip.
#pragma once
#include <algorithm>

#include "pdsc_internal.hpp"

namespace pdsc {

constexpr int BW_T = 32;           // rows per tile (one MFMA block)
constexpr int BW_NW = 4;           // waves per workgroup
constexpr int BW_ROWS = BW_NW * BW_T;  // stationary rows per workgroup
constexpr int BW_STR = CH + 4;     // LDS row stride: conflict-free ds_read_b128 columns (attention.hpp)
constexpr int BW_TARGET = 512;     // workgroups the split aims at (2 per CU)
constexpr float BW_SCALE = 0.08838834764831845f;  // 1 / sqrt(128)

// How a pair's tiles are split over workgroups (max_split: a cap on the partials).
struct BwdGrid {
    int B, N, nblk;     // nblk: blocks of BW_ROWS stationary rows per pair
    int nsplit, tps;    // splits of the streamed tiles, tiles per split
};
inline BwdGrid bwd_grid(int B, int N, int max_split = 1 << 30) {
    BwdGrid g;
    g.B = B;
    g.N = N;
    g.nblk = (N + BW_ROWS - 1) / BW_ROWS;
    const int nt = (N + BW_T - 1) / BW_T;
    int ns = (BW_TARGET + B * g.nblk - 1) / (B * g.nblk);
    ns = std::max(1, std::min(std::min(ns, max_split), std::max(1, nt / 2)));
    g.tps = (nt + ns - 1) / ns;
    g.nsplit = (nt + g.tps - 1) / g.tps;
    return g;
}

// A wave's 32 stationary rows: lane (h, l32) keeps channels 64 h .. 64 h + 63 of
// row r0 + l32 (the MFMA k-step i pairs channel i with channel 64 + i); rows >= N are 0.
PDSC_DEV void load_rows64(const float *__restrict__ x, int row, int N, int h, float out[64]) {
    if (row < N) {
        const f32x4 *src4 = reinterpret_cast<const f32x4 *>(x + (size_t)row * CH + h * 64);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const f32x4 t = src4[i];
            out[4 * i] = t[0];
            out[4 * i + 1] = t[1];
            out[4 * i + 2] = t[2];
            out[4 * i + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 64; ++i) out[i] = 0.0f;
    }
}

// The streamed tile: 32 rows of two [.][CH] arrays through registers into LDS
// (stride BW_STR), rows >= N as zeros; 256 threads, 4 float4 per array each.
struct TileRegs {
    f32x4 a[4], b[4];
};
PDSC_DEV void tile_load(const float *__restrict__ xa, const float *__restrict__ xb, int row0, int N, int tid,
                        TileRegs &t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = row0 + (idx >> 5), c4 = idx & 31;
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        t.a[i] = row < N ? *reinterpret_cast<const f32x4 *>(xa + (size_t)row * CH + 4 * c4) : z;
        t.b[i] = row < N ? *reinterpret_cast<const f32x4 *>(xb + (size_t)row * CH + 4 * c4) : z;
    }
}
PDSC_DEV void tile_store(float *la, float *lb, int tid, const TileRegs &t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 5, c4 = idx & 31;
        *reinterpret_cast<f32x4 *>(la + row * BW_STR + 4 * c4) = t.a[i];
        *reinterpret_cast<f32x4 *>(lb + row * BW_STR + 4 * c4) = t.b[i];
    }
}

// acc (32 x 32) = A B^T over the 128 channels: A's row l32 from LDS (stride
// BW_STR), B's row l32 from the lane's 64 registers.
PDSC_DEV f32x16 dot_lds_reg(const float *__restrict__ la, const float reg[64], int h, int l32) {
    f32x16 acc = zero16();
    const float *p = la + l32 * BW_STR + h * 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p + 4 * i);
        acc = mfma32(a[0], reg[4 * i], acc);
        acc = mfma32(a[1], reg[4 * i + 1], acc);
        acc = mfma32(a[2], reg[4 * i + 2], acc);
        acc = mfma32(a[3], reg[4 * i + 3], acc);
    }
    return acc;
}
// O (32 x 128, as 4 accumulators: O_t column l32 = channel 4 l32 + t) += W^T-as-held X:
// w[s] is the weight of (accumulator row acc_row(s, h), lane l32), X's row
// acc_row(s, h) comes from LDS.  (attention.hpp's O += P V.)
PDSC_DEV void accum_rows(const float w[16], const float *__restrict__ lx, int h, int l32, f32x16 &O0, f32x16 &O1,
                         f32x16 &O2, f32x16 &O3) {
    const float *p = lx + 4 * l32 + 4 * h * BW_STR;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(p + ((s & 3) + 8 * (s >> 2)) * BW_STR);
        O0 = mfma32(w[s], x[0], O0);
        O1 = mfma32(w[s], x[1], O1);
        O2 = mfma32(w[s], x[2], O2);
        O3 = mfma32(w[s], x[3], O3);
    }
}

PDSC_DEV void store_rows(float *__restrict__ out, int row0, int N, int h, int l32, const f32x16 &O0, const f32x16 &O1,
                         const f32x16 &O2, const f32x16 &O3) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + acc_row(r, h);
        if (row < N) *reinterpret_cast<f32x4 *>(out + (size_t)row * CH + 4 * l32) = f32x4{O0[r], O1[r], O2[r], O3[r]};
    }
}

}  // namespace pdsc
