// tsdf.hip -- f14: a sparse TSDF volume on the GPU, open3d's ScalableTSDFVolume
// (RGB8) as multiway/make_fragments.py:116-139 uses it: integrate every frame of a
// fragment, keep the vertices of the extracted mesh.  Restated; the contract is in
// include/pdsc.h.  All state lives in one caller-owned device buffer (bind_tsdf):
//
//   hash      open addressing, linear probing, hash_cap = the power of two >= 4
//             max_blocks: hkeys (63-bit block key, one 64-bit CAS inserts), hvals
//             (pool slot or -1), hstamp (the last frame that touched the entry)
//   pool      max_blocks blocks of 16^3 voxels (index x + 16 y + 256 z): tsdf,
//             weight fp32, colour 3 x fp32 (0 .. 255); bkeys [slot] the block's key
//   integrate tsdf_touch_kernel (a lane per 4th pixel: insert + stamp) ->
//             tsdf_alloc_kernel (a lane per hash entry: stamped entries without a
//             slot take one from the atomic counter; the frame's touched list) ->
//             tsdf_integrate_kernel (a workgroup per touched block).  Which slot a
//             block gets depends on the race; nothing the caller sees does.
//   extract   blocks sorted by key (hipCUB), tsdf_mark_kernel (a workgroup per
//             block, the 17^3 halo of tsdf and weight in LDS: every valid cube
//             flags its sign-changing edges at their base voxel, integer atomicOr),
//             counts, an exclusive scan, tsdf_emit_kernel in (key, voxel, axis) order
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "abi.hpp"
#include "pdsc_common.hpp"
#include "se3.hpp"

namespace pdsc {

typedef unsigned long long u64;
constexpr int TSDF_B = 16;                         // voxels per block edge
constexpr int TSDF_VOX = TSDF_B * TSDF_B * TSDF_B;  // 4096
constexpr int TSDF_HALO = TSDF_B + 1;
constexpr int TSDF_HALO_VOX = TSDF_HALO * TSDF_HALO * TSDF_HALO;  // 4913
constexpr int TSDF_WG = 256;
constexpr int TSDF_BIAS = 1 << 20;  // block indices in [-2^20, 2^20)
constexpr u64 TSDF_EMPTY = ~0ull;
constexpr int TSDF_MAX_BLOCKS = 1 << 17;  // 3 edges x 4096 voxels x 2^17 blocks: every count and offset fits an int
constexpr int TSDF_ERR_FULL = 1, TSDF_ERR_RANGE = 2;

struct TsdfHeader {
    int n_blocks;  // FIRST: the caller reads it (blocks that own a pool slot)
    int counter;   // the slot allocator (may overshoot inside a call)
    int status;    // of the running call: TSDF_ERR_* bits
    int n_touched;
    int frame;
    int n_points;  // of the last count pass
    int pad[2];
};
struct TsdfBufs {
    TsdfHeader *hdr;
    u64 *hkeys;
    int *hvals, *hstamp;
    int hash_cap;
    u64 *bkeys;
    int *touched;
    float *tsdf, *weight, *colour;
    unsigned *flags;
    u64 *skeys;
    int *iota, *order, *counts, *offsets;
    void *cub;
    size_t cub_bytes;
};

static int tsdf_hash_cap(int max_blocks) {
    int c = 64;
    while (c < 4 * (long long)max_blocks) c <<= 1;
    return c;
}
static size_t tsdf_cub_bytes(int n) {
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const u64 *)nullptr, (u64 *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int *)nullptr, (int *)nullptr, n + 1);
    return a > b ? a : b;
}
static void bind_tsdf(Carve &c, int max_blocks, TsdfBufs &B) {
    const size_t m = (size_t)max_blocks;
    B.hdr = c.take<TsdfHeader>(1);
    B.hash_cap = tsdf_hash_cap(max_blocks);
    B.hkeys = c.take<u64>(B.hash_cap);
    B.hvals = c.take<int>(B.hash_cap);
    B.hstamp = c.take<int>(B.hash_cap);
    B.bkeys = c.take<u64>(m);
    B.touched = c.take<int>(m);
    B.tsdf = c.take<float>(m * TSDF_VOX);
    B.weight = c.take<float>(m * TSDF_VOX);
    B.colour = c.take<float>(m * TSDF_VOX * 3);
    B.flags = c.take<unsigned>(m * TSDF_VOX);
    B.skeys = c.take<u64>(m);
    B.iota = c.take<int>(m);
    B.order = c.take<int>(m);
    B.counts = c.take<int>(m + 1);
    B.offsets = c.take<int>(m + 1);
    B.cub_bytes = tsdf_cub_bytes(max_blocks);
    B.cub = c.take_bytes(B.cub_bytes);
}

// ------------------------------------------------------------------ the hash
PDSC_DEV u64 tsdf_key(long long bx, long long by, long long bz) {
    return ((u64)(bx + TSDF_BIAS) << 42) | ((u64)(by + TSDF_BIAS) << 21) | (u64)(bz + TSDF_BIAS);
}
PDSC_DEV void tsdf_unkey(u64 k, int &bx, int &by, int &bz) {
    bx = (int)((k >> 42) & 0x1fffff) - TSDF_BIAS;
    by = (int)((k >> 21) & 0x1fffff) - TSDF_BIAS;
    bz = (int)(k & 0x1fffff) - TSDF_BIAS;
}
PDSC_DEV bool tsdf_in_range(long long b) { return b >= -TSDF_BIAS && b < TSDF_BIAS; }
PDSC_DEV unsigned tsdf_hash(u64 k, int cap) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 32) & (unsigned)(cap - 1); }

// the entry of `key`, inserted if absent; -1 when the table is full
PDSC_DEV int tsdf_insert(const TsdfBufs &B, u64 key) {
    unsigned h = tsdf_hash(key, B.hash_cap);
    for (int probe = 0; probe < B.hash_cap; ++probe) {
        const u64 cur = atomicCAS(B.hkeys + h, TSDF_EMPTY, key);
        if (cur == TSDF_EMPTY || cur == key) return (int)h;
        h = (h + 1) & (unsigned)(B.hash_cap - 1);
    }
    return -1;
}
// the pool slot of `key`, -1 if absent (or without a slot)
PDSC_DEV int tsdf_find(const TsdfBufs &B, u64 key) {
    unsigned h = tsdf_hash(key, B.hash_cap);
    for (int probe = 0; probe < B.hash_cap; ++probe) {
        const u64 cur = B.hkeys[h];
        if (cur == key) return B.hvals[h];
        if (cur == TSDF_EMPTY) return -1;
        h = (h + 1) & (unsigned)(B.hash_cap - 1);
    }
    return -1;
}

__global__ void tsdf_reset_kernel(TsdfBufs B, int max_blocks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B.hash_cap) {
        B.hkeys[i] = TSDF_EMPTY;
        B.hvals[i] = -1;
        B.hstamp[i] = -1;
    }
    if (i < max_blocks) B.iota[i] = i;
    if (i == 0) {
        TsdfHeader h = {};
        *B.hdr = h;
    }
}

__global__ void tsdf_begin_kernel(TsdfBufs B) {
    B.hdr->status = 0;
    B.hdr->n_touched = 0;
    B.hdr->frame += 1;
}

struct TsdfCam {
    int H, W;
    double fx, fy, cx, cy;
};

// step 1: every 4th pixel with depth > 0, to the world; the blocks within sdf_trunc of it
__global__ __launch_bounds__(TSDF_WG) void tsdf_touch_kernel(TsdfBufs B, const float *__restrict__ depth, TsdfCam C,
                                                             const double *__restrict__ extrinsic, double edge,
                                                             double sdf_trunc) {
    const int Ws = (C.W + 3) / 4, Hs = (C.H + 3) / 4;
    const int i = blockIdx.x * TSDF_WG + threadIdx.x;
    if (i >= Ws * Hs) return;
    const int u = 4 * (i % Ws), v = 4 * (i / Ws);
    const float d = depth[(size_t)v * C.W + u];
    if (!(d > 0.0f)) return;
    double E[12], Ei[12], p[3];
    aff_load(extrinsic, E);
    aff_inv(E, Ei);
    const double z = (double)d, x = (((double)u - C.cx) * z) / C.fx, y = (((double)v - C.cy) * z) / C.fy;
    aff_apply(Ei, x, y, z, p[0], p[1], p[2]);
    long long lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const double l = floor((p[a] - sdf_trunc) / edge), h = floor((p[a] + sdf_trunc) / edge);
        if (!(l >= -(double)TSDF_BIAS && h < (double)TSDF_BIAS)) {  // also NaN
            atomicOr(&B.hdr->status, TSDF_ERR_RANGE);
            return;
        }
        lo[a] = (long long)l;
        hi[a] = (long long)h;
    }
    const int frame = B.hdr->frame;
    for (long long bx = lo[0]; bx <= hi[0]; ++bx)
        for (long long by = lo[1]; by <= hi[1]; ++by)
            for (long long bz = lo[2]; bz <= hi[2]; ++bz) {
                const int h = tsdf_insert(B, tsdf_key(bx, by, bz));
                if (h < 0) {
                    atomicOr(&B.hdr->status, TSDF_ERR_FULL);
                    return;
                }
                B.hstamp[h] = frame;
            }
}

// pdsc_tsdf_write_blocks' touch: one lane per given block
__global__ void tsdf_touch_list_kernel(TsdfBufs B, const int *__restrict__ coords, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long bx = coords[3 * i], by = coords[3 * i + 1], bz = coords[3 * i + 2];
    if (!tsdf_in_range(bx) || !tsdf_in_range(by) || !tsdf_in_range(bz)) {
        atomicOr(&B.hdr->status, TSDF_ERR_RANGE);
        return;
    }
    const int h = tsdf_insert(B, tsdf_key(bx, by, bz));
    if (h < 0)
        atomicOr(&B.hdr->status, TSDF_ERR_FULL);
    else
        B.hstamp[h] = B.hdr->frame;
}

// a lane per hash entry: this frame's entries get a slot if they have none; the touched list
__global__ __launch_bounds__(TSDF_WG) void tsdf_alloc_kernel(TsdfBufs B, int max_blocks) {
    const int h = blockIdx.x * TSDF_WG + threadIdx.x;
    if (h >= B.hash_cap || B.hstamp[h] != B.hdr->frame) return;
    if (B.hdr->status & TSDF_ERR_RANGE) return;  // a range error: no block gets a slot, the volume is as it was
    int slot = B.hvals[h];
    if (slot < 0) {
        slot = atomicAdd(&B.hdr->counter, 1);
        if (slot >= max_blocks) {
            atomicOr(&B.hdr->status, TSDF_ERR_FULL);
            return;
        }
        B.hvals[h] = slot;
        B.bkeys[slot] = B.hkeys[h];
    }
    B.touched[atomicAdd(&B.hdr->n_touched, 1)] = slot;
}

__global__ void tsdf_alloc_finish_kernel(TsdfBufs B, int max_blocks) {
    if (B.hdr->counter > max_blocks) B.hdr->counter = max_blocks;
    B.hdr->n_blocks = B.hdr->counter;
}

// step 2: a workgroup per touched block (grid-stride over the touched list)
__global__ __launch_bounds__(TSDF_WG) void tsdf_integrate_kernel(TsdfBufs B, const float *__restrict__ depth,
                                                                 const uint8_t *__restrict__ colour, TsdfCam C,
                                                                 const double *__restrict__ extrinsic,
                                                                 double voxel_length, double sdf_trunc) {
    if (B.hdr->status) return;  // overflow: this frame changes no voxel
    double E[12];
    aff_load(extrinsic, E);
    const int nt = B.hdr->n_touched;
    for (int b = blockIdx.x; b < nt; b += gridDim.x) {
        const int slot = B.touched[b];
        int bx, by, bz;
        tsdf_unkey(B.bkeys[slot], bx, by, bz);
        for (int k = 0; k < TSDF_VOX / TSDF_WG; ++k) {
            const int vi = k * TSDF_WG + threadIdx.x;
            const int x = vi & 15, y = (vi >> 4) & 15, z = vi >> 8;
            const double wx = ((double)(bx * TSDF_B + x) + 0.5) * voxel_length,
                         wy = ((double)(by * TSDF_B + y) + 0.5) * voxel_length,
                         wz = ((double)(bz * TSDF_B + z) + 0.5) * voxel_length;
            double px, py, pz;
            aff_apply(E, wx, wy, wz, px, py, pz);
            if (!(pz > 0.0)) continue;
            const double uf = (C.fx * px) / pz + C.cx + 0.5, vf = (C.fy * py) / pz + C.cy + 0.5;
            if (!(uf > -1.0 && uf < (double)C.W && vf > -1.0 && vf < (double)C.H)) continue;
            const int u = (int)uf, v = (int)vf;
            const float d = depth[(size_t)v * C.W + u];
            if (!(d > 0.0f)) continue;
            const double rx = ((double)u - C.cx) / C.fx, ry = ((double)v - C.cy) / C.fy;
            const double sdf = ((double)d - pz) * sqrt((rx * rx + ry * ry) + 1.0);
            if (!(sdf > -sdf_trunc)) continue;
            const float tn = (float)fmin(1.0, sdf / sdf_trunc);
            const size_t g = (size_t)slot * TSDF_VOX + vi;
            const float w = B.weight[g], w1 = w + 1.0f;
            B.tsdf[g] = (B.tsdf[g] * w + tn) / w1;
            const uint8_t *c = colour + 3 * ((size_t)v * C.W + u);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) B.colour[3 * g + ch] = (B.colour[3 * g + ch] * w + (float)c[ch]) / w1;
            B.weight[g] = w1;
        }
    }
}

// ------------------------------------------------------------- blocks in and out
__global__ __launch_bounds__(TSDF_WG) void tsdf_read_kernel(TsdfBufs B, int n, int *coords, float *tsdf, float *weight,
                                                            float *colour) {
    const int slot = blockIdx.x;
    if (slot >= n) return;
    if (coords && threadIdx.x == 0) tsdf_unkey(B.bkeys[slot], coords[3 * slot], coords[3 * slot + 1], coords[3 * slot + 2]);
    for (int vi = threadIdx.x; vi < TSDF_VOX; vi += TSDF_WG) {
        const size_t g = (size_t)slot * TSDF_VOX + vi;
        if (tsdf) tsdf[g] = B.tsdf[g];
        if (weight) weight[g] = B.weight[g];
        if (colour)
            for (int ch = 0; ch < 3; ++ch) colour[3 * g + ch] = B.colour[3 * g + ch];
    }
}

__global__ __launch_bounds__(TSDF_WG) void tsdf_write_kernel(TsdfBufs B, const int *__restrict__ coords,
                                                             const float *__restrict__ tsdf,
                                                             const float *__restrict__ weight,
                                                             const float *__restrict__ colour) {
    if (B.hdr->status) return;
    const int i = blockIdx.x;
    const int slot = tsdf_find(B, tsdf_key(coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]));
    if (slot < 0) return;
    for (int vi = threadIdx.x; vi < TSDF_VOX; vi += TSDF_WG) {
        const size_t g = (size_t)slot * TSDF_VOX + vi, s = (size_t)i * TSDF_VOX + vi;
        B.tsdf[g] = tsdf[s];
        B.weight[g] = weight[s];
        for (int ch = 0; ch < 3; ++ch) B.colour[3 * g + ch] = colour[3 * s + ch];
    }
}

// ------------------------------------------------------------------ extraction
// the slots of the block and of its 7 (+x, +y, +z) neighbours: nb[dx + 2 dy + 4 dz]
PDSC_DEV void tsdf_neighbours(const TsdfBufs &B, int slot, int *nb) {
    if (threadIdx.x < 8) {
        int bx, by, bz;
        tsdf_unkey(B.bkeys[slot], bx, by, bz);
        const int dx = threadIdx.x & 1, dy = (threadIdx.x >> 1) & 1, dz = threadIdx.x >> 2;
        const long long nx = bx + dx, ny = by + dy, nz = bz + dz;
        nb[threadIdx.x] = threadIdx.x == 0 ? slot
                          : (tsdf_in_range(nx) && tsdf_in_range(ny) && tsdf_in_range(nz)) ? tsdf_find(B, tsdf_key(nx, ny, nz))
                                                                                            : -1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(TSDF_WG) void tsdf_mark_kernel(TsdfBufs B) {
    __shared__ float hf[TSDF_HALO_VOX], hw[TSDF_HALO_VOX];
    __shared__ int nb[8];
    const int slot = blockIdx.x;
    tsdf_neighbours(B, slot, nb);
    for (int i = threadIdx.x; i < TSDF_HALO_VOX; i += TSDF_WG) {
        const int x = i % TSDF_HALO, y = (i / TSDF_HALO) % TSDF_HALO, z = i / (TSDF_HALO * TSDF_HALO);
        const int s = nb[(x >> 4) + 2 * (y >> 4) + 4 * (z >> 4)];
        float f = 0.0f, w = 0.0f;  // an absent block: weight 0
        if (s >= 0) {
            const size_t g = (size_t)s * TSDF_VOX + (x & 15) + 16 * (y & 15) + 256 * (z & 15);
            f = B.tsdf[g];
            w = B.weight[g];
        }
        hf[i] = f;
        hw[i] = w;
    }
    __syncthreads();
    for (int k = 0; k < TSDF_VOX / TSDF_WG; ++k) {
        const int vi = k * TSDF_WG + threadIdx.x;
        const int x = vi & 15, y = (vi >> 4) & 15, z = vi >> 8;
        bool valid = true;
        bool neg[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int h = (x + (c & 1)) + TSDF_HALO * (y + ((c >> 1) & 1)) + TSDF_HALO * TSDF_HALO * (z + (c >> 2));
            valid = valid && hw[h] != 0.0f;
            neg[c] = hf[h] < 0.0f;
        }
        if (!valid) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int sa = 1 << a;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (c & sa) continue;  // c: the edge's base corner, c | sa its other end
                if (neg[c] == neg[c | sa]) continue;
                const int ex = x + (c & 1), ey = y + ((c >> 1) & 1), ez = z + (c >> 2);
                const int s = nb[(ex >> 4) + 2 * (ey >> 4) + 4 * (ez >> 4)];  // exists: the cube is valid
                atomicOr(B.flags + (size_t)s * TSDF_VOX + (ex & 15) + 16 * (ey & 15) + 256 * (ez & 15), 1u << a);
            }
        }
    }
}

// counts[b] = the flagged edges of the b-th block in key order
__global__ __launch_bounds__(TSDF_WG) void tsdf_count_kernel(TsdfBufs B, int n) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int slot = B.order[blockIdx.x];
    int c = 0;
    for (int vi = threadIdx.x; vi < TSDF_VOX; vi += TSDF_WG) c += __popc(B.flags[(size_t)slot * TSDF_VOX + vi]);
    atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        B.counts[blockIdx.x] = total;
        if (blockIdx.x == 0) B.counts[n] = 0;
    }
}

__global__ void tsdf_total_kernel(TsdfBufs B, int n) { B.hdr->n_points = B.offsets[n]; }

__global__ __launch_bounds__(TSDF_WG) void tsdf_emit_kernel(TsdfBufs B, double voxel_length, double *__restrict__ points,
                                                            double *__restrict__ colours) {
    __shared__ int scan[TSDF_WG];
    const int slot = B.order[blockIdx.x], t = threadIdx.x;
    int bx, by, bz;
    tsdf_unkey(B.bkeys[slot], bx, by, bz);
    unsigned fl[16];
    int c = 0;
    for (int k = 0; k < 16; ++k) {  // thread t: voxels 16 t .. 16 t + 15, in order
        fl[k] = B.flags[(size_t)slot * TSDF_VOX + 16 * t + k];
        c += __popc(fl[k]);
    }
    scan[t] = c;
    __syncthreads();
    for (int o = 1; o < TSDF_WG; o <<= 1) {  // inclusive scan
        const int add = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    size_t out = (size_t)B.offsets[blockIdx.x] + (scan[t] - c);
    for (int k = 0; k < 16; ++k) {
        if (!fl[k]) continue;
        const int vi = 16 * t + k, x = vi & 15, y = (vi >> 4) & 15, z = vi >> 8;
        const size_t g0 = (size_t)slot * TSDF_VOX + vi;
        const double f0 = fabs((double)B.tsdf[g0]);
        for (int a = 0; a < 3; ++a) {
            if (!(fl[k] & (1u << a))) continue;
            int q[3] = {x, y, z};
            long long nbk[3] = {bx, by, bz};
            q[a] += 1;
            int s1 = slot;
            if (q[a] == TSDF_B) {
                q[a] = 0;
                nbk[a] += 1;
                s1 = tsdf_find(B, tsdf_key(nbk[0], nbk[1], nbk[2]));  // exists: a valid cube flagged the edge
            }
            const size_t g1 = (size_t)s1 * TSDF_VOX + q[0] + 16 * q[1] + 256 * q[2];
            const double f1 = fabs((double)B.tsdf[g1]);
            double p[3] = {((double)(bx * TSDF_B + x) + 0.5) * voxel_length,
                           ((double)(by * TSDF_B + y) + 0.5) * voxel_length,
                           ((double)(bz * TSDF_B + z) + 0.5) * voxel_length};
            p[a] += f0 * voxel_length / (f0 + f1);
            for (int ch = 0; ch < 3; ++ch) {
                points[3 * out + ch] = p[ch];
                colours[3 * out + ch] =
                    (f1 * (double)B.colour[3 * g0 + ch] + f0 * (double)B.colour[3 * g1 + ch]) / (f0 + f1) / 255.0;
            }
            ++out;
        }
    }
}

// ------------------------------------------------------------------ launchers
static int tsdf_check_state(int max_blocks, const void *ws, size_t ws_bytes) {
    if (max_blocks < 1) return fail(PDSC_ERR_ARG, "max_blocks=%d (need >= 1)", max_blocks);
    if (max_blocks > TSDF_MAX_BLOCKS)
        return fail(PDSC_ERR_UNSUPPORTED, "max_blocks=%d (at most %d)", max_blocks, TSDF_MAX_BLOCKS);
    if (!ws) return fail(PDSC_ERR_ARG, "null pointer");
    return need_ws(ws_bytes, pdsc_tsdf_workspace_bytes(max_blocks));
}
static int tsdf_read_header(const TsdfBufs &B, TsdfHeader &h, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(&h, B.hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PDSC_OK;
}
// the call's single final synchronise: its status word
static int tsdf_status(const TsdfBufs &B, int max_blocks, hipStream_t s) {
    HIPCHK(hipGetLastError());
    TsdfHeader h;
    RET_IF(tsdf_read_header(B, h, s));
    if (h.status & TSDF_ERR_RANGE)
        return fail(PDSC_ERR_UNSUPPORTED, "a block index outside [-2^20, 2^20) (or a non-finite point)");
    if (h.status & TSDF_ERR_FULL)
        return fail(PDSC_ERR_UNSUPPORTED, "the volume is full: more than max_blocks=%d blocks", max_blocks);
    return PDSC_OK;
}
static void tsdf_alloc(const TsdfBufs &B, int max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(tsdf_alloc_kernel, dim3((B.hash_cap + TSDF_WG - 1) / TSDF_WG), dim3(TSDF_WG), 0, s, B, max_blocks);
    hipLaunchKernelGGL(tsdf_alloc_finish_kernel, dim3(1), dim3(1), 0, s, B, max_blocks);
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_tsdf_workspace_bytes(int32_t max_blocks) {
    if (max_blocks < 1 || max_blocks > TSDF_MAX_BLOCKS) return 0;
    Carve c(nullptr);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    return c.off;
}

int32_t pdsc_tsdf_reset(int32_t max_blocks, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    const size_t m = (size_t)max_blocks * TSDF_VOX;
    HIPCHK(hipMemsetAsync(B.tsdf, 0, m * sizeof(float), s));
    HIPCHK(hipMemsetAsync(B.weight, 0, m * sizeof(float), s));
    HIPCHK(hipMemsetAsync(B.colour, 0, 3 * m * sizeof(float), s));
    const int n = B.hash_cap > max_blocks ? B.hash_cap : max_blocks;
    hipLaunchKernelGGL(tsdf_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, s, B, max_blocks);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

int32_t pdsc_tsdf_integrate(const float *depth, const uint8_t *colour, int32_t H, int32_t W, double fx, double fy,
                            double cx, double cy, const double *extrinsic, double voxel_length, double sdf_trunc,
                            int32_t max_blocks, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (!depth || !colour || !extrinsic) return fail(PDSC_ERR_ARG, "null pointer");
    if (H < 1 || W < 1) return fail(PDSC_ERR_ARG, "H=%d W=%d (need >= 1)", H, W);
    const double k[4] = {fx, fy, cx, cy};
    for (double v : k)
        if (!(v > 0.0) || !std::isfinite(v))
            return fail(PDSC_ERR_ARG, "intrinsics fx=%g fy=%g cx=%g cy=%g must be > 0 and finite", fx, fy, cx, cy);
    if (!(voxel_length > 0.0) || !std::isfinite(voxel_length) || !(sdf_trunc > 0.0) || !std::isfinite(sdf_trunc))
        return fail(PDSC_ERR_ARG, "voxel_length %g / sdf_trunc %g must be > 0 and finite", voxel_length, sdf_trunc);
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    const TsdfCam C = {H, W, fx, fy, cx, cy};
    const int np = ((W + 3) / 4) * ((H + 3) / 4);
    hipLaunchKernelGGL(tsdf_begin_kernel, dim3(1), dim3(1), 0, s, B);
    hipLaunchKernelGGL(tsdf_touch_kernel, dim3((np + TSDF_WG - 1) / TSDF_WG), dim3(TSDF_WG), 0, s, B, depth, C, extrinsic,
                       voxel_length * TSDF_B, sdf_trunc);
    tsdf_alloc(B, max_blocks, s);
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(max_blocks < 8192 ? max_blocks : 8192), dim3(TSDF_WG), 0, s, B, depth,
                       colour, C, extrinsic, voxel_length, sdf_trunc);
    return tsdf_status(B, max_blocks, s);
}

int32_t pdsc_tsdf_read_blocks(int32_t max_blocks, int32_t capacity, int32_t *coords, float *tsdf, float *weight,
                              float *colour, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    if (capacity < 0) return fail(PDSC_ERR_ARG, "capacity=%d", capacity);
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    TsdfHeader h;
    RET_IF(tsdf_read_header(B, h, s));
    if (capacity < h.n_blocks) return fail(PDSC_ERR_ARG, "capacity=%d < %d blocks", capacity, h.n_blocks);
    if (h.n_blocks > 0)
        hipLaunchKernelGGL(tsdf_read_kernel, dim3(h.n_blocks), dim3(TSDF_WG), 0, s, B, h.n_blocks, coords, tsdf, weight,
                           colour);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

int32_t pdsc_tsdf_write_blocks(const int32_t *coords, int32_t n, const float *tsdf, const float *weight,
                               const float *colour, int32_t max_blocks, void *ws, size_t ws_bytes,
                               pdsc_stream_t stream) {
    if (n < 1) return fail(PDSC_ERR_ARG, "n=%d (need >= 1)", n);
    if (!coords || !tsdf || !weight || !colour) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    hipLaunchKernelGGL(tsdf_begin_kernel, dim3(1), dim3(1), 0, s, B);
    hipLaunchKernelGGL(tsdf_touch_list_kernel, dim3((n + 255) / 256), dim3(256), 0, s, B, coords, n);
    tsdf_alloc(B, max_blocks, s);
    hipLaunchKernelGGL(tsdf_write_kernel, dim3(n), dim3(TSDF_WG), 0, s, B, coords, tsdf, weight, colour);
    return tsdf_status(B, max_blocks, s);
}

int32_t pdsc_tsdf_count_surface_points(int32_t max_blocks, int64_t *n_points, void *ws, size_t ws_bytes,
                                       pdsc_stream_t stream) {
    if (!n_points) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    TsdfHeader h;
    RET_IF(tsdf_read_header(B, h, s));
    *n_points = 0;
    const int n = h.n_blocks;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(&B.hdr->n_points, 0, sizeof(int), s));
        return PDSC_OK;
    }
    size_t tb = B.cub_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(B.cub, tb, B.bkeys, B.skeys, B.iota, B.order, n, 0, 63, s));
    HIPCHK(hipMemsetAsync(B.flags, 0, (size_t)n * TSDF_VOX * sizeof(unsigned), s));
    hipLaunchKernelGGL(tsdf_mark_kernel, dim3(n), dim3(TSDF_WG), 0, s, B);
    hipLaunchKernelGGL(tsdf_count_kernel, dim3(n), dim3(TSDF_WG), 0, s, B, n);
    tb = B.cub_bytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(B.cub, tb, B.counts, B.offsets, n + 1, s));
    hipLaunchKernelGGL(tsdf_total_kernel, dim3(1), dim3(1), 0, s, B, n);
    HIPCHK(hipGetLastError());
    RET_IF(tsdf_read_header(B, h, s));
    *n_points = h.n_points;
    return PDSC_OK;
}

int32_t pdsc_tsdf_emit_surface_points(double voxel_length, int32_t max_blocks, double *points, double *colours,
                                      int64_t capacity, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (!(voxel_length > 0.0) || !std::isfinite(voxel_length))
        return fail(PDSC_ERR_ARG, "voxel_length %g must be > 0 and finite", voxel_length);
    if (!points || !colours) return fail(PDSC_ERR_ARG, "null pointer");
    if (capacity < 0) return fail(PDSC_ERR_ARG, "capacity=%lld", (long long)capacity);
    RET_IF(tsdf_check_state(max_blocks, ws, ws_bytes));
    hipStream_t s = S_(stream);
    Carve c(ws);
    TsdfBufs B;
    bind_tsdf(c, max_blocks, B);
    TsdfHeader h;
    RET_IF(tsdf_read_header(B, h, s));  // the one check that needs the device: the count of the last count pass
    if (capacity < h.n_points) return fail(PDSC_ERR_ARG, "capacity=%lld < %d points", (long long)capacity, h.n_points);
    if (h.n_points == 0) return PDSC_OK;
    hipLaunchKernelGGL(tsdf_emit_kernel, dim3(h.n_blocks), dim3(TSDF_WG), 0, s, B, voxel_length, points, colours);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
