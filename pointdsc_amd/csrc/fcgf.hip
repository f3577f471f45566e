// fcgf.hip -- FCGF descriptors on the GPU: misc/fcgf.py's ResUNetBN2C(1, C_out,
// conv1_kernel_size 5 | 7, normalize_feature) in eval mode, the sparse 3-D
// ResUNet that demo_registration.py:11-35, misc/cal_fcgf.py:12-85 and
// datasets/LidarFeatureExtractor.py:166-200 run through MinkowskiEngine.
// MinkowskiEngine is not a dependency: its published semantics are restated
// (include/pdsc.h f8 fixes every choice), parity with it is unpinned.
//
//   keys      (batch, x, y, z) packed into one 64-bit word, x most significant
//             below the batch, each coordinate offset by 2^18 so that negative
//             voxels sort below positive ones and floor(c / s) s for s = 2, 4, 8
//             is a mask of the packed word
//   quantise  floor(xyz / voxel) in fp32 (IEEE divide), stable radix sort of
//             (key, index), run-length encode: the first point of every run is
//             the voxel's lowest input index
//   levels    tensor strides 1, 2, 4, 8: the masked level-1 keys, sorted and
//             made unique (hipCUB); no hash table, no atomics
//   maps      nbr[k][u] in {-1, row} by binary search in the sorted keys; a
//             transposed convolution reads the stride-2 map backwards
//   conv      output-stationary: one wave owns 32 output rows x up to 128
//             output channels, walks the offsets k ascending, skips an offset
//             none of its rows has (wave-uniform), gathers the input rows
//             straight into the A operand of the exact fp32 MFMA (32x32x2),
//             sums each offset's products apart before adding them to the total, and
//             applies folded BN, residual, ReLU (and the final L2 norm) in the
//             epilogue.  No scatter, fixed summation order: bitwise reproducible
//             and independent of what else is in the batch.
//   conv1     C_in = 1: one wave per voxel, sum of W[k][:] f[u + o_k]
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

#include "abi.hpp"
#include "pdsc_common.hpp"

namespace pdsc {
namespace fcgf {

typedef unsigned long long u64;
constexpr int CB = 19;                 // bits per coordinate
constexpr int COFF = 1 << (CB - 1);    // coordinate offset: c in [-2^18, 2^18)
constexpr int CMASK = (1 << CB) - 1;
constexpr int BATCH_MAX = 64;          // 6 bits above the coordinates: 63-bit keys
constexpr int KEY_BITS_ALL = 3 * CB + 6;
constexpr int NLAYER = 23;

// ---- the one kernel-offset order: k = (ox + r) + K (oy + r) + K^2 (oz + r)
__host__ __device__ inline int fcgf_kernel_index(int ox, int oy, int oz, int K) {
    const int r = K >> 1;
    return (ox + r) + K * ((oy + r) + K * (oz + r));
}
// Where a checkpoint's kernel tensor [K^3, C_in, C_out] keeps the weights of
// offset (ox, oy, oz).  MinkowskiEngine is absent, so its order is unpinned and
// taken to be the same; if it differs, this function is the one to change.
__host__ __device__ inline int fcgf_checkpoint_index(int ox, int oy, int oz, int K) {
    return fcgf_kernel_index(ox, oy, oz, K);
}

PDSC_DEV u64 pack(int b, int x, int y, int z) {  // offset coordinates in [0, 2^19)
    return ((u64)b << (3 * CB)) | ((u64)x << (2 * CB)) | ((u64)y << CB) | (u64)z;
}
PDSC_DEV void unpack(u64 k, int &b, int &x, int &y, int &z) {
    z = (int)(k & CMASK), y = (int)((k >> CB) & CMASK), x = (int)((k >> (2 * CB)) & CMASK), b = (int)(k >> (3 * CB));
}
PDSC_DEV int find_key(const u64 *__restrict__ keys, int n, u64 k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && keys[lo] == k) ? lo : -1;
}
// the key of (b, x + dx, y + dy, z + dz), or false outside the packed range
PDSC_DEV bool shifted_key(u64 k, int dx, int dy, int dz, u64 &out) {
    int b, x, y, z;
    unpack(k, b, x, y, z);
    x += dx, y += dy, z += dz;
    if ((unsigned)x > (unsigned)CMASK || (unsigned)y > (unsigned)CMASK || (unsigned)z > (unsigned)CMASK) return false;
    out = pack(b, x, y, z);
    return true;
}

// --------------------------------------------------------------- the network
struct Layer {
    int K, cin, cout, bn, bias;  // kernel size per axis, channels, has BN, has bias
    size_t src, dst;             // float offsets in the flat parameters / the packed buffer
};
inline int pad32(int c) { return (c + 31) & ~31; }

// ResUNet2.__init__ (misc/fcgf.py:630-798) with BN2C's CHANNELS / TR_CHANNELS, in state-dict order
static void layers(int ks, int cout, Layer L[NLAYER], size_t *src_floats, size_t *dst_floats) {
    const int spec[NLAYER][3] = {{ks, 1, 32},   {3, 32, 32},   {3, 32, 32},   {3, 32, 64},   {3, 64, 64},  {3, 64, 64},
                                 {3, 64, 128},  {3, 128, 128}, {3, 128, 128}, {3, 128, 256}, {3, 256, 256}, {3, 256, 256},
                                 {3, 256, 128}, {3, 128, 128}, {3, 128, 128}, {3, 256, 64},  {3, 64, 64},  {3, 64, 64},
                                 {3, 128, 64},  {3, 64, 64},   {3, 64, 64},   {1, 96, 64},   {1, 64, cout}};
    size_t s = 0, d = 0;
    for (int i = 0; i < NLAYER; ++i) {
        Layer &l = L[i];
        l.K = spec[i][0], l.cin = spec[i][1], l.cout = spec[i][2];
        l.bn = i < 21, l.bias = i == 22;
        l.src = s, l.dst = d;
        const size_t k3 = (size_t)l.K * l.K * l.K;
        s += k3 * l.cin * l.cout + (l.bn ? 4 * l.cout : 0) + (l.bias ? l.cout : 0);
        d += k3 * l.cin * pad32(l.cout) + 2 * pad32(l.cout);  // W, scale, shift
    }
    *src_floats = s, *dst_floats = d;
}

// Packed layout of a layer: W as [K^3][C_in / 8][C_out padded to 32][8] (conv1,
// C_in = 1: [K^3][32]) -- the 8 floats are input channels 8 j .. 8 j + 7, so lane
// (h, col) of the MFMA reads its 4 B operands of k-step group j as one 16-byte
// load --, then scale [C_out pad] and shift [C_out pad]: BatchNorm1d(eps 1e-5)
// in eval mode folded (scale = w / sqrt(var + eps), shift = b - mean scale), or
// (1, bias | 0) for the layers without a norm; padded columns are (0, 0, 0).
__global__ void pack_layer_kernel(const float *__restrict__ src, float *__restrict__ dst, int K, int cin, int cout,
                                  int bn, int bias) {
    const int cp = (cout + 31) & ~31, k3 = K * K * K;
    const size_t nw = (size_t)k3 * cin * cp;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        int k, ci, co;
        if (cin == 1) {
            co = (int)(i % cp), k = (int)(i / cp), ci = 0;
        } else {
            const int e = (int)(i & 7);
            size_t t = i >> 3;
            co = (int)(t % cp), t /= cp;
            const int j = (int)(t % (cin / 8));
            k = (int)(t / (cin / 8)), ci = 8 * j + e;
        }
        const int r = K >> 1, ox = k % K - r, oy = (k / K) % K - r, oz = k / (K * K) - r;  // k = fcgf_kernel_index(o)
        dst[i] = co < cout ? src[((size_t)fcgf_checkpoint_index(ox, oy, oz, K) * cin + ci) * cout + co] : 0.0f;
    } else if (i < nw + cp) {
        const int c = (int)(i - nw);
        const float *p = src + (size_t)k3 * cin * cout;
        float sc = 0.0f, sh = 0.0f;
        if (c < cout) {
            if (bn) {  // weight, bias, running_mean, running_var
                sc = p[c] / sqrtf(p[3 * cout + c] + 1e-5f);
                sh = p[cout + c] - p[2 * cout + c] * sc;
            } else {
                sc = 1.0f;
                sh = bias ? p[c] : 0.0f;
            }
        }
        dst[nw + c] = sc;
        dst[nw + cp + c] = sh;
    }
}

// ------------------------------------------------------------------ quantise
// coords = floor(xyz / voxel) in fp32; err[0]: a coordinate outside the key range (or not finite)
__global__ void quantize_key_kernel(const float *__restrict__ xyz, int n, float voxel, const int *__restrict__ offsets,
                                    int batch, u64 *__restrict__ key, int *__restrict__ idx, int *__restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int b = 0;
    if (offsets) {  // the last b with offsets[b] <= i
        int lo = 0, hi = batch;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= i)
                lo = mid;
            else
                hi = mid;
        }
        b = lo;
    }
    int c[3];
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
        const float q = floorf(xyz[3 * (size_t)i + a] / voxel);
        if (!(q >= (float)-COFF && q < (float)COFF)) {
            ok = false;
            c[a] = 0;
        } else {
            c[a] = (int)q + COFF;
        }
    }
    if (!ok) err[0] = 1;
    key[i] = pack(b, c[0], c[1], c[2]);
    idx[i] = i;
}

__global__ void quantize_emit_kernel(const u64 *__restrict__ ukey, const int *__restrict__ ustart,
                                     const int *__restrict__ sidx, const int *__restrict__ nruns,
                                     int *__restrict__ inds, int *__restrict__ coords, int *__restrict__ count) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int nr = *nruns;
    if (v == 0) count[0] = nr;
    if (v >= nr) return;
    inds[v] = sidx[ustart[v]];  // stable sort: the run's first entry is its lowest input index
    int b, x, y, z;
    unpack(ukey[v], b, x, y, z);
    coords[4 * (size_t)v] = b, coords[4 * (size_t)v + 1] = x - COFF, coords[4 * (size_t)v + 2] = y - COFF,
                       coords[4 * (size_t)v + 3] = z - COFF;
}

// ----------------------------------------------------------- keys and levels
__global__ void coords_key_kernel(const int *__restrict__ coords, int m, u64 *__restrict__ key, int *__restrict__ idx,
                                  int *__restrict__ err, int *__restrict__ n1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    if (i == 0) n1[0] = m;
    const int b = coords[4 * (size_t)i];
    int c[3];
    bool ok = b >= 0 && b < BATCH_MAX;
    for (int a = 0; a < 3; ++a) {
        const int q = coords[4 * (size_t)i + 1 + a];
        ok = ok && q >= -COFF && q < COFF;
        c[a] = q + COFF;
    }
    if (!ok) {
        err[0] = 1;
        key[i] = 0;
    } else {
        key[i] = pack(b, c[0], c[1], c[2]);
    }
    idx[i] = i;
}

// floor(c / s) s per axis = clearing the low log2(s) bits of each (offset) coordinate
__global__ void coarse_key_kernel(const u64 *__restrict__ skey, int m, int shift, u64 *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const u64 low = (u64)((1 << shift) - 1);
    out[i] = skey[i] & ~(low | (low << CB) | (low << (2 * CB)));
}

__global__ void level_coords_kernel(const u64 *__restrict__ ukey, const int *__restrict__ n, int *__restrict__ coords) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= *n) return;
    int b, x, y, z;
    unpack(ukey[v], b, x, y, z);
    coords[4 * (size_t)v] = b, coords[4 * (size_t)v + 1] = x - COFF, coords[4 * (size_t)v + 2] = y - COFF,
                       coords[4 * (size_t)v + 3] = z - COFF;
}

// table[k][col(u)] = the row of source voxel c_u + sign o_k step (3^3 offsets), -1
// if absent or (align != 0) not a multiple of align + 1 on some axis.  qmap / smap:
// sorted position -> feature row (level 1: the caller's row order), or null.
__global__ void kernel_map_kernel(const u64 *__restrict__ qkey, const int *__restrict__ nq, const int *__restrict__ qmap,
                                  const u64 *__restrict__ skey, const int *__restrict__ ns, const int *__restrict__ smap,
                                  int step, int sign, int align, int *__restrict__ table, int ld) {
    const int u = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (u >= *nq) return;
    const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;  // k = fcgf_kernel_index(o, 3)
    u64 t;
    int row = -1;
    if (shifted_key(qkey[u], sign * ox * step, sign * oy * step, sign * oz * step, t)) {
        int b, x, y, z;
        unpack(t, b, x, y, z);
        if (((x | y | z) & align) == 0) {
            const int p = find_key(skey, *ns, t);
            if (p >= 0) row = smap ? smap[p] : p;
        }
    }
    table[(size_t)k * ld + (qmap ? qmap[u] : u)] = row;
}

// ------------------------------------------------------------------- conv1
// C_in = 1, K^3 = 125 | 343, 32 output channels: one wave per voxel.  The lanes
// look the offsets up (f = the neighbour's input feature, 0 if absent), then
// lane (h, c) sums W[k][c] f[k] over its half of the offsets in ascending k and
// the halves are added, low half first.
constexpr int C1_WPB = 4;
__global__ __launch_bounds__(C1_WPB * 64) void conv1_kernel(const u64 *__restrict__ skey, const int *__restrict__ sidx,
                                                            int m, const float *__restrict__ feats, int K,
                                                            const float *__restrict__ w, float *__restrict__ out) {
    __shared__ float fk[C1_WPB][344];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * C1_WPB + wave;
    if (p >= m) return;  // wave-uniform; no workgroup barrier below
    const int k3 = K * K * K, r = K >> 1;
    const u64 key = skey[p];
    for (int k = lane; k < k3; k += 64) {
        const int ox = k % K - r, oy = (k / K) % K - r, oz = k / (K * K) - r;  // k = fcgf_kernel_index(o, K)
        u64 t;
        float f = 0.0f;
        if (shifted_key(key, ox, oy, oz, t)) {
            const int q = find_key(skey, m, t);
            if (q >= 0) f = feats ? feats[sidx[q]] : 1.0f;
        }
        fk[wave][k] = f;
    }
    __builtin_amdgcn_wave_barrier();
    const int c = lane & 31, h = lane >> 5, half = k3 >> 1;
    float acc = 0.0f;
    for (int k = h ? half : 0; k < (h ? k3 : half); ++k) acc += w[k * 32 + c] * fk[wave][k];
    const float other = __shfl_xor(acc, 32);
    const float sum = h ? other + acc : acc + other;
    if (h == 0) out[(size_t)sidx[p] * 32 + c] = sum * w[k3 * 32 + c] + w[k3 * 32 + 32 + c];
}

// ------------------------------------------------------------- sparse conv
struct ConvArgs {
    const float *in;    // [rows][ldin]
    const int *nbr;     // [K3][ldn] rows of `in`, -1 = absent; null: the row itself (1x1)
    const int *n;       // device: output rows
    const float *w;     // packed layer
    const float *res;   // [n][ldres] added before the ReLU, or null
    float *out;         // [n][ldout]
    int ldin, ldn, K3, cin8, cp, cout, ldres, ldout, relu, normalize;
};

template <int NT> __global__ __launch_bounds__(256) void sparse_conv_kernel(ConvArgs a) {
    const int lane = threadIdx.x & 63, rr = lane & 31, h = lane >> 5;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    const int n = *a.n;
    if (row0 >= n) return;  // wave-uniform; the waves of a workgroup share nothing
    const int col0 = blockIdx.y * NT * 32;
    const int row = row0 + rr;
    const bool valid = row < n;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero16();
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < a.K3; ++k) {
        const int r = valid ? (a.nbr ? a.nbr[(size_t)k * a.ldn + row] : row) : -1;
        if (__ballot(r >= 0) == 0) continue;  // none of the 32 rows has this offset
        const float *src = a.in + (size_t)(r < 0 ? 0 : r) * a.ldin + 4 * h;
        const float *wk = a.w + ((size_t)k * a.cin8 * a.cp + col0 + rr) * 8 + 4 * h;
        // two-level sum: the offset's C_in products in an accumulator of their own, then
        // added to the total -- one chain of 27 C_in fp32 additions would carry the
        // rounding of thousands of terms (measured: up to 3.6x the noise of a blocked sum)
        f32x16 part[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) part[t] = zero16();
        for (int j = 0; j < a.cin8; ++j) {
            const f32x4 x = r >= 0 ? *reinterpret_cast<const f32x4 *>(src + 8 * j) : zero4;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 wv = *reinterpret_cast<const f32x4 *>(wk + ((size_t)j * a.cp + 32 * t) * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) part[t] = mfma32(x[e], wv[e], part[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] += part[t];
    }
    const float *scale = a.w + (size_t)a.K3 * a.cin8 * 8 * a.cp, *shift = scale + a.cp;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = col0 + 32 * t + rr;
        const float sc = scale[col], sh = shift[col];  // col < cp: the padded columns are 0
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int orow = row0 + acc_row(q, h);
            const bool st = orow < n && col < a.cout;
            float y = acc[t][q] * sc + sh;
            if (a.res && st) y += a.res[(size_t)orow * a.ldres + col];
            if (a.relu) y = fmaxf(y, 0.0f);
            if (a.normalize) {  // F / (||F||_2 + 1e-8) (misc/fcgf.py:847): NT == 1, the row is this half-wave's 32 lanes
                float ss = col < a.cout ? y * y : 0.0f;
                for (int o = 16; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
                y = y / (sqrtf(ss) + 1e-8f);
            }
            if (st) a.out[(size_t)orow * a.ldout + col] = y;
        }
    }
}

// ------------------------------------------------------------------ workspace
struct Bufs {
    int *flags;                 // [0] range error, [1..4] rows per level (n1 = m), [5] quantise runs
    u64 *key, *skey1, *tmpkey, *ukey[4];  // ukey[0] = skey1
    int *idx, *sidx1, *cnt, *start;
    int *nbr[4], *down[3], *up[3];  // [27][m] each: stride-1 maps, L -> L+1 conv maps, L+1 -> L transposed maps
    float *a[4], *t[4], *u[3], *cat[3], *s4, *c1;
    void *cub;
    size_t cub_bytes;
};

static size_t cub_bytes(int n) {
    size_t b[4] = {0, 0, 0, 0};
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b[0], (const u64 *)nullptr, (u64 *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n, 0, KEY_BITS_ALL);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b[1], (const u64 *)nullptr, (u64 *)nullptr, n, 0, KEY_BITS_ALL);
    (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, b[2], (const u64 *)nullptr, (u64 *)nullptr, (int *)nullptr,
                                                (int *)nullptr, n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b[3], (const int *)nullptr, (int *)nullptr, n);
    return std::max(std::max(b[0], b[1]), std::max(b[2], b[3]));
}

static const int CH[4] = {32, 64, 128, 256};      // CHANNELS
static const int TR[3] = {64, 64, 128};           // TR_CHANNELS of the levels 1..3 (BN2C)

// every level is bounded by m rows (the worst case: no two voxels share a parent)
static void bind(Carve &c, int n, Bufs &W) {
    const size_t m = (size_t)std::max(n, 1);
    W.flags = c.take<int>(8);
    W.key = c.take<u64>(m), W.skey1 = c.take<u64>(m), W.tmpkey = c.take<u64>(m);
    W.ukey[0] = W.skey1;
    for (int l = 1; l < 4; ++l) W.ukey[l] = c.take<u64>(m);
    W.idx = c.take<int>(m), W.sidx1 = c.take<int>(m), W.cnt = c.take<int>(m), W.start = c.take<int>(m);
    for (int l = 0; l < 4; ++l) W.nbr[l] = c.take<int>(27 * m);
    for (int l = 0; l < 3; ++l) W.down[l] = c.take<int>(27 * m), W.up[l] = c.take<int>(27 * m);
    for (int l = 0; l < 4; ++l) W.a[l] = c.take<float>(m * CH[l]), W.t[l] = c.take<float>(m * std::max(CH[l], l < 3 ? TR[l] : 0));
    for (int l = 0; l < 3; ++l) W.u[l] = c.take<float>(m * TR[l]), W.cat[l] = c.take<float>(m * (TR[l] + CH[l]));
    W.s4 = c.take<float>(m * CH[3]);
    W.c1 = c.take<float>(m * 64);
    W.cub_bytes = cub_bytes(n);
    W.cub = c.take_bytes(W.cub_bytes);
}

static hipError_t launch_conv(const ConvArgs &a, int rows_cap, hipStream_t s) {
    const int nt = std::min(a.cp, 128) / 32;
    const dim3 grid((rows_cap + 127) / 128, a.cp / (32 * nt)), block(256);
    if (nt == 1)
        hipLaunchKernelGGL(sparse_conv_kernel<1>, grid, block, 0, s, a);
    else if (nt == 2)
        hipLaunchKernelGGL(sparse_conv_kernel<2>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(sparse_conv_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

static int check_net(int32_t ks, int32_t cout) {
    if (ks != 5 && ks != 7) return fail(PDSC_ERR_UNSUPPORTED, "conv1_kernel_size=%d not 5 or 7", ks);
    if (cout < 1 || cout > 32) return fail(PDSC_ERR_UNSUPPORTED, "out_channels=%d not in [1, 32]", cout);
    return PDSC_OK;
}

}  // namespace fcgf
}  // namespace pdsc

using namespace pdsc;
using namespace pdsc::fcgf;

extern "C" {

size_t pdsc_fcgf_param_floats(int32_t conv1_kernel_size, int32_t out_channels) {
    if (check_net(conv1_kernel_size, out_channels) != PDSC_OK) return 0;
    Layer L[NLAYER];
    size_t s, d;
    layers(conv1_kernel_size, out_channels, L, &s, &d);
    return s;
}

size_t pdsc_fcgf_packed_floats(int32_t conv1_kernel_size, int32_t out_channels) {
    if (check_net(conv1_kernel_size, out_channels) != PDSC_OK) return 0;
    Layer L[NLAYER];
    size_t s, d;
    layers(conv1_kernel_size, out_channels, L, &s, &d);
    return d;
}

int32_t pdsc_fcgf_pack_weights(const float *params, int32_t conv1_kernel_size, int32_t out_channels, float *packed,
                               pdsc_stream_t stream) {
    RET_IF(check_net(conv1_kernel_size, out_channels));
    if (!params || !packed) return fail(PDSC_ERR_ARG, "null pointer");
    Layer L[NLAYER];
    size_t s, d;
    layers(conv1_kernel_size, out_channels, L, &s, &d);
    for (int i = 0; i < NLAYER; ++i) {
        const Layer &l = L[i];
        const size_t total = (size_t)l.K * l.K * l.K * l.cin * pad32(l.cout) + pad32(l.cout);
        hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_(stream),
                           params + l.src, packed + l.dst, l.K, l.cin, l.cout, l.bn, l.bias);
    }
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

size_t pdsc_fcgf_workspace_bytes(int32_t n_points, int32_t batch, int32_t conv1_kernel_size, int32_t out_channels) {
    if (n_points < 1 || batch < 1 || batch > BATCH_MAX || check_net(conv1_kernel_size, out_channels) != PDSC_OK) return 0;
    Carve c(nullptr);
    Bufs W;
    bind(c, n_points, W);
    return c.off;
}

int32_t pdsc_fcgf_quantize(const float *xyz, int32_t n, const int32_t *batch_offsets, int32_t batch, float voxel_size,
                           int32_t *inds, int32_t *coords, int32_t *count, void *workspace, size_t workspace_bytes,
                           pdsc_stream_t stream) {
    if (!xyz || !inds || !coords || !count || !workspace) return fail(PDSC_ERR_ARG, "null pointer");
    if (n < 1) return fail(PDSC_ERR_ARG, "n=%d", n);
    if (batch < 1 || batch > BATCH_MAX) return fail(PDSC_ERR_UNSUPPORTED, "batch=%d not in [1, %d]", batch, BATCH_MAX);
    if (batch > 1 && !batch_offsets) return fail(PDSC_ERR_ARG, "batch=%d needs batch_offsets", batch);
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size))
        return fail(PDSC_ERR_ARG, "voxel size %g must be > 0", (double)voxel_size);
    RET_IF(need_ws(workspace_bytes, pdsc_fcgf_workspace_bytes(n, batch, 7, 32)));
    hipStream_t s = S_(stream);
    Carve c(workspace);
    Bufs W;
    bind(c, n, W);
    int *nruns = W.flags + 5;
    HIPCHK(hipMemsetAsync(W.flags, 0, 8 * sizeof(int), s));
    hipLaunchKernelGGL(quantize_key_kernel, dim3((n + 255) / 256), dim3(256), 0, s, xyz, n, voxel_size, batch_offsets,
                       batch, W.key, W.idx, W.flags);
    HIPCHK(hipGetLastError());
    size_t tb = W.cub_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(W.cub, tb, W.key, W.skey1, W.idx, W.sidx1, n, 0, KEY_BITS_ALL, s));
    tb = W.cub_bytes;
    HIPCHK(hipcub::DeviceRunLengthEncode::Encode(W.cub, tb, W.skey1, W.tmpkey, W.cnt, nruns, n, s));
    tb = W.cub_bytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(W.cub, tb, W.cnt, W.start, n, s));
    hipLaunchKernelGGL(quantize_emit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, W.tmpkey, W.start, W.sidx1, nruns,
                       inds, coords, count);
    HIPCHK(hipGetLastError());
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, W.flags, sizeof e, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (e) return fail(PDSC_ERR_UNSUPPORTED, "a voxel coordinate is outside [-2^18, 2^18) (or a point is not finite)");
    return PDSC_OK;
}

int32_t pdsc_fcgf_forward(const float *packed, int32_t conv1_kernel_size, int32_t out_channels, int32_t normalize,
                          const int32_t *coords, const float *feats, int32_t m, float *out,
                          const pdsc_fcgf_debug *debug, void *workspace, size_t workspace_bytes, pdsc_stream_t stream) {
    RET_IF(check_net(conv1_kernel_size, out_channels));
    if (!packed || !coords || !out || !workspace) return fail(PDSC_ERR_ARG, "null pointer");
    if (m < 1) return fail(PDSC_ERR_ARG, "m=%d", m);
    RET_IF(need_ws(workspace_bytes, pdsc_fcgf_workspace_bytes(m, 1, conv1_kernel_size, out_channels)));
    hipStream_t s = S_(stream);
    Carve cv(workspace);
    Bufs W;
    bind(cv, m, W);
    Layer L[NLAYER];
    size_t sf, df;
    layers(conv1_kernel_size, out_channels, L, &sf, &df);
    const dim3 rows((m + 255) / 256), b256(256);
    int *nl = W.flags + 1;  // rows per level

    // ---- keys, levels
    HIPCHK(hipMemsetAsync(W.flags, 0, 8 * sizeof(int), s));
    hipLaunchKernelGGL(coords_key_kernel, rows, b256, 0, s, coords, m, W.key, W.idx, W.flags, nl);
    HIPCHK(hipGetLastError());
    size_t tb = W.cub_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(W.cub, tb, W.key, W.skey1, W.idx, W.sidx1, m, 0, KEY_BITS_ALL, s));
    for (int l = 1; l < 4; ++l) {
        hipLaunchKernelGGL(coarse_key_kernel, rows, b256, 0, s, W.skey1, m, l, W.key);
        tb = W.cub_bytes;
        HIPCHK(hipcub::DeviceRadixSort::SortKeys(W.cub, tb, W.key, W.tmpkey, m, 0, KEY_BITS_ALL, s));
        tb = W.cub_bytes;
        HIPCHK(hipcub::DeviceRunLengthEncode::Encode(W.cub, tb, W.tmpkey, W.ukey[l], W.cnt, nl + l, m, s));
    }
    // ---- kernel maps (tensor stride of level l: 1 << l)
    const dim3 grid27((m + 255) / 256, 27);
    for (int l = 0; l < 4; ++l) {
        const int *map = l == 0 ? W.sidx1 : nullptr;
        hipLaunchKernelGGL(kernel_map_kernel, grid27, b256, 0, s, W.ukey[l], nl + l, map, W.ukey[l], nl + l, map, 1 << l,
                           1, 0, W.nbr[l], m);
    }
    for (int l = 0; l < 3; ++l) {
        const int *fine = l == 0 ? W.sidx1 : nullptr;
        hipLaunchKernelGGL(kernel_map_kernel, grid27, b256, 0, s, W.ukey[l + 1], nl + l + 1, (const int *)nullptr,
                           W.ukey[l], nl + l, fine, 1 << l, 1, 0, W.down[l], m);
        hipLaunchKernelGGL(kernel_map_kernel, grid27, b256, 0, s, W.ukey[l], nl + l, fine, W.ukey[l + 1], nl + l + 1,
                           (const int *)nullptr, 1 << l, -1, (2 << l) - 1, W.up[l], m);
    }
    HIPCHK(hipGetLastError());

    // ---- the network (ResUNet2.forward, misc/fcgf.py:800-851)
    auto conv = [&](int li, const float *in, int ldin, const int *nbr, int lvl, const float *res, int ldres, float *o,
                    int ldo, int relu, int norm = 0) {
        const Layer &l = L[li];
        ConvArgs a;
        a.in = in, a.nbr = nbr, a.n = nl + lvl, a.w = packed + l.dst, a.res = res, a.out = o;
        a.ldin = ldin, a.ldn = m, a.K3 = l.K * l.K * l.K, a.cin8 = l.cin / 8, a.cp = pad32(l.cout), a.cout = l.cout;
        a.ldres = ldres, a.ldout = ldo, a.relu = relu, a.normalize = norm;
        return launch_conv(a, m, s);
    };
    // BasicBlockBN (:142-158) at level lvl on x [.., ldx]: o = relu(bn2(conv2(relu(bn1(conv1(x))))) + x)
    auto block = [&](int li, int lvl, int C, const float *x, int ldx, float *o, int ldo) {
        hipError_t e = conv(li, x, ldx, W.nbr[lvl], lvl, nullptr, 0, W.t[lvl], C, 1);
        if (e != hipSuccess) return e;
        return conv(li + 1, W.t[lvl], C, W.nbr[lvl], lvl, x, ldx, o, ldo, 1);
    };
    hipLaunchKernelGGL(conv1_kernel, dim3((m + C1_WPB - 1) / C1_WPB), dim3(C1_WPB * 64), 0, s, W.skey1, W.sidx1, m, feats,
                       conv1_kernel_size, packed + L[0].dst, W.a[0]);
    HIPCHK(hipGetLastError());
    // encoder: out_sN lands in the skip columns of the level's concat buffer (the
    // ReLU after a block, :804, is the identity on a block's output)
    float *s1 = W.cat[0] + 64, *s2 = W.cat[1] + 64, *s3 = W.cat[2] + 128;
    HIPCHK(block(1, 0, 32, W.a[0], 32, s1, 96));
    HIPCHK(conv(3, s1, 96, W.down[0], 1, nullptr, 0, W.a[1], 64, 0));
    HIPCHK(block(4, 1, 64, W.a[1], 64, s2, 128));
    HIPCHK(conv(6, s2, 128, W.down[1], 2, nullptr, 0, W.a[2], 128, 0));
    HIPCHK(block(7, 2, 128, W.a[2], 128, s3, 256));
    HIPCHK(conv(9, s3, 256, W.down[2], 3, nullptr, 0, W.a[3], 256, 0));
    HIPCHK(block(10, 3, 256, W.a[3], 256, W.s4, 256));
    // decoder: ME.cat(upsampled, skip)
    HIPCHK(conv(12, W.s4, 256, W.up[2], 2, nullptr, 0, W.u[2], 128, 0));
    HIPCHK(block(13, 2, 128, W.u[2], 128, W.cat[2], 256));
    HIPCHK(conv(15, W.cat[2], 256, W.up[1], 1, nullptr, 0, W.u[1], 64, 0));
    HIPCHK(block(16, 1, 64, W.u[1], 64, W.cat[1], 128));
    HIPCHK(conv(18, W.cat[1], 128, W.up[0], 0, nullptr, 0, W.u[0], 64, 0));
    HIPCHK(block(19, 0, 64, W.u[0], 64, W.cat[0], 96));
    HIPCHK(conv(21, W.cat[0], 96, nullptr, 0, nullptr, 0, W.c1, 64, 1));
    HIPCHK(conv(22, W.c1, 64, nullptr, 0, nullptr, 0, out, out_channels, 0, normalize != 0));

    if (debug) {
        auto tap = [&](float *dst, const float *src, int ld, int C) {
            if (!dst) return hipSuccess;
            return hipMemcpy2DAsync(dst, (size_t)C * 4, src, (size_t)ld * 4, (size_t)C * 4, m, hipMemcpyDeviceToDevice, s);
        };
        HIPCHK(tap(debug->block1, s1, 96, 32));
        HIPCHK(tap(debug->block2, s2, 128, 64));
        HIPCHK(tap(debug->block3, s3, 256, 128));
        HIPCHK(tap(debug->block4, W.s4, 256, 256));
        HIPCHK(tap(debug->block4_tr, W.cat[2], 256, 128));
        HIPCHK(tap(debug->block3_tr, W.cat[1], 128, 64));
        HIPCHK(tap(debug->block2_tr, W.cat[0], 96, 64));
        HIPCHK(tap(debug->conv1_tr, W.c1, 64, 64));
        int *lc[3] = {debug->coords2, debug->coords4, debug->coords8};
        for (int l = 1; l < 4; ++l)
            if (lc[l - 1]) hipLaunchKernelGGL(level_coords_kernel, rows, b256, 0, s, W.ukey[l], nl + l, lc[l - 1]);
        HIPCHK(hipGetLastError());
        if (debug->counts) HIPCHK(hipMemcpyAsync(debug->counts, nl, 4 * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, W.flags, sizeof e, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (e) return fail(PDSC_ERR_UNSUPPORTED, "a coordinate is outside [-2^18, 2^18) or a batch index outside [0, %d)", BATCH_MAX);
    return PDSC_OK;
}

}  // extern "C"
