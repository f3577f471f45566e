// sm_loss_fused.hip -- training: the spectral-matching loss on the normalised
// features themselves, with its gradients, in one pass that never stores an
// N x N tensor (DESIGN.md §7 "Training").
//
//   s_ij = n_i.n_j    u_ij = 1 - (1 - s_ij) / sigma^2    M_ij = clamp(u_ij, 0, 1), M_ii = 0
//   gt_ij = (l_i == 1 and l_j == 1 and i != j)             e_ij = M_ij - gt_ij
//   L = sum_b 0.5 (cP_b sum_gt e^2 + cQ_b sum_!gt e^2)
//       balanced: cP_b = 1 / (B P_b), cQ_b = 1 / (B Q_b), P_b = max(k_b (k_b - 1) - 1, 0) + 1,
//                 Q_b = max(N^2 - k_b (k_b - 1) - 1, 0) + 1, k_b = #{l_i == 1}
//       MSE:      cP_b = cQ_b = 2 / (B N^2)
//   G_ij = dL/du_ij = e_ij (gt ? cP_b : cQ_b) where 0 <= u_ij <= 1 and i != j, else 0
//   dL/dn_i = (2 / sigma^2) sum_j G_ij n_j     dL/dsigma = (2 / sigma^3) sum_ij G_ij (1 - s_ij)
//
//   sm_fused_coef   k_b and (cP_b, cQ_b), one wavefront per pair
//   sm_fused        attn_bwd_q's loop without the softmax (bwd_tile.hpp): a
//                   workgroup = 4 waves x 32 rows n_i in registers and a range of
//                   32-row tiles of n_j staged in LDS; S^T = n_j n_i^T on
//                   v_mfma_f32_32x32x2_f32 (accumulator row <-> j, lane <-> i), G in
//                   registers, dn_i += G n_j; the tile's terms of sum e^2 and of
//                   sum e (1 - s), split by gt, go into fp64 per-lane sums.  <false>:
//                   the loss alone (no second product, no gradient sums).
//   sm_fused_sum    when a pair's tiles are split over workgroups, the partials
//                   [B][split][N][CH] are added in split order
//   sm_fused_final  the fp64 partials [B][rowblock][split][4] in a fixed order -> loss, dsigma
// No atomics and no order that depends on scheduling: two calls are bit-equal.
#include "abi.hpp"
#include "bwd_tile.hpp"

namespace pdsc {

constexpr int SMF_MAX_SPLIT = 8;  // bounds the partials to 8 x [B][N][CH] floats

__global__ __launch_bounds__(64) void sm_fused_coef_kernel(const float *__restrict__ labels, int B, int N, int balanced,
                                                           double *__restrict__ coef) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int k = 0;
    for (int i = lane; i < N; i += 64) k += labels[(size_t)b * N + i] == 1.0f;
    k = wave_sum(k);
    if (lane != 0) return;
    const double nn = (double)N * N, np = (double)k * (k - 1);
    if (balanced) {
        coef[2 * b] = 1.0 / ((double)B * (fmax(np - 1.0, 0.0) + 1.0));
        coef[2 * b + 1] = 1.0 / ((double)B * (fmax(nn - np - 1.0, 0.0) + 1.0));
    } else {
        coef[2 * b] = coef[2 * b + 1] = 2.0 / ((double)B * nn);
    }
}

// The streamed tile of one [.][CH] array: 32 rows through registers into LDS
// (stride BW_STR), rows >= N as zeros; 256 threads, 4 float4 each.
PDSC_DEV void tile_load1(const float *__restrict__ x, int row0, int N, int tid, f32x4 t[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = row0 + (idx >> 5), c4 = idx & 31;
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        t[i] = row < N ? *reinterpret_cast<const f32x4 *>(x + (size_t)row * CH + 4 * c4) : z;
    }
}
PDSC_DEV void tile_store1(float *l, int tid, const f32x4 t[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 5, c4 = idx & 31;
        *reinterpret_cast<f32x4 *>(l + row * BW_STR + 4 * c4) = t[i];
    }
}

// O (as store_rows takes it) -> rows of out, each value scaled in fp64
PDSC_DEV void store_rows_scaled(float *__restrict__ out, int row0, int N, int h, int l32, double sc, const f32x16 &O0,
                                const f32x16 &O1, const f32x16 &O2, const f32x16 &O3) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + acc_row(r, h);
        if (row < N)
            *reinterpret_cast<f32x4 *>(out + (size_t)row * CH + 4 * l32) =
                f32x4{(float)(sc * O0[r]), (float)(sc * O1[r]), (float)(sc * O2[r]), (float)(sc * O3[r])};
    }
}

// 128 rows i of pair b over the tiles j in [split * tps, ...): part
// [B][nblk][nsplit][4] = sum_gt e^2, sum_!gt e^2, sum_gt e (1 - s), sum_!gt e (1 - s)
// (the last two over the clamp's open range only); GRAD: dnp [B][nsplit][N][CH],
// unscaled sums G n_j when nsplit > 1, else dL/dn itself.
template <bool GRAD>
__global__ __launch_bounds__(256) void sm_fused_kernel(const float *__restrict__ normed,
                                                       const float *__restrict__ sigma_p,
                                                       const float *__restrict__ labels,
                                                       const double *__restrict__ coef, BwdGrid g,
                                                       float *__restrict__ dnp, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Nl[BW_T * BW_STR];
    __shared__ float Ll[BW_T];
    __shared__ double red[BW_NW][4];
    const int N = g.N;
    const int split = blockIdx.x % g.nsplit, blk = (blockIdx.x / g.nsplit) % g.nblk, b = blockIdx.x / g.nsplit / g.nblk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int i0 = blk * BW_ROWS + wave * BW_T, qi = i0 + l32;
    const bool active = i0 < N;  // wave-uniform
    const int nt = (N + BW_T - 1) / BW_T;
    const int t0 = split * g.tps, t1 = min(nt, t0 + g.tps);
    const float *nb = normed + (size_t)b * N * CH, *lb = labels + (size_t)b * N;
    const float sig = sigma_p[0];
    const float sig2 = sig * sig;  // self.sigma ** 2 (a tensor: fp32), as feat_sim_kernel
    const float cP = (float)coef[2 * b], cQ = (float)coef[2 * b + 1];

    float nf[64];
    load_rows64(nb, qi, N, h, nf);
    const bool li = qi < N && lb[qi] == 1.0f;
    f32x16 dN0 = zero16(), dN1 = zero16(), dN2 = zero16(), dN3 = zero16();
    double sP = 0.0, sN = 0.0, gP = 0.0, gN = 0.0;

    f32x4 tr[4];
    float tl = 0.0f;  // threads 0..31: the tile's labels
    auto load = [&](int t) {
        tile_load1(nb, t * BW_T, N, tid, tr);
        if (tid < BW_T) {
            const int row = t * BW_T + tid;
            tl = row < N ? lb[row] : 0.0f;
        }
    };
    auto store = [&]() {
        tile_store1(Nl, tid, tr);
        if (tid < BW_T) Ll[tid] = tl;
    };
    if (t0 < t1) {
        load(t0);
        store();
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) load(t + 1);
        if (active) {
            const int j0 = t * BW_T;
            const f32x16 St = dot_lds_reg(Nl, nf, h, l32);
            float w[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ar = acc_row(r, h), j = j0 + ar;
                const bool in = j < N && qi < N && j != qi;  // tails and the diagonal contribute nothing
                const bool gt = li && Ll[ar] == 1.0f;
                const float d = 1.0f - St[r];
                const float u = 1.0f - d / sig2;
                const float m = fminf(fmaxf(u, 0.0f), 1.0f);
                const float e = gt ? m - 1.0f : m;
                const double e2 = in ? (double)e * (double)e : 0.0;
                sP += gt ? e2 : 0.0;
                sN += gt ? 0.0 : e2;
                if constexpr (GRAD) {
                    const bool live = in && u >= 0.0f && u <= 1.0f;  // torch.clamp's backward: inclusive
                    w[r] = live ? e * (gt ? cP : cQ) : 0.0f;
                    const double ed = live ? (double)e * (double)d : 0.0;
                    gP += gt ? ed : 0.0;
                    gN += gt ? 0.0 : ed;
                }
            }
            if constexpr (GRAD) accum_rows(w, Nl, h, l32, dN0, dN1, dN2, dN3);
        }
        __syncthreads();
        if (t + 1 < t1) store();
        __syncthreads();
    }
    sP = wave_sum(sP);
    sN = wave_sum(sN);
    if constexpr (GRAD) {
        gP = wave_sum(gP);
        gN = wave_sum(gN);
    }
    if (lane == 0) {
        red[wave][0] = sP;
        red[wave][1] = sN;
        red[wave][2] = gP;
        red[wave][3] = gN;
    }
    __syncthreads();
    if (tid < 4) {
        double a = red[0][tid];
        for (int wv = 1; wv < BW_NW; ++wv) a += red[wv][tid];
        part[(((size_t)b * g.nblk + blk) * g.nsplit + split) * 4 + tid] = a;
    }
    if constexpr (GRAD) {
        if (!active) return;
        float *out = dnp + ((size_t)b * g.nsplit + split) * N * CH;
        if (g.nsplit > 1)
            store_rows(out, i0, N, h, l32, dN0, dN1, dN2, dN3);
        else
            store_rows_scaled(out, i0, N, h, l32, 2.0 / ((double)sig * (double)sig), dN0, dN1, dN2, dN3);
    }
}

// dnormed [B][n] = (2 / sigma^2) sum over s (ascending, in fp64) of part [B][nsplit][n], n = N * CH, 4 per thread
__global__ void sm_fused_sum_kernel(const float *__restrict__ part, const float *__restrict__ sigma_p, int B, size_t n4,
                                    int nsplit, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * n4) return;
    const size_t b = i / n4, e = i % n4;
    const f32x4 *p = reinterpret_cast<const f32x4 *>(part) + b * nsplit * n4 + e;
    const double sig = sigma_p[0], sc = 2.0 / (sig * sig);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int s = 0; s < nsplit; ++s) {
        const f32x4 v = p[(size_t)s * n4];
        a0 += v[0];
        a1 += v[1];
        a2 += v[2];
        a3 += v[3];
    }
    reinterpret_cast<f32x4 *>(out)[i] = f32x4{(float)(sc * a0), (float)(sc * a1), (float)(sc * a2), (float)(sc * a3)};
}

// One wavefront: per pair, the partials lane-strided and a butterfly (fixed order), then
// loss = sum_b 0.5 (cP sP + cQ sN) and dsigma = (2 / sigma^3) sum_b (cP gP + cQ gN).
__global__ __launch_bounds__(64) void sm_fused_final_kernel(const double *__restrict__ part,
                                                            const double *__restrict__ coef,
                                                            const float *__restrict__ sigma_p, int B, int per_pair,
                                                            double *__restrict__ loss, double *__restrict__ dsigma) {
    const int lane = threadIdx.x;
    double total = 0.0, dsg = 0.0;
    for (int b = 0; b < B; ++b) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = lane; e < per_pair; e += 64) {
            const double *o = part + ((size_t)b * per_pair + e) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] += o[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = wave_sum(a[k]);
        const double cP = coef[2 * b], cQ = coef[2 * b + 1];
        total += 0.5 * (cP * a[0] + cQ * a[1]);
        dsg += cP * a[2] + cQ * a[3];
    }
    if (lane != 0) return;
    loss[0] = total;
    const double sig = sigma_p[0];
    if (dsigma) dsigma[0] = 2.0 / (sig * sig * sig) * dsg;
}

inline BwdGrid smf_grid(int B, int N) { return bwd_grid(B, N, SMF_MAX_SPLIT); }

// pdsc_sm_loss_fused_f32's workspace: the coefficients, the fp64 partials, and
// the gradient partials when the tiles are split
struct SmfBufs {
    double *coef, *part;
    float *dn;
};
static SmfBufs bind_smf(Carve &c, const BwdGrid &g) {
    SmfBufs a;
    a.coef = c.take<double>((size_t)g.B * 2);
    a.part = c.take<double>((size_t)g.B * g.nblk * g.nsplit * 4);
    a.dn = c.take<float>(g.nsplit > 1 ? (size_t)g.B * g.nsplit * g.N * CH : 0);
    return a;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_sm_loss_fused_workspace_bytes(int32_t B, int32_t N, int32_t C) {
    if (C != CH || B < 1 || N < 1) return 0;
    Carve c(nullptr);
    bind_smf(c, smf_grid(B, N));
    return c.off;
}

int32_t pdsc_sm_loss_fused_f32(const float *normed, const float *sigma, const float *gt_labels, int32_t B, int32_t N,
                               int32_t C, int32_t balanced, double *loss, float *dnormed, double *dsigma, void *ws,
                               size_t ws_bytes, pdsc_stream_t stream) {
    if (!normed || !sigma || !gt_labels || !loss || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || N < 1) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    if ((dnormed == nullptr) != (dsigma == nullptr))
        return fail(PDSC_ERR_ARG, "dnormed and dsigma: both or neither (null: the loss alone)");
    if (C != CH) return fail(PDSC_ERR_UNSUPPORTED, "C=%d (only %d)", C, CH);
    RET_IF(need_ws(ws_bytes, pdsc_sm_loss_fused_workspace_bytes(B, N, C)));
    hipStream_t s = S_(stream);
    const BwdGrid g = smf_grid(B, N);
    Carve c(ws);
    const SmfBufs a = bind_smf(c, g);
    const bool split = g.nsplit > 1;
    hipLaunchKernelGGL(sm_fused_coef_kernel, dim3(B), dim3(64), 0, s, gt_labels, B, N, balanced, a.coef);
    const dim3 grid((unsigned)(B * g.nblk * g.nsplit));
    if (dnormed) {
        hipLaunchKernelGGL(sm_fused_kernel<true>, grid, dim3(256), 0, s, normed, sigma, gt_labels, a.coef, g,
                           split ? a.dn : dnormed, a.part);
        if (split) {
            const size_t n4 = (size_t)N * CH / 4;
            hipLaunchKernelGGL(sm_fused_sum_kernel, dim3((unsigned)((B * n4 + 255) / 256)), dim3(256), 0, s, a.dn, sigma,
                               B, n4, g.nsplit, dnormed);
        }
    } else {
        hipLaunchKernelGGL(sm_fused_kernel<false>, grid, dim3(256), 0, s, normed, sigma, gt_labels, a.coef, g,
                           (float *)nullptr, a.part);
    }
    hipLaunchKernelGGL(sm_fused_final_kernel, dim3(1), dim3(64), 0, s, a.part, a.coef, sigma, B, g.nblk * g.nsplit,
                       loss, dsigma);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
