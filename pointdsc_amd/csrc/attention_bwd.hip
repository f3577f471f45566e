// attention_bwd.hip -- training: the exact-fp32 attention forward that keeps the
// row log-sum-exp, and its backward, which recomputes P from (q, k, M, lse)
// instead of storing it (DESIGN.md §7 "Training").
//
//   S_ij = q_i.k_j / sqrt(128)    X_ij = M_ij S_ij    L_i = logsumexp_j X_ij
//   P_ij = exp(X_ij - L_i)        msg_i = sum_j P_ij v_j
//   D_i = dmsg_i.msg_i   dP_ij = dmsg_i.v_j   dX_ij = P_ij (dP_ij - D_i)
//   dS_ij = M_ij dX_ij / sqrt(128)
//   dq_i = sum_j dS_ij k_j    dk_j = sum_i dS_ij q_i    dv_j = sum_i P_ij dmsg_i
//
// The forward is pdsc_attention_f32's PDSC_PRECISION_F32 launch (launch_attention
// on the ATT_F32 plan, then the same combine) plus one kernel that reads the
// split partials' (m, l) and writes lse = m* + ln sum_s l_s e^(m_s - m*).
//
// The backward is three kernels and two fixed-order sums:
//   attn_bwd_d    D_i, one wavefront per row
//   attn_bwd_kv   a workgroup = 4 waves x 32 keys of one pair and a contiguous
//                 range of 32-query tiles; the wave keeps its keys' k and v rows
//                 in registers, the workgroup stages each query tile's q and dmsg
//                 rows (and lse, D) in LDS.  Per tile: S = q k^T and dP = dmsg v^T
//                 on v_mfma_f32_32x32x2_f32 (accumulator row <-> query, lane <->
//                 key), P and dS in registers, then dv += P^T dmsg and
//                 dk += dS^T q with P / dS as the A operand as they lie.
//   attn_bwd_q    the mirror image: a workgroup = 4 waves x 32 queries and a
//                 range of 32-key tiles staged in LDS; S^T = k q^T and
//                 dP^T = v dmsg^T (lane <-> query; M read column-wise, it is
//                 symmetric), dq += dS k.
//   attn_bwd_sum  when a pair's tiles are split over workgroups to fill the chip,
//                 the partials [B][split][N][CH] are added in split order.
// No atomics and no order that depends on scheduling: two calls are bit-equal.
#include "abi.hpp"
#include "bwd_tile.hpp"
#include "encoder_row.hpp"

namespace pdsc {

// fp32 rows [B][N][CH] -> [B][Npad][CH], zero rows past N (the f32 attention's input)
__global__ void bwd_pad_rows_kernel(const float *__restrict__ x, int B, int N, int Npad, float *__restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Npad * CH) return;
    const int c = (int)(i % CH), row = (int)((i / CH) % Npad), b = (int)(i / CH / Npad);
    y[i] = row < N ? x[((size_t)b * N + row) * CH + c] : 0.0f;
}

// lse[b][row] from the split partials ml [B][nsplit][Npad][2] (m in natural-log
// units, l relative to m): the combine's own m* and L (encoder_row.hpp: combine16).
__global__ void attn_lse_kernel(const float *__restrict__ ml, int B, int N, int Npad, int nsplit,
                                float *__restrict__ lse) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * N) return;
    const int b = (int)(i / N), row = (int)(i % N);
    const float *mlb = ml + ((size_t)b * nsplit * Npad + row) * 2;
    float mstar = -INFINITY;
    for (int s = 0; s < nsplit; ++s) mstar = fmaxf(mstar, mlb[(size_t)s * Npad * 2]);
    float L = 0.0f;
    for (int s = 0; s < nsplit; ++s) L += expf(mlb[(size_t)s * Npad * 2] - mstar) * mlb[(size_t)s * Npad * 2 + 1];
    lse[i] = mstar + logf(L);
}

// D[b][i] = dmsg_i . msg_i: one wavefront per row, two channels per lane
__global__ __launch_bounds__(256) void attn_bwd_d_kernel(const float *__restrict__ msg, const float *__restrict__ dmsg,
                                                         size_t rows, float *__restrict__ D) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const f32x2 a = *reinterpret_cast<const f32x2 *>(msg + row * CH + 2 * lane);
    const f32x2 g = *reinterpret_cast<const f32x2 *>(dmsg + row * CH + 2 * lane);
    const float d = wave_sum(a[0] * g[0] + a[1] * g[1]);
    if (lane == 0) D[row] = d;
}

constexpr size_t BW_LDS = (size_t)(2 * BW_T * BW_STR + 2 * BW_T) * sizeof(float);

// dk, dv of 128 keys over the query tiles [split * tps, ...): into dkp, dvp
// [B][nsplit][N][CH] (nsplit = 1: the outputs themselves).
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                          const float *__restrict__ v, const float *__restrict__ M,
                                                          const float *__restrict__ lse, const float *__restrict__ D,
                                                          const float *__restrict__ dmsg, BwdGrid g,
                                                          float *__restrict__ dkp, float *__restrict__ dvp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Ql = smem, *Gl = smem + BW_T * BW_STR, *Ll = Gl + BW_T * BW_STR, *Dl = Ll + BW_T;
    const int N = g.N;
    const int split = blockIdx.x % g.nsplit, kb = (blockIdx.x / g.nsplit) % g.nblk, b = blockIdx.x / g.nsplit / g.nblk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int j0 = kb * BW_ROWS + wave * BW_T, key = j0 + l32;
    const bool active = j0 < N;  // wave-uniform
    const int nt = (N + BW_T - 1) / BW_T;
    const int t0 = split * g.tps, t1 = min(nt, t0 + g.tps);
    const size_t pb = (size_t)b * N * CH;
    const float *qb = q + pb, *gb = dmsg + pb, *Mb = M + (size_t)b * N * N;
    const float *lb = lse + (size_t)b * N, *Db = D + (size_t)b * N;

    float kf[64], vf[64];
    load_rows64(k + pb, key, N, h, kf);
    load_rows64(v + pb, key, N, h, vf);
    f32x16 dV0 = zero16(), dV1 = zero16(), dV2 = zero16(), dV3 = zero16();
    f32x16 dK0 = zero16(), dK1 = zero16(), dK2 = zero16(), dK3 = zero16();

    TileRegs tr;
    float sl = 0.0f, sd = 0.0f;  // threads 0..31: the tile's lse and D
    auto load = [&](int t) {
        tile_load(qb, gb, t * BW_T, N, tid, tr);
        if (tid < BW_T) {
            const int row = t * BW_T + tid;
            sl = row < N ? lb[row] : 0.0f;
            sd = row < N ? Db[row] : 0.0f;
        }
    };
    auto store = [&]() {
        tile_store(Ql, Gl, tid, tr);
        if (tid < BW_T) {
            Ll[tid] = sl;
            Dl[tid] = sd;
        }
    };
    // (no register prefetch of the next tile here: with k, v, dk and dv resident
    // it would not fit the register file)
    if (t0 < t1) {
        load(t0);
        store();
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        if (active) {
            const int i0 = t * BW_T;
            // M[query][key]: accumulator row <-> query, lane <-> key (128 B of a row per half-wave)
            float mv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = i0 + acc_row(r, h);
                mv[r] = (qi < N && key < N) ? Mb[(size_t)qi * N + key] : 0.0f;
            }
            const f32x16 S = dot_lds_reg(Ql, kf, h, l32);
            const f32x16 dP = dot_lds_reg(Gl, vf, h, l32);
            float p[16], ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ar = acc_row(r, h);
                const bool in = i0 + ar < N && key < N;
                const float x = mv[r] * (S[r] * BW_SCALE);
                p[r] = in ? expf(x - Ll[ar]) : 0.0f;
                ds[r] = mv[r] * (p[r] * (dP[r] - Dl[ar])) * BW_SCALE;
            }
            accum_rows(p, Gl, h, l32, dV0, dV1, dV2, dV3);
            accum_rows(ds, Ql, h, l32, dK0, dK1, dK2, dK3);
        }
        __syncthreads();
        if (t + 1 < t1) {
            load(t + 1);
            store();
        }
        __syncthreads();
    }
    if (!active) return;
    const size_t ob = ((size_t)b * g.nsplit + split) * N * CH;
    store_rows(dvp + ob, j0, N, h, l32, dV0, dV1, dV2, dV3);
    store_rows(dkp + ob, j0, N, h, l32, dK0, dK1, dK2, dK3);
}

// dq of 128 queries over the key tiles [split * tps, ...): into dqp [B][nsplit][N][CH].
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                         const float *__restrict__ v, const float *__restrict__ M,
                                                         const float *__restrict__ lse, const float *__restrict__ D,
                                                         const float *__restrict__ dmsg, BwdGrid g,
                                                         float *__restrict__ dqp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Kl = smem, *Vl = smem + BW_T * BW_STR;
    const int N = g.N;
    const int split = blockIdx.x % g.nsplit, qblk = (blockIdx.x / g.nsplit) % g.nblk, b = blockIdx.x / g.nsplit / g.nblk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int i0 = qblk * BW_ROWS + wave * BW_T, qi = i0 + l32;
    const bool active = i0 < N;  // wave-uniform
    const int nt = (N + BW_T - 1) / BW_T;
    const int t0 = split * g.tps, t1 = min(nt, t0 + g.tps);
    const size_t pb = (size_t)b * N * CH;
    const float *kb = k + pb, *vb = v + pb, *Mb = M + (size_t)b * N * N;

    float qf[64], gf[64];
    load_rows64(q + pb, qi, N, h, qf);
    load_rows64(dmsg + pb, qi, N, h, gf);
    const float lq = qi < N ? lse[(size_t)b * N + qi] : 0.0f, dq_ = qi < N ? D[(size_t)b * N + qi] : 0.0f;
    f32x16 dQ0 = zero16(), dQ1 = zero16(), dQ2 = zero16(), dQ3 = zero16();

    TileRegs tr;
    if (t0 < t1) {
        tile_load(kb, vb, t0 * BW_T, N, tid, tr);
        tile_store(Kl, Vl, tid, tr);
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) tile_load(kb, vb, (t + 1) * BW_T, N, tid, tr);
        if (active) {
            const int j0 = t * BW_T;
            // M[key][query] = M[query][key]: accumulator row <-> key, lane <-> query
            float mv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = j0 + acc_row(r, h);
                mv[r] = (key < N && qi < N) ? Mb[(size_t)key * N + qi] : 0.0f;
            }
            const f32x16 St = dot_lds_reg(Kl, qf, h, l32);
            const f32x16 dPt = dot_lds_reg(Vl, gf, h, l32);
            float ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool in = j0 + acc_row(r, h) < N && qi < N;
                const float x = mv[r] * (St[r] * BW_SCALE);
                const float p = in ? expf(x - lq) : 0.0f;
                ds[r] = mv[r] * (p * (dPt[r] - dq_)) * BW_SCALE;
            }
            accum_rows(ds, Kl, h, l32, dQ0, dQ1, dQ2, dQ3);
        }
        __syncthreads();
        if (t + 1 < t1) tile_store(Kl, Vl, tid, tr);
        __syncthreads();
    }
    if (!active) return;
    store_rows(dqp + ((size_t)b * g.nsplit + split) * N * CH, i0, N, h, l32, dQ0, dQ1, dQ2, dQ3);
}

// out [B][n] = sum over s (ascending) of part [B][nsplit][n], n = N * CH floats, 4 per thread
__global__ void attn_bwd_sum_kernel(const float *__restrict__ part, int B, size_t n4, int nsplit,
                                    float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * n4) return;
    const size_t b = i / n4, e = i % n4;
    const f32x4 *p = reinterpret_cast<const f32x4 *>(part) + b * nsplit * n4 + e;
    f32x4 acc = p[0];
    for (int s = 1; s < nsplit; ++s) acc += p[(size_t)s * n4];
    reinterpret_cast<f32x4 *>(out)[i] = acc;
}

// pdsc_attention_lse_f32's workspace: q, k, v zero-padded to Npad rows, the split partials
struct LseBufs {
    float *q, *k, *v, *op, *ml;
};
static LseBufs bind_lse(Carve &c, const EncoderPlan &plan) {
    const size_t B = plan.B, Npad = plan.Npad, ns = plan.nsplit;
    LseBufs a;
    a.q = c.take<float>(B * Npad * CH);
    a.k = c.take<float>(B * Npad * CH);
    a.v = c.take<float>(B * Npad * CH);
    a.op = c.take<float>(B * Npad * CH * ns);
    a.ml = c.take<float>(B * Npad * ns * 2);
    return a;
}

// pdsc_attention_backward_f32's workspace: D, and the partials when the tiles are split
struct BwdBufs {
    float *D, *dq, *dk, *dv;
};
static BwdBufs bind_bwd(Carve &c, const BwdGrid &g) {
    BwdBufs a;
    a.D = c.take<float>((size_t)g.B * g.N);
    const size_t part = g.nsplit > 1 ? (size_t)g.B * g.nsplit * g.N * CH : 0;
    a.dq = c.take<float>(part);
    a.dk = c.take<float>(part);
    a.dv = c.take<float>(part);
    return a;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_attention_lse_workspace_bytes(int32_t B, int32_t N, int32_t C) {
    if (C != CH || B < 1 || N < 1 || N > 32767) return 0;
    Carve c(nullptr);
    bind_lse(c, plan_encoder(B, N, true, true, false));
    return c.off;
}

int32_t pdsc_attention_lse_f32(const float *q, const float *k, const float *v, const float *M, int32_t B, int32_t N,
                               int32_t C, float *msg, float *lse, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (C != CH) return fail(PDSC_ERR_ARG, "C=%d (only %d)", C, CH);
    if (!q || !k || !v || !M || !msg || !lse || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || N < 1 || N > 32767) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    RET_IF(need_ws(ws_bytes, pdsc_attention_lse_workspace_bytes(B, N, C)));
    hipStream_t s = S_(stream);
    const EncoderPlan plan = plan_encoder(B, N, true, true, false);  // pdsc_attention_f32's PDSC_PRECISION_F32 plan
    const int Npad = plan.Npad;
    Carve c(ws);
    const LseBufs a = bind_lse(c, plan);
    const size_t n = (size_t)B * Npad * CH;
    const dim3 pg((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(bwd_pad_rows_kernel, pg, dim3(256), 0, s, q, B, N, Npad, a.q);
    hipLaunchKernelGGL(bwd_pad_rows_kernel, pg, dim3(256), 0, s, k, B, N, Npad, a.k);
    hipLaunchKernelGGL(bwd_pad_rows_kernel, pg, dim3(256), 0, s, v, B, N, Npad, a.v);
    HIPCHK(hipGetLastError());
    HIPCHK(launch_attention(plan, a.q, a.k, a.v, nullptr, M, a.op, a.ml, s));
    HIPCHK(launch_attn_combine(a.op, a.ml, true, B, N, Npad, plan.nsplit, msg, s));
    hipLaunchKernelGGL(attn_lse_kernel, dim3((unsigned)(((size_t)B * N + 255) / 256)), dim3(256), 0, s, a.ml, B, N, Npad,
                       plan.nsplit, lse);
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

size_t pdsc_attention_backward_workspace_bytes(int32_t B, int32_t N, int32_t C) {
    if (C != CH || B < 1 || N < 1 || N > 32767) return 0;
    Carve c(nullptr);
    bind_bwd(c, bwd_grid(B, N));
    return c.off;
}

int32_t pdsc_attention_backward_f32(const float *q, const float *k, const float *v, const float *M, const float *msg,
                                    const float *lse, const float *dmsg, int32_t B, int32_t N, int32_t C, float *dq,
                                    float *dk, float *dv, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    if (C != CH) return fail(PDSC_ERR_ARG, "C=%d (only %d)", C, CH);
    if (!q || !k || !v || !M || !msg || !lse || !dmsg || !dq || !dk || !dv || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || N < 1 || N > 32767) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    RET_IF(need_ws(ws_bytes, pdsc_attention_backward_workspace_bytes(B, N, C)));
    hipStream_t s = S_(stream);
    const BwdGrid g = bwd_grid(B, N);
    Carve c(ws);
    const BwdBufs a = bind_bwd(c, g);
    const bool split = g.nsplit > 1;
    const size_t rows = (size_t)B * N;
    hipLaunchKernelGGL(attn_bwd_d_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, msg, dmsg, rows, a.D);
    const dim3 grid((unsigned)(B * g.nblk * g.nsplit));
    hipLaunchKernelGGL(attn_bwd_kv_kernel, grid, dim3(256), BW_LDS, s, q, k, v, M, lse, a.D, dmsg, g, split ? a.dk : dk,
                       split ? a.dv : dv);
    hipLaunchKernelGGL(attn_bwd_q_kernel, grid, dim3(256), BW_LDS, s, q, k, v, M, lse, a.D, dmsg, g, split ? a.dq : dq);
    if (split) {
        const size_t n4 = (size_t)N * CH / 4;
        const dim3 sg((unsigned)((B * n4 + 255) / 256));
        hipLaunchKernelGGL(attn_bwd_sum_kernel, sg, dim3(256), 0, s, a.dq, B, n4, g.nsplit, dq);
        hipLaunchKernelGGL(attn_bwd_sum_kernel, sg, dim3(256), 0, s, a.dk, B, n4, g.nsplit, dk);
        hipLaunchKernelGGL(attn_bwd_sum_kernel, sg, dim3(256), 0, s, a.dv, B, n4, g.nsplit, dv);
    }
    HIPCHK(hipGetLastError());
    return PDSC_OK;
}

}  // extern "C"
