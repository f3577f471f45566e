// attention.hip -- a3 as launches of its own: one layer's split attention as
// the plan says (launch_attention: attention_h3.hpp, attention_w64.hpp,
// attention.hpp), and the standalone attention entries of include/pdsc.h with
// their input conversion (the combine kernel is in encoder.hip).  (The fused plan's attention runs inside
// encoder.hip's attn_pw2 kernels.)
#include "abi.hpp"
#include "encoder_row.hpp"

namespace pdsc {

// vexp of every 32-key tile of fp32 v [B][ld][CH] (rows >= N count as 0):
// one workgroup per (tile, pair).
static __global__ __launch_bounds__(256) void vexp_kernel(const float *__restrict__ v, int N, int ld, int Npad,
                                                         float *__restrict__ vexp) {
    __shared__ float part[4];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float m = 0.0f;
    for (int e = tid; e < H3_TILE * CH; e += 256) {
        const int row = t * H3_TILE + e / CH;
        if (row < N) m = fmaxf(m, fabsf(v[((size_t)b * ld + row) * CH + e % CH]));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) vexp[(size_t)b * (Npad / H3_TILE) + t] = (float)h3_vexp(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])));
}

// fp32 q, k, v [B][ld][CH] (ld >= N rows per pair; rows >= N of the padded
// layouts become zero) -> Qs, Ks, Vs (V scaled by its tile's 2^vexp).  One
// thread per (pair, row, channel).
static __global__ void split_qkv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                 const float *__restrict__ v, const float *__restrict__ vexp, int B, int N,
                                 int ld, int Npad, _Float16 *__restrict__ Qs, _Float16 *__restrict__ Ks,
                                 _Float16 *__restrict__ Vs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Npad * CH) return;
    const int c = (int)(i % CH);
    const int row = (int)((i / CH) % Npad);
    const int b = (int)(i / CH / Npad);
    const size_t src = ((size_t)b * ld + row) * CH + c, pb = (size_t)b * Npad * 2 * CH;
    const bool in = row < N;
    _Float16 hi, lo;
    split_h(in ? (ATT_QFMA ? q[src] * H3_QSCALE : q[src]) : 0.0f, hi, lo);
    Qs[pb + qs_off(row, 0, c)] = hi;
    Qs[pb + qs_off(row, 1, c)] = lo;
    split_h(in ? k[src] : 0.0f, hi, lo);
    Ks[pb + ks_off(row, 0, c)] = hi;
    Ks[pb + ks_off(row, 1, c)] = lo;
    const float ev = vexp[(size_t)b * (Npad / H3_TILE) + row / H3_TILE];
    split_h(in ? ldexpf(v[src], (int)ev) : 0.0f, hi, lo);
    Vs[pb + vs_off(row, 0, c)] = hi;
    Vs[pb + vs_off(row, 1, c)] = lo;
}

// One layer's attention as the plan says.
hipError_t launch_attention(const EncoderPlan &plan, const void *q, const void *k, const void *v, const float *vexp,
                            const float *M, float *opart, float *ml, hipStream_t s, Ragged rg, int layer) {
    const dim3 grid(plan.workgroups());
    const _Float16 *qs = static_cast<const _Float16 *>(q), *ks = static_cast<const _Float16 *>(k),
                   *vs = static_cast<const _Float16 *>(v);
    const AttnGridH3 g = plan_grid_h3(plan, rg, layer);
    const bool packed = plan.m_layout == M_PACKED;
    switch (plan.kind) {
    case ATT_W64_SK:
        hipLaunchKernelGGL((attention_w64_sk_kernel<true>), grid, dim3(W64_NW * 64), W64_LDS, s, qs, ks, vs, vexp, M, g,
                           plan.sk_wgs, opart, ml);
        break;
    case ATT_W64:
        hipLaunchKernelGGL((attention_w64_kernel<true>), grid, dim3(W64_NW * 64), W64_LDS, s, qs, ks, vs, vexp, M, g,
                           opart, ml);
        break;
    case ATT_F32: {  // fp32 [B][Npad][CH] rows, dense M
        const AttnGrid gf{plan.B, plan.N, plan.Npad, plan.nqb, plan.nsplit, plan.sps, rg.nv};
        hipLaunchKernelGGL((attention_kernel_t<ATT_NW, ATT_F32_KTS, false, true>), grid, dim3(ATT_NW * 64),
                           (attention_lds_bytes<ATT_NW, ATT_F32_KTS>()), s, static_cast<const float *>(q),
                           static_cast<const float *>(k), static_cast<const float *>(v), M, gf, opart, ml);
        break;
    }
    case ATT_H3_WS:
        if (plan.vfold) return hipErrorInvalidValue;
        with_int<2, 4>(plan.ws, [&](auto ws) {
            with_bool(packed, [&](auto pk) {
                constexpr int WS = decltype(ws)::value;
                hipLaunchKernelGGL((attention_h3_ws_kernel<WS, decltype(pk)::value>), grid, dim3(WS * 64),
                                   attention_h3_ws_lds_bytes<WS>(), s, qs, ks, vs, vexp, M, g, opart, ml);
            });
        });
        break;
    case ATT_H3:
        if (plan.vfold) {  // the folded V' (the register-chained chains' plans: 4 waves)
            if (plan.nw != ATT_NW) return hipErrorInvalidValue;
            with_bool(plan.early, [&](auto early) {
                with_bool(packed, [&](auto pk) {
                    hipLaunchKernelGGL((attention_h3_kernel<ATT_NW, true, decltype(pk)::value, decltype(early)::value, CH2>),
                                       grid, dim3(ATT_NW * 64), attention_h3_lds_bytes<ATT_NW>(), s, qs, ks, vs, vexp, M,
                                       g, opart, ml);
                });
            });
            break;
        }
        with_int<1, 2, ATT_NW>(plan.nw, [&](auto nw) {
            with_bool(plan.early, [&](auto early) {
                with_bool(packed, [&](auto pk) {
                    constexpr int NW = decltype(nw)::value;
                    hipLaunchKernelGGL((attention_h3_kernel<NW, true, decltype(pk)::value, decltype(early)::value>), grid,
                                       dim3(NW * 64), attention_h3_lds_bytes<NW>(), s, qs, ks, vs, vexp, M, g, opart,
                                       ml);
                });
            });
        });
        break;
    default: return hipErrorInvalidValue;  // ATT_FUSED: launch_attn_pw2
    }
    return hipGetLastError();
}

// fp32 rows [B][N][CH] -> [B][Npad][CH] with zero padding rows (the f32 attention's input)
__global__ void pad_rows_kernel(const float *__restrict__ x, int B, int N, int Npad, float *__restrict__ y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Npad * CH) return;
    const int c = (int)(i % CH), row = (int)((i / CH) % Npad), b = (int)(i / CH / Npad);
    y[i] = row < N ? x[((size_t)b * N + row) * CH + c] : 0.0f;
}

static hipError_t launch_pad_rows(const float *x, int B, int N, int Npad, float *y, hipStream_t s) {
    const size_t n = (size_t)B * Npad * CH;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, B, N, Npad, y);
    return hipGetLastError();
}

static hipError_t launch_split_qkv(const float *q, const float *k, const float *v, int B, int N, int ld, int Npad,
                            _Float16 *qs, _Float16 *ks, _Float16 *vs, float *vexp, hipStream_t s) {
    const size_t n = (size_t)B * Npad * CH;
    hipLaunchKernelGGL(vexp_kernel, dim3(Npad / H3_TILE, B), dim3(256), 0, s, v, N, ld, Npad, vexp);
    hipLaunchKernelGGL(split_qkv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, k, v, vexp, B, N, ld,
                       Npad, qs, ks, vs);
    return hipGetLastError();
}

// the standalone attention's workspace: Q, K, V in the kernels' layouts, the partials, the V-tile exponents
struct AttnBufs {
    _Float16 *qs, *ks, *vs;
    float *op, *ml, *vexp;
};
static AttnBufs bind_attention(Carve &c, const EncoderPlan &plan) {
    const size_t B = plan.B, Npad = plan.Npad, ns = plan.nsplit;
    AttnBufs a;
    a.qs = c.take<_Float16>(2 * B * Npad * CH);
    a.ks = c.take<_Float16>(2 * B * Npad * CH);
    a.vs = c.take<_Float16>(2 * B * Npad * CH);
    a.op = c.take<float>(B * Npad * CH * ns);
    a.ml = c.take<float>(B * Npad * ns * 2);
    a.vexp = c.take<float>(B * (Npad / 32));
    return a;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" {

size_t pdsc_attention_workspace_bytes(int32_t B, int32_t N, int32_t C, int32_t precision) {
    if (C != CH || B < 1 || N < 1 || (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)) return 0;
    Carve c(nullptr);
    bind_attention(c, plan_encoder(B, N, precision == PDSC_PRECISION_F32, true, false));
    return c.off;
}

int32_t pdsc_attention_f32(const float *q, const float *k, const float *v, const float *M, int32_t B,
                           int32_t N, int32_t C, int32_t precision, float *msg, void *ws, size_t ws_bytes,
                           pdsc_stream_t stream) {
    if (C != CH) return fail(PDSC_ERR_UNSUPPORTED, "C=%d (only %d)", C, CH);
    if (!q || !k || !v || !M || !msg || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    if (B < 1 || N < 1 || N > 32767) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision=%d", precision);
    RET_IF(need_ws(ws_bytes, pdsc_attention_workspace_bytes(B, N, C, precision)));
    hipStream_t s = S_(stream);
    const bool f32 = precision == PDSC_PRECISION_F32;
    const EncoderPlan plan = plan_encoder(B, N, f32, true, false);  // the split launch on the caller's dense M
    const int Npad = plan.Npad;
    Carve c(ws);
    const AttnBufs a = bind_attention(c, plan);
    if (f32) {  // the caller's rows, zero-padded to Npad rows (the same bytes as the split layouts)
        HIPCHK(launch_pad_rows(q, B, N, Npad, reinterpret_cast<float *>(a.qs), s));
        HIPCHK(launch_pad_rows(k, B, N, Npad, reinterpret_cast<float *>(a.ks), s));
        HIPCHK(launch_pad_rows(v, B, N, Npad, reinterpret_cast<float *>(a.vs), s));
    } else {  // the caller's fp32 [B][N][C] rows -> the kernel's padded fp16 hi/lo layouts
        HIPCHK(launch_split_qkv(q, k, v, B, N, N, Npad, a.qs, a.ks, a.vs, a.vexp, s));
    }
    HIPCHK(launch_attention(plan, a.qs, a.ks, a.vs, a.vexp, M, a.op, a.ml, s));
    HIPCHK(launch_attn_combine(a.op, a.ml, f32, B, N, Npad, plan.nsplit, msg, s));
    return PDSC_OK;
}

}  // extern "C"
