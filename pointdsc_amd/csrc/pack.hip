// pack.hip -- the packed-weight blob (pdsc_internal.hpp: PackLayout): the
// parameter list, the packing kernels and the weight entries of include/pdsc.h.
#include <cstdio>
#include <string>

#include "abi.hpp"
#include "pdsc_internal.hpp"

namespace pdsc {

// Per-layer power-of-two scale: max|W| 2^s <= 2^14 keeps hi and (for all but
// the weights 2^-17 below the layer's largest) lo in fp16's normal range.
__global__ __launch_bounds__(256) void wscale_kernel(const float *__restrict__ w, int n, int f32,
                                                     float *__restrict__ sc) {
    __shared__ float part[4];
    if (f32) {  // exact-fp32 weights are stored unscaled
        if (threadIdx.x == 0) sc[0] = sc[1] = 1.0f;
        return;
    }
    float m = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(w[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        int ex = 0;
        if (m > 0.0f && m < INFINITY) frexpf(m, &ex);  // m < 2^ex
        const int sh = max(-100, min(100, 14 - ex));
        sc[0] = ldexpf(1.0f, -sh);
        sc[1] = ldexpf(1.0f, sh);
    }
}

// W [out][in] (torch Conv1d weight) -> W_PLANES fp16 planes hi, mid (, lo) of
// W * 2^s ~= hi + mid (22 significant bits; with lo: 33, every fp32 weight
// exactly) in MFMA-fragment blocks (w3_index, pdsc_internal.hpp): block (t, ks)
// = outputs 32t..32t+31 x the 16 inputs of k-step ks, planes of 1 KiB
// each, lane (h, n)'s 16 B = positions 8h .. 8h+7 of output 32t + n in qk_pos
// order (bits 2 and 3 of the input index swapped: inputs {4h..4h+3,
// 8+4h..8+4h+3} of the k-step, exactly the channels a transposed product's
// accumulator half h holds).  Blocks are stored t-major, so any run of
// consecutive blocks is one contiguous copy (f32: W itself, fp32 [out][in]).
// BN folded as torch-CPU eval folds it.
__global__ void pack_dense_kernel(const float *__restrict__ w, const float *__restrict__ b,
                                  const float *__restrict__ bn_w, const float *__restrict__ bn_b,
                                  const float *__restrict__ bn_rm, const float *__restrict__ bn_rv,
                                  int in, int out, int f32, float *__restrict__ dw, float *__restrict__ db,
                                  float *__restrict__ da, float *__restrict__ dbeta,
                                  const float *__restrict__ sc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = in * out;
    if (i < total && f32) {
        dw[i] = w[i];
    } else if (i < total) {
        _Float16 *wd = reinterpret_cast<_Float16 *>(dw);
        const int o = i / in, c = i % in;
        float x = w[i] * sc[1];  // exact (power of two)
        asm("" : "+v"(x));       // one hi for both uses (see split_h)
        const _Float16 hi = (_Float16)x;
        const float r1 = x - (float)hi;  // exact
        const _Float16 mid = (_Float16)r1;
        const size_t d = w3_index(o, c, in);
        wd[d] = hi;
        wd[d + 512] = mid;
        if (W_PLANES == 3) wd[d + 1024] = (_Float16)(r1 - (float)mid);
    }
    if (i < out) {
        db[i] = b[i];
        if (bn_w) {
            // torch-CPU eval BatchNorm: invstd = 1/sqrt(var+eps); alpha = invstd*w; beta = b - mean*alpha
            const float invstd = 1.0f / sqrtf(bn_rv[i] + 1e-5f);
            const float alpha = invstd * bn_w[i];
            da[i] = alpha;
            dbeta[i] = bn_b[i] - bn_rm[i] * alpha;
        } else {
            da[i] = 1.0f;
            dbeta[i] = 0.0f;
        }
    }
}

__global__ void copy_kernel(const float *__restrict__ s, float *__restrict__ d, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = s[i];
}

static hipError_t launch_pack_dense(const float *w, const float *b, const float *bn_w, const float *bn_b,
                                    const float *bn_rm, const float *bn_rv, int in, int out, bool f32, float *dst_w,
                                    float *dst_b, float *dst_a, float *dst_beta, float *dst_scale, hipStream_t s) {
    const int n = in * out;
    hipLaunchKernelGGL(wscale_kernel, dim3(1), dim3(256), 0, s, w, n, (int)f32, dst_scale);
    hipLaunchKernelGGL(pack_dense_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, b, bn_w, bn_b,
                       bn_rm, bn_rv, in, out, (int)f32, dst_w, dst_b, dst_a, dst_beta, dst_scale);
    return hipGetLastError();
}

// The V fold: wm = W0 Wv [CH2][CH] and bm = W0 bv + b0 [CH2],
// summed in fp64 (every product of two fp32 values is exact there) and rounded
// once to fp32.  w0 [CH2][CH]: fc_message[0]; wv [CH][CH], bv: projection_v.
__global__ void fold_vm_kernel(const float *__restrict__ w0, const float *__restrict__ b0,
                               const float *__restrict__ wv, const float *__restrict__ bv,
                               float *__restrict__ wm, float *__restrict__ bm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < CH2 * CH) {
        const int o = i / CH, c = i % CH;
        double acc = 0.0;
        for (int j = 0; j < CH; ++j) acc += (double)w0[o * CH + j] * (double)wv[j * CH + c];
        wm[i] = (float)acc;
    }
    if (i < CH2) {
        double acc = (double)b0[i];
        for (int j = 0; j < CH; ++j) acc += (double)w0[i * CH + j] * (double)bv[j];
        bm[i] = (float)acc;
    }
}

static hipError_t launch_copy(const float *src, float *dst, int n, hipStream_t s) {
    hipLaunchKernelGGL(copy_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

}  // namespace pdsc

using namespace pdsc;

namespace {
thread_local std::string g_name;  // pdsc_param_name's composed names
}  // namespace

extern "C" {

// ------------------------------------------------------------------ weights
int32_t pdsc_param_count(const pdsc_config *cfg) { return cfg ? 10 + 26 * cfg->num_layers : -1; }

const char *pdsc_param_name(const pdsc_config *cfg, int32_t i) {
    if (!cfg || i < 0 || i >= pdsc_param_count(cfg)) return nullptr;
    static const char *bn[] = {"weight", "bias", "running_mean", "running_var"};
    static const char *per[] = {"fc_message.0.weight", "fc_message.0.bias", "fc_message.1.weight",
                                "fc_message.1.bias", "fc_message.1.running_mean", "fc_message.1.running_var",
                                "fc_message.3.weight", "fc_message.3.bias", "fc_message.4.weight",
                                "fc_message.4.bias", "fc_message.4.running_mean", "fc_message.4.running_var",
                                "fc_message.6.weight", "fc_message.6.bias", "projection_q.weight",
                                "projection_q.bias", "projection_k.weight", "projection_k.bias",
                                "projection_v.weight", "projection_v.bias"};
    static const char *tail[] = {"encoder.layer0.weight", "encoder.layer0.bias", "classification.0.weight",
                                 "classification.0.bias", "classification.2.weight", "classification.2.bias",
                                 "classification.4.weight", "classification.4.bias"};
    const int L = cfg->num_layers;
    if (i == 0) return "sigma";
    if (i == 1) return "sigma_spat";
    i -= 2;
    if (i < 26 * L) {
        const int l = i / 26, o = i % 26;
        char buf[128];
        if (o < 2)
            snprintf(buf, sizeof(buf), "encoder.blocks.PointCN_layer_%d.0.%s", l, o == 0 ? "weight" : "bias");
        else if (o < 6)
            snprintf(buf, sizeof(buf), "encoder.blocks.PointCN_layer_%d.1.%s", l, bn[o - 2]);
        else
            snprintf(buf, sizeof(buf), "encoder.blocks.NonLocal_layer_%d.%s", l, per[o - 6]);
        g_name = buf;
        return g_name.c_str();
    }
    return tail[i - 26 * L];
}

size_t pdsc_packed_weights_floats(const pdsc_config *cfg) {
    if (check_cfg(cfg) != PDSC_OK) return 0;
    return make_layout(cfg->num_layers, cfg->in_dim).total;
}

int32_t pdsc_pack_weights(const pdsc_config *cfg, const float *const *P, float *packed,
                          pdsc_stream_t stream) {
    RET_IF(check_cfg(cfg));
    if (!P || !packed) return fail(PDSC_ERR_ARG, "null params/packed");
    const int n = pdsc_param_count(cfg);
    for (int i = 0; i < n; ++i)
        if (!P[i]) return fail(PDSC_ERR_ARG, "param %d (%s) is NULL", i, pdsc_param_name(cfg, i));
    hipStream_t s = S_(stream);
    const PackLayout lay = make_layout(cfg->num_layers, cfg->in_dim);
    HIPCHK(hipMemsetAsync(packed, 0, lay.total * sizeof(float), s));
    HIPCHK(launch_copy(P[0], packed + lay.sigma, 1, s));
    HIPCHK(launch_copy(P[1], packed + lay.sigma_d, 1, s));
    const bool f32 = cfg->precision == PDSC_PRECISION_F32;
    auto dense = [&](const DenseOff &o, int wi, int in, int out, bool has_bn) -> hipError_t {
        return launch_pack_dense(P[wi], P[wi + 1], has_bn ? P[wi + 2] : nullptr,
                                 has_bn ? P[wi + 3] : nullptr, has_bn ? P[wi + 4] : nullptr,
                                 has_bn ? P[wi + 5] : nullptr, in, out, f32, packed + o.w, packed + o.bias,
                                 packed + o.alpha, packed + o.beta, packed + o.scale, s);
    };
    float *fold_tmp = nullptr;
    HIPCHK(hipMallocAsync(reinterpret_cast<void **>(&fold_tmp), ((size_t)CH2 * CH + CH2) * sizeof(float), s));
    for (int l = 0; l < cfg->num_layers; ++l) {
        const int b = 2 + 26 * l;
        const LayerOff &lo = lay.layer[l];
        HIPCHK(dense(lo.pcn, b + 0, CH, CH, true));
        HIPCHK(dense(lo.fc0, b + 6, CH, CH2, true));
        HIPCHK(dense(lo.fc3, b + 12, CH2, CH2, true));
        HIPCHK(dense(lo.fc6, b + 18, CH2, CH, false));
        HIPCHK(dense(lo.q, b + 20, CH, CH, false));
        HIPCHK(dense(lo.k, b + 22, CH, CH, false));
        HIPCHK(dense(lo.v, b + 24, CH, CH, false));
        // the V fold: W0 Wv and W0 bv + b0 (fp64, rounded once) packed as a dense block
        // of their own, with fc0's BatchNorm (launch_pack_dense takes the scale from W0 Wv)
        // (wm, bm: a stream-ordered temporary of the call)
        float *wm = fold_tmp, *bm = wm + (size_t)CH2 * CH;
        hipLaunchKernelGGL(fold_vm_kernel, dim3(CH2 * CH / 256), dim3(256), 0, s, P[b + 6], P[b + 7], P[b + 24], P[b + 25],
                           wm, bm);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_pack_dense(wm, bm, P[b + 8], P[b + 9], P[b + 10], P[b + 11], CH, CH2, f32, packed + lo.vm.w,
                                 packed + lo.vm.bias, packed + lo.vm.alpha, packed + lo.vm.beta, packed + lo.vm.scale, s));
    }
    HIPCHK(hipFreeAsync(fold_tmp, s));
    const int t = 2 + 26 * cfg->num_layers;
    HIPCHK(launch_copy(P[t], packed + lay.l0_w, CH * cfg->in_dim, s));
    HIPCHK(launch_copy(P[t + 1], packed + lay.l0_b, CH, s));
    HIPCHK(dense(lay.c0, t + 2, CH, CLS, false));
    HIPCHK(dense(lay.c2, t + 4, CLS, CLS, false));
    HIPCHK(launch_copy(P[t + 6], packed + lay.c4_w, CLS, s));
    HIPCHK(launch_copy(P[t + 7], packed + lay.c4_b, 1, s));
    return PDSC_OK;
}

int32_t pdsc_packed_block(const pdsc_config *cfg, int32_t layer, int32_t block, size_t offsets[5]) {
    RET_IF(check_cfg(cfg));
    if (layer < 0 || layer >= cfg->num_layers || block < 0 || block > 7 || !offsets)
        return fail(PDSC_ERR_ARG, "layer=%d block=%d", layer, block);
    const LayerOff lo = make_layout(cfg->num_layers, cfg->in_dim).layer[layer];
    const DenseOff d[8] = {lo.pcn, lo.fc0, lo.fc3, lo.fc6, lo.q, lo.k, lo.v, lo.vm};
    const DenseOff &o = d[block];
    offsets[0] = o.w, offsets[1] = o.bias, offsets[2] = o.alpha, offsets[3] = o.beta, offsets[4] = o.scale;
    return PDSC_OK;
}

}  // extern "C"
