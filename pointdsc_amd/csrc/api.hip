// api.hip -- the forward: the testing and training forwards of include/pdsc.h,
// the encoder and attention entries that share their helpers (Dims, EncBufs),
// weight packing, and the plan, timing and diag queries.  Nothing else: every
// other row's entry points live in the row's file (abi.hpp).
//
// Host-side orchestration only: argument checks, workspace carving and kernel
// launches on the caller's stream.  No allocation, no synchronisation.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "abi.hpp"
#include "launch_plan.hpp"
#include "pdsc_internal.hpp"

using namespace pdsc;

namespace {
thread_local std::string g_err;  // pdsc_last_error
thread_local std::string g_name;
}  // namespace

namespace pdsc {
thread_local int g_diag_qkv_delay = 0;  // pdsc_diag_qkv_delay (tests only)

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace pdsc

namespace {

// measurement hook (pdsc_attention_timing): events recorded around attention launches
thread_local hipEvent_t *g_tstart = nullptr, *g_tstop = nullptr;
thread_local int g_tcap = 0;
thread_local int32_t *g_tcount = nullptr;
// pdsc_forward_timing: PDSC_FORWARD_STAGES + 1 events per forward call
thread_local hipEvent_t *g_fev = nullptr;
thread_local int g_fcap = 0;
thread_local int32_t *g_fcount = nullptr;

int check_cfg(const pdsc_config *cfg) {
    if (!cfg) return fail(PDSC_ERR_ARG, "cfg is NULL");
    if (cfg->num_channels != CH)
        return fail(PDSC_ERR_UNSUPPORTED, "num_channels=%d: only %d is implemented", cfg->num_channels, CH);
    if (cfg->num_layers < 1 || cfg->num_layers > 64)
        return fail(PDSC_ERR_UNSUPPORTED, "num_layers=%d not in [1, 64]", cfg->num_layers);
    if (cfg->in_dim < 1 || cfg->in_dim > 128) return fail(PDSC_ERR_UNSUPPORTED, "in_dim=%d not in [1, 128]", cfg->in_dim);
    if (cfg->num_iterations < 0 || cfg->num_iterations > 31)
        return fail(PDSC_ERR_UNSUPPORTED, "num_iterations=%d not in [0, 31]", cfg->num_iterations);
    if (cfg->k < 1) return fail(PDSC_ERR_ARG, "k=%d", cfg->k);
    if (cfg->precision != PDSC_PRECISION_H3 && cfg->precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision=%d (PDSC_PRECISION_H3 or PDSC_PRECISION_F32)", cfg->precision);
    return PDSC_OK;
}

struct Dims {
    int B, N, Npad, S, k, T;
    bool f32;          // PDSC_PRECISION_F32
    EncoderPlan plan;  // the encoder's plan for (B, N, f32)
    TailPlan tail;     // the tail's plan for (B, N, S)
};

// dense_m_caller: the standalone encoder's plan, on the caller's dense M (plan_encoder)
int make_dims(const pdsc_config *cfg, int B, int N, Dims &d, bool dense_m_caller = false) {
    if (B < 1 || N < 2) return fail(PDSC_ERR_ARG, "B=%d N=%d (need B >= 1, N >= 2)", B, N);
    if (N > 32767) return fail(PDSC_ERR_UNSUPPORTED, "N=%d > 32767 (32-bit buffer descriptors over M)", N);
    d.B = B;
    d.N = N;
    d.Npad = round_up(N, QB);
    d.S = (int)((double)N * cfg->ratio);  // int(num_corr * self.ratio) (:174)
    d.k = std::min(cfg->k, N - 1);        // (:250)
    d.T = cfg->num_iterations;
    d.f32 = cfg->precision == PDSC_PRECISION_F32;
    d.plan = plan_encoder(B, N, d.f32, dense_m_caller);
    d.tail = plan_tail(B, N, d.S);
    if (d.S < 1) return fail(PDSC_ERR_ARG, "int(N*ratio) = 0 seeds for N=%d", N);
    if (d.k > 63) return fail(PDSC_ERR_UNSUPPORTED, "k=%d > 63", d.k);
    return PDSC_OK;
}

struct EncBufs {
    float *feat, *opart, *ml, *vexp, *vexp2;
    float *feat2;            // the split path's second feat buffer (pw_mid reads one, writes the other), else null
    _Float16 *q, *k, *v;     // attention_h3 split layouts (hi + lo per element), or fp32 rows (F32)
    _Float16 *q2, *k2, *v2;  // the other Q/K/V set of the fused path (layers alternate), else null
    float *opart1, *ml1;     // the combined split (EncoderPlan::precombine), else null
};

EncBufs carve_encoder(Carve &c, const Dims &d) {
    EncBufs e;
    const size_t rows = (size_t)d.B * d.Npad * CH;
    e.feat = c.take<float>(rows);
    e.q = c.take<_Float16>(2 * rows);
    e.k = c.take<_Float16>(2 * rows);
    e.v = c.take<_Float16>(2 * rows);
    e.opart = c.take<float>(rows * d.plan.nsplit);
    e.ml = c.take<float>((size_t)d.B * d.Npad * d.plan.nsplit * 2);
    e.vexp = c.take<float>((size_t)d.B * (d.Npad / 32));
    e.opart1 = d.plan.precombine ? c.take<float>(rows) : nullptr;
    e.ml1 = d.plan.precombine ? c.take<float>((size_t)d.B * d.Npad * 2) : nullptr;
    e.q2 = e.k2 = e.v2 = nullptr;
    e.vexp2 = nullptr;
    // pw_mid's three Q / K / V workgroups per point tile all read the layer's
    // residual rows while one of them writes the new PointCN rows: the rows
    // ping-pong between feat and feat2 so no workgroup overwrites what another
    // still reads
    e.feat2 = d.plan.fused() ? nullptr : c.take<float>(rows);
    if (d.plan.fused()) {
        e.q2 = c.take<_Float16>(2 * rows);
        e.k2 = c.take<_Float16>(2 * rows);
        e.v2 = c.take<_Float16>(2 * rows);
        e.vexp2 = c.take<float>((size_t)d.B * (d.Npad / 32));
    }
    return e;
}

// M: in the plan's layout (d.plan.m_layout)
int run_encoder(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M, const Dims &d,
                const EncBufs &e, float *feat_out, float *normed, _Float16 *normed_s, float *conf, hipStream_t s,
                Ragged rg = {}) {
    const EncoderPlan plan = d.plan.for_ragged(rg);
    HIPCHK(launch_pw_first(plan, packed, lay, corr_pos, e.feat, e.q, e.k, e.v, e.vexp, s, rg));
    if (plan.fused()) {  // every layer fused (0 .. L-2 with the next layer's PointCN/QKV, Q/K/V alternating between the two sets)
        _Float16 *q = e.q, *k = e.k, *v = e.v, *q2 = e.q2, *k2 = e.k2, *v2 = e.v2;
        float *vx = e.vexp, *vx2 = e.vexp2;
        for (int l = 0; l + 1 < lay.L; ++l) {
            const bool timed = g_tcap > 0 && g_tcount && *g_tcount < g_tcap;
            if (timed) HIPCHK(hipEventRecord(g_tstart[*g_tcount], s));
            HIPCHK(launch_attn_pw2(plan, packed, lay, l, q, k, v, vx, M, e.feat, q2, k2, v2, vx2, s, rg));
            if (timed) HIPCHK(hipEventRecord(g_tstop[(*g_tcount)++], s));
            std::swap(q, q2);
            std::swap(k, k2);
            std::swap(v, v2);
            std::swap(vx, vx2);
        }
        HIPCHK(launch_attn_pw2_last(plan, packed, lay, q, k, v, vx, M, e.feat, feat_out, normed, normed_s, conf, s, rg));
        return PDSC_OK;
    }
    float *feat = e.feat, *feat_alt = e.feat2;
    for (int l = 0; l < lay.L; ++l) {
        const bool timed = g_tcap > 0 && g_tcount && *g_tcount < g_tcap;
        if (timed) HIPCHK(hipEventRecord(g_tstart[*g_tcount], s));
        HIPCHK(launch_attention(plan, e.q, e.k, e.v, e.vexp, M, e.opart, e.ml, s, rg, l));
        if (timed) HIPCHK(hipEventRecord(g_tstop[(*g_tcount)++], s));
        const float *op = e.opart, *mlp = e.ml;
        int ns = plan.nsplit;
        if (plan.precombine) {
            HIPCHK(launch_combine_rows(e.opart, e.ml, d.B, d.Npad, plan.nsplit, e.opart1, e.ml1, s));
            op = e.opart1;
            mlp = e.ml1;
            ns = 1;
        }
        if (l + 1 < lay.L) {
            HIPCHK(launch_pw_mid(plan, packed, lay, l, op, mlp, ns, feat, feat_alt, e.q, e.k, e.v, e.vexp, s));
            std::swap(feat, feat_alt);
        } else {
            HIPCHK(launch_pw_last(plan, packed, lay, op, mlp, ns, feat, feat_out, normed, d.f32 ? nullptr : normed_s,
                                  conf, s));
        }
    }
    return PDSC_OK;
}

// Ragged batches run the fused encoder as P parts of the batch (contiguous pair
// ranges of equal pair counts), each on its own
// stream -- the caller's and P - 1 per-device side streams, forked and joined
// by events -- so one part's launches fill the others' dispatch tails: a ragged
// batch's attention launches end in a tail of a few long workgroups per XCD
// (DESIGN.md §7).  Pairs are independent through the encoder, so each part is
// the same arithmetic on its own pointer range (bitwise equal results).
// 128 pairs, N in [700, 1300], two halves: 4.54 -> 4.12 ms per forward (three
// parts 4.23, four 4.32 vs two 4.19 on another box); uniform batches (two full
// rounds of workgroups, no tail to fill) measured 3.77 -> 3.83 ms, so they stay
// on one stream.  Knobs: PDSC_ENC_HALVES 0 never, 1 uniform batches too;
// PDSC_ENC_PARTS P in [2, 4] (default 2).  Every part keeps the whole batch's
// plan (the fused launches' one key split, pw2_first's layouts).
static bool enc_halves(const Dims &d, bool ragged) {
    const Knobs &k = knobs();
    return d.plan.fused() && d.B >= 16 * k.enc_parts && (k.enc_halves == 1 || (k.enc_halves != 0 && ragged));
}
// Part boundaries bounds[0 .. P]: bounds[i] = the first pair whose work prefix
// reaches i/P of the total (counts: HOST sizes, or NULL for a uniform batch).
static void enc_bounds(const int32_t *counts, int B, int P, int *bounds) {
    std::vector<double> pre(B + 1, 0.0);
    for (int b = 0; b < B; ++b) pre[b + 1] = pre[b] + (counts ? (double)counts[b] * counts[b] : 1.0);
    bounds[0] = 0;
    bounds[P] = B;
    for (int i = 1; i < P; ++i) {
        const double goal = pre[B] * i / P;
        int h = bounds[i - 1] + 1;
        while (h < B - (P - i) && std::abs(pre[h + 1] - goal) < std::abs(pre[h] - goal)) ++h;
        bounds[i] = h;
    }
}

struct SideStream {
    std::mutex mu;  // one fork / join enqueued at a time per device
    hipStream_t s2[ENC_MAX_PARTS - 1] = {};
    hipEvent_t fork = nullptr, join[ENC_MAX_PARTS - 1] = {};
    bool ok = false;
};
// The side streams of the device that stream s runs on (the current device for
// the legacy default stream), created there on first use.
static SideStream *side_stream(hipStream_t s) {
    static SideStream ss[64];
    hipDevice_t dev = 0;
    if (!s || hipStreamGetDevice(s, &dev) != hipSuccess)
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (dev < 0 || dev >= 64) return nullptr;
    SideStream &x = ss[dev];
    static std::mutex create_mu;
    std::lock_guard<std::mutex> lock(create_mu);
    if (!x.ok) {  // all or none (a failure leaves the forward on one stream)
        int cur = dev;
        if (hipGetDevice(&cur) != hipSuccess || (cur != dev && hipSetDevice(dev) != hipSuccess)) return nullptr;
        bool ok = x.fork || hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < ENC_MAX_PARTS - 1; ++i) {
            if (!x.s2[i]) ok = hipStreamCreateWithFlags(&x.s2[i], hipStreamNonBlocking) == hipSuccess;
            if (ok && !x.join[i]) ok = hipEventCreateWithFlags(&x.join[i], hipEventDisableTiming) == hipSuccess;
        }
        if (cur != dev) (void)hipSetDevice(cur);
        x.ok = ok;
    }
    return x.ok ? &x : nullptr;
}

// The fused plan's encoder over pairs [b0, b0 + nb): every per-pair pointer
// moved to pair b0 (the pair-major layouts of carve_encoder / carve_forward).
static int run_encoder_part(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                            const Dims &d, const EncBufs &e, float *normed, _Float16 *normed_s, float *conf,
                            hipStream_t s, Ragged rg, int b0, int nb) {
    Dims dh = d;
    dh.B = nb;
    dh.plan = d.plan.for_pairs(nb);  // the batch's plan, not nb pairs' own
    const size_t rows = (size_t)b0 * d.Npad * CH;
    EncBufs eh = e;
    eh.feat = e.feat + rows;
    eh.q = e.q + 2 * rows;
    eh.k = e.k + 2 * rows;
    eh.v = e.v + 2 * rows;
    eh.q2 = e.q2 + 2 * rows;
    eh.k2 = e.k2 + 2 * rows;
    eh.v2 = e.v2 + 2 * rows;
    eh.vexp = e.vexp + (size_t)b0 * (d.Npad / 32);
    eh.vexp2 = e.vexp2 + (size_t)b0 * (d.Npad / 32);
    const size_t mstr = d.plan.m_layout == M_PACKED ? mpack_floats(d.N) : (size_t)d.N * d.N;
    Ragged rh = rg;
    if (rg.nv) rh.nv = rg.nv + b0;
    if (rg.sv) rh.sv = rg.sv + b0;
    if (rg.po) rh.po = rg.po + b0;
    return run_encoder(lay, packed, corr_pos + (size_t)b0 * d.N * lay.in_dim, M + (size_t)b0 * mstr, dh, eh, nullptr,
                       normed + (size_t)b0 * d.N * CH, normed_s + (size_t)b0 * d.N * 2 * CH, conf + (size_t)b0 * d.N, s,
                       rh);
}

// run_encoder for the forward: the fused plan as P concurrent parts given side
// streams ss and the part boundaries (enc_halves / enc_bounds; rg.po, when set,
// must then order each part's pairs on its own: launch_ragged_order per part),
// else run_encoder itself.
static int run_encoder_fwd(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                           const Dims &d, const EncBufs &e, float *normed, _Float16 *normed_s, float *conf,
                           hipStream_t s, Ragged rg, SideStream *ss, const int *bounds, int P) {
    if (!ss) return run_encoder(lay, packed, corr_pos, M, d, e, nullptr, normed, normed_s, conf, s, rg);
    std::lock_guard<std::mutex> lock(ss->mu);
    // The side streams are shared by every caller stream of the device.  A side
    // stream forked into another thread's graph capture stays in that capture
    // until it ends: enqueueing there from a stream outside that capture would
    // record into (or invalidate) the other graph, so such a call runs on one
    // stream (bitwise the same results).
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone, c2 = hipStreamCaptureStatusNone;
        unsigned long long id = 0, id2 = 0;
        HIPCHK(hipStreamGetCaptureInfo(s, &cs, &id));
        for (int i = 1; i < P; ++i) {
            HIPCHK(hipStreamGetCaptureInfo(ss->s2[i - 1], &c2, &id2));
            if (c2 != hipStreamCaptureStatusNone && (cs != hipStreamCaptureStatusActive || id2 != id))
                return run_encoder(lay, packed, corr_pos, M, d, e, nullptr, normed, normed_s, conf, s, rg);
        }
    }
    HIPCHK(hipEventRecord(ss->fork, s));
    int forked = 1, r = PDSC_OK;
    for (; forked < P; ++forked)
        if (hipStreamWaitEvent(ss->s2[forked - 1], ss->fork, 0) != hipSuccess) {
            r = fail(PDSC_ERR_HIP, "hipStreamWaitEvent (fork)");
            break;
        }
    for (int i = 0; r == PDSC_OK && i < P; ++i)
        r = run_encoder_part(lay, packed, corr_pos, M, d, e, normed, normed_s, conf, i ? ss->s2[i - 1] : s, rg,
                             bounds[i], bounds[i + 1] - bounds[i]);
    // join every side stream that was forked, on success AND on error: the
    // caller's stream must not run ahead of work a side stream may still do in
    // the workspace, and a capture must not end with an unjoined fork
    for (int i = 1; i < forked; ++i) {
        const hipError_t a = hipEventRecord(ss->join[i - 1], ss->s2[i - 1]);
        const hipError_t b = a == hipSuccess ? hipStreamWaitEvent(s, ss->join[i - 1], 0) : a;
        if (b != hipSuccess && r == PDSC_OK) r = fail(PDSC_ERR_HIP, "join: %s", hipGetErrorString(b));
    }
    return r;
}

struct FwdBufs {
    int *range;  // [B] the fp16 range guard's per-pair flags: the workspace's first bytes (pdsc_range_status)
    float *M, *normed, *conf, *lm, *kdist, *seed_trans, *weights, *hsums;
    _Float16 *normed_s;
    int *seeds, *knn, *counts;
    int *nv, *sv, *po;  // ragged batches: per-pair correspondences and seeds, attention pair order
    EncBufs enc;
    NsmBufs nsm;
};

FwdBufs carve_forward(Carve &c, const Dims &d) {
    FwdBufs f;
    f.range = c.take<int>((size_t)d.B);  // first: at the workspace's base
    // symmetric-packed tiles (PDSC_DENSE_M=1: the dense [N][N] form, for A/B measurement)
    f.M = c.take<float>((size_t)d.B * std::max(mpack_floats(d.N), (size_t)d.N * d.N));  // packed or dense
    f.enc = carve_encoder(c, d);
    f.normed = c.take<float>((size_t)d.B * d.N * CH);
    f.normed_s = c.take<_Float16>((size_t)d.B * d.N * 2 * CH);
    f.conf = c.take<float>((size_t)d.B * d.N);
    f.lm = c.take<float>((size_t)d.B * d.N);
    f.seeds = c.take<int>((size_t)d.B * d.S);
    f.kdist = c.take<float>((size_t)d.B * d.S * d.N);
    f.knn = c.take<int>((size_t)d.B * d.S * d.k);
    f.nsm = carve_nsm(c, d.B, d.S, d.k, d.T);
    f.weights = f.nsm.weights;
    f.seed_trans = c.take<float>((size_t)d.B * d.S * 16);
    f.counts = c.take<int>((size_t)d.B * d.S);
    f.hsums = c.take<float>((size_t)d.B * d.S * 15);
    f.nv = c.take<int>((size_t)d.B);
    f.sv = c.take<int>((size_t)d.B);
    f.po = c.take<int>((size_t)d.B);
    return f;
}

}  // namespace

extern "C" {

const char *pdsc_version(void) { return "pdsc 0.1.0 gfx950"; }
const char *pdsc_last_error(void) { return g_err.c_str(); }

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
        HIPCHK(launch_fold_vm(P[b + 6], P[b + 7], P[b + 24], P[b + 25], wm, bm, s));
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

// ---------------------------------------------------------------- a2-a4
// (the standalone encoder takes the caller's dense M: make_dims' dense_m_caller)
size_t pdsc_encoder_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N) {
    Dims d;
    if (check_cfg(cfg) != PDSC_OK || make_dims(cfg, B, N, d, true) != PDSC_OK) return 0;
    Carve c(nullptr);
    carve_encoder(c, d);
    return c.off;
}

int32_t pdsc_encoder_f32(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                         const float *M, int32_t B, int32_t N, float *feat, float *normed, float *conf,
                         void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_cfg(cfg));
    Dims d;
    RET_IF(make_dims(cfg, B, N, d, true));
    if (!packed || !corr_pos || !M || !normed || !conf || !ws) return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_encoder_workspace_bytes(cfg, B, N)));
    Carve c(ws);
    const EncBufs e = carve_encoder(c, d);
    const PackLayout lay = make_layout(cfg->num_layers, cfg->in_dim);
    return run_encoder(lay, packed, corr_pos, M, d, e, feat, normed, nullptr, conf, S_(stream));
}

size_t pdsc_attention_workspace_bytes(int32_t B, int32_t N, int32_t C, int32_t precision) {
    if (C != CH || B < 1 || N < 1 || (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)) return 0;
    const int Npad = round_up(N, QB), ns = plan_encoder(B, N, precision == PDSC_PRECISION_F32, true, false).nsplit;
    Carve c(nullptr);
    for (int i = 0; i < 3; ++i) c.take<_Float16>((size_t)2 * B * Npad * CH);
    c.take<float>((size_t)B * Npad * CH * ns);
    c.take<float>((size_t)B * Npad * ns * 2);
    c.take<float>((size_t)B * (Npad / 32));
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
    const int Npad = plan.Npad, ns = plan.nsplit;
    Carve c(ws);
    _Float16 *qs = c.take<_Float16>((size_t)2 * B * Npad * CH);
    _Float16 *ks = c.take<_Float16>((size_t)2 * B * Npad * CH);
    _Float16 *vs = c.take<_Float16>((size_t)2 * B * Npad * CH);
    float *op = c.take<float>((size_t)B * Npad * CH * ns);
    float *ml = c.take<float>((size_t)B * Npad * ns * 2);
    float *vexp = c.take<float>((size_t)B * (Npad / 32));
    if (f32) {  // the caller's rows, zero-padded to Npad rows (the same bytes as the split layouts)
        HIPCHK(launch_pad_rows(q, B, N, Npad, reinterpret_cast<float *>(qs), s));
        HIPCHK(launch_pad_rows(k, B, N, Npad, reinterpret_cast<float *>(ks), s));
        HIPCHK(launch_pad_rows(v, B, N, Npad, reinterpret_cast<float *>(vs), s));
    } else {  // the caller's fp32 [B][N][C] rows -> the kernel's padded fp16 hi/lo layouts
        HIPCHK(launch_split_qkv(q, k, v, B, N, N, Npad, qs, ks, vs, vexp, s));
    }
    HIPCHK(launch_attention(plan, qs, ks, vs, vexp, M, op, ml, s));
    HIPCHK(launch_attn_combine(op, ml, f32, B, N, Npad, ns, msg, s));
    return PDSC_OK;
}

int32_t pdsc_attention_timing(void *const *start_events, void *const *stop_events, int32_t capacity,
                              int32_t *count) {
    if (capacity > 0 && (!start_events || !stop_events || !count))
        return fail(PDSC_ERR_ARG, "null events/count with capacity %d", capacity);
    g_tstart = reinterpret_cast<hipEvent_t *>(const_cast<void **>(start_events));
    g_tstop = reinterpret_cast<hipEvent_t *>(const_cast<void **>(stop_events));
    g_tcap = capacity;
    g_tcount = count;
    return PDSC_OK;
}

int32_t pdsc_diag_qkv_delay(int32_t loops) {
    if (loops < 0) return fail(PDSC_ERR_ARG, "loops=%d", loops);
    g_diag_qkv_delay = loops;
    return PDSC_OK;
}

int32_t pdsc_forward_timing(void *const *events, int32_t capacity, int32_t *count) {
    if (capacity > 0 && (!events || !count)) return fail(PDSC_ERR_ARG, "null events/count with capacity %d", capacity);
    g_fev = reinterpret_cast<hipEvent_t *>(const_cast<void **>(events));
    g_fcap = capacity;
    g_fcount = count;
    return PDSC_OK;
}

int32_t pdsc_attention_layout(int32_t B, int32_t N, int32_t precision, int32_t *Npad, int32_t *nsplit) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !Npad || !nsplit) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    const EncoderPlan plan = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false);
    *Npad = plan.Npad;
    *nsplit = plan.nsplit;
    return PDSC_OK;
}

int32_t pdsc_encoder_plan(int32_t B, int32_t N, int32_t precision, int32_t *fused) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !fused) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    const EncoderPlan plan = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false);
    *fused = plan.fused() ? 1 : (plan.w64() ? 2 : 0);
    return PDSC_OK;
}

int32_t pdsc_encoder_plan_vfold(int32_t B, int32_t N, int32_t precision, int32_t *vfold) {
    if (precision != PDSC_PRECISION_H3 && precision != PDSC_PRECISION_F32)
        return fail(PDSC_ERR_ARG, "precision %d (enum pdsc_precision)", precision);
    if (B < 1 || N < 1 || !vfold) return fail(PDSC_ERR_ARG, "B=%d N=%d", B, N);
    *vfold = plan_encoder(B, N, precision == PDSC_PRECISION_F32, false).vfold ? 1 : 0;
    return PDSC_OK;
}

int32_t pdsc_launch_plan(const pdsc_config *cfg, int32_t B, int32_t N, int32_t *out, int32_t capacity) {
    RET_IF(check_cfg(cfg));
    Dims d;
    RET_IF(make_dims(cfg, B, N, d));
    if (!out || capacity < PDSC_LAUNCH_PLAN_FIELDS)
        return fail(PDSC_ERR_ARG, "out=%p capacity=%d (need %d)", (void *)out, capacity, PDSC_LAUNCH_PLAN_FIELDS);
    const EncoderPlan &p = d.plan;
    const TailPlan &t = d.tail;
    const int32_t row[PDSC_LAUNCH_PLAN_FIELDS] = {p.pw2,         p.pw_tile,   p.pw_mid8, p.pw_first_qkv3, p.pw_mid_qkv3,
                                                  p.pw_prefetch, t.seed_rows, t.nms_rpt, (int32_t)t.rank, t.wpb,
                                                  t.knn_bitonic, t.kabsch_fused, t.tail_fused};
    std::copy(row, row + PDSC_LAUNCH_PLAN_FIELDS, out);
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

// --------------------------------------------------------------- forward
size_t pdsc_forward_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N) {
    Dims d;
    if (check_cfg(cfg) != PDSC_OK || make_dims(cfg, B, N, d) != PDSC_OK) return 0;
    Carve c(nullptr);
    carve_forward(c, d);
    return c.off;
}

int32_t pdsc_forward_testing(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                             const float *src, const float *tgt, int32_t B, int32_t N, float *final_trans,
                             float *final_labels, float *conf_out, int32_t *seeds_out, void *ws,
                             size_t ws_bytes, pdsc_stream_t stream) {
    pdsc_forward_debug dbg{};
    dbg.conf = conf_out;
    dbg.seeds = seeds_out;
    return pdsc_forward_testing_debug(cfg, packed, corr_pos, src, tgt, B, N, final_trans, final_labels, &dbg, ws,
                                      ws_bytes, stream);
}

// The testing forward of B pairs; counts (HOST, may be NULL) makes it ragged:
// pair b uses the first counts[b] rows of its N-row buffers.
static int32_t forward_testing_impl(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                                    const float *src, const float *tgt, int32_t B, int32_t N, const int32_t *counts,
                                    float *final_trans, float *final_labels, const pdsc_forward_debug *dbg, void *ws,
                                    size_t ws_bytes, pdsc_stream_t stream) {
    const pdsc_forward_debug no{};
    if (!dbg) dbg = &no;
    RET_IF(check_cfg(cfg));
    Dims d;
    RET_IF(make_dims(cfg, B, N, d));
    if (!packed || !corr_pos || !src || !tgt || !final_trans || !final_labels || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    if (counts)
        for (int b = 0; b < B; ++b) {
            // every pair must keep the batch's k = min(cfg k, N - 1) and have >= 1 seed
            const int n = counts[b];
            if (n < 2 || n > N || std::min(cfg->k, n - 1) != d.k || (int)((double)n * cfg->ratio) < 1)
                return fail(PDSC_ERR_ARG, "counts[%d] = %d: need k + 1 = %d <= count <= N = %d and int(count * ratio) >= 1",
                            b, n, d.k + 1, N);
        }
    RET_IF(need_ws(ws_bytes, pdsc_forward_workspace_bytes(cfg, B, N)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    const FwdBufs f = carve_forward(c, d);
    Ragged rg;
    SideStream *halves = enc_halves(d, counts != nullptr) ? side_stream(s) : nullptr;
    const int parts = halves ? knobs().enc_parts : 1;
    int bounds[ENC_MAX_PARTS + 1] = {0, B};
    if (halves) enc_bounds(knobs().enc_bal ? counts : nullptr, B, parts, bounds);
    if (counts) {
        HIPCHK(launch_ragged_setup(counts, B, cfg->ratio, f.nv, f.sv, s));
        rg.nv = f.nv;
        rg.sv = f.sv;
        rg.eq = std::all_of(counts, counts + B, [N](int32_t n) { return n == N; });
        if (knobs().ragged_order) {  // each part's attention launches order that part's pairs
            for (int i = 0; i < parts; ++i)
                HIPCHK(launch_ragged_order(counts + bounds[i], bounds[i + 1] - bounds[i], f.po + bounds[i], s));
            rg.po = f.po;
        }
    }
    const PackLayout lay = make_layout(cfg->num_layers, cfg->in_dim);
    const float *sigma = packed + lay.sigma, *sigma_d = packed + lay.sigma_d;
    const bool timed = g_fcap > 0 && g_fcount && *g_fcount + PDSC_FORWARD_STAGES + 1 <= g_fcap;
    hipEvent_t *ev = timed ? g_fev + *g_fcount : nullptr;
    if (timed) *g_fcount += PDSC_FORWARD_STAGES + 1;
#define STAGE(i) \
    if (ev) HIPCHK(hipEventRecord(ev[i], s))
    STAGE(0);
    // a1 (:150-153).  (r04: a1 on a second stream beside the encoder's first
    // launch measured no gain at 128 x 1000 / 8 x 5000 and +44 us per single
    // pair -- the cross-stream event pair -- so the forward stays on one stream.)
    if (d.plan.m_layout == M_PACKED)
        HIPCHK(launch_compat_packed(src, tgt, d.B, d.N, sigma_d, f.M, s, rg));
    else
        HIPCHK(launch_compat(src, tgt, d.B, d.N, sigma_d, f.M, s, rg));
    STAGE(1);
    // a2-a4 (:155-156, :171)
    RET_IF(run_encoder_fwd(lay, packed, corr_pos, f.M, d, f.enc, f.normed, f.normed_s, f.conf, s, rg, halves,
                           bounds, parts));
    STAGE(2);
    // a5 (:174)
    HIPCHK(launch_local_max(d.tail, src, f.conf, d.B, d.N, cfg->nms_radius, f.lm, s, rg));
    // (kdist, written by the seed kNN next, is the ranking's scratch)
    HIPCHK(launch_seed_rank(d.tail, f.conf, f.lm, d.B, d.N, d.S, f.seeds, s, rg,
                            reinterpret_cast<uint32_t *>(f.kdist)));
    STAGE(3);
    // a6 (:250-252)
    RET_IF(run_seed_knn(d.tail, f.normed, f.normed_s, d.f32, f.seeds, d.B, d.N, d.S, d.k, f.kdist, f.knn, s, rg));
    STAGE(4);
    // a7-a8 (:257-282)
    // per pair: each pair is its own bs = 1 forward, whose allclose spans its S seeds.
    // The power iterates here; nsm_finish's step (t*, the normalised weights) runs
    // inside the hypotheses' first launch below (the same bits, one launch fewer).
    const bool tail = d.tail.tail_fused;
    if (!tail) {
        RET_IF(run_nsm(d.tail, f.normed, f.normed_s, d.f32, src, tgt, f.knn, d.B, d.N, d.S, d.k, d.T, sigma, sigma_d,
                       f.nsm, f.weights, nullptr, false, s, rg));
    } else if (d.T > 0)
        HIPCHK(launch_nsm_seed(d.tail,
                               d.f32 ? static_cast<const void *>(f.normed) : static_cast<const void *>(f.normed_s),
                               d.f32, src, tgt, f.knn, d.B, d.N, d.S, d.k, d.T, sigma, sigma_d, f.nsm.hist, f.nsm.mask,
                               s, rg));
    STAGE(5);
    // a9-a10 (:280-282, :287-335)
    HIPCHK(launch_hypotheses(d.tail, src, tgt, f.knn, f.weights, d.B, d.N, d.S, d.k, cfg->inlier_threshold,
                             f.seed_trans, f.counts, f.hsums, s, rg, tail ? f.nsm.hist : nullptr, f.nsm.mask, d.T,
                             f.weights));
    if (dbg->trans_pre_refine || !tail) {  // the pose before refinement: the two launches
        HIPCHK(launch_select_best(src, tgt, f.seed_trans, f.counts, d.B, d.N, d.S, cfg->inlier_threshold,
                                  nullptr, nullptr, final_trans, final_labels, s, rg, f.conf, f.range));
        if (dbg->trans_pre_refine)
            HIPCHK(hipMemcpyAsync(dbg->trans_pre_refine, final_trans, sizeof(float) * 16 * d.B, hipMemcpyDeviceToDevice,
                                  s));
        STAGE(6);
        // a11 (:186, :403-438)
        HIPCHK(launch_post_refine(final_trans, src, tgt, d.B, d.N, cfg->refine_threshold, s, rg, f.range));
    } else {
        // a10 best + a11 in one launch (select_best's and post_refine's workgroup
        // bodies back to back; the stage split of the two is then not measured)
        STAGE(6);
        HIPCHK(launch_best_refine(src, tgt, f.seed_trans, f.counts, d.B, d.N, d.S, cfg->inlier_threshold,
                                  cfg->refine_threshold, final_trans, final_labels, s, rg, f.conf, f.range));
    }
    STAGE(7);
#undef STAGE
    if (dbg->conf) HIPCHK(hipMemcpyAsync(dbg->conf, f.conf, sizeof(float) * d.B * d.N, hipMemcpyDeviceToDevice, s));
    if (dbg->seeds) HIPCHK(hipMemcpyAsync(dbg->seeds, f.seeds, sizeof(int) * d.B * d.S, hipMemcpyDeviceToDevice, s));
    if (dbg->knn) HIPCHK(hipMemcpyAsync(dbg->knn, f.knn, sizeof(int) * d.B * d.S * d.k, hipMemcpyDeviceToDevice, s));
    if (dbg->weights)
        HIPCHK(hipMemcpyAsync(dbg->weights, f.weights, sizeof(float) * d.B * d.S * d.k, hipMemcpyDeviceToDevice, s));
    return PDSC_OK;
}

int32_t pdsc_forward_testing_debug(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                                   const float *src, const float *tgt, int32_t B, int32_t N, float *final_trans,
                                   float *final_labels, const pdsc_forward_debug *dbg, void *ws, size_t ws_bytes,
                                   pdsc_stream_t stream) {
    return forward_testing_impl(cfg, packed, corr_pos, src, tgt, B, N, nullptr, final_trans, final_labels, dbg, ws,
                                ws_bytes, stream);
}

int32_t pdsc_forward_testing_ragged(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                                    const float *src, const float *tgt, int32_t B, int32_t N, const int32_t *counts,
                                    float *final_trans, float *final_labels, const pdsc_forward_debug *dbg, void *ws,
                                    size_t ws_bytes, pdsc_stream_t stream) {
    if (!counts) return fail(PDSC_ERR_ARG, "counts is NULL");
    return forward_testing_impl(cfg, packed, corr_pos, src, tgt, B, N, counts, final_trans, final_labels, dbg, ws,
                                ws_bytes, stream);
}


// ------------------------------------------- f3 training-mode forward and loss
size_t pdsc_forward_training_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N) {
    return pdsc_forward_workspace_bytes(cfg, B, N);
}

int32_t pdsc_forward_training(const pdsc_config *cfg, const float *packed, const float *corr_pos, const float *src,
                              const float *tgt, int32_t B, int32_t N, float *final_trans, float *confidence,
                              float *M_out, int32_t *seeds_out, void *ws, size_t ws_bytes, pdsc_stream_t stream) {
    RET_IF(check_cfg(cfg));
    Dims d;
    RET_IF(make_dims(cfg, B, N, d));
    if (!packed || !corr_pos || !src || !tgt || !final_trans || !confidence || !ws)
        return fail(PDSC_ERR_ARG, "null pointer");
    RET_IF(need_ws(ws_bytes, pdsc_forward_training_workspace_bytes(cfg, B, N)));
    hipStream_t s = S_(stream);
    Carve c(ws);
    const FwdBufs f = carve_forward(c, d);
    const PackLayout lay = make_layout(cfg->num_layers, cfg->in_dim);
    const float *sigma = packed + lay.sigma, *sigma_d = packed + lay.sigma_d;
    // a1-a4 as in testing (:150-156, :171)
    if (d.plan.m_layout == M_PACKED)
        HIPCHK(launch_compat_packed(src, tgt, d.B, d.N, sigma_d, f.M, s));
    else
        HIPCHK(launch_compat(src, tgt, d.B, d.N, sigma_d, f.M, s));
    RET_IF(run_encoder(lay, packed, corr_pos, f.M, d, f.enc, nullptr, f.normed, f.normed_s, f.conf, s));
    // the loss's feature-similarity M (:158-163)
    if (M_out)
        HIPCHK(launch_feat_sim(d.f32 ? static_cast<const void *>(f.normed) : static_cast<const void *>(f.normed_s),
                               d.f32, d.B, d.N, sigma, M_out, s));
    // seeds = argsort(confidence, descending)[:, :S] (:176): the ranking with every flag 1
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f.lm), 0x3f800000u, (size_t)d.B * d.N, s));
    HIPCHK(launch_seed_rank(d.tail, f.conf, f.lm, d.B, d.N, d.S, f.seeds, s));
    // a6-a10 as in testing (:182 -> cal_seed_trans), no post-refinement (:185-186)
    // (f.counts: the hypotheses' inlier counts later, the overflow flags here)
    RET_IF(run_seed_knn(d.tail, f.normed, f.normed_s, d.f32, f.seeds, d.B, d.N, d.S, d.k, f.kdist, f.knn, s));
    // the training batch is ONE reference forward: torch.allclose over all B * S seeds (:354)
    RET_IF(run_nsm(d.tail, f.normed, f.normed_s, d.f32, src, tgt, f.knn, d.B, d.N, d.S, d.k, d.T, sigma, sigma_d, f.nsm,
                   f.weights, nullptr, true, s));
    HIPCHK(launch_hypotheses(d.tail, src, tgt, f.knn, f.weights, d.B, d.N, d.S, d.k, cfg->inlier_threshold,
                             f.seed_trans, f.counts, f.hsums, s));
    // the labels of the best hypothesis are not returned in training mode (:189-191): f.lm is scratch
    HIPCHK(launch_select_best(src, tgt, f.seed_trans, f.counts, d.B, d.N, d.S, cfg->inlier_threshold, nullptr,
                              nullptr, final_trans, f.lm, s, {}, f.conf, f.range));
    HIPCHK(hipMemcpyAsync(confidence, f.conf, sizeof(float) * d.B * d.N, hipMemcpyDeviceToDevice, s));
    if (seeds_out) HIPCHK(hipMemcpyAsync(seeds_out, f.seeds, sizeof(int) * d.B * d.S, hipMemcpyDeviceToDevice, s));
    return PDSC_OK;
}

int32_t pdsc_range_status(const void *ws, int32_t B, int32_t *flags, pdsc_stream_t stream) {
    if (!ws || B < 1) return fail(PDSC_ERR_ARG, "ws=%p B=%d", ws, B);
    std::vector<int32_t> h((size_t)B);
    hipStream_t s = S_(stream);
    HIPCHK(hipMemcpyAsync(h.data(), ws, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int bad = 0;
    for (int b = 0; b < B; ++b) {
        if (flags) flags[b] = h[b];
        bad += h[b] != 0;
    }
    if (bad) return fail(PDSC_ERR_RANGE, "%d of %d pairs left the fp16 range (rerun them with PDSC_PRECISION_F32)", bad, B);
    return PDSC_OK;
}

// pdsc_range_poll: one wavefront ORs the B marks and stores (seq << 1) | any into
// a word of coherent page-locked host memory (a system-scope release store);
// the host spins on the word instead of a D2H copy + stream synchronisation
// (the copy alone: 12.6 us on an idle MI355X stream, tools/dropin_breakdown.py).
__global__ __launch_bounds__(64) void range_publish_kernel(const int32_t *__restrict__ range, int B,
                                                           uint32_t *word, uint32_t seq) {
    bool any = false;
    for (int b = threadIdx.x; b < B; b += 64) any |= range[b] != 0;
    const bool m = __ballot(any) != 0;
    if (threadIdx.x == 0) __hip_atomic_store(word, (seq << 1) | (m ? 1u : 0u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

namespace {
struct PollWord {
    uint32_t *host = nullptr, *dev = nullptr;
    uint32_t seq = 0;
    ~PollWord() {
        if (host) (void)hipHostFree(host);
    }
};
thread_local PollWord g_poll;  // one word per host thread: its calls wait one at a time
}  // namespace

int32_t pdsc_range_poll(const void *ws, int32_t B, pdsc_stream_t stream) {
    if (!ws || B < 1) return fail(PDSC_ERR_ARG, "ws=%p B=%d", ws, B);
    hipStream_t s = S_(stream);
    PollWord &w = g_poll;
    if (!w.host) {
        void *h = nullptr, *dp = nullptr;
        HIPCHK(hipHostMalloc(&h, 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
        if (hipHostGetDevicePointer(&dp, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return fail(PDSC_ERR_HIP, "hipHostGetDevicePointer");
        }
        w.host = static_cast<uint32_t *>(h);
        w.dev = static_cast<uint32_t *>(dp);
        __atomic_store_n(w.host, 0u, __ATOMIC_RELEASE);
    }
    w.seq = (w.seq + 1) & 0x7fffffffu;
    if (w.seq == 0) w.seq = 1;  // 0 is the word's initial value
    const uint32_t seq = w.seq;
    hipLaunchKernelGGL(range_publish_kernel, dim3(1), dim3(64), 0, s, static_cast<const int32_t *>(ws), (int)B, w.dev,
                       seq);
    HIPCHK(hipGetLastError());
    // spin ~20 ms at most (the forward's own device time is well below), then
    // block in hipStreamSynchronize: it also reports a faulted stream
    uint32_t v = 0;
    bool seen = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
        v = __atomic_load_n(w.host, __ATOMIC_ACQUIRE);
        if ((v >> 1) == seq) {
            seen = true;
            break;
        }
        __builtin_ia32_pause();
        if ((it & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    if (!seen) {
        HIPCHK(hipStreamSynchronize(s));
        v = __atomic_load_n(w.host, __ATOMIC_ACQUIRE);
        if ((v >> 1) != seq) return fail(PDSC_ERR_HIP, "range word %u after the stream drained (expected %u)", v >> 1, seq);
    }
    if (v & 1u) return fail(PDSC_ERR_RANGE, "a pair of %d left the fp16 range (rerun it with PDSC_PRECISION_F32)", B);
    return PDSC_OK;
}

}  // extern "C"
