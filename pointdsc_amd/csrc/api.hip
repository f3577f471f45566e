// api.hip -- the forward: the testing and training forwards of include/pdsc.h
// with their timing, range and launch-plan queries, and the error convention
// every entry shares (fail, check_cfg, check_shape).  Nothing else: every row's
// entry points live in the row's file (abi.hpp).
//
// Host-side orchestration only: argument checks, workspace carving and kernel
// launches on the caller's stream.  No allocation, no synchronisation.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "abi.hpp"
#include "encoder.hpp"
#include "launch_plan.hpp"
#include "pdsc_internal.hpp"

using namespace pdsc;

namespace {
thread_local std::string g_err;  // pdsc_last_error
}  // namespace

namespace pdsc {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

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

int check_shape(const pdsc_config *cfg, int B, int N, int &S, int &k) {
    if (B < 1 || N < 2) return fail(PDSC_ERR_ARG, "B=%d N=%d (need B >= 1, N >= 2)", B, N);
    if (N > 32767) return fail(PDSC_ERR_UNSUPPORTED, "N=%d > 32767 (32-bit buffer descriptors over M)", N);
    S = (int)((double)N * cfg->ratio);  // int(num_corr * self.ratio) (:174)
    k = std::min(cfg->k, N - 1);        // (:250)
    if (S < 1) return fail(PDSC_ERR_ARG, "int(N*ratio) = 0 seeds for N=%d", N);
    if (k > 63) return fail(PDSC_ERR_UNSUPPORTED, "k=%d > 63", k);
    return PDSC_OK;
}
}  // namespace pdsc

namespace {

// pdsc_forward_timing: PDSC_FORWARD_STAGES + 1 events per forward call
thread_local hipEvent_t *g_fev = nullptr;
thread_local int g_fcap = 0;
thread_local int32_t *g_fcount = nullptr;

struct Dims {
    int B, N, Npad, S, k, T;
    bool f32;          // PDSC_PRECISION_F32
    EncoderPlan plan;  // the encoder's plan for (B, N, f32)
    TailPlan tail;     // the tail's plan for (B, N, S)
};

int make_dims(const pdsc_config *cfg, int B, int N, Dims &d) {
    RET_IF(check_shape(cfg, B, N, d.S, d.k));
    d.B = B;
    d.N = N;
    d.Npad = round_up(N, QB);
    d.T = cfg->num_iterations;
    d.f32 = cfg->precision == PDSC_PRECISION_F32;
    d.plan = plan_encoder(B, N, d.f32, false);
    d.tail = plan_tail(B, N, d.S);
    return PDSC_OK;
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
    f.enc = carve_encoder(c, d.plan);
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

int32_t pdsc_forward_timing(void *const *events, int32_t capacity, int32_t *count) {
    if (capacity > 0 && (!events || !count)) return fail(PDSC_ERR_ARG, "null events/count with capacity %d", capacity);
    g_fev = reinterpret_cast<hipEvent_t *>(const_cast<void **>(events));
    g_fcap = capacity;
    g_fcount = count;
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
    SideStream *halves = enc_halves(d.plan, counts != nullptr) ? side_stream(s) : nullptr;
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
    RET_IF(run_encoder_fwd(lay, packed, corr_pos, f.M, d.plan, f.enc, f.normed, f.normed_s, f.conf, s, rg, halves,
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
    RET_IF(run_encoder_fwd(lay, packed, corr_pos, f.M, d.plan, f.enc, f.normed, f.normed_s, f.conf, s));
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
