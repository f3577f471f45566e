// pdsc_internal.hpp -- launchers and packed-weight layout shared by the
// translation units of libpdsc (not part of the C ABI).
#pragma once
#include <string>
#include "pdsc_common.hpp"
#include "../../include/pdsc.h"

namespace pdsc {

constexpr int CH = 128;       // num_channels implemented by the MFMA kernels
constexpr int CH2 = CH / 2;   // fc_message hidden width (models/PointDSC.py:12-20)
constexpr int CLS = 32;       // classifier hidden width (models/PointDSC.py:107-113)
constexpr int QB = 128;       // queries per attention workgroup (4 waves x 32)
constexpr int KT = 32;        // keys per attention tile
constexpr int PT = 64;        // points per pointwise workgroup

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// a launcher's early return on a HIP error
#define HIP_RET(expr)                      \
    do {                                      \
        hipError_t e_ = (expr);               \
        if (e_ != hipSuccess) return e_;      \
    } while (0)

// workspace.hpp: the bump allocator every stage's layout function takes
struct Carve;

// ---- symmetric-packed M (the forward's a1 output) -------------------------
// M is symmetric bit-for-bit, so the forward stores only its upper-triangle
// MPACK_T x MPACK_T tiles, each contiguous and row-major, enumerated row by
// row: tile (ti, tj), ti <= tj, at index ti*nt - ti*(ti-1)/2 + (tj - ti),
// nt = ceil(N / MPACK_T).  M[i][j] for i > j lives transposed in tile (tj, ti).
constexpr int MPACK_T = 32;  // = the attention's per-wave 32 keys x 32 queries block
__host__ __device__ inline int mpack_ntile(int N) { return (N + MPACK_T - 1) / MPACK_T; }
__host__ __device__ inline size_t mpack_floats(int N) {
    const size_t nt = mpack_ntile(N);
    return nt * (nt + 1) / 2 * MPACK_T * MPACK_T;
}
__host__ __device__ inline int mpack_tile(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

// fp16 planes per packed 1x1-conv weight (3xfp16 mode): 2 = hi + mid (22
// significant bits, products wh.xh + wh.xl + wm.xh: 3 MFMAs, as the attention's);
// 3 = hi + mid + lo (every fp32 weight exactly, 4 MFMAs; the r01-r03 format,
// kept as a build option for A/B: -DPDSC_W_PLANES=3).  r04 measured both on the
// goldens (tools/emulate_conv.py): the same error class, inside the fp32
// realisations' noise.
#ifndef PDSC_W_PLANES
#define PDSC_W_PLANES 2
#endif
constexpr int W_PLANES = PDSC_W_PLANES;
static_assert(W_PLANES == 2 || W_PLANES == 3, "weight planes");

// Weight blocks: block (t, ks) = 32 outputs x one 16-input k-step, planes
// hi / mid (/ lo) of 64 lanes x 8 halfs (1 KiB) each, blocks t-major.
// Element (o, c) of plane p sits at w3_index(o, c, in) + 512 p (halfs), with
// lane (h, n), n = o % 32, holding positions 8h .. 8h+7 of the k-step in
// qk_pos order (bits 2 and 3 of c % 16 swapped).
constexpr int W3_BLOCK = W_PLANES * 512;  // halfs per block
__host__ __device__ inline size_t w3_index(int o, int c, int in) {
    const int t = o >> 5, n = o & 31, ks = c >> 4, q = c & 15;
    const int pos = (q & ~12) | ((q & 4) << 1) | ((q & 8) >> 1);
    return ((size_t)t * (in / 16) + ks) * W3_BLOCK + (size_t)(32 * (pos >> 3) + n) * 8 + (pos & 7);
}

// ---- packed weights --------------------------------------------------------
// A "dense" layer (Conv1d k=1 [+BN] [+ReLU]) is stored as
//   W  : OUT*IN floats in MFMA fragment order:
//        Wpk[((jt*(IN/8) + g)*64 + lane)*4 + e] = W[jt*32 + (lane&31)][(lane>>5)*(IN/2) + 4g + e]
//   bias[OUT], alpha[OUT], beta[OUT]   (alpha=1, beta=0 when no BN)
// A dense layer in the packed blob: W as W_PLANES fp16 planes (hi, mid[, lo] of
// W * 2^s, s chosen per layer so max|W| 2^s <= 2^14) in MFMA-fragment blocks
// (w3_index) occupying W_PLANES/2*out*in floats at w (at least out*in) -- or, for
// PDSC_PRECISION_F32, W itself fp32 [out][in] in the first out*in of them --
// then bias, alpha, beta [out] and scale = {2^-s, 2^s}.
struct DenseOff {
    size_t w, bias, alpha, beta, scale;
};

// vm: the V fold: W0 Wv [CH2][CH] as a dense block with bias
// W0 bv + b0 and fc0's BatchNorm alpha / beta -- the plans with
// EncoderPlan::vfold project V through it and start the message chain at
// fc0's epilogue; the other plans read v and fc0.
struct LayerOff {
    DenseOff pcn, fc0, fc3, fc6, q, k, v, vm;
};

struct PackLayout {
    int L, in_dim;
    size_t sigma, sigma_d;    // header scalars
    size_t l0_w, l0_b;        // layer0 plain [CH][in_dim], bias[CH]
    size_t cls0, cls2;        // DenseOff base of the two classifier dense layers
    DenseOff c0, c2;
    size_t c4_w, c4_b;        // plain [CLS], [1]
    size_t total;
    LayerOff layer[64];
};

inline DenseOff dense_at(size_t &o, int in, int out) {
    DenseOff d;
    d.w = o;
    o += (size_t)out * in * (W_PLANES > 2 ? W_PLANES : 2) / 2;
    d.bias = o;
    o += out;
    d.alpha = o;
    o += out;
    d.beta = o;
    o += out;
    o = (o + 3) & ~size_t(3);
    d.scale = o;
    o += 4;
    return d;
}

inline PackLayout make_layout(int L, int in_dim) {
    PackLayout p{};
    p.L = L;
    p.in_dim = in_dim;
    size_t o = 0;
    p.sigma = 0;
    p.sigma_d = 1;
    o = 16;
    p.l0_w = o;
    o += (size_t)CH * in_dim;
    p.l0_b = o;
    o += CH;
    o = (o + 3) & ~size_t(3);
    for (int l = 0; l < L; ++l) {
        LayerOff &lo = p.layer[l];
        lo.pcn = dense_at(o, CH, CH);
        lo.fc0 = dense_at(o, CH, CH2);
        lo.fc3 = dense_at(o, CH2, CH2);
        lo.fc6 = dense_at(o, CH2, CH);
        lo.q = dense_at(o, CH, CH);
        lo.k = dense_at(o, CH, CH);
        lo.v = dense_at(o, CH, CH);
    }
    p.c0 = dense_at(o, CH, CLS);
    p.c2 = dense_at(o, CLS, CLS);
    p.c4_w = o;
    o += CLS;
    p.c4_b = o;
    o += 4;
    // appended, so that no earlier offset moves: the folded blocks
    for (int l = 0; l < L; ++l) p.layer[l].vm = dense_at(o, CH, CH2);
    p.total = o;
    return p;
}

// ---- ragged batches (pdsc_forward_testing_ragged) ----------------------------
// Every pair's buffers keep the batch stride N (the largest pair); pair b uses
// its first nv[b] rows and has sv[b] = int(nv[b] * ratio) seeds (S = the
// largest).  nv == sv == nullptr: a uniform batch (every pair N rows, S seeds).
struct Ragged {
    const int *nv = nullptr, *sv = nullptr;
    // the attention's pair order (longest pairs first, dealt over the XCDs), or null
    const int *po = nullptr;
    // every count equals the padded N (host-known): the attention takes the
    // uniform batch's form (stream-K on the w64 plan), so such a call is bitwise
    // the uniform entry's (same key partition, same fp32 combine order)
    bool eq = false;
    PDSC_DEV int n(int b, int N) const { return nv ? nv[b] : N; }
    PDSC_DEV int s(int b, int S) const { return sv ? sv[b] : S; }
};
constexpr int RAGGED_CHUNK = 512;  // counts per setup launch (kernel-argument array)
// counts (HOST, already validated) -> nv [B], sv [B] on the device, through
// kernel arguments (no host-to-device copy of pageable memory on the stream)
hipError_t launch_ragged_setup(const int32_t *counts_host, int B, double ratio, int *nv, int *sv, hipStream_t s);
// counts (HOST) -> po [B]: attention workgroup slot -> pair, so the workgroups
// of the largest pairs start first (each XCD's slots in decreasing pair size,
// pairs dealt to the XCD with the least N^2 so far): list scheduling of
// workgroups of unequal length, longest first
hipError_t launch_ragged_order(const int32_t *counts_host, int B, int *po, hipStream_t s);

// ---- launchers --------------------------------------------------------------
hipError_t launch_compat(const float *src, const float *tgt, int B, int N, const float *sigma_d,
                         float *M, hipStream_t s, Ragged rg = {});
// Mp: [B][mpack_floats(N)]
hipError_t launch_compat_packed(const float *src, const float *tgt, int B, int N, const float *sigma_d,
                                float *Mp, hipStream_t s, Ragged rg = {});

// M's layouts: dense [B][N][N], symmetric-packed (mpack_*)
enum MLayout { M_DENSE = 0, M_PACKED = 1 };
// The encoder's and the tail's launchers launch what the call's plans say
// (launch_plan.hpp: plan_encoder, then plan.for_ragged(rg) for a ragged batch;
// plan_tail).
struct EncoderPlan;
struct TailPlan;
// The tail: tp = plan_tail(B, N, S) of the call's own B, N and S.
hipError_t launch_local_max(const TailPlan &tp, const float *src, const float *conf, int B, int N, float radius,
                            float *lm, hipStream_t s, Ragged rg = {});
// scratch: B S N words the ranking may use (the forward's kdist), or null
hipError_t launch_seed_rank(const TailPlan &tp, const float *conf, const float *lm, int B, int N, int S, int *seeds,
                            hipStream_t s, Ragged rg = {}, uint32_t *scratch = nullptr);

// normed_s (unused when f32): normed as [rows][2][128] fp16 hi/lo in qk_pos order; feats: normed_s, or normed when f32
hipError_t launch_split_rows(const float *x, size_t rows, _Float16 *out, hipStream_t s);
int run_seed_knn(const TailPlan &tp, const float *normed, const _Float16 *normed_s, bool f32, const int *seeds, int B,
                 int N, int S, int k, float *dist, int *knn, hipStream_t s, Ragged rg = {});
hipError_t launch_nsm_seed(const TailPlan &tp, const void *feats, bool f32, const float *src, const float *tgt,
                           const int *knn, int B, int N, int S, int k, int T, const float *sigma, const float *sigma_d,
                           float *hist, unsigned *seed_flags, hipStream_t s, Ragged rg = {});
struct NsmBufs {  // a7-a8 (nsm.hip): the iterates [B][S][max(T, 1)][k], per-seed allclose bits, weights [B][S][k]
    float *hist, *weights;
    unsigned *mask;
};
NsmBufs carve_nsm(Carve &c, int B, int S, int k, int T);
int run_nsm(const TailPlan &tp, const float *normed, const _Float16 *normed_s, bool f32, const float *src,
            const float *tgt, const int *knn, int B, int N, int S, int k, int T, const float *sigma, const float *sigma_d,
            const NsmBufs &nb, float *weights, int *iters, bool batch_global, hipStream_t s, Ragged rg = {});
// sums: scratch [B][S][15]
// hist != NULL (the testing forward): the NSM weights are finished inside the
// first launch (nsm_finish's arithmetic, per-pair allclose over hist /
// seed_flags) and written to wout; `weights` is then not read.
hipError_t launch_hypotheses(const TailPlan &tp, const float *src, const float *tgt, const int *knn,
                             const float *weights, int B, int N, int S, int k, float tau, float *seed_trans, int *counts,
                             float *sums, hipStream_t s, Ragged rg = {}, const float *hist = nullptr,
                             const unsigned *seed_flags = nullptr, int T = 0, float *wout = nullptr);
// conf / range (both may be null): the forward's fp16 range guard -- a pair
// whose logits conf[b, :n] hold a non-finite value gets range[b] = 1 (else 0),
// final_trans all NaN and labels 0; post_refine leaves such a pair alone.
hipError_t launch_select_best(const float *src, const float *tgt, const float *seed_trans,
                              const int *counts, int B, int N, int S, float tau, float *fitness,
                              int *best, float *trans, float *labels, hipStream_t s, Ragged rg = {},
                              const float *conf = nullptr, int *range = nullptr);
hipError_t launch_post_refine(float *trans, const float *src, const float *tgt, int B, int N, float thr,
                              hipStream_t s, Ragged rg = {}, const int *range = nullptr);
// launch_select_best (fitness and best not written) + launch_post_refine in one launch
hipError_t launch_best_refine(const float *src, const float *tgt, const float *seed_trans, const int *counts, int B,
                              int N, int S, float tau, float thr, float *trans, float *labels, hipStream_t s,
                              Ragged rg = {}, const float *conf = nullptr, int *range = nullptr);
hipError_t launch_rigid(const float *A, const float *Bp, const float *w, int nb, int n, float *trans,
                        hipStream_t s);

// the training forward's feature-similarity M (training.hip)
// feats: the split normed copy [B][N][2][128] fp16 (H3) or normed [B][N][128] (f32)
hipError_t launch_feat_sim(const void *feats, bool f32, int B, int N, const float *sigma, float *M, hipStream_t s);

// ---- cross-stage pieces --------------------------------------------------------
// A row's entry points, workspace layouts, limits and launch code live in the
// row's file (abi.hpp); declared here is only what a second row calls.

// The uniform grid over a cloud (descriptors.hip), also ICP's target index (icp.hip).
constexpr int GRID_KEY_BITS = 21;  // bits per axis of a grid cell key
struct CloudStats {
    float mn[3], mx[3];
    double centroid[3];
};
struct GridView {  // points sorted by cell key and the occupied cells
    unsigned long long *skey, *ukey;
    int *sidx, *ustart, *ucount, *nruns;
};
struct GridBufs {
    CloudStats *st;
    GridView view;
    int *err;  // [0] extent / cell >= 2^21, [1] a kNN candidate set over capacity
    // build_grid's own scratch: the statistics partials, the unsorted keys and rows, the hipcub temp
    char *stats;
    unsigned long long *key;
    int *idx, *flags;
    void *cub;
    size_t cub_bytes[3];  // of the radix sort, the run-length encode and the scan
};
// the grid's layout over n points: its size is what the carver has advanced by
void bind_grid(Carve &c, int n, GridBufs &G);
size_t grid_workspace_bytes(int n);
hipError_t build_grid(const float *pts, int n, double cell, double half, const GridBufs &G, hipStream_t s);
// the device error flags of a grid pass as a status (abi.hpp: fail), after draining the stream
int grid_status(const GridBufs &G, hipStream_t s);

// The consistency graph and the maximum clique (clique.hip), also TEASER's inlier
// selection (teaser.hip): adj is N rows of ceil(N / 64) 64-bit words.
constexpr int CLIQUE_MAX_N = 8192;                    // one wavefront holds a row in two words per lane
constexpr long long CLIQUE_DEFAULT_BUDGET = 1 << 12;  // expanded nodes per root (DESIGN.md §7 "PMC baseline")
hipError_t launch_consistency_graph(const float *corr_pos, int N, double thr, bool length, unsigned long long *adj,
                                    int *degree, hipStream_t s);
// the clique workspace's layout inside a caller's carver; returns the base launch_max_clique takes as ws
void *reserve_clique(Carve &c, int N);
// exact = false: the greedy lower bound alone
hipError_t launch_max_clique(const unsigned long long *adj, int N, long long budget, bool exact, int *members,
                             pdsc_clique_result *res, float *labels, void *ws, hipStream_t s);

}  // namespace pdsc
