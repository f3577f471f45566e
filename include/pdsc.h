/*
 * pdsc.h -- C ABI of libpdsc.so, the MI355X (gfx950) hot path of PointDSC.
 *
 * Drop-in boundary for the reference's testing-mode forward
 * (models/PointDSC.py:128-197 of AmnonDrory/PointDSC) and the functions it
 * calls.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - Every pointer argument is a DEVICE pointer (hipMalloc / torch CUDA
 *     tensor storage) unless documented otherwise; all tensors are dense,
 *     row-major, fp32 unless stated; index tensors are int32.
 *   - B = number of independent scan pairs processed by one call (the
 *     reference's public forward is bs == 1; B > 1 is the batched API);
 *     N = correspondences per pair (same N for every pair of a call).
 *   - Calls are asynchronous on `stream` (a hipStream_t; NULL = legacy default
 *     stream), never allocate, never synchronise, and never free caller
 *     memory: scratch comes from a caller-allocated workspace whose size the
 *     matching *_workspace_bytes() query returns.  The compute functions keep
 *     no state between calls and may run concurrently on different streams;
 *     the two measurement hooks (pdsc_attention_timing, pdsc_forward_timing)
 *     are per-thread settings read by the calls of the thread that set them.
 *   - Return value: PDSC_OK or an error code; no exception crosses the ABI.
 *     pdsc_last_error() returns a thread-local message for the last failure.
 */
#ifndef PDSC_H_
#define PDSC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *pdsc_stream_t; /* hipStream_t */

enum pdsc_status {
    PDSC_OK = 0,
    PDSC_ERR_ARG = 1,         /* bad shape / null pointer / unsupported hyper-parameter */
    PDSC_ERR_HIP = 2,         /* a HIP runtime call failed (launch error) */
    PDSC_ERR_UNSUPPORTED = 3, /* valid for the reference, not implemented here */
    PDSC_ERR_RANGE = 4,       /* pdsc_range_status: a pair left the fp16 range (below) */
};

/* Arithmetic of the fp32 contractions (the reference computes them in fp32).
 *   PDSC_PRECISION_H3  (default) each fp32 operand is an exact pair hi + lo of
 *                      fp16 values and each product is hi.hi + hi.lo + lo.hi on
 *                      the fp16 matrix cores with fp32 accumulation (22-bit
 *                      operands; 5.3x the fp32 MFMA rate).
 *   PDSC_PRECISION_F32 exact fp32 MFMA (v_mfma_f32_32x32x2_f32) for the 1x1
 *                      convolutions, the attention, the seed kNN and the NSM
 *                      Gram, and libm expf in the softmax: the reference's
 *                      arithmetic, used to bound the H3 mode's error.
 * Everything else (M, NMS, power iteration, Kabsch, verification) is the
 * same code in both modes.                                                   */
enum pdsc_precision {
    PDSC_PRECISION_H3 = 0,
    PDSC_PRECISION_F32 = 1,
};

/* fp16 range guard (PDSC_PRECISION_H3).  The 3xfp16 split is exact only for
 * |x| < 65520: a larger (or non-finite) activation entering a contraction --
 * features, Q / K / V, hidden layers; the encoder's are O(10) for the trained
 * networks -- becomes hi = inf, lo = -inf, and the contraction's output NaN.
 * The encoder's ReLUs propagate NaN (as torch.relu does), so such a pair ends
 * with a non-finite logit; the testing and training forwards then (on the
 * device, asynchronously) mark it in the workspace, set its final_trans to NaN
 * and its final_labels to 0, and skip its post-refinement: never a silent
 * finite result.  After the stream has run the forward, pdsc_range_status
 * reports the marks: PDSC_ERR_RANGE when any pair is marked (flags [B], HOST
 * int32, may be NULL: 1 for a marked pair), else PDSC_OK.  It synchronises
 * `stream` and must be given the forward's workspace and B.  Rerun the marked
 * pairs with PDSC_PRECISION_F32 (pointdsc_amd.PointDSC does that itself).  In
 * PDSC_PRECISION_F32 a mark means a non-finite logit (non-finite inputs), as
 * the reference's fp32 would produce.  pdsc_encoder_f32 has no workspace
 * marks: its conf output carries the NaN.                                    */
int32_t pdsc_range_status(const void *forward_workspace, int32_t B, int32_t *flags, pdsc_stream_t stream);

/* The same answer without the per-pair flags and without a copy: enqueues on
 * `stream` a one-wavefront kernel that writes whether any of the B pairs is
 * marked into a word of coherent page-locked host memory (one per host thread,
 * allocated on first use), and spins on that word until the kernel has run --
 * i.e. until everything enqueued on `stream` before it has completed -- then
 * returns PDSC_OK or PDSC_ERR_RANGE.  After 20 ms of spinning it blocks in
 * hipStreamSynchronize instead (a long queue; a faulted stream is reported as
 * PDSC_ERR_HIP).  The bs = 1 drop-in path (pointdsc_amd.PointDSC.forward) uses
 * it: the reference's forward returns with no host synchronisation at all
 * (models/PointDSC.py:128-197); this one waits only for the guard's answer. */
int32_t pdsc_range_poll(const void *forward_workspace, int32_t B, pdsc_stream_t stream);

/* Hyper-parameters of PointDSC.__init__ (models/PointDSC.py:81-100). */
typedef struct pdsc_config {
    int32_t in_dim;           /* 6 (1 .. 128; the reference's 6, 9, 12, 70) */
    int32_t num_layers;       /* 12 in both release configs */
    int32_t num_channels;     /* 128 (the only width the HIP kernels implement) */
    int32_t num_iterations;   /* power-iteration cap, 10 */
    int32_t k;                /* NSM neighbourhood, 40 (clipped to N-1 per call, :250) */
    double ratio;             /* seed ratio, 0.1: S = int(N * ratio) as Python computes it (:174) */
    float inlier_threshold;   /* tau of :328/:335 */
    float nms_radius;         /* R of :174 */
    float refine_threshold;   /* :415-418: 0.10 if inlier_threshold == 0.10 else 1.2 */
    int32_t precision;        /* enum pdsc_precision; the packed weights must be packed with the same value */
} pdsc_config;

const char *pdsc_version(void);
const char *pdsc_last_error(void);

/* ---------------------------------------------------------------- weights --
 * Packs the reference's parameters (device pointers, in the order of
 * pdsc_param_names()) into the kernels' layout: Conv1d(k=1) weights as fp16
 * hi/lo planes scaled by a per-layer power of two (PDSC_PRECISION_H3) or plain
 * fp32 [out][in] (PDSC_PRECISION_F32); eval BatchNorm turned into the per-channel
 * (alpha, beta) torch-CPU uses (alpha = w / sqrt(var + 1e-5), beta = b - mean*alpha);
 * sigma and sigma_spat copied into the blob header (read on device, no host sync).
 * Replaces: nothing in the reference (it reads nn.Module parameters directly).
 */
int32_t pdsc_param_count(const pdsc_config *cfg);
const char *pdsc_param_name(const pdsc_config *cfg, int32_t i); /* state_dict key */
size_t pdsc_packed_weights_floats(const pdsc_config *cfg);
int32_t pdsc_pack_weights(const pdsc_config *cfg, const float *const *params_host_array,
                          float *packed, pdsc_stream_t stream);

/* ---------------------------------------------------------- a1 compat ------
 * M[b,i,j] = max(0, 1 - (|s_i-s_j| - |t_i-t_j|)^2 / sigma_d^2), bit-exact with
 * torch-CPU fp32.  Replaces models/PointDSC.py:150-153.  sigma_d is read on
 * device from `sigma_d_dev` (the checkpoint's sigma_spat, :98).
 * src,tgt [B,N,3]; M [B,N,N].                                              */
int32_t pdsc_compat_f32(const float *src, const float *tgt, int32_t B, int32_t N,
                        const float *sigma_d_dev, float *M, pdsc_stream_t stream);
/* The forward's form of the same M: the upper triangle of 32 x 32 tiles, each
 * a contiguous row-major 4 KiB block, tile (ti, tj), ti <= tj, at block index
 * ti*nt - ti*(ti-1)/2 + (tj - ti), nt = ceil(N/32); M[i][j] for i > j is
 * element (j%32, i%32) of tile (j/32, i/32); entries past N are 0.
 * Mp: B * pdsc_compat_packed_floats(N) floats.                              */
size_t pdsc_compat_packed_floats(int32_t N);
int32_t pdsc_compat_packed_f32(const float *src, const float *tgt, int32_t B, int32_t N,
                               const float *sigma_d_dev, float *Mp, pdsc_stream_t stream);

/* -------------------------------------------------- a2-a4 encoder ----------
 * SCNonlocal encoder + F.normalize + classification MLP.
 * Replaces models/PointDSC.py:155-156 and :171 (NonLocalNet.forward :65-77,
 * NonLocalBlock.forward :27-45).  corr_pos [B,N,in_dim]; M [B,N,N] (must be
 * symmetric -- the spatial compatibility is; the attention kernel reads it
 * column-wise).  Outputs: feat [B,N,C] (corr_features), normed [B,N,C],
 * conf [B,N] (the classifier logits).                                        */
size_t pdsc_encoder_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N);
int32_t pdsc_encoder_f32(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                         const float *M, int32_t B, int32_t N, float *feat, float *normed,
                         float *conf, void *workspace, size_t workspace_bytes,
                         pdsc_stream_t stream);

/* The attention core of one NonLocalBlock (models/PointDSC.py:36-42) alone:
 * msg[b,i,:] = sum_j softmax_j(M_ij * q_i.k_j / sqrt(C)) v_j, heads = 1.
 * q,k,v [B,N,C]; msg [B,N,C].  C must be 128.  precision: enum pdsc_precision. */
size_t pdsc_attention_workspace_bytes(int32_t B, int32_t N, int32_t C, int32_t precision);
int32_t pdsc_attention_f32(const float *q, const float *k, const float *v, const float *M,
                           int32_t B, int32_t N, int32_t C, int32_t precision, float *msg, void *workspace,
                           size_t workspace_bytes, pdsc_stream_t stream);

/* Training (no reference counterpart: autograd does this work there).  The same
 * attention in exact fp32 -- msg is bit-equal to pdsc_attention_f32(...,
 * PDSC_PRECISION_F32) on the same inputs -- that also writes the row
 * log-sum-exp of the logits X_ij = M_ij q_i.k_j / sqrt(C): lse [B,N].  M must
 * be symmetric and non-negative and carries no gradient.  C must be 128
 * (else PDSC_ERR_ARG).                                                       */
size_t pdsc_attention_lse_workspace_bytes(int32_t B, int32_t N, int32_t C);
int32_t pdsc_attention_lse_f32(const float *q, const float *k, const float *v, const float *M,
                               int32_t B, int32_t N, int32_t C, float *msg, float *lse, void *workspace,
                               size_t workspace_bytes, pdsc_stream_t stream);
/* Its backward: from the forward's inputs, msg and lse, and dmsg [B,N,C] = the
 * gradient of a loss with respect to msg, the gradients dq, dk, dv [B,N,C].
 * P_ij = exp(X_ij - lse_i) is recomputed tile by tile, never stored:
 * D_i = dmsg_i.msg_i, dX_ij = P_ij (dmsg_i.v_j - D_i), dS_ij = M_ij dX_ij /
 * sqrt(C), dq_i = sum_j dS_ij k_j, dk_j = sum_i dS_ij q_i, dv_j = sum_i P_ij
 * dmsg_i.  fp32 throughout, no atomics: two calls on the same inputs are
 * bit-equal.  C must be 128 (else PDSC_ERR_ARG).                            */
size_t pdsc_attention_backward_workspace_bytes(int32_t B, int32_t N, int32_t C);
int32_t pdsc_attention_backward_f32(const float *q, const float *k, const float *v, const float *M,
                                    const float *msg, const float *lse, const float *dmsg, int32_t B, int32_t N,
                                    int32_t C, float *dq, float *dk, float *dv, void *workspace,
                                    size_t workspace_bytes, pdsc_stream_t stream);
/* SpectralMatchingLoss on the features, with its gradients, without an N x N
 * tensor: normed [B,N,C] fp32 rows of unit length, sigma one device float,
 * gt_labels [B,N] (0/1).  s_ij = n_i.n_j, u_ij = 1 - (1 - s_ij) / sigma^2,
 * M_ij = clamp(u_ij, 0, 1), M_ii = 0, gt_ij = (l_i == 1 and l_j == 1 and i != j);
 * balanced != 0 -> mean over pairs of 0.5 sum gt (M-1)^2 / P_b + 0.5 sum !gt
 * M^2 / Q_b with P_b = max(k_b (k_b - 1) - 1, 0) + 1, Q_b = max(N^2 - k_b (k_b -
 * 1) - 1, 0) + 1, k_b the pair's count of labels 1; else mean((M - gt)^2).
 * loss: one device double.  dnormed [B,N,C] fp32 and dsigma (one device double)
 * are dloss/dnormed and dloss/dsigma; both NULL computes the loss alone, one of
 * them NULL is PDSC_ERR_ARG.  The clamp passes the gradient where 0 <= u <= 1
 * (inclusive).  Sums in fp64, no atomics: two calls on the same inputs are
 * bit-equal.  C must be 128 (else PDSC_ERR_UNSUPPORTED; the size query returns 0). */
size_t pdsc_sm_loss_fused_workspace_bytes(int32_t B, int32_t N, int32_t C);
int32_t pdsc_sm_loss_fused_f32(const float *normed, const float *sigma, const float *gt_labels, int32_t B, int32_t N,
                               int32_t C, int32_t balanced, double *loss, float *dnormed /*nullable*/,
                               double *dsigma /*nullable*/, void *workspace, size_t workspace_bytes,
                               pdsc_stream_t stream);

/* The TESTING / TRAINING FORWARD's attention geometry for (B, N): padded rows
 * per pair and the number of key splits (partials opart [B,nsplit,Npad,C],
 * ml [B,nsplit,Npad,2] in the forward workspace).  Both this query and
 * pdsc_encoder_plan describe pdsc_forward_testing(_ragged/_debug) and
 * pdsc_forward_training only: the standalone pdsc_encoder_f32 and
 * pdsc_attention_f32 take a dense M and always run the h3 split-K plan
 * (plan 0 or 1, never 2), whose split count may differ from the one
 * reported here for shapes where the forward picks plan 2.                  */
int32_t pdsc_attention_layout(int32_t B, int32_t N, int32_t precision, int32_t *Npad, int32_t *nsplit);

/* The encoder's launch plan for (B, N, precision) (no reference counterpart):
 * *fused = 1 when every layer but the last runs its attention and the
 * following pointwise chain (fc_message, residual, PointCN, Q/K/V) as ONE
 * launch -- these are then the launches pdsc_attention_timing times -- 0
 * when attention and chain are separate launches, and 2 when they are separate
 * and the attention is the 64-query-wave kernel (one 4-wave workgroup per CU,
 * attention_w64.hpp; the forward's M symmetric-packed as for plans 0/1).    */
int32_t pdsc_encoder_plan(int32_t B, int32_t N, int32_t precision, int32_t *fused);
/* *vfold = 1 when that plan folds fc_message[0] into the V projection (a
 * 64-channel V' = (W0 Wv) x and P.V; the PDSC_VFOLD=0 knob: never), else 0.  */
int32_t pdsc_encoder_plan_vfold(int32_t B, int32_t N, int32_t precision, int32_t *vfold);
/* Which pointwise-chain and tail kernels pdsc_forward_testing / _training
 * launch for B pairs of N correspondences under cfg (S = int(N * ratio) seeds,
 * cfg's precision) and this process's knobs; host-only, touches no device.
 * out[0 .. PDSC_LAUNCH_PLAN_FIELDS), capacity >= PDSC_LAUNCH_PLAN_FIELDS:
 *  [0] the pointwise chain: 1 register-chained (pw2_*), 0 LDS-tiled (pw_*);
 *      [1] .. [5] describe the LDS-tiled chain and are 0 under [0] = 1
 *  [1] its points per workgroup, 32 or 64
 *  [2] 1: pw_mid on 8 waves
 *  [3] 1: pw_first's Q / K / V in three workgroups per point tile
 *  [4] 1: the 8-wave pw_mid's likewise
 *  [5] 1: the 8-wave pw_mid's panel prefetch
 *  [6] rows per block of the NMS / seed-ranking compare kernels, 16 or 64
 *  [7] the NMS: compare with 1, 2 or 4 rows per thread; 0: the sorted form
 *  [8] the seed ranking: 0 compare, 1 sorted, 2 select, 3 select with the
 *      candidate ranking as a second launch (where the caller gives scratch,
 *      as the forwards do)
 *  [9] waves (seeds) per workgroup of the seed kNN select, the NSM and the
 *      hypotheses' sums: 1, 2 or 4
 * [10] the kNN select's ranking argument (0: readlane compare, else bitonic)
 * [11] 1: the Kabsch solve and inlier count inside the hypotheses' sums launch
 * [12] 1: the testing forward's fused tail launches                           */
#define PDSC_LAUNCH_PLAN_FIELDS 13
int32_t pdsc_launch_plan(const pdsc_config *cfg, int32_t B, int32_t N, int32_t *out, int32_t capacity);
/* Where one dense block of a layer sits in the packed blob (tests, tools):
 * block 0..7 = PointCN, fc_message 0 / 3 / 6, projection q / k / v, and the
 * folded W0 Wv block; offsets (in floats) of its weights, bias, BatchNorm
 * alpha and beta ([out] each) and scale {2^-s, 2^s}.                          */
int32_t pdsc_packed_block(const pdsc_config *cfg, int32_t layer, int32_t block, size_t offsets[5]);

/* Measurement hook (bench.py): while capacity > 0, every attention launch the
 * encoder issues from the calling thread records start_events[i] / stop_events[i]
 * (hipEvent_t) around itself on its stream, i = (*count)++ while < capacity.
 * Pass capacity 0 to disable.  The caller owns the events and the counter.   */
int32_t pdsc_attention_timing(void *const *start_events, void *const *stop_events, int32_t capacity,
                              int32_t *count);
/* Measurement hook (no reference counterpart): every pdsc_forward_testing
 * call from the calling thread records PDSC_FORWARD_STAGES + 1 events on its
 * stream -- events[c + 0] before a1, then one after each stage in the order
 * a1 compat, a2-a4 encoder, a5 seeds, a6 seed kNN, a7-a8 NSM, a9-a10
 * hypotheses+verification, a11 post-refinement -- with c = *count, then
 * *count += 8, while *count + 8 <= capacity.  Capacity 0 disables.           */
#define PDSC_FORWARD_STAGES 7
int32_t pdsc_forward_timing(void *const *events, int32_t capacity, int32_t *count);
/* Test hook (no reference counterpart): the small-batch pw_mid's K / V
 * workgroups of the Q / K / V split sleep `loops` x 127 x 64 cycles before
 * their first load (0: off, the default).  A per-thread setting like the
 * timing hooks; tests/test_gpu_parity.py uses it to pin that the split's
 * readers of the residual rows cannot see the Q workgroup's new rows.       */
int32_t pdsc_diag_qkv_delay(int32_t loops);

/* ------------------------------------------------------- a5 seeds ----------
 * pick_seeds: radius NMS on the confidences then the top-S of
 * conf * is_local_max in descending order (ties: ascending index).
 * Replaces models/PointDSC.py:199-217.  src [B,N,3]; conf [B,N];
 * seeds [B,S] int32; is_local_max [B,N] (0/1 fp32; required, it hosts the
 * flags between the two launches).                                          */
int32_t pdsc_pick_seeds(const float *src, const float *conf, int32_t B, int32_t N, float radius,
                        int32_t S, int32_t *seeds, float *is_local_max, pdsc_stream_t stream);

/* ------------------------------------------------------- a6 seed kNN -------
 * For each seed row: the k nearest correspondences in feature space,
 * d_j = 2 - 2 f_s.f_j, topk(k+1, smallest)[1:] -- the FIRST of the k+1
 * (ascending distance, ascending index) is dropped positionally.
 * Replaces models/common.py:48-69 + models/PointDSC.py:250-252 (only the
 * S seed rows are computed).  normed [B,N,C]; seeds [B,S]; knn [B,S,k];
 * 1 <= k <= 63, k + 1 <= N.  precision: enum pdsc_precision (distances).
 * The workspace holds the [B,S,N] distance rows.                            */
size_t pdsc_seed_knn_workspace_bytes(int32_t B, int32_t N, int32_t S);
int32_t pdsc_seed_knn(const float *normed, const int32_t *seeds, int32_t B, int32_t N, int32_t C,
                      int32_t S, int32_t k, int32_t precision, int32_t *knn, void *workspace,
                      size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------------ a7-a8 NSM weights --------
 * Local k x k feature x spatial consistency (diag 0), power iteration with
 * the batch-global allclose early exit (rtol 1e-5, atol 1e-8, evaluated over
 * all B*S seeds of the call, as torch.allclose does over the bs*S batch of one
 * cal_leading_eigenvector call), then w = v / (sum v + 1e-6); iters_used[b] is
 * the same for every b.  Replaces models/PointDSC.py:257-282, :338-358.
 * (pdsc_forward_testing exits per pair -- each pair is its own bs = 1 forward;
 * pdsc_forward_training over the whole batch -- one reference forward.)
 * sigma_dev / sigma_d_dev: device scalars (learned sigma, sigma_spat).
 * weights [B,S,k]; iters_used [B] int32 (may be NULL); 1 <= k <= min(63, N-1).
 * precision: enum pdsc_precision (the feature Gram).  The workspace holds the
 * fp16 hi/lo split of normed the H3 Gram MFMAs read.                         */
size_t pdsc_nsm_workspace_bytes(int32_t B, int32_t N, int32_t S, int32_t k, int32_t num_iterations);
int32_t pdsc_nsm_weights(const float *normed, const float *src, const float *tgt,
                         const int32_t *knn, int32_t B, int32_t N, int32_t C, int32_t S, int32_t k,
                         int32_t num_iterations, int32_t precision, const float *sigma_dev,
                         const float *sigma_d_dev, float *weights, int32_t *iters_used, void *workspace,
                         size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------------------- a9 Kabsch ---------
 * rigid_transform_3d: weighted centroids, H = Am^T diag(w) Bm, R from the SVD
 * of H (3x3, fp64 Jacobi on device) with the det(V U^T) reflection fix,
 * t = c_B - R c_A, packed as 4x4.  Replaces models/common.py:7-45 (whose SVD
 * runs on the host CPU).  A,Bp [nb,n,3]; w [nb,n] (NULL = ones); trans [nb,4,4]. */
int32_t pdsc_rigid_transform_3d(const float *A, const float *Bp, const float *w, int32_t nb,
                                int32_t n, float *trans, pdsc_stream_t stream);

/* --------------------------------------------- a10 verification ------------
 * Seed hypotheses: Kabsch on each seed's kNN set with `weights`, fitness =
 * mean(|R_s src + t_s - tgt| < tau), best = first argmax, final_labels from
 * the best hypothesis.  Replaces models/PointDSC.py:287-335.
 * seed_trans [B,S,4,4] and fitness [B,S] are required (they host the per-seed
 * scratch); best [B] int32 (may be NULL); trans [B,4,4]; labels [B,N].      */
size_t pdsc_seed_hypotheses_workspace_bytes(int32_t B, int32_t S);
int32_t pdsc_seed_hypotheses(const float *src, const float *tgt, const int32_t *knn,
                             const float *weights, int32_t B, int32_t N, int32_t S, int32_t k,
                             float tau, float *seed_trans, float *fitness, int32_t *best,
                             float *trans, float *labels, void *workspace, size_t workspace_bytes,
                             pdsc_stream_t stream);

/* ------------------------------------------------ a11 post-refinement ------
 * <= 20 IRLS re-fits on the inliers of |R src + t - tgt| < thr with weights
 * 1/(1 + (L2/thr)^2), stopping when the inlier count repeats.  Device-side
 * loop, one workgroup per pair.  Replaces models/PointDSC.py:403-438.
 * trans [B,4,4] in/out.                                                      */
int32_t pdsc_post_refine(float *trans, const float *src, const float *tgt, int32_t B, int32_t N,
                         float thr, pdsc_stream_t stream);

/* ------------------------------------- f3 spectral-matching baseline -----
 * SM of baseline_scripts/baseline_3DMatch.py:19-53 for one pair: dense
 * M_ij = max(0, 4.5 - (|c_j - c_i|_xyz - |c_j - c_i|_xyz')^2 / 2 / sigma^2),
 * sigma = inlier_threshold / 3, diag 0, over corr_pos [N,6]; num_iterations
 * power iterates v <- Mv / (|Mv| + 1e-6) from v = 1; labels [N] = the
 * int(N * top_ratio) largest entries of v (ties to the lower index); trans
 * [4,4] = rigid_transform_3d(src, tgt, v * labels).  leading_eig [N] may be
 * NULL.  Workspace: the dense M (4 N^2 B) + 3 vectors.                      */
size_t pdsc_spectral_matching_workspace_bytes(int32_t N);
int32_t pdsc_spectral_matching(const float *corr_pos, const float *src, const float *tgt, int32_t N,
                               double inlier_threshold, double top_ratio, int32_t num_iterations, float *trans,
                               float *labels, float *leading_eig, void *workspace, size_t workspace_bytes,
                               pdsc_stream_t stream);
/* The dense M [N,N] alone, by the launch pdsc_spectral_matching makes (exposed
 * so that tests can see M): same limits on N and inlier_threshold.           */
int32_t pdsc_sm_compat(const float *corr_pos, int32_t N, double inlier_threshold, float *M, pdsc_stream_t stream);
/* One M v product of the SM power iteration (the HBM-bound kernel, exposed for
 * measurement): y [N] = M [N,N] v [N].                                       */
int32_t pdsc_sm_matvec(const float *M, const float *v, int32_t N, float *y, pdsc_stream_t stream);

/* ------------------------------ f3 training-mode forward and loss ---------
 * PointDSC.forward(data) WITHOUT the 'testing' key (models/PointDSC.py:158-163,
 * 176, 182, 189-191) for B pairs (the training batch; forward only -- no
 * gradients): M = clamp(1 - (1 - F^ F^T) / sigma^2, 0, 1) with a zero diagonal
 * into M_out [B,N,N] (may be NULL), seeds = the int(N * ratio) largest logits
 * (argsort, no NMS; ties by ascending index), seed hypotheses and verification
 * as in testing, no post-refinement.  Outputs final_trans [B,4,4] and
 * confidence [B,N] (the logits the reference returns as 'final_labels');
 * seeds_out [B,int(N*ratio)] (may be NULL) receives the seed indices.       */
size_t pdsc_forward_training_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N);
int32_t pdsc_forward_training(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                              const float *src, const float *tgt, int32_t B, int32_t N, float *final_trans,
                              float *confidence, float *M_out, int32_t *seeds_out, void *workspace,
                              size_t workspace_bytes, pdsc_stream_t stream);
/* SpectralMatchingLoss (libs/loss.py:115-139) of M [B,N,N] against gt_labels
 * [B,N] (0/1): balanced != 0 -> mean over pairs of 0.5 sum gt (M-1)^2 /
 * (relu(sum gt - 1) + 1) + 0.5 sum (1-gt) M^2 / (relu(sum (1-gt) - 1) + 1), else
 * mean((M - gt)^2); gt_ij = (l_i + l_j == 2), gt_ii = 0.  Sums in fp64;
 * loss: one device float.                                                   */
size_t pdsc_spectral_matching_loss_workspace_bytes(int32_t B, int32_t N);
int32_t pdsc_spectral_matching_loss(const float *M, const float *gt_labels, int32_t B, int32_t N, int32_t balanced,
                                    float *loss, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ---------------------------------- f1 correspondence construction --------
 * Mutual nearest neighbours in descriptor space and the network inputs built
 * from them: replaces datasets/ThreeDMatch.py:277-308 (3DMatch / 3DLoMatch
 * test sets), datasets/KITTI.py:85-99 and demo_registration.py:101-108.
 *   distance = sqrt(2 - 2 src_desc tgt_desc^T + 1e-6) in fp32, never stored;
 *   nn_src[i] = argmin_j, nn_tgt[j] = argmin_i (first index on ties, like
 *   numpy.argmin).  src_desc [Ns,D], tgt_desc [Nt,D], 1 <= D <= 64.
 * Workspace: 8 (Ns + Nt) bytes (64-bit key/index words).                    */
size_t pdsc_mutual_nn_workspace_bytes(int32_t Ns, int32_t Nt);
int32_t pdsc_mutual_nn(const float *src_desc, const float *tgt_desc, int32_t Ns, int32_t Nt, int32_t D,
                       int32_t *nn_src, int32_t *nn_tgt, void *workspace, size_t workspace_bytes,
                       pdsc_stream_t stream);
/* The correspondence set (mutual != 0: i with nn_tgt[nn_src[i]] == i, in
 * ascending i; else every i) and the forward's inputs: corr [Ns,2] int32
 * (first *count rows valid), src_keypts / tgt_keypts [Ns,3], corr_pos [Ns,6]
 * = [src, tgt] - their mean (numpy's sequential fp32 column mean), and, when
 * gt_trans (a device double[16], row-major 4x4) is non-NULL, labels [Ns] =
 * |R src + t - tgt| < inlier_threshold in fp64.  count: a device int32.     */
int32_t pdsc_build_correspondences(const float *src_desc, const float *tgt_desc, const float *src_xyz,
                                   const float *tgt_xyz, int32_t Ns, int32_t Nt, int32_t D, int32_t mutual,
                                   const double *gt_trans, double inlier_threshold, int32_t *corr,
                                   int32_t *count, float *corr_pos, float *src_keypts, float *tgt_keypts,
                                   float *labels, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------- f4 descriptor stage ----------
 * The open3d calls of demo_registration.py:37-44 / misc/cal_fpfh.py:7-36 on the
 * GPU (open3d's published algorithms restated; parity with open3d itself is
 * unpinned).  Points are fp32 [n,3] device arrays; 1 <= n <= 2^31-1.  These
 * entry points synchronise `stream` before returning (they report grid-range
 * and capacity errors found on the device).
 *
 * pdsc_ply_read_xyz (HOST memory, o3d.io.read_point_cloud): the vertex x, y, z
 * of a binary_little_endian or ascii PLY.  xyz == NULL: only *n_points.  An
 * element count the file cannot back (negative, or more rows than the bytes
 * after the header hold) is PDSC_ERR_ARG, from the size query already; a zero
 * vertex count is an empty cloud (*n_points = 0).                            */
int32_t pdsc_ply_read_xyz(const char *path, float *xyz, int64_t capacity, int64_t *n_points);
/* KDTreeSearchParamHybrid(radius, max_nn) for every point of the cloud: nbr
 * [n,max_nn] (ascending (d^2, index), the point itself first, -1 padded),
 * dist2 [n,max_nn] fp64 (may be NULL), count [n].  1 <= max_nn <= 128.      */
size_t pdsc_radius_knn_workspace_bytes(int32_t n);
int32_t pdsc_radius_knn(const float *pts, int32_t n, float radius, int32_t max_nn, int32_t *nbr, double *dist2,
                        int32_t *count, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
/* EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn)) (utils/pointcloud.py:
 * 20-21) as open3d 0.9.0 (environment.yml:76) computes it with its default
 * fast_normal_computation: the fp64 cumulant covariance of the neighbourhood,
 * FastEigen3x3's smallest-eigenvalue eigenvector (A - l0 I)(A - l1 I) e0,
 * normalised -- so its sign gives n_x >= 0 --, (0,0,1) when that vector is 0
 * or under 3 neighbours.  orient (enum pdsc_normal_orientation):
 *   PDSC_NORMALS_OPEN3D    that sign, as open3d leaves it on a cloud without
 *                          normals (the demo's case; viewpoint unused, may be NULL)
 *   PDSC_NORMALS_VIEWPOINT flipped towards viewpoint (device float[3])
 *   PDSC_NORMALS_CENTROID  flipped towards the cloud's centroid (makes FPFH
 *                          invariant to rigid motions; not open3d's result)   */
enum pdsc_normal_orientation {
    PDSC_NORMALS_OPEN3D = 0,
    PDSC_NORMALS_VIEWPOINT = 1,
    PDSC_NORMALS_CENTROID = 2,
};
size_t pdsc_estimate_normals_workspace_bytes(int32_t n, int32_t max_nn);
int32_t pdsc_estimate_normals(const float *pts, int32_t n, float radius, int32_t max_nn, int32_t orient,
                              const float *viewpoint, float *normals, void *workspace, size_t workspace_bytes,
                              pdsc_stream_t stream);
/* VoxelDownSample(voxel_size): per-voxel means; normals summed and normalised
 * (open3d's AccumulatedPoint::GetAverageNormal: a zero sum stays 0);
 * normals / out_normals may be NULL; voxels in ascending key order; out_pts
 * [n,3] capacity; *out_count (device int32) = voxels.                        */
size_t pdsc_voxel_down_sample_workspace_bytes(int32_t n);
int32_t pdsc_voxel_down_sample(const float *pts, const float *normals, int32_t n, float voxel_size, float *out_pts,
                               float *out_normals, int32_t *out_count, void *workspace, size_t workspace_bytes,
                               pdsc_stream_t stream);
/* compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)): fpfh [n,33]
 * fp64 (open3d's feature.data.T); fpfh_normalized [n,33] fp32 = f / (||f|| +
 * 1e-6) (demo_registration.py:42, may be NULL).  normals must be unit.      */
size_t pdsc_compute_fpfh_workspace_bytes(int32_t n, int32_t max_nn);
int32_t pdsc_compute_fpfh(const float *pts, const float *normals, int32_t n, float radius, int32_t max_nn,
                          double *fpfh, float *fpfh_normalized, void *workspace, size_t workspace_bytes,
                          pdsc_stream_t stream);

/* ------------------------------------------- f5 ICP refinement -------------
 * The "+ICP" stage of the reference's drivers: o3d registration_icp(src, tgt,
 * max_distance, init, TransformationEstimationPointToPoint()) seeded with the
 * forward's final_trans (test.py:183-189, distance 0.6; evaluation/
 * benchmark_utils.py:40-56 icp_refine, distance 0.1, used by test.py,
 * multiway/test_multi.py:53-54 and multiway/test_multi_ate.py).  open3d's
 * RegistrationICP with its default criteria restated (parity with open3d
 * itself is unpinned): T maps source to target (T [x;1]); evaluate(T) pairs
 * every source point q = R p + t (fp64) with its nearest target point within
 * d^2 <= max_distance^2 (fp64 d^2, pdsc_radius_knn's inclusion, ties to the
 * lower target index), fitness = n_corr / Ns, inlier_rmse = sqrt(sum d^2 /
 * n_corr) (0 without correspondences).  Starting from evaluate(init), at most
 * max_iteration times: T <- Kabsch(correspondences) T (unit weights, fp64,
 * identity without correspondences), evaluate(T), and stop once |fitness
 * change| < relative_fitness and |rmse change| < relative_rmse (open3d's
 * defaults: 30, 1e-6, 1e-6).  max_iteration = 0 only evaluates init.  T and
 * every sum stay fp64 on the device, summed in a fixed order (two calls are
 * bitwise equal); nothing synchronises inside the loop.  Ns <= 512 runs the
 * loop in one launch of one workgroup (environment PDSC_ICP_ONE_WG=0, read at
 * every call, keeps the launch-per-step path; the results are bitwise the
 * same).  Like the f4 entry points it synchronises `stream` once at the end to
 * report the grid error (target extent / max_distance >= 2^21 cells:
 * PDSC_ERR_ARG, outputs unspecified).  source [Ns,3], target [Nt,3] fp32.   */
typedef struct pdsc_icp_result { /* device memory, written by the call */
    double trans[16];            /* final T, fp64 row-major */
    double fitness, inlier_rmse;
    int32_t iterations;          /* updates applied, 0 .. max_iteration */
    int32_t n_corr;
} pdsc_icp_result;
size_t pdsc_icp_workspace_bytes(int32_t Ns, int32_t Nt);
int32_t pdsc_icp_point_to_point(const float *source, int32_t Ns, const float *target, int32_t Nt,
                                const double *init_trans /* device double[16], NULL = identity */,
                                double max_distance, int32_t max_iteration, double relative_fitness,
                                double relative_rmse, float *trans_f32 /* [4,4] = (float)result.trans, may be NULL */,
                                pdsc_icp_result *result /* may be NULL */,
                                int32_t *corr /* [Ns] of the final evaluate: target index or -1, may be NULL */,
                                void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------ f6 RANSAC on correspondences ---
 * open3d's registration_ransac_based_on_correspondence with
 * TransformationEstimationPointToPoint(False), as the reference's drivers call
 * it (baseline_scripts/baseline_3DMatch.py:80-98: ransac_n 4, 1000 iterations;
 * evaluation/test_3DMatch.py:59-77, test.py:137-155: ransac_n 3, 5000;
 * algorithms/FR.py:122-150: ransac_n 4, up to 500000, edge-length checker and /
 * or confidence).  open3d's algorithm is restated (open3d is not a dependency,
 * its sampler is not reproducible: parity with open3d itself is unpinned) and
 * the choices it leaves open are fixed, so that two calls are bitwise equal and
 * a CPU restatement can follow the draws one by one.  Row i of src [N,3]
 * corresponds to row i of tgt [N,3] (fp32); H = max_iteration hypotheses h = 0
 * .. H - 1.
 *   Sampling    draw j (0 .. ransac_n - 1) of hypothesis h is u = mix64(seed +
 *               (8 h + j) * 0x9E3779B97F4A7C15) in wrapping 64-bit arithmetic,
 *               mix64 the splitmix64 finaliser (z += 0x9E3779B97F4A7C15; z = (z ^
 *               (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *               0x94D049BB133111EB; z ^ (z >> 31)); the sample index is ((u >>
 *               32) * N) >> 32.  Integer arithmetic only.  A hypothesis with a
 *               repeated index is invalid (count -1).
 *   Checker     with edge_similarity = sim > 0 (open3d's
 *               CorrespondenceCheckerBasedOnEdgeLength; its default is 0.9): for
 *               every pair a < b of the sample, |s_a - s_b| >= sim |t_a - t_b|
 *               and |t_a - t_b| >= sim |s_a - s_b| in fp64; a hypothesis that
 *               fails has count -2 and nothing else is computed for it.
 *   Estimate    unit-weight Kabsch of the ransac_n pairs in fp64: centroids c_A,
 *               c_B, H = sum (a - c_A)(b - c_B)^T, R = V diag(1, 1, det(V U^T))
 *               U^T, t = c_B - R c_A.  H is accumulated with compensated sums
 *               and R refined by one Newton step, so the pose is good to fp64
 *               rounding for nearly collinear samples too (an fp64 SVD alone
 *               is off by eps sigma_1 / sigma_2).
 *   Score       over all N correspondences d^2 = |R s + t - tgt|^2 in fp64; an
 *               inlier has d^2 < max_distance^2; count = the inliers, sumsq =
 *               sum of d^2 over them in a fixed order.
 *   Best        the highest count; among equal counts the lower sumsq; among
 *               equal sumsq the lower h (open3d's "fitness greater, or equal and
 *               rmse lower" scan in hypothesis order).
 *   Rounds      hypotheses are processed in rounds of pdsc_ransac_round().
 *               After round r = 0, 1, .., with f = best count / N: when
 *               confidence < 1 and f > 0, stop if (r + 1) round >= log(1 -
 *               confidence) / log(1 - f^ransac_n), or if f = 1 (the
 *               criterion's log(0)): open3d's confidence criterion evaluated at
 *               round granularity.  confidence = 1 never stops early.  The
 *               round size is therefore part of the result's definition.
 *               Nothing synchronises inside the loop: every round is enqueued up
 *               front and the rounds after the stop return at entry.
 *   Result      labels [N] = 1 for the inliers of the winning hypothesis, else
 *               0; fitness = n_inliers / N and inlier_rmse = sqrt(sumsq /
 *               n_inliers) (0 without inliers) refer to it.  With refit != 0
 *               trans is one fp64 Kabsch over all those inliers
 *               (algorithms/FR.py:101-114); labels, fitness and inlier_rmse stay
 *               the winner's.  Without a valid hypothesis trans is the
 *               identity, fitness 0, labels 0, best -1.  trans_f32 [4,4] =
 *               (float)trans.
 *   Errors      PDSC_ERR_UNSUPPORTED for ransac_n other than 3 or 4;
 *               PDSC_ERR_ARG for N < ransac_n, max_iteration < 1, max_distance
 *               <= 0 or not finite, confidence outside (0, 1], edge_similarity
 *               outside [0, 1], null src / tgt / workspace, a workspace that is
 *               too small: all checked on the host before any device work.
 *   Left out    open3d 0.9's max_validation: every driver sets it equal to
 *               max_iteration.  open3d's distance and normal checkers.
 * Debug rows of hypotheses never drawn (after an early stop) have count -3;
 * samples are written for every drawn hypothesis, trans / sumsq only for valid
 * ones (the other rows are left as the caller filled them).                 */
typedef struct pdsc_ransac_result {   /* device memory */
    double trans[16];                 /* fp64 row-major, source -> target */
    double fitness, inlier_rmse;      /* n_inliers / N, sqrt(sum d^2 / n_inliers) (0 if none) */
    int32_t n_inliers;
    int32_t iterations;               /* hypotheses drawn: a multiple of the round, or max_iteration */
    int32_t best;                     /* index of the winning hypothesis, -1: none valid */
    int32_t n_validated;              /* hypotheses that passed sampling + checker */
} pdsc_ransac_result;
typedef struct pdsc_ransac_debug {    /* any member may be NULL; H = max_iteration */
    int32_t *samples;                 /* [H, ransac_n] */
    int32_t *count;                   /* [H]: inliers, -1 repeated index, -2 checker, -3 not drawn (early stop) */
    double  *sumsq;                   /* [H]: sum of d^2 over the inliers */
    double  *trans;                   /* [H,16] */
} pdsc_ransac_debug;
int32_t pdsc_ransac_round(void);      /* hypotheses per round */
size_t  pdsc_ransac_workspace_bytes(int32_t N);      /* independent of max_iteration */
int32_t pdsc_ransac_correspondence(const float *src, const float *tgt, int32_t N,
                                   double max_distance, int32_t ransac_n /* 3 or 4 */,
                                   double edge_similarity /* 0: no checker */,
                                   int32_t max_iteration, double confidence /* 1.0: never stop early */,
                                   uint64_t seed, int32_t refit, float *trans_f32 /* may be NULL */,
                                   float *labels /* [N] 0/1, may be NULL */,
                                   pdsc_ransac_result *result /* may be NULL */,
                                   const pdsc_ransac_debug *debug /* HOST struct of device pointers, may be NULL */,
                                   void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------ f7 filtered RANSAC front end ---
 * The filter stage of the fork's "fast RANSAC" pipeline (algorithms/FR.py:36-58
 * and :101-114 on algorithms/matching.py; test.py:163-170, --algo RANSAC --mode
 * no_filter | MFR | GPF) between descriptor matching and f6.  Nothing here
 * synchronises the stream, counts stay in device memory, every argument is
 * checked on the host before any device work (PDSC_ERR_ARG: sizes below their
 * minimum, null pointers, a workspace that is too small, a factor or radius
 * that is negative or not finite; PDSC_ERR_UNSUPPORTED: D > 64, grid_wid >
 * 64, more than 262144 rows in pdsc_gpf_select).  Two calls are bitwise equal (integer atomics only).
 *
 * pdsc_nn2 (matching.py:22-65 find_nn(return_2nd=True), and the reverse
 * find_nn inside nn_to_mutual :225-229).  f0 [N0,D], f1 [N1,D] fp32, 1 <= D <=
 * 64, N0 >= 1, N1 >= 2.  All in fp32, no contraction except the fmaf named:
 *   dot(a, b) = fmaf(a_k, b_k, acc) for k = 0 .. D-1 ascending, acc = 0 first;
 *   dist2(i, j) = (dot(f0_i, f0_i) + dot(f1_j, f1_j)) - 2 * dot(f0_i, f1_j);
 *   dist(i, j)  = sqrt(dist2 < 1e-30 ? 1e-30 : dist2)    (clamp_min: NaN stays);
 *   nn1[i] = argmin_j, nn2[i] = argmin_{j != nn1[i]}, rev[j] = argmin_i of the
 *   same values (each is computed once, both directions see the same bits), all
 *   under the order (dist, index): ties go to the lower index in both
 *   directions (torch.min leaves that open); a NaN distance orders before
 *   every number (numpy.argmin's rule, as pdsc_mutual_nn).
 * The N0 x N1 matrix is never stored.  The column tiles of a row stripe may be
 * split over several workgroups whose (dist, index) pairs are merged exactly;
 * the result does not depend on the split.  pdsc_nn2_split is pdsc_nn2 with
 * the split given (>= 1, clamped to the column tiles and to 16): a debug entry
 * point for tests, same workspace.
 *
 * pdsc_match_ratio (matching.py:89-98 calc_distance_ratio_in_feature_space,
 * :210-223 mark_best_buddies, :122-137 normalize and the best-buddy offset):
 *   norm2(a, b) = fmaf(d_k, d_k, acc), d_k = a_k - b_k, k ascending;
 *   feat_dist[i] = sqrt(norm2(f0_i, f1_nn1[i])) / (sqrt(norm2(f0_i, f1_nn2[i])) + 1e-6)
 *   (computed directly as the reference does, not from dist above);
 *   is_bb[i] = (rev[nn1[i]] == i); the rows with is_bb in ascending i are the
 *   MFR output (nn_to_mutual); num_bb = their number (device int32);
 *   norm[i] = (feat_dist[i] - min) / (max - min) over all rows, minus 1 where
 *   is_bb.  Deviation: with max == min the reference divides by zero; here the
 *   quotient is defined as 0 (so norm is -1 on best buddies, 0 elsewhere).
 *   An index outside [0, N1) gives feat_dist NaN and is_bb 0 (nothing is read).
 * rev == NULL: only feat_dist is written (is_bb, norm, num_bb may be NULL).
 *
 * pdsc_gpf_select (matching.py:100-208 Grid_Prioritized_Filter, BB_first=False;
 * BB_first=True, which algorithms/TEASER_plus_plus.py:110 calls, is composed from it in f9).  xyz0 [N0,3]
 * are the source points of rows 0 .. N0-1, norm [N0] and num_bb as above.
 *   Cells     to_quads (:139-145) bit-exactly in fp32, in its operation order:
 *             q(X) = floor(G * ((X - m) / ((M - m) + 1e-3f))) with m, M the
 *             minimum and maximum of the column, for x and for y; cell = q(x) G
 *             + q(y).  A row with q outside [0, G) (M - m so large that the
 *             1e-3 is lost) is in no cell, as in the reference's loops, and is
 *             never kept; its debug cell is -1.  1 <= G = grid_wid <= 64.
 *   Heights   max_per_quad = integer rows per cell; TOTAL = gpf_factor * num_bb
 *             in fp64; the bisection of :163-180 as written (|max - min| > 2,
 *             the three-way compare) in fp64; per_quad = min(max_per_quad,
 *             rint(height)): np.round is round half to even.  Deviation: each
 *             step's sum over the cells is taken sequentially in cell order,
 *             where the reference's per_quad.sum() is numpy's blocked pairwise
 *             summation.  Counts and heights that are dyadic (TOTAL an integer
 *             or a half) sum exactly either way; for another gpf_factor *
 *             num_bb the two sums can differ in the last place and a step's
 *             == / < / > can then fall the other way.
 *   Selection a cell with per_quad == max_per_quad keeps every row; another
 *             keeps the int(per_quad) rows that are lowest under (norm, row):
 *             ties to the lower row (the reference's argsort is unstable).
 *   Cost      the rows of a truncated cell are ranked by counting inside the
 *             cell: n^2 word compares for a cell of n rows, N0^2 when one cell
 *             holds every row (G = 1, or one far outlier stretching the
 *             extent).  N0 is therefore limited to 262144 (PDSC_ERR_UNSUPPORTED
 *             above; the reference's clouds are a few ten thousand keypoints).
 *   Output    kept [N0 capacity]: the kept rows ascending; *count (device
 *             int32); kept_norm [N0 capacity] = norm of those rows (may be NULL).
 * pdsc_gpf_debug: any member may be NULL.
 *
 * pdsc_refit_inliers (FR.py:101-114): the inliers of pose (device double[16],
 * row-major 4x4) among the N pairs src[i], tgt[i] are the rows with |R s + t -
 * tgt|^2 < radius^2 in fp64 (f6's Score); trans = one unit-weight fp64 Kabsch
 * over them -- the same code as f6's refit, so on f6's own point set and pose
 * the two are bitwise equal.  FR calls it on the unfiltered pairs.  With fewer
 * than 3 inliers the reference's estimate is undefined: trans is then the
 * input pose, bit for bit.  *count (device int32, may be NULL) = the inliers
 * of the INPUT pose, labels [N] (may be NULL) mark them; trans_f32 = (float)
 * trans (may be NULL).  trans may alias pose.                                 */
typedef struct pdsc_gpf_debug {       /* HOST struct of device pointers */
    int32_t *cell;                    /* [N0] */
    int32_t *max_per_quad;            /* [G*G] */
    double  *per_quad;                /* [G*G] */
    double  *height;                  /* [1] the bisection's final height, before rint */
} pdsc_gpf_debug;
size_t  pdsc_nn2_workspace_bytes(int32_t N0, int32_t N1);
int32_t pdsc_nn2(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, int32_t *nn1, int32_t *nn2,
                 int32_t *rev /* [N1] */, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_nn2_split(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, int32_t split,
                       int32_t *nn1, int32_t *nn2, int32_t *rev, void *workspace, size_t workspace_bytes,
                       pdsc_stream_t stream);
int32_t pdsc_match_ratio(const float *f0, const float *f1, int32_t N0, int32_t N1, int32_t D, const int32_t *nn1,
                         const int32_t *nn2, const int32_t *rev, int32_t *is_bb, float *feat_dist, float *norm,
                         int32_t *num_bb, pdsc_stream_t stream);
size_t  pdsc_gpf_select_workspace_bytes(int32_t N0, int32_t grid_wid);
int32_t pdsc_gpf_select(const float *xyz0, const float *norm, const int32_t *num_bb, int32_t N0, int32_t grid_wid,
                        double gpf_factor, int32_t *kept, int32_t *count, float *kept_norm,
                        const pdsc_gpf_debug *debug, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_refit_inliers(const double *pose, const float *src, const float *tgt, int32_t N, double radius,
                           double *trans, float *trans_f32, int32_t *count, float *labels, pdsc_stream_t stream);

/* ------------------------------------------------- f8 PMC baseline ---------
 * PMC of baseline_scripts/baseline_3DMatch.py:56-77: a graph over the N
 * correspondences with an edge where two of them are length-consistent, its
 * maximum clique as the inlier set, one Kabsch (a9) over it.  The reference
 * builds the edge list in a Python double loop and hands it to a prebuilt x86
 * libpmc.so (utils/max_clique.py:14-40); here both halves run on the device.
 * The same two pieces are the core of TEASER++'s inlier selection
 * (algorithms/TEASER_plus_plus.py:78-93, PMC_EXACT): f9 below builds on them.
 * Nothing here synchronises the stream or allocates, every argument is checked
 * on the host before any device work, and two calls are bitwise equal (integer
 * work only; every output word has one writer).
 *
 * A graph `adj` is N rows of W = ceil(N / 64) uint64 words: bit j % 64 of word
 * j / 64 of row i is set iff i != j and (i, j) is an edge; bits past N and the
 * diagonal are 0; the matrix is symmetric.  1 <= N <= 8192
 * (PDSC_ERR_UNSUPPORTED above: one wavefront holds a row).
 *
 * pdsc_consistency_graph: corr_pos [N,6] fp32, the loader's centred [src, tgt]
 * rows.  With d = c_i[0:3] - c_j[0:3] and e = c_i[3:6] - c_j[3:6], all in fp32
 * with every product and sum rounded (no contraction):
 *   a = (dx*dx + dy*dy) + dz*dz,  b likewise of e   (np.sum of three squares);
 *   PDSC_EDGE_SQUARED  diff = a - b: the reference as written (:66-67), which
 *                      holds SQUARED lengths against inlier_threshold;
 *   PDSC_EDGE_LENGTH   diff = sqrtf(a) - sqrtf(b) (correctly rounded), the
 *                      | |s_i - s_j| - |t_i - t_j| | form of TEASER-style graphs;
 *   edge iff (double)|diff| < threshold (numpy 1.x compares the fp32 scalar in
 *   fp64).  The predicate is bit-symmetric in (i, j); the N x N values are
 *   never stored.  degree [N] int32 (may be NULL) = the row's edges.
 *   PDSC_ERR_ARG: N < 1, threshold <= 0 or not finite, an unknown mode, null
 *   corr_pos / adj.
 *
 * pdsc_max_clique: a maximum clique of adj.  members [N capacity] = its
 * vertices ascending, -1 past the size; labels [N] fp32 0/1 (may be NULL);
 * *result (device memory, required).  The clique returned is a pure function
 * of (adj, N, node_budget) -- which of several maximum cliques is this
 * implementation's choice -- and never depends on timing.  A graph without
 * edges gives {0}, size 1.
 *   Lower bound  a greedy clique from every vertex (candidates = its
 *                neighbours; take the candidate of the highest degree, ties to
 *                the lower index; intersect; repeat); the best by (size, lower
 *                start) is the first incumbent, heuristic_size its size.
 *   Reduction    16 rounds of dropping every vertex with fewer neighbours left
 *                than the incumbent's size; the survivors in ascending
 *                (remaining degree, index) order are the roots.
 *   Search       root r searches the cliques whose first member in that order
 *                is r, by branch and bound on bitsets with a greedy-colouring
 *                bound, from the incumbent of its launch; the roots run in
 *                four launches, each from the previous one's winner by (size,
 *                lower root).
 *   Budget       every colouring is one expanded node.  A root stops after
 *                node_budget nodes (0: pdsc_max_clique_default_budget()), or
 *                where its stack would pass pdsc_max_clique_depth() levels
 *                (a clique more than that many vertices beyond its root);
 *                either way it counts in roots_incomplete, exact becomes 0, and
 *                the best clique found so far is still returned.  exact == 1:
 *                size is the clique number.  nodes = the sum over the roots.
 *   PDSC_ERR_ARG: N < 1, node_budget < 0, null adj / members / result /
 *   workspace, a workspace that is too small.
 * pdsc_greedy_clique: the lower bound alone (same outputs and workspace;
 * exact = 0, roots_incomplete = 0, nodes = 0).                                */
enum pdsc_edge_mode {
    PDSC_EDGE_SQUARED = 0,
    PDSC_EDGE_LENGTH = 1,
};
typedef struct pdsc_clique_result { /* device memory, written by the call */
    int32_t size;                   /* members of the clique returned */
    int32_t exact;                  /* 1: every root was searched to the end, size is the clique number */
    int32_t heuristic_size;         /* the greedy lower bound */
    int32_t roots_incomplete;       /* roots stopped by the budget or the stack depth */
    int64_t nodes;                  /* expanded search nodes over all roots */
} pdsc_clique_result;
int32_t pdsc_consistency_graph(const float *corr_pos, int32_t N, double threshold, int32_t mode, uint64_t *adj,
                               int32_t *degree /* may be NULL */, pdsc_stream_t stream);
int32_t pdsc_max_clique_depth(void);          /* stack levels per root */
int64_t pdsc_max_clique_default_budget(void); /* nodes per root */
size_t  pdsc_max_clique_workspace_bytes(int32_t N);
int32_t pdsc_max_clique(const uint64_t *adj, int32_t N, int64_t node_budget, int32_t *members,
                        pdsc_clique_result *result, float *labels /* may be NULL */, void *workspace,
                        size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_greedy_clique(const uint64_t *adj, int32_t N, int32_t *members, pdsc_clique_result *result,
                           float *labels /* may be NULL */, void *workspace, size_t workspace_bytes,
                           pdsc_stream_t stream);

/* ------------------------------------------------------ f9 TEASER++ --------
 * The fork's --algo TEASER (algorithms/TEASER_plus_plus.py:78-93: cbar2 = 1,
 * noise_bound = 0.3, no scale estimation, PMC_EXACT, CHAIN, GNC_TLS with
 * gnc_factor 1.4, max_iterations 10000, cost_threshold 1e-16) after f8's graph
 * and clique: the GNC-TLS rotation over the clique's TIM chain and the
 * component-wise TLS translation by adaptive voting.  The reference calls the
 * x86 library teaserpp_python, which is neither installed nor in the reference
 * tree: the definitions below are written from the published algorithm and ARE
 * the contract; parity with the TEASER++ library itself is unpinned.
 * Nothing here synchronises the stream or allocates; every argument is checked
 * on the host before any device work (PDSC_ERR_ARG: K or N < 1, null pointers,
 * noise_bound not finite or <= 0, gnc_factor <= 1 or not finite, max_iterations
 * < 1, a cost_threshold that is NaN, node_budget < 0, a workspace that is too
 * small; PDSC_ERR_UNSUPPORTED: K or N > 8192).  All arithmetic is fp64 with no
 * contraction, every sum runs through one fixed tree and there are no
 * floating-point atomics: two calls are bitwise equal.
 *
 * pdsc_gnc_tls_rotation: src_tims, dst_tims [K,3] fp64 (a_j, b_j), 1 <= K <=
 * 8192.  nb2 = noise_bound^2, w = 1, prev = +inf; for i = 0 .. max_iterations-1:
 *   1. H = sum_j w_j a_j b_j^T (no centring: TIMs are differences), H = U S V^T,
 *      R = V diag(1, 1, det(V U^T)) U^T by a9's fp64 Jacobi solve.  Where H has
 *      rank < 2 the rotation is not determined by the data (K = 1; two opposite
 *      TIMs): R is then that solve's deterministic completion.
 *   2. r_j = |b_j - R a_j|^2.
 *   3. at i == 0: d = 2 max_j r_j / nb2 - 1; d <= 0 stops here with every weight
 *      1 (stop_reason 1, iterations 1); else mu = 1 / d.  Deviation: the library
 *      tests mu <= 0 after the division, which differs only at d == 0, where it
 *      goes on with mu = inf and NaN thresholds.
 *   4. th1 = (mu + 1) / mu * nb2, th2 = mu / (mu + 1) * nb2; cost = sum_j w_j r_j
 *      with the OLD weights; then w_j = 0 where r_j >= th1, 1 where r_j <= th2,
 *      else sqrt(nb2 mu (mu + 1) / r_j) - mu.
 *   5. diff = |cost - prev|, mu *= gnc_factor, prev = cost; diff < cost_threshold
 *      stops (stop_reason 2).
 * R [9] row-major; weights [K] (may be NULL); inliers [K] int32 = (w_j >= 0.5)
 * (may be NULL); info (device, may be NULL): iterations = passes of step 1,
 * cost = the last step 4 sum (step 3's stop: sum r_j), mu after the last step 5
 * (0 after step 3's stop), stop_reason 0 = max_iterations reached.  One launch
 * of one workgroup; no host read between iterations.
 *
 * pdsc_tls_translation: src [K,3] fp64 (already rotated), dst [K,3] fp64.  Per
 * axis c: x_j = dst_jc - src_jc, beta = noise_bound for every j (cbar2 = 1).
 * The 2K events (x_j - beta, tag +(j+1)) "enter" and (x_j + beta, tag -(j+1))
 * "leave", ascending by value, ties by tag; after each event C = the entered-
 * and-not-left indices; an event that leaves C empty is skipped; else xhat =
 * mean(x_C), cost = sum_{j in C} (x_j - xhat)^2 + beta (K - |C|) (the library's
 * mixed-unit cost, kept as is); t_c = xhat of the first event of minimal cost.
 * With one beta, C is a window of the sorted x: the kernel sorts x, derives
 * every event's window and place in the sequence, and takes window sums from
 * prefix sums of (x - x_median) and its square.  Deviation: two events of
 * DIFFERENT x whose x -/+ beta round to the same fp64 value are ordered by x,
 * then leave before enter, where the tag order could interleave them (events of
 * equal x give the same sets of values either way).  inliers [K] int32 (may be
 * NULL) = |x_jc - t_c| <= beta on all three axes.  Workspace:
 * pdsc_tls_translation_workspace_bytes(K) (the prefix sums).
 *
 * pdsc_teaser_solve: src, tgt [N,3] fp32, row i <-> row i, 1 <= N <= 8192; all
 * enqueued in one go, no host read in between:
 *   1. pdsc_consistency_graph on the rows [src_i, tgt_i], PDSC_EDGE_LENGTH,
 *      threshold 2 noise_bound.  Deviation: TEASER++ tests <= on fp64 lengths;
 *      this is f8's strict < on correctly rounded fp32 lengths.
 *   2. pdsc_max_clique with node_budget (0: the default).  The reference's
 *      FAIL_TOLERANT watchdog kills a stuck search after 10 s; here the budget
 *      is that bound: an incomplete search still gives a pose, clique_exact = 0.
 *   3. Kc = the clique's size, read on the device.  Kc <= 1 is the library's
 *      "clique too small": valid = 0, trans = I, labels 0, and the solver
 *      kernels return at entry.  Else the CHAIN TIMs over the members c_0 < ...
 *      < c_{Kc-1}: a_i = src[c_{(i+1) mod Kc}] - src[c_i], b_i likewise from tgt
 *      (Kc TIMs; Kc = 2 gives two opposite ones, as in the library).
 *   4. the rotation above on them;  5. s_i = R src[c_i];  6. the translation
 *      above on (s_i, tgt[c_i]).
 * result (device memory, required); trans_f32 [4,4] (may be NULL) = (float)
 * trans; labels [N] fp32 (may be NULL) = 1 for clique members that are
 * translation inliers.  Out of scope: scale estimation, the FGR rotation solver,
 * the COMPLETE and STAR TIM graphs, the heuristic / KCORE clique modes,
 * certification.                                                             */
typedef struct pdsc_gnc_info { /* device memory, written by the call */
    int32_t iterations;        /* passes of step 1 */
    int32_t stop_reason;       /* 0 max_iterations, 1 no residual above the bound at pass 0, 2 cost converged */
    double  cost;
    double  mu;
} pdsc_gnc_info;
typedef struct pdsc_teaser_result { /* device memory, written by the call */
    double  trans[16];              /* row-major 4x4 */
    int32_t valid;                  /* 0: clique of fewer than 2 members, trans = I */
    int32_t clique_size;
    int32_t clique_exact;
    int32_t roots_incomplete;
    int32_t gnc_iterations;
    int32_t n_rotation_inliers;     /* TIMs of the chain with final weight >= 0.5 */
    int32_t n_translation_inliers;
    int32_t reserved;
} pdsc_teaser_result;
int32_t pdsc_gnc_tls_rotation(const double *src_tims, const double *dst_tims, int32_t K, double noise_bound,
                              double gnc_factor, int32_t max_iterations, double cost_threshold, double *R,
                              double *weights /* may be NULL */, int32_t *inliers /* may be NULL */,
                              pdsc_gnc_info *info /* may be NULL */, pdsc_stream_t stream);
size_t  pdsc_tls_translation_workspace_bytes(int32_t K);
int32_t pdsc_tls_translation(const double *src, const double *dst, int32_t K, double noise_bound, double *t,
                             int32_t *inliers /* may be NULL */, void *workspace, size_t workspace_bytes,
                             pdsc_stream_t stream);
size_t  pdsc_teaser_solve_workspace_bytes(int32_t N);
int32_t pdsc_teaser_solve(const float *src, const float *tgt, int32_t N, double noise_bound, double gnc_factor,
                          int32_t max_iterations, double cost_threshold, int64_t node_budget,
                          pdsc_teaser_result *result, float *trans_f32 /* may be NULL */,
                          float *labels /* may be NULL */, void *workspace, size_t workspace_bytes,
                          pdsc_stream_t stream);

/* ------------------------------------------------------ f10 GC-RANSAC ------
 * The fork's --algo GC (algorithms/GC_RANSAC.py:8-50 from algorithms/FR.py:70-87;
 * baseline_scripts/baseline_3DMatch.py:101-123): Graph-Cut RANSAC (Barath &
 * Matas, CVPR 2018) for a rigid motion, in the configuration the fork runs:
 * neighborhood 0 (the grid graph), neighborhood_size 20, the uniform sampler.
 * The reference calls the x86 library pygcransac, which is neither installed nor
 * in the reference tree: the definitions below are written from the published
 * algorithm and ARE the contract; parity with the library itself is unpinned
 * (as parity with open3d is for f6).  Nothing here synchronises the stream or
 * allocates; every argument is checked on the host before any device work; all
 * arithmetic is fp64 without contraction in a fixed order and only integer
 * atomics are used: two calls are bitwise equal.  Row i of src [N,3] corresponds
 * to row i of tgt [N,3] (fp32, finite).
 *
 * pdsc_gc_grid: the neighbourhood.  The six axes a = 0 .. 5 are (sx, sy, sz, tx,
 * ty, tz); for an axis with column minimum m and maximum M (fp32) the cell
 * coordinate of x is c = min(G - 1, (int)floor((G * (x - m)) / (M - m))) in fp64
 * from the fp32 values, in that operation order, and c = 0 where M == m; key =
 * sum_a c_a G^(5 - a) as an unsigned 64-bit value.  Two rows are neighbours iff
 * their keys are equal: the graph is a disjoint union of cliques, the cells.
 *   order [N]             the rows sorted by (key, row);
 *   cell_start [N + 1]    capacity; cell k is order[cell_start[k] ..
 *                         cell_start[k + 1]), k < n_cells, cells by ascending key;
 *   cell_of [N]           the cell of each row;
 *   n_cells               device int32.
 * 1 <= G <= 1024 and 1 <= N (else PDSC_ERR_ARG), N <= 262144
 * (PDSC_ERR_UNSUPPORTED; pdsc_gpf_select's bound).  One workgroup: the sort is a
 * bitonic network, in LDS up to 2048 rows and in global memory above.
 *
 * pdsc_gc_label: the graph-cut labelling of the rows under a pose (device
 * double[16], row-major 4x4), threshold eps > 0 and spatial_coherence_weight
 * lambda in [0, 1].  d2_p = |R s_p + t - t_p|^2 as f6's Score; K_p = exp(-(d2_p
 * / (2 eps^2))), 2 eps^2 = 2.0 * (eps * eps).  The energy of a labelling L is
 *   sum_p (1 - lambda) (L_p == 1 ? 1 - K_p : K_p)
 *   + lambda sum over unordered pairs p < q of one cell of
 *       1 if L_p != L_q, (K_p + K_q) / 2 if both are 0, 1 - (K_p + K_q) / 2 if
 *       both are 1
 * (the paper's, with the implementation's convex weighting).  Inside a cell every
 * pair has the same weight (E(0,1) + E(1,0) - E(0,0) - E(1,1) = lambda), so the
 * minimum over all labellings -- what the library's max-flow computes on this
 * graph -- is found per cell of n rows exactly:
 *   sort the rows by (d2, row) ascending; P(m) = K of the first m rows summed
 *   sequentially in that order from 0.0, S = P(n); with m, n as doubles
 *     u = (m - 2 P(m)) + S
 *     a = m (n - m);  b = (((n - m) - 1) 0.5) (S - P(m))
 *     c = (m (m - 1)) 0.5;  d = ((m - 1) 0.5) P(m)
 *     E(m) = (1 - lambda) u + lambda (((a + b) + c) - d)
 *   m* = argmin of E over m = 0 .. n, ties to the lower m (with ties to the higher
 *   m, lambda = 1 would label every singleton an inlier); the first m* rows of
 *   the cell get label 1.
 * labels [N] fp32 0/1; count (device int32) = the rows labelled 1.  Debug (a HOST
 * struct of device pointers, any may be NULL): d2 [N]; per cell m_star, energy =
 * E(m*) and energy_gap = the second-lowest of the n + 1 values minus the lowest.
 * Correct for every cell size 1 .. N (one far outlier stretches an axis and can
 * put almost every row in one cell).  The split by cell size: up to
 * pdsc_gc_cell_bound(0) = 64 rows one wavefront sorts in registers; up to
 * pdsc_gc_cell_bound(1) = 1024 rows one workgroup sorts in LDS; above, the
 * workgroup sorts in the cell's segment of the workspace.  The energies and the
 * argmin are parallel, the prefix sum is sequential: a cell of n rows costs n
 * dependent additions and O(n log^2 n) compares.
 *
 * pdsc_gc_ransac: the solver; H = max_iteration hypotheses h = 0 .. H - 1.
 *   Sampling, Estimate   f6's with ransac_n = 3: the same draw formula and seed,
 *               the same Kabsch; a repeated index gives status (count) -1.
 *   Score       MSAC: an inlier has d2 < eps^2 (eps^2 = eps * eps); score = sum
 *               over the inliers of (1 - d2 / eps^2) and count = the inliers, in
 *               f6's order: chunks of 256 rows, each summed in row order from
 *               0.0, then the chunks in order from 0.0.
 *   Rounds      pdsc_gc_ransac_round() = pdsc_ransac_round() hypotheses per round
 *               (f6's size: no measurement argued for another; it is part of the
 *               result's definition).  The round's best: the higher score, then
 *               the lower h.  If its score is higher than the so-far-best's (none
 *               yet: -1) it is the candidate, and with local_optimization != 0
 *               the LO runs from it (lo_runs += 1), theta = the candidate, for at
 *               most 10 steps (lo_steps += 1 for every step that labels):
 *                 1. label under theta as above; stop if fewer than 3 rows get 1;
 *                 2. theta' = one unit-weight fp64 Kabsch over the labelled rows
 *                    (f6's refit over that row set);
 *                 3. if score(theta') > score(theta): theta = theta' (with its
 *                    score and count) and continue; otherwise stop.
 *               theta after the LO has the higher score of the round's best and
 *               the LO's result; it becomes the so-far-best (best stays the h of
 *               the round's best).  A round whose best does not beat the
 *               so-far-best changes nothing.
 *   Stop        f6's rule at round granularity with exponent 3 and f = the
 *               so-far-best's count / N: after round r, when confidence < 1 and
 *               count > 0, stop if count = N or (r + 1) round >= log(1 -
 *               confidence) / log(1 - f f f).
 *   Result      labels [N] = 1 where d2 < eps^2 under the so-far-best, n_inliers
 *               their number, score its score; trans = pdsc_refit_inliers' fit of
 *               that pose over the same rows (the same code: bitwise equal; the
 *               pose itself with fewer than 3 inliers); trans_f32 = (float)
 *               trans.  n_cells = the grid's (0 with local_optimization == 0,
 *               which builds no grid and ignores lambda and G beyond the argument
 *               check).  Without a valid hypothesis: the identity, zeros, best -1.
 *   Device loop as f6: nothing synchronises, every round and every LO step is
 *               enqueued up front, work after the stop (and LO steps that have
 *               nothing to do) returns at entry.
 *   Deviations from the library: the LO runs at round granularity, not at each
 *               new best; its refit is a least-squares fit over all labelled rows
 *               where the library draws inner samples of 7 x the minimal size;
 *               SPRT pre-emption is left out (it only saves CPU time), and so are
 *               the fork's edge-length pre-emption (its C++ is not in the tree),
 *               PROSAC and the FLANN neighbourhood.
 *   Errors      PDSC_ERR_ARG for N < 3, max_iteration < 1, threshold <= 0 or not
 *               finite, confidence outside (0, 1], lambda outside [0, 1], G
 *               outside [1, 1024], null src / tgt / workspace, a workspace that
 *               is too small; PDSC_ERR_UNSUPPORTED for N > 262144.
 * Debug rows (H = max_iteration) as f6's: count -3 for hypotheses never drawn,
 * samples for every drawn one, score / trans only for valid ones.             */
typedef struct pdsc_gc_label_debug {  /* HOST struct of device pointers, any may be NULL */
    double  *d2;                      /* [N] */
    int32_t *m_star;                  /* [n_cells] (capacity N) */
    double  *energy;                  /* [n_cells] */
    double  *energy_gap;              /* [n_cells] */
} pdsc_gc_label_debug;
typedef struct pdsc_gc_ransac_result { /* device memory, written by the call */
    double  trans[16];                /* fp64 row-major, source -> target */
    double  score;                    /* the so-far-best's MSAC score */
    int32_t n_inliers;
    int32_t iterations;               /* hypotheses drawn: a multiple of the round, or max_iteration */
    int32_t best;                     /* h of the round's best the result descends from, -1: none valid */
    int32_t lo_runs, lo_steps;
    int32_t n_cells;
} pdsc_gc_ransac_result;
typedef struct pdsc_gc_ransac_debug { /* any member may be NULL; H = max_iteration */
    int32_t *samples;                 /* [H,3] */
    int32_t *count;                   /* [H]: inliers, -1 repeated index, -3 not drawn */
    double  *score;                   /* [H] */
    double  *trans;                   /* [H,16] */
} pdsc_gc_ransac_debug;
int32_t pdsc_gc_cell_bound(int32_t which);  /* 0: rows of a wavefront cell, 1: of an LDS cell, else 0 */
size_t  pdsc_gc_grid_workspace_bytes(int32_t N);
int32_t pdsc_gc_grid(const float *src, const float *tgt, int32_t N, int32_t G, int32_t *order, int32_t *cell_start,
                     int32_t *cell_of, int32_t *n_cells, void *workspace, size_t workspace_bytes,
                     pdsc_stream_t stream);
size_t  pdsc_gc_label_workspace_bytes(int32_t N);
int32_t pdsc_gc_label(const double *pose, const float *src, const float *tgt, int32_t N, const int32_t *order,
                      const int32_t *cell_start, const int32_t *n_cells, double threshold,
                      double spatial_coherence_weight, float *labels, int32_t *count,
                      const pdsc_gc_label_debug *debug /* may be NULL */, void *workspace, size_t workspace_bytes,
                      pdsc_stream_t stream);
int32_t pdsc_gc_ransac_round(void);
size_t  pdsc_gc_ransac_workspace_bytes(int32_t N);
int32_t pdsc_gc_ransac(const float *src, const float *tgt, int32_t N, double threshold,
                       double spatial_coherence_weight, int32_t neighborhood_size, int32_t max_iteration,
                       double confidence /* 1.0: never stop early */, uint64_t seed, int32_t local_optimization,
                       float *trans_f32 /* may be NULL */, float *labels /* [N] 0/1, may be NULL */,
                       pdsc_gc_ransac_result *result /* may be NULL */,
                       const pdsc_gc_ransac_debug *debug /* HOST struct of device pointers, may be NULL */,
                       void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* --------------------------- f11 information matrix (multiway registration) --
 * open3d's get_information_matrix_from_point_clouds, which the multiway driver
 * calls once per fragment pair (multiway/test_multi_ate.py:141-146; its [5][5]
 * entry decides whether the pair becomes a loop-closure edge, :147) and at the
 * last scale of multi_scale_icp (:69-72).  open3d's algorithm restated (parity
 * with open3d itself is unpinned).  The correspondences are exactly those of
 * pdsc_icp_point_to_point's evaluate(trans): q = R p + t in fp64, the nearest
 * target point with fp64 d^2 <= max_distance^2, ties to the lower target index
 * (the same device function).  Every correspondence adds G^T G for its target
 * point (x, y, z) -- promoted to fp64, NOT transformed -- and the rows
 * (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1): info is built
 * from 10 sums (the count, sum t, the six entries of sum t t^T), each reduced
 * per 256-point source chunk by xor shuffles and an LDS stage and then over the
 * chunks in order by one wave -- no float atomics, two calls are bitwise equal.
 * info[0][0] = Syy + Szz, info[1][1] = Sxx + Szz, info[2][2] = Sxx + Syy,
 * info[5][5] = n_corr; without a correspondence info is the zero matrix.
 * Like f5 the call synchronises `stream` once at the end to report the grid
 * error (target extent / max_distance >= 2^21 cells: PDSC_ERR_ARG).  Other
 * errors (PDSC_ERR_ARG, on the host before any device work): Ns or Nt < 1,
 * max_distance <= 0 or not finite, null source / target / result / workspace,
 * a workspace that is too small.                                             */
typedef struct pdsc_information_result { /* device memory, written by the call */
    double  info[36];                    /* row-major [6,6] */
    int32_t n_corr;
    int32_t pad;
} pdsc_information_result;
size_t  pdsc_information_matrix_workspace_bytes(int32_t Ns, int32_t Nt);
int32_t pdsc_information_matrix(const float *source, int32_t Ns, const float *target, int32_t Nt,
                                const double *trans /* device double[16], NULL = identity */, double max_distance,
                                pdsc_information_result *result,
                                int32_t *corr /* [Ns]: target index or -1, may be NULL */, void *workspace,
                                size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------ f12 pose-graph optimisation (multiway) -------
 * open3d's global_optimization with GlobalOptimizationLevenbergMarquardt, as
 * multiway/test_multi_ate.py:166-174, 217-224 and multiway/optimize_posegraph.py
 * call it: the step that throws out false loop closures.  open3d's algorithm
 * restated (parity with open3d itself is unpinned); what follows is the contract.
 * All arithmetic is fp64, no float atomics, every sum in a fixed order: two
 * calls are bitwise equal.  The whole two-pass optimisation is one launch of
 * one workgroup.  Every pointer but options / criteria is device memory.
 *   Inputs      poses [n,16]: node frame -> world, row-major, updated in place
 *               (the last row is taken to be 0 0 0 1).  Edge k: edge_src[k],
 *               edge_tgt[k]; edge_trans [E,16] maps the source node's frame into
 *               the target node's (~ pose_t^-1 pose_s, test_multi_ate.py:
 *               129-135); edge_info [E,36], taken to be symmetric; edge_uncertain
 *               [E] (non-zero: a loop closure the line process may switch off).
 *   Residual    e = vec6(X^-1 Tt^-1 Ts), vec6(M) = (atan2(M21, M22), atan2(-M20,
 *               sy), atan2(M10, M00), M03, M13, M23), sy = sqrt(M00^2 + M10^2);
 *               sy < 1e-6: (atan2(-M12, M11), atan2(-M20, sy), 0).  Inverses are
 *               (R^T, -R^T t); every product is ((a0 b0 + a1 b1) + a2 b2) (+ a3).
 *   Jacobians   D_i the se(3) generators (rotations about x, y, z, translations):
 *               column i of Js = lin6(X^-1 Tt^-1 D_i Ts), of Jt = lin6(X^-1 Tt^-1
 *               (-D_i) Ts) = -Js; lin6(M) = ((M21 - M12) / 2, (M02 - M20) / 2,
 *               (M10 - M01) / 2, M03, M13, M23).
 *   Line proc.  mu = preference_loop_closure max_correspondence_distance^2 mean
 *               over the pass's uncertain edges of info[5][5] (0 without any);
 *               l = 1 for certain edges, (mu / (mu + e^T L e))^2 for uncertain
 *               ones (1 where mu + e^T L e is not positive).
 *               F = sum l e^T L e + mu sum over uncertain edges (sqrt(l) - 1)^2.
 *   System      B = Js^T L Js per edge (entries r <= c computed and mirrored, so H
 *               is symmetric bit for bit), g = Js^T L e: H_ss += l B, H_tt += l B,
 *               H_st -= l B, H_ts -= l B, b_s -= l g, b_t += l g, each 6x6 block
 *               summed over its edges in ascending edge index; then the reference
 *               node's rows and columns are zeroed, their diagonal 1, its b 0.
 *   LM          lambda = 1e-5 max diag H, nu = 2; nothing runs if max b <
 *               min_right_term or F < min_residual.  At most max_iteration outer
 *               iterations, each at most max_iteration_lm + 1 times (one more
 *               stops the pass): solve (H + lambda I) delta = b (blocked Cholesky
 *               on 6x6 blocks); stop if |delta| < min_relative_increment (|x| +
 *               min_relative_increment), x the stacked vec6 of the poses; trial
 *               poses Exp(delta_i) pose_i, Exp(d) = Rz(d2) Ry(d1) Rx(d0) with
 *               translation d3..5; rho = (F - F_new) / (delta . (lambda delta + b)
 *               + 1e-3), F_new under the current l.  rho > 0: stop if F - F_new <
 *               min_relative_residual_increment F, else accept the trial poses,
 *               recompute l, F under the new l, H and b, lambda *= max(1/3, 1 -
 *               (2 rho - 1)^3), nu = 2, and stop if max b < min_right_term.
 *               Otherwise lambda *= nu, nu *= 2.  An outer iteration ends with
 *               the F < min_residual test.
 *   Two passes  over all edges; then edge_keep = !uncertain || confidence >
 *               edge_prune_threshold; then over the kept edges, mu and l
 *               recomputed over them.  confidence [E] = the final l (a dropped
 *               edge keeps its pass-1 value).
 *   Failure     a Cholesky pivot that is not positive and finite sets
 *               solver_failed: the loop stops, the last accepted poses stay.
 *   Errors      on the host, before any device work: PDSC_ERR_ARG for n < 1, E <
 *               0, reference_node outside [0, n), null required pointers (the
 *               edge arrays, confidence and edge_keep may be NULL when E = 0),
 *               max_correspondence_distance <= 0, a negative preference, a
 *               workspace that is too small; PDSC_ERR_UNSUPPORTED for n > 256 or
 *               E > 32768 (the workspace query returns 0 there: the dense H and
 *               its factor are 2 x 18.9 MB at n = 256).  An edge with src == tgt
 *               or an id outside [0, n) is found on the device and reported
 *               (PDSC_ERR_ARG) after the call's single final synchronise; nothing
 *               is optimised then.
 * pdsc_pose_graph_linearize is one linearisation by the same device functions:
 * given poses, edges, l (line_process [E], NULL = all 1) and mu it returns
 * residual [E,6], objective [1] = F, H [6n,6n] and b [6n].                    */
#define PDSC_PG_MAX_ITERATION 100
#define PDSC_PG_MAX_ITERATION_LM 20
#define PDSC_PG_MIN_RELATIVE_INCREMENT 1e-6
#define PDSC_PG_MIN_RELATIVE_RESIDUAL_INCREMENT 1e-6
#define PDSC_PG_MIN_RIGHT_TERM 1e-6
#define PDSC_PG_MIN_RESIDUAL 1e-6
typedef struct pdsc_pose_graph_options { /* HOST; open3d's GlobalOptimizationOption */
    double  max_correspondence_distance;
    double  edge_prune_threshold;
    double  preference_loop_closure;
    int32_t reference_node;
    int32_t pad;
} pdsc_pose_graph_options;
typedef struct pdsc_pose_graph_criteria { /* HOST; open3d's GlobalOptimizationConvergenceCriteria */
    int32_t max_iteration;
    int32_t max_iteration_lm;
    double  min_relative_increment;
    double  min_relative_residual_increment;
    double  min_right_term;
    double  min_residual;
} pdsc_pose_graph_criteria;
typedef struct pdsc_pose_graph_result { /* device memory, written by the call */
    double  objective[2];               /* F at the end of each pass */
    double  mu[2];                      /* of each pass */
    int32_t iterations[2];              /* outer iterations of each pass */
    int32_t edges_kept;
    int32_t solver_failed;
} pdsc_pose_graph_result;
size_t  pdsc_pose_graph_workspace_bytes(int32_t n, int32_t E);
int32_t pdsc_pose_graph_optimize(double *poses, int32_t n, const int32_t *edge_src, const int32_t *edge_tgt,
                                 const double *edge_trans, const double *edge_info, const int32_t *edge_uncertain,
                                 int32_t E, const pdsc_pose_graph_options *options,
                                 const pdsc_pose_graph_criteria *criteria /* NULL: the defaults above */,
                                 double *confidence, int32_t *edge_keep, pdsc_pose_graph_result *result,
                                 void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_pose_graph_linearize(const double *poses, int32_t n, const int32_t *edge_src, const int32_t *edge_tgt,
                                  const double *edge_trans, const double *edge_info, const int32_t *edge_uncertain,
                                  int32_t E, const double *line_process, double mu, int32_t reference_node,
                                  double *residual, double *objective, double *H, double *b, void *workspace,
                                  size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------ f13 RGB-D odometry, hybrid term (fragments) --
 * open3d 0.10's compute_rgbd_odometry with RGBDOdometryJacobianFromHybridTerm, as
 * multiway/make_fragments.py:41-61 calls it on adjacent frames, batched over P
 * frame pairs of one sequence of F frames.  open3d's Odometry.cpp restated (parity
 * with open3d itself is unpinned); what follows is the contract.  All P pairs
 * advance together (the pair is a grid dimension), no host synchronisation between
 * iterations; the call synchronises `stream` once at the end.  A pair's result is
 * bitwise independent of the rest of the batch; two calls are bitwise equal.
 *   Inputs     intensity, depth fp32 [F,H,W] (device; depth in metres, 0 =
 *              invalid); pinhole fx, fy, cx, cy; pair_src, pair_tgt HOST int32 [P]
 *              (checked on the host, copied on the stream); init device fp64
 *              [P,16], NULL = identity; options on the host.
 *   Outputs    trans [P,16] (source frame -> target frame), info [P,36], status [P].
 *   1 frames   once per frame, fp32, shared by all pairs.  Depth d with d <
 *              min_depth, d > max_depth or d <= 0 becomes NaN (open3d's test; the
 *              bounds themselves stay).  Intensity and depth get a 3x3 Gaussian:
 *              g(a, b, c) = (0.25 a + 0.5 b) + 0.25 c along u with clamped reads,
 *              each row's value rounded to fp32, then the same along v; NaN
 *              propagates.  Level l + 1 is the 2x2 mean (((p00 + p10) + p01) + p11)
 *              0.25 (pXY: x = u offset) of level l; intensity is Gaussian-filtered
 *              again before each downsample, depth is not.  Sobel with clamped
 *              reads: dx = (h(v-1) + 2 h(v)) + h(v+1), h(v) = img(u+1, v) -
 *              img(u-1, v); dy = (k(u-1) + 2 k(u)) + k(u+1), k(u) = img(u, v+1) -
 *              img(u, v-1).  Level l's intrinsics are scaled by 2^-l (fp64).  The
 *              xyz image is not stored: X = ((u - cx) d) / fx, Y likewise, Z = d in
 *              fp64 from the fp32 depth where it is read (open3d stores fp32 xyz).
 *   2 scales   a_s = 0.5 / mean I_s, a_t = 0.5 / mean I_t over the level-0
 *              correspondences under init (fp64 sums of the fp32 values in f11's
 *              fixed order); both 1 without a correspondence.  Every filter is
 *              linear, so the scalars are applied where I and its gradients are read.
 *   3 corr.    a source pixel i = v W + u with finite depth: p = R X + t (f12's
 *              product order); needs p.z > 0; uf = (fx p.x) / p.z + cx + 0.5, vf
 *              likewise; inside iff -1 < uf < W and -1 < vf < H; u_t = int(uf)
 *              (truncation: uf in (-1, 0) is column 0, as open3d's cast); D_t(u_t,
 *              v_t) finite and |p.z - D_t| <= max_depth_diff.  A target pixel keeps
 *              the source pixel of the smallest p.z ROUNDED TO FP32, ties to the
 *              lowest source index: one 64-bit atomic min on (fp32 bits of p.z,
 *              source index) -- no order dependence.
 *   4 rows     fp64 from the fp32 images; lambda_dep = 0.968, lambda_img = 1 -
 *              lambda_dep, Sobel scale 0.125, NaN gradients count as 0.  r_I =
 *              sqrt(lambda_img) (a_t I_t - a_s I_s), r_D = sqrt(lambda_dep) (D_t -
 *              p.z).  c = 0.125 a_t (I_dx fx / p.z, I_dy fy / p.z) (target
 *              gradients at (u_t, v_t)), c2 = -(c0 p.x + c1 p.y) / p.z: J_I =
 *              sqrt(lambda_img) (-p.z c1 + p.y c2, p.z c0 - p.x c2, -p.y c0 + p.x
 *              c1, c0, c1, c2); d likewise from the depth gradients (without a_t):
 *              J_D = sqrt(lambda_dep) (-p.z d1 + p.y d2 - p.y, p.z d0 - p.x d2 +
 *              p.x, -p.y d0 + p.x d1, d0, d1, d2 - 1).
 *   5 solve    28 fp64 sums (J^T J's upper triangle row-major, J^T r, the count)
 *              per 256-target-pixel chunk by xor shuffles and an LDS stage, then
 *              over the chunks in order (f11's reduction; no float atomics).  J^T J
 *              x = -J^T r by 6x6 Cholesky in one wave; T <- Exp(x) T with f12's Exp.
 *              A pivot that is not positive and finite, a non-finite x, or zero
 *              correspondences end that pair: success = 0, trans as last accepted.
 *              iterations[k] iterations at level 2 - k (coarsest first).  success
 *              = no iteration failed: with iterations = (0, 0, 0) it is 1,
 *              n_corr_last and iterations_run are 0 and trans is init bit for bit.
 *   6 info     over the level-0 correspondences under the final trans: f11's G^T G
 *              of the back-projected target point ((u_t - cx) D_t / fx, .., D_t),
 *              f11's reduction.  Zero without a correspondence.
 *   Errors     PDSC_ERR_ARG on the host before any device work: null required
 *              pointers, H or W below 8 or not divisible by 4, F < 1, P < 1, a pair
 *              index outside [0, F) or src == tgt, intrinsics or max_depth_diff not
 *              positive and finite, not 0 <= min_depth < max_depth, iterations
 *              outside [0, 1000], a workspace that is too small.  F or P above
 *              65535, or H W above 2^26: PDSC_ERR_UNSUPPORTED (the workspace query
 *              returns 0).
 * pdsc_rgbd_odometry_linearize is one linearisation by the same kernels: steps 1
 * and 2 with `trans` as init, then at `level` the correspondence map corr
 * [P, H_l W_l] (target pixel -> source pixel or -1; may be NULL), sums [P,28] (step
 * 5's, in that order) and scales [P,2] = (a_s, a_t) (may be NULL).
 * pdsc_rgbd_odometry_pyramid is step 1 alone, by the same launches and frame
 * checks (exposed so that tests can see the images): level `level` of all F
 * frames into six device fp32 arrays [F, H_l, W_l], each may be NULL; workspace of
 * pdsc_rgbd_odometry_workspace_bytes(F, H, W, 1).
 * pdsc_rgbd_from_color_and_depth is open3d's create_from_color_and_depth: color
 * uint8 [F,H,W,3], depth16 uint16 [F,H,W] -> intensity = ((0.299 R + 0.587 G) +
 * 0.114 B) / 255 and depth = depth16 / depth_scale, 0 where that is above
 * depth_trunc (fp32; asynchronous).                                          */
typedef struct pdsc_rgbd_odometry_options { /* HOST; open3d's OdometryOption */
    double  max_depth_diff;
    double  min_depth;      /* open3d: 0 */
    double  max_depth;      /* open3d: 4.0 */
    int32_t iterations[3];  /* coarsest level first; open3d: 20, 10, 5 */
    int32_t pad;
} pdsc_rgbd_odometry_options;
typedef struct pdsc_rgbd_odometry_status { /* device memory, one per pair */
    int32_t success;
    int32_t n_corr_last;    /* correspondences of the last linearisation */
    int32_t iterations_run; /* accepted updates */
    int32_t pad;
} pdsc_rgbd_odometry_status;
size_t  pdsc_rgbd_odometry_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t P);
int32_t pdsc_rgbd_odometry(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W, double fx,
                           double fy, double cx, double cy, const int32_t *pair_src, const int32_t *pair_tgt, int32_t P,
                           const double *init, const pdsc_rgbd_odometry_options *options, double *trans, double *info,
                           pdsc_rgbd_odometry_status *status, void *workspace, size_t workspace_bytes,
                           pdsc_stream_t stream);
int32_t pdsc_rgbd_odometry_linearize(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W,
                                     double fx, double fy, double cx, double cy, const int32_t *pair_src,
                                     const int32_t *pair_tgt, int32_t P, const double *trans,
                                     const pdsc_rgbd_odometry_options *options, int32_t level, int32_t *corr,
                                     double *sums, double *scales, void *workspace, size_t workspace_bytes,
                                     pdsc_stream_t stream);
int32_t pdsc_rgbd_odometry_pyramid(const float *intensity, const float *depth, int32_t F, int32_t H, int32_t W,
                                   double min_depth, double max_depth, int32_t level, float *I, float *D, float *Idx,
                                   float *Idy, float *Ddx, float *Ddy, void *workspace, size_t workspace_bytes,
                                   pdsc_stream_t stream);
int32_t pdsc_rgbd_from_color_and_depth(const uint8_t *color, const uint16_t *depth16, int32_t F, int32_t H, int32_t W,
                                       double depth_scale, double depth_trunc, float *intensity, float *depth,
                                       pdsc_stream_t stream);

/* ------------------------------ f14 sparse TSDF volume (fragments) -----------
 * open3d's ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) as multiway/
 * make_fragments.py:116-139 uses it: integrate every frame, keep the vertices and
 * vertex colours of extract_triangle_mesh (no triangles are built).  Restated;
 * parity with open3d itself is unpinned.  ALL the state lives in one caller-owned
 * device buffer, `workspace`, of pdsc_tsdf_workspace_bytes(max_blocks) bytes, that
 * pdsc_tsdf_reset initialises; every call takes the same max_blocks.  Its first
 * int32 is the number of blocks that own a pool slot.
 *   Storage    blocks of 16^3 voxels, block edge = 16 voxel_length, block index =
 *              floor(p / edge) per axis in [-2^20, 2^20) (else PDSC_ERR_UNSUPPORTED
 *              after the call's synchronise); key = (bx + 2^20) << 42 | (by + 2^20)
 *              << 21 | (bz + 2^20).  An open-addressing hash (>= 4 max_blocks
 *              entries) from key to pool slot, insertion one 64-bit CAS, slots from
 *              an atomic counter.  Per voxel (index x + 16 y + 256 z in its block):
 *              tsdf, weight fp32, colour 3 x fp32 in 0 .. 255; 80 KB per block.
 *   integrate  depth fp32 [H,W] metres, colour uint8 [H,W,3], extrinsic fp64 [16]
 *              world -> camera (device).  Touch: every pixel (u, v) with u and v
 *              multiples of 4 and depth > 0 is back-projected (((u - cx) d) / fx, ..,
 *              d) and moved to the world by the extrinsic's inverse (R^T, -R^T t),
 *              fp64, f12's product order; every block between floor((p - sdf_trunc)
 *              / edge) and floor((p + sdf_trunc) / edge) per axis is inserted if
 *              absent and marked touched.  Then ONLY the blocks this frame touched
 *              are integrated, one workgroup each; per voxel: centre (idx + 0.5)
 *              voxel_length to the camera; z > 0; uf = (fx x) / z + cx + 0.5, u =
 *              int(uf) (f13's inside test); d = depth(u, v) > 0; sdf = (d - z)
 *              sqrt((((u - cx) / fx)^2 + ((v - cy) / fy)^2) + 1) in fp64; if sdf >
 *              -sdf_trunc: tsdf_new = (float) min(1, sdf / sdf_trunc), tsdf <- (tsdf
 *              w + tsdf_new) / (w + 1) in fp32, each colour channel likewise, w <-
 *              w + 1.  IEEE operations, no contraction.
 *   Overflow   more blocks than max_blocks (or a full hash): PDSC_ERR_UNSUPPORTED
 *              after the call's one final synchronise; that frame changes no voxel;
 *              blocks that got a slot stay, at weight 0.
 *   Range      a block index outside [-2^20, 2^20) or a non-finite point, in
 *              integrate or write_blocks: PDSC_ERR_UNSUPPORTED likewise; the call
 *              changes no voxel and NO block gets a slot, so the block count and
 *              every block read back are as before the call.  The keys the failed
 *              call named keep their hash entries without a slot, as the surplus
 *              keys of an overflow do (open addressing cannot delete): a later
 *              call finds and reuses them, but calls that keep failing on FRESH
 *              blocks can use up the 4 max_blocks entries, and the volume then
 *              reports "full" below max_blocks blocks until pdsc_tsdf_reset.
 *   extraction a cube at voxel v is valid when all 8 corners v + {0,1}^3 exist and
 *              have weight != 0 (a corner may lie in a neighbouring block).  The
 *              edge (v, axis) from v to v + e_axis, f0 = tsdf(v), f1 = tsdf(v +
 *              e_axis), is emitted once iff (f0 < 0) != (f1 < 0) and at least one of
 *              its four adjacent cubes is valid.  Position (fp64): (idx + 0.5)
 *              voxel_length with the axis coordinate moved by |f0| voxel_length /
 *              (|f0| + |f1|); colour (|f1| c0 + |f0| c1) / (|f0| + |f1|) / 255.
 *              Output in ascending (block key, voxel index, axis) order: slot
 *              assignment never shows and two runs are bitwise equal.
 *              pdsc_tsdf_count_surface_points returns the count (it synchronises);
 *              the caller allocates points / colours fp64 [n,3] and calls
 *              pdsc_tsdf_emit_surface_points with no integrate / write in between.
 *   blocks     pdsc_tsdf_read_blocks copies the blocks out in slot order (coords
 *              int32 [n,3], tsdf / weight [n,4096], colour [n,4096,3]; any may be
 *              NULL; capacity >= the block count); pdsc_tsdf_write_blocks inserts
 *              the given blocks (if absent) and overwrites their voxels -- a saved
 *              volume, or a state a test fabricates.
 *   Errors     PDSC_ERR_ARG on the host before any device work: null required
 *              pointers, H or W < 1, intrinsics / voxel_length / sdf_trunc not
 *              positive and finite, max_blocks < 1, a state buffer that is too
 *              small; max_blocks > 2^17 (every count and offset of 3 x 4096
 *              edges per block fits an int32): PDSC_ERR_UNSUPPORTED (the query
 *              returns 0).  Two checks need the block / point count the buffer
 *              holds and follow one synchronising read of it: read_blocks'
 *              capacity < the block count and emit's capacity < the point count
 *              (PDSC_ERR_ARG).  emit's points / colours must not be NULL.       */
size_t  pdsc_tsdf_workspace_bytes(int32_t max_blocks);
int32_t pdsc_tsdf_reset(int32_t max_blocks, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_tsdf_integrate(const float *depth, const uint8_t *colour, int32_t H, int32_t W, double fx, double fy,
                            double cx, double cy, const double *extrinsic, double voxel_length, double sdf_trunc,
                            int32_t max_blocks, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_tsdf_read_blocks(int32_t max_blocks, int32_t capacity, int32_t *coords, float *tsdf, float *weight,
                              float *colour, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_tsdf_write_blocks(const int32_t *coords, int32_t n, const float *tsdf, const float *weight,
                               const float *colour, int32_t max_blocks, void *workspace, size_t workspace_bytes,
                               pdsc_stream_t stream);
int32_t pdsc_tsdf_count_surface_points(int32_t max_blocks, int64_t *n_points /* HOST */, void *workspace,
                                       size_t workspace_bytes, pdsc_stream_t stream);
int32_t pdsc_tsdf_emit_surface_points(double voxel_length, int32_t max_blocks, double *points, double *colours,
                                      int64_t capacity, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ------------------------------------------- f8 FCGF descriptors ----------
 * misc/fcgf.py's ResUNetBN2C(in_channels 1, out_channels C_out, conv1_kernel_size
 * 5 | 7, normalize_feature) in eval mode -- the sparse 3-D ResUNet that
 * demo_registration.py:11-35, misc/cal_fcgf.py:12-85 and datasets/
 * LidarFeatureExtractor.py:166-200 run through MinkowskiEngine -- on the GPU.
 * MinkowskiEngine and the released FCGF checkpoints are not available to this
 * build: the semantics below are a restatement, and parity with MinkowskiEngine
 * itself and with the released checkpoints is UNPINNED.  The choices, fixed here:
 *
 *   quantise   coords = floor(xyz / voxel_size) in fp32 (an IEEE divide, not a
 *              reciprocal multiply; misc/cal_fcgf.py:73); one point per occupied
 *              voxel, the one with the lowest input index; voxels in ascending
 *              (batch, x, y, z) key order (pdsc_voxel_down_sample's convention);
 *              callers take xyz[inds], the kept ORIGINAL points, and the input
 *              feature 1 as [m,1].  Coordinates may be negative; each must lie in
 *              [-2^18, 2^18) and the batch index in [0, 64) (a 63-bit key), else
 *              PDSC_ERR_UNSUPPORTED.
 *   levels     tensor strides 1, 2, 4, 8.  A stride-2 convolution at tensor stride
 *              t has the outputs unique(floor(c / 2t) 2t) (floor: negatives round
 *              down).  A transposed convolution creates no coordinates: its outputs
 *              are the encoder's set at that stride, so ME.cat is row-aligned.
 *   kernel map HYPER_CUBE, centred: offsets o in {-r..r}^3 t_in, r = 1, 2, 3 for
 *              kernel sizes 3, 5, 7; output u reads input u + o; the weight index
 *              is k = (o_x + r) + K (o_y + r) + K^2 (o_z + r) (fcgf_kernel_index,
 *              csrc/fcgf.hip).  A checkpoint's kernel axis is read through
 *              fcgf_checkpoint_index (the same order today): if MinkowskiEngine's
 *              offset order differs, that ONE function changes.  A transposed
 *              convolution's map is the stride-2 convolution's with input and
 *              output swapped and the same k (<= 8 coarse parents per voxel).
 *   network    ResUNet2.forward (misc/fcgf.py:800-851), CHANNELS 32/64/128/256,
 *              TR_CHANNELS 64/64/64/128; BasicBlockBN (:142-158);
 *              MinkowskiBatchNorm in eval mode = BatchNorm1d(eps 1e-5) on the rows,
 *              folded into a scale and a shift; concatenation (upsampled, skip);
 *              output F / (||F||_2 + 1e-8) when normalize != 0.  fp32 throughout
 *              (exact fp32 MFMA), fixed summation order, no scatter: results are
 *              bitwise reproducible and independent of the rest of the batch.
 *
 * Parameters: ONE flat fp32 device buffer of pdsc_fcgf_param_floats floats in
 * state-dict order without num_batches_tracked: conv1.kernel [K^3,1,32],
 * norm1.bn.{weight, bias, running_mean, running_var}, block1.conv1.kernel
 * [27,32,32], block1.norm1.bn.*, block1.conv2.kernel, block1.norm2.bn.*,
 * conv2.kernel, norm2.bn.*, block2.*, conv3, norm3, block3, conv4, norm4, block4,
 * conv4_tr, norm4_tr, block4_tr, conv3_tr, norm3_tr, block3_tr, conv2_tr,
 * norm2_tr, block2_tr, conv1_tr.kernel [96,64], final.kernel [64,C_out],
 * final.bias [C_out]; every kernel [K^3, C_in, C_out] row-major.
 * pdsc_fcgf_pack_weights writes the folded device layout (csrc/fcgf.hip:
 * pack_layer_kernel) of pdsc_fcgf_packed_floats floats.  1 <= C_out <= 32.      */
size_t pdsc_fcgf_param_floats(int32_t conv1_kernel_size, int32_t out_channels);
size_t pdsc_fcgf_packed_floats(int32_t conv1_kernel_size, int32_t out_channels);
int32_t pdsc_fcgf_pack_weights(const float *params, int32_t conv1_kernel_size, int32_t out_channels, float *packed,
                               pdsc_stream_t stream);
/* The workspace of pdsc_fcgf_quantize (n_points points) and pdsc_fcgf_forward
 * (m = n_points voxels): a pure function of its arguments that bounds the worst
 * case of every level holding n_points voxels; 0 for unsupported arguments.     */
size_t pdsc_fcgf_workspace_bytes(int32_t n_points, int32_t batch, int32_t conv1_kernel_size, int32_t out_channels);
/* xyz [n,3]; batch_offsets: device int32 [batch + 1], cloud b = points
 * offsets[b] .. offsets[b + 1] - 1 (NULL with batch == 1); inds [n] capacity
 * (input index of each kept point), coords [n,4] capacity (batch, x, y, z), both
 * in ascending key order; *count (device int32) = voxels.  Synchronises `stream`
 * (reports the range error found on the device).                              */
int32_t pdsc_fcgf_quantize(const float *xyz, int32_t n, const int32_t *batch_offsets, int32_t batch, float voxel_size,
                           int32_t *inds, int32_t *coords, int32_t *count, void *workspace, size_t workspace_bytes,
                           pdsc_stream_t stream);
/* Optional intermediates of pdsc_fcgf_forward (any member may be NULL): the
 * feature tensors after block1..4, block4_tr..2_tr and conv1_tr (+ ReLU), each
 * [m, C] capacity with the level's first counts[level] rows valid -- level-1
 * tensors in the caller's row order, coarser ones in ascending key order --,
 * the coordinates [m,4] of the levels of tensor stride 2, 4, 8 and counts [4].  */
typedef struct pdsc_fcgf_debug {
    float *block1;      /* [m,32]   stride 1 */
    float *block2;      /* [m,64]   stride 2 */
    float *block3;      /* [m,128]  stride 4 */
    float *block4;      /* [m,256]  stride 8 */
    float *block4_tr;   /* [m,128]  stride 4 */
    float *block3_tr;   /* [m,64]   stride 2 */
    float *block2_tr;   /* [m,64]   stride 1 */
    float *conv1_tr;    /* [m,64]   stride 1 */
    int32_t *coords2;   /* [m,4] */
    int32_t *coords4;   /* [m,4] */
    int32_t *coords8;   /* [m,4] */
    int32_t *counts;    /* [4] voxels per level */
} pdsc_fcgf_debug;
/* coords [m,4] int32 (batch, x, y, z), unique rows in any order (pdsc_fcgf_quantize's
 * output); feats [m,1] (NULL: the constant 1); out [m, out_channels], row i the
 * descriptor of coords row i.  Synchronises `stream` (range errors).          */
int32_t pdsc_fcgf_forward(const float *packed, int32_t conv1_kernel_size, int32_t out_channels, int32_t normalize,
                          const int32_t *coords, const float *feats, int32_t m, float *out,
                          const pdsc_fcgf_debug *debug, void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ----------------------------------------------- full testing forward ------
 * PointDSC.forward(data) with 'testing' in data (models/PointDSC.py:128-197)
 * for B independent pairs: compat -> encoder -> classifier -> seeds -> kNN ->
 * NSM -> hypotheses -> post-refinement.  corr_pos [B,N,in_dim];
 * src,tgt [B,N,3]; final_trans [B,4,4]; final_labels [B,N].
 * Optional debug outputs (NULL to skip): conf [B,N], seeds [B,S].           */
size_t pdsc_forward_workspace_bytes(const pdsc_config *cfg, int32_t B, int32_t N);
int32_t pdsc_forward_testing(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                             const float *src, const float *tgt, int32_t B, int32_t N,
                             float *final_trans, float *final_labels, float *conf_out,
                             int32_t *seeds_out, void *workspace, size_t workspace_bytes,
                             pdsc_stream_t stream);
/* The same forward with the intermediates of every stage (no reference
 * counterpart: the parity tests pin each stage on the forward's own values).
 * Any member may be NULL.  k = min(cfg->k, N - 1), S = int(N * ratio).       */
typedef struct pdsc_forward_debug {
    float *conf;             /* [B,N] classifier logits (:171) */
    int32_t *seeds;          /* [B,S] (:174) */
    int32_t *knn;            /* [B,S,k] seed neighbourhoods (:250-252) */
    float *weights;          /* [B,S,k] NSM weights (:280-282) */
    float *trans_pre_refine; /* [B,4,4] the best hypothesis (:182) */
} pdsc_forward_debug;
int32_t pdsc_forward_testing_debug(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                                   const float *src, const float *tgt, int32_t B, int32_t N,
                                   float *final_trans, float *final_labels, const pdsc_forward_debug *debug,
                                   void *workspace, size_t workspace_bytes, pdsc_stream_t stream);

/* ---------------------------------------------- ragged testing forward -----
 * B pairs of DIFFERENT sizes in one call: the evaluation loop's pairs
 * (datasets/ThreeDMatch.py:268-290 keeps every keypoint, so N varies per pair;
 * evaluation/test_3DMatch.py:33-53 runs them one by one at bs = 1).  Each pair
 * b occupies the first counts[b] rows of N-row buffers (corr_pos [B,N,in_dim],
 * src/tgt [B,N,3]; rows past counts[b] are ignored), and the result equals B
 * separate bs = 1 forwards: final_trans [B,4,4]; final_labels [B,N] with rows
 * past counts[b] set to 0.  counts: HOST int32 [B] (passed to the device as
 * kernel arguments, no copy on the stream), each with min(cfg->k, count - 1)
 * = min(cfg->k, N - 1) (every pair keeps the batch's k) and int(count *
 * ratio) >= 1.  debug: as pdsc_forward_testing_debug (may be NULL), with the
 * batch's strides S = int(N * ratio) and k; conf rows past counts[b], and seeds,
 * knn and weights entries past a pair's own seeds, are unspecified.
 * From 32 pairs on the fused encoder plan the encoder runs as two half batches,
 * one on `stream` and one on a per-device side stream the library owns, forked
 * from and joined back into `stream` by events (still asynchronous; the same
 * results as one stream; environment PDSC_ENC_HALVES=0 keeps one stream).
 * Workspace: pdsc_forward_workspace_bytes(cfg, B, N).                        */
int32_t pdsc_forward_testing_ragged(const pdsc_config *cfg, const float *packed, const float *corr_pos,
                                    const float *src, const float *tgt, int32_t B, int32_t N,
                                    const int32_t *counts, float *final_trans, float *final_labels,
                                    const pdsc_forward_debug *debug, void *workspace, size_t workspace_bytes,
                                    pdsc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDSC_H_ */
