// launch_plan.hpp -- which kernels a call runs at a shape, and with which grids.
// Host-only.  The process's knobs are read once, into Knobs.  plan_encoder
// (encoder.hip) and plan_tail (seeds.hip), each beside the kernels' grid helpers
// it calls, decide once per call from the call's sizes and the knobs; the entries
// size the workspace by the plans and the launchers launch what they say.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "pdsc_internal.hpp"

namespace pdsc {

constexpr int ENC_MAX_PARTS = 4;  // parts of a batch the forward's encoder may run on side streams (encoder.hip)

// Every run-time knob of libpdsc.so (A/B measurement and bit-identity tests only;
// the defaults are the product), read once per process, each as an integer
// (atoi).  Not here: PDSC_ICP_ONE_WG, which api.hip reads at every call on
// purpose (tests toggle it within a process), and PDSC_LIB_VARIANT, which the
// Python loader reads to pick the library file.
struct Knobs {
    // ---- the encoder's attention (plan_encoder)
    // PDSC_ATT_TARGET: resident workgroups per round of the split-K decomposition
    // (2 per CU on 256 CUs; attention_split_count).  (The exact-fp32 attention
    // keeps its round-2 rule: splits = ceil(target / blocks).)
    int target;
    int nw;          // PDSC_ATT_NW=1|2|4: the small batches' waves per workgroup (plan_encoder); not 1 or 2 means 4
    int tiny;        // PDSC_ATT_TINY=n: the tiny plan up to n blocks of 128 queries; 0: off
    int tiny_slots;  // PDSC_ATT_TINY_SLOTS: the tiny plan's slot target
    int ws;          // PDSC_ATT_WS=1|2|4: the tiny plan's waves per key split; 1 = the one-wave kernel
    int w64;         // PDSC_W64: 0 never, 1 wherever the split path runs, else the 128-block rule
    bool w64_sk;     // PDSC_W64_SK=0: never the stream-K form
    bool fuse;       // PDSC_FUSE=0: attention and pointwise chain stay two launches
    bool precombine; // PDSC_PRECOMBINE=0: never
    int zigzag;      // PDSC_ZIGZAG: 0 off, 2 inverted
    bool dense_m;    // PDSC_DENSE_M=1: the forward writes and reads M dense
    bool vfold;      // PDSC_VFOLD=0: no plan folds fc_message[0] into V (EncoderPlan::vfold)
    // ---- the encoder's pointwise chain (plan_encoder)
    int pw2;             // PDSC_PW2: 0 never, 2 always, else the 320-workgroup rule
    int pw_small_limit;  // PDSC_PW_SMALL_LIMIT: 32-point tiles below this many 64-point tiles (512)
    bool pw_waves8;      // PDSC_PW_WAVES=4: never the 8-wave pw_mid
    bool pw_qkv_split;   // PDSC_PW_QKV_SPLIT=0: one workgroup per point tile writes Q, K and V (the same bits either way)
    bool pw_prefetch;    // PDSC_PW_PREFETCH=0: the Q / K / V split chain without the panel prefetch (message_resid + pcn_qkv8)
    // ---- the encoder parts (encoder.hip) and the ragged order (api.hip) of the forward
    int enc_halves;  // PDSC_ENC_HALVES: 0 never, 1 uniform batches too, else ragged batches only
    int enc_parts;   // PDSC_ENC_PARTS=P in [2, ENC_MAX_PARTS] (default 2)
    // PDSC_ENC_BAL=1: parts of equal work sum(n^2) instead of equal pair counts
    // (measured slower: 128 pairs, N in [700, 1300], 4.150 / 4.159 vs 4.021 /
    // 4.056 ms per forward, one stream 4.423 / 4.437).
    bool enc_bal;
    bool ragged_order;  // PDSC_RAGGED_ORDER=0: the ragged attention workgroups stay in pair order
    // ---- the tail (plan_tail)
    int seed_blocks;    // PDSC_SEED_BLOCKS: the 16-row seed kernels below this many blocks of 64 rows (1024)
    bool seed_sort;     // PDSC_SEED_SORT=1: the bitonic-sorted NMS and seed ranking
    int lm_rpt;         // PDSC_LM_RPT=1|2|4: the NMS compare's rows per thread at every batch size; 0: plan_tail's rule
    int seed_select;    // PDSC_SEED_SELECT: 0 never the select form, 1 at every batch size, else the 1e8-compare rule
    bool sel_split;     // PDSC_SEL_SPLIT=0: the select form's A^2 candidate compares stay in its one launch
    int seed_wpb;       // PDSC_SEED_WPB=1|2|4: waves per one-wave-per-seed workgroup; 0: plan_tail's rule
    int knn_bitonic;    // PDSC_KNN_BITONIC=0: the kNN fast path's readlane compare ranking (knn_select_kernel's argument)
    bool kabsch_fused;  // PDSC_KABSCH_FUSED=0: the separate Kabsch solve kernel at every batch size (the same bits either way)
    bool tail_fused;    // PDSC_TAIL_FUSED=0: the testing forward's unfused tail launches
};
inline const Knobs &knobs() {
    static const Knobs k = [] {
        auto env_int = [](const char *name, int dflt) {
            const char *e = getenv(name);
            return e ? atoi(e) : dflt;
        };
        Knobs v;
        const int t = env_int("PDSC_ATT_TARGET", 0), nw = env_int("PDSC_ATT_NW", 2), ws = env_int("PDSC_ATT_WS", 4),
                  sl = env_int("PDSC_ATT_TINY_SLOTS", 0), wpb = env_int("PDSC_SEED_WPB", 0);
        v.target = t > 0 ? t : 512;
        v.nw = (nw == 1 || nw == 2) ? nw : 4;
        v.tiny = env_int("PDSC_ATT_TINY", 16);
        v.tiny_slots = sl > 0 ? sl : 128;
        v.ws = (ws == 1 || ws == 2) ? ws : 4;
        v.w64 = env_int("PDSC_W64", 2);
        v.w64_sk = env_int("PDSC_W64_SK", 1) != 0;
        v.fuse = env_int("PDSC_FUSE", 1) != 0;
        v.precombine = env_int("PDSC_PRECOMBINE", 1) != 0;
        v.zigzag = env_int("PDSC_ZIGZAG", 1);
        v.dense_m = env_int("PDSC_DENSE_M", 0) == 1;
        v.vfold = env_int("PDSC_VFOLD", 1) != 0;
        v.pw2 = env_int("PDSC_PW2", 1);
        v.pw_small_limit = env_int("PDSC_PW_SMALL_LIMIT", 512);
        v.pw_waves8 = env_int("PDSC_PW_WAVES", 8) != 4;
        v.pw_qkv_split = env_int("PDSC_PW_QKV_SPLIT", 1) != 0;
        v.pw_prefetch = env_int("PDSC_PW_PREFETCH", 1) != 0;
        v.enc_halves = env_int("PDSC_ENC_HALVES", 2);
        v.enc_parts = std::min(std::max(env_int("PDSC_ENC_PARTS", 2), 2), ENC_MAX_PARTS);
        v.enc_bal = env_int("PDSC_ENC_BAL", 0) == 1;
        v.ragged_order = env_int("PDSC_RAGGED_ORDER", 1) != 0;
        v.seed_blocks = env_int("PDSC_SEED_BLOCKS", 1024);
        v.seed_sort = env_int("PDSC_SEED_SORT", 0) == 1;
        v.lm_rpt = env_int("PDSC_LM_RPT", 0);
        v.seed_select = env_int("PDSC_SEED_SELECT", 2);
        v.sel_split = env_int("PDSC_SEL_SPLIT", 1) != 0;
        v.seed_wpb = (wpb == 1 || wpb == 2 || wpb == 4) ? wpb : 0;
        v.knn_bitonic = env_int("PDSC_KNN_BITONIC", 1);
        v.kabsch_fused = env_int("PDSC_KABSCH_FUSED", 1) != 0;
        v.tail_fused = env_int("PDSC_TAIL_FUSED", 1) != 0;
        return v;
    }();
    return k;
}

// the register-chained pointwise kernels' workgroup (encoder.hip, pw2): PW2_W waves x 32 points
#ifndef PW2_WAVES
#define PW2_WAVES 4
#endif
constexpr int PW2_W = PW2_WAVES;
constexpr int PW2_PTS = PW2_W * 32;

enum AttnKind {
    ATT_FUSED,   // attn_pw2 / attn_pw2_last: the attention and the pointwise chain in one launch per layer
    ATT_F32,     // exact-fp32 split-K (attention.hpp)
    ATT_H3,      // split-K attention_h3_kernel<nw>
    ATT_H3_WS,   // the tiny plan's wave-split attention_h3_ws_kernel<ws>
    ATT_W64,     // attention_w64_kernel on the split grid
    ATT_W64_SK,  // attention_w64_sk_kernel: stream-K, sk_wgs workgroups
};

struct EncoderPlan {
    AttnKind kind;
    int B, N, Npad;
    bool f32;
    int nw;      // ATT_H3: waves (x 32 queries) per workgroup: 1, 2 or 4
    int ws;      // ATT_H3_WS: waves sharing one block of 32 queries and splitting each key split's tiles: 2 or 4
    bool early;  // ATT_H3: attention_h3_core's early-issue loop
    int sk_wgs;  // ATT_W64_SK: stream-K workgroups (one per CU); else 0
    int nqb;     // query blocks per pair of the launch grid
    int sps;     // key tiles (f32: stages) per split of the launch grid
    // Partial slots as the workspace sees them (opart, ml).  W64: the split grid's
    // or, if more, the stream-K segments'; slots past the split grid's own are
    // empty splits.  ATT_FUSED launches one key split and leaves the partials
    // unused: this is then still the h3 split plan's count, which carve_encoder
    // sizes opart by (workspace byte counts are ABI-visible).
    int nsplit;
    bool precombine;  // the split partials combined by combine_rows ahead of the pointwise kernels
    int m_layout;     // MLayout of the M this plan reads
    // fc_message[0] folded into the V projection: V' = (W0 Wv) x, a
    // 64-channel P.V, the message chain from fc0's BatchNorm / ReLU on.  True where
    // the pointwise chain is the register-chained one (the fused plan, and the
    // split plans from pw2's 320 workgroups on); attention_w64 then runs its
    // 128-channel P.V on V' padded with zero channels.  The LDS-tiled chains (small
    // batches) and the exact-fp32 mode keep V and fc0.
    bool vfold;
    // The pointwise chain (launch_pw_first / _mid / _last): the register-chained
    // pw2_* kernels (the fused plan's pw2_first among them), else the LDS-tiled
    // pw_* ones, whose form the fields below hold (all 0 under pw2).
    bool pw2;
    int pw_tile;         // points per workgroup: 32 or 64
    bool pw_mid8;        // pw_mid on 8 waves (32-point tiles)
    bool pw_first_qkv3;  // pw_first's Q / K / V in three workgroups per point tile
    bool pw_mid_qkv3;    // the 8-wave pw_mid's likewise
    bool pw_prefetch;    // the 8-wave pw_mid's panel prefetch

    bool fused() const { return kind == ATT_FUSED; }
    bool w64() const { return kind == ATT_W64 || kind == ATT_W64_SK; }

    // A ragged batch whose counts are not all the padded N takes the split grid in
    // place of stream-K (which shares key TILES evenly, so needs pairs of equal
    // length) and keeps the slots.  A ragged batch with rg.eq keeps stream-K: such
    // a call is bitwise the uniform entry's.
    EncoderPlan for_ragged(const Ragged &rg) const {
        EncoderPlan p = *this;
        if (kind == ATT_W64_SK && rg.nv && !rg.eq) {
            p.kind = ATT_W64;
            p.sk_wgs = 0;
        }
        return p;
    }
    // The batch's plan on a contiguous part of its pairs (run_encoder_part): the
    // same kernels, pointwise chain and per-pair grid, whatever plan nb pairs alone would get.
    EncoderPlan for_pairs(int nb) const {
        EncoderPlan p = *this;
        p.B = nb;
        return p;
    }

    // The attention's workgroup order, reversed on alternate layers (fused and
    // split-K launches; the stream-K form excepted): a launch starts on the pairs
    // whose M (and featL) the previous one read last, while they may still sit in
    // the Infinity Cache.  Ragged batches keep their longest-first order.
    int rev(const Ragged &rg, int layer) const {
        const int mode = knobs().zigzag;
        if (rg.po || kind == ATT_W64_SK) return 0;
        return mode == 0 ? 0 : mode == 2 ? !(layer & 1) : (layer & 1);
    }
    int workgroups() const { return kind == ATT_W64_SK ? sk_wgs : B * nqb * (fused() ? 1 : nsplit); }
};

// The plan of B pairs of N correspondences.
// dense_m_caller: the caller brings its own dense M (pdsc_encoder_f32,
// pdsc_attention_f32): the plan reads M dense and never runs attention_w64
// (symmetric-packed M only).
// allow_fused = false: the split launch alone (pdsc_attention_f32).
EncoderPlan plan_encoder(int B, int N, bool f32, bool dense_m_caller, bool allow_fused = true);

// The tail's launches (NMS and seed ranking, seed kNN, NSM, hypotheses) for B
// pairs of N correspondences and S seeds each: what launch_local_max,
// launch_seed_rank, launch_knn_select, launch_nsm_seed and launch_hypotheses run.
enum SeedRank {
    RANK_COMPARE,       // seed_rank_kernel<seed_rows>
    RANK_SORT,          // seed_rank_sort_kernel
    RANK_SELECT,        // seed_select_kernel<false>
    RANK_SELECT_SPLIT,  // seed_select_kernel<true> + seed_cand_rank_kernel where the caller gives scratch, else RANK_SELECT
};
struct TailPlan {
    int seed_rows;      // rows per block of the NMS and seed-ranking compare kernels: 16 or 64
    int nms_rpt;        // the NMS compare's rows per thread: 1, 2 or 4; 0: local_max_sort_kernel
    SeedRank rank;
    int wpb;            // waves (= seeds) per workgroup of knn_select, nsm_seed and kabsch_sums: 1, 2 or 4
    int knn_bitonic;    // knn_select_kernel's ranking argument
    bool kabsch_fused;  // the Kabsch solve and the inlier count inside kabsch_sums_kernel
    bool tail_fused;    // the testing forward: nsm_finish inside the hypotheses' first launch, select_best + post_refine in one
};
TailPlan plan_tail(int B, int N, int S);

}  // namespace pdsc
