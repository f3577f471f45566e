// attention_plan.hpp -- which attention kernel the encoder runs at a shape, and
// with which grid.  Host-only: plan_encoder (encoder.hip, beside the kernels'
// grid helpers it calls) decides it once per call from (B, N, precision) and the
// process's knobs; api.hip sizes the workspace by the plan and encoder.hip's
// launchers launch what it says.
#pragma once
#include <cstdlib>

#include "pdsc_internal.hpp"

namespace pdsc {

inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// The attention and encoder-plan knobs (A/B measurement only), read once per process.
struct AttnKnobs {
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
    int pw2;         // PDSC_PW2: 0 never, 2 always, else the 320-workgroup rule
    bool precombine; // PDSC_PRECOMBINE=0: never
    int zigzag;      // PDSC_ZIGZAG: 0 off, 2 inverted
    bool dense_m;    // PDSC_DENSE_M=1: the forward writes and reads M dense
    bool vfold;      // PDSC_VFOLD=0: no plan folds fc_message[0] into V (EncoderPlan::vfold)
};
inline const AttnKnobs &attn_knobs() {
    static const AttnKnobs k = [] {
        AttnKnobs v;
        const int t = env_int("PDSC_ATT_TARGET", 0), nw = env_int("PDSC_ATT_NW", 2), ws = env_int("PDSC_ATT_WS", 4),
                  sl = env_int("PDSC_ATT_TINY_SLOTS", 0);
        v.target = t > 0 ? t : 512;
        v.nw = (nw == 1 || nw == 2) ? nw : 4;
        v.tiny = env_int("PDSC_ATT_TINY", 16);
        v.tiny_slots = sl > 0 ? sl : 128;
        v.ws = (ws == 1 || ws == 2) ? ws : 4;
        v.w64 = env_int("PDSC_W64", 2);
        v.w64_sk = env_int("PDSC_W64_SK", 1) != 0;
        v.fuse = env_int("PDSC_FUSE", 1) != 0;
        v.pw2 = env_int("PDSC_PW2", 1);
        v.precombine = env_int("PDSC_PRECOMBINE", 1) != 0;
        v.zigzag = env_int("PDSC_ZIGZAG", 1);
        v.dense_m = env_int("PDSC_DENSE_M", 0) == 1;
        v.vfold = env_int("PDSC_VFOLD", 1) != 0;
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

// pw2 for launches of at least 320 128-point workgroups, 1.25 per CU.  Measured
// encoder ms, pw2 vs pw_mid chains: 8 x N=5000 (320 WGs; 3 key splits) 4.48
// vs 4.61; 40 x 1000 (320, fused) 1.47 vs 1.78; 56 x 1000 (448, fused) 1.68 vs
// 2.12; 32 x 1000 (256) 1.26 vs 1.22 and 1.24 fused; 16 x 1000 (128) 0.95 vs 0.80.
inline bool use_pw2(int B, int Npad, bool f32) {
    const int mode = attn_knobs().pw2;
    if (f32 || mode == 0) return false;
    return mode == 2 || (long)B * ((Npad + PW2_PTS - 1) / PW2_PTS) >= 320;
}

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
    // split plans from use_pw2's 320 workgroups on); attention_w64 then runs its
    // 128-channel P.V on V' padded with zero channels.  The LDS-tiled chains (small
    // batches) and the exact-fp32 mode keep V and fc0.
    bool vfold;

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
    // same kernel and per-pair grid, whatever plan nb pairs alone would get.
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
        const int mode = attn_knobs().zigzag;
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

}  // namespace pdsc
