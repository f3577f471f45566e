// encoder.hpp -- what the forwards (api.hip) take from the encoder row
// (encoder.hip): the row's workspace and its run loop.  Host only.
#pragma once
#include "launch_plan.hpp"
#include "workspace.hpp"

namespace pdsc {

struct EncBufs {
    float *feat, *opart, *ml, *vexp, *vexp2;
    float *feat2;            // the split path's second feat buffer (pw_mid reads one, writes the other), else null
    _Float16 *q, *k, *v;     // attention_h3 split layouts (hi + lo per element), or fp32 rows (F32)
    _Float16 *q2, *k2, *v2;  // the other Q/K/V set of the fused path (layers alternate), else null
    float *opart1, *ml1;     // the combined split (EncoderPlan::precombine), else null
};
EncBufs carve_encoder(Carve &c, const EncoderPlan &plan);

// The encoder's parts on side streams (encoder.hip has the measurements): whether
// a batch of this plan runs as parts, the device's side streams, the part boundaries.
struct SideStream;
bool enc_halves(const EncoderPlan &plan, bool ragged);
SideStream *side_stream(hipStream_t s);
void enc_bounds(const int32_t *counts, int B, int P, int *bounds);

// a2-a4 of plan.B pairs on stream s; M in the plan's layout (plan.m_layout).
// ss != NULL: the fused plan as P concurrent parts at `bounds` (rg.po, when set,
// must then order each part's pairs on its own: launch_ragged_order per part).
int run_encoder_fwd(const PackLayout &lay, const float *packed, const float *corr_pos, const float *M,
                    const EncoderPlan &plan, const EncBufs &e, float *normed, _Float16 *normed_s, float *conf,
                    hipStream_t s, Ragged rg = {}, SideStream *ss = nullptr, const int *bounds = nullptr, int P = 1);

}  // namespace pdsc
