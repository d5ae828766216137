// gs_density.h -- density control on the device (gs_density.hip) as its host side sees it (gs_api_density.hip): statistics of the
// screen-space positional gradient, the clone / split / prune decision, the ordered restructuring of the model and of gradient-shaped
// companion arrays (Adam's moments), and the opacity reset.  Semantics: include/gsplat.h, DESIGN.md 5.8b.
#pragma once
#include "gs_chunk.h"
#include "gs_common.h"

#define GS_DENSITY_CLASSES 3         // output classes a source row feeds: survivors (actions 0, 1), clones (1), split sources (2)
#define GS_DENSITY_MAX_SETS 4        // gradient-shaped companion sets a restructure carries along

struct GsDensityAccArgs {
    int64_t n;
    const GsPayload *payload;        // the view's rows: sig and the packed pixel box
    const float *invcov;             // 4 x n raw conic
    const float *g2d;                // the composite backward's sums (float mode) ...
    const long long *g2d_fixed;      // ... or their fixed-point form (deterministic mode); exactly one is set
    float half_w, half_h;            // 0.5f * W, 0.5f * H: pixels -> NDC units
    float *grad_sum;
    int32_t *count, *max_extent;
};
hipError_t gs_launch_density_accumulate(const GsDensityAccArgs &a, hipStream_t s);

struct GsDensityDecideArgs {
    int64_t n;
    const float *scales, *opac;      // 3 x n (log), n (logit)
    const float *grad_sum;
    const int32_t *count, *max_extent;
    float grad_threshold, log_split_scale, log_shrink, min_opacity_logit, log_max_world_scale;
    int32_t max_extent_px;
    int32_t *action;
};
hipError_t gs_launch_density_decide(const GsDensityDecideArgs &a, hipStream_t s);

// The plan and the restructure run one workgroup per chunk of GS_CHUNK gaussians (gs_chunk.h).  chunk_cnt: [GS_DENSITY_CLASSES][gs_chunks(n)]
// counts; chunk_off: the same shape, exclusive offsets inside each class; totals: four words
// {survivors, clones, split sources, != 0: an action outside 0..3 was seen}.  Enqueues the zeroing of `totals` as well.
hipError_t gs_launch_density_plan(const int32_t *action, int64_t n, uint32_t *chunk_cnt, int64_t *chunk_off, int64_t *totals, hipStream_t s);

struct GsDensityRestructureArgs {
    int64_t n;
    int k3;                          // floats of an SH row
    const int32_t *action;
    const float *noise;              // [n][2][3]; may be null when splits == 0
    const int64_t *chunk_off;        // [GS_DENSITY_CLASSES][chunks]
    int64_t survivors, clones, splits;   // the plan's totals: rows are written only inside them, whatever `action` says by now
    float log_shrink;
    const float *src[5];             // the model
    float *dst[5];
    int nsets;
    const float *set_src[GS_DENSITY_MAX_SETS][5];   // a pair with a null array on either side is skipped: the caller leaves BOTH null
    float *set_dst[GS_DENSITY_MAX_SETS][5];         // (gs_api_density.hip does; the +0 rows of clones and children test set_dst alone)
};
hipError_t gs_launch_density_restructure(const GsDensityRestructureArgs &a, hipStream_t s);

hipError_t gs_launch_opacity_reset(float *opac, float max_logit, float *m_opac, float *v_opac, int64_t n, hipStream_t s);
