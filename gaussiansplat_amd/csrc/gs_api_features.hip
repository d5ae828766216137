// gs_api_features.hip -- feature maps: a finished frame's composite forward and backward run over a SECOND payload whose three colour
// floats are the caller's (depth, opacity, any per-gaussian triple), and the view-space depth with its adjoint.
// The composite kernels do not know that the three floats they composite are colours (GsPayload::r, g, b), so nothing in gs_composite.hip
// changes: the launches below are the frame's own, from composite_args(debug = true) -- "an isolated launch over the finished frame, as
// the frame's plan ran it": no per-tile counters, no snapshots -- pointed at buffers that are not the frame's.  What the frame owns stays
// what gs_forward left: image, transmittance, work counters, the view slot's history, launch orders, snapshots, g2d and g2d_clean, dpc, the
// stage.  Every refusal is made before anything is enqueued or allocated.
#include "gs_ctx.h"
#include "gs_features.h"

using Stage = gs_ctx::Stage;

// what the two frame calls share: the 3-D renderer, a frame that has its image, lists of one round
static int feature_frame_ok(gs_ctx *c, const char *who) {
    if (const int rc = need_3d(c, who)) return rc;
    if (c->stage < Stage::RENDERED) return fail(c, GS_ERR_INVALID, std::string(who) + ": gs_forward first");
    if (c->bin.n_rounds > 1)
        return fail(c, GS_ERR_UNSUPPORTED, std::string(who) + ": this frame was binned in depth slabs (lists spread over rounds); use gs_config.slab_mode = 0");
    return GS_OK;
}

// the feature payload: the frame's rows with r, g, b = feat
static int build_feature_payload(gs_ctx *c, const float *feat) {
    HIPCHK(c, c->feat_payload.ensure(sizeof(GsPayload) * c->n1()));
    HIPCHK(c, gs_launch_feature_payload(c->payload.as<GsPayload>(), feat, c->n, c->feat_payload.as<GsPayload>(), c->stream));
    return GS_OK;
}

extern "C" {

int gs_view_depth(gs_ctx *c, float *z) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_view_depth")) return rc;
    if (!z) return fail(c, GS_ERR_INVALID, "gs_view_depth: NULL argument");
    if (!c->have_cam || (c->n > 0 && !c->means)) return fail(c, GS_ERR_INVALID, "gs_view_depth: gs_set_model and gs_set_camera first");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_view_depth(c->means, c->n, c->cam, z, c->stream));
    return GS_OK;
}

int gs_view_depth_backward(gs_ctx *c, const float *dz, float *d_means) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_view_depth_backward")) return rc;
    if (!dz || !d_means) return fail(c, GS_ERR_INVALID, "gs_view_depth_backward: NULL argument");
    if (!c->have_cam) return fail(c, GS_ERR_INVALID, "gs_view_depth_backward: gs_set_camera first");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_view_depth_bwd(dz, c->n, c->cam, d_means, c->stream));
    return GS_OK;
}

int gs_render_features(gs_ctx *c, const float *feat, float *out, float *trans_out) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = feature_frame_ok(c, "gs_render_features")) return rc;
    if (!feat || !out) return fail(c, GS_ERR_INVALID, "gs_render_features: NULL argument");
    const size_t px = c->pixels(), fb = sizeof(float);
    const ByteRange o{out, 3 * px * fb}, t{trans_out, px * fb}, image{c->img(), 3 * px * fb}, trans{c->tr(), px * fb};
    if (overlaps(o, image) || overlaps(o, trans) || overlaps(t, image) || overlaps(t, trans) || overlaps(o, t))
        return fail(c, GS_ERR_INVALID, "gs_render_features: out / trans_out overlap the frame's image or transmittance, or each other");
    if (bind_device(c)) return GS_ERR_HIP;
    if (!trans_out) HIPCHK(c, c->feat_trans.ensure(fb * (px ? px : 1)));
    if (const int rc = build_feature_payload(c, feat)) return rc;
    // the frame's forward over the finished frame: its lists (capped ones as far as the frame's forward left them: tile_ext -- the same walk
    // never reaches their written end with a pixel still taking entries), its order, its waves per tile, its early-out and no-op rules
    GsCompositeArgs a = composite_args(c, false, 0, true);
    a.payload = c->feat_payload.as<GsPayload>();
    a.image = out;
    a.trans = trans_out ? trans_out : c->feat_trans.as<float>();
    a.final_round = 1;                                                     // the transmittance is written plain
    HIPCHK(c, gs_launch_composite_fwd(a, c->stream));                      // no background: out = sum feat alpha T
    return GS_OK;
}

int gs_backward_features(gs_ctx *c, const float *feat, const float *image_f, const float *dF, float *d_feat, const gs_grads *grads) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = feature_frame_ok(c, "gs_backward_features")) return rc;
    if (!feat || !image_f || !dF || !d_feat) return fail(c, GS_ERR_INVALID, "gs_backward_features: NULL argument");
    if (bind_device(c)) return GS_ERR_HIP;
    // auxiliary rows of 2-D gradient sums, of the frame's mode, zeroed: c->g2d is the colour backward's
    HIPCHK(c, c->feat_g2d.ensure(c->g2d_bytes()));
    const bool chain = grads && (grads->d_means || grads->d_scales || grads->d_quats || grads->d_opacities);
    if (chain) {
        // the geometry chain's colour-path input: zeros that nothing writes again (not c->dpc: a caller may stand between GS_BWD_PARAMS_SH and _GEOM)
        HIPCHK(c, c->feat_dpc.ensure(sizeof(float) * 4 * c->n1()));
        if (c->feat_dpc_zeroed != c->feat_dpc.cap) {
            HIPCHK(c, hipMemsetAsync(c->feat_dpc.p, 0, c->feat_dpc.cap, c->stream));
            c->feat_dpc_zeroed = c->feat_dpc.cap;
        }
    }
    if (const int rc = build_feature_payload(c, feat)) return rc;
    HIPCHK(c, hipMemsetAsync(c->feat_g2d.p, 0, c->g2d_bytes(), c->stream));
    // The composite backward over WHOLE tiles (the by-tile form of gs_debug_tile_clock): no snapshots, no list segments, no split entries,
    // no tail fill, no per-tile counters.  The snapshots the frame holds are of the COLOUR image: a segment would start from the wrong S.
    GsCompositeArgs a = composite_args(c, true, 0, true);
    a.split_ok = 0; a.snap = nullptr; a.seg_hist = nullptr; a.seg_n = 0; a.seg_len = nullptr; a.snap_walked = nullptr; a.front = 0;
    a.payload = c->feat_payload.as<GsPayload>();
    a.image = const_cast<float *>(image_f);                                // (read only by the backward: S = image . dC)
    a.trans = c->tr();
    a.dC = dF;
    c->rows_mut(c->feat_g2d).into(a);
    HIPCHK(c, gs_launch_composite_bwd(a, c->stream));
    const gs_ctx::Rows rows = c->rows(c->feat_g2d);
    HIPCHK(c, gs_launch_pack_drgb(rows.g2d, rows.g2d_fixed, d_feat, c->n, c->stream));
    if (chain) {
        // the alpha path alone: the moments of the auxiliary rows through the geometry chain, accumulated into the caller's arrays
        const GsPreprocessBwdArgs b = chain_args(c, rows, c->feat_dpc.as<float>(), {{grads->d_means, grads->d_scales, grads->d_quats, grads->d_opacities, nullptr}}, 0, 0, 0.0f);
        const GsPreprocessBwdMode mode{2, nullptr, 0};
        HIPCHK(c, gs_launch_preprocess_bwd(b, c->cam, c->stream, mode));
    }
    return GS_OK;
}

}  // extern "C"
