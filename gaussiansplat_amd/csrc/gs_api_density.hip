// gs_api_density.hip -- density control below the C ABI: gs_density_accumulate / _decide / _plan / _restructure and gs_opacity_reset
// (3-D renderer; the kernels are in gs_density.hip, the semantics in include/gsplat.h and DESIGN.md 5.8b).  Every refusal happens before
// anything is enqueued.  gs_density_plan holds the one synchronise: the host needs the class totals to size the new arrays.  The plan it
// leaves (offsets per chunk in ctx scratch, totals here) is tagged with the action array and n, and dropped by gs_ctx::inputs_changed().
#include "gs_ctx.h"
#include "gs_density.h"


extern "C" {

int gs_density_accumulate(gs_ctx *c, const gs_density_stats *st) {
    if (!c) return GS_ERR_INVALID;
    if (!st) return fail(c, GS_ERR_INVALID, "gs_density_accumulate: NULL stats");
    if (const int rc = need_3d(c, "gs_density_accumulate")) return rc;
    if (const int rc = need_stage(c, gs_ctx::Stage::COMPOSITE_ADJOINT, "gs_density_accumulate: gs_backward first (a non-fused backward of the frame)")) return rc;
    if (c->n > 0 && (!st->grad_sum || !st->count || !st->max_extent)) return fail(c, GS_ERR_INVALID, "gs_density_accumulate: NULL statistics array");
    if (bind_device(c)) return GS_ERR_HIP;
    GsDensityAccArgs a{};
    a.n = c->n;
    a.payload = c->payload.as<GsPayload>(); a.invcov = c->invcov.as<float>();
    c->rows(c->g2d).into(a);
    a.half_w = 0.5f * (float)c->cam.W; a.half_h = 0.5f * (float)c->cam.H;
    a.grad_sum = st->grad_sum; a.count = st->count; a.max_extent = st->max_extent;
    HIPCHK(c, gs_launch_density_accumulate(a, c->stream));
    return GS_OK;
}

int gs_density_decide(gs_ctx *c, const gs_density_stats *st, const gs_density_params *p, int32_t *action) {
    if (!c) return GS_ERR_INVALID;
    if (!st || !p) return fail(c, GS_ERR_INVALID, "gs_density_decide: NULL argument");
    if (const int rc = need_3d(c, "gs_density_decide")) return rc;
    if (p->struct_size != (int32_t)sizeof(gs_density_params)) return fail(c, GS_ERR_INVALID, "gs_density_decide: gs_density_params.struct_size mismatch");
    if (std::isnan(p->grad_threshold) || std::isnan(p->log_shrink)) return fail(c, GS_ERR_INVALID, "gs_density_decide: grad_threshold and log_shrink must not be NaN");
    if (c->n > 0 && (!st->grad_sum || !st->count || !st->max_extent || !action)) return fail(c, GS_ERR_INVALID, "gs_density_decide: NULL array");
    if (bind_device(c)) return GS_ERR_HIP;
    GsDensityDecideArgs a{};
    a.n = c->n; a.scales = c->scales; a.opac = c->opac;
    a.grad_sum = st->grad_sum; a.count = st->count; a.max_extent = st->max_extent;
    a.grad_threshold = p->grad_threshold; a.log_split_scale = p->log_split_scale; a.log_shrink = p->log_shrink;
    a.min_opacity_logit = p->min_opacity_logit; a.log_max_world_scale = p->log_max_world_scale; a.max_extent_px = p->max_extent_px;
    a.action = action;
    HIPCHK(c, gs_launch_density_decide(a, c->stream));
    c->density_log_shrink = p->log_shrink;                                 // what the children of these split actions shrink by
    return GS_OK;
}

int gs_density_plan(gs_ctx *c, const int32_t *action, int64_t counts[4]) {
    if (!c) return GS_ERR_INVALID;
    if (!counts) return fail(c, GS_ERR_INVALID, "gs_density_plan: NULL counts");
    if (const int rc = need_3d(c, "gs_density_plan")) return rc;
    if (c->n > 0 && !action) return fail(c, GS_ERR_INVALID, "gs_density_plan: NULL action");
    if (bind_device(c)) return GS_ERR_HIP;
    c->density.planned = false;
    const size_t cells = (size_t)GS_DENSITY_CLASSES * (size_t)std::max<int64_t>(gs_chunks(c->n), 1);
    HIPCHK(c, c->density_cnt.ensure(sizeof(uint32_t) * cells));
    HIPCHK(c, c->density_off.ensure(sizeof(int64_t) * cells));
    HIPCHK(c, c->density_tot.ensure(sizeof(int64_t) * 4));
    HIPCHK(c, gs_launch_density_plan(action, c->n, c->density_cnt.as<uint32_t>(), c->density_off.as<int64_t>(), c->density_tot.as<int64_t>(), c->stream));
    int64_t tot[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(tot, c->density_tot.p, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tot[3]) return fail(c, GS_ERR_INVALID, "gs_density_plan: an action outside 0..3");
    if (tot[0] < 0 || tot[1] < 0 || tot[2] < 0 || tot[1] > tot[0] || tot[0] + tot[2] > c->n) return fail(c, GS_ERR_HIP, "gs_density_plan: inconsistent class totals");
    gs_ctx::DensityPlan &d = c->density;
    d.action = action; d.n = c->n; d.survivors = tot[0]; d.clones = tot[1]; d.splits = tot[2];
    d.planned = true;
    counts[0] = tot[0]; counts[1] = tot[1]; counts[2] = tot[2]; counts[3] = c->n - tot[0] - tot[2];
    return GS_OK;
}

int gs_density_restructure(gs_ctx *c, const int32_t *action, const float *noise, const gs_grads *dst_model, int32_t nsets,
                           const gs_grads *src_sets, const gs_grads *dst_sets, int64_t n_out) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_density_restructure")) return rc;
    const gs_ctx::DensityPlan &d = c->density;
    if (!d.planned || d.action != action || d.n != c->n)
        return fail(c, GS_ERR_INVALID, "gs_density_restructure: no plan for this action array and model (gs_density_plan first; a model or camera change drops it)");
    if (n_out != d.n_out()) return fail(c, GS_ERR_INVALID, "gs_density_restructure: n_out differs from the plan's");
    if (nsets < 0 || nsets > GS_DENSITY_MAX_SETS) return fail(c, GS_ERR_INVALID, "gs_density_restructure: nsets must be 0..4");
    if (nsets > 0 && (!src_sets || !dst_sets)) return fail(c, GS_ERR_INVALID, "gs_density_restructure: NULL companion sets");
    if (!dst_model) return fail(c, GS_ERR_INVALID, "gs_density_restructure: NULL dst_model");
    if (d.splits > 0 && !noise) return fail(c, GS_ERR_INVALID, "gs_density_restructure: the plan has splits: noise must not be NULL");
    const size_t n = (size_t)c->n, no = (size_t)n_out;
    GsDensityRestructureArgs a{};
    const Five<const float> src = c->model5();
    const Five<float> dst = five(*dst_model);
    // every destination against the model, the source sets and the other destinations (gs_adam_prepare's rule)
    ByteRange rd[5 + 5 * GS_DENSITY_MAX_SETS], rs[5 + 5 * GS_DENSITY_MAX_SETS];
    int nd = 0, ns = 0;
    for (int i = 0; i < 5; ++i) {
        if (no && !dst[i]) return fail(c, GS_ERR_INVALID, "gs_density_restructure: NULL array in dst_model");
        if (n && !src[i]) return fail(c, GS_ERR_INVALID, "gs_density_restructure: no model (gs_set_model first)");
        a.src[i] = src[i]; a.dst[i] = dst[i];
        rd[nd++] = {dst[i], sizeof(float) * c->width[i] * no};
        rs[ns++] = {src[i], sizeof(float) * c->width[i] * n};
    }
    for (int t = 0; t < nsets; ++t) {
        const Five<float> ss = five(src_sets[t]), sd = five(dst_sets[t]);
        for (int i = 0; i < 5; ++i) {
            if (!ss[i] || !sd[i]) continue;                                // skipped (the kernel tests the same pair)
            a.set_src[t][i] = ss[i]; a.set_dst[t][i] = sd[i];
            rd[nd++] = {sd[i], sizeof(float) * c->width[i] * no};
            rs[ns++] = {ss[i], sizeof(float) * c->width[i] * n};
        }
    }
    for (int i = 0; i < nd; ++i) {
        for (int j = 0; j < ns; ++j)
            if (overlaps(rd[i], rs[j])) return fail(c, GS_ERR_INVALID, "gs_density_restructure: a destination overlaps the model or a source set");
        for (int j = i + 1; j < nd; ++j)
            if (overlaps(rd[i], rd[j])) return fail(c, GS_ERR_INVALID, "gs_density_restructure: destinations overlap");
    }
    if (bind_device(c)) return GS_ERR_HIP;
    if (!n || !no) return GS_OK;                                           // nothing to read, or nothing to write (every gaussian pruned)
    a.n = c->n; a.k3 = (int)c->width[4];
    a.action = action; a.noise = noise; a.chunk_off = c->density_off.as<int64_t>();
    a.survivors = d.survivors; a.clones = d.clones; a.splits = d.splits;
    a.log_shrink = c->density_log_shrink;
    a.nsets = nsets;
    HIPCHK(c, gs_launch_density_restructure(a, c->stream));
    return GS_OK;
}

int gs_opacity_reset(gs_ctx *c, float max_logit, float *m_opac, float *v_opac) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_opacity_reset")) return rc;
    if (c->n > 0 && !c->opac) return fail(c, GS_ERR_INVALID, "gs_opacity_reset: no model (gs_set_model first)");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_opacity_reset(const_cast<float *>(c->opac), max_logit, m_opac, v_opac, c->n, c->stream));
    c->inputs_changed();
    return GS_OK;
}

}  // extern "C"
