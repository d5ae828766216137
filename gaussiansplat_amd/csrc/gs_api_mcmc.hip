// gs_api_mcmc.hip -- MCMC densification below the C ABI: gs_mcmc_plan / _sample / _relocate / _noise / _regularize (3-D renderer; the kernels
// are in gs_mcmc.hip, the statements in gs_mcmc.h, the semantics in include/gsplat.h and DESIGN.md 5.8l).  Every refusal happens before anything
// is enqueued.  gs_mcmc_plan holds the one synchronise: the host needs the dead count to draw that many numbers.  The plan it leaves (the caller's
// dead list, n, the count) is dropped by gs_ctx::inputs_changed(), which gs_mcmc_noise and gs_mcmc_relocate call like every step of the model.
#include "gs_ctx.h"
#include "gs_mcmc.h"

typedef unsigned long long u64;

extern "C" {

int gs_mcmc_plan(gs_ctx *c, float min_opacity_logit, uint64_t *cdf, int32_t *dead, int64_t counts[3]) {
    if (!c) return GS_ERR_INVALID;
    if (!counts) return fail(c, GS_ERR_INVALID, "gs_mcmc_plan: NULL counts");
    if (const int rc = need_3d(c, "gs_mcmc_plan")) return rc;
    if (std::isnan(min_opacity_logit)) return fail(c, GS_ERR_INVALID, "gs_mcmc_plan: min_opacity_logit must not be NaN");
    if (const int rc = need_model(c, "gs_mcmc_plan")) return rc;
    if (c->n > 0 && (!cdf || !dead)) return fail(c, GS_ERR_INVALID, "gs_mcmc_plan: NULL array");
    if (c->n > 0x7fffffffLL) return fail(c, GS_ERR_UNSUPPORTED, "gs_mcmc_plan: more than 2^31 - 1 gaussians");
    if (bind_device(c)) return GS_ERR_HIP;
    c->mcmc.planned = false;
    const size_t cells = 2 * (size_t)std::max<int64_t>(gs_chunks(c->n), 1);
    HIPCHK(c, c->mcmc_sum.ensure(sizeof(u64) * cells));
    HIPCHK(c, c->mcmc_off.ensure(sizeof(u64) * cells));
    HIPCHK(c, c->mcmc_tot.ensure(sizeof(u64) * 2));
    HIPCHK(c, gs_launch_mcmc_plan(c->opac, c->n, min_opacity_logit, c->mcmc_sum.as<u64>(), c->mcmc_off.as<u64>(), c->mcmc_tot.as<u64>(),
                                  reinterpret_cast<u64 *>(cdf), dead, c->stream));
    u64 tot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(tot, c->mcmc_tot.p, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tot[1] > (u64)c->n || tot[0] > ((u64)c->n << 24)) return fail(c, GS_ERR_HIP, "gs_mcmc_plan: inconsistent totals");
    gs_ctx::McmcPlan &p = c->mcmc;
    p.dead = dead; p.n = c->n; p.dead_count = (int64_t)tot[1];
    p.planned = true;
    counts[0] = c->n - (int64_t)tot[1]; counts[1] = (int64_t)tot[1]; counts[2] = (int64_t)tot[0];
    return GS_OK;
}

int gs_mcmc_sample(gs_ctx *c, const uint64_t *cdf, int64_t n, const float *u, int64_t m, int32_t *src) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_mcmc_sample")) return rc;
    if (n < 0 || m < 0 || n > 0x7fffffffLL) return fail(c, GS_ERR_INVALID, "gs_mcmc_sample: n must be in 0..2^31 - 1 and m >= 0");
    if (m == 0) return GS_OK;
    if (n == 0) return GS_OK;                                              // no CDF, no total: nothing is written
    if (!cdf || !u || !src) return fail(c, GS_ERR_INVALID, "gs_mcmc_sample: NULL array");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_mcmc_sample(reinterpret_cast<const u64 *>(cdf), n, u, m, src, c->stream));
    return GS_OK;
}

int gs_mcmc_relocate(gs_ctx *c, const int32_t *src, const int32_t *dst, int64_t m, float min_opacity, int32_t nsets, const gs_grads *sets) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_mcmc_relocate")) return rc;
    if (m < 0) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: m must be >= 0");
    if (!(min_opacity > 0.0f && min_opacity < 1.0f)) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: min_opacity must lie in (0, 1)");
    if (nsets < 0 || nsets > GS_DENSITY_MAX_SETS) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: nsets must be 0..4");
    if (nsets > 0 && !sets) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: NULL companion sets");
    if (m > 0 && !src) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: NULL src");
    if (!dst) {
        const gs_ctx::McmcPlan &p = c->mcmc;
        if (!p.planned || p.n != c->n)
            return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: dst is NULL and there is no plan for this model (gs_mcmc_plan first; a model change, a step or noise drop it)");
        if (m > p.dead_count) return fail(c, GS_ERR_INVALID, "gs_mcmc_relocate: m exceeds the plan's dead count");
        dst = p.dead;
    }
    if (const int rc = need_model(c, "gs_mcmc_relocate")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    if (m == 0 || c->n == 0) return GS_OK;                                 // nothing changes: the frame and the plan stand
    if (!c->mcmc_binom_ready) {
        static double table[GS_MCMC_BINOM];                                // the same values every time: a second ctx filling it again writes the same bits
        gs_mcmc_binom_fill(table);
        HIPCHK(c, c->mcmc_binom.ensure(sizeof(table)));
        HIPCHK(c, hipMemcpyAsync(c->mcmc_binom.p, table, sizeof(table), hipMemcpyHostToDevice, c->stream));
        c->mcmc_binom_ready = true;
    }
    HIPCHK(c, c->mcmc_hist.ensure(sizeof(int32_t) * c->n1()));
    GsMcmcRelocateArgs a{};
    a.n = c->n; a.m = m; a.k3 = (int)c->width[4];
    a.src = src; a.dst = dst; a.hist = c->mcmc_hist.as<int32_t>(); a.binom = c->mcmc_binom.as<double>();
    a.min_opacity = min_opacity;
    const Five<float> model = c->model5_mut();
    for (int i = 0; i < 5; ++i) a.model[i] = model[i];
    a.nsets = nsets;
    for (int t = 0; t < nsets; ++t) {
        const Five<float> s = five(sets[t]);
        for (int i = 0; i < 5; ++i) a.set[t][i] = s[i];
    }
    HIPCHK(c, gs_launch_mcmc_relocate(a, c->stream));
    c->inputs_changed();
    return GS_OK;
}

int gs_mcmc_noise(gs_ctx *c, const float *z, float lr, float gate_k, float gate_t) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_mcmc_noise")) return rc;
    if (!std::isfinite(lr) || !std::isfinite(gate_k) || !std::isfinite(gate_t)) return fail(c, GS_ERR_INVALID, "gs_mcmc_noise: lr, gate_k and gate_t must be finite");
    if (lr < 0.0f) return fail(c, GS_ERR_INVALID, "gs_mcmc_noise: lr must be >= 0");
    if (lr == 0.0f) return GS_OK;
    if (const int rc = need_model(c, "gs_mcmc_noise")) return rc;
    if (c->n > 0 && !z) return fail(c, GS_ERR_INVALID, "gs_mcmc_noise: NULL z");
    const size_t n = (size_t)c->n;
    const Five<const float> model = c->model5();
    for (int i = 0; i < 5; ++i)
        if (overlaps({z, sizeof(float) * 3 * n}, {model[i], sizeof(float) * c->width[i] * n})) return fail(c, GS_ERR_INVALID, "gs_mcmc_noise: z overlaps the model");
    if (bind_device(c)) return GS_ERR_HIP;
    if (c->n == 0) return GS_OK;
    HIPCHK(c, gs_launch_mcmc_noise(const_cast<float *>(c->means), c->scales, c->quats, c->opac, z, c->n, lr, gate_k, gate_t, c->stream));
    c->inputs_changed();
    return GS_OK;
}

int gs_mcmc_regularize(gs_ctx *c, const gs_grads *grads, float c_opacity, float c_scale) {
    if (!c) return GS_ERR_INVALID;
    if (!grads) return fail(c, GS_ERR_INVALID, "gs_mcmc_regularize: NULL grads");
    if (const int rc = need_3d(c, "gs_mcmc_regularize")) return rc;
    if (!std::isfinite(c_opacity) || !std::isfinite(c_scale)) return fail(c, GS_ERR_INVALID, "gs_mcmc_regularize: the coefficients must be finite");
    if (const int rc = need_model(c, "gs_mcmc_regularize")) return rc;
    float *d_opac = c_opacity != 0.0f ? grads->d_opacities : nullptr;
    float *d_scales = c_scale != 0.0f ? grads->d_scales : nullptr;
    const size_t n = (size_t)c->n;
    const Five<const float> model = c->model5();
    for (int i = 0; i < 5; ++i)
        if (overlaps({d_opac, sizeof(float) * n}, {model[i], sizeof(float) * c->width[i] * n}) ||
            overlaps({d_scales, sizeof(float) * 3 * n}, {model[i], sizeof(float) * c->width[i] * n}))
            return fail(c, GS_ERR_INVALID, "gs_mcmc_regularize: a gradient array overlaps the model");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_mcmc_regularize(c->scales, c->opac, d_scales, d_opac, c->n, c_opacity, c_scale, c->stream));
    return GS_OK;                                                          // the model stands: so do the frame and the plans
}

}  // extern "C"
