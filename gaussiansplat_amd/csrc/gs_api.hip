// gs_api.hip -- host side of the C ABI declared in include/gsplat.h.
//
// Mirrors the reference's host drivers -- getRenderer (src/renderer.jl:119-149), preprocess
// (src/forward.jl:35-111), compactIdxs (src/forward.jl:118-161), forward (src/forward.jl:163-198),
// backward (src/backward.jl:3-38), resetGrads (src/splat.jl:158-173) -- without their
// per-frame costs: the model stays resident (the reference re-uploads it with `|> CuArray`
// on every call, forward.jl:63-69,169-170), scratch is grow-only (the reference re-allocates
// hitIdxs/hits/hitScans each frame, forward.jl:120,137,142), every stage is enqueued on one
// stream with a single host read-back (the instance count; the reference syncs after every
// kernel and reads maxHits back, forward.jl:72-156).
// (The ctx itself and the helpers shared by the gs_api_*.hip files: gs_ctx.h.)
#include "gs_ctx.h"

std::string g_create_error;

// What the preprocess kernels of the two renderers share: the grid, the four outputs and, with export_debug, the debug arrays (2-D: no ts, tps, cov3d)
template <typename A> static int preprocess_outputs(gs_ctx *c, A &a) {
    a.gx = c->gx; a.gy = c->gy;
    a.payload = c->payload.as<GsPayload>(); a.invcov = c->invcov.as<float>(); a.depth_key = c->depth_key.as<uint32_t>(); a.rect = c->rect.as<uint16_t>();
    if (!c->cfg.export_debug) return GS_OK;
    for (int i = 0; i < gs_ctx::DBG_COUNT; ++i) HIPCHK(c, c->dbg[i].ensure(sizeof(float) * gs_ctx::DBG_WIDTH[i] * c->n1()));
    auto arr = [c](gs_ctx::Dbg i) { return c->dbg[i].as<float>(); };
    a.dbg.mu = arr(gs_ctx::DBG_MU); a.dbg.cov2d = arr(gs_ctx::DBG_COV2D); a.dbg.invcov = arr(gs_ctx::DBG_INVCOV); a.dbg.bbs = arr(gs_ctx::DBG_BBS);
    if (c->kind == 0) { a.dbg.ts = arr(gs_ctx::DBG_TS); a.dbg.tps = arr(gs_ctx::DBG_TPS); a.dbg.cov3d = arr(gs_ctx::DBG_COV3D); }
    return GS_OK;
}

extern "C" {

void gs_default_config(gs_config *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(gs_config);
    cfg->abi_version = GS_ABI_VERSION;
    cfg->tile_size = GS_TILE;
    cfg->order = GS_ORDER_DEPTH_DESC;
    cfg->t_min = 1e-5f;
    cfg->deterministic = 0;
    cfg->export_debug = 0;
    cfg->profile_stages = 0;
    cfg->rank_mode = 1;                  // ballots: with the two-level binning the LDS-atomic rank only serves the depth sort (0.3 % of a C3 frame)
    cfg->alpha_cull = 1;
    cfg->schedule = 3;
    cfg->slab_mode = 1;
}

int gs_abi_version(void) { return GS_ABI_VERSION; }

const char *gs_last_error(const gs_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int gs_create(gs_ctx **out, int device, const gs_config *cfg) {
    if (!out) return fail(nullptr, GS_ERR_INVALID, "gs_create: out is NULL");
    *out = nullptr;
    gs_config c0;
    gs_default_config(&c0);
    if (cfg) {
        if (cfg->struct_size != (int32_t)sizeof(gs_config) || cfg->abi_version != GS_ABI_VERSION)
            return fail(nullptr, GS_ERR_INVALID, "gs_create: gs_config.struct_size / abi_version mismatch (caller built against another gsplat.h)");
        c0 = *cfg;
    }
    if (c0.schedule == 0) c0.schedule = 3;                               // 0 = the library default
    if (c0.tile_size != GS_TILE) return fail(nullptr, GS_ERR_UNSUPPORTED, "gs_create: only tile_size 16 is supported (reference threads=(16,16))");
    if (c0.order < GS_ORDER_INDEX || c0.order > GS_ORDER_DEPTH_ASC) return fail(nullptr, GS_ERR_INVALID, "gs_create: bad order");
    if (!(c0.t_min >= 0.0f)) return fail(nullptr, GS_ERR_INVALID, "gs_create: t_min must be >= 0");
    if (c0.schedule != 1 && c0.schedule != 3 && c0.schedule != 4) return fail(nullptr, GS_ERR_INVALID, "gs_create: bad schedule (0, 1, 3 or 4)");
    if (c0.slab_mode < 0 || c0.slab_mode > 1) return fail(nullptr, GS_ERR_INVALID, "gs_create: bad slab_mode");
    if (c0.bin_path < 0 || c0.bin_path > 3) return fail(nullptr, GS_ERR_INVALID, "gs_create: bad bin_path");
    if (!(c0.slab_max_ratio >= 0.0f && c0.slab_max_ratio <= 1.0f)) return fail(nullptr, GS_ERR_INVALID, "gs_create: slab_max_ratio must be in [0, 1]");
    for (int i = 0; i < 3; ++i)
        if (!(c0.slab_fractions[i] >= 0.0f && c0.slab_fractions[i] < 1.0f)) return fail(nullptr, GS_ERR_INVALID, "gs_create: slab_fractions must be in [0, 1)");
    if (c0.debug_flags & ~(GS_DEBUG_WIDE_CURSORS | GS_DEBUG_ALWAYS_ORDER | GS_DEBUG_TINY_CAPS | GS_DEBUG_SUPER16 | GS_DEBUG_SUPER8 | GS_DEBUG_NO_TAIL_FILL)) return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown debug_flags");
    if (c0.depth_sort < 0 || c0.depth_sort > 2) return fail(nullptr, GS_ERR_INVALID, "gs_create: depth_sort must be 0, 1 or 2");
    if (c0.list_cap < 0 || c0.list_cap > 2) return fail(nullptr, GS_ERR_INVALID, "gs_create: list_cap must be 0, 1 or 2");
    if (c0.tile_parts != 0 && c0.tile_parts != 1 && c0.tile_parts != 2 && c0.tile_parts != 4) return fail(nullptr, GS_ERR_INVALID, "gs_create: tile_parts must be 0, 1, 2 or 4");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, GS_ERR_NO_DEVICE, "gs_create: no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, GS_ERR_INVALID, "gs_create: device index out of range");
    gs_ctx *c = new (std::nothrow) gs_ctx();
    if (!c) return fail(nullptr, GS_ERR_OOM, "gs_create: host allocation failed");
    c->device = device;
    c->cfg = c0;
    c->slots.resize(GS_MAX_VIEW_SLOTS + 1);
    if ((e = hipSetDevice(device)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipSetDevice"); }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipStreamCreate"); }
    c->own_stream = true;
    {   // wave slots: CUs x 4 SIMDs x 5 by definition -- what "the grid fills the chip" means (the composite backward holds six waves per SIMD by now)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->wave_slots = prop.multiProcessorCount * 4 * 5;
        else (void)hipGetLastError();
    }
    if ((e = hipHostMalloc((void **)&c->pinned, sizeof(PinnedWords), hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipHostMalloc"); }
    if ((e = hipHostMalloc((void **)&c->pinned_split, sizeof(uint32_t) * 2 * (GS_MAX_VIEW_SLOTS + 1), hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess) {
        (void)hipGetLastError(); c->pinned_split = nullptr;              // (speed only: without it every order counts as "may hold split tiles")
    } else {
        std::memset(c->pinned_split, 0, sizeof(uint32_t) * 2 * (GS_MAX_VIEW_SLOTS + 1));
        for (size_t k = 0; k < c->slots.size(); ++k) c->slots[k].split_words = c->pinned_split + 2 * k;      // each slot knows its own two words
    }
    for (auto &pair : c->ev)
        for (hipEvent_t &ev : pair) if ((e = hipEventCreate(&ev)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipEventCreate"); }
    if ((e = hipEventCreateWithFlags(&c->ev_count, hipEventDisableTiming | hipEventReleaseToSystem)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipEventCreate"); }
    if ((e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipStreamCreate"); }
    for (hipEvent_t *ev : {&c->ev_main, &c->ev_order})
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) { delete c; return hipfail(nullptr, e, "hipEventCreate"); }
    if (c->cfg.rank_mode == 0) {
        // The one-instruction stable rank (ds_add_rtn pre-values in ascending lane order) is a measured property of
        // gfx950's LDS, not an architectural guarantee: check it on THIS device before relying on it; ballots otherwise.
        int bad = 0;
        if ((e = gs_probe_lds_atomic_order(c->stream, &bad)) != hipSuccess) { delete c; return hipfail(nullptr, e, "gs_probe_lds_atomic_order"); }
        c->rank_probe = bad ? 1 : 0;
        if (bad) c->cfg.rank_mode = 1;
    }
    *out = c;
    return GS_OK;
}

int gs_destroy(gs_ctx *c) {
    if (!c) return GS_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->side) (void)hipStreamSynchronize(c->side);
    delete c;
    return GS_OK;
}

int gs_set_stream(gs_ctx *c, void *hip_stream) {
    if (!c) return GS_ERR_INVALID;
    // GS_STREAM_LEGACY (= hipStreamLegacy) names the device's default (null) stream, which a NULL argument cannot
    hipStream_t want = hip_stream == (void *)1 ? (hipStream_t) nullptr : (hipStream_t)hip_stream;
    if (hip_stream && !c->own_stream && c->stream == want && c->borrowed_stream) return GS_OK;      // unchanged: no sync
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
    if (c->own_stream && c->stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    if (hip_stream) { c->stream = want; c->borrowed_stream = true; }
    else { HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; c->borrowed_stream = false; }
    return GS_OK;
}

int gs_synchronize(gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
    return GS_OK;
}

// the five arrays of a model become the ctx's: copied into its own buffers (host arrays) or borrowed (device arrays)
static int adopt_model(gs_ctx *c, int64_t n, int sh_degree, int kind, const float *const src[5], const size_t (&width)[5], int mem) {
    if (bind_device(c)) return GS_ERR_HIP;
    const float *dst[5];
    for (int i = 0; i < 5; ++i) {
        dst[i] = src[i];
        if (mem != GS_MEM_HOST) continue;
        const size_t bytes = sizeof(float) * width[i] * (size_t)n;
        HIPCHK(c, c->model[i].ensure(bytes ? bytes : 4));
        if (bytes) HIPCHK(c, hipMemcpyAsync(c->model[i].p, src[i], bytes, hipMemcpyHostToDevice, c->stream));
        dst[i] = c->model[i].as<float>();
    }
    if (mem == GS_MEM_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));            // caller may free its host arrays on return
    c->n = n; c->sh_degree = sh_degree; c->kind = kind;
    for (int i = 0; i < 5; ++i) c->width[i] = width[i];
    c->set_model5(dst);
    c->inputs_changed();
    return GS_OK;
}

int gs_set_model(gs_ctx *c, int64_t n, int sh_degree, const float *means, const float *scales, const float *quats,
                 const float *opacities, const float *shs, int mem) {
    if (!c) return GS_ERR_INVALID;
    if (n < 0 || n > 0x7FFFFFF0LL) return fail(c, GS_ERR_INVALID, "gs_set_model: n out of range");
    if (sh_degree < 0 || sh_degree > 3) return fail(c, GS_ERR_UNSUPPORTED, "gs_set_model: sh_degree must be 0..3");
    if (n > 0 && (!means || !scales || !quats || !opacities || !shs)) return fail(c, GS_ERR_INVALID, "gs_set_model: NULL array");
    if (const int rc = need_mem(c, "gs_set_model", mem)) return rc;
    const int K = (sh_degree + 1) * (sh_degree + 1);
    const float *src[5] = {means, scales, quats, opacities, shs};
    return adopt_model(c, n, sh_degree, 0, src, {3, 3, 4, 1, (size_t)3 * K}, mem);
}

int gs_set_model_2d(gs_ctx *c, int64_t n, const float *means, const float *scales, const float *rotations,
                    const float *opacities, const float *colors, int mem) {
    if (!c) return GS_ERR_INVALID;
    if (n < 0 || n > 0x7FFFFFF0LL) return fail(c, GS_ERR_INVALID, "gs_set_model_2d: n out of range");
    if (n > 0 && (!means || !scales || !rotations || !opacities || !colors)) return fail(c, GS_ERR_INVALID, "gs_set_model_2d: NULL array");
    if (const int rc = need_mem(c, "gs_set_model_2d", mem)) return rc;
    const float *src[5] = {means, scales, rotations, opacities, colors};
    return adopt_model(c, n, 0, 1, src, {2, 2, 1, 1, 3}, mem);
}

// The active degree: the kernels that touch SH evaluate bands 0 .. active only; rows keep the model's stride.  A change of the EFFECTIVE value is a
// change of the model as far as the frame is concerned (an optimiser step does the same); the value in force costs nothing.
int gs_set_active_sh_degree(gs_ctx *c, int degree) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_set_active_sh_degree")) return rc;
    if (degree < -1 || degree > 3) return fail(c, GS_ERR_INVALID, "gs_set_active_sh_degree: degree must be -1 (the model's own) or 0..3");
    const int before = c->active_sh_degree();
    c->sh_active_request = degree;
    if (c->active_sh_degree() != before) c->inputs_changed();
    return GS_OK;
}

int gs_get_active_sh_degree(const gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (c->kind != 0) return GS_ERR_UNSUPPORTED;
    return c->active_sh_degree();
}

// The background colour: what gs_forward adds behind the last splat.  The lists do not depend on it, so a change takes the frame back to
// Stage::BINNED only -- the image is stale and a backward asks for gs_forward first; the value in force costs nothing.
int gs_set_background(gs_ctx *c, const float rgb[3]) {
    if (!c) return GS_ERR_INVALID;
    if (!rgb) return fail(c, GS_ERR_INVALID, "gs_set_background: NULL argument");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(rgb[i])) return fail(c, GS_ERR_INVALID, "gs_set_background: the components must be finite");
    if (rgb[0] == c->background[0] && rgb[1] == c->background[1] && rgb[2] == c->background[2]) return GS_OK;
    for (int i = 0; i < 3; ++i) c->background[i] = rgb[i];
    c->fall_back(gs_ctx::Stage::BINNED);
    return GS_OK;
}

int gs_get_background(const gs_ctx *c, float rgb[3]) {
    if (!c || !rgb) return GS_ERR_INVALID;
    for (int i = 0; i < 3; ++i) rgb[i] = c->background[i];
    return GS_OK;
}

// A training target with straight alpha, composited over the ctx's background: what the loss compares the frame against.
int gs_compose_target(gs_ctx *c, const float *rgba, int32_t W, int32_t H, float *rgb_out) {
    if (!c) return GS_ERR_INVALID;
    if (!rgba || !rgb_out) return fail(c, GS_ERR_INVALID, "gs_compose_target: NULL argument");
    if (const int rc = need_image_size(c, "gs_compose_target", W, H)) return rc;
    const size_t px = (size_t)W * H;
    if (overlaps({rgb_out, sizeof(float) * 3 * px}, {rgba, sizeof(float) * 4 * px})) return fail(c, GS_ERR_INVALID, "gs_compose_target: rgb_out overlaps rgba");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, gs_launch_compose_target(rgba, rgb_out, px, c->background, c->stream));
    return GS_OK;
}

int gs_set_image_size(gs_ctx *c, int32_t W, int32_t H) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_image_size(c, "gs_set_image_size", W, H)) return rc;
    if (!c->have_cam) {                                  // a harmless camera, so the shared paths have one
        std::memset(&c->cam, 0, sizeof(c->cam));
        c->cam.near_ = -1.0f; c->cam.far_ = 1.0f;
    }
    c->cam.W = W; c->cam.H = H;
    c->have_cam = true;
    c->inputs_changed();
    return GS_OK;
}

int gs_set_camera(gs_ctx *c, const float T[16], const float P[16], float fx, float fy, float near_, float far_,
                  const float eye[3], const float lookAt[3], int32_t W, int32_t H) {
    if (!c) return GS_ERR_INVALID;
    if (!T || !P || !eye || !lookAt) return fail(c, GS_ERR_INVALID, "gs_set_camera: NULL argument");
    if (const int rc = need_image_size(c, "gs_set_camera", W, H)) return rc;
    std::memcpy(c->cam.T, T, sizeof(float) * 16);
    std::memcpy(c->cam.P, P, sizeof(float) * 16);
    c->cam.fx = fx; c->cam.fy = fy; c->cam.near_ = near_; c->cam.far_ = far_;
    for (int i = 0; i < 3; ++i) { c->cam.eye[i] = eye[i]; c->cam.lookAt[i] = lookAt[i]; }
    c->cam.W = W; c->cam.H = H;
    c->have_cam = true;
    c->inputs_changed();
    return GS_OK;
}

int gs_preprocess(gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (!c->have_cam) return fail(c, GS_ERR_INVALID, "gs_preprocess: gs_set_camera first");
    if (bind_device(c)) return GS_ERR_HIP;
    if (int rc = settle_totals(c, nullptr, false)) return rc;               // totals of a frame that was binned but never rendered
    c->frame_id += 1;
    HIPCHK(c, c->payload.ensure(sizeof(GsPayload) * c->n1()));
    HIPCHK(c, c->invcov.ensure(sizeof(float) * 4 * c->n1()));
    HIPCHK(c, c->depth_key.ensure(sizeof(uint32_t) * c->n1()));
    HIPCHK(c, c->rect.ensure(sizeof(uint16_t) * 4 * c->n1()));
    // the tile grid is fixed by the image: the reference passes blocks = size/threads (main.jl:9-11)
    c->gx = (c->cam.W + GS_TILE - 1) / GS_TILE;
    c->gy = (c->cam.H + GS_TILE - 1) / GS_TILE;
    c->range_valid = false;
    GsPreprocessArgs a{};
    GsPreprocess2DArgs a2{};
    if (c->kind == 1) {                                  // preprocess(::GaussianRenderer2D), forward.jl:9-33
        a2.n = c->n; a2.W = c->cam.W; a2.H = c->cam.H;
        a2.means = c->means; a2.scales = c->scales; a2.rots = c->quats; a2.opac = c->opac; a2.colors = c->shs;
        if (int rc = preprocess_outputs(c, a2)) return rc;
    } else {
        model_head(c, a);
        a.order = c->cfg.order;
        // the key range is folded only when this frame's depth sort can take the bucket path: while the classic sort runs (the 64-frame
        // fallback, N beyond the bucket path's limit) nothing would reset the accumulators and the atomics would be wasted
        if (c->dsort_can_bucket() && c->order() != GS_ORDER_INDEX && c->n > 0 && !c->small_bin_possible()) {
            if (!c->key_range.p) {
                HIPCHK(c, c->key_range.ensure(sizeof(uint32_t) * gs_depth_range_words()));
                HIPCHK(c, gs_depth_range_reset(c->key_range.as<uint32_t>(), c->stream));
            }
            c->range_parity ^= 1;
            a.key_range = key_range_of(c, c->range_parity);
            c->range_valid = true;
        }
        if (int rc = preprocess_outputs(c, a)) return rc;
    }
    StageTimer t(c, GS_STAGE_PREPROCESS);
    HIPCHK(c, c->kind == 1 ? gs_launch_preprocess2d(a2, c->stream) : gs_launch_preprocess(a, c->cam, c->sh_row_floats(), c->stream));
    c->reach(gs_ctx::Stage::PREPROCESSED);
    return GS_OK;
}

int gs_loss_l1_dssim(gs_ctx *c, const float *img, const float *gt, int32_t W, int32_t H, int32_t C, float lam, float *dC,
                     double *loss_out, int mem) {
    if (!c || !img || !gt) return GS_ERR_INVALID;
    if (W <= 0 || H <= 0 || C <= 0) return fail(c, GS_ERR_INVALID, "gs_loss_l1_dssim: bad image size");
    if (const int rc = need_mem(c, "gs_loss_l1_dssim", mem)) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)W * H * C;
    HIPCHK(c, c->loss_maps.ensure(sizeof(float) * 3 * n));
    HIPCHK(c, c->loss_acc.ensure(sizeof(double) * GS_LOSS_SLOTS * GS_LOSS_SLOT_STRIDE));
    const float *d_img = img, *d_gt = gt;
    float *d_dc = dC;
    if (mem == GS_MEM_HOST) {
        HIPCHK(c, c->loss_in[0].ensure(sizeof(float) * n));
        HIPCHK(c, c->loss_in[1].ensure(sizeof(float) * n));
        HIPCHK(c, hipMemcpyAsync(c->loss_in[0].p, img, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->loss_in[1].p, gt, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
        d_img = c->loss_in[0].as<float>(); d_gt = c->loss_in[1].as<float>();
    }
    if (mem == GS_MEM_HOST || !dC) { HIPCHK(c, c->loss_dc.ensure(sizeof(float) * n)); d_dc = c->loss_dc.as<float>(); }
    // window of loss.jl:5-12: exp(-r)/sqrt(2 sigma^2), r = distance from (6,6), normalised (sigma cancels); Float64 -> Float32
    float win[121];
    {
        double k[121], sum = 0.0;
        for (int j = 0; j < 11; ++j)
            for (int i = 0; i < 11; ++i) { k[j * 11 + i] = std::exp(-std::sqrt((double)((5 - j) * (5 - j) + (5 - i) * (5 - i)))); sum += k[j * 11 + i]; }
        for (int i = 0; i < 121; ++i) win[i] = (float)(k[i] / sum);
    }
    HIPCHK(c, gs_loss_run(W, H, C, d_img, d_gt, c->loss_maps.as<float>(), c->loss_acc.as<double>(), d_dc, lam, win, c->stream));
    if (mem == GS_MEM_HOST && dC) HIPCHK(c, hipMemcpyAsync(dC, d_dc, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (loss_out) {
        double slots[GS_LOSS_SLOTS * GS_LOSS_SLOT_STRIDE], acc[2] = {0.0, 0.0};
        HIPCHK(c, hipMemcpyAsync(slots, c->loss_acc.p, sizeof(slots), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < GS_LOSS_SLOTS; ++k) { acc[0] += slots[k * GS_LOSS_SLOT_STRIDE]; acc[1] += slots[k * GS_LOSS_SLOT_STRIDE + 1]; }
        *loss_out = (1.0 - (double)lam) * acc[0] / (2.0 * (double)n) + (double)lam * (1.0 - acc[1] / (double)n) / 2.0;
    } else if (mem == GS_MEM_HOST) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

int gs_sgd_step(gs_ctx *c, float lr, const gs_grads *g) {
    if (!c || !g) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)c->n;
    const Five<float> p = c->model5_mut(), gr = five(*g);
    for (int i = 0; i < 5; ++i) HIPCHK(c, gs_launch_sgd(p[i], gr[i], lr, c->width[i] * n, c->stream));
    c->inputs_changed();
    return GS_OK;
}

int gs_reset_grads(gs_ctx *c, const gs_grads *g) {
    if (!c || !g) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)c->n;
    const Five<float> p = five(*g);
    for (int i = 0; i < 5; ++i)
        if (p[i] && n) HIPCHK(c, hipMemsetAsync(p[i], 0, sizeof(float) * c->width[i] * n, c->stream));
    return GS_OK;
}

int gs_grads_alloc(gs_ctx *c, gs_grads *out) {
    if (!c || !out) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)c->n;
    size_t off[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 5; ++i) off[i + 1] = off[i] + c->width[i] * n;
    const size_t total = off[5];
    HIPCHK(c, c->grads_flat.ensure(sizeof(float) * (total ? total : 1)));
    HIPCHK(c, hipMemsetAsync(c->grads_flat.p, 0, sizeof(float) * total, c->stream));
    float *f = c->grads_flat.as<float>();
    out->d_means = f; out->d_scales = f + off[1]; out->d_quats = f + off[2]; out->d_opacities = f + off[3]; out->d_shs = f + off[4];
    return GS_OK;
}

int gs_grads_read(gs_ctx *c, const gs_grads *g, float *h_means, float *h_scales, float *h_quats, float *h_opacities, float *h_shs) {
    if (!c || !g) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)c->n;
    const Five<float> src = five(*g);
    float *dst[5] = {h_means, h_scales, h_quats, h_opacities, h_shs};
    for (int i = 0; i < 5; ++i)
        if (dst[i] && src[i] && n) HIPCHK(c, hipMemcpyAsync(dst[i], src[i], sizeof(float) * c->width[i] * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

}  // extern "C"
