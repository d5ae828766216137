// gs_api_debug.hip -- introspection for the parity tests (gs_get_array: the reference's scratch arrays and the tile lists) and the
// profiling hooks (per-stage hipEvent timers, work counters, per-tile clocks, isolated composite launches).
#include "gs_ctx.h"
#include "gs_pergaussian.h"

using Stage = gs_ctx::Stage;

extern "C" {

int64_t gs_num_gaussians(const gs_ctx *c) { return c ? c->n : 0; }
int64_t gs_num_instances(gs_ctx *c) { if (!c) return 0; (void)settle_totals(c, nullptr, true); return c->n_inst; }
int64_t gs_num_coarse_instances(gs_ctx *c) { if (!c) return 0; (void)settle_totals(c, nullptr, true); return c->bin.radix() ? 0 : c->n_coarse; }
int gs_num_rounds(const gs_ctx *c) { return c ? c->bin.n_rounds : 0; }

int gs_get_array(gs_ctx *c, int which, void *dst, int64_t bytes) {
    if (!c || !dst) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t n = (size_t)c->n;
    const void *src = nullptr;
    size_t need = 0;
    auto need_dbg = [&](gs_ctx::Dbg i) -> int {
        if (!c->cfg.export_debug) return fail(c, GS_ERR_INVALID, "gs_get_array: needs gs_config.export_debug = 1");
        src = c->dbg[i].p; need = sizeof(float) * gs_ctx::DBG_WIDTH[i] * n; return GS_OK;
    };
    int rc = GS_OK;
    if (which <= GS_ARR_TILE_RECT && (rc = need_stage(c, Stage::PREPROCESSED, "gs_get_array: gs_preprocess first"))) return rc;
    if (which >= GS_ARR_SORT_IDXS && which <= GS_ARR_SORTED_KEYS && (rc = need_stage(c, Stage::BINNED, "gs_get_array: gs_bin first"))) return rc;
    if (which >= GS_ARR_TILE_RANGES && which <= GS_ARR_SORTED_KEYS && (rc = settle_totals(c, nullptr, true))) return rc;
    if (which >= GS_ARR_TILE_RANGES && which <= GS_ARR_SORTED_KEYS && c->bin.n_rounds > 1)
        return fail(c, GS_ERR_INVALID, "gs_get_array: this frame was binned in depth slabs (lists spread over rounds); use gs_config.slab_mode = 0");
    if ((which == GS_ARR_SORTED_IDS || which == GS_ARR_SORTED_KEYS) && c->live.frame_capped && c->live.have_l2) {
        // capped lists: only the part of every list the view slot's history says is walked has been written.  Write the rest now (the
        // same kernel with the caps off: same positions, same order); from here on the frame's lists are complete.
        GsBin3Args a = c->live.last_l2;
        a.cap_src = nullptr; a.tile_nopen = nullptr; a.smax = nullptr; a.tile_ext = nullptr;
        HIPCHK(c, gs_bin3_write_lists(a, c->stream));
        c->live.frame_capped = false;
    }
    switch (which) {
        case GS_ARR_TS: if ((rc = need_dbg(gs_ctx::DBG_TS))) return rc; break;
        case GS_ARR_TPS: if ((rc = need_dbg(gs_ctx::DBG_TPS))) return rc; break;
        case GS_ARR_COV3D: if ((rc = need_dbg(gs_ctx::DBG_COV3D))) return rc; break;
        case GS_ARR_COV2D: if ((rc = need_dbg(gs_ctx::DBG_COV2D))) return rc; break;
        case GS_ARR_BBS: if ((rc = need_dbg(gs_ctx::DBG_BBS))) return rc; break;
        case GS_ARR_INVCOV: src = c->invcov.p; need = sizeof(float) * 4 * n; break;
        case GS_ARR_MU: case GS_ARR_RGB: case GS_ARR_SIG: {
            const size_t w = which == GS_ARR_MU ? 2 : which == GS_ARR_RGB ? 3 : 1;
            if ((size_t)bytes != sizeof(float) * w * n) return fail(c, GS_ERR_INVALID, "gs_get_array: size mismatch");
            std::vector<GsPayload> h(c->n1());
            HIPCHK(c, hipMemcpyAsync(h.data(), c->payload.p, sizeof(GsPayload) * n, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            float *o = static_cast<float *>(dst);
            for (size_t g = 0; g < n; ++g) {
                const GsPayload &p = h[g];
                if (which == GS_ARR_MU) { o[2 * g] = p.mx; o[2 * g + 1] = p.my; }
                else if (which == GS_ARR_RGB) { o[3 * g] = p.r; o[3 * g + 1] = p.g; o[3 * g + 2] = p.b; }
                else o[g] = p.sig;
            }
            return GS_OK;
        }
        case GS_ARR_DEPTH_KEY: src = c->depth_key.p; need = sizeof(uint32_t) * n; break;
        case GS_ARR_TILE_RECT: src = c->rect.p; need = sizeof(uint16_t) * 4 * n; break;
        case GS_ARR_SORT_IDXS: {
            if ((size_t)bytes != sizeof(uint32_t) * n) return fail(c, GS_ERR_INVALID, "gs_get_array: size mismatch");
            // a frame binned by the small path (gs_bin_small.hip) sorted nothing globally
            if (c->bin.perm_on_demand && !c->live.perm_ptr && (rc = depth_order(c))) return rc;
            if (c->live.perm_ptr) { src = c->live.perm_ptr; need = sizeof(uint32_t) * n; break; }
            uint32_t *o = static_cast<uint32_t *>(dst);
            for (size_t g = 0; g < n; ++g) o[g] = (uint32_t)g;
            return GS_OK;
        }
        case GS_ARR_TILE_RANGES: src = c->ranges.p; need = sizeof(uint32_t) * 2 * c->ntiles(); break;
        case GS_ARR_SORTED_IDS: case GS_ARR_SORTED_KEYS: {
            const size_t ni = (size_t)c->n_inst, nt = (size_t)c->ntiles();
            const size_t w = which == GS_ARR_SORTED_IDS ? sizeof(uint32_t) : sizeof(uint64_t);
            if ((size_t)bytes != w * ni) return fail(c, GS_ERR_INVALID, "gs_get_array: size mismatch");
            std::vector<uint32_t> h(ni ? ni : 1), dk(c->n1()), rg(2 * c->ntiles1());
            HIPCHK(c, hipMemcpyAsync(h.data(), c->ids.p, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(dk.data(), c->depth_key.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(rg.data(), c->ranges.p, sizeof(uint32_t) * 2 * nt, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (which == GS_ARR_SORTED_IDS) {
                std::memcpy(dst, h.data(), sizeof(uint32_t) * ni);
            } else {                                   // tile<<32 | depth key (or | id): the key the list order realises
                uint64_t *o = static_cast<uint64_t *>(dst);
                const bool by_index = c->order() == GS_ORDER_INDEX;
                for (size_t t = 0; t < nt; ++t)
                    for (size_t p = rg[2 * t]; p < rg[2 * t + 1] && p < ni; ++p)
                        o[p] = ((uint64_t)t << 32) | (by_index ? h[p] : dk[h[p]]);
            }
            return GS_OK;
        }
        case GS_ARR_GRAD2D: {
            if ((rc = need_stage(c, Stage::COMPOSITE_ADJOINT, "gs_get_array: gs_backward first"))) return rc;
            if ((size_t)bytes != sizeof(float) * 10 * n) return fail(c, GS_ERR_INVALID, "gs_get_array: size mismatch");
            float *o = static_cast<float *>(dst);
            // the device rows (float, or fixed point in deterministic mode) hold raw moments: apply the per-gaussian factors with the view's payload (sig, conic)
            const bool fixed = c->cfg.deterministic;
            std::vector<long long> fx(fixed ? GS_G2D_STRIDE * c->n1() : 0);
            std::vector<float> fl(fixed ? 0 : GS_G2D_STRIDE * c->n1());
            std::vector<GsPayload> pay(c->n1());
            std::vector<float> ic(4 * c->n1());
            if (n) HIPCHK(c, hipMemcpyAsync(fixed ? (void *)fx.data() : (void *)fl.data(), c->g2d.p, c->g2d_bytes(), hipMemcpyDeviceToHost, c->stream));
            if (n) HIPCHK(c, hipMemcpyAsync(pay.data(), c->payload.p, sizeof(GsPayload) * n, hipMemcpyDeviceToHost, c->stream));
            if (n) HIPCHK(c, hipMemcpyAsync(ic.data(), c->invcov.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (size_t g = 0; g < n; ++g) {
                float row[10];
                gs_g2d_row_load(GsG2dRows{fl.data(), fixed ? fx.data() : nullptr}, (int64_t)g, row);
                gs_g2d_to_grads(row, pay[g].sig, ic[4 * g], 0.5f * (ic[4 * g + 1] + ic[4 * g + 2]), ic[4 * g + 3]);
                for (int i = 0; i < 10; ++i) o[10 * g + i] = row[i];
            }
            return GS_OK;
        }
        default: return fail(c, GS_ERR_INVALID, "gs_get_array: unknown array");
    }
    if ((size_t)bytes != need) return fail(c, GS_ERR_INVALID, "gs_get_array: size mismatch");
    if (need) HIPCHK(c, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_get_stage_times(gs_ctx *c, float ms[GS_STAGE_COUNT]) {
    if (!c || !ms) return GS_ERR_INVALID;
    if (!c->cfg.profile_stages) return fail(c, GS_ERR_INVALID, "gs_get_stage_times: needs gs_config.profile_stages = 1");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < GS_STAGE_COUNT; ++s) {
        ms[s] = 0.0f;
        if (c->ev_valid[s]) HIPCHK(c, hipEventElapsedTime(&ms[s], c->ev[s][0], c->ev[s][1]));
    }
    return GS_OK;
}

int gs_get_stage_stats(gs_ctx *c, double sum_ms[GS_STAGE_COUNT], int64_t count[GS_STAGE_COUNT], int reset) {
    if (!c || !sum_ms || !count) return GS_ERR_INVALID;
    if (!c->cfg.profile_stages) return fail(c, GS_ERR_INVALID, "gs_get_stage_stats: needs gs_config.profile_stages = 1");
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    harvest_events(c);
    for (int s = 0; s < GS_STAGE_COUNT; ++s) {
        sum_ms[s] = c->ev_sum[s]; count[s] = c->ev_cnt[s];
        if (reset) { c->ev_sum[s] = 0.0; c->ev_cnt[s] = 0; }
    }
    return GS_OK;
}

// An isolated launch over the finished frame, as the frame's plan ran it (composite_args) -- but for: no per-tile counters, a forward
// without snapshots in the order the backward had, and what the variant asks for.
// variant tens digit (gs_composite.hip: apply_sched_variant): 0 the frame's own launch order (what production uses for the
// backward and for the next forward of the slot), 1 tile order, 3 = 0 explicitly
static int debug_composite_args(gs_ctx *c, int which, int variant, GsCompositeArgs &a) {
    a = composite_args(c, which != 0, 0, true);
    a.dC = c->last_dC;
    if (variant >= 10000) {                                                  // + 10000: with the two work-counter atomics per tile of a real frame (scratch words; tools/atomics_tail.py)
        variant -= 10000;
        a.walked = c->counters.as<CounterBlock>()->scratch;
    }
    a.final_round = 1;
    c->live.rows_dirtied();
    a.variant = variant % 100;
    a.cull = (c->cfg.alpha_cull != 0) != (variant >= 1000);                  // +1000: the other cull setting
    if (c->dbg_win_len > 0) {                                                // gs_debug_set_window: a slice of the launch order
        // (a forward over a slice rewrites the slice's tiles only: the blend behind it would add the background to the others a second time)
        if (which == 0 && c->has_background()) return fail(c, GS_ERR_UNSUPPORTED, "gs_debug_set_window: forward launches over a window need a black background");
        if (!a.tile_order || a.parts > 1) return fail(c, GS_ERR_INVALID, "gs_debug_set_window: the frame has no launch order (or several waves per tile)");
        if (c->dbg_win_start + c->dbg_win_len > a.order_len) return fail(c, GS_ERR_INVALID, "gs_debug_set_window: beyond the launch order");
        a.tile_order += c->dbg_win_start; a.order_len = c->dbg_win_len;
    }
    return GS_OK;
}

int gs_debug_set_window(gs_ctx *c, int32_t start, int32_t len) {
    if (!c) return GS_ERR_INVALID;
    if (start < 0 || len < 0 || (start & 7) || (len & 7)) return fail(c, GS_ERR_INVALID, "gs_debug_set_window: start and len must be non-negative multiples of 8");
    c->dbg_win_start = start; c->dbg_win_len = len;
    return GS_OK;
}

int gs_debug_time_composite(gs_ctx *c, int which, int variant, int reps, float *mean_ms) {
    if (!c || !mean_ms || reps == 0) return GS_ERR_INVALID;
    const bool cold = reps < 0;                                               // negative: -reps launches WITHOUT the warm-up launch (tools/cold_fwd.py)
    if (cold) reps = -reps;
    int rc = need_stage(c, Stage::RENDERED, "gs_debug_time_composite: gs_forward first");
    if (rc || (which == 1 && (rc = need_stage(c, Stage::COMPOSITE_ADJOINT, "gs_debug_time_composite: gs_backward first")))) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    GsCompositeArgs a{};
    if (int rc = debug_composite_args(c, which, variant, a)) return rc;
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
    auto launch = [&]() -> hipError_t { return which == 0 ? gs_launch_composite_fwd(a, c->stream) : gs_launch_composite_bwd(a, c->stream); };
    if (!cold) HIPCHK(c, launch());   // warm
    HIPCHK(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < reps; ++i) HIPCHK(c, launch());
    HIPCHK(c, hipEventRecord(e1, c->stream));
    if (which == 0) { if (int rc = blend_background(c)) return rc; }          // the launches left C in the bound image: the frame stays what gs_forward left
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    *mean_ms = ms / reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return GS_OK;
}

int gs_debug_tile_clock(gs_ctx *c, int which, int variant, uint64_t *out) {
    if (!c || !out) return GS_ERR_INVALID;
    int rc = need_stage(c, Stage::RENDERED, "gs_debug_tile_clock: gs_forward first");
    if (rc || (which == 1 && (rc = need_stage(c, Stage::COMPOSITE_ADJOINT, "gs_debug_tile_clock: gs_backward first")))) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    GsCompositeArgs a{};
    const bool by_block = variant < 0;                                        // negative variant: records per WORKGROUP (launches with split tiles):
    if (by_block) variant = -variant;                                         // out holds gs_debug_tile_clock_rows() rows
    if (int rc = debug_composite_args(c, which, variant, a)) return rc;
    if (by_block) {
        // a frame with a launch order, or a small grid whose tiles are shared between waves (pixel parts / list segments)
        if ((!a.tile_order && a.parts <= 1 && !a.seg_hist) || (a.variant / 10) % 10 == 1)
            return fail(c, GS_ERR_INVALID, "gs_debug_tile_clock: records by workgroup need the frame's launch order (or a small grid's tile parts)");
        a.clock_by_block = 1;
    } else { a.split_ok = 0; a.snap = nullptr; }                              // records by tile: whole tiles only
    const size_t rows = a.clock_by_block ? (size_t)gs_debug_tile_clock_rows(c) : (size_t)c->ntiles();
    if (a.clock_by_block && (size_t)gs_composite_grid_blocks(a, which) > rows) return fail(c, GS_ERR_INVALID, "gs_debug_tile_clock: launch larger than its record");
    HIPCHK(c, c->tile_clock.ensure(sizeof(uint64_t) * GS_TILE_CLOCK_WORDS * (rows ? rows : 1)));
    HIPCHK(c, hipMemsetAsync(c->tile_clock.p, 0, sizeof(uint64_t) * GS_TILE_CLOCK_WORDS * rows, c->stream));
    a.tile_clock = c->tile_clock.as<unsigned long long>();
    for (int rep = 0; rep < 2; ++rep) {                                       // the second launch (warm) is the one kept
        HIPCHK(c, which == 0 ? gs_launch_composite_fwd(a, c->stream) : gs_launch_composite_bwd(a, c->stream));
    }
    if (which == 0) { if (int rc = blend_background(c)) return rc; }          // (as gs_debug_time_composite)
    HIPCHK(c, hipMemcpyAsync(out, c->tile_clock.p, sizeof(uint64_t) * GS_TILE_CLOCK_WORDS * rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_debug_tail_fill(gs_ctx *c, int32_t blocks[2]) {
    if (!c || !blocks) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_debug_tail_fill: gs_forward first")) return rc;
    blocks[0] = c->fill_blocks_fwd; blocks[1] = c->stage >= Stage::COMPOSITE_ADJOINT ? c->fill_blocks_bwd : 0;
    return GS_OK;
}

int gs_debug_tile_clock_rows(gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (c->lpt_schedule()) return c->lpt_order_entries() + gs_seg_units(c->lpt_front());
    // small grids: blocks of one part x the most waves a tile is given (pixel parts x list segments of the backward); 0: one wave per tile
    const int len = (((int)c->ntiles() + 7) / 8) * 8;
    const int units = c->plan.parts * (c->plan.snap == gs_ctx::FramePlan::Snap::ALL ? 4 * c->plan.seg_n : 1);   // (an upper bound: at most four parts on top of the segments)
    return units > 1 ? len * units : 0;
}

int gs_debug_clock_mhz(gs_ctx *c, float *mhz) {
    if (!c || !mhz) return GS_ERR_INVALID;
    if (bind_device(c)) return GS_ERR_HIP;
    HIPCHK(c, c->counters.ensure(GS_COUNTER_BYTES));
    unsigned long long *d = c->counters.as<CounterBlock>()->scratch, h[2] = {0, 1};
    HIPCHK(c, gs_launch_clock_probe(d, c->stream));
    HIPCHK(c, hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mhz = h[1] ? (float)((double)h[0] / (double)h[1] * 100.0) : 0.0f;       // s_memrealtime ticks at 100 MHz
    return GS_OK;
}

int gs_rank_probe_result(const gs_ctx *c) { return c ? c->rank_probe : -1; }

// counters[0..3] = {walked, evaluated} of the last forward and of the last composite backward, summed from the per-tile arrays
static int sum_work_counters(gs_ctx *c) {
    unsigned long long *w = c->counters.as<unsigned long long>();
    const int nt = (int)c->ntiles();
    HIPCHK(c, gs_launch_sum_tiles(c->feedback.walk, c->tile_work.as<uint32_t>(), nt, w, c->stream));
    if (c->stage >= Stage::COMPOSITE_ADJOINT && c->tile_walked_b.p && c->tile_work_b.p)
        HIPCHK(c, gs_launch_sum_tiles(c->tile_walked_b.as<uint32_t>(), c->tile_work_b.as<uint32_t>(), nt, w + 2, c->stream));
    else HIPCHK(c, hipMemsetAsync(w + 2, 0, 16, c->stream));
    return GS_OK;
}

int gs_get_work_counters(gs_ctx *c, int64_t *walked_fwd, int64_t *walked_bwd) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_get_work_counters: gs_forward first")) return rc;
    int64_t o[4];
    if (int rc = gs_get_work_counters_ex(c, o)) return rc;
    if (walked_fwd) *walked_fwd = o[0];
    if (walked_bwd) *walked_bwd = o[1];
    return GS_OK;
}

int gs_get_list_stats(gs_ctx *c, int64_t out[3]) {
    if (!c || !out) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_get_list_stats: gs_forward first")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    if (int rc = settle_totals(c, nullptr, true)) return rc;
    out[0] = c->n_inst; out[1] = 0; out[2] = 0;
    if (!c->live.frame_capped || c->bin.n_rounds != 1) return GS_OK;
    unsigned long long *d = c->counters.as<CounterBlock>()->scratch, h = 0;
    uint32_t e = 0;
    HIPCHK(c, gs_launch_sum_listed(c->tile_ext.as<uint2>(), (int)c->ntiles(), d, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&e, c->ext_count(), sizeof(e), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = (int64_t)h; out[1] = (int64_t)e; out[2] = 1;
    return GS_OK;
}

int gs_get_tile_parts(gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_get_tile_parts: gs_forward first")) return rc;
    return c->plan.parts;
}

int gs_get_bin_path(gs_ctx *c) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::BINNED, "gs_get_bin_path: gs_bin first")) return rc;
    return (int)c->bin.path;
}

int gs_get_work_counters_ex(gs_ctx *c, int64_t out[4]) {
    if (!c || !out) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_get_work_counters_ex: gs_forward first")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    unsigned long long h[4] = {0, 0, 0, 0};
    if (int rc = sum_work_counters(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(h, c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = (int64_t)h[0]; out[1] = (int64_t)h[2]; out[2] = (int64_t)h[1]; out[3] = (int64_t)h[3];
    return GS_OK;
}

}  // extern "C"
