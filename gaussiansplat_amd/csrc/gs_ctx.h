// gs_ctx.h -- the renderer context behind the C ABI (include/gsplat.h) and the host-side helpers its translation units share.
// Internal: nothing here is part of the ABI.  The entry points live in
//   gs_api.hip            create / destroy, model, camera, gs_preprocess (what both renderers share: preprocess_outputs), gradients buffers, loss, SGD
//   gs_api_bin.hip        gs_bin: the frame's bin plan (plan_bin), depth order, one function per path (bin_small, bin_two_level, bin_radix), settle_totals
//   gs_api_composite.hip  gs_forward / gs_backward: the frame's plan (plan_frame), the one builder of the composite launches' arguments
//                         (composite_args), the launch orders of the view slots; the backward family's plan (plan_backward) and run_backward
//   gs_api_comm.hip       RCCL below the boundary (gs_comm_*, gs_allreduce_grads)
//   gs_api_touched.hip    the touched-rows colour exchange (gs_color_rows_pack, gs_sh_grads_from_touched)
//   gs_api_density.hip    density control (gs_density_accumulate / _decide / _plan / _restructure, gs_opacity_reset)
//   gs_api_knn.hip        point-cloud initialisation (gs_knn_mean_dist2, gs_init_from_points)
//   gs_api_features.hip   feature maps (gs_view_depth, gs_render_features, gs_backward_features, gs_view_depth_backward)
//   gs_api_camera.hip     the camera gradient (gs_backward_camera)
//   gs_api_metrics.hip    evaluation metrics (gs_image_metrics, gs_metrics_finish)
//   gs_api_exposure.hip   the per-view exposure stage (gs_exposure_apply, gs_exposure_backward, gs_exposure_adam)
//   gs_api_bilagrid.hip   the per-view bilateral grid (gs_bilagrid_apply, gs_bilagrid_backward, gs_bilagrid_tv, gs_bilagrid_adam)
//   gs_api_mcmc.hip       MCMC densification (gs_mcmc_plan / _sample / _relocate / _noise / _regularize)
//   gs_background.hip     the background colour's two elementwise kernels (the forward's epilogue, gs_compose_target)
//   gs_api_debug.hip      introspection and profiling hooks (gs_get_array, stage timers, tile clocks, counters, isolated composite launches)
// How far the frame has come is ONE ordered value (gs_ctx::Stage): every entry point compares it, reaches a stage or falls back to one.
// What the ctx holds it owns: DevBuf frees itself, ~gs_ctx releases the communicator, events, streams and pinned blocks -- no list to keep.
// What every entry point needs is written ONCE, here: the refusals they share (need_3d, need_mem, need_model, need_image_size, need_stage, overlaps), the sizes
// (n1, ntiles, pixels), a buffer of gradient rows in the ctx's mode (gs_ctx::rows), the model head of an argument struct (model_head), the per-gaussian
// chain's arguments (chain_args), the export_debug arrays (gs_ctx::Dbg, DBG_WIDTH); what changes behind a frame's plans is one value (gs_ctx::FrameLive);
// what a frame takes from EARLIER frames has one owner each (HISTORY: ViewSlot, WalkFeedback, the order kernel's hand-off; the kernel itself: gs_order.hip).
#pragma once
#include "../../include/gsplat.h"
#include "gs_common.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

struct DevBuf {                               // grow-only device scratch that frees itself: what a gs_ctx holds of them goes with the ctx
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }   // movable (ViewSlot lives in a std::vector, sized once in gs_create), not copyable
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;                 // grow-only with slack
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
// five device arrays in the order of gs_ctx::width: a gs_grads (gradients, moments), or the model
template <typename T> struct Five { T *p[5]; T *operator[](int i) const { return p[i]; } };
inline Five<float> five(const gs_grads &g) { return {{g.d_means, g.d_scales, g.d_quats, g.d_opacities, g.d_shs}}; }

extern std::string g_create_error;         // message of the last failed gs_create (gs_last_error(NULL))

#define GS_COUNTER_BYTES 192
struct CounterBlock {                        // gs_ctx::counters on the device, and its copy inside the pinned block
    uint32_t work[8];                        // 4 x u64 {walked, evaluated} of the forward and of the backward: sums, on demand (sum_work_counters)
    uint32_t pad0[24];
    uint32_t totals[4];                      // byte 128: the binning totals {coarse instances listed, fine instances of the slab, of all n}
    uint32_t ext_count;                      // byte 144: list segments appended by composite waves (capped lists)
    uint32_t pad1[3];
    unsigned long long scratch[4];           // byte 160: debug scratch (clock probe, listed-entry sum, the work-counter atomics of a debug launch)
};
// The 512 coherent pinned host bytes of a ctx: what kernels and copies of the frame in flight leave for the host behind ev_count.
struct PinnedWords {
    uint32_t readback[2];                    // words 0, 1: copied back by the paths whose host waits.  Radix frame: {instances, generated positions of round 0};
                                             // later radix round: {its instances}; later two-level round: {coarse, fine instances of its slab}
    uint32_t walked_prev[2];                 // word 2: u64, entries the previous forward walked (radix paths)
    uint32_t pad0[4];
    CounterBlock counters;                   // word 8: two-level and small paths: `work[0..1]` = the previous forward's walk, `totals` = this frame's
    uint32_t pad1[44];
    uint32_t dsort_stat[2];                  // word 100: status of the depth sort's bucket path, two frame parities
    uint32_t pad2[26];
};
static_assert(sizeof(CounterBlock) == GS_COUNTER_BYTES && offsetof(CounterBlock, totals) == 128 && offsetof(CounterBlock, ext_count) == 144 &&
              offsetof(CounterBlock, scratch) == 160, "counter block layout (the kernels address it by these offsets)");
static_assert(sizeof(PinnedWords) == 512 && offsetof(PinnedWords, readback) == 0 && offsetof(PinnedWords, walked_prev) == 8 &&
              offsetof(PinnedWords, counters) == 32 && offsetof(PinnedWords, dsort_stat) == 400, "pinned block layout");
void comm_release(struct gs_ctx *c);         // gs_api_comm.hip: destroys the ctx's RCCL communicator, if any
struct gs_ctx {
    // the device is bound; gs_destroy has drained both streams (gs_create giving up has at most its failed probe behind it, which hipStreamDestroy
    // waits out on its own): the communicator first, the rest in any order, the DevBufs by themselves
    ~gs_ctx() {
        comm_release(this);
        for (auto &pair : ev) for (hipEvent_t e : pair) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_count, ev_main, ev_order}) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        for (void *h : {(void *)pinned, (void *)pinned_split}) if (h) (void)hipHostFree(h);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false, borrowed_stream = false;
    gs_config cfg{};
    std::string err;

    int64_t n = 0;
    int sh_degree = 0;
    // the active SH degree (gs_set_active_sh_degree): the REQUEST is the ctx's and outlives gs_set_model (densification re-adopts the model every
    // window); what the kernels evaluate is the effective value -- bands below it, on rows that keep the stored stride 3 (sh_degree + 1)^2
    int sh_active_request = -1;              // -1: the model's own degree
    int active_sh_degree() const { return sh_active_request < 0 || sh_active_request > sh_degree ? sh_degree : sh_active_request; }
    int sh_row_floats() const { return 3 * (sh_degree + 1) * (sh_degree + 1); }   // the stored row stride of shs, d_shs and their moments
    // the background colour (gs_set_background): like the active degree the request is the ctx's and outlives gs_set_model.  gs_forward leaves
    // C + T bg in the image (gs_background.hip, one launch behind the last composite round); all zeros: no launch, the frame over black
    float background[3] = {0.0f, 0.0f, 0.0f};
    bool has_background() const { return background[0] != 0.0f || background[1] != 0.0f || background[2] != 0.0f; }
    int kind = 0;                            // 0: 3-D renderer (SplatData3D), 1: 2-D image-fitting renderer (SplatData2D)
    size_t width[5] = {3, 3, 4, 1, 3};       // floats per gaussian of the five parameter / gradient arrays
    int order() const { return kind == 1 ? (int)GS_ORDER_INDEX : cfg.order; }    // the 2-D model has no depth
    const float *means = nullptr, *scales = nullptr, *quats = nullptr, *opac = nullptr, *shs = nullptr;
    DevBuf model[5];
    Five<const float> model5() const { return {{means, scales, quats, opac, shs}}; }
    // ... to write: the optimiser steps and the fused backwards update the resident model in place (the ctx's copy, or the caller's device arrays)
    Five<float> model5_mut() const { return {{const_cast<float *>(means), const_cast<float *>(scales), const_cast<float *>(quats), const_cast<float *>(opac), const_cast<float *>(shs)}}; }
    void set_model5(const float *const a[5]) { means = a[0]; scales = a[1]; quats = a[2]; opac = a[3]; shs = a[4]; }
    GsCamera cam{};
    bool have_cam = false;
    // ---- how far the frame has come, one linear progress: an entry point asks for the stage it needs, reaches its own once its work is enqueued, or falls back
    enum class Stage {
        NOTHING,                             // no frame: the model or the view changed (inputs_changed)
        PREPROCESSED,                        // gs_preprocess: payload rows, depth keys, tile rectangles
        BINNED,                              // gs_bin: the tile lists
        RENDERED,                            // gs_forward: image and transmittance, in the buffers bound at its time
        COMPOSITE_ADJOINT,                   // the composite backward ran on this forward: the 2-D gradient sums g2d exist (GS_BWD_PARAMS_ONLY, gs_color_grads_pack, GS_ARR_GRAD2D)
        BACKWARD                             // ... and the per-gaussian kernels behind it
    } stage = Stage::NOTHING;
    void reach(Stage s) { stage = s; }
    void fall_back(Stage s) { if (stage > s) stage = s; }                  // to at most s
    void inputs_changed() { fall_back(Stage::NOTHING); density.planned = false; mcmc.planned = false; }   // the model or the view changed: nothing of the frame stands, nor a density or MCMC plan
    int gx = 0, gy = 0;
    int64_t grid_key() const { return ((int64_t)gx << 32) | (int64_t)gy; }        // what per-grid history is tagged with (0: none)
    int64_t ntiles() const { return (int64_t)gx * gy; }                           // tiles of the grid (at most 2048 x 2048: fits an int) ...
    size_t ntiles1() const { const size_t nt = (size_t)ntiles(); return nt ? nt : 1; }   // ... and for buffer sizes (never zero)
    size_t n1() const { return n ? (size_t)n : 1; }                               // gaussians, for buffer sizes (never zero)
    size_t pixels() const { return (size_t)cam.W * cam.H; }

    DevBuf invcov;                           // 4 x n raw conic (introspection; the payload rows carry it scaled)
    DevBuf payload, depth_key, rect, pairs_a, pairs_b, perm, offsets, block_sums;
    DevBuf inst_a, inst_b, table, digit_total, ranges, image, trans, g2d, stage_in;
    // the export_debug arrays and their floats per gaussian: what gs_preprocess fills (the 2-D renderer: mu, cov2d, invcov, bbs) and gs_get_array hands out
    enum Dbg { DBG_TS, DBG_TPS, DBG_MU, DBG_COV3D, DBG_COV2D, DBG_INVCOV, DBG_BBS, DBG_COUNT };
    static constexpr size_t DBG_WIDTH[DBG_COUNT] = {4, 4, 2, 9, 4, 4, 4};
    DevBuf dbg[DBG_COUNT];
    DevBuf ids, words, cs, diff;             // sorted gaussian ids; pass-1 words; chunk owners; 2-D difference array
    int64_t n_inst = 0;
    PinnedWords *pinned = nullptr;
    const float *last_dC = nullptr;          // device dC of the last gs_backward (debug timing)

    hipEvent_t ev_count = nullptr;           // instance count landed in pinned memory
    hipEvent_t ev[GS_STAGE_COUNT][2] = {};
    bool ev_valid[GS_STAGE_COUNT] = {};      // a start/stop pair has been recorded
    bool ev_fresh[GS_STAGE_COUNT] = {};      // ... and not yet added to the accumulators
    double ev_sum[GS_STAGE_COUNT] = {};
    int64_t ev_cnt[GS_STAGE_COUNT] = {};
    DevBuf counters;                         // GS_COUNTER_BYTES: 4 x u64 {walked, evaluated} of the forward and of the backward (sum_work_counters), ...
    DevBuf tile_work, tile_clock;            // per-tile evaluated entries of the forward (the launch orders' input); debug clocks
    int wave_slots = 5120;                  // CUs x 4 SIMDs x 5 BY DEFINITION (gs_create): the unit of every threshold; the backward holds six waves per SIMD by now
    DevBuf tile_nopen, smax, tile_ext, zero_tiles;   // capped lists (gs_config.list_cap; FrameLive::frame_capped)
    // ---- the frame's LIVE state: what calls behind the plans change.  gs_bin starts every frame with a fresh value, so a member added here cannot be
    // forgotten in a reset.  Written by two_level_lists (capped lists), bin_small / gs_forward (g2d_clean), depth_order, gs_get_array's list completion, and
    // the member functions.  What outlives a gs_bin is NOT here: the frame's totals (n_inst, n_coarse, round_gen, round_ids_off, pending_totals), fwd_fills_g2d
    // and the fill-block counts, the depth sort's feedback words -- and the HISTORY below the plans: the view slots, `feedback`, the order kernel's hand-off.
    struct FrameLive {
        bool frame_capped = false;           // capped lists (gs_config.list_cap): the tile lists were written only as far as the slot's history says they
                                             // are walked; gs_get_array(GS_ARR_SORTED_IDS / _KEYS) completes them and clears it
        const uint32_t *cap_src = nullptr;   // the history the caps of this frame come from (null: none)
        bool have_l2 = false;                // the frame has level-2 lists, built with ...
        GsBin3Args last_l2{};                // ... these arguments (read under have_l2 only: gs_get_array writes the capped rest with them)
        bool spec_lists = false;             // speculative binning: the lists of this frame were enqueued before the totals were known ...
        size_t spec_cap_coarse = 0, spec_cap_fine = 0;   // ... against these capacities (entries; read under spec_lists only)
        bool g2d_clean = false;              // the gradient rows are cleared (enqueued: by the small path's kernel, or by the fill workgroups of the frame's
                                             // forward): the frame's first composite backward needs no fill
        uint32_t *perm_ptr = nullptr;        // the frame's depth order (null: index order, or BinPlan::perm_on_demand and nobody has asked yet)
        void speculate(size_t cap_coarse, size_t cap_fine) { spec_lists = true; spec_cap_coarse = cap_coarse; spec_cap_fine = cap_fine; }
        bool speculation_held(size_t coarse, size_t fine) { spec_lists = false; return coarse <= spec_cap_coarse && fine <= spec_cap_fine; }   // the totals are here: over
        void relist_in_full() { cap_src = nullptr; frame_capped = false; have_l2 = false; }   // what two_level_lists(round 0) expects of its caller
        void rows_dirtied() { g2d_clean = false; }                                            // a composite backward is about to accumulate into them
    } live;
    // ---- the frame's bin plan: HOW gs_bin builds its lists.  Filled once per frame by plan_bin (gs_api_bin.hip), the one place that decides.  What later calls
    // change is live state (FrameLive, or a ctx member with a longer lifetime) and stays outside.
    struct BinPlan {
        enum class Path { TWO_LEVEL = 0, RADIX64 = 1, RADIX32 = 2, SMALL = 3 } path = Path::RADIX64;   // the values: what gs_get_bin_path reports
        int tile_bits = 0, gid_bits = 0, lo_bits = 0, hi_bits = 0;                        // bits of a tile index (low / high radix pass) and of a gaussian id
        int sbs = 3, sgx = 0, sgy = 0;       // two-level path: log2 of the super-tile edge in tiles (3, or 4 on 4K-class grids), super-tile grid
        int n_rounds = 1;                    // binning rounds of the frame (depth slabs, gs_config.slab_mode) ...
        int64_t slab_lo[GS_MAX_ROUNDS + 1] = {};   // ... round r covers the list positions [slab_lo[r], slab_lo[r+1]) of the depth order
        bool perm_on_demand = false;         // SMALL sorts nothing globally: the depth order (renderer.sortIdxs) is built when gs_get_array asks (perm_ptr null until then)
        int ns() const { return sgx * sgy; }
        bool radix() const { return path == Path::RADIX32 || path == Path::RADIX64; }
    } bin;
    // ---- the frame's plan: HOW its composite launches run.  Filled once per frame by plan_frame (gs_api_composite.hip), the one place that
    // decides; composite_args turns it into the arguments of every launch of the frame: forward rounds, backward, debug launches.
    struct FramePlan {
        int parts = 1;                       // waves per tile of the forward (pixel parts; gs_config.tile_parts, gs_get_tile_parts)
        int bwd_parts = 1;                   // ... and of the backward: the same, or (Snap::ALL) what still fits on top of the list segments
        const uint32_t *order = nullptr;     // launch order of the forward (null: tile order) ...
        const uint32_t *bwd_order = nullptr; // ... and of the backward: the same, or (a slot's first frame; no side stream) what build_frame_order made of this forward
        bool side = false;                   // the order kernel behind the forward runs on the side stream, for the slot's NEXT frame: bwd_order == order
        int front = 0;                       // lpt_front: entries of the orders' front region
        bool split = false;                  // launches over an order honour its split entries (heavy tiles run as several waves) while the lists are full
        // snapshots the forward leaves for list segments of the backward (GsCompositeArgs.snap)
        enum class Snap { NONE, HEAVY, ALL } snap = Snap::NONE;
        uint32_t *snap_walked = nullptr;     // HEAVY (the split tiles of `order`; seg_len sits behind its entries): this frame's parity slice of gs_ctx::snap_walked
        int seg_n = 0;                       // ALL (small grid): every tile, seg_n segments each ...
        const uint32_t *seg_hist = nullptr;  // ... their lengths from the walk of the slot's previous forward
        bool bwd_segments = false;           // the backward runs as list segments: the forward LEFT snapshots, and for the order the backward takes
    } plan;
    // ---- the backward's plan: WHAT one call of the backward family (gs_backward, _ex, _sgd, _adam) runs.  Filled once per call by plan_backward
    // (gs_api_composite.hip), the one place that decides and refuses -- it enqueues and allocates nothing; run_backward is its one consumer.
    struct BackwardPlan {
        bool composite = true;               // phases that run: the composite adjoint (dC -> the 2-D gradient sums g2d) ...
        int chain = 3;                       // ... and the per-gaussian kernels: bit 0 the SH kernel, bit 1 the geometry chain (0: none, GS_BWD_COMPOSITE_ONLY)
        // what the per-gaussian kernels do with a gradient float: add it to the target, store it, or step the target with it
        enum class Update { ACCUMULATE, OVERWRITE, SGD, ADAM_DENSE, ADAM_SELECTIVE } update = Update::ACCUMULATE;
        float lr = 0.0f; const GsAdamFused *adam = nullptr;   // SGD: target = fma(-lr, gradient, target); ADAM_*: the moments and the step's scalars
        bool fused() const { return update >= Update::SGD; }
        Five<float> target{};                // the caller's gs_grads, or (fused) the model's own arrays
        const float *dC = nullptr; bool stage_dC = false;   // dC is host memory: staged through stage_in ...
        bool host_sync = false;              // ... and GS_MEM_HOST calls return with the stream drained
        bool fill_g2d = false;               // the gradient rows need the in-line zero fill (nobody cleared them: g2d_clean)
        bool fill_shs = false;               // the composite launch carries the zero fill of d_shs: the SH kernel stores live rows only (shs_zeroed)
        bool model_changes() const { return fused(); }   // the frame falls back to nothing when the call succeeds
    };
    // ================ HISTORY: what a frame takes from the frames before it, each with ONE owner here: a view slot's launch order and its per-tile walk
    // (ViewSlot), the ctx's walked share (WalkFeedback), the order kernel's hand-off.  (The depth sort's feedback words keep their own rules: further down.)
    // ---- longest-first launch orders (gs_config.schedule 3 / 4).  After every forward ONE order kernel turns the frame's per-tile
    // work into a launch order: this frame's backward uses it, and so does the NEXT forward rendered under the same view slot.
    int view_slot = -1;                      // gs_set_view_slot: the slot of the frame being rendered (-1: none)
    // Index GS_MAX_VIEW_SLOTS = frames without a slot.  A slot owns two double buffers, each tagged with the grid (grid_key) it is valid for:
    struct ViewSlot {
        // launch orders: [sel] is the newest one; a frame that runs on it has its order kernel write the OTHER buffer (on the side stream,
        // while the frame's backward still reads [sel]), a frame without history writes [sel] itself
        DevBuf order[2]; int sel = 0;
        int64_t tiles = 0;                   // grid of order[sel] (0: no history)
        uint32_t *split_words = nullptr;     // coherent pinned host words, one per order buffer (gs_create): split tiles of that order, as its order
                                             // kernel counted them (0xFFFFFFFF: the kernel has not reported yet); null: unknown, assume some
        uint32_t *split_word(int buf) const { return split_words ? split_words + buf : nullptr; }
        int order_dst(bool in_use) const { return in_use ? sel ^ 1 : sel; }
        void order_written(int buf, int64_t grid) { sel = buf; tiles = grid; }          // order[buf] is the newest one now
        // per tile: list entries the slot's forwards walked (the next frame's list caps and segment lengths): [wsel] = the last completed
        // forward's, which the frame being rendered may still read while it writes its own into the other one
        DevBuf walkbuf[2]; int wsel = 0;
        int64_t walked_grid = 0;             // grid of walkbuf[wsel] (0: none yet)
        DevBuf &walk_dst() { return walkbuf[wsel ^ 1]; }
        void walk_written(int64_t grid) { wsel ^= 1; walked_grid = grid; }      // the frame's forward is enqueued: its walk is the slot's history now
        // what a frame on `grid` may READ of the slot, each null unless made on this grid: newest order, its split word, previous walk (the ONE tag compare)
        struct History { const uint32_t *order, *order_split, *walk; };
        History history(int64_t grid) const {
            const bool o = tiles == grid, w = walked_grid == grid;
            return {o ? order[sel].as<uint32_t>() : nullptr, o ? split_word(sel) : nullptr, w ? walkbuf[wsel].as<uint32_t>() : nullptr};
        }
    };
    std::vector<ViewSlot> slots;             // GS_MAX_VIEW_SLOTS + 1 (allocated at gs_create; device buffers on first use)
    uint32_t *pinned_split = nullptr;        // the slots' split words (ViewSlot::split_words): one pinned block, freed with the ctx
    // The slot of the frame being rendered, asked two ways.  STORAGE: where its order kernel writes -- never null: a slot-less frame's backward needs an order
    // too.  HISTORY: whose order and walk it may read, where its forward leaves its walk -- null for a slot-less frame unless schedule 4: nothing says two such
    // frames show one view, so under schedule 3 the last slot's order is storage no later frame reads, and the walk goes to feedback.own
    ViewSlot &storage_slot() { return slots[view_slot >= 0 ? view_slot : GS_MAX_VIEW_SLOTS]; }
    ViewSlot *history_slot() { return view_slot >= 0 || cfg.schedule == 4 ? &storage_slot() : nullptr; }
    // A launch order is built only when there are more tiles than wave slots (wave_slots: 256 CUs x 4 SIMDs x 5 on MI355X).  Below that the isolated
    // kernels do gain from it (C2, 2500 tiles: forward 68 -> 61 us, backward 145 -> 122 us, tools/xcd_order.py C2 -- in tile order the
    // heavy tiles of the image centre land on neighbouring SIMDs), but the frame does not: its forward is bound by cold gathers, not by
    // balance, and the order kernel is one more launch in a frame that is bound by launches (C2 0.382 -> 0.400 ms, C1 0.183 -> 0.205 ms
    // with it, same box; 0.393 / 0.197 with the kernel on the side stream).
    bool lpt_schedule() const { return (cfg.schedule == 3 || cfg.schedule == 4) && (ntiles() > wave_slots || (cfg.debug_flags & GS_DEBUG_ALWAYS_ORDER)); }
    // Heavy tiles (round 5): the launch orders reserve a front region for the extra parts of split tiles (tile_lpt_order_kernel) when the
    // ctx may use them at all: automatic tile_parts, the early-out on, and a grid on which the frame-wide 2 / 4 waves per tile cannot engage.
    // A property of the ctx and the grid, so every order of a slot has one layout; whether a LAUNCH honours the split entries is decided
    // per frame (plan_frame: FramePlan::split).
    int lpt_front() const { return (lpt_schedule() && cfg.tile_parts == 0 && cfg.t_min > 0.0f && 2 * ntiles() > wave_slots && ntiles() <= GS_LPT_MAX_TILES) ? GS_LPT_FRONT : 0; }
    int lpt_order_entries() const { return lpt_front() + gs_lpt_order_len(gx, gy); }   // = workgroups of a launch over the order
    // the words behind an order's entries: list entries per backward segment of the split tiles (GS_SEG_SLOTS of them)
    const uint32_t *order_seg_len(const uint32_t *order) const { return order + lpt_order_entries(); }
    int lpt_split_div() const { return wave_slots * 4 / 5; }      // a tile with more work than an even share of ~4 waves per SIMD is split
    // The side stream (order kernel beside the backward) costs four more runtime calls per frame: it pays when the composite kernels
    // are long, and costs when the frame is bound by the host's launch rate (config C2, together with the zero fill it once carried: + 9 %).
    bool use_side_stream() const { return n >= 262144 || (cfg.debug_flags & GS_DEBUG_ALWAYS_ORDER); }
    // ---- the ctx's walk feedback: the share of its list entries the last completed forward walked (slab rounds, capped lists).  The forward leaves per-tile
    // counts; the NEXT frame's binning sums them on their way to the host (previous_walk), where the sum meets its instance count (sum_arrived)
    struct WalkFeedback {
        DevBuf own;                          // per-tile walk of forwards without a history slot
        const uint32_t *walk = nullptr;      // per-tile walked counts of the most recent forward (a slot's array, or `own`) ...
        int64_t grid = 0, n_inst = 0;        // ... the grid (grid_key) it was written for, and the frame's instances
        bool sum_due = false;                // a forward has been enqueued whose walk no binning has sent to the host yet
        double ratio = -1.0; double walked_ratio() const { return ratio; }   // entries walked / instances of the last completed frame (-1: none yet)
        // binning a frame on grid g: the walk to sum for the host, or null (none due, or not of this grid: never sent)
        const uint32_t *previous_walk(int64_t g) { if (grid != g || !walk) sum_due = false; return sum_due ? walk : nullptr; }
        void forward_enqueued(int64_t inst, int64_t g, const uint32_t *dst) { n_inst = inst; grid = g; walk = dst; sum_due = true; }
        // the frame's totals are on the host; sum: the u64 previous_walk's kernel stored, read only when one was sent
        void sum_arrived(const uint32_t *sum) {
            if (sum_due && n_inst > 0) { unsigned long long w = 0; std::memcpy(&w, sum, sizeof(w)); ratio = (double)w / (double)n_inst; }
            sum_due = false;
        }
    } feedback;
    // ---- the order kernel's hand-off.  On the side stream the kernel (needed by the slot's NEXT frame, not by this one) runs beside the backward composite
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_order = nullptr;
    bool order_pending = false;              // an order kernel is in flight on the side stream (ev_order): await_order_kernel (gs_api_composite.hip)
    // heavy tiles, list segments of the backward: walked lengths of the forward's snapshots, two frame parities (the order kernel re-arms the NEXT frame's)
    struct SnapWalked {
        DevBuf buf; int parity = 0;
        void next_frame() { parity ^= 1; }   // (the order kernel behind the previous forward re-armed this parity)
        uint32_t *slice(int p) const { return buf.as<uint32_t>() + (size_t)p * GS_SEG_SLOTS; }
        uint32_t *of_frame() const { return slice(parity); }         // this frame's forward writes it, its backward reads it
        uint32_t *to_rearm() const { return slice(parity ^ 1); }
    } snap_walked;
    DevBuf snap;                             // the forward's snapshots (HEAVY: of the split tiles, ALL: of every tile)
    // ---- speculative binning: the lists are enqueued with the capacities of the buffers at hand while the frame's totals travel
    bool pending_totals = false;             // ev_count recorded, pinned totals not read yet (the speculation itself: FrameLive::spec_lists)
    int64_t n_coarse = 0;                    // coarse instances listed by the frame (two-level and small paths; 0 on the radix paths)
    DevBuf tile_dead;                        // slab frames: 4 lane masks per tile (frozen pixels between rounds)
    int dbg_win_start = 0, dbg_win_len = 0;  // gs_debug_set_window: the part of the launch order the debug launches cover (len 0: all)
    int rank_probe = -1;                     // lane-order probe of the LDS atomic rank: -1 not run, 0 passed, 1 failed (ballots forced)
    // ---- binning in depth slabs (BinPlan::n_rounds, slab_lo)
    int64_t round_gen[GS_MAX_ROUNDS] = {};   // generated instance positions of the round (>= the instances it lists)
    size_t round_ids_off[GS_MAX_ROUNDS] = {};// where the round's ids start inside `ids`
    DevBuf ranges_r[GS_MAX_ROUNDS];          // tile ranges of rounds 1.. (round 0 uses `ranges`)
    DevBuf tile_pos, tile_done, live2d, rect_r, offsets_r, live_total;
    // ---- two-level binning (gs_bin3.hip): lists per super-tile of 8 x 8 tiles, then per tile
    DevBuf rect_sorted, l1_table, l1_rows, l1_partials, cids, clr, cranges, segcnt, sdone, tilecnt;
    uint32_t *bin_totals() { return counters.as<CounterBlock>()->totals; }
    uint32_t *ext_count() { return &counters.as<CounterBlock>()->ext_count; }
    // ---- per-tile work counters of the composite launches (walked / evaluated list entries): counters[0..3] hold their sums only
    // after sum_work_counters() (gs_get_work_counters, the radix binning paths); the two-level path sums the walked counts of the
    // previous forward inside l1_rowscan on their way to the host.  The forward's walked counts: feedback.walk; the backward's:
    DevBuf tile_walked_b, tile_work_b;
    hipError_t ensure_bwd_counters() { const hipError_t e = tile_walked_b.ensure(sizeof(uint32_t) * ntiles1()); return e != hipSuccess ? e : tile_work_b.ensure(sizeof(uint32_t) * ntiles1()); }
    // ---- depth sort in two steps (gs_depth_sort_buckets; gs_config.depth_sort)
    DevBuf key_range;                        // two frame parities of the key-range accumulators the preprocess kernel fills
    int range_parity = 0;                    // parity of the frame being built
    bool range_valid = false;                // the 3-D preprocess of this frame filled key_range[range_parity]
    bool dsort_buckets_used = false;         // this frame's depth order came from the bucket path (its pinned stat word is live)
    int64_t dsort_classic_until = 0;         // frame id up to which the classic sort is used (an oversize bucket was reported)
    int dsort_stat_parity = 0;               // the parity gs_bin used for the bucket path's pinned stat word (gs_preprocess of the NEXT frame flips range_parity
                                             // before settle_totals of this one may run)
    uint32_t *dsort_stat() { return &pinned->dsort_stat[dsort_stat_parity & 1]; }
    // the bucket path is possible for the frame being built (same predicate in gs_preprocess, which then folds the key range, and in gs_bin)
    bool dsort_can_bucket() const {
        return cfg.depth_sort != 1 && (cfg.depth_sort == 2 || (n <= gs_depth_buckets_max_n() && frame_id > dsort_classic_until));
    }
    // ---- small frames (gs_bin_small.hip): the whole of gs_bin in one launch.  Same predicate in gs_preprocess (which then folds no key
    // range: nothing is sorted globally) and in gs_bin.  bin_path 0 only (3 = the two-level path whatever the size; tests, A/B)
    bool small_bin_possible() const {
        if (cfg.bin_path != 0 || cfg.depth_sort != 0 || cfg.list_cap == 2 || cfg.slab_fractions[0] > 0.0f) return false;
        if (cfg.debug_flags & (GS_DEBUG_WIDE_CURSORS | GS_DEBUG_SUPER8 | GS_DEBUG_SUPER16 | GS_DEBUG_TINY_CAPS)) return false;
        return gs_bin_small_supported(n, gx, gy);
    }
    // ---- the rows of 2-D gradient sums (g2d, feat_g2d): float, or fixed point in deterministic mode -- the ONE place that chooses.  A kernel takes a
    // buffer of them as a pair of pointers of which exactly one is set: const for the readers, mutable for the composite backward (GsCompositeArgs)
    template <typename F, typename L> struct RowsOf {
        F *g2d; L *g2d_fixed;
        template <typename A> void into(A &a) const { a.g2d = g2d; a.g2d_fixed = g2d_fixed; }   // the two members of an argument struct
    };
    using Rows = RowsOf<const float, const long long>; using RowsMut = RowsOf<float, long long>;
    RowsMut rows_mut(const DevBuf &b) const { return cfg.deterministic ? RowsMut{nullptr, b.as<long long>()} : RowsMut{b.as<float>(), nullptr}; }
    Rows rows(const DevBuf &b) const { const RowsMut m = rows_mut(b); return {m.g2d, m.g2d_fixed}; }
    size_t g2d_bytes() const { return (cfg.deterministic ? sizeof(long long) : sizeof(float)) * GS_G2D_STRIDE * n1(); }
    size_t shs_bytes() const { return sizeof(float) * width[4] * (size_t)(n > 0 ? n : 0); }   // the fifth gradient array: 3K x n floats
    bool fwd_fills_g2d = false;              // this frame's forward (round 0) carries the zero fill of g2d: decided once, in gs_forward
    bool tail_fill() const { return !(cfg.debug_flags & GS_DEBUG_NO_TAIL_FILL) && ntiles() > 0; }   // the composite launches may carry zero fills
    int fill_blocks_fwd = 0, fill_blocks_bwd = 0;   // fill workgroups the frame's last forward (round 0) / composite backward launch carried (gs_debug_tail_fill)
    float *bound_image = nullptr, *bound_trans = nullptr;   // gs_bind_outputs: caller-owned device buffers the forward writes directly
    float *img() { return bound_image ? bound_image : image.as<float>(); }
    float *tr() { return bound_trans ? bound_trans : trans.as<float>(); }
    int64_t frame_id = 0, ev_frame[GS_STAGE_COUNT] = {};   // a stage may run once per binning round: ev_cnt counts frames, not launches
    int64_t ev_counted[GS_STAGE_COUNT] = {};               // last frame whose pair of this stage was added to ev_cnt
    DevBuf grads_flat;                       // gs_grads_alloc
    DevBuf dpc;                              // 4 x n scratch between the two backward kernels
    DevBuf loss_maps, loss_acc, loss_in[2], loss_dc, view_cams;
    DevBuf touched_cnt, touched_off, touched_zero;   // touched-rows exchange: per (view, chunk) counts and exclusive row offsets; three +0 floats (gs_api_touched.hip)
    // ---- density control (gs_api_density.hip): per chunk of GS_CHUNK gaussians the counts of the three output classes (survivors,
    // clones, split sources), their exclusive offsets, and {three totals, bad-action flag}; the plan gs_density_plan leaves for gs_density_restructure
    DevBuf density_cnt, density_off, density_tot;
    struct DensityPlan {
        bool planned = false;                // dropped by inputs_changed()
        const int32_t *action = nullptr;     // the tag: the action array and n the offsets were made from
        int64_t n = 0, survivors = 0, clones = 0, splits = 0;
        int64_t n_out() const { return survivors + clones + 2 * splits; }
    } density;
    float density_log_shrink = 0.4700036292457356f;   // (float)log(1.6) until a gs_density_decide says otherwise: what the children of a split shrink by
    // ---- MCMC densification (gs_api_mcmc.hip): per chunk of GS_CHUNK gaussians {sum of the weights, dead count} and their exclusive offsets, the two
    // totals, the histogram of a relocation's sources (n int32), the binomial table (uploaded once); the plan gs_mcmc_plan leaves for gs_mcmc_relocate(dst = NULL)
    DevBuf mcmc_sum, mcmc_off, mcmc_tot, mcmc_hist, mcmc_binom;
    bool mcmc_binom_ready = false;
    struct McmcPlan {
        bool planned = false;                // dropped by inputs_changed()
        const int32_t *dead = nullptr;       // the caller's dead list, n and the number of entries the plan wrote
        int64_t n = 0, dead_count = 0;
    } mcmc;
    // ---- point-cloud initialisation (gs_api_knn.hip): scratch of its own, so that gs_knn_mean_dist2 is legal in the middle of a frame --
    // (key | index) pairs and the sort's table, the sorted points, box and super-box bounds, {bounding box, count of finite points}
    DevBuf knn_pairs_a, knn_pairs_b, knn_table, knn_digit_total, knn_sorted, knn_boxes, knn_supers, knn_stats;
    // ---- feature maps (gs_api_features.hip): the frame's composite launches over a SECOND payload whose three colour floats are the caller's.
    // Buffers of their own, so that the frame's image, transmittance, g2d and dpc stay what gs_forward / gs_backward left: the payload copy, the
    // transmittance of a render without trans_out, the auxiliary rows of 2-D gradient sums and the geometry chain's colour-path input, which
    // nothing ever writes but the zero fill behind its allocation (feat_dpc_zeroed: the capacity that fill covered)
    DevBuf feat_payload, feat_trans, feat_g2d, feat_dpc;
    size_t feat_dpc_zeroed = 0;
    // ---- camera gradient (gs_api_camera.hip): the staged 40 floats of a GS_MEM_HOST call, then one row of 40 doubles per workgroup of gs_camera_grad_kernel
    DevBuf camera_partials;
    // ---- evaluation metrics (gs_api_metrics.hip): the staged four sums of a GS_MEM_HOST call, then one row of four doubles per tile of
    // gs_metrics.hip's kernel; the staged images and weight, and the staged map, of a GS_MEM_HOST call.  Buffers of their own: the call is legal in
    // the middle of a frame and beside the loss
    DevBuf metrics_partials, metrics_in[3], metrics_map;
    // ---- per-view exposure (gs_api_exposure.hip): one row of 12 doubles per workgroup of exposure_bwd_kernel, as many as (W, H) says
    DevBuf exposure_partials;
    ncclComm_t comm = nullptr;
    int comm_ranks = 0;
};

// ---------------------------------------------------------------- shared helpers
inline int fail(gs_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}
inline int hipfail(gs_ctx *c, hipError_t e, const char *what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return fail(c, e == hipErrorOutOfMemory ? GS_ERR_OOM : GS_ERR_HIP, m);
}
#define HIPCHK(c, call)                                              \
    do {                                                             \
        hipError_t e__ = (call);                                     \
        if (e__ != hipSuccess) return hipfail((c), e__, #call);      \
    } while (0)

// ---- the refusals entry points share: GS_OK, or the code with "<who>: ..." left for gs_last_error (built only when the call is refused)
inline int need_3d(gs_ctx *c, const char *who) { return c->kind == 0 ? GS_OK : fail(c, GS_ERR_UNSUPPORTED, std::string(who) + ": 3-D renderer only"); }
inline int need_mem(gs_ctx *c, const char *who, int mem) { return mem == GS_MEM_HOST || mem == GS_MEM_DEVICE ? GS_OK : fail(c, GS_ERR_INVALID, std::string(who) + ": bad mem"); }
inline int need_image_size(gs_ctx *c, const char *who, int W, int H) {
    return W > 0 && H > 0 && W <= 32767 && H <= 32767 ? GS_OK : fail(c, GS_ERR_INVALID, std::string(who) + ": image size must be in 1..32767");
}
// the five arrays of the model are there (n == 0: nothing to have)
inline int need_model(gs_ctx *c, const char *who) {
    const Five<const float> m = c->model5();
    for (int i = 0; i < 5; ++i)
        if (c->n > 0 && !m[i]) return fail(c, GS_ERR_INVALID, std::string(who) + ": no model (gs_set_model first)");
    return GS_OK;
}
// the frame has come at least as far as s, else GS_ERR_INVALID with this message (whole: the calls word what they need in their own way)
inline int need_stage(gs_ctx *c, gs_ctx::Stage s, const char *msg) { return c->stage >= s ? GS_OK : fail(c, GS_ERR_INVALID, msg); }
// two byte ranges share a byte (an empty or null one shares none)
struct ByteRange { const void *p; size_t bytes; };
inline bool overlaps(const ByteRange &a, const ByteRange &b) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
    return a.p && b.p && a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}

// ---- the model head of an argument struct: n, the five arrays, the ACTIVE degree and, where the struct carries it, the stored row stride
template <typename A> auto model_head_stride(A &a, int stride, int) -> decltype((void)a.sh_stride) { a.sh_stride = stride; }
template <typename A> void model_head_stride(A &, int, long) {}
template <typename A> void model_head(const gs_ctx *c, A &a) {
    a.n = c->n; a.sh_degree = c->active_sh_degree(); model_head_stride(a, c->sh_row_floats(), 0);
    a.means = c->means; a.scales = c->scales; a.quats = c->quats; a.opac = c->opac; a.shs = c->shs;
}
// the per-gaussian chain behind a composite backward: the rows it reads, the colour path's scratch, the targets and what is done with a gradient float
inline GsPreprocessBwdArgs chain_args(const gs_ctx *c, gs_ctx::Rows rows, float *dpc, const Five<float> &target, int overwrite, int shs_zeroed, float sgd_scale) {
    GsPreprocessBwdArgs b{};
    model_head(c, b); rows.into(b);
    b.dpc = dpc; b.overwrite = overwrite; b.shs_zeroed = shs_zeroed; b.sgd_scale = sgd_scale;
    b.d_means = target[0]; b.d_scales = target[1]; b.d_quats = target[2]; b.d_opac = target[3]; b.d_shs = target[4];
    return b;
}

// One recorded pair of a stage -> the accumulators; false when the pair has not completed yet (it stays `fresh`).
inline bool harvest_stage(gs_ctx *c, int s) {
    if (!c->ev_fresh[s]) return true;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev[s][0], c->ev[s][1]) != hipSuccess) { (void)hipGetLastError(); return false; }
    c->ev_sum[s] += ms;
    if (c->ev_counted[s] != c->ev_frame[s]) { c->ev_counted[s] = c->ev_frame[s]; c->ev_cnt[s] += 1; }      // one count per frame
    c->ev_fresh[s] = false;
    return true;
}
struct StageTimer {
    gs_ctx *c; int st; bool on;
    StageTimer(gs_ctx *c_, int st_) : c(c_), st(st_), on(c_->cfg.profile_stages == 1 || c_->cfg.profile_stages == 2 + st_) {
        if (on) {
            if (c->ev_fresh[st] && !harvest_stage(c, st)) {            // about to re-record a pair nobody has read: wait for it (rare:
                (void)hipEventSynchronize(c->ev[st][1]);               // the host ran a whole frame ahead of the GPU)
                (void)harvest_stage(c, st);
            }
            c->ev_frame[st] = c->frame_id;
            (void)hipEventRecord(c->ev[st][0], c->stream);
        }
    }
    ~StageTimer() {
        if (on) { (void)hipEventRecord(c->ev[st][1], c->stream); c->ev_valid[st] = true; c->ev_fresh[st] = true; }
    }
};

// Fold every pair that has completed into the accumulators (pairs still in flight stay fresh for the next call).
inline void harvest_events(gs_ctx *c, int skip_stage = -1) {
    if (!c->cfg.profile_stages) return;
    for (int s = 0; s < GS_STAGE_COUNT; ++s)
        if (s != skip_stage) (void)harvest_stage(c, s);
}

inline int bind_device(gs_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    return GS_OK;
}

inline uint32_t *key_range_of(const gs_ctx *c, int parity) { return c->key_range.as<uint32_t>() + (size_t)parity * gs_depth_range_parity_words(); }   // one frame parity's accumulators

// ---------------------------------------------------------------- across the translation units
// gs_api_bin.hip
int settle_totals(gs_ctx *c, bool *redo, bool may_relist);
int bin_round(gs_ctx *c, int r);
int depth_order(gs_ctx *c);                   // the frame's depth order -> c->perm, c->live.perm_ptr
int blend_background(gs_ctx *c);              // gs_api_composite.hip: image += T bg over the frame's image, on the stream (no launch over black)
// gs_api_composite.hip: the arguments of a composite launch of the frame, as its plan says (round r of the forward / the backward; debug: an isolated launch)
GsCompositeArgs composite_args(gs_ctx *c, bool bwd, int r, bool debug = false);
