// gs_api_composite.hip -- gs_forward / gs_backward (reference src/forward.jl:163-198, src/backward.jl:3-38): the frame's plan, the
// composite launches, the per-gaussian chain behind the backward, and the longest-first launch orders kept per view slot.
#include "gs_ctx.h"

using Snap = gs_ctx::FramePlan::Snap;
using Stage = gs_ctx::Stage;
using BackwardPlan = gs_ctx::BackwardPlan;
using Update = BackwardPlan::Update;

using History = gs_ctx::ViewSlot::History;

// the frame's launches run over a launch order (gs_config.schedule 3 / 4; the order kernel refuses grids beyond 8K-class images)
static bool frame_has_orders(const gs_ctx *c) { return c->lpt_schedule() && c->ntiles() > 0 && c->ntiles() <= GS_LPT_MAX_TILES; }
// Launch order of the frame's forward: what the last forward under the same view slot measured, else (schedule 4) what this ctx's previous
// slot-less forward measured (h: the history slot's, gs_forward); null = no history: tile order.  A lookup: await_order_kernel comes first.
static const uint32_t *forward_order(const gs_ctx *c, const History &h) { return frame_has_orders(c) ? h.order : nullptr; }
// the main stream waits for the order kernel in flight, if any (long complete by now; an event wait on the stream costs nothing)
static int await_order_kernel(gs_ctx *c) {
    if (c->order_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_order, 0)); c->order_pending = false; }
    return GS_OK;
}

// pixel parts (waves per tile, each owning 4 / parts of its pixel strips) that fit the wave slots when a tile runs as `units` waves already
static int parts_that_fit(const gs_ctx *c, int units) {
    const long long w = (long long)units * c->ntiles();
    return 4 * w <= c->wave_slots ? 4 : 2 * w <= c->wave_slots ? 2 : 1;
}

// In which mode do this frame's composite launches run, and why: decided HERE, once per frame, from the config, the grid, the lists as
// gs_bin left them, the forward's launch order and the walk history of the view slot (null: none on this grid).  Beside it: lpt_schedule
// and lpt_front (gs_ctx.h), which are properties of ctx and grid -- they fix the layout of every order of a slot.
static void plan_frame(gs_ctx *c, const History &h) {
    gs_ctx::FramePlan p;
    const uint32_t *const order = forward_order(c, h), *const hist = h.walk;
    const int want = c->cfg.tile_parts;
    // launches that composite whole tiles, one wave each: no early-out, slab rounds, capped lists
    const bool whole = !(c->cfg.t_min > 0.0f) || c->bin.n_rounds > 1 || c->live.frame_capped;
    p.parts = p.bwd_parts = want == 1 || whole ? 1 : (want == 2 || want == 4) ? want : parts_that_fit(c, 1);
    p.order = p.bwd_order = order;
    // The backward runs in the forward's order while the order kernel works beside it, on the side stream, for the slot's next frame; else
    // (a slot's first frame; no side stream) it waits for that kernel and takes the fresh order: build_frame_order then sets bwd_order
    p.side = order && c->use_side_stream();
    p.front = c->lpt_front();
    p.split = p.front > 0 && p.parts == 1 && c->bin.n_rounds == 1;            // heavy tiles run as the orders' split entries say (full lists: asked at every launch, frame_capped is live)
    // neither snapshot mode looks at cfg.deterministic, so deterministic gradients depend on the slot's history
    const bool may_split = !h.order_split || *h.order_split != 0u;        // (the order kernel's count; 0xFFFFFFFF: not reported yet)
    if (order && p.split && c->snap_walked.buf.p && may_split) {
        p.snap = Snap::HEAVY;                                              // ... and leave snapshots for the list segments of their backward
        p.snap_walked = c->snap_walked.of_frame();
    } else if (hist && want == 0 && p.parts > 1 && !c->lpt_schedule() && c->kind == 0 && c->ntiles() > 0) {
        // small grids (the automatic choice gave pixel parts: full lists, one round, at most half as many tiles as wave slots; no launch order):
        // with the slot's previous walk at hand EVERY tile's backward runs as list segments instead, the forward's waves leave the
        // snapshots.  Two segments, and as many pixel parts on top as still fit the wave slots (C1: 4 x 2 waves per tile; C2: 1 x 2)
        // (C1, lists of two or three batches: four segments instead of four pixel parts lost, 0.049 against 0.034 ms; three segments x four
        // parts ran like two, 0.0239 against 0.0243 -- a lone wave needs 0.33 us per evaluated entry and the launch lasts as long as the
        // batch with the most of them, which no cut at a batch boundary shortens)
        p.snap = Snap::ALL;
        p.seg_n = 2; p.seg_hist = hist;
        p.bwd_parts = parts_that_fit(c, p.seg_n);
    }
    c->plan = p;
}

// The arguments of a composite launch of the frame, as its plan says: round r of the forward, or the backward (every round's lists).
// The callers add what is theirs alone -- forward: per-tile counters, slab state, bw_*; backward: dC, its counters; debug: variant, clocks,
// window.  debug = an isolated launch over the finished frame: the forward then runs in the BACKWARD's order (what the slot's next forward
// will use), leaves no snapshots, and keeps its hands off the per-tile counters.
GsCompositeArgs composite_args(gs_ctx *c, bool bwd, int r, bool debug) {
    const gs_ctx::FramePlan &p = c->plan;
    GsCompositeArgs a{};
    a.W = c->cam.W; a.H = c->cam.H; a.gx = c->gx; a.gy = c->gy; a.t_min = c->cfg.t_min;
    a.payload = c->payload.as<GsPayload>(); a.image = c->img(); a.trans = c->tr();
    a.cull = c->cfg.alpha_cull != 0;
    for (int q = 0; q < c->bin.n_rounds; ++q) {                                // the lists, round by round (a round that listed nothing: skipped)
        if (q > 0 && c->round_gen[q] == 0) continue;
        a.seg_ranges[a.nseg] = q == 0 ? c->ranges.as<uint32_t>() : c->ranges_r[q].as<uint32_t>();
        a.seg_ids[a.nseg] = c->ids.as<uint32_t>() + c->round_ids_off[q];
        ++a.nseg;
    }
    a.ranges = r == 0 ? c->ranges.as<uint32_t>() : c->ranges_r[r].as<uint32_t>(); a.ids = c->ids.as<uint32_t>() + c->round_ids_off[r];
    if (bwd) c->rows_mut(c->g2d).into(a);
    a.tile_order = bwd || debug ? p.bwd_order : p.order; a.order_len = a.tile_order ? c->lpt_order_entries() : 0;
    a.parts = bwd ? p.bwd_parts : p.parts;
    a.split_ok = a.tile_order && p.split && !c->live.frame_capped;
    if (c->live.frame_capped && c->bin.n_rounds == 1) {
        a.tile_ext = c->tile_ext.as<uint2>();                              // the lists end where gs_bin / the forward stopped writing them
        if (!bwd) {                                                        // the forward's wave extends its tile's list when it must
            a.cranges = c->cranges.as<uint32_t>(); a.cids = c->cids.as<uint32_t>(); a.clr = c->clr.as<uint16_t>();
            a.ids_w = c->ids.as<uint32_t>(); a.sgx = c->bin.sgx; a.sbs = c->bin.sbs; a.ext_count = c->ext_count();
        }
    }
    if (bwd ? p.bwd_segments : !debug) {                                   // snapshots: the forward leaves them, the backward starts its list segments from them
        if (p.snap == Snap::ALL) { a.snap = c->snap.as<float>(); a.seg_hist = p.seg_hist; a.seg_n = p.seg_n; }
        if (p.snap == Snap::HEAVY && a.split_ok) {
            a.snap = c->snap.as<float>(); a.seg_len = c->order_seg_len(a.tile_order); a.front = p.front; a.snap_walked = p.snap_walked;
        }
    }
    return a;
}

// After the frame's (last) forward: ONE order kernel turns its per-tile work into a launch order.  When the forward already ran
// on the slot's history, the backward uses the same order and the kernel runs on the SIDE stream, beside the backward, into the
// slot's other buffer -- for the slot's next frame; nothing of this frame waits for it.  Without history (a slot's first frame)
// the backward waits for it: it is its only source of a longest-first order.
static int build_frame_order(gs_ctx *c) {
    gs_ctx::FramePlan &p = c->plan;
    if (!frame_has_orders(c)) return GS_OK;
    gs_ctx::ViewSlot &vs = c->storage_slot();
    const int dst = vs.order_dst(p.order != nullptr);
    DevBuf &ob = vs.order[dst];
    HIPCHK(c, ob.ensure(sizeof(uint32_t) * ((size_t)c->lpt_order_entries() + GS_SEG_SLOTS + 16)));
    // heavy tiles: the order kernel also sizes the backward's list segments (from what this forward walked) and re-arms the walked
    // lengths of the NEXT frame's snapshots (this frame's are being read by its backward)
    const uint32_t *walked = p.front > 0 ? c->feedback.walk : nullptr;
    uint32_t *rearm = nullptr, *nsplit = vs.split_word(dst);
    if (nsplit) *nsplit = 0xFFFFFFFFu;                                     // unknown until the order kernel has stored its count
    if (p.front > 0) {
        if (!c->snap_walked.buf.p) {
            HIPCHK(c, c->snap_walked.buf.ensure(sizeof(uint32_t) * 2 * GS_SEG_SLOTS));
            HIPCHK(c, hipMemsetAsync(c->snap_walked.buf.p, 0, sizeof(uint32_t) * 2 * GS_SEG_SLOTS, c->stream));
        }
        rearm = c->snap_walked.to_rearm();
    }
    if (int rc = await_order_kernel(c)) return rc;                         // (never two in flight; gs_forward has waited already)
    if (p.side) {
        HIPCHK(c, hipEventRecord(c->ev_main, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
    }
    HIPCHK(c, gs_launch_tile_lpt_order(c->tile_work.as<uint32_t>(), 0, c->gx, c->gy, ob.as<uint32_t>(), p.side ? c->side : c->stream, nullptr, 0, p.front,
                                       c->lpt_split_div(), walked, rearm, nsplit));
    if (p.side) {
        HIPCHK(c, hipEventRecord(c->ev_order, c->side));
        c->order_pending = true;
        vs.order_written(dst, c->grid_key());
        // (tile_work is rewritten by the next forward of this ctx: it waits for ev_order first, await_order_kernel in gs_forward)
    } else {
        p.bwd_order = ob.as<uint32_t>();
        // with p.order (no side stream) the fresh order sits in order[dst] but sel is not flipped: the slot's forwards keep the old one
        // (the single place a slot's order is written: a fix flips here, order_written(dst, ...))
        vs.order_written(vs.sel, c->grid_key());
    }
    return GS_OK;
}

// The background, blended into the image the frame's forward left: image = C + T bg, in place (gs_background.hip).  Everything that reads the
// image afterwards -- the copy-out, the loss, the composite backward's seed S = image . dC, whole tiles, strips, list segments and the fused
// backwards alike -- finds the blended one.  Over black nothing is launched.
int blend_background(gs_ctx *c) {
    if (!c->has_background()) return GS_OK;
    HIPCHK(c, gs_launch_blend_background(c->img(), c->tr(), c->pixels(), c->background, c->stream));
    return GS_OK;
}

extern "C" {

int gs_bind_outputs(gs_ctx *c, float *image, float *transmittance) {
    if (!c) return GS_ERR_INVALID;
    if ((image == nullptr) != (transmittance == nullptr)) return fail(c, GS_ERR_INVALID, "gs_bind_outputs: bind both buffers or neither");
    c->bound_image = image; c->bound_trans = transmittance;
    c->fall_back(Stage::BINNED);                                          // the forward's result lives in the buffers bound at its time
    return GS_OK;
}

int gs_set_view_slot(gs_ctx *c, int32_t slot) {
    if (!c) return GS_ERR_INVALID;
    if (slot >= GS_MAX_VIEW_SLOTS) return fail(c, GS_ERR_INVALID, "gs_set_view_slot: slot must be below GS_MAX_VIEW_SLOTS (or negative: none)");
    c->view_slot = slot < 0 ? -1 : (int)slot;
    return GS_OK;
}

// the composite launch of round r of the frame (r = 0 unless the frame is binned in depth slabs)
static int enqueue_forward_round(gs_ctx *c, int r, uint32_t *walk_dst) {        // walk_dst: where the frame's per-tile walk goes
    gs_ctx::FramePlan &p = c->plan;
    if (p.snap != Snap::NONE && !c->live.frame_capped) {                         // this launch leaves snapshots (composite_args)
        HIPCHK(c, c->snap.ensure(sizeof(float) * (p.snap == Snap::ALL ? (size_t)c->ntiles() * (size_t)(p.seg_n - 1) * 4 * 256 : (size_t)GS_SEG_SLOTS * GS_SEG_SNAP_FLOATS)));
        HIPCHK(c, c->ensure_bwd_counters());
    }
    GsCompositeArgs a = composite_args(c, false, r);
    a.resume = r > 0; a.final_round = r == c->bin.n_rounds - 1;
    a.tile_work = c->tile_work.as<uint32_t>(); a.tile_walked = walk_dst;
    p.bwd_segments = a.snap && (p.side || !p.order);                       // snapshots left, and (HEAVY) the backward takes the order they belong to
    if (a.snap) { a.bw_walked = c->tile_walked_b.as<uint32_t>(); a.bw_work = c->tile_work_b.as<uint32_t>(); }   // (its waves zero the segmented tiles' words)
    if (c->bin.n_rounds > 1) { a.tile_pos = c->tile_pos.as<uint32_t>(); a.tile_done = c->tile_done.as<uint8_t>(); a.tile_dead = c->tile_dead.as<unsigned long long>(); }
    if (r == 0 && c->fwd_fills_g2d) {                                      // the zero fill of the gradient rows, at the end of this launch's grid (gs_forward)
        a.fill_dst = c->g2d.p; a.fill_bytes = c->g2d_bytes(); a.fill_blocks = gs_composite_fill_blocks(a.fill_dst, a.fill_bytes);
    }
    StageTimer t(c, GS_STAGE_COMPOSITE_FWD);                               // the kernel alone ...
    HIPCHK(c, gs_launch_composite_fwd(a, c->stream));
    // ... and, behind the frame's last round, the background: inside the same pair of events, in front of the order kernel and the copy-out.  A
    // round 0 that gs_forward enqueues again (settle_totals rebuilt the lists) rewrites every pixel and is blended again
    if (a.final_round) { if (int rc = blend_background(c)) return rc; }
    if (r == 0) c->fill_blocks_fwd = a.fill_blocks;
    return GS_OK;
}

int gs_forward(gs_ctx *c, float *image, float *transmittance, int mem) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, Stage::BINNED, "gs_forward: gs_bin first")) return rc;
    if (const int rc = need_mem(c, "gs_forward", mem)) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t px = c->pixels(), ntiles = (size_t)c->ntiles(), nt1 = c->ntiles1();
    if (!c->bound_image) {
        HIPCHK(c, c->image.ensure(sizeof(float) * 3 * px));
        HIPCHK(c, c->trans.ensure(sizeof(float) * px));
    }
    HIPCHK(c, c->counters.ensure(GS_COUNTER_BYTES));
    HIPCHK(c, c->tile_work.ensure(sizeof(uint32_t) * nt1));
    // the per-tile walked counts go to the frame's history slot (its next frame's list caps and segment lengths), else to the ctx's own array
    const int64_t grid = c->grid_key();
    gs_ctx::ViewSlot *const vs = c->history_slot();
    DevBuf &walk_buf = vs ? vs->walk_dst() : c->feedback.own;
    HIPCHK(c, walk_buf.ensure(sizeof(uint32_t) * nt1));
    uint32_t *const walk_dst = walk_buf.as<uint32_t>();
    const int R = c->bin.n_rounds;
    if (R > 1) {
        HIPCHK(c, c->tile_pos.ensure(sizeof(uint32_t) * nt1));
        HIPCHK(c, c->tile_done.ensure(nt1));
        HIPCHK(c, c->tile_dead.ensure(sizeof(unsigned long long) * 4 * nt1));
        HIPCHK(c, hipMemsetAsync(c->tile_pos.p, 0, sizeof(uint32_t) * ntiles, c->stream));
    }
    c->snap_walked.next_frame();
    if (int rc = await_order_kernel(c)) return rc;                         // the order kernel in flight writes the slot's order and reads tile_work
    plan_frame(c, vs ? vs->history(grid) : History{});                     // the slot's newest order and previous walk, as far as they are of this grid
    // The zero fill of the 2-D gradient rows (64 B per gaussian) rides at the END of the forward's grid (round 0): workgroups appended behind
    // the tiles', which the dispatcher hands out last, into the launch's ragged end -- no fill command and no kernel boundary in front of the
    // composite backward.  Plain stores: the backward's atomics must find the rows where the in-line fill leaves them.
    // Why the rows may be cleared HERE: nothing reads a frame's g2d after the next gs_forward of the ctx.  Its readers are the composite
    // backward and the per-gaussian kernels of gs_backward (both renderers), gs_color_grads_pack and gs_get_array(GS_ARR_GRAD2D); all of
    // them ask for Stage::COMPOSITE_ADJOINT, which this call takes back below (reach(RENDERED); gs_bin, gs_preprocess and gs_bind_outputs
    // fall back further), and all of them run on c->stream, in front of this launch.  Only when the buffer stands as the coming backward
    // will want it (same n, same mode: DevBuf never shrinks, so its ensure() will not move it) and is not clean already; a ctx's first
    // frame, a ctx that only renders and a model that grew keep the fill command in run_backward.
    c->fwd_fills_g2d = c->tail_fill() && !c->live.g2d_clean && c->g2d.p && c->g2d.cap >= c->g2d_bytes() &&
                       gs_composite_fill_blocks(c->g2d.p, c->g2d_bytes()) > 0;
    for (int r = 0; r < R; ++r) {
        if (r > 0) { if (int rc = bin_round(c, r)) return rc; }
        if (int rc = enqueue_forward_round(c, r, walk_dst)) return rc;
        if (r == 0) {
            // the frame's totals: by now the composite is enqueued behind the lists, so the GPU has work while the host looks
            bool redo = false;
            if (int rc = settle_totals(c, &redo, true)) return rc;
            if (redo) { if (int rc = enqueue_forward_round(c, 0, walk_dst)) return rc; }     // the lists outgrew a buffer and were rebuilt: composite again, same plan
        }
    }
    if (c->fwd_fills_g2d) c->live.g2d_clean = true;                             // (a forward enqueued again after settle_totals filled again: idempotent)
    if (vs) vs->walk_written(grid);
    c->feedback.forward_enqueued(c->n_inst, grid, walk_dst);               // (n_inst: settled behind round 0)
    if (int rc = build_frame_order(c)) return rc;
    const hipMemcpyKind kind = mem == GS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (image && image != c->img()) HIPCHK(c, hipMemcpyAsync(image, c->img(), sizeof(float) * 3 * px, kind, c->stream));
    if (transmittance && transmittance != c->tr()) HIPCHK(c, hipMemcpyAsync(transmittance, c->tr(), sizeof(float) * px, kind, c->stream));
    if (mem == GS_MEM_HOST && (image || transmittance)) HIPCHK(c, hipStreamSynchronize(c->stream));
    c->reach(Stage::RENDERED);
    return GS_OK;
}

// What this call of the backward family runs: decided HERE, once, from the flags, the update its entry point names in `p` (none: by
// GS_BWD_OVERWRITE), the renderer and how far the frame has come.  Every refusal of the family is made here, and nothing is enqueued or
// allocated: a refused call leaves the frame and every buffer as they were.  grads null with a fused update: the targets are the model.
static int plan_backward(gs_ctx *c, const float *dC, int mem, const gs_grads *grads, int flags, BackwardPlan &p) {
    if (!c) return GS_ERR_INVALID;
    if (p.fused()) { if (const int rc = need_3d(c, p.update == Update::SGD ? "gs_backward_sgd" : "gs_backward_adam")) return rc; }
    if (const int rc = need_stage(c, Stage::RENDERED, "gs_backward: gs_forward first")) return rc;
    const bool params_only = (flags & GS_BWD_PARAMS_ONLY) != 0, composite_only = (flags & GS_BWD_COMPOSITE_ONLY) != 0;
    if (params_only && composite_only) return fail(c, GS_ERR_INVALID, "gs_backward: COMPOSITE_ONLY and PARAMS_ONLY exclude each other");
    const int chain = (flags & (GS_BWD_PARAMS_SH | GS_BWD_PARAMS_GEOM)) >> 3;             // bit 0: SH kernel, bit 1: geometry chain; 0 = both
    if (chain && !params_only) return fail(c, GS_ERR_INVALID, "gs_backward: GS_BWD_PARAMS_SH / _GEOM need GS_BWD_PARAMS_ONLY");
    if (chain) { if (const int rc = need_3d(c, "gs_backward: GS_BWD_PARAMS_SH / _GEOM")) return rc; }
    if (params_only) { if (const int rc = need_stage(c, Stage::COMPOSITE_ADJOINT, "gs_backward: GS_BWD_PARAMS_ONLY needs a GS_BWD_COMPOSITE_ONLY call on this frame")) return rc; }
    if ((!dC && !params_only) || (!grads && !p.fused() && !composite_only)) return fail(c, GS_ERR_INVALID, "gs_backward: NULL argument");
    if (const int rc = need_mem(c, "gs_backward", mem)) return rc;
    p.composite = !params_only;
    p.chain = composite_only ? 0 : chain ? chain : 3;
    if (!p.fused() && (flags & GS_BWD_OVERWRITE)) p.update = Update::OVERWRITE;
    if (p.fused()) p.target = c->model5_mut(); else if (grads) p.target = five(*grads);
    p.dC = dC;
    p.stage_dC = mem == GS_MEM_HOST && p.composite;
    p.host_sync = mem == GS_MEM_HOST;
    p.fill_g2d = p.composite && !c->live.g2d_clean;                             // (the fill command itself, and why it is in line: run_backward)
    // An overwriting backward of the 3-D renderer, both phases in this call, no fused optimiser: the zeros of the SH gradient rows no pixel
    // touched (63 % of the gaussians at C3, 90 % at C5; 192 B each at degree 3) depend on nothing -- the fill workgroups at the end of the
    // composite backward's grid zero ALL of d_shs, and gs_sh_bwd_kernel then stores the live rows only.  Past the caches, like that kernel's
    // own stores (GS_NT_STORES): the model's SH rows stay in the infinity cache for the next preprocess.  Split phases, GS_BWD_PARAMS_SH /
    // _GEOM, the fused optimisers and accumulating views keep the kernel's own zeros.
    p.fill_shs = c->tail_fill() && p.composite && p.chain == 3 && c->kind == 0 && p.update == Update::OVERWRITE &&
                 gs_composite_fill_blocks(p.target[4], c->shs_bytes()) > 0;
    return GS_OK;
}

// The plan, enqueued: staging copy, the composite adjoint with what is the backward's alone, the per-gaussian kernels, the host's wait.
static int run_backward(gs_ctx *c, const BackwardPlan &p) {
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t px = c->pixels();
    const float *dC_dev = p.dC;
    if (p.stage_dC) {
        HIPCHK(c, c->stage_in.ensure(sizeof(float) * 3 * px));
        HIPCHK(c, hipMemcpyAsync(c->stage_in.p, p.dC, sizeof(float) * 3 * px, hipMemcpyHostToDevice, c->stream));
        dC_dev = c->stage_in.as<float>();
    }
    HIPCHK(c, c->g2d.ensure(c->g2d_bytes()));
    HIPCHK(c, c->ensure_bwd_counters());
    if (p.composite) {
        GsCompositeArgs a = composite_args(c, true, 0);                    // order, parts, list segments: as the frame's plan says
        a.dC = c->last_dC = dC_dev;
        // the segments of a tile ADD to these words, which only the frame's forward zeroed: a second backward launch of the frame inflates them
        a.tile_walked = c->tile_walked_b.as<uint32_t>(); a.tile_work = c->tile_work_b.as<uint32_t>();
        if (p.fill_shs) { a.fill_dst = p.target[4]; a.fill_bytes = c->shs_bytes(); a.fill_blocks = gs_composite_fill_blocks(a.fill_dst, a.fill_bytes); a.fill_nt = 1; }
        // zero fill of the gradient rows (64 B per gaussian), in line: on a side stream beside the forward composite it cost more than
        // it hid (C3, same box, interleaved: 1.433 ms with the fill beside the forward, 1.412 ms in line -- its workgroups take wave slots
        // from the forward's tiles, and the two event hand-shakes per frame delay the depth sort's launches)
        // (a fill with streaming stores, which would spare the caches 64 B per gaussian, was measured: the atomics of the composite backward then
        // find their rows in memory instead of the cache, C3 + 1 %; profiles/r04t_ab_nontemporal.log)
        // (a small frame's gs_bin kernel has cleared them already: gs_bin_small.hip)
        // (... and otherwise the fill workgroups of the frame's forward: gs_forward)
        if (p.fill_g2d) HIPCHK(c, hipMemsetAsync(c->g2d.p, 0, c->g2d_bytes(), c->stream));
        c->live.rows_dirtied();
        {
            StageTimer t(c, GS_STAGE_COMPOSITE_BWD);                       // the kernel alone (what rocprof reports for it)
            HIPCHK(c, gs_launch_composite_bwd(a, c->stream));
        }
        c->fill_blocks_bwd = a.fill_blocks;
    }
    const int overwrite = p.update == Update::ACCUMULATE || p.update == Update::SGD ? 0 : 1;   // the fused Adam IS the overwriting backward, stepping instead of storing
    if (p.chain && c->kind == 1) {                       // SplatGrads2D, splat.jl:28-34
        GsPreprocess2DBwdArgs b2{};
        b2.n = c->n; b2.W = c->cam.W; b2.H = c->cam.H;
        b2.scales = c->scales; b2.rots = c->quats; b2.opac = c->opac;
        c->rows(c->g2d).into(b2); b2.overwrite = overwrite;
        b2.d_means = p.target[0]; b2.d_scales = p.target[1]; b2.d_rots = p.target[2]; b2.d_opac = p.target[3]; b2.d_colors = p.target[4];
        StageTimer t(c, GS_STAGE_PREPROCESS_BWD);
        HIPCHK(c, gs_launch_preprocess2d_bwd(b2, c->stream));
    } else if (p.chain) {
        HIPCHK(c, c->dpc.ensure(sizeof(float) * 4 * c->n1()));
        const GsPreprocessBwdArgs b = chain_args(c, c->rows(c->g2d), c->dpc.as<float>(), p.target, overwrite, p.fill_shs ? 1 : 0,
                                                 p.update == Update::SGD ? -p.lr : 0.0f);   // with the model as target this IS the SGD step
        const GsPreprocessBwdMode mode{p.chain, p.adam, p.update == Update::ADAM_DENSE ? 1 : p.update == Update::ADAM_SELECTIVE ? 2 : 0};
        StageTimer t(c, GS_STAGE_PREPROCESS_BWD);
        HIPCHK(c, gs_launch_preprocess_bwd(b, c->cam, c->stream, mode));
    }
    if (p.host_sync) HIPCHK(c, hipStreamSynchronize(c->stream));           // the host's dC buffer is no longer needed
    if (p.model_changes()) c->inputs_changed();
    else c->reach(p.chain ? Stage::BACKWARD : Stage::COMPOSITE_ADJOINT);
    return GS_OK;
}

int gs_backward(gs_ctx *c, const float *dC, int mem, const gs_grads *grads) { return gs_backward_ex(c, dC, mem, grads, 0); }

int gs_backward_ex(gs_ctx *c, const float *dC, int mem, const gs_grads *grads, int flags) {
    BackwardPlan p;
    if (const int rc = plan_backward(c, dC, mem, grads, flags, p)) return rc;
    return run_backward(c, p);
}

// backward + SGD in one pass: the per-gaussian kernels apply param = fma(-lr, gradient, param) to the resident model instead
// of storing the gradient (the same fma gs_sgd_step applies to the stored float): one read-modify-write of the parameters
// instead of gradient write + gradient read + parameter read-modify-write.  Single-view steps only (nothing is accumulated).
int gs_backward_sgd(gs_ctx *c, const float *dC, int mem, float lr) {
    if (!c) return GS_ERR_INVALID;
    if (!(lr != 0.0f)) return fail(c, GS_ERR_INVALID, "gs_backward_sgd: lr must be non-zero");
    BackwardPlan p;
    p.update = Update::SGD; p.lr = lr;
    if (const int rc = plan_backward(c, dC, mem, nullptr, 0, p)) return rc;
    return run_backward(c, p);
}

// backward + Adam in one pass (gs_sh_bwd_kernel<.., ADAM>): the OVERWRITE backward whose per-gaussian kernel steps p, m and v with each
// gradient float instead of storing it -- bit-identical to gs_backward_ex(GS_BWD_OVERWRITE) + gs_adam_step, without the gradient's store
// and re-read.
int gs_backward_adam(gs_ctx *c, const float *dC, int mem, const gs_grads *exp_avg, const gs_grads *exp_avg_sq, const float lr[GS_ADAM_GROUPS],
                     float beta1, float beta2, float eps, int64_t step, int flags) {
    if (!c) return GS_ERR_INVALID;
    if (!dC || !exp_avg || !exp_avg_sq) return fail(c, GS_ERR_INVALID, "gs_backward_adam: NULL argument");
    GsAdamFused ad{};
    const Five<float> m = five(*exp_avg), v = five(*exp_avg_sq);
    for (int i = 0; i < 5; ++i) {
        if (!m[i] || !v[i]) return fail(c, GS_ERR_INVALID, "gs_backward_adam: all ten moment arrays must be non-NULL");
        ad.m[i] = m[i]; ad.v[i] = v[i];
    }
    if (const int rc = gs_adam_prepare(c, "gs_backward_adam", c->model5().p, nullptr, m.p, v.p, lr, beta1, beta2, eps, step, flags, &ad.h)) return rc;
    BackwardPlan p;
    p.update = (flags & GS_ADAM_SELECTIVE) ? Update::ADAM_SELECTIVE : Update::ADAM_DENSE; p.adam = &ad;
    if (const int rc = plan_backward(c, dC, mem, nullptr, 0, p)) return rc;
    return run_backward(c, p);
}

int gs_color_grads_pack(gs_ctx *c, float *drgb) {
    if (!c || !drgb) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_color_grads_pack")) return rc;
    if (const int rc = need_stage(c, Stage::COMPOSITE_ADJOINT, "gs_color_grads_pack: gs_backward first")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const gs_ctx::Rows rows = c->rows(c->g2d);
    HIPCHK(c, gs_launch_pack_drgb(rows.g2d, rows.g2d_fixed, drgb, c->n, c->stream));
    return GS_OK;
}

int gs_sh_grads_from_views(gs_ctx *c, int32_t nviews, const float *cams, const float *drgb, float *d_shs, int flags) {
    if (!c || !cams || !drgb || !d_shs || nviews <= 0) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_sh_grads_from_views")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const size_t bytes = sizeof(float) * GS_VIEW_RECORD_FLOATS * (size_t)nviews;
    HIPCHK(c, c->view_cams.ensure(bytes));
    HIPCHK(c, hipMemcpyAsync(c->view_cams.p, cams, bytes, hipMemcpyHostToDevice, c->stream));   // pageable source: staged before return
    HIPCHK(c, gs_launch_sh_from_views(c->n, c->active_sh_degree(), c->sh_row_floats(), c->means, nviews, c->view_cams.as<float>(), drgb, d_shs,
                                      (flags & GS_BWD_OVERWRITE) ? 1 : 0, c->stream));
    return GS_OK;
}

}  // extern "C"
