// gs_api_bin.hip -- gs_bin (compactIdxs, reference src/forward.jl:118-161): the depth order and the per-tile splat lists.
// plan_bin decides once per frame HOW it is binned (gs_ctx::BinPlan); one function per path builds the lists from that plan: bin_small, bin_two_level
// (enqueued speculatively against the capacities at hand, written only as far as the view slot's history says they are walked, or in depth slabs), bin_radix.
#include "gs_ctx.h"
using Path = gs_ctx::BinPlan::Path;

// ---------------------------------------------------------------- binning in depth slabs
// A dense scene walks only the front of every tile's list before the transmittance early-out stops it (C3: 28 % of the
// 30 M instances, C5: 6 % of 507 M), yet the classic path sorts all of them.  With gs_config.slab_mode the frame is binned
// in rounds over slabs of the depth order: round 0 lists the front slab for every tile and composites it; a tile whose
// 256 pixels are all frozen is complete; round r lists the next slab only for the tiles still open (a gaussian whose
// rectangle holds no open tile drops out, instances of completed tiles inside the other rectangles are dropped while they
// are generated) and the forward resumes each open tile where it stopped -- same entries, same order, same 64-entry batch
// boundaries as the single list, so image, transmittance and (deterministic mode) gradients are bit-identical to the
// classic path.  The slab bounds come from the share of the instances the previous frame walked; a first frame, a sparse
// scene (share >= GS_SLAB_MAX_RATIO) or t_min = 0 take the classic single round.
// Measured on MI355X.  With the radix binning of round 1 (16 B of traffic per instance): at C3 (share 0.28) two rounds cost
// more than they save, at C5 (share 0.06) three rounds cut the frame from 10.4 to 6.8 ms.  With the two-level binning
// (gs_bin3.hip: 4 B written per instance, no pass over the instances) the single round wins at C5 as well (5.54 vs 5.67 ms:
// three forward launches with their tails and three level-1 passes cost more than the 0.4 ms of list writes they save), so
// the automatic mode now engages only below a share of 0.03 (GS_SLAB_MAX_RATIO overrides; the tests use 0.15).
#define GS_SLAB_MAX_RATIO 0.03
static double slab_max_ratio(const gs_ctx *c) { return c->cfg.slab_max_ratio > 0.0f ? (double)c->cfg.slab_max_ratio : GS_SLAB_MAX_RATIO; }
static void plan_rounds(const gs_ctx *c, gs_ctx::BinPlan &p) {
    p.n_rounds = 1;
    p.slab_lo[0] = 0; p.slab_lo[1] = c->n;
    if ((p.path != Path::TWO_LEVEL && p.path != Path::RADIX32) || c->cfg.t_min <= 0.0f || c->n < 1024 || c->order() == GS_ORDER_INDEX) return;
    double f[GS_MAX_ROUNDS] = {1.0, 1.0, 1.0, 1.0};
    int R = 1;
    if (c->cfg.slab_fractions[0] > 0.0f) {                                  // tests / experiments: explicit fractions
        for (int k = 0; k < 3 && k + 1 < GS_MAX_ROUNDS && c->cfg.slab_fractions[k] > 0.0f; ++k) { f[k] = c->cfg.slab_fractions[k]; R = k + 2; }
    } else if (const double rho = c->feedback.walked_ratio(); c->cfg.slab_mode == 1 && rho >= 0.0 && rho < slab_max_ratio(c)) {
        f[0] = std::min(0.9, std::max(0.02, 2.0 * rho + 0.02));
        f[1] = std::min(0.95, std::max(f[0] + 0.05, 6.0 * rho + 0.05));
        R = 3;
    }
    if (R == 1) return;
    int64_t prev = 0;
    int r = 0;
    for (int k = 0; k + 1 < R; ++k) {
        int64_t b = (int64_t)(f[k] * (double)c->n);
        b = std::min(c->n, std::max(prev, b));
        if (b > prev && b < c->n) { p.slab_lo[++r] = b; prev = b; }
    }
    p.slab_lo[++r] = c->n;
    p.n_rounds = r;
}

// The frame's bin plan.  The slab rounds need the previous frame's walked share, which this frame's read-back delivers: the plan of THIS
// frame uses the share known so far (one frame of lag; only speed depends on it).
static void plan_bin(gs_ctx *c) {
    gs_ctx::BinPlan p{};
    const int64_t ntiles = c->ntiles();
    p.tile_bits = 1;
    while ((1LL << p.tile_bits) < ntiles) ++p.tile_bits;
    p.gid_bits = 1;
    while ((1LL << p.gid_bits) < c->n) ++p.gid_bits;
    const int passes = (p.tile_bits + 7) / 8;
    p.lo_bits = passes <= 1 ? p.tile_bits : (p.tile_bits + 1) / 2; p.hi_bits = p.tile_bits - p.lo_bits;
    // two-level path (gs_bin3.hip): lists per super-tile of 8 x 8 tiles first; its bitmap must fit in LDS
    p.sbs = gs_bin3_sb_shift(c->gx, c->gy, (c->cfg.debug_flags & GS_DEBUG_SUPER16) ? 4 : (c->cfg.debug_flags & GS_DEBUG_SUPER8) ? 3 : 0);
    const int sb = 1 << p.sbs;
    p.sgx = (c->gx + sb - 1) / sb; p.sgy = (c->gy + sb - 1) / sb;
    const int asked = c->cfg.bin_path == 3 ? 0 : c->cfg.bin_path;
    const bool fast = asked != 1 && passes <= 2 && p.hi_bits + p.gid_bits <= 32 && gs_tile_ranges_supported(c->gx, c->gy);
    p.path = c->small_bin_possible() ? Path::SMALL : fast && asked == 0 && gs_bin3_supported(p.ns()) ? Path::TWO_LEVEL : fast ? Path::RADIX32 : Path::RADIX64;
    p.perm_on_demand = p.path == Path::SMALL && c->order() != GS_ORDER_INDEX;
    plan_rounds(c, p);
    c->bin = p;
}

// Two-level binning of one round (gs_bin3.hip).  two_level_count enqueues the level-1 histogram of the slab's gaussians
// (after it the round's three totals are on the device: coarse instances listed, fine instances of the slab, of all n);
// two_level_lists enqueues the super-tile lists and the tile lists for buffers that hold `coarse` / `fine` entries -- the
// actual totals once the host knows them, or (speculative launch) the capacities of the buffers at hand: the kernels compare
// the totals on the device with these numbers and list nothing when a buffer would overflow.
static GsBin3L1 two_level_args(gs_ctx *c, const uint32_t *perm_slab, int64_t n_all, int64_t nr, const uint8_t *sdone, size_t cap_coarse, size_t cap_fine) {
    GsBin3L1 b{};
    b.rect = c->rect.as<uint16_t>(); b.perm = perm_slab; b.sdone = sdone; b.n = n_all; b.n_slab = nr; b.sgx = c->bin.sgx; b.ns = c->bin.ns(); b.sbs = c->bin.sbs;
    b.rect_sorted = c->rect_sorted.as<uint32_t>(); b.table = c->l1_table.as<uint32_t>(); b.row_total = c->l1_rows.as<uint32_t>();
    b.partials = c->l1_partials.as<uint32_t>(); b.totals = c->bin_totals(); b.cranges = c->cranges.as<uint32_t>();
    b.cids = c->cids.as<uint32_t>(); b.clr = c->clr.as<uint16_t>();
    b.tilecnt = c->tilecnt.as<uint32_t>(); b.ntiles = (int)c->ntiles();
    b.cap_coarse = (uint32_t)std::min<size_t>(cap_coarse, 0xFFFFFFFEu); b.cap_fine = (uint32_t)std::min<size_t>(cap_fine, 0xFFFFFFFEu);
    return b;
}
static int two_level_count(gs_ctx *c, const uint32_t *perm_slab, int64_t n_all, int64_t nr, const uint8_t *sdone, bool to_host = false) {
    const int ns = c->bin.ns();
    HIPCHK(c, c->rect_sorted.ensure(sizeof(uint32_t) * 2 * (size_t)(nr ? nr : 1)));
    HIPCHK(c, c->l1_table.ensure(sizeof(uint32_t) * gs_bin3_table_words(nr, ns)));
    HIPCHK(c, c->l1_rows.ensure(sizeof(uint32_t) * (size_t)ns));
    HIPCHK(c, c->l1_partials.ensure(sizeof(uint32_t) * gs_bin3_partial_words(n_all, ns)));
    HIPCHK(c, c->counters.ensure(GS_COUNTER_BYTES));
    HIPCHK(c, c->cranges.ensure(sizeof(uint32_t) * 2 * (size_t)ns));
    HIPCHK(c, c->tilecnt.ensure(sizeof(uint32_t) * c->ntiles()));
    GsBin3L1 b = two_level_args(c, perm_slab, n_all, nr, sdone, 0, 0);
    if (to_host) {                                                          // where settle_totals reads them: the pinned copy of the counter block
        b.host_totals = c->pinned->counters.totals; b.host_walked = c->pinned->counters.work; b.walked_src = c->counters.as<uint32_t>();
        b.tile_walked = c->feedback.previous_walk(c->grid_key()); b.n_tile_walked = (int)c->ntiles();   // the previous forward's walked entries, per tile
    }
    HIPCHK(c, gs_bin3_l1_count(b, c->stream));
    return GS_OK;
}
// Round 0 (done == nullptr) writes the frame's list state in c->live and only ever SETS its flags: gs_bin's fresh FrameLive or relist_in_full() comes first.
// cap_src (round 0 of a one-round frame only): per-tile walked counts of the view slot's previous forward -> capped lists
static int two_level_lists(gs_ctx *c, const uint32_t *perm_slab, int64_t n_all, int64_t nr, size_t coarse, size_t fine, uint32_t *ranges, uint32_t *ids_out,
                           const uint8_t *done, const uint8_t *sdone, const uint32_t *cap_src = nullptr) {
    const int ns = c->bin.ns();
    gs_ctx::FrameLive &live = c->live;
    assert(done || (!live.frame_capped && !live.have_l2));
    if (!done) live.cap_src = cap_src;
    if (coarse == 0) {                                      // nothing listed: every tile range of the round is empty
        HIPCHK(c, hipMemsetAsync(ranges, 0, sizeof(uint32_t) * 2 * c->ntiles(), c->stream));
        return GS_OK;
    }
    const int64_t max_work = gs_bin3_max_work((int64_t)coarse, ns);
    HIPCHK(c, c->cids.ensure(sizeof(uint32_t) * coarse));
    HIPCHK(c, c->clr.ensure(sizeof(uint16_t) * coarse));
    HIPCHK(c, c->segcnt.ensure(sizeof(uint32_t) * ((size_t)1 << (2 * c->bin.sbs)) * (size_t)max_work));
    HIPCHK(c, gs_bin3_l1_scatter(two_level_args(c, perm_slab, n_all, nr, sdone, coarse, fine), c->stream));
    GsBin3Args a{};
    a.cranges = c->cranges.as<uint32_t>(); a.cids = c->cids.as<uint32_t>(); a.clr = c->clr.as<uint16_t>(); a.ranges = ranges; a.tilecnt = c->tilecnt.as<uint32_t>();
    a.done = done; a.segcnt = c->segcnt.as<uint32_t>(); a.ids_out = ids_out;
    a.gx = c->gx; a.gy = c->gy; a.sgx = c->bin.sgx; a.ns = ns; a.sbs = c->bin.sbs; a.max_work = (int)max_work;
    a.wide = (uint64_t)fine * 4ull >= (1ull << 32) || (c->cfg.debug_flags & GS_DEBUG_WIDE_CURSORS) != 0;
    a.totals = c->bin_totals(); a.cap_coarse = (uint32_t)std::min<size_t>(coarse, 0xFFFFFFFEu); a.cap_fine = (uint32_t)std::min<size_t>(fine, 0xFFFFFFFEu);
    if (cap_src && !done) {
        const size_t nt = (size_t)c->ntiles();
        HIPCHK(c, c->tile_nopen.ensure(sizeof(uint32_t) * nt));
        HIPCHK(c, c->smax.ensure(sizeof(uint32_t) * (size_t)ns));
        HIPCHK(c, c->tile_ext.ensure(sizeof(uint2) * nt));
        a.cap_src = cap_src; a.tile_nopen = c->tile_nopen.as<uint32_t>(); a.smax = c->smax.as<uint32_t>(); a.tile_ext = c->tile_ext.as<uint2>();
        a.ext_count = c->ext_count();
        live.frame_capped = true;
    }
    HIPCHK(c, gs_bin3_build_lists(a, c->stream));
    if (!done) { live.last_l2 = a; live.have_l2 = true; }
    return GS_OK;
}

// Capped lists: whose history, if any, caps the lists of the frame being binned (null: every list is written in full).  Engages on
// one-round frames of the two-level path with the early-out on, when the frame's view slot has rendered this grid before, and --
// unless gs_config.list_cap = 2 -- only when the ctx's previous frame walked less than GS_LIST_CAP_MAX_RATIO of its list entries on a
// grid with more tiles than wave slots.
#define GS_LIST_CAP_MAX_RATIO 0.15
static int list_cap_source(gs_ctx *c, const uint32_t **out) {
    *out = nullptr;
    const int64_t ntiles = c->ntiles();
    if (c->bin.path != Path::TWO_LEVEL || c->bin.n_rounds != 1 || c->cfg.list_cap == 1 || !(c->cfg.t_min > 0.0f) || ntiles <= 0) return GS_OK;
    if (c->cfg.debug_flags & GS_DEBUG_TINY_CAPS) {          // tests: every tile capped at the minimum, whatever it walked
        if (c->zero_tiles.cap < sizeof(uint32_t) * (size_t)ntiles) {
            HIPCHK(c, c->zero_tiles.ensure(sizeof(uint32_t) * (size_t)ntiles));
            HIPCHK(c, hipMemsetAsync(c->zero_tiles.p, 0, c->zero_tiles.cap, c->stream));
        }
        *out = c->zero_tiles.as<uint32_t>();
        return GS_OK;
    }
    // Engages where it pays (measured, profiles/r04b_kernel_stats_*): the write pass is bound by its entries only when most of them
    // are never walked -- C5 (6 % walked): 591 -> 129 us; at C3 (28 % walked) the pass goes 45 -> 37 us and the cap pass costs that.
    if (c->cfg.list_cap != 2 && (ntiles <= c->wave_slots || !(c->feedback.walked_ratio() >= 0.0 && c->feedback.walked_ratio() < GS_LIST_CAP_MAX_RATIO))) return GS_OK;
    if (const gs_ctx::ViewSlot *vs = c->history_slot()) *out = vs->history(c->grid_key()).walk;   // (frames without a slot: history only under schedule 4)
    return GS_OK;
}

// The 32-bit radix lists (gs_bin2.hip) of round r: round 0 reads the frame's offsets and rectangles, a later round those of the live gaussians (bin_round)
static GsBin2Args bin2_args(gs_ctx *c, int r) {
    const gs_ctx::BinPlan &p = c->bin;
    GsBin2Args b{};
    b.n = p.slab_lo[r + 1] - p.slab_lo[r]; b.n_inst = c->round_gen[r]; b.gx = c->gx; b.lo_bits = p.lo_bits; b.hi_bits = p.hi_bits; b.gid_bits = p.gid_bits;
    b.offsets = (r ? c->offsets_r : c->offsets).as<uint32_t>(); b.perm = c->live.perm_ptr ? c->live.perm_ptr + p.slab_lo[r] : nullptr;
    b.rect = (r ? c->rect_r : c->rect).as<uint16_t>();
    b.cs = c->cs.as<uint32_t>(); b.block_hist = c->table.as<uint32_t>(); b.digit_total = c->digit_total.as<uint32_t>();
    b.buf_a = c->words.as<uint32_t>(); b.ids_out = c->ids.as<uint32_t>() + c->round_ids_off[r]; b.ballot_ranks = c->cfg.rank_mode != 0;
    if (r) { b.done = c->tile_done.as<uint8_t>(); b.live_total = c->live_total.as<uint32_t>() + r; }
    return b;
}

// later round of a slab frame on the two-level path
static int bin_round_two_level(gs_ctx *c, int r) {
    const gs_ctx::BinPlan &p = c->bin;
    const int64_t lo = p.slab_lo[r], nr = p.slab_lo[r + 1] - lo;
    const uint32_t *perm = c->live.perm_ptr + lo;
    HIPCHK(c, c->ranges_r[r].ensure(sizeof(uint32_t) * 2 * c->ntiles()));
    HIPCHK(c, c->sdone.ensure((size_t)p.ns()));
    {
        StageTimer t(c, GS_STAGE_COUNT_SCAN);
        HIPCHK(c, gs_launch_super_done(c->tile_done.as<uint8_t>(), c->gx, c->gy, p.sgx, p.sgy, p.sbs, c->sdone.as<uint8_t>(), c->stream));
        if (int rc = two_level_count(c, perm, nr, nr, c->sdone.as<uint8_t>())) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(c->pinned->readback, c->bin_totals(), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_count, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_count));
    harvest_events(c);
    const int64_t coarse = (int64_t)c->pinned->readback[0];
    c->round_gen[r] = (int64_t)c->pinned->readback[1];
    c->round_ids_off[r] = c->round_ids_off[r - 1] + (size_t)c->round_gen[r - 1];
    if (c->round_ids_off[r] + (size_t)c->round_gen[r] > (size_t)c->n_inst) return fail(c, GS_ERR_HIP, "gs_forward: slab instance accounting out of range");
    {
        StageTimer t(c, GS_STAGE_TILE_SORT);
        if (int rc = two_level_lists(c, perm, nr, nr, (size_t)coarse, (size_t)c->round_gen[r], c->ranges_r[r].as<uint32_t>(), c->ids.as<uint32_t>() + c->round_ids_off[r],
                                     c->tile_done.as<uint8_t>(), c->sdone.as<uint8_t>())) return rc;
    }
    return GS_OK;
}

// Lists of round r (r >= 1) for the tiles still open; called from gs_forward after the forward of round r - 1.
int bin_round(gs_ctx *c, int r) {
    if (c->bin.path == Path::TWO_LEVEL) return bin_round_two_level(c, r);
    const int64_t lo = c->bin.slab_lo[r], nr = c->bin.slab_lo[r + 1] - lo;
    const uint32_t *perm = c->live.perm_ptr + lo;
    HIPCHK(c, c->live2d.ensure(sizeof(uint32_t) * 2 * (size_t)(c->gx + 1) * (c->gy + 1)));      // the table + the row-pass scratch
    HIPCHK(c, c->rect_r.ensure(sizeof(uint16_t) * 4 * c->n1()));
    HIPCHK(c, c->offsets_r.ensure(sizeof(uint32_t) * ((size_t)nr + 1)));
    HIPCHK(c, c->live_total.ensure(sizeof(uint32_t) * GS_MAX_ROUNDS));
    HIPCHK(c, c->ranges_r[r].ensure(sizeof(uint32_t) * 2 * c->ntiles()));
    {
        StageTimer t(c, GS_STAGE_COUNT_SCAN);
        HIPCHK(c, gs_launch_live_prefix(c->tile_done.as<uint8_t>(), c->gx, c->gy, c->live2d.as<uint32_t>(),
                                        c->live2d.as<uint32_t>() + (size_t)(c->gx + 1) * (c->gy + 1), c->stream));
        HIPCHK(c, gs_launch_count_scan_live(c->rect.as<uint16_t>(), perm, c->live2d.as<uint32_t>(), c->gx, c->rect_r.as<uint16_t>(),
                                            c->offsets_r.as<uint32_t>(), c->block_sums.as<uint32_t>(), nr, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->pinned->readback, c->offsets_r.as<uint32_t>() + nr, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_count, c->stream));
    {
        StageTimer t(c, GS_STAGE_RANGES);                               // does not need the count: keeps the GPU busy while the host waits
        HIPCHK(c, gs_launch_tile_ranges(c->rect_r.as<uint16_t>(), perm, nr, c->diff.as<int>(), c->gx, c->gy, c->ranges_r[r].as<uint32_t>(),
                                        c->tile_done.as<uint8_t>(), c->stream));
    }
    HIPCHK(c, hipEventSynchronize(c->ev_count));
    harvest_events(c, GS_STAGE_RANGES);
    c->round_gen[r] = (int64_t)c->pinned->readback[0];
    c->round_ids_off[r] = c->round_ids_off[r - 1] + (size_t)c->round_gen[r - 1];
    if (c->round_gen[r] == 0) return GS_OK;
    if (c->round_ids_off[r] + (size_t)c->round_gen[r] > (size_t)c->n_inst) return fail(c, GS_ERR_HIP, "gs_forward: slab instance accounting out of range");
    {
        StageTimer t(c, GS_STAGE_TILE_SORT);
        HIPCHK(c, gs_bin2_build_lists(bin2_args(c, r), c->stream));
    }
    return GS_OK;
}

// The bucket path of the depth sort reported a bucket beyond a workgroup's capacity (it was sorted through global memory: correct,
// slow): the next 64 frames use the classic sort, then the bucket path is tried again.  Read once the frame's ev_count has passed.
static void dsort_feedback(gs_ctx *c) {
    if (!c->dsort_buckets_used) return;
    c->dsort_buckets_used = false;
    if (*c->dsort_stat() != 0u && c->cfg.depth_sort != 2) c->dsort_classic_until = c->frame_id + 64;
}

// The frame's totals have arrived on the host, however they travelled (the pinned counter block; the radix paths' copies): coarse instances listed, fine
// instances of round 0's slab and of all n; walked_prev: the u64 sum of the previous forward's walk, read only when one was sent (WalkFeedback::sum_arrived).
static int totals_arrived(gs_ctx *c, uint32_t coarse, uint32_t fine_slab, uint32_t fine_all, const uint32_t *walked_prev) {
    if (fine_all == 0xFFFFFFFFu)
        return fail(c, GS_ERR_UNSUPPORTED, "gs_bin: more than 2^32 - 2 tile instances (32-bit list offsets); reduce the scene or the image");
    c->feedback.sum_arrived(walked_prev);
    c->n_inst = (int64_t)fine_all;
    c->n_coarse = (int64_t)coarse;
    c->round_gen[0] = c->bin.n_rounds > 1 ? (int64_t)fine_slab : c->n_inst;
    c->round_ids_off[0] = 0;
    return GS_OK;
}

// The frame's totals arrive in pinned memory behind ev_count.  On the two-level path the host does not wait for them inside
// gs_bin (speculative launch): it enqueues the lists against the CAPACITIES of the buffers it already has, the kernels compare
// the totals on the device with those capacities (gs_bin3.hip: lists_overflow) and list nothing if a buffer is too small;
// settle_totals, called once the host needs the numbers (after gs_forward has enqueued the composite), reads them and -- in
// the rare frame whose lists outgrew a buffer -- grows the buffers and enqueues the lists again (returns 1: the caller
// re-enqueues what it had enqueued on top of the empty lists).  The GPU never idles while the host wakes up, and there is no
// stream synchronisation between gs_preprocess and the end of the frame.
int settle_totals(gs_ctx *c, bool *redo, bool may_relist) {
    if (redo) *redo = false;
    if (!c->pending_totals) return GS_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_count));
    c->pending_totals = false;
    harvest_events(c);
    dsort_feedback(c);
    const CounterBlock &h = c->pinned->counters;
    const uint32_t coarse = h.totals[0], fine_slab = h.totals[1];
    if (int rc = totals_arrived(c, coarse, fine_slab, h.totals[2], h.work)) return rc;
    if (!c->live.spec_lists || c->live.speculation_held(coarse, fine_slab)) return GS_OK;
    if (!may_relist) { c->fall_back(gs_ctx::Stage::PREPROCESSED); return GS_OK; }                  // the frame is being abandoned (a new gs_preprocess / gs_bin follows)
    // a list outgrew its buffer: nothing was listed (all ranges empty).  Grow and list again with the real totals -- in FULL.  (The caps'
    // source would still stand: the slot's walk is double buffered, and the forward that just ran on the empty lists wrote the OTHER
    // buffer.  But this is a rare frame -- a model that outgrew its buffers -- and full lists are the fast choice there)
    HIPCHK(c, c->ids.ensure(sizeof(uint32_t) * (size_t)(c->n_inst ? c->n_inst : 1)));
    c->live.relist_in_full();
    {
        StageTimer t(c, GS_STAGE_TILE_SORT);
        if (int rc = two_level_lists(c, c->live.perm_ptr, c->n, c->bin.slab_lo[1], (size_t)coarse, (size_t)fine_slab, c->ranges.as<uint32_t>(), c->ids.as<uint32_t>(), nullptr, nullptr,
                                     nullptr)) return rc;
    }
    if (redo) *redo = true;
    return GS_OK;
}

// The depth order of the frame (CUDA.sortperm, forward.jl:103) -> c->perm.  Also called by gs_get_array for a frame binned by the small
// path, which needs no global order.
int depth_order(gs_ctx *c) {
    const size_t n1 = c->n1();
    StageTimer t(c, GS_STAGE_DEPTH_SORT);
    HIPCHK(c, c->pairs_a.ensure(sizeof(uint64_t) * n1));
    HIPCHK(c, c->pairs_b.ensure(sizeof(uint64_t) * n1));
    HIPCHK(c, c->perm.ensure(sizeof(uint32_t) * n1));
    HIPCHK(c, c->table.ensure(sizeof(uint32_t) * gs_sort_table_entries(c->n)));
    HIPCHK(c, c->digit_total.ensure(sizeof(uint32_t) * 4 * 256));
    int in_b = 0;
    uint32_t *perm = c->perm.as<uint32_t>();            // the last pass writes the permutation itself (low word of the pairs)
    // Two steps (256 key-range buckets, then one workgroup per bucket in LDS: 4 launches) when this frame's preprocess left the
    // key range, the mean bucket is well inside a workgroup's capacity, and no oversize bucket was reported lately; else the
    // classic four LSD passes (12 launches).  Same permutation either way.
    const bool buckets = c->range_valid && c->dsort_can_bucket();
    c->dsort_buckets_used = buckets;
    if (c->range_valid && !buckets)                     // folded but not consumed (cannot happen with one predicate; kept so that a stale union never survives)
        HIPCHK(c, gs_depth_range_reset(key_range_of(c, c->range_parity), c->stream, 1));
    if (buckets) {
        uint32_t *range = key_range_of(c, c->range_parity), *other = key_range_of(c, c->range_parity ^ 1);
        c->dsort_stat_parity = c->range_parity;
        *c->dsort_stat() = 0u;                          // (no kernel of an earlier frame writes this parity's word any more: two frames back)
        HIPCHK(c, gs_depth_sort_buckets(c->depth_key.as<uint32_t>(), c->pairs_a.as<uint64_t>(), c->pairs_b.as<uint64_t>(), c->n, c->table.as<uint32_t>(),
                                        c->digit_total.as<uint32_t>(), perm, range, other, c->dsort_stat(), c->stream, c->cfg.rank_mode != 0));
    } else {
        // (depth | id) pairs are formed by the first pass from the 32-bit keys; the last pass writes only the ids
        HIPCHK(c, gs_radix_sort_u64(c->pairs_a.as<uint64_t>(), c->pairs_b.as<uint64_t>(), c->n, 32, 64, c->table.as<uint32_t>(),
                                    c->digit_total.as<uint32_t>(), &in_b, c->stream, c->cfg.rank_mode != 0, perm, c->depth_key.as<uint32_t>()));
    }
    c->live.perm_ptr = perm;
    return GS_OK;
}

// Small frames (gs_bin_small.hip): the whole of gs_bin in one launch, one workgroup per tile.  The ids buffer holds every (gaussian, tile)
// pair the path admits, so nothing is speculative; the totals travel to the host as on the two-level path.
static int bin_small(gs_ctx *c) {
    const size_t n = (size_t)c->n, nt = (size_t)c->ntiles();
    HIPCHK(c, c->ids.ensure(sizeof(uint32_t) * n * nt));
    if (c->range_valid)                                                     // (gs_preprocess judged otherwise and folded the key range: nobody will consume it)
        HIPCHK(c, gs_depth_range_reset(key_range_of(c, c->range_parity), c->stream, 1));
    GsBinSmallArgs a{};
    a.depth_key = c->order() != GS_ORDER_INDEX ? c->depth_key.as<uint32_t>() : nullptr; a.rect = c->rect.as<uint2>();
    a.n = (int)c->n; a.gx = c->gx; a.gy = c->gy; a.ntiles = (int)nt;
    a.ranges = c->ranges.as<uint32_t>(); a.ids = c->ids.as<uint32_t>(); a.totals = c->bin_totals();
    a.host_totals = c->pinned->counters.totals; a.host_walked = c->pinned->counters.work; a.walked_src = c->counters.as<uint32_t>();
    a.tile_walked = c->feedback.previous_walk(c->grid_key()); a.n_tile_walked = (int)nt;
    {   // the rows the composite backward accumulates into (64 B per gaussian; nothing touches them between here and that kernel)
        HIPCHK(c, c->g2d.ensure(c->g2d_bytes()));                          // (this path has n >= 1: every row of the model, no more)
        a.zero = c->g2d.as<uint4>(); a.zero_words16 = c->g2d_bytes() / sizeof(uint4);
    }
    {
        StageTimer t(c, GS_STAGE_TILE_SORT);
        HIPCHK(c, gs_bin_small(a, c->stream));
    }
    c->live.g2d_clean = true;
    HIPCHK(c, hipEventRecord(c->ev_count, c->stream));
    c->pending_totals = true;
    return GS_OK;
}

// Two-level path (gs_bin3.hip): count, totals on their way to the host, then the lists -- speculatively when there is one round and buffers to launch against
static int bin_two_level(gs_ctx *c) {
    uint32_t *perm = c->live.perm_ptr;
    const int64_t n0 = c->bin.slab_lo[1];                                   // list positions of round 0
    {
        StageTimer t(c, GS_STAGE_COUNT_SCAN);
        if (int rc = two_level_count(c, perm, c->n, n0, nullptr, c->n > 0)) return rc;
    }
    // the previous frame's walked count (bytes 0..7 of the counter block) and this frame's totals (bytes 128..139) travel to the host:
    // stored into coherent pinned memory by the scan kernel itself (no copy command in the stream); an empty model launches nothing
    if (c->n <= 0) HIPCHK(c, hipMemcpyAsync(&c->pinned->counters, c->counters.p, GS_COUNTER_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_count, c->stream));
    c->pending_totals = true;
    const size_t cap_coarse = std::min(c->cids.cap / sizeof(uint32_t), c->clr.cap / sizeof(uint16_t)), cap_fine = c->ids.cap / sizeof(uint32_t);
    const uint32_t *cap_src = nullptr;
    if (int rc = list_cap_source(c, &cap_src)) return rc;
    if (c->bin.n_rounds == 1 && cap_coarse > 0 && cap_fine > 0) {
        c->live.speculate(cap_coarse, cap_fine);
        StageTimer t(c, GS_STAGE_TILE_SORT);
        return two_level_lists(c, perm, c->n, n0, cap_coarse, cap_fine, c->ranges.as<uint32_t>(), c->ids.as<uint32_t>(), nullptr, nullptr, cap_src);
    }
    // first frame of a ctx, or a slab frame: the host needs the totals now
    if (int rc = settle_totals(c, nullptr, true)) return rc;
    HIPCHK(c, c->ids.ensure(sizeof(uint32_t) * (size_t)(c->n_inst ? c->n_inst : 1)));
    StageTimer t(c, GS_STAGE_TILE_SORT);
    return two_level_lists(c, perm, c->n, n0, (size_t)c->n_coarse, (size_t)c->round_gen[0], c->ranges.as<uint32_t>(), c->ids.as<uint32_t>(), nullptr, nullptr, cap_src);
}

// RADIX64: explicit 64-bit tile|id instances, two radix passes (fallback; identical lists)
static int radix64_lists(gs_ctx *c) {
    const size_t ni1 = c->n_inst ? (size_t)c->n_inst : 1;
    HIPCHK(c, c->inst_a.ensure(sizeof(uint64_t) * ni1));
    HIPCHK(c, c->inst_b.ensure(sizeof(uint64_t) * ni1));
    {
        StageTimer t(c, GS_STAGE_EMIT);
        HIPCHK(c, gs_launch_emit(c->rect.as<uint16_t>(), c->live.perm_ptr, c->offsets.as<uint32_t>(), c->inst_a.as<uint64_t>(), c->n, c->gx, c->stream));
    }
    uint64_t *sorted = nullptr;
    {
        StageTimer t(c, GS_STAGE_TILE_SORT);
        int in_b = 0;
        HIPCHK(c, gs_radix_sort_u64(c->inst_a.as<uint64_t>(), c->inst_b.as<uint64_t>(), c->n_inst, 32, 32 + c->bin.tile_bits,
                                    c->table.as<uint32_t>(), c->digit_total.as<uint32_t>(), &in_b, c->stream, c->cfg.rank_mode != 0));
        sorted = in_b ? c->inst_b.as<uint64_t>() : c->inst_a.as<uint64_t>();
    }
    StageTimer t(c, GS_STAGE_RANGES);
    HIPCHK(c, gs_launch_ranges(sorted, c->n_inst, c->ranges.as<uint32_t>(), c->ntiles(), c->stream));
    HIPCHK(c, gs_launch_split_ids(sorted, c->ids.as<uint32_t>(), c->n_inst, c->stream));
    return GS_OK;
}

// Radix paths (bin_path 2 / 1; grids the two-level path refuses): the host reads the instance count before the instance passes
static int bin_radix(gs_ctx *c) {
    const size_t n = (size_t)c->n;
    const bool fast = c->bin.path == Path::RADIX32, slabs = c->bin.n_rounds > 1;
    const int64_t n0 = c->bin.slab_lo[1];                                   // list positions of round 0
    uint32_t *perm = c->live.perm_ptr;
    PinnedWords *h = c->pinned;
    {
        StageTimer t(c, GS_STAGE_COUNT_SCAN);
        HIPCHK(c, c->offsets.ensure(sizeof(uint32_t) * (n + 1)));
        HIPCHK(c, gs_launch_count_scan(c->rect.as<uint16_t>(), perm, c->offsets.as<uint32_t>(), c->block_sums.as<uint32_t>(), c->n, c->stream));
    }
    // the one host read-back of the frame (the reference reads maxHits back, forward.jl:139): the instance count, the
    // generated positions of round 0 and the previous frame's walked count.  Work that does not need the count (the tile
    // ranges) is enqueued BEFORE the host waits, so the GPU stays busy while the host wakes up and launches the instance passes.
    HIPCHK(c, hipMemcpyAsync(&h->readback[0], c->offsets.as<uint32_t>() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h->readback[1], c->offsets.as<uint32_t>() + n0, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (const uint32_t *walk = c->feedback.previous_walk(c->grid_key())) {
        HIPCHK(c, gs_launch_sum_tiles(walk, c->tile_work.as<uint32_t>(), (int)c->ntiles(), c->counters.as<unsigned long long>(), c->stream));
        HIPCHK(c, hipMemcpyAsync(h->walked_prev, c->counters.p, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_count, c->stream));
    if (fast) {
        HIPCHK(c, c->diff.ensure(sizeof(int) * gs_tile_ranges_scratch_ints(c->gx, c->gy)));
        StageTimer t(c, GS_STAGE_RANGES);
        HIPCHK(c, gs_launch_tile_ranges(c->rect.as<uint16_t>(), slabs ? perm : nullptr, slabs ? n0 : c->n, c->diff.as<int>(), c->gx, c->gy,
                                        c->ranges.as<uint32_t>(), nullptr, c->stream));
    }
    HIPCHK(c, hipEventSynchronize(c->ev_count));
    harvest_events(c, fast ? GS_STAGE_RANGES : -1);
    dsort_feedback(c);
    if (int rc = totals_arrived(c, 0, h->readback[1], h->readback[0], h->walked_prev)) return rc;
    const size_t ni1 = c->n_inst ? (size_t)c->n_inst : 1;
    HIPCHK(c, c->table.ensure(sizeof(uint32_t) * gs_sort_table_entries(c->n_inst > c->n ? c->n_inst : c->n)));
    HIPCHK(c, c->digit_total.ensure(sizeof(uint32_t) * 4 * 256));
    HIPCHK(c, c->ids.ensure(sizeof(uint32_t) * ni1));
    if (!fast) return radix64_lists(c);
    // ---- generate-in-pass binning on 32-bit words (gs_bin2.hip)
    const size_t nchunks = ((size_t)c->n_inst + 4095) / 4096;
    HIPCHK(c, c->cs.ensure(sizeof(uint32_t) * (nchunks + 2)));
    if (c->bin.hi_bits > 0) HIPCHK(c, c->words.ensure(sizeof(uint32_t) * ni1));
    StageTimer t(c, GS_STAGE_TILE_SORT);
    HIPCHK(c, gs_bin2_build_lists(bin2_args(c, 0), c->stream));
    return GS_OK;
}

// The frame as its plan says: the depth order (unless the path needs none), the buffers every path writes, the path
static int bin_frame(gs_ctx *c) {
    const Path path = c->bin.path;
    if (c->order() != GS_ORDER_INDEX && path != Path::SMALL) { if (int rc = depth_order(c)) return rc; }
    HIPCHK(c, c->ranges.ensure(sizeof(uint32_t) * 2 * c->ntiles1()));
    HIPCHK(c, c->counters.ensure(GS_COUNTER_BYTES));
    if (path != Path::SMALL) HIPCHK(c, c->block_sums.ensure(sizeof(uint32_t) * 3 * ((size_t)c->n / 2048 + 2)));
    if (int rc = path == Path::SMALL ? bin_small(c) : path == Path::TWO_LEVEL ? bin_two_level(c) : bin_radix(c)) return rc;
    c->reach(gs_ctx::Stage::BINNED);
    return GS_OK;
}

extern "C" int gs_bin(gs_ctx *c, int32_t gx, int32_t gy) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_stage(c, gs_ctx::Stage::PREPROCESSED, "gs_bin: gs_preprocess first")) return rc;
    if ((gx != 0 || gy != 0) && (gx != c->gx || gy != c->gy))
        return fail(c, GS_ERR_UNSUPPORTED, "gs_bin: blocks must equal ceil(W/16) x ceil(H/16)");
    if (bind_device(c)) return GS_ERR_HIP;
    if (int rc = settle_totals(c, nullptr, false)) return rc;               // a frame that was binned but never rendered
    // the frame's live state starts here, whatever its path; the plan is fixed from here to the next gs_bin
    c->live = gs_ctx::FrameLive{};
    plan_bin(c);
    return bin_frame(c);
}
