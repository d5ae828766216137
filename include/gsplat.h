/*
 * gsplat.h -- C ABI of libgsplat_hip.so, the MI355X (gfx950) differentiable Gaussian-splat
 * rasterizer that sits behind arhik/GaussianSplat's (empty) backend.jl.
 *
 * The reference defines no FFI: src/backend.jl:1 is empty and the de-facto surface is five
 * Julia functions over a mutable renderer struct.  Each entry point below names the
 * reference function it replaces (paths relative to /root/reference):
 *
 *   gs_create / gs_destroy    getRenderer(...)                    src/renderer.jl:119-149,164-186
 *   gs_set_model              initData + `|> CuArray` uploads     src/splat.jl:106-119, src/forward.jl:63-69,169-170
 *   gs_set_camera             defaultCamera/computeTransform/...  src/forward.jl:53-62, src/camera.jl:88-111
 *   gs_set_model_2d           initData(Val(SPLAT2D)) / SplatData2D src/splat.jl:20-26,74-87 (2-D image-fitting renderer)
 *   gs_set_image_size         size(renderer.imageData)            src/forward.jl:29
 *   gs_preprocess             preprocess(renderer)                src/forward.jl:35-111 (3-D), :9-33 (2-D)
 *   gs_bin                    compactIdxs(renderer,threads,blocks) src/forward.jl:118-161
 *   gs_forward                forward(renderer,tps,threads,blocks) src/forward.jl:163-198
 *   gs_backward               backward(renderer, dC)              src/backward.jl:3-38
 *   gs_reset_grads            resetGrads(renderer.splatGrads)     src/splat.jl:158-173
 *   gs_backward_camera        (none: the reference's camera is a constant) the frame's gradient into T, P, eye, lookAt, fx, fy
 *   gs_exposure_apply         (none: the reference's loss sees the raw frame) out = w (M rgb + b), a 3 x 4 colour affine per view and a mask
 *   gs_exposure_backward      (none: the reference's loss sees the raw frame) its adjoints into the image and into the 12 floats
 *   gs_exposure_adam          (none: the reference's loss sees the raw frame) the Adam step of one view's 12 floats
 *   gs_bilagrid_apply / _backward / _tv / _adam  (none: the reference's loss sees the raw frame) a per-view bilateral grid of colour affines
 *
 * Conventions
 *   - plain C: pointers + sizes, no exceptions; every function returns 0 (GS_OK) or a
 *     negative gs_status; gs_last_error(ctx) gives the message of the last failure.
 *   - array layouts are the reference's column-major ones so a Julia `pointer(A)` can be
 *     passed unpermuted: parameters [component, gaussian] (component fastest), images
 *     [x, y, channel] (x fastest, channel planes), T and P 4x4 column-major.
 *   - `mem` says where a caller buffer lives: GS_MEM_HOST (copied over PCIe) or
 *     GS_MEM_DEVICE (a HIP device pointer on the ctx's device; used in place).
 *   - the caller owns every buffer it passes; the library owns the ctx scratch (grow-only,
 *     no per-frame allocation once sizes are stable).
 *   - one ctx = one GPU = one stream; a ctx is not thread-safe, different ctxs are.
 *   - all work is enqueued on the ctx stream; functions that return data to HOST buffers
 *     synchronise that stream before returning, device-buffer variants do not.  gs_bin does not wait for the GPU either
 *     (from a ctx's second frame on): the tile lists are enqueued with the buffer sizes of the previous frame while the
 *     frame's instance counts are still on their way to the host; gs_forward reads them after it has enqueued the
 *     composite and, in the rare case that a list outgrew its buffer, rebuilds lists and image with larger ones.
 *   - there is NO CPU fallback: without a HIP device gs_create fails with GS_ERR_NO_DEVICE.
 */
#ifndef GSPLAT_H
#define GSPLAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: gs_config carries abi_version (gs_create refuses any other value: a caller built against another header fails loudly
 *    instead of running with shifted fields); schedule 0 now means "library default"; view slots (gs_set_view_slot);
 *    speculative binning (no host wait inside gs_bin); GS_BWD_PARAMS_SH / _GEOM; 64-byte payload and gradient rows.
 * 3: gs_config.list_cap (capped tile lists from the view slot's history; a former reserved word, sizeof unchanged); 4096 view
 *    slots; gs_get_list_stats.  (gs_config.tile_parts, a later reserved word: 0 = the library's choice, as reserved words must be.) */
#define GS_ABI_VERSION 3

typedef enum {
    GS_OK = 0,
    GS_ERR_INVALID = -1,      /* bad argument / call order                                  */
    GS_ERR_NO_DEVICE = -2,    /* no usable HIP device                                       */
    GS_ERR_HIP = -3,          /* a HIP runtime call failed (see gs_last_error)              */
    GS_ERR_OOM = -4,          /* device allocation failed                                   */
    GS_ERR_UNSUPPORTED = -5   /* e.g. tile size != 16, sh_degree > 3                        */
} gs_status;

typedef enum { GS_MEM_HOST = 0, GS_MEM_DEVICE = 1 } gs_mem;

/* Order of every per-tile splat list (what the radix sort realises).
 *   INDEX       literal reference behaviour: compact.jl:3-21 places a gaussian at slot
 *               inclusive-scan(hits) over the GAUSSIAN INDEX axis, so sortIdxs has no effect.
 *   DEPTH_DESC  the order forward.jl:103 computes (sortperm(-tps[3,:]), far -> near) and the
 *               TODO at forward.jl:123-131 intends; ties by gaussian index (stable).
 *   DEPTH_ASC   near -> far (extension).                                                      */
typedef enum { GS_ORDER_INDEX = 0, GS_ORDER_DEPTH_DESC = 1, GS_ORDER_DEPTH_ASC = 2 } gs_order;

typedef struct {
    int32_t struct_size;      /* = sizeof(gs_config); ABI guard                              */
    int32_t abi_version;      /* = GS_ABI_VERSION of the header the caller was built with    */
    int32_t tile_size;        /* threads=(16,16) of examples/main.jl:9; only 16 is supported */
    int32_t order;            /* gs_order; default GS_ORDER_DEPTH_DESC                       */
    float   t_min;            /* transmittance early-out: a pixel stops taking splats once
                                 its T < t_min.  0 = literal reference (splat.jl:224-261 has
                                 no early-out).  Default 1e-5 (pixel error <= t_min*max|rgb|) */
    int32_t deterministic;    /* 1: the per-(tile,splat) gradient sums are accumulated as 2^-40 fixed
                                 point (2^-28 for the second-order moments) with integer atomics (order independent ->
                                 bitwise reproducible run to run; absolute resolution 9e-13 / 3.7e-9 per add);
                                 0: float atomics (run-to-run differences in the last bits)    */
    int32_t export_debug;     /* 1: gs_preprocess also materialises the reference's scratch
                                 arrays (ts, tps, mu', cov3ds, cov2ds, invCov2ds, bbs) for
                                 gs_get_array; costs 124 extra bytes/gaussian of HBM writes   */
    int32_t profile_stages;   /* 1: record hipEvents around every stage (gs_get_stage_times; costs ~3 % of a C3 frame);
                                 2 + s: around stage s (gs_stage) only; 0: none */
    int32_t bin_path;         /* tile lists (same lists on every path, bit for bit): 0 (default) two-level binning -- lists per
                                 super-tile of 8 x 8 tiles from an LDS bitmap, tile lists as filtered copies -- and, for SMALL frames
                                 (up to 16 384 gaussians, 1024 tiles, 4 M gaussian x tile pairs: BASELINE C1), the whole of gs_bin in ONE
                                 launch, one workgroup per tile that ranks the tile's gaussians by depth in up to 128 KB of dynamic LDS
                                 (no global depth order: renderer.sortIdxs is computed on demand, gs_get_array(GS_ARR_SORT_IDXS));
                                 3: two-level whatever the size (tests, A/B); 2: radix sort of instances generated in-pass (32-bit
                                 words); 1: explicit 64-bit tile|id instances + two radix passes */
    int32_t rank_mode;        /* radix-sort stable ranks: 1 (default) = wave64 ballots (portable); 0 = one LDS atomic-add-return per
                                 key -- its pre-values come back in ascending lane order on gfx950, which is an observed, not a
                                 documented property: gs_create CHECKS it on the device with a probe kernel and falls back to 1 if
                                 the check fails.  Same lists either way.  Since the two-level binning only the depth sort ranks
                                 keys at all; there the atomic form saves 4 us of a 1.44 ms C3 frame, so ballots are the default */
    int32_t alpha_cull;       /* 1 (default): while staging a tile's list the composite kernels drop every
                                 (tile, splat) entry whose largest alpha over that tile's pixels is below 2^-27
                                 -- a no-op in the reference's own fp32 arithmetic (T*(1-alpha) == T, colour term
                                 < 7.5e-9*|rgb|).  The lists (gs_bin) are unchanged.  0: evaluate every entry. */
    int32_t schedule;         /* composite kernels (speed only: every mode gives the same image and, up to atomic order, gradients):
                                 0 the library default (= 3);
                                 3 one wave per tile, plain launch over a longest-first permutation of the tiles (groups of 8 x 8
                                   tiles dealt to the XCDs): the backward by the forward's per-tile count of evaluated
                                   entries of the same frame (C3: 0.84 -> 0.74 ms); the forward by the count the last forward
                                   rendered under the same VIEW SLOT measured (gs_set_view_slot: training cycles over a fixed
                                   camera set), in tile order when the slot has no history yet;
                                 4 as 3, and a forward without slot history uses the work of this ctx's PREVIOUS forward
                                   (pays when consecutive frames see similar views);
                                 1 one wave per tile in launch (tile) order.
                                 (Persistent waves pulling tiles from per-XCD ticket counters were measured slower and are gone:
                                 profiles/HISTORY.md.)                                                                          */
    int32_t slab_mode;        /* binning in depth slabs (speed only; image, transmittance and deterministic-mode gradients are
                                 bit-identical either way): 1 (default) automatic -- when the previous frame walked under 3 % of
                                 its tile instances before the transmittance early-out stopped every tile (with the two-level
                                 binning a single round is faster above that share), the next frame is
                                 binned in three rounds over slabs of the depth order and only the tiles still open take the later
                                 slabs; 0 always one round (the classic full lists).  In a slab frame the per-tile lists are
                                 spread over the rounds, so GS_ARR_TILE_RANGES / SORTED_IDS / SORTED_KEYS are unavailable (a
                                 ctx's first frame is always a classic one).                                              */
    float   slab_max_ratio;   /* slab_mode 1 engages when the previous frame walked less than this share of its tile instances;
                                 0 = the library default (0.03, where three rounds start to beat one with the two-level binning)  */
    float   slab_fractions[3];/* tests / experiments: != 0 forces depth slabs that end at these fractions of the depth order
                                 (0 < f1 [< f2 [< f3]] < 1), whatever the previous frame walked                               */
    int32_t debug_flags;      /* GS_DEBUG_* bits; 0 in production                                                              */
    int32_t depth_sort;       /* the depth order (CUDA.sortperm of forward.jl:103; same permutation on every path, bit for bit):
                                 0 (default) automatic -- two steps (256 buckets over the frame's key range, then one workgroup
                                 per bucket: inside LDS up to 8192 pairs, else through global memory in chunks; 4 launches) for 3-D frames
                                 of up to 8.4 M gaussians, the four-pass LSD radix sort (12 launches) otherwise and for 64 frames after
                                 a frame whose depths piled up in one bucket (more than eight chunks); 1 always the four-pass sort; 2 always the two-step sort (tests)                          */
    int32_t list_cap;         /* capped tile lists (speed only; image, transmittance and deterministic-mode gradients are bit-identical
                                 either way).  The reference allocates and fills every tile's list in full (forward.jl:139-142:
                                 hitIdxs of maxBinSize per tile), although with the transmittance early-out a dense scene walks a
                                 fraction of it (C3: 28 %, C5: 6 % of the entries).  0 (default) automatic: when the frame's VIEW SLOT
                                 (gs_set_view_slot) has rendered this image size before, gs_bin writes every tile's list only as far
                                 as that frame walked it (+ 25 % + 128 entries, rounded up to a segment of the two-level binning); a
                                 composite wave that gets to the written end with pixels still taking entries writes the next
                                 segment of its tile's list itself and goes on, so nothing depends on the history being right.
                                 Engages when the ctx's previous frame walked less than 15 % of its list entries on a grid of more
                                 than 5120 tiles (measured: at 28 % walked the shorter write pass only pays for the extra cap pass).
                                 1 never; 2 also on small grids (tests).  GS_ARR_TILE_RANGES is always the full ranges; asking for
                                 GS_ARR_SORTED_IDS / _KEYS of a capped frame first writes the unwritten rest.                   */
    int32_t tile_parts;       /* how a tile is shared between waves (speed only).  The reference runs one 16 x 16 thread block per tile
                                 (splat.jl:224-231, threads = (16, 16)); here one wave64 composites a tile, four pixels per lane in four
                                 16 x 4 strips.  0 (default) automatic:
                                 (a) a grid with fewer tiles than the chip has wave slots (256 CUs x 4 SIMDs x 5) leaves slots idle and every
                                     wave runs alone on its SIMD: 4 waves share a tile when 4 x tiles fit the slots, else 2 when 2 x tiles fit,
                                     each owning two strips or one and walking the tile's list on its own (the entries a wave evaluates are
                                     tested against ITS pixels, so pixels may differ from the one-wave result by contributions below 2^-27
                                     -- the no-op rule of alpha_cull).  Once the frame's VIEW SLOT has history, the BACKWARD of every tile
                                     runs instead as two segments of its list (x pixel parts where they still fit): the forward's waves
                                     leave a snapshot (C, T) of their pixels at the boundary, the second segment starts from it (a list of
                                     two or three batches is cut after its first batch, longer ones at 5/8 of the slot's previous walk), and
                                     a wave keeps two entries in flight (it is alone on its SIMD there: the per-entry chain is latency);
                                 (b) on larger grids the launch order (schedule 3 / 4) gives the FEW tiles whose work stands far above an
                                     even share -- a trained scene's heavy tail -- two or four waves (by strips) in the forward, and up to
                                     eight list segments in the backward (snapshots as above); a spatially uniform scene splits nothing.
                                 Gradients of a tile shared this way differ from the one-wave result by the order of the additions
                                 (<= 1e-5 relative; bitwise reproducible run to run in deterministic mode).
                                 1: always one wave per tile (what cross-mode bit-identity tests pin); 2, 4: that many pixel parts on every
                                 tile (small grids only).  Always 1 for frames without the early-out (t_min = 0), frames binned in depth
                                 slabs and capped lists.  With several waves per tile the forward's per-tile work counters are those of the
                                 tile's first part.                                                                                   */
    int32_t reserved[3];      /* sizeof(gs_config) == 96                                                                       */
} gs_config;
#define GS_DEBUG_WIDE_CURSORS 1   /* two-level binning: 64-bit list cursors although the lists fit 32-bit byte offsets (tests)    */
#define GS_DEBUG_ALWAYS_ORDER 2    /* longest-first launch orders (and their side stream) also on grids with fewer tiles than wave slots (tests) */
#define GS_DEBUG_SUPER16 8          /* two-level binning with super-tiles of 16 x 16 tiles whatever the grid (default: on grids whose 8 x 8 super-tiles
                                      would be more than 256, i.e. 4K-class images); GS_DEBUG_SUPER8 16: 8 x 8 whatever the grid (tests) */
#define GS_DEBUG_SUPER8 16
#define GS_DEBUG_TINY_CAPS 4       /* capped lists with the minimum cap on every tile, history or not: every tile that walks more than its
                                      first segment extends its list in the composite kernel (tests)                               */
#define GS_DEBUG_NO_TAIL_FILL 32   /* no zero fills at the end of the composite launches' grids: the 2-D gradient rows are cleared by a fill command in
                                      front of the composite backward and the per-gaussian kernel of an overwriting backward writes the zeros of the
                                      untouched SH rows itself -- the in-line forms; same results bit for bit (A/B runs, tests)         */

typedef struct gs_ctx gs_ctx;

/* Fill cfg with the defaults above. */
void gs_default_config(gs_config *cfg);

int gs_abi_version(void);

/* getRenderer: create a renderer context on HIP device `device`. */
int gs_create(gs_ctx **out, int device, const gs_config *cfg);
int gs_destroy(gs_ctx *ctx);
const char *gs_last_error(const gs_ctx *ctx);   /* ctx may be NULL: last gs_create error */

/* Use an existing hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream; GS_STREAM_LEGACY
 * (= hipStreamLegacy) = the device's default (null) stream.  Switching streams synchronises the old one; setting
 * the stream that is already in use returns at once, so a host may call this before every frame. */
#define GS_STREAM_LEGACY ((void *)1)
int gs_set_stream(gs_ctx *ctx, void *hip_stream);
int gs_synchronize(gs_ctx *ctx);

/* Model (SplatData3D, splat.jl:36-43).  means 3xN, scales 3xN (log), quats 4xN (w,x,y,z, not
 * normalised by the kernels), opacities 1xN (logit), shs (3*K)xN with K=(sh_degree+1)^2 and
 * element [c + 3k] = channel c of coefficient k (splat.jl:117 for degree 1).
 * GS_MEM_HOST: copied once and kept resident.  GS_MEM_DEVICE: borrowed (the caller keeps them
 * alive and may update them in place between frames, e.g. an optimiser step). */
int gs_set_model(gs_ctx *ctx, int64_t n, int sh_degree,
                 const float *means, const float *scales, const float *quats,
                 const float *opacities, const float *shs, int mem);

/* The 2-D image-fitting renderer (RendererType GAUSSIAN_2D; renderer.jl:7-18, SplatData2D splat.jl:20-26): means 2xN
 * in [0,1]^2 (pixel position (W*mx, H*my), splat.jl:337-339), scales 2xN (log, cov2d.jl:14-17), rotations 1xN (theta,
 * cov2d.jl:5), opacities 1xN (used raw, splat.jl:341: alpha = opacity*exp(-dist/2), clamped to [0, 1 - 2^-24] so that a step
 * of the optimiser cannot push alpha to 1 or below 0; the clamp has zero gradient outside), colors 3xN.  After this call gs_preprocess runs cov2d.jl:3-45 + boundingbox.jl on the
 * pixel position, gs_bin builds the lists in gaussian-index order (there is no depth), gs_forward / gs_backward use the
 * same composite kernels, and every gs_grads argument is read as SplatGrads2D (splat.jl:28-34):
 *   d_means 2xN, d_scales 2xN, d_quats -> d_rotations 1xN, d_opacities 1xN, d_shs -> d_colors 3xN.
 * Needs gs_set_image_size (or gs_set_camera, of which only W and H are used). */
int gs_set_model_2d(gs_ctx *ctx, int64_t n, const float *means, const float *scales, const float *rotations,
                    const float *opacities, const float *colors, int mem);

/* The ACTIVE SH degree (3-D renderer; after gs_set_model_2d both calls return GS_ERR_UNSUPPORTED): render and train a model below the
 * degree it stores -- the SH degree schedule of a training run, or a viewer drawing a degree-3 model at degree 0.
 * degree: -1 (the default: the model's own degree) or 0..3, anything else GS_ERR_INVALID.  The effective degree is
 * requested < 0 ? model degree : min(requested, model degree); gs_get_active_sh_degree returns it (negative: an error).  The request is
 * the ctx's: it survives gs_set_model, also onto a model of another size or degree.  With Ka = (active+1)^2, Ks = (stored+1)^2:
 *   forward   the colour is the sum over the bands k < Ka in the usual order; the rows of `shs` stay 3Ks floats apart.  Payload, lists, image
 *             and gradients are bit for bit those of the model truncated to its first 3Ka floats per row.
 *   backward  floats j < 3Ka of a d_shs row: the truncated model's; the colour -> direction term uses k < Ka.  Floats j >= 3Ka: +0.0 under
 *             GS_BWD_OVERWRITE, neither read nor written when accumulating and in gs_backward_sgd.  gs_backward_adam keeps its contract:
 *             it steps the inactive floats of every row it steps with a gradient of +0 (the moments decay), as gs_adam_step does with the
 *             stored zeros.  gs_sh_grads_from_views / _from_touched: bands < Ka rebuilt, the rest +0 (overwrite) or untouched (accumulate).
 * A call that changes the effective degree drops the frame to before gs_preprocess (as an optimiser step does); one that does not
 * returns at once and keeps the frame. */
int gs_set_active_sh_degree(gs_ctx *ctx, int degree);
int gs_get_active_sh_degree(const gs_ctx *ctx);

/* The BACKGROUND colour (both renderers; default 0, 0, 0: the reference composites over black, splat.jl:224-261).  With C = sum c_i alpha_i T_i
 * and T = prod (1 - alpha_i) as the composite kernels leave them, gs_forward gives
 *   image[c][p] = C[c][p] + (T[p] * bg[c])        one fp32 multiply, then one fp32 add, never fused; transmittance unchanged,
 * in the ctx's or the bound image and in whatever it copies out; with bg = 0 nothing is added and nothing is launched.  The backward needs no
 * argument: it reads the image the forward left, and its gradients are those of sum (C + T bg) . dC.  No gradient with respect to bg.
 * rgb: three HOST floats; a non-finite one is GS_ERR_INVALID and changes nothing.  The request is the ctx's: it survives gs_set_model and a
 * density restructure.  A value that differs from the current one drops the image, not the lists: the frame falls back to after gs_bin, and
 * a backward asks for gs_forward first.  The same value returns at once and keeps the frame. */
int gs_set_background(gs_ctx *ctx, const float rgb[3]);
int gs_get_background(const gs_ctx *ctx, float rgb[3]);
/* A target with straight (non-premultiplied) alpha over the ctx's background, for the loss of a frame rendered over it: rgba planar
 * [4, H, W] and rgb_out planar [3, H, W] (the image layout), both DEVICE and not overlapping; with a = rgba[3][p]
 *   rgb_out[c][p] = (rgba[c][p] * a) + (bg[c] * (1 - a))        four fp32 operations, each rounded on its own, in this order.
 * Runs on the ctx stream, needs no frame and no model, does not synchronise. */
int gs_compose_target(gs_ctx *ctx, const float *rgba, int32_t W, int32_t H, float *rgb_out);

int gs_set_image_size(gs_ctx *ctx, int32_t W, int32_t H);

/* Camera + image size (forward.jl:41,53-62).  T, P: 16 floats each, column-major. */
int gs_set_camera(gs_ctx *ctx, const float T[16], const float P[16], float fx, float fy,
                  float near_, float far_, const float eye[3], const float lookAt[3],
                  int32_t W, int32_t H);

/* Optional: name the view about to be rendered (call before gs_preprocess; e.g. the `id` of the camera in cameras.json,
 * camera.jl:119-151).  A training loop cycles over a fixed camera set, and how the work of a frame is spread over the tiles is a
 * property of the view: the ctx keeps, per slot 0 .. GS_MAX_VIEW_SLOTS - 1, the longest-first tile order of the last frame
 * rendered under that slot and launches the next forward of the same slot in that order (gs_config.schedule 3 / 4), and how
 * many entries of its list each tile walked, which caps the lists gs_bin writes for the slot's next frame (gs_config.list_cap).  Speed
 * only -- a stale or wrong slot costs nothing but the benefit.  slot < 0 (default): the frame belongs to no slot.  A slot costs
 * three arrays of one word per tile (100 KB at 1080p), allocated when it is first rendered. */
#define GS_MAX_VIEW_SLOTS 4096
int gs_set_view_slot(gs_ctx *ctx, int32_t slot);

/* preprocess(renderer): projection, 2-D covariance + inverse, bounding box, SH colour,
 * sigmoid, depth key, tile rectangle. */
int gs_preprocess(gs_ctx *ctx);

/* compactIdxs(renderer, threads, blocks): per-tile splat lists = tile|depth keys, stable
 * radix sort, tile ranges.  gx, gy = the reference's `blocks`; pass 0,0 for ceil(W/16),
 * ceil(H/16). */
int gs_bin(gs_ctx *ctx, int32_t gx, int32_t gy);

/* Optional: the forward writes image [3,H,W] and transmittance [H,W] DIRECTLY into these caller-owned DEVICE buffers instead of
 * the ctx's own (and gs_backward reads them back from there), which saves the two device-to-device copies of
 * gs_forward(..., GS_MEM_DEVICE).  Contract: the buffers stay valid and unmodified from gs_forward until the last
 * gs_backward of the frame; size them for the image set with gs_set_camera.  Passing the bound pointers to gs_forward is
 * allowed (no copy).  NULL, NULL unbinds.  (The reference keeps imageData / transmittance in the renderer, renderer.jl:89-117;
 * this is the same ownership with the host's allocator.) */
int gs_bind_outputs(gs_ctx *ctx, float *image_dev, float *transmittance_dev);

/* forward(renderer, tps, threads, blocks): per-tile alpha composite.  image: W*H*3 floats
 * (planar), transmittance: W*H floats.  Either may be NULL. */
int gs_forward(gs_ctx *ctx, float *image, float *transmittance, int mem);

typedef struct {              /* SplatGrads3D, splat.jl:45-52; any pointer may be NULL       */
    float *d_means;           /* 3 x N                                                        */
    float *d_scales;          /* 3 x N                                                        */
    float *d_quats;           /* 4 x N                                                        */
    float *d_opacities;       /* 1 x N                                                        */
    float *d_shs;             /* 3K x N                                                       */
} gs_grads;

/* backward(renderer, dC): dC is W*H*3 (same layout as the image).  Gradients ACCUMULATE (+=)
 * into `grads` (DEVICE pointers), exactly as the reference's grads persist until resetGrads.
 * Requires gs_forward on the same frame. */
int gs_backward(gs_ctx *ctx, const float *dC, int mem, const gs_grads *grads);

/* gs_backward with flags.  GS_BWD_OVERWRITE: store the gradients instead of accumulating -- for
 * the first backward after a reset, so the caller can skip the zero fill and this pass skips
 * the read of the old values (the result equals reset + accumulate). */
#define GS_BWD_OVERWRITE 1
/* Split backward, so a multi-GPU host can start exchanging the colour gradients while the per-gaussian chain still runs:
 * GS_BWD_COMPOSITE_ONLY stops after the composite adjoint (the per-gaussian 2-D sums exist: gs_color_grads_pack,
 * GS_ARR_GRAD2D; grads may be NULL); GS_BWD_PARAMS_ONLY runs only the chain from those sums to `grads` (dC may be NULL). */
#define GS_BWD_COMPOSITE_ONLY 2
#define GS_BWD_PARAMS_ONLY 4
/* With GS_BWD_PARAMS_ONLY, the chain in two steps so that a multi-GPU host can start the all-reduce of d_shs (81 % of the
 * gradient buffer at SH degree 3) while the geometry chain still runs: GS_BWD_PARAMS_SH runs only the SH / colour kernel
 * (d_shs and the colour -> position term), GS_BWD_PARAMS_GEOM only the geometry chain (after a GS_BWD_PARAMS_SH call of the
 * same frame).  Neither bit = both, in that order. */
#define GS_BWD_PARAMS_SH 8
#define GS_BWD_PARAMS_GEOM 16
int gs_backward_ex(gs_ctx *ctx, const float *dC, int mem, const gs_grads *grads, int flags);
/* Backward AND the optimiser step of train.jl:39-46 in one pass (3-D renderer, single-view steps): the per-gaussian kernels apply
 * param = fma(-lr, gradient, param) to the resident model instead of storing gradients -- bit-identical to gs_backward
 * (GS_BWD_OVERWRITE) followed by gs_sgd_step, at one read-modify-write of the 59 N parameter floats instead of three passes. */
int gs_backward_sgd(gs_ctx *ctx, const float *dC, int mem, float lr);

/* resetGrads: zero the arrays of `grads` (DEVICE pointers) on the ctx stream. */
int gs_reset_grads(gs_ctx *ctx, const gs_grads *grads);

/* initGrads (splat.jl:137-156) for hosts without their own device allocator: allocates ONE flat
 * zeroed device buffer [d_means 3N | d_scales 3N | d_quats 4N | d_opac N | d_shs 3K*N] owned by
 * the ctx (freed by gs_destroy or the next gs_grads_alloc) and points `out` into it.
 * gs_grads_read copies gradient arrays back to HOST buffers (any may be NULL); synchronises. */
int gs_grads_alloc(gs_ctx *ctx, gs_grads *out);
int gs_grads_read(gs_ctx *ctx, const gs_grads *grads, float *h_means, float *h_scales, float *h_quats,
                  float *h_opacities, float *h_shs);

/* ---- multi-GPU: one camera view per GPU, ONE all-reduce of the gradients -------- */

/* RCCL (librccl.so.1, loaded on first use) over xGMI.  Rank 0 calls gs_comm_unique_id and hands
 * the 128 bytes to the other ranks by any host transport; every rank then calls gs_comm_init on its
 * own ctx (one process per GPU).  gs_allreduce_grads sums the gradient arrays across ranks on the ctx
 * stream: a single ncclAllReduce when `grads` is one contiguous buffer
 * [d_means 3N | d_scales 3N | d_quats 4N | d_opac N | d_shs 3K*N] (the layout of gs_grads_alloc and of
 * the Python mirror), else one per array. */
/* Colour-factored exchange (optional; same gradients, ~2.6x less xGMI traffic at SH degree 3).  The SH gradient of one
 * view is basis_k(dir_view) * d rgb[c], so instead of all-reducing the 3K floats per gaussian (81 % of the buffer) the
 * ranks all-gather the THREE floats d rgb per (view, gaussian) and every rank rebuilds sum_v basis(dir_v) (x) d rgb_v:
 *   per view:  gs_backward with grads.d_shs = NULL (everything else accumulates as usual), then
 *              gs_color_grads_pack(ctx, drgb_view)            3 x N floats, DEVICE
 *   per step:  all-reduce of [d_means | d_scales | d_quats | d_opacities] (11 N floats), all-gather of the packed d rgb,
 *              gs_sh_grads_from_views(ctx, nviews, cams, drgb_all, d_shs, flags)
 * cams: HOST, nviews records of GS_VIEW_RECORD_FLOATS floats {T[16], P[16], eye[3], lookAt[3]} in the order of drgb_all
 * ([nviews][3 x N], DEVICE); flags: GS_BWD_OVERWRITE stores, 0 accumulates into d_shs (DEVICE, 3K x N). */
#define GS_VIEW_RECORD_FLOATS 38
int gs_color_grads_pack(gs_ctx *ctx, float *drgb);
int gs_sh_grads_from_views(gs_ctx *ctx, int32_t nviews, const float *cams, const float *drgb, float *d_shs, int flags);
/* Touched-rows exchange (optional; the colour-factored exchange with fewer bytes still).  A view's composite adjoint leaves
 * d rgb = 0 for every gaussian no pixel evaluated, so a view travels as a bitmap plus the rows of the gaussians it TOUCHED:
 *   touched:  any of the gaussian's three floats has (bit pattern & 0x7fffffff) != 0 -- +0 and -0 are untouched; denormals, NaN
 *             and Inf are touched (the bits are tested, not the float value)
 *   bits:     bit g % 32 of int32 word g / 32, ceil(n / 32) words; the bits of the last word beyond n are 0
 *   rows:     the touched rows in ascending gaussian order from row 0, copied bit for bit; rows at and beyond *count are not written
 *   per view: gs_backward as above, then gs_color_rows_pack(ctx, NULL, N, bits, rows, count) -- straight from the ctx's sums, no
 *             dense 3 x N slot (or from a caller's dense array: drgb != NULL, any n)
 *   per step: all-reduce of the 11 N geometry floats; all-gather of the counts, of the bitmaps, and of the rows padded to the
 *             largest count (rows_cap); gs_sh_grads_from_touched(ctx, nviews, cams, bits_all, rows_all, rows_cap, d_shs, flags)
 * gs_sh_grads_from_touched gives what gs_sh_grads_from_views gives on the unpacked views, bit for bit, without building them.  It
 * reads nothing outside a view's rows_cap rows whatever the bitmaps say: bits at positions >= N are ignored, a row index
 * >= rows_cap (a truncated gather) reads as a zero row, and the padding rows behind a view's count are never read.
 * Neither call synchronises; both are 3-D-renderer only (GS_ERR_UNSUPPORTED otherwise).
 * drgb: DEVICE [3 x n] or NULL = the ctx's own sums of the last backward (then n must equal gs_num_gaussians and a gs_backward of the
 * frame must have run: GS_ERR_INVALID otherwise).  bits: DEVICE, ceil(n/32) words; rows: DEVICE, room for 3*n floats; count: DEVICE.
 * n == 0: GS_OK, *count = 0. */
int gs_color_rows_pack(gs_ctx *ctx, const float *drgb, int64_t n, int32_t *bits, float *rows, int64_t *count);
/* bits: DEVICE [nviews][ceil(N/32)]; rows: DEVICE [nviews][rows_cap][3], rows_cap >= 1; cams, d_shs, flags as gs_sh_grads_from_views. */
int gs_sh_grads_from_touched(gs_ctx *ctx, int32_t nviews, const float *cams, const int32_t *bits, const float *rows,
                             int64_t rows_cap, float *d_shs, int flags);

#define GS_COMM_ID_BYTES 128
int gs_comm_unique_id(void *id128);
int gs_comm_init(gs_ctx *ctx, int rank, int nranks, const void *id128);
int gs_allreduce_grads(gs_ctx *ctx, const gs_grads *grads);
int gs_comm_destroy(gs_ctx *ctx);

/* ---- the step after backward ---------------------------------------- */

/* Loss of src/loss.jl:62-72 and its gradient w.r.t. the rendered image:
 *   loss = (1-lam) * sum|img-gt| / (2*length) + lam * (1 - mean ssim) / 2,   11x11 window of loss.jl:5-12.
 * img, gt, dC: W*H*C floats in the image layout (x fastest, channel planes); dC may be NULL.
 * loss_out (HOST, may be NULL): receives the loss; when non-NULL the call synchronises. */
int gs_loss_l1_dssim(gs_ctx *ctx, const float *img, const float *gt, int32_t W, int32_t H, int32_t C, float lam,
                     float *dC, double *loss_out, int mem);

/* train.jl:42-46: param .-= lr * grad on the ctx's resident model arrays (DEVICE gradients). */
int gs_sgd_step(gs_ctx *ctx, float lr, const gs_grads *grads);

/* Adam on the ctx's resident model arrays, updated in place exactly like gs_sgd_step (the ctx's frame state is dropped: the next
 * frame starts at gs_preprocess).  Six learning rates, one per parameter group:
 *   lr[0] means, [1] scales, [2] quaternions, [3] opacities, [4] SH band 0 (floats 0..2 of a d_shs row), [5] SH bands >= 1
 *   (floats 3..3K-1).  2-D renderer: means, scales, rotations, opacities, colors -> lr[4]; lr[5] is unused.
 * Moments are caller-owned: exp_avg (m) and exp_avg_sq (v) are two gs_grads-shaped sets of DEVICE arrays with the parameters' layout
 * (zero before the first step; checkpointing is the caller's copy of them).  t = step counts from 1.  The host computes, each in
 * double and rounded to float once, omb1 = 1-beta1, omb2 = 1-beta2, step_size[grp] = lr[grp] / (1-beta1^t) and
 * sqrt_bc2 = sqrt(1-beta2^t); every float is then stepped in float32, without fma contraction, with correctly rounded sqrt and '/':
 *   m = beta1*m + omb1*g;   v = beta2*v + (omb2*g)*g;   p = p - step_size[grp] * (m / (sqrt(v)/sqrt_bc2 + eps))
 * (torch.optim.Adam's order; torch forms m with lerp, so it agrees to rounding, this statement bit for bit).
 * Frozen groups: a NULL array in `grads` leaves that group's p, m and v untouched; a non-NULL gradient array with a NULL moment array
 * is GS_ERR_INVALID.  lr[grp] = 0 leaves p unchanged and still updates m and v.
 * GS_ADAM_SELECTIVE: a gaussian is live if any float of its non-NULL gradient rows (11 + 3K for 3-D) compares != 0.0f (-0 is dead,
 * NaN live); the p, m and v rows of a dead gaussian are neither read nor written.  Without the flag every row is stepped (torch).
 * GS_ERR_INVALID, with nothing written: step < 1, a beta outside [0, 1), eps not finite or not > 0, an lr negative or not finite,
 * unknown flag bits, or any two of the stepped p, g, m, v arrays overlapping. */
#define GS_ADAM_GROUPS 6
#define GS_ADAM_SELECTIVE 1
int gs_adam_step(gs_ctx *ctx, const gs_grads *grads, const gs_grads *exp_avg, const gs_grads *exp_avg_sq,
                 const float lr[GS_ADAM_GROUPS], float beta1, float beta2, float eps, int64_t step, int flags);
/* Backward AND gs_adam_step in one pass (3-D renderer: the 2-D one gets GS_ERR_UNSUPPORTED; needs gs_forward on the frame, as
 * gs_backward does): the per-gaussian kernels step p, m and v where gs_backward would store the gradient, which never reaches memory.
 * All ten moment arrays must be non-NULL; no gradient buffer is filled.  Contract: the result is bit-identical to
 * gs_backward_ex(GS_BWD_OVERWRITE) into a scratch gs_grads followed by gs_adam_step with the same arguments, dense and selective. */
int gs_backward_adam(gs_ctx *ctx, const float *dC, int mem, const gs_grads *exp_avg, const gs_grads *exp_avg_sq,
                     const float lr[GS_ADAM_GROUPS], float beta1, float beta2, float eps, int64_t step, int flags);

/* ---- density control: statistics, clone / split / prune, opacity reset (3-D renderer) ---------- */

/* The other half of the 3DGS recipe (Kerbl et al. 2023) whose rates gs_adam_step takes: the number of gaussians changes on the
 * device.  Five calls, every one a pure function of its inputs (random numbers stay with the caller), every decision a comparison
 * of stored floats and integers -- the host passes its thresholds already in log / logit space:
 *   per view:    gs_backward_ex (any non-fused backward), gs_density_accumulate
 *   per window:  gs_density_decide -> gs_density_plan (the one synchronise) -> gs_density_restructure into new arrays ->
 *                gs_set_model on them; zero the statistics
 *   now and then: gs_opacity_reset
 * The 2-D renderer gets GS_ERR_UNSUPPORTED.  Not covered: accumulation inside the fused backwards (gs_backward_sgd / _adam leave
 * no frame to accumulate from), multi-GPU restructuring (deterministic given equal noise, so replicated ranks may each run it). */
typedef struct {            /* caller-owned DEVICE arrays of N elements; zero them to start a window */
    float   *grad_sum;      /* sum over accumulated views of |d L / d mu'| in NDC units                */
    int32_t *count;         /* views in which the gaussian was visible                                 */
    int32_t *max_extent;    /* largest pixel extent seen                                               */
} gs_density_stats;

typedef struct {
    int32_t struct_size;        /* = sizeof(gs_density_params)                                         */
    float grad_threshold;       /* densify when grad_sum >= grad_threshold * count and count > 0       */
    float log_split_scale;      /* densified: split when max_j scale_j > this (log space), else clone  */
    float log_shrink;           /* children of a split: scale_j - log_shrink (3DGS: log 1.6)           */
    float min_opacity_logit;    /* prune when opacity < this                                           */
    float log_max_world_scale;  /* prune when the scale that would remain > this; +Inf = off           */
    int32_t max_extent_px;      /* prune when max_extent > this; 0 = off                               */
} gs_density_params;

/* After a backward of the frame (GS_ERR_INVALID before one; the fused backwards drop the frame), per gaussian, with row = the
 * gaussian's GS_ARR_GRAD2D row (d L / d mu' in pixels at [4], [5]), every operation rounded on its own, sqrt correctly rounded:
 *   grad_sum += sqrt(((0.5f*W)*row[4])^2 + ((0.5f*H)*row[5])^2);   visible = the view's pixel box is not empty;
 *   count += visible;   max_extent = max(max_extent, visible ? max(xmax - xmin, ymax - ymin) + 1 : 0).   No synchronise. */
int gs_density_accumulate(gs_ctx *ctx, const gs_density_stats *stats);

/* action[g] (DEVICE, N words) = 0 keep, 1 clone, 2 split, 3 prune.  With smax = max_j scales[g][j]:
 *   dens   = count > 0 && grad_sum >= grad_threshold * (float)count;     split = dens && smax > log_split_scale;
 *   remain = split ? smax - log_shrink : smax;
 *   prune  = opacity < min_opacity_logit || (max_extent_px > 0 && max_extent > max_extent_px) || remain > log_max_world_scale;
 *   action = prune ? 3 : split ? 2 : dens ? 1 : 0        (a NaN compares false everywhere: a NaN gaussian is kept)
 * GS_ERR_INVALID: struct_size, a NaN grad_threshold or log_shrink.  No synchronise. */
int gs_density_decide(gs_ctx *ctx, const gs_density_stats *stats, const gs_density_params *params, int32_t *action);

/* counts (HOST) = {survivors (actions 0 and 1), clones, splits, pruned}; n_out = survivors + clones + 2 * splits (a split source is
 * replaced by its two children).  Leaves the output offsets in ctx scratch, tagged with (action, N); the one call of the five that
 * synchronises.  An action outside 0..3: GS_ERR_INVALID, no plan. */
int gs_density_plan(gs_ctx *ctx, const int32_t *action, int64_t counts[4]);

/* Writes the restructured model into dst_model (five DEVICE arrays of n_out rows, the model's layouts) and up to four gradient-shaped
 * companion sets (Adam's moments) from src_sets into dst_sets (nsets 0..4; an array that is NULL on either side is skipped).  Rows:
 * the survivors in ascending source order, then the clones in ascending source order, then for every split source in ascending
 * order its child 0 and its child 1.  Survivors and clones are copied bit for bit.  Child c of source g copies quaternion, opacity and
 * SH row; scale_j - log_shrink;  mean_i + w_i with e_j = exp(scale_j) * noise[(2g + c) * 3 + j] (the preprocess's exp),
 * w_i = (R[i][0]*e_0 + R[i][1]*e_1) + R[i][2]*e_2 and R the rotation the preprocess forms from the raw quaternion.  Companion rows of
 * survivors are copied, those of clones and children are +0.  noise: DEVICE [N][2][3] standard normals, read for split sources only
 * (NULL is fine when the plan has no split).  log_shrink is the one of the ctx's last successful gs_density_decide (the call that
 * produces split actions); before any, 3DGS's (float)log(1.6).
 * GS_ERR_INVALID, nothing enqueued: no plan for (action, N) -- gs_set_model, a step of the optimiser or a new camera drop it --, n_out
 * differs from the plan's, or a destination overlaps the model, a source set or another destination.  The ctx's model is NOT
 * switched: call gs_set_model on the new arrays.  No synchronise. */
int gs_density_restructure(gs_ctx *ctx, const int32_t *action, const float *noise, const gs_grads *dst_model, int32_t nsets, const gs_grads *src_sets, const gs_grads *dst_sets, int64_t n_out);

/* opacity = opacity > max_logit ? max_logit : opacity on the resident model (a NaN stays); +0 into the gaussians' words of the two
 * moment arrays (DEVICE, N floats; either may be NULL).  The frame is dropped, as after an optimiser step.  No synchronise. */
int gs_opacity_reset(gs_ctx *ctx, float max_logit, float *m_opac, float *v_opac);

/* ---- MCMC densification: relocate, grow, noise, regularisers (3-D renderer) ---------- */

/* The other densification strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al. 2024): a fixed budget of
 * gaussians, dead ones relocated onto live ones drawn with probability proportional to opacity, growth by the same draw, noise shaped by
 * every gaussian's covariance after every step, two L1 regularisers that let unused gaussians die.  Five calls, every one a pure function
 * of its inputs (random numbers stay with the caller), on the ctx stream, device pointers throughout:
 *   per iteration:  any non-fused backward, gs_mcmc_regularize into its gradients, the optimiser step, gs_mcmc_noise
 *   per interval:   gs_mcmc_plan (the one synchronise) -> gs_mcmc_sample -> gs_mcmc_relocate
 *   growth:         gs_mcmc_sample m sources; arrays of N + m rows, the first N copied, moment rows past N zero; gs_set_model on them;
 *                   gs_mcmc_relocate with dst = N .. N + m - 1
 * sig = e / (1 + e) with e = the preprocess's exp of the logit opacity, as everywhere.  The 2-D renderer gets GS_ERR_UNSUPPORTED. */

/* Weights, their prefix sum and the dead list.  alive = opacity > min_opacity_logit (a NaN is not alive);
 *   w = alive && sig is finite ? (uint32_t)floorf(sig * 16777216.0f) : 0    -- integers: the sums below are exact in any order;
 *   cdf[i] (N words) = w[0] + ... + w[i];   dead (N words) = the indices of the gaussians that are not alive, ascending; the words past
 *   their number are left unwritten;   counts (HOST) = {alive, dead, cdf[N-1]}.
 * The ctx remembers (dead, N, the dead count) as the current plan; gs_set_model, a step of the optimiser, gs_mcmc_noise, a relocation
 * or a new camera drop it.  The one call of the five that synchronises.  GS_ERR_INVALID: a NaN threshold, a NULL array. */
int gs_mcmc_plan(gs_ctx *ctx, float min_opacity_logit, uint64_t *cdf, int32_t *dead, int64_t counts[3]);

/* m draws from a CDF of n words (total = cdf[n-1]): with uc = u[j] clamped into [0, 1 - 2^-24] (a NaN: 0),
 *   t = min((uint64_t)((double)uc * (double)total), total - 1);   src[j] = the smallest i with cdf[i] > t
 * -- one binary search per draw.  total == 0 (decided on the device), n == 0 or m == 0: GS_OK, nothing written.  No synchronise. */
int gs_mcmc_sample(gs_ctx *ctx, const uint64_t *cdf, int64_t n, const float *u, int64_t m, int32_t *src);

/* In place on the resident model: gaussian dst[j] becomes a copy of src[j], j < m, and both get the opacity and scales that leave the
 * rendered result unchanged (the paper's Eq. 9).  With c[s] = the number of j with src[j] == s (counted on the device), for every source
 * with c >= 1, in DOUBLE, n = min(c + 1, 51):
 *   o = (double)sig clamped to [0, 1 - 2^-24];   p = -expm1(log1p(-o) / n);
 *   s = sum_{i=1..n} sum_{k=0..i-1} (C(i-1, k) * ((-1)^k / sqrt(k + 1))) * p^(k+1), in that loop order, p^(k+1) by repeated multiplication;
 *   pc = min(max(p, min_opacity), 1 - 2^-23);   opacity' = (float)(log(pc) - log1p(-pc));   scale_j' = (float)((double)scale_j + log(o / s)).
 * Every read sees the model as it was before the call.  Row dst[j]: means, quaternion and SH row of src[j] bit for bit, opacity' and
 * scale' of src[j].  Every source with c >= 1: opacity' and scale', its other arrays untouched.  Every other row keeps every bit.
 * dst == NULL: the first m entries of the current plan's dead list, read on the device (GS_ERR_INVALID without a plan, or with m larger
 * than its dead count).  sets: nsets (0..4) gradient-shaped companion sets (Adam's moments): every non-NULL array gets +0 in the rows of
 * the sources with c >= 1 and of all destinations, nothing else of them is written.  An entry of src or dst outside [0, N) makes that j
 * a no-op and is not counted.  Contract, not checked: the dst entries are pairwise distinct and none is a source (the plan's dead list
 * satisfies it: a dead gaussian has weight 0).  GS_ERR_INVALID, nothing enqueued: m < 0, min_opacity not in (0, 1), nsets out of range,
 * NULL src with m > 0.  The frame and the plan are dropped, as after an optimiser step (m == 0: nothing changes).  No synchronise. */
int gs_mcmc_relocate(gs_ctx *ctx, const int32_t *src, const int32_t *dst, int64_t m, float min_opacity, int32_t nsets, const gs_grads *sets);

/* mean += noise shaped by the covariance that is drawn, per gaussian, every operation a single fp32 one; z: [N][3] standard normals:
 *   gate = 1.0f / (1.0f + exp(gate_k * (sig - gate_t)));   e_j = exp(scale_j);   R = the rotation the preprocess forms from the RAW quaternion;
 *   a_j = (R[0][j]*z0 + R[1][j]*z1) + R[2][j]*z2;   b_j = (e_j*e_j) * a_j;   d_i = (R[i][0]*b_0 + R[i][1]*b_1) + R[i][2]*b_2;
 *   mean_i = mean_i + (lr*gate) * d_i      -- all three, or (one of them would not be finite) none.
 * lr == 0: GS_OK, nothing enqueued.  GS_ERR_INVALID: a non-finite argument, lr < 0, z NULL or overlapping the model.  The frame and
 * the plans are dropped, as after an optimiser step.  No synchronise. */
int gs_mcmc_noise(gs_ctx *ctx, const float *z, float lr, float gate_k, float gate_t);

/* The gradients of lambda_o * mean(sig) + lambda_s * mean(exp(scale)) with respect to the stored logit / log parameters, ADDED to the
 * caller's gradient arrays, fp32:   d_opacities += c_opacity * (sig * (1.0f - sig));   d_scales[j] += c_scale * exp(scale_j)
 * with c_opacity = (float)(lambda_o / N) and c_scale = (float)(lambda_s / (3 N)) formed by the caller.  Only d_opacities and d_scales of
 * `grads` are read; a NULL array or a zero coefficient skips that half.  GS_ERR_INVALID: NULL grads, a non-finite coefficient, an array
 * overlapping the model.  The frame stands (gs_density_accumulate and gs_backward_camera stay legal).  No synchronise. */
int gs_mcmc_regularize(gs_ctx *ctx, const gs_grads *grads, float c_opacity, float c_scale);

/* ---- point-cloud initialisation: exact 3-NN scales, a model on the device ---------- */

/* The FIRST step of the 3DGS recipe: a model from an SfM point cloud.  Means are the points, SH band 0 the point colours, quaternions the
 * identity, and every scale the mean distance to the three nearest neighbours (distCUDA2 in the original).  Both calls run on the ctx
 * stream, need no model, camera or frame and leave the ctx's frame, its plans and every frame buffer exactly as they were (their scratch
 * is the ctx's own, grow-only): they are legal between gs_forward and gs_backward.  Neither synchronises.  All pointers are DEVICE pointers.
 *
 * gs_knn_mean_dist2.  points: 3 x N, the component fastest; dist2: N floats, not overlapping points.  A point is finite if its three
 * coordinates are; m = the number of finite points.  With every operation a single fp32 operation rounded on its own, no contraction:
 *   dx = xi - xj (dy, dz likewise);   d2(i, j) = ((dx*dx + dy*dy) + dz*dz)        (an overflowed square is +Inf and takes part as such)
 * For a finite point i and m >= 4, with b0 <= b1 <= b2 the three smallest values of the multiset { d2(i, j) : j != i, j finite } --
 * j != i by INDEX: a duplicate of i counts, with distance 0 --
 *   dist2[i] = ((b0 + b1) + b2) / 3.0f
 * A function of a multiset of individually rounded values: it does not depend on the search order and equals a brute-force evaluation
 * bit for bit.  m >= 4, point i not finite: dist2[i] = NaN (any NaN).  m < 4: every dist2[i] = NaN.
 * N == 0: GS_OK, nothing enqueued.  GS_ERR_INVALID, nothing written: a NULL pointer, N < 0, dist2 overlapping points.
 * GS_ERR_UNSUPPORTED: N > 2^31 - 1. */
int gs_knn_mean_dist2(gs_ctx *ctx, const float *points, int64_t n, float *dist2);

/* colors: 3 x N rgb in [0, 1], or NULL for grey 0.5; dist2: what gs_knn_mean_dist2 left; dst_model: five arrays of N rows in the model's
 * layouts, passed as gs_density_restructure takes them (d_shs: 3 (sh_degree + 1)^2 floats per row).  Per point, bit for bit but the scales:
 *   means = the point;   v = dist2 > 1e-7f ? dist2 : 1e-7f  (a NaN gives 1e-7f);   scales[0..2] = (float)(0.5 * log((double)v)), within
 *   1 float ulp of the correctly rounded value;   quats = (1, 0, 0, 0);   opacities = opacity_logit (the host passes the logit, as the
 *   density calls take theirs);   shs[c] = (rgb[c] - 0.5f) / SH_C0 for c < 3, one subtract and one correctly rounded divide by
 *   SH_C0 = 0.28209479177387814f -- the inverse of the + 0.5 of the preprocess -- or +0.0 with NULL colours;   shs[3 ..] = +0.0.
 * GS_ERR_INVALID, nothing written: sh_degree outside 0..3, N < 0, a NULL points, dist2 or destination, any overlap between destinations
 * or of one with a source.  The ctx's model is NOT switched: call gs_set_model on the new arrays. */
int gs_init_from_points(gs_ctx *ctx, const float *points, const float *colors, const float *dist2, int64_t n,
                        int sh_degree, float opacity_logit, const gs_grads *dst_model);

/* ---- feature maps: depth, opacity and per-gaussian features, with gradients (3-D renderer) ---------- */

/* The composite forward computes C = sum c_g alpha T for three per-gaussian floats; that they are colours is the preprocess's business.
 * These calls run a FINISHED frame's composite launches over a second, ctx-owned payload whose three colour floats are the caller's: the
 * same tile lists, entries, order, early-out (t_min) and no-op rule (alpha_cull) as the frame's forward, so a depth or opacity map is
 * consistent with the colour image pixel by pixel.  Features wider than three are rendered in triples.  All four calls: 3-D renderer only
 * (GS_ERR_UNSUPPORTED after gs_set_model_2d), every pointer a DEVICE pointer, work enqueued on the ctx stream, no synchronise.
 *
 * gs_view_depth.  z: N floats; z[g] = ts[2], the view-space depth of gaussian g, as the preprocess states it -- with m the mean and T
 * column major, every step a single fp32 operation:
 *   s = T[2]*m1;  s = s + T[6]*m2;  s = s + T[10]*m3;  s = s + T[14]*1.0f
 * equal to row 2 of GS_ARR_TS bit for bit (non-finite means pass through as IEEE gives them).  Needs a model and a camera, no frame, and
 * leaves the frame alone.  gs_view_depth_backward is its adjoint: d_means[3g+j] = d_means[3g+j] + (T[2+4j] * dz[g]), one multiply and one
 * add; a dz[g] that compares == 0 leaves row g unread (the "untouched" rule of the per-gaussian chain). */
int gs_view_depth(gs_ctx *ctx, float *z);
int gs_view_depth_backward(gs_ctx *ctx, const float *dz, float *d_means);

/* gs_render_features.  feat: 3 x N, component fastest; out: [3, H, W] planar (the image layout); trans_out: [H, W] or NULL.
 *   out[c][p] = sum over the frame's entries of feat[c][g] * alpha * T        no background is added; trans_out = the frame's transmittance
 * Needs a frame at gs_forward or later (GS_ERR_INVALID otherwise) and is legal before, between and after its backward calls.  With
 * feat = GS_ARR_RGB and one wave per tile (gs_config.tile_parts = 1) out and trans_out equal the frame's image (over black) and
 * transmittance bit for bit; with tiles shared between waves, within the no-op rule of tile_parts.  The features should be finite: the
 * composite kernels mask arithmetically, so a NaN or Inf feature of a LISTED gaussian reaches the pixels of the tiles that list it.
 * The frame is left exactly as gs_forward left it: image, transmittance, work counters, the view slot's history, launch orders,
 * snapshots and gradient sums; the ctx pays one payload copy (64 B per gaussian) of scratch.
 * GS_ERR_UNSUPPORTED, nothing enqueued: a frame binned in depth slabs (gs_num_rounds > 1) -- a caller that renders feature maps sets
 * gs_config.slab_mode = 0.  GS_ERR_INVALID, nothing enqueued: a NULL feat or out; out or trans_out overlapping the frame's image or
 * transmittance (the ctx's own or the bound ones) or each other. */
int gs_render_features(gs_ctx *ctx, const float *feat, float *out, float *trans_out);

/* gs_backward_features.  The gradients of sum out . dF for the `out` gs_render_features wrote for this `feat` on this frame (image_f; dF:
 * [3, H, W]).  d_feat (3 x N) is OVERWRITTEN with d / d feat; the alpha-path gradients ACCUMULATE (+=) into grads->d_means, d_scales,
 * d_quats and d_opacities (any may be NULL, as may grads); d_shs is neither read nor written -- the features do not depend on the model
 * here: a caller whose features do (depth) chains d_feat itself (gs_view_depth_backward).  The composite adjoint runs over whole tiles into
 * auxiliary gradient sums of the frame's mode, then the geometry chain alone runs over them; the call is legal before, between or after
 * the frame's colour backward calls (also between GS_BWD_PARAMS_SH and GS_BWD_PARAMS_GEOM) and changes nothing they read or write apart
 * from the accumulation into `grads`.  gs_config.deterministic: bitwise reproducible run to run; the fixed-point sums hold +-8.4e6 in the
 * first six words of a row (d feat, and the moments of order 0 and 1), and what they hold scales with |feat| * |dF| -- a depth feature
 * in scene units of thousands wants dF scaled down accordingly.  Refusals as gs_render_features (a NULL feat, image_f, dF or d_feat). */
int gs_backward_features(gs_ctx *ctx, const float *feat, const float *image_f, const float *dF, float *d_feat, const gs_grads *grads);

/* gs_backward_camera.  The gradient of the frame's loss with respect to the arguments of gs_set_camera, taken as independent inputs: pose
 * refinement, registering a new photograph against a trained model.  out: GS_CAMERA_GRAD_FLOATS floats, OVERWRITTEN (a camera gradient
 * belongs to one view), in the order of a view record and two more:
 *   [0..15] d_T   [16..31] d_P  (column major, like T and P)   [32..34] d_eye   [35..37] d_lookAt   [38] d_fx   [39] d_fy
 * each the sum over the gaussians of the statement in csrc/gs_camera_grad.h (d_T[i + 4 j] = sum dt[i] * [m; 1][j], d_P[i + 4 j] = sum dp[i] * t[j],
 * d_eye = - d_lookAt = the colour path's direction term), evaluated in fp64 from the fp32 inputs at the ACTIVE SH degree, summed in fp64
 * in a fixed tree without atomics and rounded to float once: the 40 floats are a pure function of the frame's rows of 2-D gradient sums,
 * the model and the camera, bitwise reproducible call to call (and run to run with gs_config.deterministic).  The fourth row of T is zero
 * in the reference's cameras; its gradient row is still the formal one.  near and far have no gradient (they only cull).
 * Needs the frame's colour backward: a gs_backward / gs_backward_ex on this frame that ran the composite adjoint (GS_BWD_COMPOSITE_ONLY is
 * enough) -- else GS_ERR_INVALID "gs_backward first".  MUST be called before anything steps the model: the chain is recomputed from the
 * RESIDENT parameters (gs_sgd_step and gs_adam_step on the ctx's own arrays change them under the frame; the fused gs_backward_sgd and
 * gs_backward_adam drop the frame, so after them the call is refused).  3-D renderer only (GS_ERR_UNSUPPORTED).  Every refusal is made before
 * anything is enqueued or allocated.  The call reads the frame and writes `out` and scratch of its own: image, transmittance, gradient
 * sums, stage, view-slot history and stage timers stay as they were.  GS_MEM_HOST synchronises, GS_MEM_DEVICE does not.  N = 0: 40 x +0. */
#define GS_CAMERA_GRAD_FLOATS 40
int gs_backward_camera(gs_ctx *ctx, float *out, int mem);

/* ---- evaluation metrics: PSNR, MAE and the standard SSIM of a rendered image against its target ---- */

/* gs_image_metrics.  img, gt: [C, H, W] float32 (x fastest, channel planes: the layout of the loss); weight: [H, W] float32 shared by all
 * channels, or NULL (w = 1).  sums, OVERWRITTEN, over the C H W pixel-channels:
 *   sums[0] = sum w (x - y)^2    sums[1] = sum w |x - y|    sums[2] = sum w S    sums[3] = sum w
 * S is the standard SSIM map: window g_i = exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1 in double, the 2-D window its outer
 * product; zero padding of 5 (samples outside the image contribute 0 to all five window sums); C1 = 0.01^2, C2 = 0.03^2;
 *   S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)).
 * The map is always that of the whole unweighted images: the weight enters only the four sums.  ssim_map ([C, H, W] float32, may be NULL)
 * receives the map, one rounding from the double value.  Arithmetic: the float32 samples are widened to double, and the products, the five
 * window sums, the map formula and (x - y) are evaluated in double -- a float32 SSIM is off by more than 1e-3 per pixel on nearly flat images,
 * the size of the differences models are compared by.  The sums are added without atomics in a fixed order: bitwise reproducible call to call,
 * the same through GS_MEM_HOST and GS_MEM_DEVICE, and independent of what the ctx did before.
 * GS_MEM_HOST: every pointer is a host pointer, the data is staged through the ctx and the call synchronises.  GS_MEM_DEVICE: every pointer,
 * sums included, is a device pointer; the work is enqueued on the ctx stream, no synchronise.  Needs no model, camera or frame and works
 * under both renderers; image, transmittance, gradient sums, stage, view-slot history and stage timers stay as they were.
 * GS_ERR_INVALID, nothing written, enqueued or allocated: a NULL ctx, img, gt or sums; W, H or C <= 0; C * H * W >= 2^31; a bad mem. */
#define GS_METRIC_SUMS 4
enum { GS_METRIC_MSE = 0, GS_METRIC_MAE, GS_METRIC_SSIM, GS_METRIC_PSNR, GS_METRIC_COUNT };
int gs_image_metrics(gs_ctx *ctx, const float *img, const float *gt, const float *weight, int32_t W, int32_t H, int32_t C,
                     float *ssim_map, double *sums, int mem);

/* gs_metrics_finish.  Pure host arithmetic on the four sums (no ctx, no GPU): out[GS_METRIC_MSE] = s0 / s3, out[GS_METRIC_MAE] = s1 / s3,
 * out[GS_METRIC_SSIM] = s2 / s3, out[GS_METRIC_PSNR] = -10 log10(mse) (data range 1; +inf when mse == 0).  All four are NaN when s3 is not
 * > 0.  GS_OK for non-NULL arguments, else GS_ERR_INVALID. */
int gs_metrics_finish(const double sums[GS_METRIC_SUMS], double out[GS_METRIC_COUNT]);

/* ---- per-view exposure: a learned 3 x 4 colour affine and a mask between gs_forward and the loss ---- */

/* Images are planar [3, H, W] float32 (the layout of the loss); exposure: 12 floats E, row-major 3 x 4 -- E[4 r + 0..2] row r of the matrix,
 * E[4 r + 3] its offset; weight: [H, W] float32 or NULL.  Float32 throughout, one rounding per operation, no fma contraction, in this order:
 *   gs_exposure_apply     a_r = ((E[r][0] x0 + E[r][1] x1) + E[r][2] x2) + E[r][3];   out_r = w a_r   (no weight: out_r = a_r)
 *   gs_exposure_backward  g_r = w d_r   (no weight: g_r = d_r);   d_img_k = (E[0][k] g0 + E[1][k] g1) + E[2][k] g2;   and, unless d_exposure
 *                         is NULL, d_exposure[4 r + k] = sum over the pixels of (double)g_r * (double)x_k, x_3 = 1: exact products, added
 *                         in double in a fixed order without atomics and rounded to float once.  OVERWRITTEN, 12 floats.
 * Identity E ([I | 0]) without a weight returns x for every finite x (the bits but for -0, which becomes +0); identity E with a weight
 * returns w * x exactly, which is how a target is masked.  d_img may be d_out itself (in place).  Results are bitwise reproducible call to
 * call and independent of what the ctx did before, of the alignment of the buffers and of d_exposure being asked for.
 * Every pointer is a DEVICE pointer on the ctx's device (E too: the row of a table that gs_exposure_adam has just stepped); the work is
 * enqueued on the ctx stream, no synchronise.  Needs no model, camera or frame and works under both renderers; image, transmittance,
 * gradient sums, stage, view-slot history and stage timers stay as they were.
 * GS_ERR_INVALID, nothing written, enqueued or allocated: a NULL ctx, img, exposure, out, d_out or d_img; W or H <= 0; 3 * W * H >= 2^31; out
 * overlapping img, weight or exposure; d_img overlapping img, weight, exposure or d_exposure, or d_out in any way but d_img == d_out. */
int gs_exposure_apply(gs_ctx *ctx, const float *img, const float *exposure, const float *weight, int32_t W, int32_t H, float *out);
int gs_exposure_backward(gs_ctx *ctx, const float *img, const float *d_out, const float *exposure, const float *weight, int32_t W, int32_t H,
                         float *d_img, float *d_exposure);
/* One Adam step of the 12 floats of a row from d_exposure, with its own moments exp_avg and exp_avg_sq (12 floats each, zero before the
 * first step): gs_adam_step's update and host scalars exactly (t = step counts from 1 and is the ROW's own count: a view is stepped when it
 * is rendered).  Device pointers, enqueued on the ctx stream, no synchronise; the ctx's frame stays as it was (no model array is touched).
 * lr == 0 leaves the row unchanged and still updates the moments.  GS_ERR_INVALID, nothing written: a NULL pointer, step < 1, a beta
 * outside [0, 1), eps not finite or not > 0, lr negative or not finite, any two of the four rows overlapping. */
int gs_exposure_adam(gs_ctx *ctx, float *exposure, const float *d_exposure, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, int64_t step);

/* ---- per-view bilateral grid: local colour correction between gs_forward and the loss ---- */

/* A lattice of 3 x 4 colour affines per view, indexed by pixel position and pixel luminance, sliced per pixel and applied to the colour: what
 * a single affine per view (gs_exposure_*) cannot absorb -- vignetting, local tone mapping, a blown-out corner.  Images are planar [3, H, W]
 * float32; weight: [H, W] float32 or NULL; grid: [Gz][Gy][Gx][12] float32, the 12 floats of a vertex A[r][k] row-major 3 x 4 as a row of the
 * exposure table; 1 <= Gx, Gy, Gz <= GS_BILAGRID_MAX_DIM; the identity grid has [I | 0] at every vertex.  Float32, one rounding per operation,
 * no fma contraction, in the order written in csrc/gs_bilagrid.h (restated in tests/bilagrid_ref.py):
 *   pixel (column c, row r): gx = c sx, sx = (Gx - 1) / (W - 1) (0 when W == 1), gy likewise, gz = clamp(l, 0, 1) (Gz - 1) with the luminance
 *       l = 0.299 x0 + 0.587 x1 + 0.114 x2 (a NaN l gives 0); on each axis the cell i0 = min((int)g, max(n - 2, 0)), i1 = min(i0 + 1, n - 1),
 *       f = g - i0; A = the trilinear interpolation of the eight vertex rows, as three nested a + f (b - a), x innermost: equal corners give
 *       that value exactly.  This is torch.nn.functional.grid_sample(bilinear, border, align_corners=True) at (c / (W - 1), r / (H - 1), l).
 *   gs_bilagrid_apply     a_r = ((A[r][0] x0 + A[r][1] x1) + A[r][2] x2) + A[r][3];   out_r = w a_r   (no weight: out_r = a_r)
 *   gs_bilagrid_backward  g_r = w d_r (no weight: d_r);  d_img_k = ((A[0][k] g0 + A[1][k] g1) + A[2][k] g2) + lam_k dl, where dl, the gradient
 *                         through the luminance, is (Gz - 1) sum_m dA[m] dA_m/dfz with dA[r][k] = g_r x_k (x_3 = 1) when 0 < l < 1, else 0; and,
 *                         unless d_grid is NULL, d_grid[v][4 r + k] = the sum over every (pixel, corner) whose vertex is v of
 *                         (double)u ((double)g_r (double)x_k), u the corner's trilinear weight in float32 -- added in double in a fixed order
 *                         without atomics and rounded to float once.  OVERWRITTEN, all Gz Gy Gx 12 floats: a vertex no pixel touches gets +0.
 *   gs_bilagrid_tv        tv = sum over the axes with n >= 2 of mean((G[+1] - G)^2), differences in float32, squares and sums in double, written
 *                         to tv_out (one DEVICE double; may be NULL); and, unless d_grid is NULL, the gradient of coef * tv ADDED to d_grid in
 *                         float32 (csrc/gs_bilagrid.h states the order).  coef must be finite and >= 0.
 * The identity grid without a weight returns x for every finite x (the bits but for -0, which becomes +0); with a weight it returns w * x
 * exactly.  d_img may be d_out itself (in place).  Results are bitwise reproducible call to call and independent of what the ctx did before, of
 * the alignment of the buffers, of d_img being d_out and of d_grid being asked for.
 * Every pointer is a DEVICE pointer on the ctx's device; the work is enqueued on the ctx stream, no synchronise.  Needs no model, camera or
 * frame and works under both renderers; image, transmittance, gradient sums, stage, view-slot history and stage timers stay as they were.
 * GS_ERR_INVALID, nothing written, enqueued or allocated: a NULL ctx, img, grid, out, d_out or d_img; W or H <= 0; 3 * W * H >= 2^31; a grid
 * dimension outside 1..GS_BILAGRID_MAX_DIM; out overlapping img, weight or grid; d_img overlapping img, weight, grid or d_grid, or d_out in any
 * way but d_img == d_out; d_grid overlapping img, d_out, weight or grid; in gs_bilagrid_tv a bad coef or any two of grid, d_grid and tv_out
 * overlapping. */
#define GS_BILAGRID_FLOATS 12
#define GS_BILAGRID_MAX_DIM 64
int gs_bilagrid_apply(gs_ctx *ctx, const float *img, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz, const float *weight, int32_t W,
                      int32_t H, float *out);
int gs_bilagrid_backward(gs_ctx *ctx, const float *img, const float *d_out, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz,
                         const float *weight, int32_t W, int32_t H, float *d_img, float *d_grid);
int gs_bilagrid_tv(gs_ctx *ctx, const float *grid, int32_t Gx, int32_t Gy, int32_t Gz, float coef, float *d_grid, double *tv_out);
/* One Adam step of the n_floats floats of a view's grid from d_grid, with its own moments (zero before the first step): gs_adam_step's update
 * and host scalars exactly (t = step counts from 1 and is the VIEW's own count).  Device pointers, enqueued on the ctx stream, no synchronise;
 * the ctx's frame stays as it was.  lr == 0 leaves the grid unchanged and still updates the moments.  GS_ERR_INVALID, nothing written: a NULL
 * pointer, n_floats outside 1..64^3 * 12, step < 1, a beta outside [0, 1), eps not finite or not > 0, lr negative or not finite, any two of the
 * four arrays overlapping. */
int gs_bilagrid_adam(gs_ctx *ctx, float *grid, const float *d_grid, float *exp_avg, float *exp_avg_sq, int64_t n_floats, float lr, float beta1,
                     float beta2, float eps, int64_t step);

/* ---- introspection (parity tests, profiling) ------------------------------------------- */

typedef enum {
    GS_ARR_TS = 0,            /* 4 x N  f32   view-space position            (export_debug) */
    GS_ARR_TPS = 1,           /* 4 x N  f32   clip-space position            (export_debug) */
    GS_ARR_MU = 2,            /* 2 x N  f32   renderer.positions             (export_debug) */
    GS_ARR_COV3D = 3,         /* 9 x N  f32   renderer.cov3ds                (export_debug) */
    GS_ARR_COV2D = 4,         /* 4 x N  f32   renderer.cov2ds                (export_debug) */
    GS_ARR_INVCOV = 5,        /* 4 x N  f32   renderer.invCov2ds             (export_debug) */
    GS_ARR_BBS = 6,           /* 4 x N  f32   renderer.bbs [xmin ymin xmax ymax] (export_debug) */
    GS_ARR_RGB = 7,           /* 3 x N  f32   sh2color result                                */
    GS_ARR_SIG = 8,           /* 1 x N  f32   cusigmoid(opacity)                             */
    GS_ARR_DEPTH_KEY = 9,     /* 1 x N  u32   radix key of clip z for the ctx order          */
    GS_ARR_TILE_RECT = 10,    /* 4 x N  u16   x0 x1 y0 y1, 1-based inclusive; x0=0: no tile  */
    GS_ARR_SORT_IDXS = 11,    /* 1 x N  u32   renderer.sortIdxs (0-based)                    */
    GS_ARR_TILE_RANGES = 12,  /* 2 x gx*gy u32 [start,end) into the sorted instance list     */
    GS_ARR_SORTED_IDS = 13,   /* 1 x I  u32   gaussian id per sorted instance (0-based)      */
    GS_ARR_SORTED_KEYS = 14,  /* 1 x I  u64   tile<<32 | depth key (or | id in INDEX order)  */
    GS_ARR_GRAD2D = 15        /* 10 x N f32   d{rgb3,sig,mu2,inv4} after gs_backward          */
} gs_array;

int64_t gs_num_gaussians(const gs_ctx *ctx);
int64_t gs_num_instances(gs_ctx *ctx);            /* I of the last gs_bin (waits for the frame's totals if they are still in flight) */
int64_t gs_num_coarse_instances(gs_ctx *ctx);      /* two-level binning: (super-tile, gaussian) instances of the last gs_bin, else 0 */
int gs_num_rounds(const gs_ctx *ctx);             /* binning rounds of the last gs_bin: 1 = classic full lists, 2..4 = depth slabs */

/* Copy an internal array to a HOST buffer of `bytes` bytes (synchronises). */
int gs_get_array(gs_ctx *ctx, int which, void *host_dst, int64_t bytes);

typedef enum {
    GS_STAGE_PREPROCESS = 0, GS_STAGE_DEPTH_SORT, GS_STAGE_COUNT_SCAN, GS_STAGE_EMIT,
    GS_STAGE_TILE_SORT, GS_STAGE_RANGES, GS_STAGE_COMPOSITE_FWD, GS_STAGE_COMPOSITE_BWD,
    GS_STAGE_PREPROCESS_BWD, GS_STAGE_COUNT
} gs_stage;

/* Milliseconds of the last execution of each stage (profile_stages=1); synchronises. */
int gs_get_stage_times(gs_ctx *ctx, float ms[GS_STAGE_COUNT]);

/* Accumulated hipEvent time (ms) and launch count per stage since the last reset
 * (profile_stages=1); synchronises.  reset != 0 clears the accumulators afterwards. */
int gs_get_stage_stats(gs_ctx *ctx, double sum_ms[GS_STAGE_COUNT], int64_t count[GS_STAGE_COUNT], int reset);

/* Work counters of the last frame: list entries actually walked by the composite kernels
 * (== gs_num_instances when t_min == 0; fewer with the transmittance early-out). */
int gs_get_work_counters(gs_ctx *ctx, int64_t *walked_fwd, int64_t *walked_bwd);

/* Tile lists of the last frame: out = {entries actually written into the tile lists (== gs_num_instances unless the lists were
 * capped, gs_config.list_cap; includes what composite waves appended), list segments appended by composite waves (0 when the
 * slot's history covered the frame), 1 if the frame's lists were capped else 0}.  Call after gs_forward; synchronises. */
int gs_get_list_stats(gs_ctx *ctx, int64_t out[3]);

/* Waves per tile (1, 2 or 4) of the last frame's composite launches (gs_config.tile_parts); negative: error.  Call after gs_forward.
 * No counterpart in the reference (one thread block per tile, splat.jl:224-231). */
int gs_get_tile_parts(gs_ctx *ctx);

/* The path that built the last frame's tile lists (gs_config.bin_path says what was asked for): 0 two-level binning, 1 / 2 the radix
 * paths, 3 the small-frame path (gs_bin_small.hip: one launch, one workgroup per tile, up to 128 KB of dynamic LDS; no global depth
 * order, sortIdxs on demand; taken by bin_path 0 for up to 16 384 gaussians x 1024 tiles x 4 M gaussian x tile pairs).  Same lists on
 * every path.  Negative: error.  Call after gs_bin. */
int gs_get_bin_path(gs_ctx *ctx);

/* out = {walked_fwd, walked_bwd, evaluated_fwd, evaluated_bwd}: `evaluated` counts the walked entries that
 * survived the alpha_cull no-op test and were evaluated per pixel (== walked when alpha_cull == 0). */
int gs_get_work_counters_ex(gs_ctx *ctx, int64_t out[4]);

/* Profiling aid: re-launch the composite forward (which=0) or backward (which=1) kernel of the
 * current frame `reps` times with kernel variant `variant` and return the mean hipEvent time.
 * Backward gradients of these launches go to the internal 2-D gradient scratch only. */
int gs_debug_time_composite(gs_ctx *ctx, int which, int variant, int reps, float *mean_ms);

/* Profiling aid: one launch of the composite forward (which=0) or backward (which=1) kernel of the current frame with
 * per-tile clocks.  out (HOST): 15 x gx*gy uint64 per tile {start, end (100 MHz s_memrealtime ticks), HW_ID | XCC_ID << 32,
 * walked << 32 | evaluated, shader cycles inside the per-entry loops, shader cycles outside them (staging a batch and waiting
 * for its gathers), per-entry strip slots executed << 32 | the slots needed if the tile's live pixels were packed 64 to a slot,
 * strips holding a live pixel << 32 | live pixels (the last four summed over the evaluated entries), and (forward) six words: the
 * evaluated entries by the number of 64-lane slots they would need with live pixels packed anywhere / by whole rows / inside columns,
 * and the entries that would survive the no-op test against the rectangle of the live pixels instead of the whole tile}.
 * tools/tile_tail.py turns it into the occupancy-over-time, tail and frozen-pixel summaries under profiles/. */
int gs_debug_tile_clock(gs_ctx *ctx, int which, int variant, uint64_t *out);
/* A NEGATIVE variant v runs variant -v with one record per WORKGROUP of the launch instead of per tile -- the launch as production runs
 * it, heavy tiles split into two or four waves (the parts of a split tile would overwrite each other's per-tile record): out then
 * holds gs_debug_tile_clock_rows(ctx) rows of 15 words, rows of workgroups without a tile all zero.  0: the frame has no launch order. */
int gs_debug_tile_clock_rows(gs_ctx *ctx);
/* Fill workgroups the composite launches of the last frame carried at the end of their grids: blocks[0] the forward (zero fill of the 2-D
 * gradient rows), blocks[1] the composite backward (zeros of d_shs; 0 before a backward of the frame).  0: the in-line form ran (tests). */
int gs_debug_tail_fill(gs_ctx *ctx, int32_t blocks[2]);

/* Profiling hook: the shader clock (MHz) the chip runs at right now, from one wave that counts s_memtime cycles over 20 us of
 * s_memrealtime on the ctx stream (waits for the stream).  tools/frames_probe.py samples it between frames. */
int gs_debug_clock_mhz(gs_ctx *ctx, float *mhz);

/* Profiling aid: restrict the debug launches above (gs_debug_time_composite, gs_debug_tile_clock) to the `len` workgroups of
 * the frame's longest-first launch order that start at entry `start` (a multiple of 8, so that a tile keeps its XCD); len = 0:
 * the whole order again.  Needs a frame with a launch order (gs_config.schedule 3 / 4 on a grid above the wave slots).  With it
 * tools/occupancy_curve.py launches 1024, 2048 .. 5120 tiles at once -- one to five waves per SIMD -- and reads the SIMD
 * throughput by resident waves directly instead of inferring it from tile lifetimes. */
int gs_debug_set_window(gs_ctx *ctx, int32_t start, int32_t len);

/* -1: the lane-order probe of the LDS-atomic rank was not run (rank_mode = 1 was asked for); 0: it ran at gs_create and
 * passed; 1: it failed on this device and ballots were forced. */
int gs_rank_probe_result(const gs_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_H */
