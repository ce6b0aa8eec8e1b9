/*
 * splat_hip.h -- C ABI of libsplat_hip.so, the MI355X (gfx950) Gaussian-splat
 * rasterizer (forward + backward).
 *
 * This is the drop-in boundary for the one hot path of SplaTAM: the un-vendored
 * extension `diff_gaussian_rasterization._C` (pinned at
 * /root/reference/requirements.txt:15, imported at
 * /root/reference/scripts/splatam.py:37 and /root/reference/utils/recon_helpers.py:2).
 * Each entry point below names the reference-side call it replaces.  Every
 * pointer is a raw DEVICE pointer owned by the caller (PyTorch's caching
 * allocator in the Python binding); the library never allocates, never frees,
 * never synchronises the device and launches everything on the stream it is
 * handed.  All functions return 0 on success and a SPLAT_E_* code otherwise
 * (nothing is thrown across the ABI); splat_error_string() maps codes to text.
 *
 * Conventions (/root/reference/utils/recon_helpers.py:8-13):
 *   - viewmatrix / projmatrix: 16 floats, element (row r, col c) at m[c*4+r],
 *     i.e. the bytes of the settings tensor `w2c^T` / `(P w2c)^T` as stored.
 *   - quaternions (r,x,y,z), not renormalised; opacities already in (0,1);
 *     scales already exponentiated (/root/reference/utils/slam_helpers.py:131-138).
 *   - images are planar [C][H][W] float32.
 */
#ifndef SPLAT_HIP_H
#define SPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_ABI_VERSION 17       /* 17: the hole count of a novel view (SplatEvalConfig.holes, SPLAT_EVAL_HOLES);
                                      ADDED WITHIN 17 (no struct changed, no symbol removed, so the number stays and every binding built against
                                      17 keeps working): SplatLossConfigEx, SPLAT_LOSS_SPLATAM / SPLAT_LOSS_GS, splat_iter_loss_backward_ex,
                                      splat_iter_mapping_step_ex -- the mapping loss of the refinement script (get_loss_gs);
                                      SPLAT_EVAL_LPIPS, SplatLpipsWorkspace, splat_lpips_* -- LPIPS from caller-supplied AlexNet weights (csrc/lpips.hip);
                                      splat_mesh_components, splat_mesh_component_stats -- connected components of a mesh (csrc/meshclean.hip);
                                      SPLAT_MESH_SIMPLIFY_*, splat_mesh_simplify_keys / _vertices / _quadrics / _place / _faces -- vertex clustering with quadric placement (csrc/meshsimplify.hip);
                                      SplatMeshShade, SPLAT_MESH_SHADE_*, splat_mesh_vertex_normals, splat_mesh_visibility, splat_mesh_shade -- pictures of a mesh (csrc/meshshade.hip);
                                      16: the view layer (SplatViewArgs, splat_view_camera, splat_view_finish, SPLAT_VIEW_COLOR / _DEPTH / _SILHOUETTE);
                                      15: sensor bytes to the loop's planes in one launch (splat_frame_ingest_planes, SPLAT_DEPTH_U16 / _F32);
                                      14: frame ingest (splat_frame_ingest);
                                      13: frame preparation (splat_frame_prepare);
                                      12: evaluation metrics (SplatEvalConfig, SplatEvalWorkspace, splat_eval_workspace_layout / _bind, splat_eval_metrics, splat_iter_eval);
                                      11: SplatAdamMap.one_minus_beta1 / _beta2 (torch's 1 - beta, formed in double);
                                      10: group binning behind the reference API (SplatState.group_* in splat_preprocess_forward / splat_render_forward,
                                      SPLAT_LAYOUT_GROUPS), SplatState.tile_recs (staged records handed from the forward to the backward composite), SplatCamera.bg == NULL = black, SplatGrads.flags (SPLAT_GRADS_UPSTREAM_SCALE), SplatState.status_host,
                                      SplatState.tile_order entries hold tile + 1 (a zeroed buffer is the natural order) and are laid out on request (SPLAT_LAYOUT_TILE_ORDER),
                                      SplatState.tile_queue (persistent composites: measured, not adopted, removed) is gone;
                                      9: scratch layouts (splat_workspace_bytes, splat_state_layout / _bind, splat_iter_workspace_layout / _bind);
                                      8: SplatIterWorkspace.d_cam is SPLAT_ITER_DCAM floats (loss terms, status snapshot, gated-iteration count),
                                      the Adam steps skip while the capacity flag is up (SplatAdamMap.gate), per-group bc2_sqrt;
                                      7: SplatState.long_items (work-item table of the multi-workgroup sort);
                                      6: SplatState.tile_row_begin / _end, SplatLossConfig.defer_finish, splat_iter_finish (tile-row-sharded tracking);
                                      5: SplatState.group_count / group_recs / group_stride (group binning), splat_iter_mapping_step; 4: densification (splat_iter_means2d_accumulate, splat_map_densify_select / _duplicate);
                                      3: SplatState.keys_alt / long_base (multi-workgroup sort of lists beyond LDS); 2: map edits,
                                      splat_iter_render / _tracking_step, outlier scratch in SplatIterWorkspace */
/* the words of SplatState.status */
#define SPLAT_STATUS_INSTANCES 0   /* num_rendered */
#define SPLAT_STATUS_OVERFLOW 1    /* overflow flag (num_rendered > capacity) */
#define SPLAT_STATUS_LONGEST 2     /* longest tile list */
#define SPLAT_STATUS_STALE_HINT 3  /* a list longer than the wave-sort limit met a stale max_list_hint that had skipped the long-list
                                      sort kernel (the lists are then NOT sorted: re-run) */

#define SPLAT_TILE 16            /* tile edge in pixels (one 256-thread workgroup per tile, one wave64 per 8x8 quadrant) */
#define SPLAT_MAX_CHANNELS 8     /* colour channels per call: 3 for the reference API, up to 8 for fused passes */
#define SPLAT_GRAD_STRIDE 16     /* floats per Gaussian in the backward accumulator (one 64-byte line) */
#define SPLAT_GROUP_TILES 2      /* group binning: a group is 2 x 2 tiles (SplatState.group_count) */
#define SPLAT_COUNTER_STRIDE 32  /* uint32 words between two tile counters: one 128-byte line per counter, so that
                                    the ~200 atomics a tile receives do not serialise with its neighbours' */

enum {
    SPLAT_OK = 0,
    SPLAT_E_INVALID = 1,         /* bad argument (null pointer, channel count, negative size) */
    SPLAT_E_LAUNCH = 2,          /* hipGetLastError() != hipSuccess after a launch */
    SPLAT_E_UNSUPPORTED = 3      /* feature not built into this library */
};

/* Mirrors the reference settings tuple field by field
 * (/root/reference/utils/recon_helpers.py:14-26); tensors become device pointers. */
typedef struct SplatCamera {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    const float *bg;             /* [channels], or NULL = black (every SplaTAM camera: /root/reference/utils/recon_helpers.py:17); with NULL
                                    the backward composite drops the background term of dL/dalpha at compile time */
    float scale_modifier;
    const float *viewmatrix;     /* [16] */
    const float *projmatrix;     /* [16] */
    int32_t sh_degree;
    const float *campos;         /* [3] (only read when shs != NULL) */
    int32_t prefiltered;
} SplatCamera;

/* The per-Gaussian inputs of GaussianRasterizer.__call__
 * (/root/reference/scripts/splatam.py:249; kwargs built at
 * /root/reference/utils/slam_helpers.py:131-138). */
typedef struct SplatGaussians {
    int32_t P;                   /* number of Gaussians */
    int32_t channels;            /* colour channels C (3 through the reference API) */
    const float *means3D;        /* [P][3] */
    const float *opacities;      /* [P] */
    const float *colors_precomp; /* [P][C] or NULL when shs is given */
    const float *scales;         /* [P][3] or NULL when cov3D_precomp is given */
    const float *rotations;      /* [P][4] or NULL when cov3D_precomp is given */
    const float *cov3D_precomp;  /* [P][6] or NULL */
    const float *shs;            /* [P][sh_coeffs][3] or NULL */
    int32_t sh_coeffs;           /* M */
} SplatGaussians;

/* State that lives from forward to backward (the reference keeps the same
 * information in its geomBuffer / binningBuffer / imgBuffer byte tensors). */
typedef struct SplatState {
    /* per-Gaussian geometry, written by splat_preprocess_forward */
    float *depth;                /* [P]     view-space z */
    float *xy;                   /* [P][2]  pixel centre */
    float *conic_opacity;        /* [P][4]  inverse 2D covariance (xx, xy, yy) + opacity */
    uint32_t *rect;              /* [P][2]  tile rect packed (minx | miny<<16, maxx | maxy<<16); max exclusive */
    int32_t *radii;              /* [P]     3-sigma radius in pixels, 0 = culled (an OUTPUT of the reference API) */
    float *rgb;                  /* [P][3]  colours evaluated from SH (NULL unless shs is used) */
    uint8_t *clamped;            /* [P][3]  SH clamp flags (NULL unless shs is used) */
    /* per-tile */
    uint32_t *tile_count;        /* [T * max(sub_bins, 1) * SPLAT_COUNTER_STRIDE] instances per tile, counter t at t * SPLAT_COUNTER_STRIDE */
    uint32_t *tile_base;         /* [T+1]   exclusive prefix sum of tile_count */
    uint32_t *tile_cursor;       /* [T * max(sub_bins, 1) * SPLAT_COUNTER_STRIDE] scatter cursors, same spacing (spare words of the
                                    lines hold the partial records of the tile scan) */
    /* per-instance ((Gaussian, tile) pairs) */
    uint64_t *keys;              /* [capacity] (float bits of depth << 32) | Gaussian id, bucketed by tile */
    uint32_t *point_list;        /* [capacity] Gaussian ids, each tile's slice sorted by key */
    int64_t capacity;
    /* optional (NULL: none): [capacity][12] floats, the STAGED RECORD of every list entry as the forward composite held it -- conic
     * (pre-scaled) + opacity, colours, centre, id, quadrant mask: 48 bytes, at the entry's position in point_list.  The forward
     * composite writes it (calls with up to three colour channels + depth, and the fused iteration's six), the backward composite
     * then re-stages a tile's list with one coalesced read per entry instead of gathering conic / centre / colours through the
     * id and repeating the culling tests.  Valid only for the backward pass that follows THAT forward pass on this state */
    float *tile_recs;
    /* scratch of the multi-workgroup sort of per-tile lists longer than 4096 entries (NULL: such a list is sorted in place
     * by one workgroup -- correct, but O(n log^2 n) barrier stages) */
    uint64_t *keys_alt;          /* [capacity] ping-pong partner of `keys` for the merge passes */
    uint32_t *long_base;         /* [T+1] first work item of every tile with a long list */
    uint32_t *long_items;        /* [capacity / 1024 + T + 1] tile of every work item (1024 keys of a long list), written by the scan
                                  * with long_base; NULL: the kernels find an item's tile by a binary search of long_base (13 dependent
                                  * reads per item: ~4x slower run sort) */
    /* group binning (fused iteration, bucketed lists short enough for the composite's own sort): the per-Gaussian kernel
     * files ONE record per touched GROUP of SPLAT_GROUP_TILES x SPLAT_GROUP_TILES tiles (slots taken per (workgroup, group)
     * through an LDS histogram: ~1 global atomic per Gaussian in random row order, far fewer in creation order, instead of one
     * per (Gaussian, tile) instance; sixteen groups' counters share 64 bytes, so that a wave's atomics coalesce); the forward
     * composite of a tile filters its group's records by their tile rectangle, sorts, and publishes point_list / tile_count
     * exactly as the per-tile buckets would have held them.  NULL / group_stride 0: per-tile buckets */
    uint32_t *group_count;       /* [G * SPLAT_COUNTER_STRIDE] records per group, G = ceil(tiles_x / 2) * ceil(tiles_y / 2): the LIVE counter of
                                    group g is word 16 + g % 16 of line g / 16 (sixteen consecutive groups in the upper 64 bytes of a
                                    line), zero between iterations; word 1 of line g keeps the count of the last fused iteration; every
                                    other word stays zero */
    uint32_t *group_recs;        /* [G * group_stride][4] (Gaussian id, float bits of depth, rect word 0, rect word 1) */
    int32_t max_list_hint;       /* longest tile list if the host knows it (status[2] of an earlier read), 0 = unknown */
    int32_t order_hint;          /* fused iteration, bucketed lists: non-zero = the map is (mostly) in creation order (neighbouring rows
                                    are neighbouring pixels: SplaTAM appends one Gaussian per pixel in scan order), so a workgroup's
                                    instances fall on a few tiles and the bucket slots are taken per (workgroup, tile) through LDS;
                                    0 = unknown / random order: one returning atomic per instance.  Results do not depend on it */
    int32_t sub_bins;            /* exact path: counters per tile (a power of two; 0 / 1 = one).  tile_count / tile_cursor then hold
                                    T * sub_bins counters ((tile * sub_bins + (Gaussian index & (sub_bins - 1))) * SPLAT_COUNTER_STRIDE):
                                    spreads the count / scatter atomics of very long lists over several addresses.  The
                                    lists themselves are unchanged.  Must be 0 / 1 with bucketed lists */
    int32_t tile_stride;         /* 0: compact lists, tile t = [tile_base[t], tile_base[t+1]) (the exact path);
                                    > 0: BUCKETED lists (fused iteration only): tile t = [t*stride, t*stride + min(count, stride)),
                                    filled by the per-Gaussian kernel itself -- no scan, no scatter pass; a tile that
                                    receives more than `stride` instances sets status[1] and is truncated */
    int32_t group_stride;        /* > 0 (with group_count, group_recs, tile_stride > 0 and 0 < max_list_hint <= 819): group binning,
                                    records per group bucket (>= SPLAT_GROUP_TILES^2 * tile_stride can never overflow first) */
    /* fused iteration only: composite just the tile ROWS [tile_row_begin, tile_row_end) of the frame (0, 0 = all).  The
     * per-Gaussian kernels still run over the whole map; lists, planes, per-pixel state and loss sums are produced for those
     * rows only, and the per-Gaussian partial sums (hence the pose sums) hold those rows' share.  This is how the tracking
     * iteration shards over GPUs: every quantity the pose gradient needs is a SUM over pixels, so the ranks' copies of
     * SplatIterWorkspace.sums add up to the whole frame's (one all-reduce of 16 KB per iteration; splat_iter_finish) */
    int32_t tile_row_begin, tile_row_end;
    /* launch order of the composites' workgroups (fused iteration, whole frames; NULL / NULL = the natural order).  A launch of
     * 3 225 tile workgroups of very different length on 1 024 resident slots leaves a long tail (time-weighted occupancy 67-76 %,
     * profiles/r04_k7_account.md): the forward composite leaves a work estimate per tile in tile_work ([T]: the sum over the
     * tile's four 8x8 quadrants of the deepest list entry any pixel blended -- what the backward composite will walk), eight extra
     * workgroups of the iteration's last kernel turn it into tile_order ([8 * ceil(T / 8)]: the tiles of every XCD band, heaviest first; an
     * entry holds tile + 1, 0 = not written yet: the natural tile of the slot -- a ZERO-INITIALISED buffer is the natural order --,
     * 0xFFFFFFFF = no tile),
     * and the NEXT iteration that is given this tile_order buffer starts its
     * composites' workgroups in that order (a caller that alternates between views keeps one buffer per view: the estimate belongs
     * to the view it was measured on -- splatam_amd/fused.py).  Only a schedule: any permutation of each band gives the same results. */
    uint32_t *tile_work;
    uint32_t *tile_order;
    /* per-pixel */
    float *final_T;              /* [H][W] */
    int32_t *n_contrib;          /* [H][W] 1-based list position of the last contributor */
    int32_t *status;             /* [4] the SPLAT_STATUS_* words */
    /* optional (NULL: none): ONE int32 in pinned HOST memory that the group-binning kernels set to 1 whenever they raise status[1] or
     * status[3] -- a caller that never waits for the device between the forward and the backward pass reads it (after an event that
     * follows the forward composite) without queueing a copy.  The caller zeroes it before the call. */
    int32_t *status_host;
    /* optional (NULL: none; group binning behind the reference API only): the backward accumulator [P][SPLAT_GRAD_STRIDE] that the backward
     * pass of THIS forward pass will use -- splat_preprocess_forward zeroes row i beside Gaussian i's geometry (stores the kernel has
     * room for), and splat_backward with SPLAT_GRADS_ACCUM_ZEROED then skips its 64-byte-per-Gaussian memset launch */
    float *accum_to_zero;
} SplatState;

const char *splat_error_string(int code);
int splat_abi_version(void);
/* sizeof() of the struct named `name` ("SplatState", "SplatIterWorkspace", ...) as this library was compiled, 0 for an unknown
 * name: a binding that mirrors the structs by hand (ctypes, cgo, JNA) checks its layout against it at load time. */
size_t splat_sizeof(const char *name);

size_t splat_num_tiles(int32_t width, int32_t height);


/* GROUP BINNING behind the reference API (ABI 10) -- the front end of the fused iteration for callers of splat_forward / splat_backward
 * who know that the scene's per-tile lists are short (an earlier call on the same scene left its longest list in status[2]):
 *   st->tile_stride  = S > 0      bucket of tile t in point_list = [t * S, t * S + count); S <= 1024 entries is all the composite sorts
 *   st->max_list_hint = L with L + L / 4 <= 1024   (the longest list the caller expects)
 *   st->group_count / group_recs / group_stride (>= 4 * S can never overflow first), st->capacity >= S * tiles; st->keys may be NULL
 * splat_preprocess_forward then zeroes group_count and status, and files ONE 16-byte record per (Gaussian, touched group of 2 x 2 tiles);
 * splat_bin_forward is a no-op; splat_render_forward (3 colour channels) filters, sorts and publishes every tile's list itself
 * (point_list, tile_count) and composites; splat_backward walks the published lists.  Two launches forward instead of six, and NOTHING
 * the host has to read before the composite may be launched (the exact path reads status[0] to size keys / point_list, as the CUDA
 * original reads num_rendered).  A list longer than S or 1024 entries, or a group bucket that overflowed, raises status[1] / status[3]:
 * the images and gradients of that call are then built from TRUNCATED lists (memory-safe, wrong) and the caller must repeat the call
 * on exact lists (tile_stride = 0).  status[0] and status[2] are not maintained in this mode.
 * The lists of this mode are the library's own business (built, sorted, published and replayed by its kernels; `rect` / `radii` keep the
 * reference's values): a Gaussian is filed only in those tiles of its ceil(3 sigma) rectangle that can hold a pixel with
 * alpha >= 1/255 (csrc/splat_math.h live_tile_rect) -- 12-13 % fewer entries at the SplaTAM workloads, identical images and gradients
 * (a dropped entry fails the alpha test at every pixel of its tile).  The exact path keeps the reference's lists entry for entry. */

/* K1 + tile scan.  Replaces the first half of `_C.rasterize_gaussians`
 * (preprocess, prefix sum).  Writes depth/xy/conic_opacity/rect/radii,
 * tile_count/tile_base/tile_cursor and status[0..2].  The host may read
 * status[0] (num_rendered) to size keys/point_list, as the reference does.
 * The scan compares the count with st->capacity and publishes EMPTY ranges (status[1] set) when it is larger: a caller that
 * allocates its lists AFTER this call sets st->capacity to an upper bound (e.g. INT64_MAX / 2) for this call and to the real
 * capacity before splat_bin_forward (tests/capi_smoke.c, splatam_amd/rasterizer.py do). */
int splat_preprocess_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, void *stream);

/* Scatter (Gaussian, tile) instances into per-tile buckets and sort every
 * bucket by (depth bits, id).  Replaces duplicateWithKeys + the global radix
 * sort + identifyTileRanges of the reference.  A no-op that leaves status[1]
 * set when num_rendered > st->capacity.
 * CONTRACT: the second half of ONE forward pass -- call it on the SplatState that splat_preprocess_forward has just filled, with the
 * same cam, the same g->P and unchanged st->sub_bins / st->tile_stride (the caller may only set keys / point_list / capacity in
 * between, after reading status[0]).  With sub_bins > 1 the per-tile counters are split over sub-bins by (workgroup of 4 096
 * Gaussians) and the scatter walks the SAME partition the count used; a caller that fills tile_count itself, or changes P or
 * sub_bins between the two calls, gets ranges that do not match the scatter (undefined lists).  splat_forward() does both. */
int splat_bin_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, void *stream);

/* Tile-wise alpha compositing.  out_color [C][H][W], out_depth [H][W].
 * `colors` is [P][C]: colors_precomp, or st->rgb when SH were evaluated. */
int splat_render_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st,
                         float *out_color, float *out_depth, void *stream);

/* All three of the above back to back (capacity must already be sufficient). */
int splat_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st,
                  float *out_color, float *out_depth, void *stream);

/* Gradient outputs of `_C.rasterize_gaussians_backward`
 * (autograd backward reached from /root/reference/scripts/splatam.py:702,854). */
typedef struct SplatGrads {
    const float *dL_dcolor;      /* [C][H][W] incoming gradient of out_color */
    float *accum;                /* [P][SPLAT_GRAD_STRIDE] scratch, zeroed by the library */
    float *dL_dmeans3D;          /* [P][3] */
    float *dL_dmeans2D;          /* [P][3] NDC-space gradient of the projected centre, z = 0 */
    float *dL_dcolors;           /* [P][C] (NULL when shs are used) */
    float *dL_dopacities;        /* [P] */
    float *dL_dscales;           /* [P][3] or NULL.  Gradient w.r.t. the UNMODIFIED scales the caller passed: it carries the factor
                                    cam->scale_modifier (Sigma = R diag((modifier s)^2) R^T).  DEVIATION from the CUDA original as recalled
                                    (SURVEY.md Appendix A): its computeCov3D adjoint returns dL/d(modifier s) without that factor.  Equal at
                                    modifier 1.0 -- every SplaTAM configuration, the viewers render without gradients --; a caller that
                                    trains with another modifier and wants the original's numbers divides by it.  The oracle follows this
                                    library (oracle/raster_ref.c), tests/test_gpu_configs.py covers modifier 1.6 */
    float *dL_drotations;        /* [P][4] or NULL */
    float *dL_dcov3D;            /* [P][6] or NULL */
    float *dL_dshs;              /* [P][M][3] or NULL */
    int32_t flags;               /* SPLAT_GRADS_* */
} SplatGrads;
#define SPLAT_GRADS_POISON_IF_FLAGGED 2 /* group binning behind the reference API: splat_preprocess_backward writes NaN into EVERY gradient output when
                                        the forward pass of this state raised status[1] or status[3] (its lists were truncated).  For a caller that
                                        launches the backward pass without having looked at the flags: gradients formed on truncated lists never
                                        reach an optimizer as plausible numbers */
#define SPLAT_GRADS_ACCUM_ZEROED 4 /* gr->accum is zero already (SplatState.accum_to_zero of the forward pass): splat_render_backward does not clear it */
#define SPLAT_GRADS_UPSTREAM_SCALE 1 /* dL_dscales WITHOUT the factor cam->scale_modifier: the numbers the CUDA original returns (its computeCov3D
                                        adjoint forms dL/d(modifier * s) and hands it out as dL/ds; see dL_dscales above).  Identical at modifier 1.0 */

/* Per-pixel back-to-front replay; accumulates per-Gaussian partial sums into gr->accum. */
int splat_render_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st,
                          SplatGrads *gr, void *stream);

/* Per-Gaussian chain rule from gr->accum to every dL_d* output. */
int splat_preprocess_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st,
                              SplatGrads *gr, void *stream);

/* Both of the above back to back. */
int splat_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st,
                   SplatGrads *gr, void *stream);

/* `_C.mark_visible` of the reference extension: present[i] = (view-space z > 0.2). */
int splat_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, uint8_t *present, void *stream);

/* Do two rasterizer calls see the same geometry?  *differ (device int32) = 0 when opacities [P], scales [P][3] and rotations [P][4]
 * of call A and call B hold the same bits, non-zero otherwise.  The two renders of the reference's get_loss
 * (/root/reference/scripts/splatam.py:249,253) receive equal-valued but distinct tensors (sigmoid / exp / normalize are applied
 * twice: /root/reference/utils/slam_helpers.py:124-139, 234-249); a binding that has proven the rest equal (same means3D storage,
 * same camera) may then hand the second call the first call's SplatState -- geometry and sorted lists -- and run only
 * splat_render_forward for it. */
int splat_same_geometry(int32_t P, const float *opacities_a, const float *opacities_b, const float *scales_a, const float *scales_b,
                        const float *rotations_a, const float *rotations_b, int32_t *differ, void *stream);

/* Kernel-only timing helper for bench.py: runs `fn` (0 = render forward,
 * 1 = render backward) `iters` times on `stream` between two hipEvents created
 * on that same stream and returns the mean milliseconds per launch in *ms. */
int splat_time_kernel(int fn, int iters, const SplatCamera *cam, const SplatGaussians *g, SplatState *st,
                      SplatGrads *gr, float *out_color, float *out_depth, void *stream, float *ms);


/* ------------------------------------------------------------------------------------------------------------
 * Fused SplaTAM iteration: everything the reference does in Python around the two
 * rasterizer calls of one optimisation iteration, as a handful of kernels with no host synchronisation:
 *   transform_to_frame + transformed_params2rendervar + transformed_params2depthplussilhouette
 *     (/root/reference/utils/slam_helpers.py:252-304, :124-139, :234-249)  -> one per-Gaussian kernel,
 *   the RGB and the depth/silhouette renders (/root/reference/scripts/splatam.py:249,253)
 *     -> ONE 6-channel composite (r, g, b, z, 1, z^2) over shared geometry and lists,
 *   the masked losses of get_loss (/root/reference/scripts/splatam.py:256-290, calc_ssim
 *     /root/reference/utils/slam_external.py:54-97) and their gradients -> per-pixel kernels,
 *   loss.backward() through the render variables and the camera pose -> one per-Gaussian kernel,
 *   optimizer.step() (/root/reference/scripts/splatam.py:160-166,704,860) -> fused Adam kernels,
 *   the best-candidate pose bookkeeping of the tracking loop (/root/reference/scripts/splatam.py:706-711).
 * Every argument of get_loss is supported (use_l1, use_sil_for_loss, ignore_outlier_depth_loss with torch.median's
 * exact lower median, tracking / mapping / do_ba); the one thing the fused path does not produce is the colour pass'
 * own means2D.grad (gradient-based densification, off in every SLAM config): the caller uses the two-call path for it.
 * ------------------------------------------------------------------------------------------------------------ */

/* The reference's `params` dict (/root/reference/scripts/splatam.py:120-157).  Adam updates it in place. */
typedef struct SplatMap {
    int32_t P;
    int32_t isotropic;           /* log_scales is [P][1] (1) or [P][3] (0) */
    float *means3D;              /* [P][3] world frame */
    float *rgb_colors;           /* [P][3] */
    float *unnorm_rotations;     /* [P][4] */
    float *logit_opacities;      /* [P] */
    float *log_scales;           /* [P][1] or [P][3] */
    float *cam_unnorm_rots;      /* [1][4][num_frames] */
    float *cam_trans;            /* [1][3][num_frames] */
    int32_t num_frames;
} SplatMap;

/* `curr_data` of get_loss.  im and depth may be any contiguous view: they need the 4-byte alignment of a float only (the loss kernels
 * take their 16-byte loads only where every plane they touch starts on 16 bytes, and read scalar-wise otherwise). */
typedef struct SplatFrameData {
    const float *im;             /* [3][H][W] */
    const float *depth;          /* [1][H][W] */
    const float *w2c;            /* [16] row-major curr_data['w2c'] (first-frame world-to-camera) */
    int32_t time_idx;            /* iter_time_idx: which camera pose of the map transforms the Gaussians */
} SplatFrameData;

/* Arguments of get_loss (/root/reference/scripts/splatam.py:214-216). */
typedef struct SplatLossConfig {
    int32_t tracking;            /* 1: tracking=True (summed losses); 0: mapping=True (means + SSIM) */
    int32_t camera_grad;         /* transform_to_frame(camera_grad=...) */
    int32_t gaussians_grad;      /* transform_to_frame(gaussians_grad=...) */
    int32_t use_sil_for_loss;
    float sil_thres;
    int32_t use_l1;
    int32_t ignore_outlier_depth_loss;
    float w_im;                  /* loss_weights['im'] */
    float w_depth;               /* loss_weights['depth'] */
    int32_t defer_finish;        /* 1: stop before the last kernel (pose gradient, loss value, pose Adam step): the caller completes the
                                    partial sums (all-reduce over the ranks that composited other tile rows) and calls splat_iter_finish */
    int32_t fused_composite;     /* tracking with a pixel-local loss (no outlier rejection), lists the composite sorts itself (with map
                                    gradients wanted -- ws->d_rgb_colors / d_logit_opacities -- the kernel carries the backward composite's
                                    mapping form): 1 = forward composite, loss and backward composite as ONE kernel (the backward pass
                                    walks the batch the forward pass left in LDS; ws->out6, dL_dout6, st.final_T, st.n_contrib are NOT
                                    written), 2 = the same kernel, planes written as well, 0 = two kernels.  Ignored where it does not apply */
} SplatLossConfig;

#define SPLAT_ITER_SUMS 32       /* doubles per copy of the partial sums */
#define SPLAT_ITER_SUM_COPIES 64 /* copies: workgroups spread their atomics over them (one hot cache line otherwise) */
#define SPLAT_ITER_DCAM 32       /* floats of SplatIterWorkspace.d_cam */
/* the slots of SplatIterWorkspace.d_cam, the iteration's report (written by its last kernel; 10 spare) */
#define SPLAT_REPORT_DROT 0        /* [0..3] dL/dcam_unnorm_rots[..., t] */
#define SPLAT_REPORT_DTRANS 4      /* [4..6] dL/dcam_trans[..., t] */
#define SPLAT_REPORT_LOSS 7
#define SPLAT_REPORT_SUMS 8        /* [8..11] the raw sums [0..3] of this iteration */
#define SPLAT_REPORT_FLAG 12       /* STICKY "lists overflowed / unsorted" flag (set by any iteration whose status OVERFLOW or STALE_HINT
                                      was set; cleared by the host).  While it is up the Adam steps of this ABI (inside
                                      splat_iter_tracking_step / _mapping_step / _finish, splat_iter_adam_pose, and splat_iter_adam_map
                                      with SplatAdamMap.gate) leave parameters, moments and the best-candidate record untouched: an
                                      iteration on truncated lists never moves the map */
#define SPLAT_REPORT_MEDIAN 13     /* the median depth error of this iteration when ignore_outlier_depth_loss is set */
#define SPLAT_REPORT_DEPTH_TERM 14 /* loss_weights['depth'] * the depth term, and ... */
#define SPLAT_REPORT_IM_TERM 15    /* ... loss_weights['im'] * the image term of the loss (weighted_losses['depth' / 'im'] of
                                      /root/reference/scripts/splatam.py:339) */
#define SPLAT_REPORT_STATUS 16     /* [16..19] int32 bit patterns of st.status[0..3] as this iteration left them */
#define SPLAT_REPORT_FLAGGED 20    /* int32: 1 when THIS iteration was flagged */
#define SPLAT_REPORT_SKIPPED 21    /* int32: iterations whose Adam step was skipped since the host last cleared it */

/* Device scratch + outputs of one fused iteration; every array is caller-owned.  The caller ZERO-INITIALISES sums,
 * st.tile_count, accum and dL_dout6 once; each iteration leaves them zeroed again (the kernels that consume a buffer
 * reset it), so the steady state has no memset launches. */
typedef struct SplatIterWorkspace {
    SplatState st;               /* geometry, lists (fixed capacity; overflow -> st.status[1]) and per-pixel state */
    float *feat8;                /* [P][8]  r, g, b, z, 1, z^2, 0, 0 */
    float *out6;                 /* [6][H][W] rendered r, g, b, depth, silhouette, depth^2 */
    float *dL_dout6;             /* [6][H][W] */
    float *accum;                /* [P][SPLAT_GRAD_STRIDE] */
    float *ssim_maps;            /* [9][H][W] mapping only (NULL for tracking) */
    double *sums;                /* [SPLAT_ITER_SUM_COPIES][SPLAT_ITER_SUMS]: [0] masked depth L1 sum, [1] image L1 sum,
                                    [2] mask count, [3] SSIM map sum ([2], [3]: mapping only -- the tracking loss divides by nothing
                                    and forms neither: 0), [8..23] camera-pose partial sums, [31] != 0: a capacity flag was
                                    raised on some band of a tile-row-sharded iteration (cfg.defer_finish) */
    float *max_2D_radius;        /* [P] variables['max_2D_radius'], updated in place, or NULL */
    /* gradients of the map (written when non-NULL; means3D / unnorm_rotations only with gaussians_grad) */
    float *d_means3D;            /* [P][3] */
    float *d_rgb_colors;         /* [P][3] */
    float *d_unnorm_rotations;   /* [P][4] */
    float *d_logit_opacities;    /* [P] */
    float *d_log_scales;         /* [P][1|3] */
    float *d_cam;                /* [SPLAT_ITER_DCAM] the iteration's report: the SPLAT_REPORT_* slots */
    /* only read when cfg->ignore_outlier_depth_loss (/root/reference/scripts/splatam.py:266-268), NULL otherwise */
    float *outlier_err;          /* [H*W] scratch: depth error per pixel */
    uint32_t *outlier_scratch;   /* splat_map_scratch_words(H*W) words: histograms of the radix selection of torch.median */
} SplatIterWorkspace;

/* ------------------------------------------------------------------------------------------------------------
 * Scratch layouts: what a binding needs to size and wire the caller-owned scratch WITHOUT reading the Python binding
 * (`splat_workspace_bytes(P, W, H, R_cap)`).  The reference extension sizes its geomBuffer / binningBuffer /
 * imgBuffer through a resize callback into torch byte tensors; here the library describes ONE slab: every array of a SplatState
 * (+ SplatGrads.accum) or of a SplatIterWorkspace by field name, with its size, its offset in the slab (SPLAT_SLAB_ALIGN-aligned)
 * and whether the caller must zero it once before the first call.  `splat_*_bind` writes the pointers into the struct.
 * A caller may also allocate the arrays one by one from `bytes` and set the pointers itself (the Python binding of the fused
 * iteration does: its per-Gaussian arrays grow with the map).
 * ------------------------------------------------------------------------------------------------------------ */
#define SPLAT_SLAB_ALIGN 256
typedef struct SplatArrayInfo {
    const char *name;            /* field name in SplatState / SplatGrads / SplatIterWorkspace ("st.keys" for the embedded state) */
    size_t bytes;
    size_t offset;               /* in the slab */
    int32_t zero_init;           /* 1: zero it once before the first call (the kernels leave it zeroed afterwards) */
} SplatArrayInfo;
#define SPLAT_LAYOUT_SH 1        /* shs are used: SplatState.rgb / clamped */
#define SPLAT_LAYOUT_LONG_LISTS 2 /* lists may exceed 4 096 entries: keys_alt, long_items (always needed while the lengths are unknown) */
#define SPLAT_LAYOUT_BACKWARD 4  /* SplatGrads.accum */
#define SPLAT_LAYOUT_SSIM 8      /* fused iteration: ssim_maps (mapping) */
#define SPLAT_LAYOUT_OUTLIER 16  /* fused iteration: outlier_err / outlier_scratch (ignore_outlier_depth_loss) */
#define SPLAT_LAYOUT_GROUPS 32   /* splat_state_layout: group binning behind the reference API -- group_count (right in front of status: the library
                                    zeroes both with one memset), group_recs for `group_stride` = 4 * tile_stride records per group, where
                                    tile_stride = capacity / tiles; no key buckets */
#define SPLAT_LAYOUT_RECS 128     /* tile_recs: 48 bytes x capacity (a forward pass that a backward pass will follow) */
#define SPLAT_LAYOUT_TILE_ORDER 64 /* splat_iter_workspace_layout / _bind: st.tile_work, st.tile_order (launch order of the composites; the
                                    library's first iteration on a workspace treats an order buffer it has not written yet as the natural
                                    order -- see SplatState.tile_order) */
#define SPLAT_LAYOUT_MAX_ARRAYS 48
/* One rasterizer call (forward, + backward with SPLAT_LAYOUT_BACKWARD): arrays of SplatState for P Gaussians, a width x height
 * image, `sub_bins` counters per tile (0 / 1 = one) and lists of `capacity` instances.  Writes up to `max_entries` entries to `out`
 * (NULL: count only) and the slab size to *total_bytes; returns the number of arrays, or -SPLAT_E_INVALID. */
int splat_state_layout(int32_t P, int32_t width, int32_t height, int32_t sub_bins, int64_t capacity, int32_t flags,
                       SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes);
/* Points the fields of *st (and gr->accum when gr != NULL and the layout has it) into `slab` and sets st->capacity / st->sub_bins;
 * fields the layout does not name are left as they are. */
int splat_state_bind(SplatState *st, SplatGrads *gr, void *slab, const SplatArrayInfo *arrays, int32_t n, int32_t sub_bins,
                     int64_t capacity);
/* The slab size of splat_state_layout(P, width, height, 1, capacity, SPLAT_LAYOUT_LONG_LISTS | SPLAT_LAYOUT_BACKWARD): enough for
 * any call without SHs whose lists hold at most `capacity` instances. */
size_t splat_workspace_bytes(int32_t P, int32_t width, int32_t height, int64_t capacity);
/* The fused iteration's SplatIterWorkspace (its embedded state as "st.<field>"): `group_stride` records per group bucket (0: no group
 * binning).  Not in the layout: the gradient outputs d_* and max_2D_radius (the caller's own tensors). */
int splat_iter_workspace_layout(int32_t P, int32_t width, int32_t height, int64_t capacity, int32_t group_stride, int32_t flags,
                                SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes);
int splat_iter_workspace_bind(SplatIterWorkspace *ws, void *slab, const SplatArrayInfo *arrays, int32_t n, int64_t capacity,
                              int32_t group_stride);
size_t splat_iter_workspace_bytes(int32_t P, int32_t width, int32_t height, int64_t capacity, int32_t group_stride, int32_t flags);

/* get_loss + loss.backward() of one iteration.  On return (stream order) ws->d_* hold the gradients and
 * ws->d_cam[7] the loss value.  The fused iteration renders on a ZERO background, as setup_camera builds it
 * (/root/reference/utils/recon_helpers.py:17): cam->bg must point at six zeros (the backward composite drops the term). */
int splat_iter_loss_backward(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                             const SplatLossConfig *cfg, SplatIterWorkspace *ws, void *stream);

/* torch.optim.Adam over the five Gaussian groups (mapping: /root/reference/scripts/splatam.py:160-166 with
 * eps = 1e-15, lr per group from the config).  step_size[k] = lr_k / (1 - beta1^t_k) and bc2_sqrt[k] = sqrt(1 - beta2^t_k)
 * are formed by the caller in double, as torch does -- per group, because torch keeps a step count per parameter and a
 * parameter the caller re-created (pruning, opacity reset) restarts or skips its count.  Group order: means3D, rgb_colors,
 * unnorm_rotations, logit_opacities, log_scales.  exp_avg / exp_avg_sq have the shapes of the parameters.  gate: NULL, or
 * the d_cam of the iteration that formed the gradients -- the step is skipped while d_cam[12] (the capacity flag) is up.
 * one_minus_beta1 / one_minus_beta2: 1 - beta formed by the caller in double, as torch forms the weights of its moment updates
 * (1.0f - 0.999f is 1.3e-5 away from float(1 - 0.999): every exp_avg_sq would be ~100 ulps off torch's). */
typedef struct SplatAdamMap {
    float beta1, beta2, eps;
    float one_minus_beta1, one_minus_beta2;
    float bc2_sqrt[5];
    float step_size[5];
    const float *grad[5];
    float *exp_avg[5];
    float *exp_avg_sq[5];
    const float *gate;
} SplatAdamMap;
int splat_iter_adam_map(const SplatMap *map, const SplatAdamMap *opt, void *stream);

/* Adam step of the camera pose of frame `time_idx` (tracking: default eps 1e-8) followed by the reference's
 * best-candidate bookkeeping: if loss < min_loss, remember the UPDATED pose.  d_cam: the report of the iteration
 * (gradient [0..6], loss [7]); skipped while d_cam[12] is up.
 * state [24] floats: exp_avg q(4) t(3), exp_avg_sq q(4) t(3), min_loss, candidate q(4) t(3), 2 spare. */
#define SPLAT_POSE_STATE 24
int splat_iter_adam_pose(const SplatMap *map, int32_t time_idx, const float *d_cam, float *state,
                         float beta1, float beta2, float eps, float bc2_sqrt, float step_size_rot, float step_size_trans,
                         void *stream);

/* One whole tracking iteration (/root/reference/scripts/splatam.py:690-711) in one call: splat_iter_loss_backward with
 * cfg->tracking set, with the pose's Adam step and the best-candidate bookkeeping of splat_iter_adam_pose folded into its last
 * kernel (one launch less per iteration).  `state` and the step sizes as for splat_iter_adam_pose. */
typedef struct SplatPoseAdam {
    float *state;                /* [SPLAT_POSE_STATE] */
    float beta1, beta2, eps, bc2_sqrt, step_size_rot, step_size_trans;
} SplatPoseAdam;
int splat_iter_tracking_step(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                             const SplatLossConfig *cfg, SplatIterWorkspace *ws, const SplatPoseAdam *adam, void *stream);

/* The last kernel of an iteration whose splat_iter_loss_backward / splat_iter_tracking_step ran with cfg->defer_finish: totals
 * ws->sums into ws->d_cam (pose gradient, loss), resets them, and takes the pose's Adam step when `adam` is given (as
 * splat_iter_tracking_step would have).  Tile-row-sharded tracking: all-reduce ws->sums (SPLAT_ITER_SUM_COPIES x SPLAT_ITER_SUMS
 * doubles, sum) over the ranks between the two calls; every rank then holds the same sums and takes the same step. */
int splat_iter_finish(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatLossConfig *cfg,
                      SplatIterWorkspace *ws, const SplatPoseAdam *adam, void *stream);

/* Between an iteration that ran with cfg->defer_finish and its all-reduce: folds the SPLAT_ITER_SUM_COPIES copies of ws->sums into
 * copy 0 and zeroes the others, so that the exchange carries SPLAT_ITER_SUMS doubles (256 bytes) instead of all the copies (16 KB);
 * splat_iter_finish totals the copies either way. */
int splat_iter_fold_sums(double *sums, void *stream);

/* One whole single-view mapping iteration (/root/reference/scripts/splatam.py:846-863: get_loss, backward, optimizer.step) in
 * one call: splat_iter_loss_backward with cfg->tracking clear, with splat_iter_adam_map folded into its last kernel (every
 * Gaussian's parameters, gradients and moments are touched once).  adam->grad[k] != NULL: group k is stepped; it must then be the
 * ws->d_* buffer of group k (the gradients are still written there) -- or ws->d_* of the group is NULL and the gradient is formed,
 * stepped on and NOT stored (a loop that discards its gradients after the step).  Not for the view-sharded batch: there the gradients are
 * exchanged between splat_iter_loss_backward and splat_iter_adam_map. */
int splat_iter_mapping_step(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                            const SplatLossConfig *cfg, SplatIterWorkspace *ws, const SplatAdamMap *adam, void *stream);

/* ---- added within ABI 17: the loss of the refinement script ------------------------------------------------------------------
 * get_loss_gs (/root/reference/scripts/post_splatam_opt.py:111-147) is get_loss(mapping=True) with another depth term: the mask is
 * gt_depth != 0 (not > 0, no NaN mask), the term is the masked sum of |depth - gt_depth| over ALL H W pixels (not over the mask
 * count), its gradient per valid pixel w_depth * sign / (H W); no silhouette, no outlier rejection, no pose gradient.  The image
 * term (0.8 L1 + 0.2 (1 - SSIM)) is get_loss'.  SplatLossConfig has no room for the choice and ABI 17 is pinned by its callers, so
 * the mode travels in a struct of its own that EMBEDS the old one, and through entry points of its own; the old entry points are
 * the new ones with SPLAT_LOSS_SPLATAM.  With SPLAT_LOSS_GS: base.tracking, base.camera_grad, base.ignore_outlier_depth_loss and
 * base.defer_finish must be clear and base.gaussians_grad set (SPLAT_E_INVALID otherwise); SPLAT_REPORT_LOSS / _DEPTH_TERM /
 * _IM_TERM report the gs values, SPLAT_REPORT_SUMS the same raw sums (the mask count is gt_depth != 0's). */
#define SPLAT_LOSS_SPLATAM 0     /* get_loss (/root/reference/scripts/splatam.py:214-347) */
#define SPLAT_LOSS_GS 1          /* get_loss_gs */
typedef struct SplatLossConfigEx {
    SplatLossConfig base;
    int32_t loss_mode;           /* SPLAT_LOSS_* */
    int32_t reserved[3];         /* zero */
} SplatLossConfigEx;
/* splat_iter_loss_backward / splat_iter_mapping_step under cfg->loss_mode */
int splat_iter_loss_backward_ex(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                                const SplatLossConfigEx *cfg, SplatIterWorkspace *ws, void *stream);
int splat_iter_mapping_step_ex(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                               const SplatLossConfigEx *cfg, SplatIterWorkspace *ws, const SplatAdamMap *adam, void *stream);

/* Kernel-only timing helper for bench.py on the fused path: fn 0 = 6-channel composite forward reading published lists, 1 = 6-channel
 * composite backward (the kernel alone: the launches accumulate on top of each other and the accumulator is zeroed again AFTER the
 * timed bracket, so the workspace stays usable), 2 = the forward composite in the form the iteration launches on short lists
 * (it filters its group's records / reads its bucket, sorts and publishes the tile's list itself; needs bucketed lists and a list
 * length hint <= 819, SPLAT_E_INVALID otherwise), 3 = forward (sorting form when the state allows it) and backward composite
 * alternating, `iters` pairs (time(3) - time(2 or 0) = the backward composite between other kernels), 4 = the backward composite in its
 * tracking form (depth colour sum only, no opacity sum), launched `iters` times on `stream` between two hipEvents; the workspace must hold
 * the state of a completed splat_iter_loss_backward. */
int splat_iter_time_kernel(int fn, int iters, const SplatCamera *cam, int32_t P, SplatIterWorkspace *ws, void *stream, float *ms);

/* ------------------------------------------------------------------------------------------------------------
 * Map growth and maintenance: the per-frame callers that change the NUMBER of Gaussians.
 * The reference re-allocates every parameter tensor with torch.cat / boolean indexing
 * (/root/reference/scripts/splatam.py:378-420, /root/reference/utils/slam_external.py:139-188); here the map is a
 * capacity-managed struct of arrays that is edited in place: rows are appended at the tail / compacted stably, so
 * that after an edit the first `count` rows hold exactly what the reference's tensors would hold, in the same order.
 * Every edit leaves its result count in store->counts (device); the host reads it once per edit (the reference
 * synchronises at the same places: `if torch.sum(non_presence_mask) > 0`, boolean indexing).
 * ------------------------------------------------------------------------------------------------------------ */

/* The map arrays with room for `capacity` rows + what has to move with them. */
typedef struct SplatMapStore {
    SplatMap map;                /* map.P = rows in use, as the HOST knows them (it is the launch bound) */
    int32_t capacity;            /* rows every per-Gaussian array can hold */
    float *exp_avg[5];           /* Adam moments of the live optimizer, group order of SplatAdamMap; NULL = none */
    float *exp_avg_sq[5];
    float *max_2D_radius;        /* variables['max_2D_radius'] [capacity] or NULL */
    float *means2D_gradient_accum; /* variables['means2D_gradient_accum'] [capacity] or NULL */
    float *denom;                /* variables['denom'] [capacity] or NULL */
    float *timestep;             /* variables['timestep'] [capacity] or NULL */
    int32_t *counts;             /* device [8]: [0] rows after the edit, [1] rows appended / removed by it,
                                    [2] the append did not fit `capacity` (then nothing was written),
                                    [3] add_new_gaussians: sum(non_presence_mask) BEFORE the valid-depth mask,
                                    [4] float bits of the median used by add_new_gaussians, 3 spare */
} SplatMapStore;

/* Forward-only pass of the fused composite (kernels F1, K2..K4, K6; no loss, no gradients, nothing accumulated):
 * ws->out6 = r, g, b, depth, silhouette, depth^2 of `map` seen from pose `frame->time_idx`.  This is the render of
 * add_new_gaussians (/root/reference/scripts/splatam.py:381-385) and of the evaluation / keyframe code.
 * frame->im / frame->depth may be NULL. */
int splat_iter_render(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, SplatIterWorkspace *ws,
                      void *stream);

/* Which pixels of an RGB-D frame become new Gaussians. */
enum {
    SPLAT_ADD_VALID_DEPTH = 0,   /* initialize_first_timestep: mask = depth > 0 (/root/reference/scripts/splatam.py:197-202) */
    SPLAT_ADD_NON_PRESENCE = 1   /* add_new_gaussians: silhouette < sil_thres, or rendered depth behind the measured one
                                    by more than 50 x the median depth error; and depth > 0 (:386-408) */
};

typedef struct SplatAddArgs {
    int32_t mode;                /* SPLAT_ADD_* */
    int32_t width, height;
    const float *im;             /* [3][H][W] curr_data['im'] */
    const float *depth;          /* [1][H][W] curr_data['depth'] */
    const float *out6;           /* [6][H][W] render at the tracked pose (planes 3 = depth, 4 = silhouette are read);
                                    NULL for SPLAT_ADD_VALID_DEPTH */
    float fx, fy, cx, cy;        /* curr_data['intrinsics'] (the densification intrinsics) */
    float sil_thres;
    int32_t time_idx;            /* SPLAT_ADD_NON_PRESENCE: pose of the map that back-projects; value of variables['timestep'] */
    const float *w2c;            /* SPLAT_ADD_VALID_DEPTH: [16] row-major rigid world-to-camera of the frame (device) */
    float *err;                  /* scratch [H*W] floats (depth error) */
    uint32_t *scratch;           /* scratch, splat_map_scratch_words(width*height) uint32 words */
} SplatAddArgs;

/* uint32 words of SplatAddArgs.scratch / SplatPruneArgs.scratch for `n` pixels / rows */
size_t splat_map_scratch_words(int64_t n);

/* get_pointcloud + initialize_new_params + the torch.cat of add_new_gaussians / initialize_params
 * (/root/reference/scripts/splatam.py:67-116, 350-376, 378-420): appends one Gaussian per selected pixel, in pixel
 * order: means3D = c2w [x z, y z, z, 1] with (x, y) = ((u - cx) / fx, (v - cy) / fy), rgb from `im`, rotation (1,0,0,0),
 * logit opacity 0, log scale log(sqrt((z / ((fx + fy) / 2))^2)) (1 or 3 columns), timestep = time_idx; when anything was
 * selected before the valid-depth mask, max_2D_radius / means2D_gradient_accum / denom are zeroed for ALL rows, as the
 * reference does.  Moments (exp_avg*) of appended rows are zeroed.  counts[0..4] are written. */
int splat_map_add_new_gaussians(SplatMapStore *store, const SplatAddArgs *args, void *stream);

typedef struct SplatPruneArgs {
    float removal_opacity_threshold; /* remove rows with sigmoid(logit_opacity) < this */
    int32_t remove_big;          /* also remove rows whose largest exp(log_scale) > big_scale */
    float big_scale;             /* 0.1 * variables['scene_radius'] */
    const uint8_t *to_remove;    /* [P] caller-supplied flags (remove_points); NULL = form them from the two rules above */
    uint8_t *flags;              /* scratch [capacity] */
    float *stage;                /* scratch: ((capacity + 3) & ~3) * splat_map_row_floats(store) floats */
    uint32_t *scratch;           /* splat_map_scratch_words(capacity) words */
} SplatPruneArgs;

/* floats per row over every non-NULL array of the store (the staging buffer of a prune holds capacity, rounded up to a
 * multiple of 4, times this) */
int32_t splat_map_row_floats(const SplatMapStore *store);

/* prune_gaussians' removal rule + remove_points (/root/reference/utils/slam_external.py:139-188): stable compaction of
 * the five parameter arrays, the Adam moments and the per-Gaussian variables.  counts[0], counts[1] are written. */
int splat_map_prune(SplatMapStore *store, const SplatPruneArgs *args, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient-based densification (/root/reference/utils/slam_external.py:100-104, 191-240; on in
 * /root/reference/configs/replica/gaussian_splatting.py:82, off in the SLAM configs).
 * ------------------------------------------------------------------------------------------------------------ */

/* accumulate_mean2d_gradient for the iteration whose splat_iter_loss_backward has just run on `ws`: the COLOUR pass' own
 * dL/dmeans2D (what variables['means2D'].grad holds in the reference: the r, g, b planes of the loss gradient only, not the
 * depth render's) is formed by one more backward composite over the three colour planes, and for every Gaussian seen by the
 * render (radius > 0):  means2D_gradient_accum += |dL/dmeans2D.xy|,  denom += 1.  means2D_grad ([P][2], may be NULL)
 * receives the gradient itself; means2D_gradient_accum and denom may BOTH be NULL when only the gradient is wanted (a caller that
 * keeps the reference's own accumulate_mean2d_gradient statement: splatam_amd.plugin).  Leaves ws->accum zeroed. */
int splat_iter_means2d_accumulate(const SplatCamera *cam, const SplatMap *map, SplatIterWorkspace *ws,
                                  float *means2D_gradient_accum, float *denom, float *means2D_grad, void *stream);

enum { SPLAT_DENSIFY_CLONE = 0, SPLAT_DENSIFY_SPLIT = 1 };

typedef struct SplatDensifyArgs {
    int32_t mode;                /* CLONE: grads >= grad_thresh and max exp(log_scales) <= small_scale; SPLIT: ... > small_scale */
    float grad_thresh;           /* densify_dict['grad_thresh'] */
    float small_scale;           /* 0.01 * variables['scene_radius'] */
    int32_t rows_with_grad;      /* rows [0, rows_with_grad) carry an accumulated gradient (store->means2D_gradient_accum / denom,
                                    NaN -> 0); later rows -- the clones appended just before the split -- count as 0 (padded_grad) */
    int32_t num_to_split_into;   /* n (SPLIT) */
    const float *samples;        /* splat_map_duplicate, SPLIT: [S * n][3] draws of torch.normal(0, exp(log_scales)[to_split].repeat(n, 3)) */
    uint8_t *flags;              /* [capacity] selection flags: written by _select, read by _duplicate */
    uint32_t *scratch;           /* splat_map_scratch_words(capacity) words */
} SplatDensifyArgs;

/* Selection: flags + store->counts[1] = selected rows S, counts[0] = rows after appending S (CLONE) / S * n (SPLIT) rows,
 * counts[2] = the append would not fit `capacity`. */
int splat_map_densify_select(SplatMapStore *store, const SplatDensifyArgs *args, void *stream);

/* Appends the selected rows (after a _select with the same args): CLONE: copies, in row order; SPLIT: n blocks of the selected
 * rows (torch's v[mask].repeat(n, 1)) with means3D += build_rotation(unnorm_rotations) @ sample and
 * log_scales = log(exp(log_scales) / (0.8 n)).  Adam moments and max_2D_radius / means2D_gradient_accum / denom of the new rows
 * are zero.  The caller then sets map.P = counts[0]; the split originals are removed with splat_map_prune(to_remove = flags). */
int splat_map_duplicate(SplatMapStore *store, const SplatDensifyArgs *args, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation of a finished run (the per-frame part of eval(), /root/reference/utils/eval_helpers.py:408-623): PSNR, depth
 * "RMSE", depth L1 and MS-SSIM of one rendered frame against its RGB-D frame, as ONE ROW OF EIGHT DOUBLES in device memory.
 * Nothing is read back: a caller evaluates frame after frame into a table and reads the table once.
 *   valid = gt_depth > 0, presence = silhouette > sil_thres;
 *   sil_mask = 1 (the reference's `mapping_iters == 0 and not add_new_gaussians` branch): images are weighted by presence * valid
 *     and the depth difference by presence; sil_mask = 0: images by valid;
 *   PSNR = mean over r, g, b of 20 log10(1 / sqrt(mean over ALL H * W pixels of (weighted_im - weighted_gt)^2)) (calc_psnr,
 *     /root/reference/utils/slam_external.py:49-51: masked pixels count as zeros);
 *   depth RMSE = sum(sqrt(d^2) * valid) / sum(valid) -- the reference takes the root per pixel, so its "RMSE" IS the L1 below; both
 *     slots are kept, as both of its files are;
 *   MS-SSIM = pytorch_msssim.ms_ssim(weighted_im, weighted_gt, data_range = 1): 11-tap sigma-1.5 window without padding, five
 *     levels, 2 x 2 average pooling between them (an odd dimension is zero-padded in front), weights 0.0448 0.2856 0.3001 0.2363
 *     0.1333 (restated in splatam_amd/slam.py `ms_ssim`; upstream asserts min(H, W) > 160, and so does this).
 * A count of zero valid pixels or a NaN in a plane gives what the torch expressions give (inf / NaN); no special cases.
 * With cfg->holes (eval_nvs(), /root/reference/utils/eval_helpers.py:708-712) the first-level kernel also counts the HOLES of a novel view,
 *   pixels with gt_depth > 0 && !(silhouette > sil_thres) -- the frame has depth where the map shows nothing; a NaN silhouette is a hole --,
 *   into row slot SPLAT_EVAL_HOLES.  The count does not depend on sil_mask or ms_ssim, costs no pass and no launch, and needs the silhouette.
 *   The reference counts a frame towards its novel-view averages unless holes / (H * W) * 100 > 0.1 in float32.
 * LPIPS goes into row slot SPLAT_EVAL_LPIPS when the caller supplies AlexNet weights (splat_lpips_planes, "LPIPS" below); this library
 *   carries none, and without them the slot stays 0.
 * ------------------------------------------------------------------------------------------------------------ */
#define SPLAT_EVAL_ROW 8         /* doubles per output row */
#define SPLAT_EVAL_PSNR 0
#define SPLAT_EVAL_DEPTH_RMSE 1
#define SPLAT_EVAL_DEPTH_L1 2
#define SPLAT_EVAL_MS_SSIM 3     /* NaN when cfg->ms_ssim is 0 */
#define SPLAT_EVAL_VALID 4       /* number of pixels with gt_depth > 0 */
#define SPLAT_EVAL_FLAGGED 5     /* != 0: the render behind this row ran on truncated / unsorted lists (st.status OVERFLOW or STALE_HINT):
                                    re-size the lists and evaluate the frame again (splat_iter_eval only; 0 from splat_eval_metrics) */
#define SPLAT_EVAL_HOLES 6       /* number of holes when cfg->holes is set, otherwise 0 */
#define SPLAT_EVAL_LPIPS 7       /* (added within ABI 17) 0 from the entries above; splat_lpips_planes writes it when the caller asks */
#define SPLAT_EVAL_LEVELS 5
#define SPLAT_EVAL_SUMS 40       /* doubles per copy of SplatEvalWorkspace.sums: [0..2] squared error per channel, [3] depth term, [4] valid count, [5] hole count (cfg->holes),
                                    [8 + 6 level + 2 channel] sum of the contrast-structure term, [... + 1] sum of ssim over the level's window positions */

typedef struct SplatEvalConfig {
    float sil_thres;
    int32_t sil_mask;            /* 1: presence * valid weighting (see above) */
    int32_t ms_ssim;             /* 0: PSNR and depth only (one kernel less per level; any frame size) */
    int32_t holes;               /* != 0: also count the holes into SPLAT_EVAL_HOLES (needs the silhouette) */
} SplatEvalConfig;

/* The evaluation's own scratch (it borrows nothing of SplatIterWorkspace: map edits and iterations own ssim_maps / sums). */
typedef struct SplatEvalWorkspace {
    float *pyramid;              /* pooled weighted_im and weighted_gt of levels 1..4, three channels each (NULL without MS-SSIM) */
    double *sums;                /* [SPLAT_ITER_SUM_COPIES + 1][SPLAT_EVAL_SUMS]: the copies the workgroups add into -- zero before the first call,
                                    left zeroed by every call --, then one row the finish kernel leaves the frame's TOTALS in (a report
                                    for tests and tools: the level means are totals / window positions) */
} SplatEvalWorkspace;
#define SPLAT_EVAL_LAYOUT_MS_SSIM 1 /* splat_eval_workspace_layout: with the pyramid (needs min(width, height) > 160) */
/* Arrays "pyramid" (with SPLAT_EVAL_LAYOUT_MS_SSIM) and "sums" in the SplatArrayInfo convention; returns their number or -SPLAT_E_INVALID. */
int splat_eval_workspace_layout(int32_t width, int32_t height, int32_t flags, SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes);
int splat_eval_workspace_bind(SplatEvalWorkspace *ews, void *slab, const SplatArrayInfo *arrays, int32_t n);

/* The metric kernels alone, on caller-supplied planes (a render of the drop-in rasterizer, or of anything else): rgb [3][H][W],
 * depth [H][W], silhouette [H][W] (may be NULL with sil_mask 0 and holes 0), gt_im [3][H][W], gt_depth [H][W]; out_row: SPLAT_EVAL_ROW device doubles.
 * At most six launches (five levels + finish), two without MS-SSIM.  SPLAT_E_INVALID with cfg->ms_ssim when min(width, height) <= 160. */
int splat_eval_metrics(int32_t width, int32_t height, const float *rgb, const float *depth, const float *silhouette, const float *gt_im,
                       const float *gt_depth, const SplatEvalConfig *cfg, const SplatEvalWorkspace *ews, double *out_row, void *stream);

/* splat_iter_render of `map` at pose frame->time_idx followed by splat_eval_metrics of ws->out6 against frame->im / frame->depth;
 * the render's capacity status goes into out_row[SPLAT_EVAL_FLAGGED].  Leaves the workspace as splat_iter_render leaves it. */
int splat_iter_eval(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatEvalConfig *cfg,
                    SplatIterWorkspace *ws, const SplatEvalWorkspace *ews, double *out_row, void *stream);

/* The three frame entries below are ONE resampling pass (csrc/frameprep.hip, arithmetic in csrc/frame_math.h) under three contracts; their
 * Python forms, on the device and in torch, are splatam_amd/frames.py. */

/* Frame preparation: a frame as a dataset hands it over -- color_hwc [src_h][src_w][3] in 0..255, depth_hw [src_h][src_w] (the
 * trailing 1 of [H][W][1] changes nothing) -- to the planes every other entry takes: im_out [3][dst_h][dst_w] in 0..1 (one float32
 * division by 255), depth_out [dst_h][dst_w].  With dst == src this is the layout change alone.  Otherwise colour is resampled
 * bilinearly on the 0..255 values with pixel centres at half-integers (per axis f = (d + 0.5) * src / dst - 0.5, taps floor(f) and the
 * next, clamped to the row with weight 0) and depth takes the nearest source pixel min(floor(d * (1 / (dst / src))), src - 1), the index
 * evaluated in double: the documented rules of cv2.resize INTER_LINEAR / INTER_NEAREST, which the reference's datasets apply on the host
 * (csrc/frame_math.h; restated, not checked against OpenCV itself).  One launch on `stream`, no allocation, nothing read back; the
 * outputs may be views into larger buffers (16-byte stores are used only where width and alignment allow). */
int splat_frame_prepare(int32_t src_w, int32_t src_h, const float *color_hwc, const float *depth_hw, int32_t dst_w, int32_t dst_h,
                        float *im_out, float *depth_out, void *stream);

/* Frame ingest, the step before: what an image decoder leaves -- rgb_hwc [color_h][color_w][3] bytes and depth_raw [depth_h][depth_w],
 * the integers of a 16-bit depth PNG, whose size may differ from the colour image's (ScanNet) -- to the frame a dataset hands over:
 * color_out_hwc [dst_h][dst_w][3] float32 in 0..255 and depth_out [dst_h][dst_w] float32 in metres.  Colour is resampled with the
 * rules of splat_frame_prepare on the byte values (no division: at dst == colour size every output is the byte itself, exactly);
 * depth takes the nearest source pixel by the same index rule and is float32(double(raw) / png_depth_scale): one division in double,
 * one narrowing, which is what the reference's datasets compute on the host (bit-equal for every uint16 and every scale > 0).  The
 * loop's planes follow by splat_frame_prepare or by permute / 255.  One launch on `stream`, no allocation, nothing read back; the
 * outputs may be views into larger buffers (16-byte stores are used only where dst_w is a multiple of 4 and both outputs start on
 * 16 bytes).  SPLAT_E_INVALID for a non-positive size or scale and for NULL pointers. */
int splat_frame_ingest(int32_t color_w, int32_t color_h, const uint8_t *rgb_hwc, int32_t depth_w, int32_t depth_h, const uint16_t *depth_raw,
                       double png_depth_scale, int32_t dst_w, int32_t dst_h, float *color_out_hwc, float *depth_out, void *stream);

/* Both steps in one launch, for frames that arrive one at a time from a sensor or a decoder: rgb_hwc [color_h][color_w][3] bytes and
 * depth_raw [depth_h][depth_w] at a size of its own (smaller than the destination too: a 256 x 192 LiDAR image under 960 x 720) -> the
 * loop's planes im_out [3][dst_h][dst_w] in 0..1 and depth_out [dst_h][dst_w] in metres.  Colour: the blend of splat_frame_ingest on the
 * byte values, then ONE float32 division by 255 -- the operations of splat_frame_ingest followed by splat_frame_prepare at equal size
 * in their order, so the planes are bit-equal to that pair's (float32(byte) / 255 at dst == colour size).  Depth: the nearest source
 * pixel; SPLAT_DEPTH_U16: float32(double(raw) / depth_scale) as splat_frame_ingest; SPLAT_DEPTH_F32: the source float's 32 bits, copied
 * (zeros, negatives, inf and NaN payloads unchanged: the loop's masks decide), depth_scale must be 1.0.  One launch on `stream`, no
 * allocation, nothing read back; the outputs may be views into larger buffers (16-byte stores only where dst_w is a multiple of 4 and
 * both outputs start on 16 bytes).  SPLAT_E_INVALID for a non-positive size or scale, an unknown depth_type, a scale other than 1.0
 * with SPLAT_DEPTH_F32 and for NULL pointers. */
#define SPLAT_DEPTH_U16 0
#define SPLAT_DEPTH_F32 1
int splat_frame_ingest_planes(int32_t color_w, int32_t color_h, const uint8_t *rgb_hwc, int32_t depth_w, int32_t depth_h, const void *depth_raw,
                              int32_t depth_type, double depth_scale, int32_t dst_w, int32_t dst_h, float *im_out, float *depth_out, void *stream);

/* The view layer (csrc/view.hip, arithmetic in csrc/view_math.h): any view of the map as display bytes and a point cloud, on the
 * device.  One struct for both entry points; each reads the fields under its name and `width`, `height`, the intrinsics.
 *
 * splat_view_camera: one small launch that writes what a camera of the fused iteration reads -- w2c (16 floats row-major: what
 * SplatFrameData.w2c points to), viewmatrix (its transpose), projmatrix ((P w2c)^T with the OpenGL-style P of the reference's
 * setup_camera, /root/reference/utils/recon_helpers.py:8-13) and campos (-R^T t, 3 floats) -- into buffers the caller owns, so that ONE
 * SplatCamera renders from any pose without a host read.  The pose is either `w2c_in` (16 device floats, row-major, rigid) or, with
 * w2c_in == NULL, the map's pose of frame `time_idx`: first_w2c . rel_w2c[time_idx] with rel_w2c from cam_unnorm_rots / cam_trans
 * ([1][4][num_frames] / [1][3][num_frames]) as transform_to_frame forms it.  `offset` (HOST pointer to 16 doubles, row-major, or NULL)
 * is multiplied from the left (the follow camera of the reference's online viewer).  Evaluated in double, each output rounded once.
 *
 * splat_view_finish: one streaming pass over out6 ([6][height][width]: r, g, b, depth, silhouette, depth^2); every output is optional
 * (NULL = not asked for).
 *   rgb8   [height][width][3] bytes.  SPLAT_VIEW_COLOR: c = rgb + (1 - silhouette) bg (the composite ran on a zero background and the
 *          weights sum to the silhouette), clamped to 0..1 (NaN -> 0), times 255, rounded to nearest.  SPLAT_VIEW_DEPTH: row
 *          trunc(clip((depth - vmin) / (vmax - vmin), 0, 1) * 255) of `lut` ([256][3] device bytes; vmin == vmax: row 255 above vmin, else
 *          row 0).  SPLAT_VIEW_SILHOUETTE: grey 1 - silhouette.
 *   points [height * width][3] floats: pixel (u, v) at depth z as c2w ((u - cx) / fx z, (v - cy) / fy z, z), c2w the rigid inverse of
 *          `w2c` (device, as splat_view_camera wrote it; read only when points are asked for).
 *   colors [height * width][3] floats: what SPLAT_VIEW_COLOR shows, in 0..1.
 * 16-byte loads and stores where width is a multiple of 4, out6 / points / colors start on 16 bytes and rgb8 on 4; a scalar path
 * otherwise.  No allocation, nothing read back.  SPLAT_E_INVALID for a non-positive size, NULL inputs an asked-for output needs, an
 * unknown mode, a time_idx outside the map. */
#define SPLAT_VIEW_COLOR 0
#define SPLAT_VIEW_DEPTH 1
#define SPLAT_VIEW_SILHOUETTE 2
typedef struct SplatViewArgs {
    int32_t width, height;
    double fx, fy, cx, cy, near_z, far_z;
    /* splat_view_camera */
    const float *w2c_in;
    const float *cam_unnorm_rots, *cam_trans, *first_w2c;
    int32_t num_frames, time_idx;
    const double *offset;        /* HOST, or NULL */
    float *w2c, *viewmatrix, *projmatrix, *campos;     /* outputs of splat_view_camera; w2c is an input of splat_view_finish (points) */
    /* splat_view_finish */
    const float *out6;
    int32_t mode;
    float bg[3];
    float vmin, vmax;
    const uint8_t *lut;
    uint8_t *rgb8;
    float *points, *colors;
} SplatViewArgs;
int splat_view_camera(const SplatViewArgs *view, void *stream);
int splat_view_finish(const SplatViewArgs *view, void *stream);

/* The view overlay (csrc/viewoverlay.hip, arithmetic in csrc/viewoverlay_math.h; added within ABI 17): the cameras of a run, its
 * trajectory and the centres of the map's Gaussians drawn into a view -- what the reference's viewers show besides the composite
 * (/root/reference/viz_scripts/final_recon.py:194-223, online_recon.py:245-273 and its render_mode 'centers').  Caller's stream, caller's
 * memory, no allocation, nothing read back.
 *
 * The KEY PLANE keys [height][width] uint64: splat_view_overlay_clear sets it to all ones; splat_view_points and splat_view_segments
 * enter primitives by unsigned 64-bit atomic minimum of (bits(z) << 32) | id (device scope, as splat_mesh_visibility).  z: the float32
 * camera-space depth (positive: its bits order like the floats).  id: bit 31 set = a segment, the other bits its index in the segment
 * array; bit 31 clear = a row of the map.  Equal depth bits resolve to the lowest id, so points win over segments; the plane holds the
 * same bits on every run and for every order of the launches.  The camera: w2c (16 device floats, row-major, as splat_view_camera
 * writes them), pinhole fx, fy, cx, cy, near plane near_z > 0.
 *
 * splat_view_run_segments: one lane per frame t of [first, first + count) of a run of num_frames frames.  The pose is the map's,
 * first_w2c . rel_w2c[t] exactly as splat_view_camera composes it (double), or, with w2c_all != NULL, row t of w2c_all [num_frames][16];
 * c2w is its rigid inverse.  Written into segments [.][6] float32 (two world points) and colors [.][3] bytes:
 *   trajectory  segment t - 1 (t > 0): camera centre t - 1 -> centre t, colour cool(0.5 (t - 1) / (num_frames - 1) + 0.5);
 *   frustum     (frusta != 0) segments num_frames - 1 + 8 t ..: apex = the centre, corners c2w (K^-1 (u, v, 1) scale) for
 *               (u, v) = (0, 0), (width - 1, 0), (width - 1, height - 1), (0, height - 1) with K of fx, fy, cx, cy; apex-corner x 4,
 *               then the rectangle; colour cool(0.5 t / num_frames).  A stated definition: Open3D's create_camera_visualization as
 *               recalled, with the viewers' scale 0.045 as the usual value; no parity with Open3D is claimed.
 *   cool(x)     entry min(int(256 x), 255) of matplotlib's 256-entry `cool`, entry i = (i / 255, 1 - i / 255, 1), as the bytes
 *               round(255 v) = (i, 255 - i, 255).  With fixed_color != 0 every segment gets `color` instead.
 * A prefix of each part is "the run up to t".  Endpoints are evaluated in double and rounded once.
 *
 * splat_view_points: one lane per row of means3D [count][3]: pc = w2c p; skipped unless pc.z > near_z; the pixel is
 * (floor(fx pc.x / pc.z + cx + 0.5), floor(fy pc.y / pc.z + cy + 0.5)) as for mesh vertices below; the footprint is the square of
 * point_size (1..8) pixels from pixel - (point_size - 1) / 2, clipped to the image; id = row.  Non-finite centres write nothing.
 *
 * splat_view_segments: segments [first, first + count) of an array as splat_view_run_segments writes it, id = index in the array.
 * Each is clipped in camera space to z >= near_z, projected, clipped to the pixels' rectangle (Liang-Barsky, double), and walked along
 * its major axis from the end with the smaller major coordinate: one step per pixel centre the clipped span covers along that axis
 * (a span that covers none, a zero-length segment among them: one step where it starts), the minor pixel floor(minor + 0.5), one stamp of
 * line_width (1..4) pixels across the minor axis per step, at most max(width, height) + 1 steps; depth is interpolated perspective-correctly (1 / z linear on the screen) and rounded to float32 once
 * per step.  A segment and its reverse give the same keys.  A non-finite endpoint or a segment wholly behind near_z writes nothing; a
 * zero-length segment writes one stamp.  One wave per segment.
 *
 * splat_view_overlay_finish: one lane per pixel, after splat_view_finish wrote the scene's bytes.  Where the key is not all ones:
 * z its high word, d = depth[pixel] (depth: out6's plane 3, or NULL = no scene); the primitive's bytes replace rgb8's iff occlude == 0
 * or d <= 0 or z <= d.  A point's bytes: round(255 clamp01(rgb_colors[row][c])) as splat_view_finish rounds; a segment's: its
 * segment_colors entry; ids outside num_rows / num_segments change nothing.  With fill != 0 every pixel nothing is drawn on gets bg
 * (the `centers` picture: no composite runs).
 *
 * SPLAT_E_INVALID for a NULL struct or array that is needed, a non-positive size, a size outside its range, a negative range. */
#define SPLAT_VIEW_MAX_POINT_SIZE 8
#define SPLAT_VIEW_MAX_LINE_WIDTH 4
#define SPLAT_VIEW_FRUSTUM_SEGMENTS 8
typedef struct SplatViewOverlay {
    int32_t width, height;
    float fx, fy, cx, cy, near_z;
    const float *w2c;
    uint64_t *keys;
} SplatViewOverlay;
typedef struct SplatViewRun {
    int32_t num_frames, first, count;
    const float *w2c_all;                                   /* [num_frames][16], or NULL: */
    const float *cam_unnorm_rots, *cam_trans, *first_w2c;   /* [1][4][num_frames], [1][3][num_frames], [16] */
    int32_t width, height;
    double fx, fy, cx, cy, scale;
    int32_t frusta, fixed_color;
    uint8_t color[4];                                       /* r, g, b (the fourth byte is not read) */
    float *segments;
    uint8_t *colors;
} SplatViewRun;
typedef struct SplatViewOverlayFinish {
    const float *depth;
    int32_t occlude, fill;
    const float *rgb_colors;
    int32_t num_rows;
    const uint8_t *segment_colors;
    int32_t num_segments;
    float bg[3];
    uint8_t *rgb8;
} SplatViewOverlayFinish;
int splat_view_run_segments(const SplatViewRun *run, void *stream);
int splat_view_overlay_clear(const SplatViewOverlay *view, void *stream);
int splat_view_points(const SplatViewOverlay *view, const float *means3D, int32_t count, int32_t point_size, void *stream);
int splat_view_segments(const SplatViewOverlay *view, const float *segments, int32_t first, int32_t count, int32_t line_width, void *stream);
int splat_view_overlay_finish(const SplatViewOverlay *view, const SplatViewOverlayFinish *finish, void *stream);

/* The mesh layer (csrc/tsdf.hip, arithmetic in csrc/tsdf_math.h; added within ABI 17): composites of the map at known poses fused into
 * a truncated signed distance volume on the device, and the volume's zero surface as a triangle mesh.
 *
 * The volume: grid points p(i, j, k) = origin + voxel (i, j, k), nx ny nz of them (fewer than 2^40), x fastest; five float32 arrays of
 * that many elements in the caller's memory: tsdf (reset 1), weight (reset 0), r, g, b (reset 0).  splat_tsdf_bytes: the bytes of
 * all five together (0 for a volume that would be refused).  splat_tsdf_reset: one launch.
 *
 * splat_tsdf_integrate: one launch per view.  For every grid point: pc = w2c p (w2c: 16 device floats, row-major, as
 * splat_view_camera writes them); skip unless pc.z > 0; the pixel is (floor(fx pc.x / pc.z + cx + 0.5), floor(fy pc.y / pc.z + cy + 0.5)),
 * skip outside the image; s = out6's silhouette there, skip unless s > sil_thres; d = depth / s, skip unless d > 0 and (depth_max > 0)
 * d <= depth_max; sdf = d - pc.z, skip when sdf < -trunc; f = min(1, sdf / trunc); W' = W + 1, tsdf = (tsdf W + f) / W', r / g / b the
 * same running mean of clamp(rgb / s, 0, 1); W = min(W', weight_max) when weight_max > 0.  Bricks of the grid outside the view's
 * frustum are not touched; 16-byte volume accesses where nx is a multiple of 4 and the five arrays start on 16 bytes, a scalar path
 * otherwise; out6 ([>= 5][height][width]) may be a view into a larger buffer.  `skip` (device int32, or NULL): when it holds a
 * non-zero value -- the truncation status of the render behind out6 -- the launch leaves the volume as it is and adds 1 to `skipped`
 * (device int32): nothing is read on the host per view.
 *
 * splat_tsdf_triangles: marching tetrahedra on Kuhn's split (six tetrahedra along the paths c -> c + e_a -> c + e_a + e_b -> c + (1, 1, 1))
 * of every cell whose eight corners have weight >= min_weight; a corner is inside when tsdf < 0.  Each triangle is three VERTEX KEYS,
 * key = linear(a) 8 + (dx + 2 dy + 4 dz) for the vertex on the grid edge from corner a to a + (dx, dy, dz), wound with the normal
 * towards positive tsdf (by the sign pattern alone; zero-area triangles at corners that are exactly zero are kept: the surface stays
 * closed).  keys: [capacity][3] int64; count: one device int64 that receives the number of triangles the volume asks for, whether or
 * not they fit (the call zeroes it first); nothing is written at or beyond `capacity`, in no particular order below it.
 * splat_tsdf_cubes: the same pass by MARCHING CUBES -- same arguments, same cells, same keys, same count and capacity rules --: vertices
 * on the twelve axis edges of a cell only (keys with dx + 2 dy + 4 dz in {1, 2, 4}: the keys, positions and colours the tetrahedra give
 * on those edges), at most 5 triangles per cell against 12, a third of the triangles and a third to a half of the vertices.  The case table follows from
 * one rule on sign patterns (csrc/tsdf_math.h "SURFACE, cubes"): on every face of a cell, walked counter-clockwise seen from outside,
 * each run of inside corners gives one directed segment, so two diagonal inside corners are cut off one by one; the segments chain
 * into loops, fanned from their lowest edge.  Neighbouring cells put reversed segments on their shared face, so the mesh is a closed
 * oriented cycle wherever the volume was seen.  Not the asymptotic decider / MC33, not any library's table, no dual contouring; on
 * adversarial sign noise a few edges can be shared by four triangles (each direction as often as its reverse).
 * splat_tsdf_cubes_table: a host copy of that table, out[256][16] int8: row = inside mask (bit c: corner dx + 2 dy + 4 dz), the
 * number of triangles, then three edge numbers each (edge = 4 axis + n: from the n-th corner, ascending, whose bit `axis` is clear).
 * splat_tsdf_vertices: vertices [n][3] (and colors [n][3], or NULL) of n keys: p(a) + t (p(b) - p(a)) with t = f_a / (f_a - f_b), the
 * colour interpolated alike.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for non-positive sizes, voxel or trunc, NULL
 * pointers, and nx ny nz >= 2^40. */
typedef struct SplatTsdfVolume {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel, trunc;
    float *tsdf, *weight, *r, *g, *b;
} SplatTsdfVolume;
typedef struct SplatTsdfView {
    int32_t width, height;
    float fx, fy, cx, cy;
    float sil_thres, depth_max, weight_max;
    const float *out6;
    const float *w2c;
    const int32_t *skip;
    int32_t *skipped;
} SplatTsdfView;
size_t splat_tsdf_bytes(const SplatTsdfVolume *volume);
int splat_tsdf_reset(const SplatTsdfVolume *volume, void *stream);
int splat_tsdf_integrate(const SplatTsdfVolume *volume, const SplatTsdfView *view, void *stream);
int splat_tsdf_triangles(const SplatTsdfVolume *volume, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream);
int splat_tsdf_cubes(const SplatTsdfVolume *volume, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream);
int splat_tsdf_cubes_table(int8_t *out /* [256][16] */);
int splat_tsdf_vertices(const SplatTsdfVolume *volume, const int64_t *keys, int64_t n, float *vertices, float *colors, void *stream);

/* The mesh layer on a SPARSE volume (csrc/tsdf_sparse.hip; added within ABI 17): the same virtual grid, of which only BRICKS near
 * observed surfaces are stored.  A brick is brick[0] x brick[1] x brick[2] = 2048 grid points, x fastest inside it, 8 KiB contiguous per
 * array in a POOL of `slots` bricks (tsdf, weight, r, g, b: [slots][2048] float32 each, 16-byte aligned); `directory`
 * ([ceil(nx / brick[0]) ceil(ny / brick[1]) ceil(nz / brick[2])] int32, x fastest) holds the slot of every brick of the grid or -1,
 * `brick_of_slot` ([slots] int32) the brick of every slot.  splat_tsdf_sparse_brick_shape(n, shape): the n-th brick shape the library
 * accepts (0: the default), returns how many there are.  splat_tsdf_sparse_bytes: pool + directory + brick_of_slot for the struct's
 * grid, shape and `slots` (0 for a volume that would be refused; the pointers are not looked at).
 *
 * splat_tsdf_sparse_mark: one launch per view, one lane per pixel.  A pixel that passes splat_tsdf_integrate's gates (the depth limit
 * widened to depth_max + trunc) stores 1 into flags[brick] (int32 [bricks], the caller zeroes it once) for every brick that meets a
 * conservative index box around the grid points that pixel can update with f < 0, their 3 x 3 x 3 neighbourhood included: the eight
 * corners of the frustum segment of (u +- 0.5, v +- 0.5) between depths d and d + trunc, in world space, half a voxel and one index
 * wider.  Every cell that can emit a triangle has all eight corners in a marked brick.  `skip` / `skipped` as in splat_tsdf_integrate.
 * Allocation is the caller's: slots for the marked bricks that have none (any deterministic order), then splat_tsdf_sparse_reset_slots
 * over the new slot range [first, first + count): tsdf = 1, the rest 0.
 *
 * splat_tsdf_sparse_integrate: splat_tsdf_integrate's update, the same float32 operations in the same order, on every grid point of
 * every allocated brick: a brick allocated before the first view and given every view holds the dense volume's bits.
 * splat_tsdf_sparse_triangles / _vertices: splat_tsdf_triangles / _vertices with the same keys (they name edges of the virtual grid);
 * a cell belongs to the brick of its corner 0 and emits nothing when a brick of one of its corners is not allocated.
 * splat_tsdf_sparse_cubes: splat_tsdf_cubes on the sparse volume, with splat_tsdf_sparse_triangles' arguments and cell rule.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for what splat_tsdf_* refuse, a brick shape that
 * is not listed, slots < 0, 2^31 bricks or more, and NULL pointers where they are used. */
typedef struct SplatTsdfSparse {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel, trunc;
    int32_t brick[3];
    int32_t slots;
    int32_t *directory;
    int32_t *brick_of_slot;
    float *tsdf, *weight, *r, *g, *b;
} SplatTsdfSparse;
int splat_tsdf_sparse_brick_shape(int index, int32_t *shape);
size_t splat_tsdf_sparse_bytes(const SplatTsdfSparse *volume);
int splat_tsdf_sparse_mark(const SplatTsdfSparse *volume, const SplatTsdfView *view, int32_t *flags, void *stream);
int splat_tsdf_sparse_reset_slots(const SplatTsdfSparse *volume, int64_t first, int64_t count, void *stream);
int splat_tsdf_sparse_integrate(const SplatTsdfSparse *volume, const SplatTsdfView *view, void *stream);
int splat_tsdf_sparse_triangles(const SplatTsdfSparse *volume, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream);
int splat_tsdf_sparse_cubes(const SplatTsdfSparse *volume, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream);
int splat_tsdf_sparse_vertices(const SplatTsdfSparse *volume, const int64_t *keys, int64_t n, float *vertices, float *colors, void *stream);

/* The mesh score layer (csrc/meshscore.hip, arithmetic in csrc/meshscore_math.h; added within ABI 17): points sampled uniformly by area
 * on a triangle mesh, and the exact nearest target of every query through a uniform grid -- what accuracy, completion and completion
 * ratio of a reconstruction against a ground-truth mesh are made of.
 *
 * splat_mesh_areas: area [num_faces] double of faces [num_faces][3] int32 over vertices [num_vertices][3] float32: half the norm of
 * (b - a) x (c - a), formed in double from the float32 vertices; 0 for a face with an index outside the vertices or an area that is
 * not > 0.  The caller forms the INCLUSIVE prefix sum.
 * splat_mesh_sample: sample i of n (points [n][3] float32, face [n] int32): (u0, u1, u2) = Philox4x32-10 of the counter (i, 0) under the
 * key `seed`, words 0..2 as (word >> 8) 2^-24; the face is the first whose prefix exceeds (double)u0 prefix[num_faces - 1] (a zero-area
 * face is never chosen); (u1, u2) become (1 - u1, 1 - u2) when u1 + u2 > 1; the point is (a + u1 (b - a)) + u2 (c - a) in float32, one
 * operation per step.  Sample i depends on (seed, i) alone.  A mesh without area: face -1, point 0.
 *
 * SplatNnGrid: cells of edge `cell` from `lo`, dims[0] dims[1] dims[2] <= SPLAT_NN_MAX_CELLS of them; the cell of a point is
 * floor((p - lo) / cell) per axis in float32, clamped into the grid (so every point has one); key = (z dims[1] + y) dims[0] + x.
 * splat_nn_cell_keys: key [n] int32 of points [n][3] -- targets and queries alike; the caller sorts both by key (a stable sort).
 * splat_nn_cell_starts: from the `count` targets' sorted keys and the sort's permutation `order` (sorted position -> original index):
 * records [count] of 16 bytes (x, y, z float32, original index int32; 16-byte aligned) and start [cells + 1] int32, start[k] the first
 * sorted position with key >= k.  The grid's `records` and `start` are those two arrays.
 * splat_nn_query: for query order[i] (order == NULL: i), i < n: dist2 and index of its nearest target, stored at the query's ORIGINAL
 * position.  d2 = (dx dx + dy dy) + dz dz in float32; the least d2 wins, the lowest original index among equals.  The search walks
 * Chebyshev shells of cells outward from the query's (clamped) cell and stops only when best d2 < b^2 (1 - 2^-20), b the query's
 * distance to the complement of the box of the shells searched, with its planes moved towards the query by 4 2^-24 of their offset
 * from `lo` (the float32 rounding of the cell assignment) and b = 0 while the query is outside the box or b <= 1e-15 -- or when the
 * shells cover the grid.  Exact: the result is that of comparing every target, no distance clamp.  No target: dist2 +inf, index -1.  `account`
 * (or NULL): [n][2] int32, candidates evaluated and shells walked per query.
 * splat_nn_reduce: row[0..3] = (sum of d, count of d < threshold, max of d, n) over d = sqrt((double)dist2[i]) as doubles, through
 * `partials` (3 SPLAT_NN_REDUCE_ROWS doubles of scratch) in a fixed order, without atomics: the same bits on every run.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for negative sizes, NULL pointers where
 * something would be read or written, a grid with a non-positive or non-finite cell, non-finite lo, non-positive dims or more than
 * SPLAT_NN_MAX_CELLS cells, and records that are not 16-byte aligned. */
#define SPLAT_NN_MAX_CELLS (1 << 21)
#define SPLAT_NN_REDUCE_ROWS 256
typedef struct SplatNnGrid {
    float lo[3];
    float cell;
    int32_t dims[3];
    int32_t count;
    const float *records;
    const int32_t *start;
} SplatNnGrid;
int splat_mesh_areas(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, double *area, void *stream);
int splat_mesh_sample(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const double *prefix, uint64_t seed,
                      int64_t n, float *points, int32_t *face, void *stream);
int splat_nn_cell_keys(const SplatNnGrid *grid, const float *points, int64_t n, int32_t *key, void *stream);
int splat_nn_cell_starts(const SplatNnGrid *grid, const int32_t *sorted_key, const int32_t *order, const float *points, float *records,
                         int32_t *start, void *stream);
int splat_nn_query(const SplatNnGrid *grid, const float *points, const int32_t *order, int64_t n, float *dist2, int32_t *index, int32_t *account,
                   void *stream);
int splat_nn_reduce(const float *dist2, int64_t n, double threshold, double *partials, double *row, void *stream);

/* The mesh render layer (csrc/meshrender.hip, arithmetic in csrc/meshrender_math.h; added within ABI 17): the depth image of a triangle
 * mesh, how many of a set of views see each vertex, and the sums depth L1 between two depth images is made of -- what culling a mesh to
 * the frusta a run saw and the protocol's depth L1 on rendered mesh views are made of.
 *
 * The camera is splat_tsdf_integrate's: w2c is 16 device floats, row-major, as splat_view_camera writes them; pc = w2c p per row as
 * ((m0 x + m1 y) + m2 z) + m3; pixel (i, j) looks along d = ((i - cx) / fx, (j - cy) / fy, 1); a point lands on pixel
 * (floor(fx x / z + cx + 0.5), floor(fy y / z + cy + 0.5)).  All float32, one operation per step.
 *
 * splat_mesh_depth: depth [height][width] float32 of faces [num_faces][3] int32 over vertices [num_vertices][3] float32 seen by `view`:
 * the smallest camera-space z with near_z <= z < +inf at which the pixel's ray meets a triangle, 0 where it meets none (the datasets'
 * "no depth").  Both faces of a triangle count.  With a, b, c the camera-space vertices: the edge plane of (a, b) is a x b (each
 * component one product minus one product), ALWAYS formed from the endpoint of lower vertex index first and negated when the triangle
 * names them the other way round, so the two triangles of a shared edge hold exact negatives; E(d) = (dx e0 + dy e1) + e2; the pixel is
 * covered when E_ab, E_bc, E_ca are all >= 0 or all <= 0; the hit is z = (n . a) / (n . d), n = (b - a) x (c - a),
 * n . a = (n0 ax + n1 ay) + n2 az, n . d = (dx n0 + dy n1) + n2.  There is no near-plane clipping: a triangle behind the camera gives
 * z < near_z, one that crosses z = 0 is decided by the same three signs.  A face with an index outside the vertices or a non-finite
 * vertex renders nothing.  Pixels tested per face: the box ceil(min u - 0.5) .. floor(max u + 0.5) of the projected vertices (v alike)
 * clipped to the image when all three have z > near_z; otherwise the same box of the face's part at z >= near_z (its vertices there and
 * the points where its edges meet the plane z = near_z), grown by 1 + 2^-16 max|u| pixels, or the whole image when a projection is not
 * a number.  A face whose box holds at most 16 pixels is walked by one lane; a larger one, and every face with a vertex at z <= near_z,
 * by a wave (16 was measured; splat_debug_option(5, n) moves it for measurements, the plane does not depend on it).  The plane is cleared to the bits of +inf, lowered by an
 * integer atomic min on the floats' bits and finished to 0 by the same call: the result does not depend on order and is the same bits
 * on every run.  `depth` may be one plane of a [k][height][width] buffer.  num_faces == 0 or num_vertices == 0: a plane of zeros.
 *
 * splat_mesh_seen: seen [num_vertices] int32 is INCREMENTED, per vertex, by the number of the `n` views w2c [n][16] (one size, one set
 * of intrinsics: `view`, whose own w2c and near_z are not read) in which the vertex has z > 0, lands on a pixel with
 * edge <= i <= width - 1 - edge and edge <= j <= height - 1 - edge and -- when `depth` ([n][height][width], or NULL) is given -- has
 * d = depth[view][j][i] > 0 and z <= d + eps (one float32 addition).  One lane per vertex, no atomics: exact and the same on every
 * run; incrementing lets a caller feed a long sequence in chunks of planes.
 *
 * splat_mesh_depth_compare: row[0..7] doubles from the planes a (ground truth) and b (reconstruction) of n pixels, a value that is not
 * > 0 being a hole and counting as 0: sum |a - b| over all pixels; sum |a - b| over the pixels where both are > 0; the count of those;
 * holes of a; holes of b; n; max |a - b|; 0.  Through `partials` (SPLAT_MESH_COMPARE_PARTIALS doubles of scratch) in a fixed order,
 * without atomics: the same bits on every run.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for a NULL view, a non-positive size or more
 * than 2^30 - 1 pixels, fx or fy that is zero or not finite, cx / cy not finite, near_z that is not a positive finite number
 * (splat_mesh_depth), a negative edge, eps or count, eps that is not a number, and NULL pointers where something would be
 * read or written. */
#define SPLAT_MESH_COMPARE_ROWS 256
#define SPLAT_MESH_COMPARE_PARTIALS (6 * SPLAT_MESH_COMPARE_ROWS)
typedef struct SplatMeshView {
    int32_t width, height;
    float fx, fy, cx, cy;
    float near_z;
    const float *w2c;
} SplatMeshView;
int splat_mesh_depth(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const SplatMeshView *view, float *depth,
                     void *stream);
int splat_mesh_seen(const float *vertices, int32_t num_vertices, const SplatMeshView *view, const float *w2c, int32_t n, int32_t edge,
                    const float *depth, float eps, int32_t *seen, void *stream);
int splat_mesh_depth_compare(const float *a, const float *b, int64_t n, double *partials, double *row, void *stream);

/* The mesh shade layer (csrc/meshshade.hip, arithmetic in csrc/meshshade_math.h; added within ABI 17): pictures of a triangle mesh --
 * vertex normals, a z-buffer that remembers which triangle won each pixel, and a shading pass from that buffer to display bytes.  The
 * camera, the edge planes, the coverage test and the hit are the mesh render layer's, unchanged.
 *
 * splat_mesh_vertex_normals: normals [num_vertices][3] float32, area-weighted, the same bits on every run and for every order of the
 * faces.  accum [num_vertices][3] int64 is scratch, which the call clears.  A face adds n = (b - a) x (c - a), formed in double from
 * the float32 vertices, to its three vertices as quanta rint(n_k 2^SPLAT_MESH_AREA_BITS) by 64-bit integer atomics (exact, independent
 * of order; a vertex holds 2^23 m^2 per component and wraps beyond).  A face with an index out of range, a non-finite vertex or a
 * component |n_k| >= 2^22 m^2 adds nothing; a repeated index gives n = 0.  Per vertex s = sqrt((x^2 + y^2) + z^2) on the sums converted
 * to double, each component divided and rounded once to float32; s == 0 -- a vertex no face names, faces that cancel -- gives (0, 0, 0).
 * Three launches (clear, faces, vertices); num_vertices == 0 succeeds without one.
 *
 * splat_mesh_visibility: keys [height][width] uint64: splat_mesh_depth's raster (the same setup, boxes, split and hit) with a hit
 * entering the plane by a 64-bit unsigned atomic min of ((uint64)bits(z) << 32) | face index.  The plane is cleared to all ones, which
 * stays where no triangle is met.  The high word of every other key is exactly what splat_mesh_depth holds at that pixel; among faces
 * that hit at the same z bits (every pixel on a shared edge) the LOWEST face index wins: the same keys on every run.
 *
 * splat_mesh_shade: rgb8 [H][W][3] bytes from a key plane.  `view` describes the KEY plane, which holds samples x samples sub-pixels
 * per output pixel: width = W samples, height = H samples, fx samples, fy samples, cx' = (cx + 0.5) samples - 0.5, cy' alike.  One lane
 * per output pixel (i, j) loops over the sub-pixels (i samples + a, j samples + b) in row order.  A key of all ones, a face index
 * >= num_faces and a face the raster's setup turns away are background and contribute bg.  Otherwise the winning face is set up again
 * and its edge planes at the sub-pixel's ray d give the barycentrics l_a = E_bc / S, l_b = E_ca / S, l_c = E_ab / S,
 * S = (E_ab + E_bc) + E_ca (homogeneous in camera space: perspective-correct without a division by w; S == 0: thirds).  An attribute is
 * (l_a x_a + l_b x_b) + l_c x_c.  colour: of colors [num_vertices][3] in 0..1; albedo where colors is NULL.  normal: of normals
 * [num_vertices][3], divided by its length; where that is 0, smooth == 0 or normals is NULL, the face's own (b - a) x (c - a) from the
 * world-frame vertices in float32, normalised ((0, 0, 0) without area).  The depth is the key's high word, not recomputed.
 *   SPLAT_MESH_SHADE_COLOR         colour
 *   SPLAT_MESH_SHADE_SHADED        albedo L, L = ambient + (1 - ambient) |n . w| / |w|, w = R^T d: a head light, two-sided
 *   SPLAT_MESH_SHADE_SHADED_COLOR  colour L
 *   SPLAT_MESH_SHADE_NORMAL        (n + 1) / 2; normal_frame 0: n in the mesh's frame; 1: in the camera's, negated where it looks away
 *   SPLAT_MESH_SHADE_DEPTH         row trunc(clip((z - vmin) / (vmax - vmin), 0, 1) 255) of lut (device, [256][3] bytes), as
 *                                  SPLAT_VIEW_DEPTH; background pixels hold bg here too
 * The sub-pixels' channel values are summed in float32 in loop order, multiplied by 1 / samples^2, clamped to 0..1 and rounded to
 * nearest (ties to even) as splat_view_finish rounds.  depth [H][W] float32 (0 = none; bit for bit splat_mesh_depth's plane), face
 * [H][W] int32 (-1 = none) and normal [H][W][3] float32 (the shading normal in the mesh's frame, zeros = none) are written where given,
 * with samples == 1 only.  One launch.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for what splat_mesh_depth refuses (more than
 * 2^30 - 1 pixels in the key plane among it), NULL keys, args or rgb8, samples outside 1..4 or not dividing the key plane's size, an
 * unknown mode, SPLAT_MESH_SHADE_DEPTH without lut, and depth, face or normal with samples > 1.  Empty meshes succeed: a picture of bg. */
#define SPLAT_MESH_SHADE_COLOR 0
#define SPLAT_MESH_SHADE_SHADED 1
#define SPLAT_MESH_SHADE_SHADED_COLOR 2
#define SPLAT_MESH_SHADE_NORMAL 3
#define SPLAT_MESH_SHADE_DEPTH 4
typedef struct SplatMeshShade {
    int32_t mode;                /* SPLAT_MESH_SHADE_* */
    int32_t samples;             /* sub-pixels per axis, 1..4 */
    int32_t smooth;              /* 0: every face its own normal */
    int32_t normal_frame;        /* SPLAT_MESH_SHADE_NORMAL: 0 = the mesh's frame, 1 = the camera's */
    float bg[3], albedo[3];
    float ambient;
    float vmin, vmax;            /* SPLAT_MESH_SHADE_DEPTH */
    const uint8_t *lut;
} SplatMeshShade;
int splat_mesh_vertex_normals(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, int64_t *accum, float *normals,
                              void *stream);
int splat_mesh_visibility(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const SplatMeshView *view,
                          uint64_t *keys, void *stream);
int splat_mesh_shade(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const float *colors, const float *normals,
                     const SplatMeshView *view, const uint64_t *keys, const SplatMeshShade *args, uint8_t *rgb8, float *depth, int32_t *face,
                     float *normal, void *stream);

/* The ICP layer (csrc/icp.hip, arithmetic in csrc/icp_math.h; added within ABI 17): point-to-point registration of a source cloud onto
 * the targets of a SplatNnGrid -- the alignment the NICE-SLAM mesh protocol runs before it measures (threshold 0.1 m, identity start, at
 * most 30 iterations, stop when fitness and inlier RMSE both change by less than 1e-6).  One iteration is splat_icp_transform,
 * splat_nn_query on `moved`, splat_icp_accumulate, splat_icp_solve; all arithmetic is double, one operation per step.
 *
 * state: SPLAT_ICP_STATE doubles on the device: T [16] row-major (bottom row 0 0 0 1), then SPLAT_ICP_ITERATION, SPLAT_ICP_STATUS
 * (0 running, 1 converged, 2 iteration limit, 3 fewer than three correspondences), SPLAT_ICP_FITNESS / SPLAT_ICP_RMSE of the current
 * evaluation, SPLAT_ICP_PREV_FITNESS / SPLAT_ICP_PREV_RMSE of the one before, SPLAT_ICP_COUNT (correspondences), SPLAT_ICP_POINTS (n).
 * The caller writes T and zeros before the first iteration.  history: [max_iterations + 1][4] doubles, row k = (count, fitness,
 * inlier RMSE, status after this evaluation) of iteration k.
 *
 * splat_icp_transform: moved[i] = float32(R p + t), p the float32 source point widened, per row ((r0 x + r1 y) + r2 z) + t, T read from
 * `state` on the device.
 * splat_icp_accumulate: point i is a correspondence when 0 <= index[i] < num_targets and sqrt((double)dist2[i]) < threshold (dist2 /
 * index: what splat_nn_query returned for `moved`; the comparison is splat_nn_reduce's).  partials [SPLAT_ICP_ROWS][SPLAT_ICP_SUMS]:
 * per workgroup the count, sum of (double)dist2, sum of (p' - c) [3], sum of (q - c) [3], sum of (p' - c)(q - c)^T [9] (row: p') over
 * its correspondences, p' = R p + t formed in double again (not the rounded `moved`), q = targets[index[i]] widened, c = origin: 3 HOST
 * doubles near the points (the centre of the targets' box), which only limit cancellation.  Fixed assignment of points to lanes, fixed
 * order of the wave and workgroup reductions, no atomics: the same bits on every run.  n == 0: one row of zeros.
 * splat_icp_solve (one workgroup; n, origin as given to splat_icp_accumulate): returns at once when the status is not 0 -- T is frozen,
 * iterations enqueued after the end change nothing.  Otherwise adds the rows in order; fitness = count / n, inlier RMSE =
 * sqrt(sum d2 / count), both 0 without correspondences; writes the history row; status 1 when iteration > 0 and both changed by less
 * than relative_fitness / relative_rmse since the evaluation before, else 2 when iteration == max_iterations, else 3 when count < 3;
 * while it stays 0: the proper rotation U and translation u that minimise sum |U p' + u - q|^2 (Horn's quaternion form: the eigenvector
 * of the largest eigenvalue of a symmetric 4 x 4 matrix by cyclic Jacobi sweeps; det U = +1 whatever the sums), T <- (U, u) T, current
 * becomes previous, iteration + 1.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for negative sizes or max_iterations, a
 * threshold or relative_* that is not a number, and NULL pointers where something would be read or written. */
#define SPLAT_ICP_STATE 24
#define SPLAT_ICP_ROWS 256
#define SPLAT_ICP_SUMS 17
#define SPLAT_ICP_ITERATION 16
#define SPLAT_ICP_STATUS 17
#define SPLAT_ICP_FITNESS 18
#define SPLAT_ICP_RMSE 19
#define SPLAT_ICP_PREV_FITNESS 20
#define SPLAT_ICP_PREV_RMSE 21
#define SPLAT_ICP_COUNT 22
#define SPLAT_ICP_POINTS 23
int splat_icp_transform(const float *source, int64_t n, const double *state, float *moved, void *stream);
int splat_icp_accumulate(const float *source, const float *targets, int64_t num_targets, const float *dist2, const int32_t *index, int64_t n,
                         double threshold, const double *origin, const double *state, double *partials, void *stream);
int splat_icp_solve(const double *partials, int64_t n, int32_t max_iterations, double relative_fitness, double relative_rmse,
                    const double *origin, double *state, double *history, void *stream);

/* The mesh cleaning layer (csrc/meshclean.hip, loop bodies in csrc/meshclean_math.h; added within ABI 17): connected components of a
 * triangle mesh and per-component statistics -- what removing the floaters of a fused mesh (every component below a size) is made of.
 *
 * Two vertices belong to one component when a chain of faces that share a vertex INDEX joins them; coincident vertices with different
 * indices do not connect.  A face with an index outside 0..num_vertices-1 links nothing and counts for nothing; a face with a repeated
 * index links the vertices it names and counts as a face of area 0; a vertex no face names is a component of its own, with 0 faces.
 *
 * splat_mesh_components: labels [num_vertices] int32, labels[v] = the SMALLEST vertex index of v's component: canonical, the same bits
 * on every run and for every order of the faces.  A concurrent union-find over `labels` itself (one lane per face: find with path
 * halving, the larger root hooked under the smaller by a compare-and-swap; every access an agent-scope atomic; bounded because a word
 * never holds more than its own index), then a launch that flattens.  num_faces == 0: labels[v] = v.
 *
 * splat_mesh_component_stats: five arrays indexed by ROOT LABEL, all of length num_vertices (lo / hi: [num_vertices][3]), which the call
 * initialises itself; entries of indices that are no root keep their initial value (0; SPLAT_MESH_KEY_HIGHEST in lo, _LOWEST in hi).
 * num_v / num_f: the component's vertices / faces (a face counts for the label of its first vertex).  area_q: the sum over its faces of
 * rint(area 2^SPLAT_MESH_AREA_BITS), area being splat_mesh_areas' double: a 64-bit integer sum of quanta of 2^-40 m^2, exact in the
 * quanta and independent of order; it holds 2^23 m^2 (about 8.4e6 m^2) per component and wraps beyond; a face whose area is not below
 * 2^22 m^2 (an infinite one included) adds SPLAT_MESH_AREA_BAD quanta instead.  lo / hi: the component's box as KEYS of the float32
 * coordinates, key = bits >= 0 ? bits : bits ^ 0x7fffffff on the bits as int32 (-0 taken as +0): signed integer order is the floats'
 * order for both signs, and the same expression maps a key back.  Only integer atomics: the same bits on every run.  `labels` is what
 * splat_mesh_components gave (an entry outside 0..num_vertices-1 counts for nothing).
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for negative sizes and NULL pointers where
 * something would be read or written; num_vertices == 0 succeeds without a launch. */
#define SPLAT_MESH_AREA_BITS 40
#define SPLAT_MESH_AREA_BAD (1LL << 62)
#define SPLAT_MESH_KEY_HIGHEST 2147483647
#define SPLAT_MESH_KEY_LOWEST (-2147483647 - 1)
int splat_mesh_components(const int32_t *faces, int32_t num_faces, int32_t num_vertices, int32_t *labels, void *stream);
int splat_mesh_component_stats(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const int32_t *labels,
                               int32_t *num_v, int32_t *num_f, int64_t *area_q, int32_t *lo, int32_t *hi, void *stream);

/* The mesh simplification layer (csrc/meshsimplify.hip, loop bodies in csrc/meshsimplify_math.h; added within ABI 17): vertex clustering
 * with quadric placement (P. Lindstrom, "Out-of-core simplification of large polygonal models", SIGGRAPH 2000).  All vertices in one cell
 * of a uniform grid of edge `cell` (metres) anchored at the WORLD ORIGIN become one vertex, placed where the summed plane quadrics of
 * the faces around the cell are smallest: flat regions stay flat, edges and corners stay sharp.
 *
 * splat_mesh_simplify_keys: keys [num_vertices] int64.  Per axis i = floor((double)x / cell) (negative coordinates count, x = j cell
 * belongs to cell j), |i| < 2^20; key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20); -1 for a vertex that is not finite or
 * has an index out of range.  The CLUSTER of a vertex is the rank of its key among the distinct keys in ascending order (the caller's
 * work: a stable sort, a flag where a key differs from its predecessor, a prefix sum), -1 for a key of -1; clusters < num_vertices.
 *
 * splat_mesh_simplify_vertices: ADDS, per cluster, to count [num_vertices] int32 and to words 0..5 of sums
 * [num_vertices][SPLAT_MESH_SIMPLIFY_SUMS] int64: the vertices, the sum of rint(p 2^32) (p = (x - centre) / cell, the vertex local to
 * its cell, in [-1/2, 1/2)) and, with colors, the sum of rint(colour 2^32).  The caller zeroes count and sums first.
 *
 * splat_mesh_simplify_quadrics: ADDS to words 6..15 of sums.  Per face, n = (b - a) x (c - a) in double, n^ = n / |n|, area = |n| / 2; for
 * every DISTINCT cluster g among the face's three, d = n^ . p of its first corner in g (|d| <= sqrt(3) / 2), and the ten numbers
 * area {n^ n^T (xx xy xz yy yz zz), d n^ (x y z), d^2} as rint(. 2^SPLAT_MESH_AREA_BITS).  A face adds nothing when it names a vertex
 * that does not exist or has no cluster, has no area, or has an area not below 2^22 m^2: then *refused is raised to 1 (the caller
 * zeroes it).  A word holds 2^23 m^2 of faces.
 *
 * Both add by 64-bit integer atomics only (a wave adds up runs of lanes that share a cluster by shuffles first): the sums are exact in
 * their quanta, independent of order and the same bits on every run.
 *
 * splat_mesh_simplify_place: per cluster c < num_clusters, from count, sums and cell_keys [num_clusters] (the key of the cluster's
 * cell): positions [num_clusters][3] float32, colors (the mean; may be NULL), rank, fallback (int32) and value (double).  The mean
 * m = sum p / count; with SPLAT_MESH_SIMPLIFY_QUADRIC the eigen-decomposition of A (cyclic Jacobi) and
 * p = m + sum over l_i > 1e-3 max |l| of v_i (v_i . (b - A m)) / l_i; max |l| == 0 or a p outside [-1/2, 1/2]^3 gives p = m and
 * fallback = 1.  rank: the eigenvalues used (0 with the mean); value: the quadric at p, the sum of area x (distance from the face's plane,
 * in cells)^2, as it comes out (it may be a few quanta below zero).  The vertex is centre + p cell in double, rounded once.  A cluster with count <= 0 gets zeros.
 *
 * splat_mesh_simplify_faces: triples [num_faces][3] int32: the face's three clusters rotated so that the smallest comes first (the winding
 * is kept), or (-1, -1, -1) for a face that names a vertex that does not exist or has no cluster, or two vertices of one cluster.
 *
 * Caller's stream, caller's memory, no allocation, nothing read back.  SPLAT_E_INVALID for negative sizes, a cell that is not positive
 * and finite, and NULL pointers where something would be read or written; zero sizes succeed without a launch. */
#define SPLAT_MESH_SIMPLIFY_SUMS 16
#define SPLAT_MESH_SIMPLIFY_MEAN 0
#define SPLAT_MESH_SIMPLIFY_QUADRIC 1
int splat_mesh_simplify_keys(const float *vertices, int32_t num_vertices, double cell, int64_t *keys, void *stream);
int splat_mesh_simplify_vertices(const float *vertices, const float *colors, int32_t num_vertices, const int32_t *cluster, double cell,
                                 int32_t *count, int64_t *sums, void *stream);
int splat_mesh_simplify_quadrics(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const int32_t *cluster,
                                 double cell, int64_t *sums, int32_t *refused, void *stream);
int splat_mesh_simplify_place(const int32_t *count, const int64_t *sums, const int64_t *cell_keys, int32_t num_clusters, double cell,
                              int32_t placement, float *positions, float *colors, int32_t *rank, int32_t *fallback, double *value, void *stream);
int splat_mesh_simplify_faces(const int32_t *faces, int32_t num_faces, int32_t num_vertices, const int32_t *cluster, int32_t *triples,
                              void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * LPIPS (added within ABI 17; csrc/lpips.hip, arithmetic in csrc/lpips_math.h): what the reference's eval() / eval_nvs() compute with
 * torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True) on clamp(weighted_im, 0, 1) and
 * clamp(weighted_gt_im, 0, 1), from weights THE CALLER SUPPLIES.  The definition is restated from the public implementation as recalled
 * (DESIGN.md 4): x <- 2x - 1, (x - shift_c) / scale_c with shift (-0.030, -0.088, -0.188), scale (0.458, 0.448, 0.450); the five AlexNet
 * `features` convolutions (3->64 11x11 stride 4 pad 2; maxpool 3x3 stride 2, 64->192 5x5 pad 2; maxpool, 192->384 3x3 pad 1; 384->256 3x3
 * pad 1; 256->256 3x3 pad 1), each with bias and ReLU, tapped after the ReLU; per tap and pixel u = f / (sqrt(sum_c f_c^2) + 1e-10) for
 * both images, d_l = mean over the tap's pixels of sum_c w_lc (u0_c - u1_c)^2; LPIPS = sum_l d_l.
 * The convolutions are one implicit GEMM on the exact-f32 MFMA, k = (c KH + dy) KH + dx: per 32 consecutive k a k-ordered fmaf chain
 * from zero, the blocks' sums added in order of k -- float32 as torch computes it, the same bits on every run, no atomics anywhere.  Both images go through every kernel as a batch of two, so an image
 * scored against itself -- or a frame whose every pixel is masked -- gives exactly 0.0.  Nothing is read back.
 *
 * weights: splat_lpips_weight_floats() floats on the device, in the canonical order: per layer the weight [Cout][Cin][KH][KH] then the
 * bias [Cout], conv1 .. conv5; then lin0 .. lin4 ([Cout] each, the non-negative 1x1 `lin` weights).
 * splat_lpips_pack turns them, ONCE per network, into the packed network `net` (splat_lpips_pack_floats() floats) that every other entry
 * reads: per layer the weights as [Kpad][Cout] (zero rows behind K: conv1's 363 -> 384), then the five biases, then the five lin vectors.
 * It does not depend on the image size, so it lives beside the workspaces, not in them.
 * The workspace (per image size; both extents >= SPLAT_LPIPS_MIN_SIZE, refused otherwise) holds the transformed input, the five taps,
 * the two pooled maps and the distance's double partials: arrays "input", "tap0" .. "tap4", "pool1", "pool2", "partials" in the
 * SplatArrayInfo convention.  It MUST come from splat_lpips_workspace_layout for the very size it is used at: the kernels write what the
 * size implies.  splat_lpips_workspace_bind records the size, and splat_lpips_planes / _images refuse a workspace bound for another.
 * ------------------------------------------------------------------------------------------------------------ */
#define SPLAT_LPIPS_LAYERS 5
#define SPLAT_LPIPS_MIN_SIZE 31
typedef struct SplatLpipsWorkspace {
    float *input;                        /* [2][3][H][W] */
    float *taps[SPLAT_LPIPS_LAYERS];     /* tap l: [2][C_l][H_l][W_l], C = 64, 192, 384, 256, 256 */
    float *pooled[2];                    /* what conv2 / conv3 read */
    double *partials;
    int32_t width, height;               /* the image size it was laid out and bound for (splat_lpips_workspace_bind) */
} SplatLpipsWorkspace;
size_t splat_lpips_weight_floats(void);
size_t splat_lpips_pack_floats(void);
/* extent of tap `layer` (0..4) along an image dimension of n pixels; 0 when there is none */
int32_t splat_lpips_tap_size(int32_t n, int32_t layer);
/* returns the number of arrays or -SPLAT_E_INVALID (an extent under SPLAT_LPIPS_MIN_SIZE) */
int splat_lpips_workspace_layout(int32_t width, int32_t height, SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes);
/* width, height: what splat_lpips_workspace_layout was asked for */
int splat_lpips_workspace_bind(SplatLpipsWorkspace *ws, void *slab, const SplatArrayInfo *arrays, int32_t n, int32_t width, int32_t height);
int splat_lpips_pack(const float *weights, float *net, void *stream);
/* One layer alone (tests, measurements): convolution `layer` + bias + ReLU of x [2][Cin][in_height][in_width] into
 * y [2][Cout][out_h][out_w]; no pool. */
int splat_lpips_conv(int32_t layer, int32_t in_width, int32_t in_height, const float *x, const float *net, float *y, void *stream);
/* LPIPS of an evaluated frame: weighted_im / weighted_gt_im formed from rgb [3][H][W], silhouette [H][W] (may be NULL with sil_mask 0),
 * gt_im [3][H][W], gt_depth [H][W] exactly as splat_eval_metrics forms them, clamped to 0..1; one double to out (a caller passes
 * &row[SPLAT_EVAL_LPIPS], AFTER the call that writes the row). */
int splat_lpips_planes(int32_t width, int32_t height, const float *rgb, const float *silhouette, const float *gt_im, const float *gt_depth,
                       float sil_thres, int32_t sil_mask, const float *net, const SplatLpipsWorkspace *workspace, double *out, void *stream);
/* ... of two plain images [3][H][W] in 0..1 (values outside are clamped) */
int splat_lpips_images(int32_t width, int32_t height, const float *im0, const float *im1, const float *net,
                       const SplatLpipsWorkspace *workspace, double *out, void *stream);

/* Developer switches used by scripts/ (never by the product path): key 0 = skip the per-tile count atomics of K1 (timing
 * experiment; results are then invalid); key 4 = measurement builds of the fused backward composite (bits: 1 = per-workgroup
 * wall-clock stamps into the buffer of splat_debug_stamps, 2 = stage the batches but visit nothing, 4 = no accumulator atomics,
 * 8 = phase 1 only; results are then invalid; 0 = the product kernel); key 5 = the largest pixel box one lane of splat_mesh_depth walks
 * alone (0 = the library's 16; the result does not depend on it); key 6 = measurement builds of splat_mesh_depth's raster kernel
 * (1 = a plain load in front of the atomic min spares it where the pixel already holds something nearer: the same result; 2 = a plain
 * store in place of the atomic: results are then invalid; 0 = the product kernel).  Returns the previous value, -1 for an unknown key. */
int splat_debug_option(int key, int value);
/* device buffer of 2 x (workgroups of the launch) int64 for splat_debug_option(4, 1): (start, end) of every workgroup in
 * wall_clock64() ticks (100 MHz); NULL switches it off. */
int splat_debug_stamps(void *buffer);

#ifdef __cplusplus
}
#endif
#endif /* SPLAT_HIP_H */
