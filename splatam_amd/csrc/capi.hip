// capi.hip -- the extern "C" surface declared in include/splat_hip.h.
#include <cstring>

#include "splat_device.h"
#include "lpips_math.h"
#include "tsdf_math.h"

using namespace splat;

namespace {
int check(hipError_t e) { return e == hipSuccess ? SPLAT_OK : SPLAT_E_LAUNCH; }

bool valid_inputs(const SplatCamera *cam, const SplatGaussians *g) {
    if (!cam || !g) return false;
    if (g->P < 0 || cam->image_width <= 0 || cam->image_height <= 0) return false;
    if (cam->image_width > 65535 * SPLAT_TILE || cam->image_height > 65535 * SPLAT_TILE) return false;
    if (g->channels < 1 || g->channels > SPLAT_MAX_CHANNELS) return false;
    if (!cam->viewmatrix || !cam->projmatrix) return false;         // (bg == NULL: black)
    if (g->P > 0) {
        if (!g->means3D || !g->opacities) return false;
        if ((g->colors_precomp == nullptr) == (g->shs == nullptr)) return false;
        const bool sr = g->scales && g->rotations;
        if (sr == (g->cov3D_precomp != nullptr)) return false;
        if (g->shs) {
            if (g->channels != 3 || !cam->campos || cam->sh_degree < 0 || cam->sh_degree > 3) return false;
            if (g->sh_coeffs < (cam->sh_degree + 1) * (cam->sh_degree + 1)) return false;
        }
    }
    return true;
}
bool valid_state(const SplatGaussians *g, const SplatState *st, bool need_lists) {
    if (!st || !st->tile_count || !st->tile_base || !st->tile_cursor || !st->status) return false;
    if (g->P > 0 && (!st->depth || !st->xy || !st->conic_opacity || !st->rect || !st->radii)) return false;
    if (g->shs && g->P > 0 && (!st->rgb || !st->clamped)) return false;
    // (group binning: the composite builds the lists from the group records -- no key buckets)
    const bool groups = st->group_stride > 0 && st->group_count && st->group_recs && st->tile_stride > 0;
    if (need_lists && (st->capacity < 0 || (st->capacity > 0 && ((!st->keys && !groups) || !st->point_list)))) return false;
    if (st->tile_stride < 0 || st->group_stride < 0) return false;
    return true;
}
}  // namespace

extern "C" {

const char *splat_error_string(int code) {
    switch (code) {
        case SPLAT_OK: return "ok";
        case SPLAT_E_INVALID: return "invalid argument";
        case SPLAT_E_LAUNCH: return "HIP launch failed";
        case SPLAT_E_UNSUPPORTED: return "unsupported";
        default: return "unknown error";
    }
}

int splat_abi_version(void) { return SPLAT_ABI_VERSION; }

size_t splat_sizeof(const char *name) {
    if (!name) return 0;
#define SPLAT_SIZEOF_CASE(T) if (strcmp(name, #T) == 0) return sizeof(T)
    SPLAT_SIZEOF_CASE(SplatCamera); SPLAT_SIZEOF_CASE(SplatGaussians); SPLAT_SIZEOF_CASE(SplatState); SPLAT_SIZEOF_CASE(SplatGrads);
    SPLAT_SIZEOF_CASE(SplatMap); SPLAT_SIZEOF_CASE(SplatFrameData); SPLAT_SIZEOF_CASE(SplatLossConfig); SPLAT_SIZEOF_CASE(SplatLossConfigEx); SPLAT_SIZEOF_CASE(SplatIterWorkspace);
    SPLAT_SIZEOF_CASE(SplatAdamMap); SPLAT_SIZEOF_CASE(SplatPoseAdam); SPLAT_SIZEOF_CASE(SplatMapStore); SPLAT_SIZEOF_CASE(SplatAddArgs);
    SPLAT_SIZEOF_CASE(SplatPruneArgs); SPLAT_SIZEOF_CASE(SplatDensifyArgs); SPLAT_SIZEOF_CASE(SplatArrayInfo);
    SPLAT_SIZEOF_CASE(SplatEvalConfig); SPLAT_SIZEOF_CASE(SplatEvalWorkspace); SPLAT_SIZEOF_CASE(SplatViewArgs);
    SPLAT_SIZEOF_CASE(SplatTsdfVolume); SPLAT_SIZEOF_CASE(SplatTsdfView); SPLAT_SIZEOF_CASE(SplatNnGrid); SPLAT_SIZEOF_CASE(SplatMeshView);
    SPLAT_SIZEOF_CASE(SplatLpipsWorkspace); SPLAT_SIZEOF_CASE(SplatTsdfSparse); SPLAT_SIZEOF_CASE(SplatMeshShade);
    SPLAT_SIZEOF_CASE(SplatViewOverlay); SPLAT_SIZEOF_CASE(SplatViewRun); SPLAT_SIZEOF_CASE(SplatViewOverlayFinish);
#undef SPLAT_SIZEOF_CASE
    return 0;
}

size_t splat_num_tiles(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    return (size_t)((width + SPLAT_TILE - 1) / SPLAT_TILE) * (size_t)((height + SPLAT_TILE - 1) / SPLAT_TILE);
}

// bucketed lists behind the reference API exist in ONE form: group binning with lists the composite sorts itself, three colour channels,
// buckets inside the capacity (include/splat_hip.h "GROUP BINNING behind the reference API"); anything else with tile_stride > 0 is refused
static bool valid_list_mode(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st) {
    if (st->tile_stride == 0) return true;
    if (!group_binning(*st, cam->image_width, cam->image_height) || g->channels != 3 || g->shs) return false;
    return (long long)st->tile_stride * (long long)splat_num_tiles(cam->image_width, cam->image_height) <= st->capacity && st->point_list;
}

int splat_preprocess_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, void *stream) {
    if (!valid_inputs(cam, g) || !valid_state(g, st, false) || !valid_list_mode(cam, g, st)) return SPLAT_E_INVALID;
    return check(launch_preprocess_forward(*cam, *g, *st, (hipStream_t)stream));
}

int splat_bin_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, void *stream) {
    if (!valid_inputs(cam, g) || !valid_state(g, st, true)) return SPLAT_E_INVALID;
    // (splat_preprocess_forward of the same state counted per workgroup under the same predicate)
    return check(launch_bin_forward(*cam, *g, *st, (hipStream_t)stream, true, true));
}

int splat_render_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, float *out_color,
                         float *out_depth, void *stream) {
    if (!valid_inputs(cam, g) || !valid_state(g, st, true)) return SPLAT_E_INVALID;
    if (!out_color || !out_depth || !st->final_T || !st->n_contrib || !valid_list_mode(cam, g, st)) return SPLAT_E_INVALID;
    return check(launch_render_forward(*cam, *g, *st, out_color, out_depth, (hipStream_t)stream));
}

int splat_forward(const SplatCamera *cam, const SplatGaussians *g, SplatState *st, float *out_color, float *out_depth,
                  void *stream) {
    int rc = splat_preprocess_forward(cam, g, st, stream);
    if (rc) return rc;
    rc = splat_bin_forward(cam, g, st, stream);
    if (rc) return rc;
    return splat_render_forward(cam, g, st, out_color, out_depth, stream);
}

static bool valid_grads(const SplatGaussians *g, const SplatGrads *gr) {
    if (!gr || !gr->dL_dcolor) return false;
    if (g->P > 0) {
        if (!gr->accum || !gr->dL_dmeans3D || !gr->dL_dmeans2D || !gr->dL_dopacities) return false;
        if ((gr->dL_dscales == nullptr) != (gr->dL_drotations == nullptr)) return false;
        if (g->shs ? !gr->dL_dshs : !gr->dL_dcolors) return false;
    }
    return true;
}

int splat_render_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st, SplatGrads *gr,
                          void *stream) {
    if (!valid_inputs(cam, g) || !valid_state(g, st, true) || !valid_grads(g, gr)) return SPLAT_E_INVALID;
    if (!st->final_T || !st->n_contrib) return SPLAT_E_INVALID;
    return check(launch_render_backward(*cam, *g, *st, *gr, (hipStream_t)stream));
}

int splat_preprocess_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st, SplatGrads *gr,
                              void *stream) {
    if (!valid_inputs(cam, g) || !valid_state(g, st, false) || !valid_grads(g, gr)) return SPLAT_E_INVALID;
    return check(launch_preprocess_backward(*cam, *g, *st, *gr, (hipStream_t)stream));
}

int splat_backward(const SplatCamera *cam, const SplatGaussians *g, const SplatState *st, SplatGrads *gr, void *stream) {
    int rc = splat_render_backward(cam, g, st, gr, stream);
    if (rc) return rc;
    return splat_preprocess_backward(cam, g, st, gr, stream);
}

int splat_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, uint8_t *present, void *stream) {
    if (P < 0 || (P > 0 && (!means3D || !present)) || !viewmatrix) return SPLAT_E_INVALID;
    return check(launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
}

int splat_same_geometry(int32_t P, const float *opacities_a, const float *opacities_b, const float *scales_a, const float *scales_b,
                        const float *rotations_a, const float *rotations_b, int32_t *differ, void *stream) {
    if (P < 0 || !differ) return SPLAT_E_INVALID;
    if (P > 0 && (!opacities_a || !opacities_b || !scales_a || !scales_b || !rotations_a || !rotations_b)) return SPLAT_E_INVALID;
    return check(launch_same_geometry(P, opacities_a, opacities_b, scales_a, scales_b, rotations_a, rotations_b, differ, (hipStream_t)stream));
}

int splat_time_kernel(int fn, int iters, const SplatCamera *cam, const SplatGaussians *g, SplatState *st, SplatGrads *gr,
                      float *out_color, float *out_depth, void *stream, float *ms) {
    if (!ms || iters <= 0 || !valid_inputs(cam, g) || !valid_state(g, st, true)) return SPLAT_E_INVALID;
    if (fn == 1 && !valid_grads(g, gr)) return SPLAT_E_INVALID;
    if (fn != 0 && fn != 1) return SPLAT_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return SPLAT_E_LAUNCH;
    hipError_t err = hipSuccess;
    // the accumulator memset of the backward is part of launch_render_backward; time the kernel alone
    // by issuing the memsets first and recording around the launches only for fn == 0; for fn == 1 the
    // (tiny) memset is inside the bracket and documented as such.
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters && err == hipSuccess; ++i)
        err = fn == 0 ? launch_render_forward(*cam, *g, *st, out_color, out_depth, s) : launch_render_backward(*cam, *g, *st, *gr, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = t / iters;
    return check(err);
}

static int iter_loss_backward_impl(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                                   const SplatLossConfig *cfg, SplatIterWorkspace *ws, const SplatPoseAdam *adam, void *stream,
                                   const SplatAdamMap *map_adam = nullptr, int loss_mode = SPLAT_LOSS_SPLATAM) {
    if (!cam || !map || !frame || !cfg || !ws) return SPLAT_E_INVALID;
    if (loss_mode != SPLAT_LOSS_SPLATAM && loss_mode != SPLAT_LOSS_GS) return SPLAT_E_INVALID;
    // get_loss_gs: a mapping loss without pose gradient, outlier rejection or a deferred finish
    if (loss_mode == SPLAT_LOSS_GS && (cfg->tracking || cfg->camera_grad || !cfg->gaussians_grad || cfg->ignore_outlier_depth_loss || cfg->defer_finish || adam))
        return SPLAT_E_INVALID;
    if (map->P < 0 || cam->image_width <= 0 || cam->image_height <= 0 || !cam->viewmatrix || !cam->projmatrix) return SPLAT_E_INVALID;
    if (map->num_frames <= 0 || frame->time_idx < 0 || frame->time_idx >= map->num_frames) return SPLAT_E_INVALID;
    if (!map->cam_unnorm_rots || !map->cam_trans || !frame->im || !frame->depth || !frame->w2c) return SPLAT_E_INVALID;
    if (map->P > 0 && (!map->means3D || !map->rgb_colors || !map->unnorm_rotations || !map->logit_opacities || !map->log_scales))
        return SPLAT_E_INVALID;
    if (cfg->ignore_outlier_depth_loss && (!ws->outlier_err || !ws->outlier_scratch)) return SPLAT_E_INVALID;
    const SplatState &st = ws->st;
    if (!st.tile_count || !st.tile_base || !st.tile_cursor || !st.status || !st.final_T || !st.n_contrib) return SPLAT_E_INVALID;
    if (map->P > 0 && (!st.depth || !st.xy || !st.conic_opacity || !st.rect || !st.radii || !ws->feat8 || !ws->accum)) return SPLAT_E_INVALID;
    if (st.capacity <= 0 || !st.keys || !st.point_list || st.tile_stride < 0) return SPLAT_E_INVALID;
    if (st.tile_stride > 0 && (long long)st.tile_stride * (long long)splat_num_tiles(cam->image_width, cam->image_height) > st.capacity)
        return SPLAT_E_INVALID;
    if (!ws->out6 || !ws->dL_dout6 || !ws->sums || !ws->d_cam) return SPLAT_E_INVALID;
    if (!cfg->tracking && !ws->ssim_maps) return SPLAT_E_INVALID;
    if (st.tile_row_begin < 0 || st.tile_row_end < 0 || (st.tile_row_end > 0 && st.tile_row_end <= st.tile_row_begin) ||
        st.tile_row_end > (cam->image_height + SPLAT_TILE - 1) / SPLAT_TILE)
        return SPLAT_E_INVALID;
    if (st.tile_row_end > st.tile_row_begin && (!cfg->tracking || cfg->ignore_outlier_depth_loss || map_adam)) return SPLAT_E_INVALID;
    return check(launch_iter_loss_backward(*cam, *map, *frame, *cfg, *ws, (hipStream_t)stream, adam, map_adam, loss_mode));
}

int splat_iter_loss_backward(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                             const SplatLossConfig *cfg, SplatIterWorkspace *ws, void *stream) {
    return iter_loss_backward_impl(cam, map, frame, cfg, ws, nullptr, stream);
}

int splat_iter_tracking_step(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                             const SplatLossConfig *cfg, SplatIterWorkspace *ws, const SplatPoseAdam *adam, void *stream) {
    if (!cfg || !cfg->tracking || !cfg->camera_grad || !adam || !adam->state) return SPLAT_E_INVALID;
    return iter_loss_backward_impl(cam, map, frame, cfg, ws, adam, stream);
}

int splat_iter_finish(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatLossConfig *cfg,
                      SplatIterWorkspace *ws, const SplatPoseAdam *adam, void *stream) {
    if (!cam || !map || !frame || !cfg || !ws || !ws->sums || !ws->d_cam || !ws->st.status) return SPLAT_E_INVALID;
    if (!map->cam_unnorm_rots || !map->cam_trans || map->num_frames <= 0 || frame->time_idx < 0 || frame->time_idx >= map->num_frames)
        return SPLAT_E_INVALID;
    if (adam && !adam->state) return SPLAT_E_INVALID;
    return check(launch_iter_finish(*cam, *map, *frame, *cfg, *ws, (hipStream_t)stream, adam));
}

int splat_iter_fold_sums(double *sums, void *stream) {
    if (!sums) return SPLAT_E_INVALID;
    return check(launch_iter_fold_sums(sums, (hipStream_t)stream));
}

// splat_iter_mapping_step under either loss: ONE check for the old entry point and the extended one
static int mapping_step_impl(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatLossConfig *cfg,
                             SplatIterWorkspace *ws, const SplatAdamMap *adam, void *stream, int loss_mode) {
    if (!cfg || cfg->tracking || !cfg->gaussians_grad || !adam || !ws) return SPLAT_E_INVALID;
    // a stepped group (adam->grad[k] != NULL) takes the gradient this iteration forms in registers; adam->grad[k] names the buffer it is
    // ALSO written to -- or, when the workspace carries no buffer for the group (ws->d_* NULL), it is not stored at all (a loop that
    // discards its gradients after the step, as the reference's zero_grad(set_to_none=True) does: 48 bytes per Gaussian not written)
    const float *const grads[5] = {ws->d_means3D, ws->d_rgb_colors, ws->d_unnorm_rotations, ws->d_logit_opacities, ws->d_log_scales};
    for (int k = 0; k < 5; ++k)
        if (adam->grad[k] && ((grads[k] && adam->grad[k] != grads[k]) || !adam->exp_avg[k] || !adam->exp_avg_sq[k])) return SPLAT_E_INVALID;
    return iter_loss_backward_impl(cam, map, frame, cfg, ws, nullptr, stream, adam, loss_mode);
}

int splat_iter_mapping_step(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                            const SplatLossConfig *cfg, SplatIterWorkspace *ws, const SplatAdamMap *adam, void *stream) {
    return mapping_step_impl(cam, map, frame, cfg, ws, adam, stream, SPLAT_LOSS_SPLATAM);
}

static bool valid_config_ex(const SplatLossConfigEx *cfg) {
    return cfg && cfg->reserved[0] == 0 && cfg->reserved[1] == 0 && cfg->reserved[2] == 0;
}

int splat_iter_loss_backward_ex(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                                const SplatLossConfigEx *cfg, SplatIterWorkspace *ws, void *stream) {
    if (!valid_config_ex(cfg)) return SPLAT_E_INVALID;
    return iter_loss_backward_impl(cam, map, frame, &cfg->base, ws, nullptr, stream, nullptr, cfg->loss_mode);
}

int splat_iter_mapping_step_ex(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame,
                               const SplatLossConfigEx *cfg, SplatIterWorkspace *ws, const SplatAdamMap *adam, void *stream) {
    if (!valid_config_ex(cfg)) return SPLAT_E_INVALID;
    return mapping_step_impl(cam, map, frame, &cfg->base, ws, adam, stream, cfg->loss_mode);
}

int splat_iter_adam_map(const SplatMap *map, const SplatAdamMap *opt, void *stream) {
    if (!map || !opt || map->P < 0) return SPLAT_E_INVALID;
    for (int k = 0; k < 5; ++k)
        if (opt->grad[k] && (!opt->exp_avg[k] || !opt->exp_avg_sq[k])) return SPLAT_E_INVALID;
    return check(launch_iter_adam_map(*map, *opt, (hipStream_t)stream));
}

int splat_iter_adam_pose(const SplatMap *map, int32_t time_idx, const float *d_cam, float *state, float beta1, float beta2,
                         float eps, float bc2_sqrt, float step_size_rot, float step_size_trans, void *stream) {
    if (!map || !d_cam || !state || !map->cam_unnorm_rots || !map->cam_trans) return SPLAT_E_INVALID;
    if (time_idx < 0 || time_idx >= map->num_frames) return SPLAT_E_INVALID;
    return check(launch_iter_adam_pose(*map, time_idx, d_cam, state, beta1, beta2, eps, bc2_sqrt, step_size_rot, step_size_trans,
                                       (hipStream_t)stream));
}

int splat_iter_time_kernel(int fn, int iters, const SplatCamera *cam, int32_t P, SplatIterWorkspace *ws, void *stream, float *ms) {
    if (!ms || iters <= 0 || !cam || !ws || fn < 0 || fn > 4 || P < 0) return SPLAT_E_INVALID;
    if (!ws->feat8 || !ws->out6 || !ws->dL_dout6 || !ws->accum || !ws->st.tile_base || !ws->st.point_list) return SPLAT_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return SPLAT_E_LAUNCH;
    hipError_t err = hipSuccess;
    // bucketed lists: the iteration's last kernel consumed and reset the tile counters and left the counts in the cursor words
    SplatState st = ws->st;
    if (st.tile_stride > 0) st.tile_count = st.tile_cursor;
    // the backward composite ALONE (fn 1, 4): the records in tile_recs belong to whatever forward composite ran last on this state
    // (the one-kernel tracking form writes none for a list's last batch): it gathers.  fn 3 alternates with the forward composite,
    // which writes them: the product's pair
    if (fn == 1 || fn == 4) st.tile_recs = nullptr;
    // fn 2: the forward composite in the form the iteration launches when the lists are short -- it filters its group's records (or
    // reads its bucket), sorts and publishes the tile's list itself.  The iteration's last kernel left the groups' record counts in
    // word 1 of their counter lines (group_kept: the live counters are set from them for the timed launches and zeroed again) and the
    // tiles' counts in the cursor words; the re-published lists and counts are the same values
    bool sort_form = false;
    int live_groups = 0;
    // fn 3: forward and backward composite ALTERNATING, as the iteration issues them (the forward one in its sorting form when the
    // state allows it): time(fn 3) - time(fn 2 or 0) is the backward composite between other kernels -- 30 launches of it in a row
    // read ~10 % longer than rocprofv3's per-kernel average of the loop
    const bool can_sort = st.tile_stride > 0 && lists_sorted_by_composite(st);
    if (fn == 2 || (fn == 3 && can_sort)) {
        if (!can_sort) return SPLAT_E_INVALID;
        sort_form = true;
        if (st.group_stride > 0 && st.group_count && st.group_recs) live_groups = tile_groups(cam->image_width, cam->image_height);
        else st.group_stride = 0;
    } else {
        st.group_stride = 0;
    }
    if (live_groups) err = launch_group_counters_restore(st, live_groups, true, s);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters && err == hipSuccess; ++i) {
        if (fn != 1 && fn != 4) err = launch_render_forward_feat8(*cam, ws->feat8, st, ws->out6, sort_form, s);
        if ((fn == 1 || fn == 3) && err == hipSuccess) err = launch_render_backward_feat8(*cam, ws->feat8, st, ws->dL_dout6, ws->accum, P, false, IterSums::MapRgb, s);
        if (fn == 4) err = launch_render_backward_feat8(*cam, ws->feat8, st, ws->dL_dout6, ws->accum, P, false, IterSums::Track, s);
    }
    (void)hipEventRecord(e1, s);
    if (live_groups) {                          // (whatever the launches returned: the next iteration's per-Gaussian kernel starts from zero)
        const hipError_t e = launch_group_counters_restore(st, live_groups, false, s);
        if (err == hipSuccess) err = e;
    }
    // the timed backward launches accumulated into ws->accum: restore the workspace invariant (every iteration leaves the
    // accumulator zeroed; fused_backward_kernel relies on it) outside the timed bracket
    if ((fn == 1 || fn == 3 || fn == 4) && err == hipSuccess && P > 0) err = hipMemsetAsync(ws->accum, 0, sizeof(float) * SPLAT_GRAD_STRIDE * (size_t)P, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = t / iters;
    return check(err);
}

static bool valid_iter_common(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatIterWorkspace *ws) {
    if (!cam || !map || !frame || !ws) return false;
    if (map->P < 0 || cam->image_width <= 0 || cam->image_height <= 0 || !cam->viewmatrix || !cam->projmatrix) return false;
    if (map->num_frames <= 0 || frame->time_idx < 0 || frame->time_idx >= map->num_frames) return false;
    if (!map->cam_unnorm_rots || !map->cam_trans || !frame->w2c) return false;
    if (map->P > 0 && (!map->means3D || !map->rgb_colors || !map->unnorm_rotations || !map->logit_opacities || !map->log_scales))
        return false;
    const SplatState &st = ws->st;
    if (!st.tile_count || !st.tile_base || !st.tile_cursor || !st.status || !st.final_T || !st.n_contrib) return false;
    if (map->P > 0 && (!st.depth || !st.xy || !st.conic_opacity || !st.rect || !st.radii || !ws->feat8)) return false;
    if (st.capacity <= 0 || !st.keys || !st.point_list || st.tile_stride < 0) return false;
    if (st.tile_stride > 0 && (long long)st.tile_stride * (long long)splat_num_tiles(cam->image_width, cam->image_height) > st.capacity)
        return false;
    return ws->out6 != nullptr;
}

int splat_iter_render(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, SplatIterWorkspace *ws, void *stream) {
    if (!valid_iter_common(cam, map, frame, ws)) return SPLAT_E_INVALID;
    return check(launch_iter_render(*cam, *map, *frame, *ws, (hipStream_t)stream));
}

static bool valid_eval(int32_t width, int32_t height, const SplatEvalConfig *cfg, const SplatEvalWorkspace *ews, const double *out_row) {
    if (width <= 0 || height <= 0 || (long long)width * height > 0x3fffffffLL || !cfg || !ews || !ews->sums || !out_row) return false;
    // (pytorch_msssim asserts the same: four poolings must leave room for the 11-tap window)
    if (cfg->ms_ssim && ((width < height ? width : height) <= 160 || !ews->pyramid)) return false;
    return true;
}

int splat_eval_metrics(int32_t width, int32_t height, const float *rgb, const float *depth, const float *silhouette, const float *gt_im,
                       const float *gt_depth, const SplatEvalConfig *cfg, const SplatEvalWorkspace *ews, double *out_row, void *stream) {
    if (!valid_eval(width, height, cfg, ews, out_row) || !rgb || !depth || !gt_im || !gt_depth || ((cfg->sil_mask || cfg->holes) && !silhouette)) return SPLAT_E_INVALID;
    return check(launch_eval_metrics(width, height, rgb, depth, silhouette, gt_im, gt_depth, *cfg, *ews, nullptr, out_row, (hipStream_t)stream));
}

int splat_iter_eval(const SplatCamera *cam, const SplatMap *map, const SplatFrameData *frame, const SplatEvalConfig *cfg,
                    SplatIterWorkspace *ws, const SplatEvalWorkspace *ews, double *out_row, void *stream) {
    if (!valid_iter_common(cam, map, frame, ws) || !frame->im || !frame->depth) return SPLAT_E_INVALID;
    if (!valid_eval(cam->image_width, cam->image_height, cfg, ews, out_row)) return SPLAT_E_INVALID;
    const hipError_t e = launch_iter_render(*cam, *map, *frame, *ws, (hipStream_t)stream);
    if (e != hipSuccess) return SPLAT_E_LAUNCH;
    const size_t HW = (size_t)cam->image_width * (size_t)cam->image_height;
    return check(launch_eval_metrics(cam->image_width, cam->image_height, ws->out6, ws->out6 + 3 * HW, ws->out6 + 4 * HW, frame->im, frame->depth,
                                     *cfg, *ews, ws->st.status, out_row, (hipStream_t)stream));
}

// what the three frame entries share: positive sizes of at most 0x3fffffff pixels each, a positive scale, no NULL pointer
static bool valid_frame_args(int32_t color_w, int32_t color_h, int32_t depth_w, int32_t depth_h, int32_t dst_w, int32_t dst_h, double scale,
                             const void *color, const void *depth, const void *color_out, const void *depth_out) {
    return color_w > 0 && color_h > 0 && depth_w > 0 && depth_h > 0 && dst_w > 0 && dst_h > 0 && (long long)color_w * color_h <= 0x3fffffffLL
        && (long long)depth_w * depth_h <= 0x3fffffffLL && (long long)dst_w * dst_h <= 0x3fffffffLL && scale > 0.0
        && color && depth && color_out && depth_out;
}

int splat_frame_prepare(int32_t src_w, int32_t src_h, const float *color_hwc, const float *depth_hw, int32_t dst_w, int32_t dst_h,
                        float *im_out, float *depth_out, void *stream) {
    if (!valid_frame_args(src_w, src_h, src_w, src_h, dst_w, dst_h, 1.0, color_hwc, depth_hw, im_out, depth_out)) return SPLAT_E_INVALID;
    return check(launch_frame_prepare(src_w, src_h, color_hwc, depth_hw, dst_w, dst_h, im_out, depth_out, (hipStream_t)stream));
}

int splat_frame_ingest(int32_t color_w, int32_t color_h, const uint8_t *rgb_hwc, int32_t depth_w, int32_t depth_h, const uint16_t *depth_raw,
                       double png_depth_scale, int32_t dst_w, int32_t dst_h, float *color_out_hwc, float *depth_out, void *stream) {
    if (!valid_frame_args(color_w, color_h, depth_w, depth_h, dst_w, dst_h, png_depth_scale, rgb_hwc, depth_raw, color_out_hwc, depth_out))
        return SPLAT_E_INVALID;
    return check(launch_frame_ingest(color_w, color_h, rgb_hwc, depth_w, depth_h, depth_raw, png_depth_scale, dst_w, dst_h, color_out_hwc,
                                     depth_out, (hipStream_t)stream));
}

int splat_frame_ingest_planes(int32_t color_w, int32_t color_h, const uint8_t *rgb_hwc, int32_t depth_w, int32_t depth_h, const void *depth_raw,
                              int32_t depth_type, double depth_scale, int32_t dst_w, int32_t dst_h, float *im_out, float *depth_out, void *stream) {
    if (!valid_frame_args(color_w, color_h, depth_w, depth_h, dst_w, dst_h, depth_scale, rgb_hwc, depth_raw, im_out, depth_out)
        || (depth_type != SPLAT_DEPTH_U16 && depth_type != SPLAT_DEPTH_F32) || (depth_type == SPLAT_DEPTH_F32 && depth_scale != 1.0))
        return SPLAT_E_INVALID;
    return check(launch_frame_ingest_planes(color_w, color_h, rgb_hwc, depth_w, depth_h, depth_raw, depth_type == SPLAT_DEPTH_F32, depth_scale,
                                            dst_w, dst_h, im_out, depth_out, (hipStream_t)stream));
}

int splat_view_camera(const SplatViewArgs *v, void *stream) {
    if (!v || v->width <= 0 || v->height <= 0 || !v->w2c || !v->viewmatrix || !v->projmatrix || !v->campos) return SPLAT_E_INVALID;
    if (!(v->fx > 0.0) || !(v->fy > 0.0) || !(v->far_z > v->near_z)) return SPLAT_E_INVALID;
    if (!v->w2c_in && (!v->cam_unnorm_rots || !v->cam_trans || !v->first_w2c || v->num_frames <= 0 || v->time_idx < 0 || v->time_idx >= v->num_frames))
        return SPLAT_E_INVALID;
    return check(launch_view_camera(*v, (hipStream_t)stream));
}

int splat_view_finish(const SplatViewArgs *v, void *stream) {
    if (!v || v->width <= 0 || v->height <= 0 || (long long)v->width * v->height > 0x3fffffffLL || !v->out6) return SPLAT_E_INVALID;
    if (v->mode != SPLAT_VIEW_COLOR && v->mode != SPLAT_VIEW_DEPTH && v->mode != SPLAT_VIEW_SILHOUETTE) return SPLAT_E_INVALID;
    if (v->rgb8 && v->mode == SPLAT_VIEW_DEPTH && !v->lut) return SPLAT_E_INVALID;
    if (v->points && (!v->w2c || !(v->fx > 0.0) || !(v->fy > 0.0))) return SPLAT_E_INVALID;
    if (!v->rgb8 && !v->points && !v->colors) return SPLAT_OK;
    return check(launch_view_finish(*v, (hipStream_t)stream));
}

// the view overlay (csrc/viewoverlay.hip)
static bool valid_overlay(const SplatViewOverlay *v) {
    return v && v->width > 0 && v->height > 0 && (long long)v->width * v->height <= 0x3fffffffLL && v->keys;
}
// ... as a camera to draw through: positive finite focal lengths and near plane, finite centre
static bool valid_overlay_camera(const SplatViewOverlay *v) {
    return valid_overlay(v) && v->w2c && v->fx > 0.f && v->fy > 0.f && v->near_z > 0.f && v->fx - v->fx == 0.f && v->fy - v->fy == 0.f
           && v->cx - v->cx == 0.f && v->cy - v->cy == 0.f && v->near_z - v->near_z == 0.f;
}

int splat_view_run_segments(const SplatViewRun *r, void *stream) {
    if (!r || r->num_frames <= 0 || r->first < 0 || r->count < 0 || r->count > r->num_frames - r->first || !r->segments || !r->colors)
        return SPLAT_E_INVALID;
    if (!r->w2c_all && (!r->cam_unnorm_rots || !r->cam_trans || !r->first_w2c)) return SPLAT_E_INVALID;
    if (r->frusta && (r->width <= 0 || r->height <= 0 || !(r->fx > 0.0) || !(r->fy > 0.0) || !(r->scale > 0.0))) return SPLAT_E_INVALID;
    if (r->num_frames > 0x7fffffff / (SPLAT_VIEW_FRUSTUM_SEGMENTS + 1)) return SPLAT_E_INVALID;
    return check(launch_view_run_segments(*r, (hipStream_t)stream));
}

int splat_view_overlay_clear(const SplatViewOverlay *v, void *stream) {
    if (!valid_overlay(v)) return SPLAT_E_INVALID;
    return check(launch_view_overlay_clear(*v, (hipStream_t)stream));
}

int splat_view_points(const SplatViewOverlay *v, const float *means3D, int32_t count, int32_t point_size, void *stream) {
    if (!valid_overlay_camera(v) || count < 0 || (count > 0 && !means3D) || point_size < 1 || point_size > SPLAT_VIEW_MAX_POINT_SIZE)
        return SPLAT_E_INVALID;
    return check(launch_view_points(*v, means3D, count, point_size, (hipStream_t)stream));
}

int splat_view_segments(const SplatViewOverlay *v, const float *segments, int32_t first, int32_t count, int32_t line_width, void *stream) {
    if (!valid_overlay_camera(v) || first < 0 || count < 0 || count > 0x7fffffff - first || (count > 0 && !segments) || line_width < 1
        || line_width > SPLAT_VIEW_MAX_LINE_WIDTH)
        return SPLAT_E_INVALID;
    return check(launch_view_segments(*v, segments, first, count, line_width, (hipStream_t)stream));
}

int splat_view_overlay_finish(const SplatViewOverlay *v, const SplatViewOverlayFinish *f, void *stream) {
    if (!valid_overlay(v) || !f || !f->rgb8 || f->num_rows < 0 || f->num_segments < 0 || (f->num_rows > 0 && !f->rgb_colors)
        || (f->num_segments > 0 && !f->segment_colors))
        return SPLAT_E_INVALID;
    return check(launch_view_overlay_finish(*v, *f, (hipStream_t)stream));
}

// the mesh layer (csrc/tsdf.hip)
// the grid of either volume struct: positive dims, voxel and trunc, fewer than 2^40 grid points (tsdf_math.h kTsdfMaxPoints)
static bool valid_tsdf_dims(int nx, int ny, int nz, float voxel, float trunc) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || !(voxel > 0.f) || !(trunc > 0.f)) return false;
    return (long long)nx * ny < kTsdfMaxPoints && (long long)nx * ny * (long long)nz < kTsdfMaxPoints;
}
static bool valid_tsdf_grid(const SplatTsdfVolume *v) { return v && valid_tsdf_dims(v->nx, v->ny, v->nz, v->voxel, v->trunc); }
static bool valid_tsdf_volume(const SplatTsdfVolume *v) {
    return valid_tsdf_grid(v) && v->tsdf && v->weight && v->r && v->g && v->b;
}
static bool valid_tsdf_view(const SplatTsdfView *w) {
    if (!w || w->width <= 0 || w->height <= 0 || (long long)w->width * w->height > 0x3fffffffLL) return false;
    return w->out6 && w->w2c && !(w->skip && !w->skipped);
}
// room for `capacity` triangles' keys (none needed at capacity 0) and somewhere to put the count
static bool valid_tsdf_keys(const int64_t *keys, int64_t capacity, const int64_t *count) { return capacity >= 0 && (capacity == 0 || keys) && count; }

size_t splat_tsdf_bytes(const SplatTsdfVolume *v) {
    return valid_tsdf_grid(v) ? 5 * sizeof(float) * (size_t)v->nx * (size_t)v->ny * (size_t)v->nz : 0;
}

int splat_tsdf_reset(const SplatTsdfVolume *v, void *stream) {
    if (!valid_tsdf_volume(v)) return SPLAT_E_INVALID;
    return check(launch_tsdf_reset(*v, (hipStream_t)stream));
}

int splat_tsdf_integrate(const SplatTsdfVolume *v, const SplatTsdfView *w, void *stream) {
    if (!valid_tsdf_volume(v) || !valid_tsdf_view(w)) return SPLAT_E_INVALID;
    return check(launch_tsdf_integrate(*v, *w, (hipStream_t)stream));
}

int splat_tsdf_triangles(const SplatTsdfVolume *v, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream) {
    if (!valid_tsdf_volume(v) || !valid_tsdf_keys(keys, capacity, count)) return SPLAT_E_INVALID;
    return check(launch_tsdf_triangles(*v, min_weight, keys, (long long)capacity, count, false, (hipStream_t)stream));
}

int splat_tsdf_cubes(const SplatTsdfVolume *v, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream) {
    if (!valid_tsdf_volume(v) || !valid_tsdf_keys(keys, capacity, count)) return SPLAT_E_INVALID;
    return check(launch_tsdf_triangles(*v, min_weight, keys, (long long)capacity, count, true, (hipStream_t)stream));
}

int splat_tsdf_cubes_table(int8_t *out) {
    if (!out) return SPLAT_E_INVALID;
    memcpy(out, kTsdfCubesCases, sizeof(kTsdfCubesCases));
    return SPLAT_OK;
}

int splat_tsdf_vertices(const SplatTsdfVolume *v, const int64_t *keys, int64_t n, float *vertices, float *colors, void *stream) {
    if (!valid_tsdf_volume(v) || n < 0 || (n > 0 && (!keys || !vertices))) return SPLAT_E_INVALID;
    return check(launch_tsdf_vertices(*v, keys, (long long)n, vertices, colors, (hipStream_t)stream));
}

// the mesh layer on a sparse volume (csrc/tsdf_sparse.hip)
static const int32_t kSparseBrickShapes[2][3] = {{16, 16, 8}, {64, 4, 8}};     // (the first is the default: profiles/mesh_sparse.md 1)

int splat_tsdf_sparse_brick_shape(int index, int32_t *shape) {
    if (shape && index >= 0 && index < 2)
        for (int a = 0; a < 3; ++a) shape[a] = kSparseBrickShapes[index][a];
    return 2;
}

static long long sparse_bricks(const SplatTsdfSparse *v) {
    return (long long)((v->nx + v->brick[0] - 1) / v->brick[0]) * ((v->ny + v->brick[1] - 1) / v->brick[1]) * ((v->nz + v->brick[2] - 1) / v->brick[2]);
}
static bool valid_sparse_grid(const SplatTsdfSparse *v) {
    if (!v || !valid_tsdf_dims(v->nx, v->ny, v->nz, v->voxel, v->trunc) || v->slots < 0) return false;
    bool listed = false;
    for (int n = 0; n < 2; ++n)
        listed |= v->brick[0] == kSparseBrickShapes[n][0] && v->brick[1] == kSparseBrickShapes[n][1] && v->brick[2] == kSparseBrickShapes[n][2];
    return listed && sparse_bricks(v) < (1ll << 31);
}
static bool valid_sparse_volume(const SplatTsdfSparse *v) {
    return valid_sparse_grid(v) && v->directory && (v->slots == 0 || (v->brick_of_slot && v->tsdf && v->weight && v->r && v->g && v->b));
}

size_t splat_tsdf_sparse_bytes(const SplatTsdfSparse *v) {
    if (!valid_sparse_grid(v)) return 0;
    return (5 * sizeof(float) * 2048 + sizeof(int32_t)) * (size_t)v->slots + sizeof(int32_t) * (size_t)sparse_bricks(v);
}

int splat_tsdf_sparse_mark(const SplatTsdfSparse *v, const SplatTsdfView *w, int32_t *flags, void *stream) {
    if (!valid_sparse_grid(v) || !valid_tsdf_view(w) || !flags) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_mark(*v, *w, flags, (hipStream_t)stream));
}

int splat_tsdf_sparse_reset_slots(const SplatTsdfSparse *v, int64_t first, int64_t count, void *stream) {
    if (!valid_sparse_volume(v) || first < 0 || count < 0 || first + count > v->slots) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_reset_slots(*v, (long long)first, (long long)count, (hipStream_t)stream));
}

int splat_tsdf_sparse_integrate(const SplatTsdfSparse *v, const SplatTsdfView *w, void *stream) {
    if (!valid_sparse_volume(v) || !valid_tsdf_view(w)) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_integrate(*v, *w, (hipStream_t)stream));
}

int splat_tsdf_sparse_triangles(const SplatTsdfSparse *v, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream) {
    if (!valid_sparse_volume(v) || !valid_tsdf_keys(keys, capacity, count)) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_triangles(*v, min_weight, keys, (long long)capacity, count, false, (hipStream_t)stream));
}

int splat_tsdf_sparse_cubes(const SplatTsdfSparse *v, float min_weight, int64_t *keys, int64_t capacity, int64_t *count, void *stream) {
    if (!valid_sparse_volume(v) || !valid_tsdf_keys(keys, capacity, count)) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_triangles(*v, min_weight, keys, (long long)capacity, count, true, (hipStream_t)stream));
}

int splat_tsdf_sparse_vertices(const SplatTsdfSparse *v, const int64_t *keys, int64_t n, float *vertices, float *colors, void *stream) {
    if (!valid_sparse_volume(v) || n < 0 || (n > 0 && (!keys || !vertices))) return SPLAT_E_INVALID;
    return check(launch_tsdf_sparse_vertices(*v, keys, (long long)n, vertices, colors, (hipStream_t)stream));
}

// the mesh score layer (csrc/meshscore.hip)
static bool valid_nn_grid(const SplatNnGrid *g) {
    if (!g || g->count < 0) return false;
    if (!(g->cell > 0.f) || !(g->cell <= 3.0e38f) || g->dims[0] <= 0 || g->dims[1] <= 0 || g->dims[2] <= 0) return false;
    for (int k = 0; k < 3; ++k)
        if (!(g->lo[k] >= -3.0e38f && g->lo[k] <= 3.0e38f)) return false;
    return (long long)g->dims[0] * g->dims[1] <= SPLAT_NN_MAX_CELLS && (long long)g->dims[0] * g->dims[1] * (long long)g->dims[2] <= SPLAT_NN_MAX_CELLS;
}

// the rule of every entry point that takes a mesh: counts that are not negative, and an array wherever its count is positive
static bool valid_mesh_arrays(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces) {
    return num_vertices >= 0 && num_faces >= 0 && (num_faces == 0 || faces) && (num_vertices == 0 || vertices);
}

int splat_mesh_areas(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, double *area, void *stream) {
    if (!valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || (num_faces > 0 && !area)) return SPLAT_E_INVALID;
    return check(launch_mesh_areas(vertices, num_vertices, faces, num_faces, area, (hipStream_t)stream));
}

int splat_mesh_sample(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const double *prefix, uint64_t seed,
                      int64_t n, float *points, int32_t *face, void *stream) {
    if (!valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || n < 0 || (num_faces > 0 && !prefix)) return SPLAT_E_INVALID;
    if (n > 0 && (!points || !face)) return SPLAT_E_INVALID;
    return check(launch_mesh_sample(vertices, num_vertices, faces, num_faces, prefix, seed, (long long)n, points, face, (hipStream_t)stream));
}

int splat_nn_cell_keys(const SplatNnGrid *grid, const float *points, int64_t n, int32_t *key, void *stream) {
    if (!valid_nn_grid(grid) || n < 0 || (n > 0 && (!points || !key))) return SPLAT_E_INVALID;
    return check(launch_nn_cell_keys(*grid, points, (long long)n, key, (hipStream_t)stream));
}

int splat_nn_cell_starts(const SplatNnGrid *grid, const int32_t *sorted_key, const int32_t *order, const float *points, float *records,
                         int32_t *start, void *stream) {
    if (!valid_nn_grid(grid) || !start) return SPLAT_E_INVALID;
    if (grid->count > 0 && (!sorted_key || !order || !points || !records || ((uintptr_t)records & 15) != 0)) return SPLAT_E_INVALID;
    return check(launch_nn_cell_starts(*grid, sorted_key, order, points, records, start, (hipStream_t)stream));
}

int splat_nn_query(const SplatNnGrid *grid, const float *points, const int32_t *order, int64_t n, float *dist2, int32_t *index, int32_t *account,
                   void *stream) {
    if (!valid_nn_grid(grid) || !grid->start || (grid->count > 0 && (!grid->records || ((uintptr_t)grid->records & 15) != 0))) return SPLAT_E_INVALID;
    if (n < 0 || (n > 0 && (!points || !dist2 || !index))) return SPLAT_E_INVALID;
    return check(launch_nn_query(*grid, points, order, (long long)n, dist2, index, account, (hipStream_t)stream));
}

int splat_nn_reduce(const float *dist2, int64_t n, double threshold, double *partials, double *row, void *stream) {
    if (n < 0 || (n > 0 && !dist2) || !partials || !row) return SPLAT_E_INVALID;
    return check(launch_nn_reduce(dist2, (long long)n, threshold, partials, row, (hipStream_t)stream));
}

// the ICP layer (csrc/icp.hip)
int splat_icp_transform(const float *source, int64_t n, const double *state, float *moved, void *stream) {
    if (n < 0 || !state || (n > 0 && (!source || !moved))) return SPLAT_E_INVALID;
    return check(launch_icp_transform(source, (long long)n, state, moved, (hipStream_t)stream));
}

int splat_icp_accumulate(const float *source, const float *targets, int64_t num_targets, const float *dist2, const int32_t *index, int64_t n,
                         double threshold, const double *origin, const double *state, double *partials, void *stream) {
    if (n < 0 || num_targets < 0 || !origin || !state || !partials || !(threshold == threshold)) return SPLAT_E_INVALID;
    if (n > 0 && (!source || !dist2 || !index || (num_targets > 0 && !targets))) return SPLAT_E_INVALID;
    return check(launch_icp_accumulate(source, targets, (long long)num_targets, dist2, index, (long long)n, threshold, origin, state, partials,
                                       (hipStream_t)stream));
}

int splat_icp_solve(const double *partials, int64_t n, int32_t max_iterations, double relative_fitness, double relative_rmse,
                    const double *origin, double *state, double *history, void *stream) {
    if (n < 0 || max_iterations < 0 || !partials || !origin || !state || !history) return SPLAT_E_INVALID;
    if (!(relative_fitness == relative_fitness) || !(relative_rmse == relative_rmse)) return SPLAT_E_INVALID;
    return check(launch_icp_solve(partials, (long long)n, max_iterations, relative_fitness, relative_rmse, origin, state, history,
                                  (hipStream_t)stream));
}

// the mesh cleaning layer (csrc/meshclean.hip)
int splat_mesh_components(const int32_t *faces, int32_t num_faces, int32_t num_vertices, int32_t *labels, void *stream) {
    if (num_vertices < 0 || num_faces < 0 || (num_faces > 0 && !faces) || (num_vertices > 0 && !labels)) return SPLAT_E_INVALID;
    return check(launch_mesh_components(faces, num_faces, num_vertices, labels, (hipStream_t)stream));
}

int splat_mesh_component_stats(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const int32_t *labels,
                               int32_t *num_v, int32_t *num_f, int64_t *area_q, int32_t *lo, int32_t *hi, void *stream) {
    if (!valid_mesh_arrays(vertices, num_vertices, faces, num_faces)) return SPLAT_E_INVALID;
    if (num_vertices > 0 && (!labels || !num_v || !num_f || !area_q || !lo || !hi)) return SPLAT_E_INVALID;
    return check(launch_mesh_component_stats(vertices, num_vertices, faces, num_faces, labels, num_v, num_f, area_q, lo, hi, (hipStream_t)stream));
}

// the mesh simplification layer (csrc/meshsimplify.hip)
static bool valid_cell(double cell) { return cell > 0.0 && cell <= 1.7e308; }

int splat_mesh_simplify_keys(const float *vertices, int32_t num_vertices, double cell, int64_t *keys, void *stream) {
    if (num_vertices < 0 || !valid_cell(cell) || (num_vertices > 0 && (!vertices || !keys))) return SPLAT_E_INVALID;
    return check(launch_mesh_simplify_keys(vertices, num_vertices, cell, keys, (hipStream_t)stream));
}

int splat_mesh_simplify_vertices(const float *vertices, const float *colors, int32_t num_vertices, const int32_t *cluster, double cell,
                                 int32_t *count, int64_t *sums, void *stream) {
    if (num_vertices < 0 || !valid_cell(cell) || (num_vertices > 0 && (!vertices || !cluster || !count || !sums))) return SPLAT_E_INVALID;
    return check(launch_mesh_simplify_vertices(vertices, colors, num_vertices, cluster, cell, count, sums, (hipStream_t)stream));
}

int splat_mesh_simplify_quadrics(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const int32_t *cluster,
                                 double cell, int64_t *sums, int32_t *refused, void *stream) {
    if (!valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || !valid_cell(cell)) return SPLAT_E_INVALID;
    if (num_vertices > 0 && num_faces > 0 && (!cluster || !sums || !refused)) return SPLAT_E_INVALID;
    return check(launch_mesh_simplify_quadrics(vertices, num_vertices, faces, num_faces, cluster, cell, sums, refused, (hipStream_t)stream));
}

int splat_mesh_simplify_place(const int32_t *count, const int64_t *sums, const int64_t *cell_keys, int32_t num_clusters, double cell,
                              int32_t placement, float *positions, float *colors, int32_t *rank, int32_t *fallback, double *value, void *stream) {
    if (num_clusters < 0 || !valid_cell(cell) || (placement != SPLAT_MESH_SIMPLIFY_MEAN && placement != SPLAT_MESH_SIMPLIFY_QUADRIC))
        return SPLAT_E_INVALID;
    if (num_clusters > 0 && (!count || !sums || !cell_keys || !positions || !rank || !fallback || !value)) return SPLAT_E_INVALID;
    return check(launch_mesh_simplify_place(count, sums, cell_keys, num_clusters, cell, placement == SPLAT_MESH_SIMPLIFY_QUADRIC, positions, colors,
                                            rank, fallback, value, (hipStream_t)stream));
}

int splat_mesh_simplify_faces(const int32_t *faces, int32_t num_faces, int32_t num_vertices, const int32_t *cluster, int32_t *triples,
                              void *stream) {
    if (num_faces < 0 || num_vertices < 0 || (num_faces > 0 && (!faces || !triples)) || (num_faces > 0 && num_vertices > 0 && !cluster))
        return SPLAT_E_INVALID;
    return check(launch_mesh_simplify_faces(faces, num_faces, num_vertices, cluster, triples, (hipStream_t)stream));
}

// the mesh render layer (csrc/meshrender.hip)
static bool finite_f(float x) { return x >= -3.0e38f && x <= 3.0e38f; }
static bool valid_mesh_view(const SplatMeshView *v) {
    if (!v || v->width <= 0 || v->height <= 0 || (long long)v->width * v->height > 0x3fffffffLL) return false;
    return finite_f(v->fx) && finite_f(v->fy) && v->fx != 0.f && v->fy != 0.f && finite_f(v->cx) && finite_f(v->cy);
}
// a view to render through: a valid view with a pose and a positive finite near plane
static bool valid_mesh_camera(const SplatMeshView *v) { return valid_mesh_view(v) && v->w2c && v->near_z > 0.f && finite_f(v->near_z); }

int splat_mesh_depth(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const SplatMeshView *view, float *depth,
                     void *stream) {
    if (!valid_mesh_camera(view) || !valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || !depth) return SPLAT_E_INVALID;
    return check(launch_mesh_depth(vertices, num_vertices, faces, num_faces, *view, depth, (hipStream_t)stream));
}

int splat_mesh_seen(const float *vertices, int32_t num_vertices, const SplatMeshView *view, const float *w2c, int32_t n, int32_t edge,
                    const float *depth, float eps, int32_t *seen, void *stream) {
    if (!valid_mesh_view(view) || num_vertices < 0 || n < 0 || edge < 0 || !(eps >= 0.f)) return SPLAT_E_INVALID;
    if ((num_vertices > 0 && (!vertices || !seen)) || (n > 0 && !w2c)) return SPLAT_E_INVALID;
    return check(launch_mesh_seen(vertices, num_vertices, *view, w2c, n, edge, depth, eps, seen, (hipStream_t)stream));
}

int splat_mesh_depth_compare(const float *a, const float *b, int64_t n, double *partials, double *row, void *stream) {
    if (n < 0 || (n > 0 && (!a || !b)) || !partials || !row) return SPLAT_E_INVALID;
    return check(launch_mesh_depth_compare(a, b, (long long)n, partials, row, (hipStream_t)stream));
}

// the mesh shade layer (csrc/meshshade.hip)
int splat_mesh_vertex_normals(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, int64_t *accum, float *normals,
                              void *stream) {
    if (!valid_mesh_arrays(vertices, num_vertices, faces, num_faces)) return SPLAT_E_INVALID;
    if (num_vertices > 0 && (!accum || !normals)) return SPLAT_E_INVALID;
    return check(launch_mesh_vertex_normals(vertices, num_vertices, faces, num_faces, accum, normals, (hipStream_t)stream));
}

int splat_mesh_visibility(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const SplatMeshView *view,
                          uint64_t *keys, void *stream) {
    if (!valid_mesh_camera(view) || !valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || !keys) return SPLAT_E_INVALID;
    return check(launch_mesh_visibility(vertices, num_vertices, faces, num_faces, *view, keys, (hipStream_t)stream));
}

int splat_mesh_shade(const float *vertices, int32_t num_vertices, const int32_t *faces, int32_t num_faces, const float *colors, const float *normals,
                     const SplatMeshView *view, const uint64_t *keys, const SplatMeshShade *args, uint8_t *rgb8, float *depth, int32_t *face,
                     float *normal, void *stream) {
    if (!valid_mesh_camera(view) || !valid_mesh_arrays(vertices, num_vertices, faces, num_faces) || !keys || !args || !rgb8) return SPLAT_E_INVALID;
    if (args->samples < 1 || args->samples > 4 || view->width % args->samples != 0 || view->height % args->samples != 0) return SPLAT_E_INVALID;
    if (args->mode < SPLAT_MESH_SHADE_COLOR || args->mode > SPLAT_MESH_SHADE_DEPTH) return SPLAT_E_INVALID;
    if (args->mode == SPLAT_MESH_SHADE_DEPTH && !args->lut) return SPLAT_E_INVALID;
    if (args->samples > 1 && (depth || face || normal)) return SPLAT_E_INVALID;
    return check(launch_mesh_shade(vertices, num_vertices, faces, num_faces, colors, normals, *view, keys, *args, rgb8, depth, face, normal,
                                   (hipStream_t)stream));
}

size_t splat_map_scratch_words(int64_t n) { return map_scratch_words(n < 0 ? 0 : n); }

static bool valid_store(const SplatMapStore *st) {
    if (!st || !st->counts || st->capacity < 0 || st->map.P < 0 || st->map.P > st->capacity) return false;
    const SplatMap &m = st->map;
    if (st->capacity > 0 && (!m.means3D || !m.rgb_colors || !m.unnorm_rotations || !m.logit_opacities || !m.log_scales)) return false;
    for (int k = 0; k < 5; ++k)
        if ((st->exp_avg[k] == nullptr) != (st->exp_avg_sq[k] == nullptr)) return false;
    return true;
}

int32_t splat_map_row_floats(const SplatMapStore *store) {
    if (!store) return 0;
    return map_row_floats(*store);
}

int splat_map_add_new_gaussians(SplatMapStore *store, const SplatAddArgs *a, void *stream) {
    if (!valid_store(store) || !a) return SPLAT_E_INVALID;
    if (a->width < 0 || a->height < 0 || (long long)a->width * a->height > 0x7fffffffLL) return SPLAT_E_INVALID;
    if (a->mode != SPLAT_ADD_VALID_DEPTH && a->mode != SPLAT_ADD_NON_PRESENCE) return SPLAT_E_INVALID;
    if (!a->scratch || !a->im || !a->depth || a->fx == 0.f || a->fy == 0.f) return SPLAT_E_INVALID;
    if (a->mode == SPLAT_ADD_NON_PRESENCE) {
        if (!a->out6 || !a->err || !store->map.cam_unnorm_rots || !store->map.cam_trans) return SPLAT_E_INVALID;
        if (a->time_idx < 0 || a->time_idx >= store->map.num_frames) return SPLAT_E_INVALID;
    } else if (!a->w2c) {
        return SPLAT_E_INVALID;
    }
    return check(launch_map_add(*store, *a, (hipStream_t)stream));
}

int splat_map_prune(SplatMapStore *store, const SplatPruneArgs *a, void *stream) {
    if (!valid_store(store) || !a || !a->scratch) return SPLAT_E_INVALID;
    if (store->map.P > 0 && (!a->flags || !a->stage)) return SPLAT_E_INVALID;
    return check(launch_map_prune(*store, *a, (hipStream_t)stream));
}

int splat_iter_means2d_accumulate(const SplatCamera *cam, const SplatMap *map, SplatIterWorkspace *ws, float *gaccum, float *denom,
                                  float *means2D_grad, void *stream) {
    if (!cam || !map || !ws || map->P < 0 || cam->image_width <= 0 || cam->image_height <= 0) return SPLAT_E_INVALID;
    if (map->P > 0 && ((!gaccum != !denom) || (!gaccum && !means2D_grad) || !ws->accum || !ws->feat8 || !ws->dL_dout6 || !ws->st.radii || !ws->st.conic_opacity)) return SPLAT_E_INVALID;
    if (!ws->st.point_list || !ws->st.final_T || !ws->st.n_contrib || !ws->st.tile_base) return SPLAT_E_INVALID;
    return check(launch_iter_means2d_accumulate(*cam, *map, *ws, gaccum, denom, means2D_grad, (hipStream_t)stream));
}

static bool valid_densify(const SplatMapStore *store, const SplatDensifyArgs *a) {
    if (!valid_store(store) || !a || !a->flags || !a->scratch) return false;
    if (a->mode != SPLAT_DENSIFY_CLONE && a->mode != SPLAT_DENSIFY_SPLIT) return false;
    if (a->rows_with_grad < 0 || a->rows_with_grad > store->map.P) return false;
    if (a->rows_with_grad > 0 && (!store->means2D_gradient_accum || !store->denom)) return false;
    if (a->mode == SPLAT_DENSIFY_SPLIT && a->num_to_split_into < 1) return false;
    return true;
}

int splat_map_densify_select(SplatMapStore *store, const SplatDensifyArgs *a, void *stream) {
    if (!valid_densify(store, a)) return SPLAT_E_INVALID;
    return check(launch_map_densify_select(*store, *a, (hipStream_t)stream));
}

int splat_map_duplicate(SplatMapStore *store, const SplatDensifyArgs *a, void *stream) {
    if (!valid_densify(store, a)) return SPLAT_E_INVALID;
    if (a->mode == SPLAT_DENSIFY_SPLIT && !a->samples) return SPLAT_E_INVALID;
    return check(launch_map_duplicate(*store, *a, (hipStream_t)stream));
}

int splat_debug_option(int key, int value) {
    if (key == 0) { const int old = g_debug_skip_count; g_debug_skip_count = value; return old; }
    if (key == 4) { const int old = g_debug_k7_bits; g_debug_k7_bits = value; return old; }
    if (key == 5) { const int old = g_debug_mesh_split; g_debug_mesh_split = value > 0 ? value : 0; return old; }
    if (key == 6) { const int old = g_debug_mesh_bits; g_debug_mesh_bits = value; return old; }
    return -1;
}

int splat_debug_stamps(void *buffer) {
    g_debug_stamps = reinterpret_cast<long long *>(buffer);
    return SPLAT_OK;
}

// test hook (tests/test_gpu_primitives.py): see launch_selftest in binning.hip
int splat_selftest(int which, const void *in, void *out, int n, void *stream) {
    return check(launch_selftest(which, in, out, n, (hipStream_t)stream));
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// scratch layouts (include/splat_hip.h: "Scratch layouts")
// ---------------------------------------------------------------------------------------------------------
namespace {
struct LayoutWriter {
    SplatArrayInfo *out;
    int32_t max_entries, n = 0;
    size_t offset = 0;
    void add(const char *name, size_t bytes, int zero_init) {
        offset = (offset + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN;
        if (out && n < max_entries) out[n] = SplatArrayInfo{name, bytes, offset, zero_init};
        ++n;
        offset += bytes;
    }
};

// the arrays of a SplatState; `prefix`: the names as fields of SplatState ("") or of SplatIterWorkspace ("st.").  `iter`: the fused
// iteration's state (bucketed lists + group binning + launch order; its counters must start zeroed: no memset launches in the loop)
void state_arrays(LayoutWriter &w, bool iter, int32_t P, int32_t width, int32_t height, int32_t sub_bins, int64_t capacity,
                  int32_t group_stride, int32_t flags) {
    const size_t T = splat_num_tiles(width, height), S = sub_bins > 1 ? (size_t)sub_bins : 1, n = (size_t)P, cap = (size_t)capacity;
    const size_t G = (size_t)(((width + SPLAT_TILE - 1) / SPLAT_TILE + SPLAT_GROUP_TILES - 1) / SPLAT_GROUP_TILES) *
                     (size_t)(((height + SPLAT_TILE - 1) / SPLAT_TILE + SPLAT_GROUP_TILES - 1) / SPLAT_GROUP_TILES);
    const size_t HW = (size_t)width * (size_t)height;
    const int z = iter ? 1 : 0;
#define NAME(f) (iter ? "st." f : f)
    w.add(NAME("depth"), 4 * n, 0);
    w.add(NAME("xy"), 8 * n, 0);
    w.add(NAME("conic_opacity"), 16 * n, 0);
    w.add(NAME("rect"), 8 * n, 0);
    w.add(NAME("radii"), 4 * n, z);
    if (flags & SPLAT_LAYOUT_SH) {
        w.add(NAME("rgb"), 12 * n, 0);
        w.add(NAME("clamped"), 3 * n, 0);
    }
    w.add(NAME("tile_count"), 4 * T * S * SPLAT_COUNTER_STRIDE, z);
    w.add(NAME("tile_base"), 4 * (T + 1), 0);
    w.add(NAME("tile_cursor"), 4 * T * S * SPLAT_COUNTER_STRIDE, 0);
    if (iter || !(flags & SPLAT_LAYOUT_GROUPS)) w.add(NAME("keys"), 8 * cap, 0);
    w.add(NAME("point_list"), 4 * cap, 0);
    if (flags & SPLAT_LAYOUT_RECS) w.add(NAME("tile_recs"), 48 * cap, 0);
    if (flags & SPLAT_LAYOUT_LONG_LISTS) {
        w.add(NAME("keys_alt"), 8 * cap, 0);
        w.add(NAME("long_items"), 4 * (cap / 1024 + T + 1), 0);
    }
    w.add(NAME("long_base"), 4 * (T + 1), z);
    if (iter) {
        w.add("st.group_count", 4 * G * SPLAT_COUNTER_STRIDE, 1);
        if (group_stride > 0) w.add("st.group_recs", 16 * G * (size_t)group_stride, 0);
        if (flags & SPLAT_LAYOUT_TILE_ORDER) {
            w.add("st.tile_work", 4 * T, 1);
            w.add("st.tile_order", 4 * 8 * ((T + 7) / 8), 1);        // (zero = the natural order: SplatState.tile_order)
        }
    }
    w.add(NAME("final_T"), 4 * HW, 0);
    w.add(NAME("n_contrib"), 4 * HW, 0);
    if (!iter && (flags & SPLAT_LAYOUT_GROUPS)) {
        // group binning behind the reference API: the counters sit right in front of the status words (the library zeroes both with
        // one memset per call: launch_preprocess_forward)
        if (group_stride > 0) w.add("group_recs", 16 * G * (size_t)group_stride, 0);
        // (padded to the slab alignment: the status words then sit EXACTLY behind it, and the padding is the array's own)
        w.add("group_count", (4 * G * SPLAT_COUNTER_STRIDE + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN, 0);
    }
    w.add(NAME("status"), 4 * 4, z);
#undef NAME
}

bool layout_args_ok(int32_t P, int32_t width, int32_t height, int64_t capacity) {
    return P >= 0 && width > 0 && height > 0 && capacity >= 0 && width <= 65535 * SPLAT_TILE && height <= 65535 * SPLAT_TILE;
}
}  // namespace

extern "C" {

int splat_state_layout(int32_t P, int32_t width, int32_t height, int32_t sub_bins, int64_t capacity, int32_t flags,
                       SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes) {
    if (!layout_args_ok(P, width, height, capacity) || sub_bins < 0 || (sub_bins & (sub_bins - 1)) != 0) return -SPLAT_E_INVALID;
    LayoutWriter w{out, max_entries};
    const size_t tiles = splat_num_tiles(width, height);
    const int64_t tile_stride = tiles ? capacity / (int64_t)tiles : 0;
    if ((flags & SPLAT_LAYOUT_GROUPS) && (tile_stride < 1 || tile_stride > (1 << 20) || sub_bins > 1)) return -SPLAT_E_INVALID;
    state_arrays(w, false, P, width, height, sub_bins, capacity, (flags & SPLAT_LAYOUT_GROUPS) ? (int32_t)(SPLAT_GROUP_TILES * SPLAT_GROUP_TILES * tile_stride) : 0, flags);
    if (flags & SPLAT_LAYOUT_BACKWARD) w.add("accum", 4 * (size_t)SPLAT_GRAD_STRIDE * (size_t)P, 0);
    if (total_bytes) *total_bytes = (w.offset + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN;
    return w.n;
}

size_t splat_workspace_bytes(int32_t P, int32_t width, int32_t height, int64_t capacity) {
    size_t total = 0;
    if (splat_state_layout(P, width, height, 1, capacity, SPLAT_LAYOUT_LONG_LISTS | SPLAT_LAYOUT_BACKWARD, nullptr, 0, &total) < 0) return 0;
    return total;
}

int splat_state_bind(SplatState *st, SplatGrads *gr, void *slab, const SplatArrayInfo *arrays, int32_t n, int32_t sub_bins,
                     int64_t capacity) {
    if (!st || !slab || !arrays || n < 0 || ((uintptr_t)slab % SPLAT_SLAB_ALIGN) != 0) return SPLAT_E_INVALID;
    char *base = static_cast<char *>(slab);
    for (int32_t i = 0; i < n; ++i) {
        const char *name = arrays[i].name;
        void *p = base + arrays[i].offset;
        if (!name) return SPLAT_E_INVALID;
        if (strncmp(name, "st.", 3) == 0) name += 3;
#define BIND(field, T) if (strcmp(name, #field) == 0) { st->field = static_cast<T>(p); continue; }
        BIND(depth, float *) BIND(xy, float *) BIND(conic_opacity, float *) BIND(rect, uint32_t *) BIND(radii, int32_t *)
        BIND(rgb, float *) BIND(clamped, uint8_t *) BIND(tile_count, uint32_t *) BIND(tile_base, uint32_t *) BIND(tile_cursor, uint32_t *)
        BIND(keys, uint64_t *) BIND(point_list, uint32_t *) BIND(tile_recs, float *) BIND(keys_alt, uint64_t *) BIND(long_base, uint32_t *) BIND(long_items, uint32_t *)
        BIND(group_count, uint32_t *) BIND(group_recs, uint32_t *) BIND(tile_work, uint32_t *) BIND(tile_order, uint32_t *)
        BIND(final_T, float *) BIND(n_contrib, int32_t *) BIND(status, int32_t *)
#undef BIND
        if (strcmp(name, "accum") == 0) { if (gr) gr->accum = static_cast<float *>(p); continue; }
    }
    st->capacity = capacity;
    st->sub_bins = sub_bins;
    return SPLAT_OK;
}

int splat_iter_workspace_layout(int32_t P, int32_t width, int32_t height, int64_t capacity, int32_t group_stride, int32_t flags,
                                SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes) {
    if (!layout_args_ok(P, width, height, capacity) || group_stride < 0) return -SPLAT_E_INVALID;
    LayoutWriter w{out, max_entries};
    const size_t n = (size_t)P, HW = (size_t)width * (size_t)height;
    state_arrays(w, true, P, width, height, 1, capacity, group_stride, flags | SPLAT_LAYOUT_LONG_LISTS);
    w.add("feat8", 4 * 8 * n, 0);
    w.add("out6", 4 * 6 * HW, 0);
    w.add("dL_dout6", 4 * 6 * HW, 1);
    w.add("accum", 4 * (size_t)SPLAT_GRAD_STRIDE * n, 1);
    if (flags & SPLAT_LAYOUT_SSIM) w.add("ssim_maps", 4 * 9 * HW, 0);
    w.add("sums", 8 * (size_t)SPLAT_ITER_SUM_COPIES * SPLAT_ITER_SUMS, 1);
    w.add("d_cam", 4 * SPLAT_ITER_DCAM, 1);
    if (flags & SPLAT_LAYOUT_OUTLIER) {
        w.add("outlier_err", 4 * HW, 0);
        w.add("outlier_scratch", 4 * splat_map_scratch_words((int64_t)HW), 1);
    }
    if (total_bytes) *total_bytes = (w.offset + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN;
    return w.n;
}

size_t splat_iter_workspace_bytes(int32_t P, int32_t width, int32_t height, int64_t capacity, int32_t group_stride, int32_t flags) {
    size_t total = 0;
    if (splat_iter_workspace_layout(P, width, height, capacity, group_stride, flags, nullptr, 0, &total) < 0) return 0;
    return total;
}

int splat_iter_workspace_bind(SplatIterWorkspace *ws, void *slab, const SplatArrayInfo *arrays, int32_t n, int64_t capacity,
                              int32_t group_stride) {
    if (!ws) return SPLAT_E_INVALID;
    int rc = splat_state_bind(&ws->st, nullptr, slab, arrays, n, 1, capacity);
    if (rc) return rc;
    char *base = static_cast<char *>(slab);
    for (int32_t i = 0; i < n; ++i) {
        const char *name = arrays[i].name;
        void *p = base + arrays[i].offset;
#define BIND(field, T) if (strcmp(name, #field) == 0) { ws->field = static_cast<T>(p); continue; }
        BIND(feat8, float *) BIND(out6, float *) BIND(dL_dout6, float *) BIND(accum, float *) BIND(ssim_maps, float *)
        BIND(sums, double *) BIND(d_cam, float *) BIND(outlier_err, float *) BIND(outlier_scratch, uint32_t *)
#undef BIND
    }
    ws->st.group_stride = ws->st.group_recs ? group_stride : 0;
    return SPLAT_OK;
}

int splat_eval_workspace_layout(int32_t width, int32_t height, int32_t flags, SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes) {
    if (width <= 0 || height <= 0 || (long long)width * height > 0x3fffffffLL) return -SPLAT_E_INVALID;
    if ((flags & SPLAT_EVAL_LAYOUT_MS_SSIM) && (width < height ? width : height) <= 160) return -SPLAT_E_INVALID;
    LayoutWriter w{out, max_entries};
    if (flags & SPLAT_EVAL_LAYOUT_MS_SSIM) w.add("pyramid", eval_pyramid_bytes(width, height), 0);
    w.add("sums", 8 * (size_t)(SPLAT_ITER_SUM_COPIES + 1) * SPLAT_EVAL_SUMS, 1);
    if (total_bytes) *total_bytes = (w.offset + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN;
    return w.n;
}

int splat_eval_workspace_bind(SplatEvalWorkspace *ews, void *slab, const SplatArrayInfo *arrays, int32_t n) {
    if (!ews || !slab || !arrays || n < 0 || ((uintptr_t)slab % SPLAT_SLAB_ALIGN) != 0) return SPLAT_E_INVALID;
    char *base = static_cast<char *>(slab);
    for (int32_t i = 0; i < n; ++i) {
        if (!arrays[i].name) return SPLAT_E_INVALID;
        if (strcmp(arrays[i].name, "pyramid") == 0) ews->pyramid = reinterpret_cast<float *>(base + arrays[i].offset);
        if (strcmp(arrays[i].name, "sums") == 0) ews->sums = reinterpret_cast<double *>(base + arrays[i].offset);
    }
    return SPLAT_OK;
}

// the LPIPS layer (csrc/lpips.hip)
static_assert(SPLAT_LPIPS_LAYERS == kLpipsLayers && SPLAT_LPIPS_MIN_SIZE == kLpipsMinSize, "include/splat_hip.h and lpips_math.h agree");

size_t splat_lpips_weight_floats(void) { return lpips_weight_floats(); }
size_t splat_lpips_pack_floats(void) { return lpips_pack_floats(); }
int32_t splat_lpips_tap_size(int32_t n, int32_t layer) { return n <= 0 || layer < 0 || layer >= kLpipsLayers ? 0 : lpips_tap_size(n, layer); }

static bool valid_lpips_size(int32_t width, int32_t height) {
    return width >= kLpipsMinSize && height >= kLpipsMinSize && (long long)width * height <= 0x3ffffffLL;
}

int splat_lpips_workspace_layout(int32_t width, int32_t height, SplatArrayInfo *out, int32_t max_entries, size_t *total_bytes) {
    if (!valid_lpips_size(width, height)) return -SPLAT_E_INVALID;
    static const char *const tap_names[kLpipsLayers] = {"tap0", "tap1", "tap2", "tap3", "tap4"};
    static const char *const pool_names[2] = {"pool1", "pool2"};
    LayoutWriter w{out, max_entries};
    w.add("input", 4 * 6 * (size_t)width * height, 0);
    int pools = 0;
    for (int l = 0; l < kLpipsLayers; ++l) {
        const LpipsLayer L = lpips_layer(l);
        if (L.pool) w.add(pool_names[pools++], 4 * 2 * (size_t)L.cin * lpips_layer_in(width, l) * lpips_layer_in(height, l), 0);
        w.add(tap_names[l], 4 * 2 * (size_t)L.cout * lpips_tap_size(width, l) * lpips_tap_size(height, l), 0);
    }
    w.add("partials", 8 * lpips_partial_rows(width, height), 0);
    if (total_bytes) *total_bytes = (w.offset + SPLAT_SLAB_ALIGN - 1) / SPLAT_SLAB_ALIGN * SPLAT_SLAB_ALIGN;
    return w.n;
}

int splat_lpips_workspace_bind(SplatLpipsWorkspace *ws, void *slab, const SplatArrayInfo *arrays, int32_t n, int32_t width, int32_t height) {
    if (!ws || !slab || !arrays || n < 0 || ((uintptr_t)slab % SPLAT_SLAB_ALIGN) != 0 || !valid_lpips_size(width, height)) return SPLAT_E_INVALID;
    *ws = SplatLpipsWorkspace{};
    char *base = static_cast<char *>(slab);
    for (int32_t i = 0; i < n; ++i) {
        const char *name = arrays[i].name;
        if (!name) return SPLAT_E_INVALID;
        float *p = reinterpret_cast<float *>(base + arrays[i].offset);
        if (strcmp(name, "input") == 0) ws->input = p;
        else if (strncmp(name, "tap", 3) == 0 && name[3] >= '0' && name[3] < '0' + kLpipsLayers && !name[4]) ws->taps[name[3] - '0'] = p;
        else if (strcmp(name, "pool1") == 0) ws->pooled[0] = p;
        else if (strcmp(name, "pool2") == 0) ws->pooled[1] = p;
        else if (strcmp(name, "partials") == 0) ws->partials = reinterpret_cast<double *>(p);
    }
    ws->width = width;
    ws->height = height;
    return SPLAT_OK;
}

int splat_lpips_pack(const float *weights, float *net, void *stream) {
    if (!weights || !net) return SPLAT_E_INVALID;
    return check(launch_lpips_pack(weights, net, (hipStream_t)stream));
}

int splat_lpips_conv(int32_t layer, int32_t in_width, int32_t in_height, const float *x, const float *net, float *y, void *stream) {
    if (layer < 0 || layer >= kLpipsLayers || !x || !net || !y || in_width <= 0 || in_height <= 0) return SPLAT_E_INVALID;
    const LpipsLayer L = lpips_layer(layer);
    if (lpips_conv_out(in_width, L.k, L.stride, L.pad) <= 0 || lpips_conv_out(in_height, L.k, L.stride, L.pad) <= 0) return SPLAT_E_INVALID;
    if ((long long)in_width * in_height * L.cin > 0x1fffffffLL) return SPLAT_E_INVALID;
    return check(launch_lpips_conv(layer, in_width, in_height, x, net, y, (hipStream_t)stream));
}

// laid out and bound for exactly this size: the kernels write what the size implies, a smaller slab would be overrun
static bool valid_lpips_workspace(const SplatLpipsWorkspace *ws, int32_t width, int32_t height) {
    if (!ws || ws->width != width || ws->height != height || !ws->input || !ws->pooled[0] || !ws->pooled[1] || !ws->partials) return false;
    for (int l = 0; l < kLpipsLayers; ++l)
        if (!ws->taps[l]) return false;
    return true;
}

int splat_lpips_planes(int32_t width, int32_t height, const float *rgb, const float *silhouette, const float *gt_im, const float *gt_depth,
                       float sil_thres, int32_t sil_mask, const float *net, const SplatLpipsWorkspace *workspace, double *out, void *stream) {
    if (!valid_lpips_size(width, height) || !valid_lpips_workspace(workspace, width, height) || !rgb || !gt_im || !gt_depth || !net || !out ||
        (sil_mask && !silhouette))
        return SPLAT_E_INVALID;
    return check(launch_lpips(width, height, rgb, gt_im, silhouette, gt_depth, sil_thres, sil_mask, net, *workspace, out, (hipStream_t)stream));
}

int splat_lpips_images(int32_t width, int32_t height, const float *im0, const float *im1, const float *net,
                       const SplatLpipsWorkspace *workspace, double *out, void *stream) {
    if (!valid_lpips_size(width, height) || !valid_lpips_workspace(workspace, width, height) || !im0 || !im1 || !net || !out) return SPLAT_E_INVALID;
    return check(launch_lpips(width, height, im0, im1, nullptr, nullptr, 0.f, 0, net, *workspace, out, (hipStream_t)stream));
}

}  // extern "C"
