"""Fused SplaTAM iteration: the reference's per-iteration Python (``get_loss`` ->
``loss.backward()`` -> ``optimizer.step()``, /root/reference/scripts/splatam.py:690-711
and :828-869) as ~10 kernel launches of libsplat_hip.so with no host synchronisation.

``FusedEngine`` owns the device scratch (geometry, per-tile lists, the 6-channel
render, loss gradients, Adam moments) and updates the caller's ``params`` tensors
IN PLACE, exactly as ``torch.optim.Adam`` does for the reference.  Results are the
same function of the same inputs as ``splatam_amd.slam.get_loss`` + autograd +
``torch.optim.Adam`` (tests/test_gpu_fused.py), for every argument of ``get_loss``
(incl. ``ignore_outlier_depth_loss``: ``torch.median`` by exact radix selection); only
the colour pass' own ``means2D.grad`` (gradient-based densification) is not produced.

Everything is computed by the C ABI (include/splat_hip.h, "Fused SplaTAM
iteration"); PyTorch only owns the memory and the stream.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from collections import ChainMap, namedtuple
from types import MappingProxyType

import torch

from . import _capi, slam
from .map_pass import fit_lists
from .frames import ingest_frame, ingest_planes, prepare_frame  # noqa: F401  (the frame path lives in frames.py)
from .rasterizer import _cached_contiguous

PARAM_ORDER = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
VARIABLE_KEYS = ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")
_FLAG_SLOTS = 16        # floats ahead of the flat gradient bucket (one 64-byte line): slot 0 = capacity flag of the exchange
# the iteration report's slots and the status words (include/splat_hip.h), bound once for the host paths
_REPORT_FLAG, _REPORT_STATUS, _REPORT_SKIPPED = _capi.SPLAT_REPORT_FLAG, _capi.SPLAT_REPORT_STATUS, _capi.SPLAT_REPORT_SKIPPED
_STATUS_INSTANCES, _STATUS_OVERFLOW = _capi.SPLAT_STATUS_INSTANCES, _capi.SPLAT_STATUS_OVERFLOW
_STATUS_LONGEST, _STATUS_STALE_HINT = _capi.SPLAT_STATUS_LONGEST, _capi.SPLAT_STATUS_STALE_HINT


def _layout(W, H, rows=0, capacity=0, group_stride=0, outlier=False):
    """Every array of the iteration's workspace is sized by the LIBRARY (splat_iter_workspace_layout, include/splat_hip.h "Scratch
    layouts"); they are tensors of their own here because the per-Gaussian ones grow with the map, the lists with a camera's needs."""
    flags = _capi.SPLAT_LAYOUT_SSIM | _capi.SPLAT_LAYOUT_TILE_ORDER | _capi.SPLAT_LAYOUT_RECS | (_capi.SPLAT_LAYOUT_OUTLIER if outlier else 0)
    return _capi.iter_workspace_layout(int(rows), W, H, int(capacity), int(group_stride), flags)


def _new(dev, lay, name, dtype, tail=()):
    n = lay.bytes[name] // torch.empty((), dtype=dtype).element_size()
    t = (torch.zeros if lay.zero_init[name] else torch.empty)(n, dtype=dtype, device=dev)
    return t.view((-1,) + tuple(tail)) if tail else t


class _Camera:
    """What ONE camera of a ``FusedEngine`` owns: its size and launch struct, the per-pixel and per-tile arrays, the lists and what has
    been learnt about them, the tile orders.  Arrays live in ``buf`` under the names the engine's ``buf`` shows them by.  Complete when
    the constructor returns; the map, its Adam state and the per-Gaussian scratch are the engine's."""
    # workspace arrays by the library's field names: (name in the layout, key in ``buf``, dtype)
    _FIXED_ARRAYS = (("st.tile_count", "tile_count", torch.int32), ("st.tile_base", "tile_base", torch.int32),
                     ("st.tile_cursor", "tile_cursor", torch.int32), ("st.long_base", "long_base", torch.int32),
                     ("st.group_count", "group_count", torch.int32), ("st.status", "status", torch.int32),
                     ("st.tile_work", "tile_work", torch.int32), ("st.tile_order", "tile_order", torch.int32),
                     ("st.final_T", "final_T", torch.float32), ("st.n_contrib", "n_contrib", torch.int32),
                     ("out6", "out6", torch.float32), ("dL_dout6", "dL_dout6", torch.float32),
                     ("ssim_maps", "ssim_maps", torch.float32), ("sums", "sums", torch.float64), ("d_cam", "d_cam", torch.float32))

    def __init__(self, dev, settings, rows, capacity, use_recs):
        """settings: a GaussianRasterizationSettings; rows: the map's row capacity; capacity: (Gaussian, tile) instances the lists
        hold.  List statistics start unknown: the camera learns them on its first use (``FusedEngine.check_overflow``)."""
        self.dev, self.settings = dev, settings
        self.H, self.W = H, W = int(settings.image_height), int(settings.image_width)
        self.num_tiles = int(_capi.lib().splat_num_tiles(W, H))
        GT = _capi.SPLAT_GROUP_TILES
        self.num_groups = (((W + 15) // 16 + GT - 1) // GT) * (((H + 15) // 16 + GT - 1) // GT)
        self.struct = self._make_struct(settings)   # (raises for a camera the fused path cannot render, before anything is allocated)
        self.buf = {}
        self._alloc_fixed(_layout(W, H, rows))
        # launch order of the composites' workgroups (SplatState.tile_work / tile_order): heaviest tiles of every XCD band first.  An entry
        # holds tile + 1; the zero-initialised buffer of the library's layout IS the natural order.  One order PER VIEW (keyed by the
        # frame's time index, the last 64 views): an iteration leaves the order for the NEXT visit of its view.  Mapping draws a random
        # keyframe per iteration (/root/reference/scripts/splatam.py:831-845): the order the previous iteration left belongs to another view
        self._natural_order, self._orders = torch.zeros_like(self.buf['tile_order']), {}
        self.max_list_hint = 0          # longest tile list seen at the last check_overflow(); 0 = unknown
        self.tile_stride = 0            # > 0: bucketed lists (no scan / scatter pass), learnt by check_overflow()
        self._tile_rows = None          # (begin, end): the band of tile rows the next iteration composites (tile-row-sharded tracking)
        self._stats_partial = False     # the last iteration's list statistics cover a band only: check_overflow() does not learn from them
        self.sub_bins = 1               # counters per tile on the exact-list path (16 once lists get very long: SplatState.sub_bins)
        self.learnt_P = None            # rows of the map the list statistics were learnt on (keep_lists)
        self.alloc_lists(capacity, use_recs)

    def _make_struct(self, settings):
        if float(settings.bg.abs().max()) != 0.0:
            raise RuntimeError("the fused iteration renders with a zero background (as setup_camera builds it)")
        view = _cached_contiguous(settings.viewmatrix)
        proj = _cached_contiguous(settings.projmatrix)
        campos = _cached_contiguous(settings.campos)
        bg6 = torch.zeros(8, dtype=torch.float32, device=self.dev)
        cam = _capi.SplatCamera()
        cam.image_height, cam.image_width = self.H, self.W
        cam.tanfovx, cam.tanfovy = float(settings.tanfovx), float(settings.tanfovy)
        cam.bg, cam.scale_modifier = bg6.data_ptr(), float(settings.scale_modifier)
        cam.viewmatrix, cam.projmatrix = view.data_ptr(), proj.data_ptr()
        cam.sh_degree, cam.campos, cam.prefiltered = 0, campos.data_ptr(), 0
        self._struct_keep = (bg6, view, proj, campos)
        return cam

    def _alloc_fixed(self, lay):
        for name, key, dtype in self._FIXED_ARRAYS:
            self.buf[key] = _new(self.dev, lay, name, dtype)
        for key, lead in (('final_T', ()), ('n_contrib', ()), ('out6', (6,)), ('dL_dout6', (6,)), ('ssim_maps', (9,))):
            self.buf[key] = self.buf[key].view(lead + (self.H, self.W))

    def alloc_lists(self, capacity, use_recs):
        self.capacity = int(capacity)
        lay = _layout(self.W, self.H, capacity=self.capacity)
        for name, key, dtype in (("st.keys", "keys", torch.int64), ("st.keys_alt", "keys_alt", torch.int64),        # keys_alt: merge passes of lists beyond LDS
                                 ("st.point_list", "point_list", torch.int32),
                                 # work-item table of the multi-workgroup sort (SplatState.long_items): one word per 1024 keys of a long list
                                 ("st.long_items", "long_items", torch.int32)):
            self.buf[key] = _new(self.dev, lay, name, dtype)
        # the staged record of every list entry, handed from the forward to the backward composite (SplatState.tile_recs: 48 bytes per
        # slot; left out beyond 16 GB -- the clustered stress scenes' hundreds of millions of slots -- where the backward composite
        # gathers as before)
        self.buf['tile_recs'] = None
        if use_recs and lay.bytes["st.tile_recs"] <= 16 << 30:
            self.buf['tile_recs'] = _new(self.dev, lay, "st.tile_recs", torch.float32)

    def alloc_group_recs(self, group_stride):   # the records of group binning, when first needed or outgrown (FusedEngine._workspace)
        recs = self.buf['group_recs'] = _new(self.dev, _layout(self.W, self.H, group_stride=group_stride), "st.group_recs", torch.int32)
        assert recs.numel() == self.num_groups * group_stride * 4
        return recs

    def alloc_outlier_scratch(self):            # of the median selection (ignore_outlier_depth_loss), on first use
        lay = _layout(self.W, self.H, outlier=True)
        self.buf['outlier_err'] = _new(self.dev, lay, "outlier_err", torch.float32)
        self.buf['outlier_scratch'] = _new(self.dev, lay, "outlier_scratch", torch.int32)

    def set_sub_bins(self, S):
        """Very long per-tile lists stay on the exact-list path (their buckets would not fit); their count / scatter atomics
        are then spread over S counters per tile (same-address serialisation otherwise: 0.9 ms per pass at 11 M instances)."""
        if S == self.sub_bins:
            return
        CS = _capi.SPLAT_COUNTER_STRIDE
        self.sub_bins = S
        self.buf['tile_count'] = torch.zeros(self.num_tiles * CS * S, dtype=torch.int32, device=self.dev)
        self.buf['tile_cursor'] = torch.zeros(self.num_tiles * CS * S, dtype=torch.int32, device=self.dev)

    def select_order(self, view):
        """Point ``buf['tile_order']`` at the launch order view ``view`` left at its last visit (the natural order at its first)."""
        o = self._orders.pop(view, None)
        if o is None:
            if len(self._orders) >= 64:
                self._orders.pop(next(iter(self._orders)))          # the view visited longest ago
            o = self._natural_order.clone()
        self._orders[view] = o                                      # (most recently visited last)
        self.buf['tile_order'] = o

    def reset_status(self):
        """Forget what the renders so far flagged: the status words and the list counters they left (before a re-learn, in a digest)."""
        for key in ('status', 'tile_count', 'group_count'):
            self.buf[key].zero_()

    def keep_lists(self, P, within, only_bucketed):
        """Keep or forget the list statistics for a map of ``P`` rows: kept when the rows moved by less than ``within`` of the rows the
        statistics were learnt on.  ``only_bucketed``: a camera without buckets (``tile_stride == 0``) forgets in any case, which
        resets a ``max_list_hint`` it still holds."""
        ref = self.learnt_P
        if ref is None or (only_bucketed and self.tile_stride == 0) or abs(P - ref) > within * max(ref, 1):
            self.tile_stride, self.max_list_hint = 0, 0     # exact lists until check_overflow() / relearn_lists() learns them again


class FusedEngine:
    def __init__(self, params, cam, capacity=None, track_max_radius=None, gaussian_capacity=None, variables=None, row_headroom=0.0):
        """params: the reference's dict of float32 CUDA tensors / Parameters (updated in place);
        cam: a GaussianRasterizationSettings; capacity: (Gaussian, tile) instances the lists can hold;
        gaussian_capacity: rows the map may grow to.  When given, the five Gaussian tensors (and ``variables``' per-Gaussian
        entries) move into capacity-sized backing arrays owned by the engine and ``params[k]`` / ``variables[k]`` become
        views of their first P rows, re-made after every ``add_new_gaussians`` / ``prune_gaussians`` -- the reference
        replaces the dict entries at the same places (/root/reference/scripts/splatam.py:410-411).
        row_headroom (engines that do NOT own the map): the per-Gaussian scratch is allocated for (1 + row_headroom) x P rows, so
        that ``rebind`` to a map the caller has grown (splatam_amd.plugin) need not re-allocate it."""
        self.L = _capi.lib()
        self.params = params
        self.variables = variables
        dev = params['means3D'].device
        if dev.type != "cuda":
            raise RuntimeError("FusedEngine needs CUDA/HIP tensors; the HIP library has no CPU path")
        self.dev = dev
        self._check_params(params)
        # ---- the map, once: parameters / ``store``, per-Gaussian scratch rows, pose state, gradients and Adam moments; its arrays are in ``map_buf``
        P = params['means3D'].shape[0]
        self.P = P
        self.iso = params['log_scales'].shape[1] == 1
        self.managed = gaussian_capacity is not None
        self.Pcap = max(int(gaussian_capacity), P) if self.managed else int(P * (1.0 + float(row_headroom)))
        self.store = None
        if self.managed:
            self._adopt(params, variables)
        elif variables is not None and track_max_radius is None:
            track_max_radius = variables.get('max_2D_radius')
        self.num_frames = params['cam_unnorm_rots'].shape[-1]
        self.map_buf = {}
        self._alloc_rows(_layout(int(cam.image_width), int(cam.image_height), self.Pcap))
        self.map_buf['pose_state'] = torch.zeros(_capi.SPLAT_POSE_STATE, dtype=torch.float32, device=dev)
        self.max_2D_radius = self.store['max_2D_radius'] if self.managed else track_max_radius
        self.map_buf['counts'] = torch.zeros(8, dtype=torch.int32, device=dev)
        self._widths = [3, 3, 4, 1, 1 if self.iso else 3]
        self._alloc_map_state(self.Pcap)
        self._layout_rows()
        self.map_step = 0
        self.pose_step = 0
        self.track_time_idx = None
        self.map_version = 0            # counts the edits of the map's rows (_set_rows, rebind): what render_view's replay caches are keyed by
        self.allow_buckets = True
        # group binning (SplatState.group_count): with bucketed lists short enough for the composite's own sort, the per-Gaussian
        # kernel files one record per 2 x 2-tile group (slots through an LDS histogram) and the composite filters its group's
        # records: ~10x fewer global atomics in the per-Gaussian kernel.  Results do not depend on it
        self.group_bins = True
        # the Adam step inside F6 touches moments and parameters row by row (12-byte rows).  Round 2: it lost to the separate, fully
        # coalesced adam_map_kernel once the rows no longer stayed cache resident (96 us fused vs 42 + 42 us at 830 k rows) and maps above
        # 500 k rows took the two-kernel form.  Since F6 requests all its moments in one round (round 3) the fused form is ahead at every
        # size measured (mapping at 816 k rows 1 491 -> 1 505 it/s, at 5 M 383 -> 386): no limit by default (SPLAT_FUSED_ADAM_MAX_ROWS)
        self.fused_adam_max_rows = int(os.environ.get("SPLAT_FUSED_ADAM_MAX_ROWS", 1 << 30))
        # rows in creation (pixel-scan) order: true for a map this engine grew itself (add_valid_depth_points / add_new_gaussians
        # append per pixel in scan order); callers that hand over such a map may set it.  Only a speed hint (SplatState.order_hint)
        self.creation_order = bool(self.managed and P == 0)
        self.keep_map_grads = True      # mapping_iteration: store the gradients beside the fused Adam step (False: as the reference's loop, which discards them)
        self._frame_keep = None
        self.track_fused = os.environ.get("SPLAT_TRACK_FUSED", "1") != "0"    # tracking: forward + loss + backward composite in one kernel
        self.track_fused_full = os.environ.get("SPLAT_TRACK_FUSED_FULL", "1") != "0"   # ... also when the map's gradients are wanted (the mapping form inside)
        self.fold_sums = os.environ.get("SPLAT_FOLD_SUMS", "1") != "0"     # tile-row-sharded tracking: exchange 256 B instead of 16 KB
        self.skipped_iterations = 0     # of the last check_overflow() / digest_report(): iterations whose Adam step the device skipped
        # ---- the cameras: each a _Camera that owns what belongs to it; ``_camera`` names the current one, whose arrays ``buf`` shows beside
        # the map's.  The engine's: whether the composites launch in a learnt order, one per view, and whether records are staged
        self.tile_order_on = os.environ.get("SPLAT_TILE_ORDER", "1") != "0"
        self.order_per_view = os.environ.get("SPLAT_TILE_ORDER_PER_VIEW", "1") != "0"
        self.use_recs = {"0": 0, "1": 1}.get(os.environ.get("SPLAT_TILE_RECS", "auto"), 2)      # SplatState.tile_recs: 0 never, 1 always, 2 by list length
        self._cams, self._cam_ok, self._camera = [], {}, None
        self.auto_cameras = False       # True: a curr_data['cam'] the engine does not know is registered on first use (add_camera)
        self.add_camera(cam, capacity)

    def _check_params(self, params):
        for k in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans"):
            t = params[k]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.dev:
                raise RuntimeError(f"params['{k}'] must be a contiguous float32 tensor on {self.dev}")

    # ------------------------------------------------------------------ cameras
    def _use(self, camera):
        """Make ``camera`` the current one: two references -- no allocation, no launch, nothing read."""
        if camera is not self._camera:
            self._camera = camera   # (``buf``: what callers read.  Read-only: the engine's own writes name the owner's dict)
            self.buf = MappingProxyType(ChainMap(camera.buf, self.map_buf))

    def _same_camera(self, cam, ref):
        return (int(cam.image_height) == int(ref.image_height) and int(cam.image_width) == int(ref.image_width)
                and float(cam.tanfovx) == float(ref.tanfovx) and float(cam.tanfovy) == float(ref.tanfovy)
                and float(cam.scale_modifier) == float(ref.scale_modifier)
                and all(torch.equal(getattr(cam, f).to(self.dev).float().reshape(-1), getattr(ref, f).to(self.dev).float().reshape(-1))
                        for f in ("viewmatrix", "projmatrix", "bg")))

    def _find_camera(self, cam):
        """Index of the known camera ``cam`` equals (size, tan-fov, scale modifier, view, projection, background), or None.  The
        comparison reads the matrices once per settings object; the object is remembered afterwards."""
        hit = self._cam_ok.get(id(cam))
        if hit is not None:
            return hit[1]
        for i, known in enumerate(self._cams):
            if cam is known.settings or self._same_camera(cam, known.settings):
                self._cam_ok[id(cam)] = (cam, i)        # keeps the tuple alive, so the id stays unique
                return i
        return None

    @property
    def num_cameras(self):
        return len(self._cams)

    def is_current(self, cam):
        """The settings ``cam`` are, or equal, the current camera's: selecting them would change nothing."""
        i = self._find_camera(cam)
        return i is not None and self._cams[i] is self._camera

    def add_camera(self, cam, capacity=None):
        """Register another camera (a GaussianRasterizationSettings) on this engine's map and make it the current one; a camera the
        engine already knows is selected.  The new camera gets per-pixel planes, tile arrays and lists of its own (``capacity``
        instances, default as at construction) and learns its list statistics on its first use, like a new engine does.  The map,
        its Adam state and the per-Gaussian scratch are shared.  Returns the camera's index.
        The capacity flag is the camera's (``d_cam``) while the backward accumulator is the map's: call ``check_overflow()`` BEFORE leaving
        a camera whose last iterations may have been flagged -- it clears the accumulator a flagged iteration left dirty, and the next
        camera's own flag is down, so its iteration would step on it."""
        i = self._find_camera(cam)
        if i is None:
            # built completely before the engine learns of it: a camera the fused path refuses leaves the engine as it was
            new = _Camera(self.dev, cam, self.Pcap, int(capacity) if capacity else 4 * self.P + 65536, self.use_recs)
            i = len(self._cams)
            self._cams.append(new)
            self._cam_ok[id(cam)] = (cam, i)
        self._use(self._cams[i])
        return i

    def select_camera(self, cam):
        """Make the known camera ``cam`` equals the current one (``lists_known`` / ``check_overflow`` / ``rendered`` speak for it).
        As with ``add_camera``: ``check_overflow()`` first when the camera being left may have been flagged."""
        i = self._find_camera(cam)
        if i is None:
            raise RuntimeError("select_camera: this FusedEngine does not know that camera (add_camera registers it)")
        self._use(self._cams[i])
        return i

    def _keep_lists(self, within, only_bucketed):
        """Every camera keeps or forgets its list statistics for the map as it is now, on the rows ITS statistics were learnt on."""
        for camera in self._cams:
            camera.keep_lists(self.P, within, only_bucketed)

    # ------------------------------------------------------------------ capacity-managed map
    # the per-Gaussian workspace arrays by the library's field names: (name in the layout, key in ``map_buf``, dtype, trailing shape)
    _ROW_ARRAYS = (("st.conic_opacity", "conic", torch.float32, (4,)), ("st.xy", "xy", torch.float32, (2,)), ("st.rect", "rect", torch.int32, (2,)),
                   ("st.depth", "depth", torch.float32, ()), ("st.radii", "radii", torch.int32, ()), ("feat8", "feat8", torch.float32, (8,)),
                   ("accum", "accum", torch.float32, (_capi.SPLAT_GRAD_STRIDE,)))

    def _alloc_rows(self, lay):
        for name, key, dtype, tail in self._ROW_ARRAYS:
            self.map_buf[key] = _new(self.dev, lay, name, dtype, tail)

    def _alloc_map_state(self, rows):
        """Gradients and Adam moments of a map of up to ``rows`` rows, zeroed.  The gradients are ONE flat buffer (the all-reduce bucket
        of the view-sharded mapping step), viewed per parameter (_layout_rows)."""
        z = dict(dtype=torch.float32, device=self.dev)
        self._grad_store = torch.zeros(_FLAG_SLOTS + sum(self._widths) * rows, **z)
        self._m_store = {k: torch.zeros(rows, w, **z) for k, w in zip(PARAM_ORDER, self._widths)}
        self._v_store = {k: torch.zeros(rows, w, **z) for k, w in zip(PARAM_ORDER, self._widths)}

    def _adopt(self, params, variables):
        """Move the caller's Gaussian tensors into backing arrays of ``self.Pcap`` rows."""
        dev, P = self.dev, self.P
        self.store = {}
        for k in PARAM_ORDER:
            src = params[k].detach()
            back = torch.zeros((self.Pcap,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
            back[:P] = src
            self.store[k] = back
        for k in VARIABLE_KEYS:
            back = torch.zeros(self.Pcap, dtype=torch.float32, device=dev)
            if variables is not None and k in variables:
                back[:P] = variables[k]
            self.store[k] = back
        self._publish()

    def _publish(self):
        """params[k] / variables[k] = views of the first P rows of the backing arrays."""
        P = self.P
        for k in PARAM_ORDER:
            self.params[k] = torch.nn.Parameter(self.store[k][:P], requires_grad=True)
        if self.variables is not None:
            for k in VARIABLE_KEYS:
                self.variables[k] = self.store[k][:P]
        self.max_2D_radius = self.store['max_2D_radius']

    def _layout_rows(self):
        """Views that depend on the number of rows: the flat gradient bucket and the moment views."""
        P = self.P
        # [0, _FLAG_SLOTS): the exchange's header -- slot 0 carries this rank's capacity flag through the SAME collective as the gradients
        # (exchange_gradients); the gradients follow, 64-byte aligned
        self.grad_flat = self._grad_store[_FLAG_SLOTS:_FLAG_SLOTS + sum(self._widths) * P]
        # the rotations go last: for an isotropic map their gradient is exactly zero and the exchange skips them
        order = [k for k in PARAM_ORDER if k != "unnorm_rotations"] + ["unnorm_rotations"]
        widths = dict(zip(PARAM_ORDER, self._widths))
        self.grads, o = {}, 0
        for k in order:
            self.grads[k] = self.grad_flat[o:o + widths[k] * P].view(P, widths[k])
            o += widths[k] * P
        self.reduce_flat = self.grad_flat[:(sum(self._widths) - 4) * P] if self.iso else self.grad_flat
        self._exchange_flat = self._grad_store[:_FLAG_SLOTS + self.reduce_flat.numel()]
        self.exp_avg = {k: self._m_store[k][:P] for k in PARAM_ORDER}
        self.exp_avg_sq = {k: self._v_store[k][:P] for k in PARAM_ORDER}

    def rebind(self, params, track_max_radius=None, keep_lists_within=0.10):
        """The caller replaced its tensors (the reference's add_new_gaussians / remove_points re-create every parameter:
        /root/reference/scripts/splatam.py:410-411, /root/reference/utils/slam_external.py:139-162): point the engine at the new
        ones.  The workspace (per-pixel planes, lists, records), the list statistics and the bucket stride are KEPT when the number
        of rows moved by less than ``keep_lists_within`` of the rows they were learnt on -- an engine built from scratch starts on
        exact lists (scan + scatter + sort launches) and re-learns them through a host read.  Engines that own their map
        (gaussian_capacity) are edited through add_new_gaussians / remove_points instead."""
        if self.managed:
            raise RuntimeError("rebind is for engines on caller-owned tensors")
        self._check_params(params)
        if (params['log_scales'].shape[1] == 1) != self.iso or params['cam_unnorm_rots'].shape[-1] != self.num_frames:
            raise RuntimeError("rebind: the map's layout (isotropy, number of frames) differs from the engine's")
        P = int(params['means3D'].shape[0])
        self.params = params
        self.max_2D_radius = track_max_radius
        if P > self.Pcap:
            # per-Gaussian scratch for the grown map (+12.5 %: the next few edits fit); accum must be zero, the others are written
            # by the per-Gaussian kernel before they are read
            cap = P + P // 8 + 1024
            self._alloc_rows(_layout(self._camera.W, self._camera.H, cap))
            self._alloc_map_state(cap)
            self.Pcap = cap
        changed = P != self.P
        self.P = P
        self.map_version += 1
        self._layout_rows()
        if changed:
            # (a camera that holds a list length but no buckets keeps it here; a map edit, _set_rows, drops it)
            self._keep_lists(keep_lists_within, only_bucketed=False)
        return self

    def _grow_rows(self, new_cap):
        """Re-allocate every per-Gaussian array for ``new_cap`` rows (contents of the first P rows kept)."""
        if not self.managed:
            raise RuntimeError("this FusedEngine was built without gaussian_capacity: the map cannot grow")
        dev, P = self.dev, self.P
        self.Pcap = int(new_cap)
        for k, t in self.store.items():
            self.store[k] = torch.zeros((self.Pcap,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            self.store[k][:P] = t[:P]
        m, v = self._m_store, self._v_store
        self._alloc_map_state(self.Pcap)
        for k in PARAM_ORDER:
            self._m_store[k][:P] = m[k][:P]
            self._v_store[k][:P] = v[k][:P]
        self._alloc_rows(_layout(self._camera.W, self._camera.H, self.Pcap))
        for key in ('flags', 'stage', 'map_scratch'):          # (sized by the rows: allocated again when next needed)
            self.map_buf.pop(key, None)
        self._publish()
        self._layout_rows()

    def _store_struct(self, with_moments):
        st = _capi.SplatMapStore()
        st.map = self._map_struct()
        st.capacity = self.Pcap
        for i, k in enumerate(PARAM_ORDER):
            st.exp_avg[i] = self._m_store[k].data_ptr() if with_moments else None
            st.exp_avg_sq[i] = self._v_store[k].data_ptr() if with_moments else None
        if self.managed:
            st.max_2D_radius = self.store['max_2D_radius'].data_ptr()
            st.means2D_gradient_accum = self.store['means2D_gradient_accum'].data_ptr()
            st.denom = self.store['denom'].data_ptr()
            st.timestep = self.store['timestep'].data_ptr()
        st.counts = self.map_buf['counts'].data_ptr()
        return st

    def _map_scratch(self, n):
        words = int(self.L.splat_map_scratch_words(int(n)))
        sc = self.map_buf.get('map_scratch')
        if sc is None or sc.numel() < words:
            sc = self.map_buf['map_scratch'] = torch.zeros(words, dtype=torch.int32, device=self.dev)
        return sc

    def _flags(self):               # one byte per row of the map: the selection of a pruning / densification step
        f = self.map_buf.get('flags')
        if f is None or f.numel() < self.Pcap:
            f = self.map_buf['flags'] = torch.empty(self.Pcap, dtype=torch.uint8, device=self.dev)
        return f

    def _set_rows(self, P, keep_lists_within=0.10):
        self.P = int(P)
        self.map_version += 1
        self._publish()
        self._layout_rows()
        # the per-tile list statistics were learnt for another map: back to exact lists until check_overflow() / relearn_lists()
        # re-learns them -- unless the number of rows moved by less than ``keep_lists_within`` of the rows they were learnt on (the frame
        # loop's edits: +0.7 % per add_new_gaussians, a handful of rows per pruning): the buckets are 1.5x the longest list seen, the
        # statistics are refreshed at the end of every phase, and a list that does outgrow its bucket raises the flag (the skipped
        # iterations are run again), so stale statistics can cost time, never a wrong step
        # (only_bucketed: a camera that holds a list length but no buckets drops it as well; rebind keeps it)
        self._keep_lists(keep_lists_within, only_bucketed=True)

    def replace_map(self, params):
        """A map read from a file takes the place of the engine's (the reference's checkpoint loader replaces ``params`` wholesale and
        zeroes the per-Gaussian variables, ``timestep`` included: /root/reference/scripts/splatam.py:609-614).  ``params``: the seven
        tensors; the two pose arrays must have the engine's number of frames.  Every camera forgets its list statistics."""
        if not self.managed:
            raise RuntimeError("replace_map is for engines that own their map (gaussian_capacity)")
        P = int(params['means3D'].shape[0])
        for k, w in zip(PARAM_ORDER, self._widths):
            if tuple(params[k].shape) != (P, w):
                raise ValueError(f"checkpoint entry '{k}' has shape {tuple(params[k].shape)}, this map's layout wants {(P, w)}")
        for k in ("cam_unnorm_rots", "cam_trans"):
            if tuple(params[k].shape) != tuple(self.params[k].shape):
                raise ValueError(f"checkpoint entry '{k}' has shape {tuple(params[k].shape)}, the run was declared with "
                                 f"{tuple(self.params[k].shape)} (num_frames = {self.num_frames})")
        if P > self.Pcap:
            self._grow_rows(P + P // 8 + 1024)
        with torch.no_grad():
            for k in PARAM_ORDER:
                self.store[k][:P] = params[k].detach().to(self.dev, torch.float32)
            for k in VARIABLE_KEYS:
                self.store[k].zero_()
            for k in ("cam_unnorm_rots", "cam_trans"):
                self.params[k].copy_(params[k].detach().to(self.dev, torch.float32))
        for k in PARAM_ORDER:
            self._m_store[k].zero_()
            self._v_store[k].zero_()
        self.creation_order = False
        self._set_rows(P, keep_lists_within=-1.0)

    def list_sizing(self):
        """What decides whether an iteration of this engine gets flagged, per camera in registration order: the lists' capacity, the
        bucket stride, the longest list and the rows it was learnt on, the counters per tile.  Host integers (an exact checkpoint
        keeps them: a flagged phase draws fresh random views for the iterations it runs again, so the loop's random stream depends on
        them)."""
        return [dict(H=c.H, W=c.W, capacity=c.capacity, tile_stride=c.tile_stride, max_list_hint=c.max_list_hint, learnt_P=c.learnt_P,
                     sub_bins=c.sub_bins) for c in self._cams]

    def set_list_sizing(self, sizing):
        """Inverse of ``list_sizing`` on an engine with the same cameras in the same order."""
        if len(sizing) != len(self._cams):
            raise ValueError(f"list sizing of {len(sizing)} cameras, this engine has {len(self._cams)}")
        for c, s in zip(self._cams, sizing):
            if (c.H, c.W) != (int(s['H']), int(s['W'])):
                raise ValueError(f"list sizing of a {s['H']} x {s['W']} camera, this engine's is {c.H} x {c.W}")
            if int(s['capacity']) != c.capacity:
                c.alloc_lists(int(s['capacity']), self.use_recs)
            c.set_sub_bins(int(s['sub_bins']))
            c.tile_stride, c.max_list_hint = int(s['tile_stride']), int(s['max_list_hint'])
            c.learnt_P = None if s['learnt_P'] is None else int(s['learnt_P'])

    def _frame(self, curr_data, time_idx, images=True):
        """The SplatFrameData of ``curr_data`` at pose ``time_idx`` (``images``: with its planes); ``_frame_keep`` keeps what it names alive.
        curr_data['w2c'] as the kernels read it: 16 contiguous floats on the engine's device (row 2 is the depth channel of
        the depth / silhouette render).  Anything else -- float64 from an inverse taken in double, a CPU tensor, a batch of
        matrices -- would be read as 16 floats of something else; the reference's own matmul raises a RuntimeError for a dtype or
        device mismatch (/root/reference/utils/slam_helpers.py:196-213), and so does this, before anything is launched.
        Attribute reads only; a non-contiguous view is made contiguous."""
        w2c = curr_data['w2c']
        if not (isinstance(w2c, torch.Tensor) and w2c.dtype == torch.float32 and w2c.device == self.dev and tuple(w2c.shape) == (4, 4)):
            got = f"{w2c.dtype}, {tuple(w2c.shape)}, {w2c.device}" if isinstance(w2c, torch.Tensor) else type(w2c).__name__
            raise RuntimeError(f"curr_data['w2c'] must be a float32 tensor of shape [4, 4] on {self.dev} (got {got})")
        if not w2c.is_contiguous():
            w2c = w2c.contiguous()
        fr = _capi.SplatFrameData()
        fr.w2c, fr.time_idx = w2c.data_ptr(), int(time_idx)
        if images:
            im, depth = curr_data['im'], curr_data['depth']
            if not (im.is_contiguous() and depth.is_contiguous()):
                im, depth = im.contiguous(), depth.contiguous()
            fr.im, fr.depth = im.data_ptr(), depth.data_ptr()
            self._frame_keep = (im, depth, w2c)
        else:
            self._frame_keep = (w2c,)
        return fr

    def _whole_frame_workspace(self, time_idx):
        """The workspace of a forward-only render of the whole frame (its list statistics are the frame's) in view ``time_idx``'s order."""
        self._camera._tile_rows, self._camera._stats_partial = None, False
        self._select_order(int(time_idx))
        ws = self._workspace(False, with_ssim=False)
        ws.max_2D_radius = None
        return ws

    def render(self, curr_data, time_idx):
        """Forward-only 6-channel render of the map from pose ``time_idx`` (no loss, no gradients): returns
        ``rendered()``.  The render of add_new_gaussians (/root/reference/scripts/splatam.py:381-385)."""
        self._check_cam(curr_data)
        fr = self._frame(curr_data, time_idx, images=False)
        ws = self._whole_frame_workspace(time_idx)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_render(C.byref(self._camera.struct), C.byref(m), C.byref(fr), C.byref(ws), self._stream()),
                        "splat_iter_render")
        return self.rendered()

    # ------------------------------------------------------------------ evaluation (csrc/evalmetrics.hip; nothing is read here)
    def evaluate_frame(self, curr_data, time_idx, out_row, sil_thres, sil_mask=False, ms_ssim=True, lpips=None):
        """Render the map from pose ``time_idx`` and write the frame's metrics against ``curr_data['im']`` / ``['depth']`` into
        ``out_row`` (8 float64 on the device: psnr, depth_rmse, depth_l1, ms_ssim -- NaN when off --, valid count, != 0 when the
        render ran on truncated lists, the hole count (0 here: ``evaluate_view`` counts), LPIPS (0 without ``lpips``); include/splat_hip.h SPLAT_EVAL_*).  Enqueues only: rows are read by the caller, as a
        table, when it pleases.  The planes stay in ``rendered()``.  ``lpips``: an ``lpips.Lpips`` on this device -- the frame's LPIPS
        goes into slot SPLAT_EVAL_LPIPS (``evaluate_lpips`` on the planes the render left); None: the slot stays 0, nothing more is launched."""
        self._check_cam(curr_data)
        _check_eval_row(out_row, self.dev)
        cam = self._camera
        _check_eval_frame(curr_data, cam.H, cam.W, self.dev)
        fr = self._frame(curr_data, time_idx)
        ews, _ = eval_workspace(self.dev, cam.W, cam.H, ms_ssim)
        cfg = _eval_config(sil_thres, sil_mask, ms_ssim)
        ws = self._whole_frame_workspace(time_idx)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_eval(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(cfg), C.byref(ws), C.byref(ews),
                                               out_row.data_ptr(), self._stream()), "splat_iter_eval")
        if lpips is not None:
            o = self.buf['out6']
            evaluate_lpips(lpips, o[0:3], o[4], curr_data, out_row, sil_thres, sil_mask=sil_mask)      # (after the finish kernel, which leaves 0 there)

    def evaluate_metrics(self, rgb, depth, sil, curr_data, out_row, sil_thres, sil_mask=False, ms_ssim=True, holes=False):
        """``evaluate_metrics`` of this module (the metric kernels alone, on caller-supplied planes of any size)."""
        return evaluate_metrics(rgb, depth, sil, curr_data, out_row, sil_thres, sil_mask=sil_mask, ms_ssim=ms_ssim, holes=holes)

    def evaluate_view(self, view, w2c, curr_data, out_row, sil_thres, sil_mask=False, ms_ssim=True, holes=True, intrinsics=None, lpips=None):
        """A held-out frame scored at ITS pose (the per-frame part of the reference's eval_nvs()): ``render_view(view, w2c=w2c,
        rgb8=False)`` -- the view camera moves to ``w2c`` (float32 [4, 4] on the device: the frame's effective world-to-camera), the
        unchanged splat_iter_render composites the map there -- followed by ``evaluate_metrics`` of the view's planes against
        ``curr_data['im']`` / ``['depth']`` (of the view's size) into ``out_row``, with the hole count (``holes``) in slot
        SPLAT_EVAL_HOLES and the view's truncation status in slot SPLAT_EVAL_FLAGGED.  ``intrinsics``: the view's (default
        ``curr_data['intrinsics']``, which must then be on the host).  Nothing is read on the host and nothing is allocated after the
        view's first call; the current camera, the map, its Adam state and ``variables`` stay untouched (``render_view``).  Returns the
        ``ViewImage`` (its ``out6`` holds the planes the row was formed from).  ``lpips``: as in ``evaluate_frame``."""
        _check_eval_row(out_row, self.dev)
        _check_eval_frame(curr_data, view.H, view.W, self.dev)
        img = self.render_view(view, w2c=w2c, intrinsics=curr_data['intrinsics'] if intrinsics is None else intrinsics, rgb8=False)
        o = img.out6
        evaluate_metrics(o[0:3], o[3], o[4], curr_data, out_row, sil_thres, sil_mask=sil_mask, ms_ssim=ms_ssim, holes=holes)
        out_row[_capi.SPLAT_EVAL_FLAGGED:_capi.SPLAT_EVAL_FLAGGED + 1].copy_(img.truncated)     # (after the finish kernel, which leaves 0 there)
        if lpips is not None:
            evaluate_lpips(lpips, o[0:3], o[4], curr_data, out_row, sil_thres, sil_mask=sil_mask)
        return img

    def lists_known(self, curr_data=None):
        """The per-tile list statistics (bucket stride, longest list) are usable for the map as it is: an edit kept them (_set_rows).
        They are a camera's own: of the camera of ``curr_data`` (which becomes the current one), or of the current camera."""
        if curr_data is not None:
            self._check_cam(curr_data)
        return self._camera.tile_stride > 0 and self._camera.max_list_hint > 0

    def relearn_lists(self, curr_data, time_idx, view=None, w2c=None, intrinsics=None):
        """One probe render with exact lists + ``check_overflow()``: sizes the list capacity and the per-tile buckets
        for the map as it is now (call after an edit that did not keep them -- ``lists_known()``; one D2H read).
        Of the camera of ``curr_data`` -- or, with ``view`` (a ``view_camera``), of that view at pose ``w2c`` (``render_view`` with
        ``intrinsics``, default ``curr_data['intrinsics']``, and ``view.check_overflow()``; ``time_idx`` is then not read)."""
        if view is not None:
            view.camera.tile_stride, view.camera.max_list_hint = 0, 0
            k = curr_data['intrinsics'] if intrinsics is None else intrinsics
            return fit_lists(lambda: self.render_view(view, w2c=w2c, intrinsics=k, rgb8=False), view.check_overflow, "per-tile lists could not be sized")
        self._check_cam(curr_data)
        self._camera.tile_stride, self._camera.max_list_hint = 0, 0
        fit_lists(lambda: self.render(curr_data, time_idx), self.check_overflow, "per-tile lists could not be sized")

    def _append(self, mode, curr_data, time_idx, sil_thres, w2c=None):
        if not self.managed:
            raise RuntimeError("this FusedEngine was built without gaussian_capacity: the map cannot grow")
        self._check_cam(curr_data)          # the frame's camera: its size, its render (out6), its scratch plane
        cam = self._camera
        H, W = cam.H, cam.W
        im, depth = curr_data['im'].contiguous(), curr_data['depth'].contiguous()
        if tuple(im.shape) != (3, H, W) or tuple(depth.shape) != (1, H, W):
            raise RuntimeError("frame size differs from the engine's camera")
        k = curr_data['intrinsics']
        fx, fy, cx, cy = float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2])
        a = _capi.SplatAddArgs()
        a.mode, a.width, a.height = mode, W, H
        a.im, a.depth = im.data_ptr(), depth.data_ptr()
        a.out6 = cam.buf['out6'].data_ptr() if mode == _capi.SPLAT_ADD_NON_PRESENCE else None
        a.fx, a.fy, a.cx, a.cy, a.sil_thres, a.time_idx = fx, fy, cx, cy, float(sil_thres), int(time_idx)
        keep = (im, depth)
        if w2c is not None:
            w2c = w2c.to(device=self.dev, dtype=torch.float32).contiguous()
            a.w2c = w2c.data_ptr()
            keep += (w2c,)
        a.err = cam.buf['ssim_maps'].data_ptr()
        a.scratch = self._map_scratch(max(H * W, self.Pcap)).data_ptr()
        while True:
            st = self._store_struct(with_moments=True)
            with torch.cuda.device(self.dev):
                _capi.check(self.L.splat_map_add_new_gaussians(C.byref(st), C.byref(a), self._stream()), "splat_map_add_new_gaussians")
            counts = self.map_buf['counts'].tolist()        # the one host sync of the edit
            if not counts[2]:
                break
            self._grow_rows(int((self.P + counts[1]) * 1.5) + 1024)
            a.scratch = self._map_scratch(max(H * W, self.Pcap)).data_ptr()
        added = counts[0] - self.P
        if added or counts[3]:
            self._set_rows(counts[0])
        return added

    def add_new_gaussians(self, curr_data, sil_thres, time_idx, mean_sq_dist_method="projective", gaussian_distribution=None,
                          depth_sil=None):
        """/root/reference/scripts/splatam.py:378-420 on the device, in place: render at the tracked pose, select the
        pixels the map does not explain, append one Gaussian per selected pixel (pixel order).  Returns the number added.
        ``depth_sil`` ([>=2,H,W]: depth, silhouette) replaces the render (tests)."""
        if mean_sq_dist_method != "projective":
            raise ValueError(f"Unknown mean_sq_dist_method {mean_sq_dist_method}")
        if gaussian_distribution is not None and (gaussian_distribution == "isotropic") != self.iso:
            raise ValueError("gaussian_distribution differs from the map's log_scales layout")
        self._check_cam(curr_data)
        if depth_sil is None:
            # the densification render must come from complete, sorted lists: a spilled bucket / stale list-length hint would
            # permanently add wrong Gaussians (the status words are overwritten by the next relearn_lists)
            fit_lists(lambda: self.render(curr_data, time_idx), self.check_overflow,
                      "add_new_gaussians: the per-tile lists could not be sized for the densification render")
        else:
            out6 = self._camera.buf['out6']
            out6[3], out6[4] = depth_sil[0], depth_sil[1]
        return self._append(_capi.SPLAT_ADD_NON_PRESENCE, curr_data, time_idx, sil_thres)

    def add_valid_depth_points(self, color, depth, intrinsics, w2c, time_idx=0, cam=None):
        """get_pointcloud(mask = depth > 0) + initialize_params' Gaussian rows (/root/reference/scripts/splatam.py:197-206):
        one Gaussian per valid-depth pixel of the frame, appended to the map.  ``cam``: the frame's camera when it is not the
        current one (a densification frame of its own size: /root/reference/scripts/splatam.py:185-200)."""
        data = {'im': color, 'depth': depth, 'intrinsics': intrinsics}
        if cam is not None:
            data['cam'] = cam
        return self._append(_capi.SPLAT_ADD_VALID_DEPTH, data, time_idx, 0.0, w2c=w2c)

    def remove_points(self, to_remove=None, removal_opacity_threshold=0.0, big_scale=None):
        """remove_points (/root/reference/utils/slam_external.py:139-162): stable in-place compaction of parameters,
        Adam moments and per-Gaussian variables.  ``to_remove``: bool[P], or None to form the flags on the device from
        prune_gaussians' two rules.  Returns the number removed."""
        if not self.managed:
            raise RuntimeError("this FusedEngine was built without gaussian_capacity: rows cannot be removed")
        if self.P == 0:
            return 0
        a = _capi.SplatPruneArgs()
        a.removal_opacity_threshold = float(removal_opacity_threshold)
        a.remove_big, a.big_scale = int(big_scale is not None), float(big_scale or 0.0)
        keep = None
        if to_remove is not None:
            keep = to_remove.to(device=self.dev, dtype=torch.uint8).contiguous()
            a.to_remove = keep.data_ptr()
        st = self._store_struct(with_moments=True)
        need = ((self.Pcap + 3) // 4 * 4) * int(self.L.splat_map_row_floats(C.byref(st)))
        stage = self.map_buf.get('stage')
        if stage is None or stage.numel() < need:
            stage = self.map_buf['stage'] = torch.empty(need, dtype=torch.float32, device=self.dev)
        a.flags, a.stage = self._flags().data_ptr(), stage.data_ptr()
        a.scratch = self._map_scratch(max(self.H * self.W, self.Pcap)).data_ptr()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_map_prune(C.byref(st), C.byref(a), self._stream()), "splat_map_prune")
        counts = self.map_buf['counts'].tolist()
        if counts[1]:
            self._set_rows(counts[0])
        return counts[1]

    def prune_gaussians(self, iter, prune_dict, scene_radius):
        """prune_gaussians (/root/reference/utils/slam_external.py:169-196) on the schedule of ``prune_dict``."""
        sched = slam.edit_schedule(iter, prune_dict, 'prune_every')
        removed = 0
        if sched.edits:
            # 0.1 * variables['scene_radius'] as the reference forms it (a float32 tensor product when given a tensor)
            removed = self.remove_points(None, sched.opacity_threshold, float(0.1 * scene_radius) if sched.remove_big else None)
        if sched.resets:
            with torch.no_grad():
                self._reset_opacities()
        return removed

    def _reset_opacities(self):
        """The reference's opacity reset re-creates the parameter through update_params_and_optimizer
        (/root/reference/utils/slam_external.py:186-190, :236-240): value inverse_sigmoid(0.01), fresh Adam state and NO .grad, so
        the optimizer.step() of that iteration leaves logit_opacities alone.  Same here: moments and this iteration's gradient are
        zeroed (adam_map skips elements whose gradient and both moments are zero)."""
        self.params['logit_opacities'].fill_(math.log(0.01 / (1 - 0.01)))
        self.exp_avg['logit_opacities'].zero_()
        self.exp_avg_sq['logit_opacities'].zero_()
        self.grads['logit_opacities'].zero_()

    # ------------------------------------------------------------------ gradient-based densification
    def accumulate_mean2d_gradient(self, want_grad=False):
        """accumulate_mean2d_gradient (/root/reference/utils/slam_external.py:100-104) for the iteration whose ``loss_backward``
        has just run: variables['means2D_gradient_accum'][seen] += |colour pass' dL/dmeans2D.xy|, variables['denom'][seen] += 1.
        The fused backward sums the RGB and the depth render together, so the colour pass' own screen-space gradient takes one
        more backward composite over the three colour planes (splat_iter_means2d_accumulate).  ``want_grad``: also return that
        gradient ([P, 2], the first two columns of the reference's variables['means2D'].grad)."""
        if not self.managed:
            raise RuntimeError("this FusedEngine was built without gaussian_capacity / variables: there is nothing to accumulate into")
        out = torch.empty(self.P, 2, dtype=torch.float32, device=self.dev) if want_grad else None
        ws = self._workspace(False, with_ssim=False)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_means2d_accumulate(C.byref(self._camera.struct), C.byref(m), C.byref(ws),
                                                             self.store['means2D_gradient_accum'].data_ptr(), self.store['denom'].data_ptr(),
                                                             out.data_ptr() if out is not None and self.P else None, self._stream()),
                        "splat_iter_means2d_accumulate")
        return out

    def means2d_gradient(self):
        """The colour pass' screen-space gradient of the iteration whose ``loss_backward`` has just run (planes kept: every mapping
        iteration, tracking with ``keep_planes``): [P, 2], the first two columns of the reference's ``variables['means2D'].grad``
        (/root/reference/scripts/splatam.py:248-250).  One more backward composite over the three colour planes; nothing is
        accumulated (the caller's own accumulate_mean2d_gradient statement does that)."""
        out = torch.zeros(self.P, 2, dtype=torch.float32, device=self.dev)
        if self.P == 0:
            return out
        ws = self._workspace(False, with_ssim=False)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_means2d_accumulate(C.byref(self._camera.struct), C.byref(m), C.byref(ws), None, None, out.data_ptr(),
                                                             self._stream()), "splat_iter_means2d_accumulate")
        return out

    def _densify_args(self, mode, thr, small, rows_with_grad, n=1, samples=None):
        a = _capi.SplatDensifyArgs()
        a.mode, a.grad_thresh, a.small_scale = mode, float(thr), float(small)
        a.rows_with_grad, a.num_to_split_into = int(rows_with_grad), int(n)
        a.samples = samples.data_ptr() if samples is not None and samples.numel() else None
        a.flags = self._flags().data_ptr()
        a.scratch = self._map_scratch(max(self.H * self.W, self.Pcap)).data_ptr()
        return a

    def _select_and_append(self, mode, thr, small, rows_with_grad, n=1):
        """One clone / split step: select on the device, (split: draw the samples with torch's generator, as the reference does),
        append.  Returns the number of selected rows."""
        while True:
            a = self._densify_args(mode, thr, small, rows_with_grad, n)
            st = self._store_struct(with_moments=True)
            with torch.cuda.device(self.dev):
                _capi.check(self.L.splat_map_densify_select(C.byref(st), C.byref(a), self._stream()), "splat_map_densify_select")
            counts = self.map_buf['counts'].tolist()        # host sync (the reference synchronises on its boolean indexing here)
            if not counts[2]:
                break
            self._grow_rows(int((self.P + counts[1] * n) * 1.5) + 1024)
        S = counts[1]
        if S == 0:
            return 0
        samples = None
        if mode == _capi.SPLAT_DENSIFY_SPLIT:
            sel = self.map_buf['flags'][:self.P].bool()
            ls = self.store['log_scales'][:self.P]
            stds = torch.exp(ls)[sel].repeat(n, 3) if self.iso else torch.exp(ls)[sel].repeat(n, 1)
            # (the reference's repeat(n, 3) of an [S, 3] anisotropic scale would be [S n, 9]: its densify only works for isotropic maps)
            samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=self.dev), std=stds).contiguous()
        a = self._densify_args(mode, thr, small, rows_with_grad, n, samples)
        st = self._store_struct(with_moments=True)
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_map_duplicate(C.byref(st), C.byref(a), self._stream()), "splat_map_duplicate")
        self._set_rows(counts[0])
        return S

    def densify(self, iter, densify_dict, scene_radius, accumulate=True):
        """densify (/root/reference/utils/slam_external.py:191-240) on the device, in place, called where the reference calls it
        (between backward() and optimizer.step()): accumulate the screen-space gradient; on the schedule clone the small /
        split the large Gaussians whose mean gradient reaches ``grad_thresh``, reset the three per-Gaussian variables, remove
        the split originals, prune by opacity / size; optional opacity reset.  Returns True when the number of rows changed."""
        sched = slam.edit_schedule(iter, densify_dict, 'densify_every')
        if not sched.active:
            return False
        if accumulate:
            # re-runs the RGB backward composite over THIS iteration's workspace (lists, radii, feat8 indexed by the rows the
            # render saw): a caller that removes rows between loss_backward() and densify() must accumulate BEFORE it does
            # (accumulate_mean2d_gradient(), then densify(..., accumulate=False)) -- pipeline._map_frame does
            self.accumulate_mean2d_gradient()
        changed = False
        if sched.edits:
            thr, small = densify_dict['grad_thresh'], float(0.01 * scene_radius)
            P0 = self.P
            self._select_and_append(_capi.SPLAT_DENSIFY_CLONE, thr, small, P0)
            n = int(densify_dict['num_to_split_into'])
            P1 = self.P
            S = self._select_and_append(_capi.SPLAT_DENSIFY_SPLIT, thr, small, P0, n)
            for k in ('means2D_gradient_accum', 'denom', 'max_2D_radius'):
                self.store[k][:self.P].zero_()
            if S:
                to_remove = torch.zeros(self.P, dtype=torch.uint8, device=self.dev)
                to_remove[:P1] = self.map_buf['flags'][:P1]
                self.remove_points(to_remove)
            self.remove_points(None, sched.opacity_threshold, float(0.1 * scene_radius) if sched.remove_big else None)
            changed = True
        if sched.resets:
            with torch.no_grad():
                self._reset_opacities()
        return changed

    # ------------------------------------------------------------------ views (csrc/view.hip; nothing of the map or the loop is written)
    def view_camera(self, width, height, capacity=None):
        """A camera for LOOKING at the map: created once, moved in place by every ``render_view`` (``ViewCamera``).  It owns planes, lists
        and list statistics of its own, like a camera of ``add_camera``, but the engine does not count it (``num_cameras``) and never
        makes it the current one.  ``capacity``: (Gaussian, tile) instances its lists hold (default as at construction)."""
        return ViewCamera(self, int(width), int(height), capacity)

    def _rows_at(self, view, t):
        """Rows of the map with ``timestep <= t``: a PREFIX of the rows, because rows are appended in time order and compacted stably.
        Checked once per map version (one host read), and refused otherwise: gradient-based densification clones rows, and such a map
        would be rendered wrongly from a prefix.  One more small host read per distinct ``t`` and version."""
        ts = None if self.variables is None else self.variables.get('timestep')
        if ts is None:
            raise RuntimeError("render_view(max_timestep=...): this FusedEngine was built without variables['timestep']")
        ts = ts[:self.P]
        key = (self.map_version, self.P, ts.data_ptr() if self.P else 0)
        if view._replay_key != key:
            if self.P > 1 and not bool((ts[1:] >= ts[:-1]).all()):
                raise RuntimeError("render_view(max_timestep=...): variables['timestep'] is not non-decreasing along the rows (gradient-based "
                                   "densification clones rows): the Gaussians up to a time step are not a prefix of the map")
            view._replay_key, view._replay_rows = key, {}
        t = float(t)
        rows = view._replay_rows.get(t)
        if rows is None:
            rows = int(torch.searchsorted(ts.contiguous(), torch.tensor([t], dtype=ts.dtype, device=ts.device), right=True)) if self.P else 0
            view._replay_rows[t] = rows
        return rows

    def render_view(self, view, w2c=None, time_idx=None, intrinsics=None, mode="color", background=(0.0, 0.0, 0.0), depth_range=(0.0, 6.0),
                    lut=None, max_timestep=None, points=False, offset=None, near=0.01, far=100, first_w2c=None, rgb8=True, point_size=1,
                    overlay=None, overlay_upto=None, frusta="all", line_width=1, occlude=True, overlay_planes=False):
        """The map from any pose, as display bytes (and a point cloud): three launches on the current stream -- splat_view_camera moves
        ``view`` to the pose, splat_iter_render composites the map's own Gaussian arrays at it, splat_view_finish turns the six planes
        into ``rgb8`` [H, W, 3] uint8 (``mode`` "color" on ``background``, "depth" through ``lut`` over ``depth_range``, "sil": grey
        1 - silhouette) and, with ``points``, ``points`` / ``colors`` [H W, 3] float32 (the reference's rgbd2pcd).  Nothing is read on the
        host.  Returns a ``ViewImage`` of tensors the VIEW keeps: the next call on it overwrites them.

        The pose: ``w2c`` (float32 [4, 4] on the device, rigid), or ``time_idx``: the map's pose of that frame,
        ``first_w2c . rel_w2c[time_idx]`` (``first_w2c``: float32 [4, 4] on the device, default the identity); ``offset`` (a 4 x 4 on
        the host) is multiplied from the left.  ``intrinsics``: a 3 x 3 (or 4 x 4) matrix or ``(fx, fy, cx, cy)`` on the host, for the
        view's size; a zoom is another matrix, not another view.  ``lut``: [256, 3] uint8 on the device (default: ``view.jet_lut``).
        ``max_timestep = t``: only the Gaussians with ``timestep <= t`` (the reference's online replay), see ``_rows_at``.

        Nothing is allocated after the view's first call, whatever the pose, mode or zoom, with two exceptions a caller chooses:
        ``points`` asked for the first time allocates the two cloud arrays then, and the first render after a
        ``view.check_overflow()`` that learnt or changed the bucket stride lays out the view's group records (and the digest itself may
        grow the lists).  ``w2c`` / ``first_w2c`` must be contiguous (nothing is copied per call).  The current camera, its
        ``rendered()``, list statistics and tile orders are left as they were; the render writes nothing into the map, its Adam moments
        or ``variables`` (not ``max_2D_radius`` either).  The per-Gaussian scratch (``radii``, ``xy``, ...) IS shared with the loop:
        a view render belongs BETWEEN iterations, not between an iteration and the read of its ``seen`` or its
        ``accumulate_mean2d_gradient``.  The DIGEST of a flagged view (``view.check_overflow()``) does touch one array of the map's:
        like every digest it zeroes the backward accumulator (``accum``), which is zero between iterations anyway -- so it, too,
        belongs between iterations, never between ``loss_backward`` and the step that reads the accumulator.

        Lists that did not fit do not stop the call: the picture is then incomplete and ``truncated`` (a device int32, != 0) says so,
        from the view camera's status.  ``view.check_overflow()`` is the digest for that camera (grows the lists, learns the buckets):
        call it where the image is read anyway, then render again.

        The overlay (csrc/viewoverlay.hip): ``mode="centers"`` is the viewers' render mode of that name -- no composite; every Gaussian's
        centre (of the rows ``max_timestep`` selects) as a square of ``point_size`` (1..8) pixels in the Gaussian's colour on
        ``background``, the nearest centre winning each pixel.  ``overlay``: a ``view.RunOverlay`` -- the run's cameras drawn into the
        picture of any mode as line segments ``line_width`` (1..4) pixels wide: the trajectory up to time step ``overlay_upto``
        (default: the whole run) and, with ``frusta="all"``, every camera frustum up to it, with ``"current"`` that step's alone,
        with ``None`` none; the overlay's ground-truth polyline, if it has one, up to the same step.  Segments (and centres) are
        depth-tested among themselves and, unless ``occlude=False``, against the picture's depth plane (``out6[3]``: the cloud the
        reference's viewers test against; in ``centers`` mode there is none).  ``overlay_planes=True`` adds ``key`` to the result: the
        key plane as int64 [H, W] (include/splat_hip.h; -1 where nothing was drawn).  The view allocates that plane at its first call
        with an overlay or in ``centers`` mode, and nothing after it; the launches are the clear, one per kind of primitive and
        the resolve behind splat_view_finish.  An overlay without segments to draw leaves ``rgb8`` as the call without one gives it."""
        if (w2c is None) == (time_idx is None):
            raise ValueError("render_view takes a w2c or a time_idx")
        if view.engine is not self:
            raise RuntimeError("this view camera belongs to another FusedEngine")
        if intrinsics is None:
            raise ValueError("render_view needs the view's intrinsics")
        centers = mode == "centers"
        try:
            view_mode = {"color": _capi.SPLAT_VIEW_COLOR, "depth": _capi.SPLAT_VIEW_DEPTH, "sil": _capi.SPLAT_VIEW_SILHOUETTE,
                         "silhouette": _capi.SPLAT_VIEW_SILHOUETTE, "centers": _capi.SPLAT_VIEW_COLOR}[mode]
        except KeyError:
            raise ValueError(f"mode must be 'color', 'depth', 'sil' or 'centers' (got {mode!r})") from None
        ranges = ()
        if centers or overlay is not None or overlay_planes:
            if not rgb8 or (centers and points):
                raise ValueError("an overlay is drawn into rgb8; the centers picture has no point cloud")
            if not 1 <= int(point_size) <= _capi.SPLAT_VIEW_MAX_POINT_SIZE or not 1 <= int(line_width) <= _capi.SPLAT_VIEW_MAX_LINE_WIDTH:
                raise ValueError(f"point_size is 1..{_capi.SPLAT_VIEW_MAX_POINT_SIZE}, line_width 1..{_capi.SPLAT_VIEW_MAX_LINE_WIDTH}")
            if overlay is not None:
                if overlay.dev != self.dev:
                    raise RuntimeError(f"the overlay's arrays are on {overlay.dev}, the engine on {self.dev}")
                ranges = overlay.ranges(overlay_upto, frusta)                      # (may raise: before anything is launched)
        fx, fy, cx, cy = _intrinsics4(intrinsics)
        a = view.args
        a.fx, a.fy, a.cx, a.cy, a.near_z, a.far_z = fx, fy, cx, cy, float(near), float(far)
        keep = []
        if w2c is not None:
            a.w2c_in = _device_mat4(w2c, "w2c", self.dev, keep).data_ptr()
        else:
            time_idx = int(time_idx)
            if not 0 <= time_idx < self.num_frames:
                raise ValueError(f"time_idx {time_idx} is outside the map's {self.num_frames} frames")
            rots, trans = self.params['cam_unnorm_rots'], self.params['cam_trans']
            a.w2c_in = None
            a.cam_unnorm_rots, a.cam_trans, a.num_frames, a.time_idx = rots.data_ptr(), trans.data_ptr(), self.num_frames, time_idx
            a.first_w2c = (view.identity if first_w2c is None else _device_mat4(first_w2c, "first_w2c", self.dev, keep)).data_ptr()
        if offset is None:
            a.offset = None
        else:
            flat = [float(x) for row in (offset.tolist() if hasattr(offset, "tolist") else offset) for x in row]
            if len(flat) != 16:
                raise ValueError("offset must be a 4 x 4 matrix on the host")
            view._offset[:] = flat
            a.offset = view._offset
        P = self.P if max_timestep is None else self._rows_at(view, max_timestep)          # (may raise: before anything is launched)
        a.mode = view_mode
        a.bg[:] = [float(c) for c in background]
        a.vmin, a.vmax = float(depth_range[0]), float(depth_range[1])
        if view_mode == _capi.SPLAT_VIEW_DEPTH and rgb8:
            if lut is None:
                lut = view.default_lut()
            elif not (isinstance(lut, torch.Tensor) and lut.dtype == torch.uint8 and lut.device == self.dev and tuple(lut.shape) == (256, 3)
                      and lut.is_contiguous()):
                raise RuntimeError(f"lut must be a contiguous uint8 tensor of shape [256, 3] on {self.dev}")
            a.lut = lut.data_ptr()
            keep.append(lut)
        cam = view.camera
        a.out6 = cam.buf['out6'].data_ptr()
        a.rgb8 = view.rgb8.data_ptr() if rgb8 else None
        if points:
            view.alloc_cloud()
        a.points, a.colors = (view.points.data_ptr(), view.colors.data_ptr()) if points else (None, None)
        cam.struct.tanfovx, cam.struct.tanfovy = view.W / (2.0 * fx), view.H / (2.0 * fy)
        cam.keep_lists(P, 0.10, only_bucketed=True)         # (statistics learnt on another map: exact lists again)
        current = self._camera
        self._use(cam)
        try:
            ws = self._whole_frame_workspace(0)             # (forward only, max_2D_radius = None: FusedEngine.render's)
            m = self._map_struct()
            m.P = P
            m.cam_unnorm_rots, m.cam_trans, m.num_frames = view.pose_rot.data_ptr(), view.pose_trans.data_ptr(), 1
            fr = _capi.SplatFrameData()
            fr.w2c, fr.time_idx = view.w2c.data_ptr(), 0
            with torch.cuda.device(self.dev):
                stream = self._stream()
                _capi.check(self.L.splat_view_camera(C.byref(a), stream), "splat_view_camera")
                if centers:                                  # (no composite: nothing of the lists is used, nothing can be truncated)
                    view.truncated.zero_()
                else:
                    _capi.check(self.L.splat_iter_render(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(ws), stream), "splat_iter_render")
                    _capi.check(self.L.splat_view_finish(C.byref(a), stream), "splat_view_finish")
                    status = cam.buf['status']
                    torch.bitwise_or(status[_STATUS_OVERFLOW:_STATUS_OVERFLOW + 1], status[_STATUS_STALE_HINT:_STATUS_STALE_HINT + 1], out=view.truncated)
                if centers or overlay is not None or overlay_planes:
                    ov = view.overlay_args()
                    ov.fx, ov.fy, ov.cx, ov.cy, ov.near_z = fx, fy, cx, cy, float(near)
                    _capi.check(self.L.splat_view_overlay_clear(C.byref(ov), stream), "splat_view_overlay_clear")
                    if centers and P > 0:
                        _capi.check(self.L.splat_view_points(C.byref(ov), self.params['means3D'].data_ptr(), P, int(point_size), stream), "splat_view_points")
                    for first, count in ranges:
                        _capi.check(self.L.splat_view_segments(C.byref(ov), overlay.segments.data_ptr(), first, count, int(line_width), stream),
                                    "splat_view_segments")
                    f = _capi.SplatViewOverlayFinish()
                    f.depth = None if centers else cam.buf['out6'][3].data_ptr()
                    f.occlude, f.fill = int(bool(occlude)), int(centers)
                    if centers and P > 0:
                        f.rgb_colors, f.num_rows = self.params['rgb_colors'].data_ptr(), P
                    if overlay is not None:
                        f.segment_colors, f.num_segments = overlay.colors.data_ptr(), overlay.num_segments
                        keep.append(overlay)
                    f.bg[:] = a.bg[:]
                    f.rgb8 = view.rgb8.data_ptr()
                    _capi.check(self.L.splat_view_overlay_finish(C.byref(ov), C.byref(f), stream), "splat_view_overlay_finish")
        finally:
            self._use(current)
        view._keep = keep
        if not centers:
            view._rendered_P = P
        o = cam.buf['out6']
        return ViewImage(view.rgb8 if rgb8 else None, view.points if points else None, view.colors if points else None, view.truncated, o,
                         view.keys if overlay_planes else None)

    # ------------------------------------------------------------------ plumbing
    def _alloc_lists(self, capacity):
        self._camera.alloc_lists(capacity, self.use_recs)

    def _check_cam(self, curr_data):
        """The camera is the one of ``curr_data['cam']``, as the reference's get_loss reads it on every call
        (/root/reference/scripts/splatam.py:249): a settings tuple that equals a camera of this engine selects it.  One the engine does
        not know is registered on first use with ``auto_cameras``; otherwise it is an error, not a silently ignored argument."""
        cam = curr_data.get('cam') if hasattr(curr_data, 'get') else None
        if cam is None or cam is self._camera.settings:
            return
        if self._find_camera(cam) is None and not self.auto_cameras:
            raise RuntimeError("curr_data['cam'] differs from the camera(s) this FusedEngine was built for "
                               "(add_camera(cam) registers another one; auto_cameras = True does so on first use)")
        self.add_camera(cam)

    def _map_struct(self):
        p = self.params
        if self.managed:          # the backing arrays (a zero-row view has no data pointer)
            p = dict(self.store, cam_unnorm_rots=p['cam_unnorm_rots'], cam_trans=p['cam_trans'])
        m = _capi.SplatMap()
        m.P, m.isotropic = self.P, int(self.iso)
        m.means3D, m.rgb_colors = p['means3D'].data_ptr(), p['rgb_colors'].data_ptr()
        m.unnorm_rotations, m.logit_opacities = p['unnorm_rotations'].data_ptr(), p['logit_opacities'].data_ptr()
        m.log_scales = p['log_scales'].data_ptr()
        m.cam_unnorm_rots, m.cam_trans = p['cam_unnorm_rots'].data_ptr(), p['cam_trans'].data_ptr()
        m.num_frames = self.num_frames
        return m

    def _workspace(self, with_map_grads, with_ssim):
        cam = self._camera
        b, rows, hint, stride = cam.buf, self.map_buf, cam.max_list_hint, cam.tile_stride
        ws = _capi.SplatIterWorkspace()
        st = ws.st
        st.depth, st.xy, st.conic_opacity, st.rect = rows['depth'].data_ptr(), rows['xy'].data_ptr(), rows['conic'].data_ptr(), rows['rect'].data_ptr()
        st.radii = rows['radii'].data_ptr()
        st.tile_count, st.tile_base, st.tile_cursor = b['tile_count'].data_ptr(), b['tile_base'].data_ptr(), b['tile_cursor'].data_ptr()
        st.keys, st.point_list, st.capacity = b['keys'].data_ptr(), b['point_list'].data_ptr(), cam.capacity
        st.keys_alt, st.long_base = b['keys_alt'].data_ptr(), b['long_base'].data_ptr()
        # staged records handed from the forward to the backward composite (B-loop, mapping +1.4 %; B: the forward composite's 34 MB of
        # extra stores, mapping -1.4 %).  SPLAT_TILE_RECS=1 / 0 forces them on / off
        recs_on = self.use_recs == 1 or (self.use_recs == 2 and hint > _capi.RECS_MIN_LIST)
        st.tile_recs = b['tile_recs'].data_ptr() if (recs_on and b['tile_recs'] is not None) else None
        st.long_items = b['long_items'].data_ptr()
        st.max_list_hint, st.tile_stride = hint, stride
        st.tile_row_begin, st.tile_row_end = cam._tile_rows or (0, 0)
        st.group_count, st.group_recs, st.group_stride = b['group_count'].data_ptr(), None, 0
        if self.group_bins and stride > 0 and _capi.lists_sorted_by_composite(hint):
            gs = _capi.SPLAT_GROUP_TILES ** 2 * stride
            need = cam.num_groups * gs * 4
            if need <= 1 << 30:                       # (int32 words; 4 GiB of records)
                recs = b.get('group_recs')
                if recs is None or recs.numel() < need:
                    recs = cam.alloc_group_recs(gs)
                st.group_recs, st.group_stride = recs.data_ptr(), gs
        st.order_hint = int(self.creation_order)
        if self.tile_order_on:
            st.tile_work, st.tile_order = b['tile_work'].data_ptr(), b['tile_order'].data_ptr()
        st.sub_bins = cam.sub_bins if stride == 0 else 1
        st.final_T, st.n_contrib, st.status = b['final_T'].data_ptr(), b['n_contrib'].data_ptr(), b['status'].data_ptr()
        ws.feat8, ws.out6, ws.dL_dout6, ws.accum = rows['feat8'].data_ptr(), b['out6'].data_ptr(), b['dL_dout6'].data_ptr(), rows['accum'].data_ptr()
        ws.ssim_maps = b['ssim_maps'].data_ptr() if with_ssim else None
        ws.sums = b['sums'].data_ptr()
        ws.max_2D_radius = self.max_2D_radius.data_ptr() if self.max_2D_radius is not None else None
        if with_map_grads and with_map_grads != "step only":      # ("step only": the fused Adam step takes them from registers, nothing is stored)
            g = self.grads
            ws.d_means3D, ws.d_rgb_colors = g['means3D'].data_ptr(), g['rgb_colors'].data_ptr()
            ws.d_unnorm_rotations, ws.d_logit_opacities = g['unnorm_rotations'].data_ptr(), g['logit_opacities'].data_ptr()
            ws.d_log_scales = g['log_scales'].data_ptr()
        ws.d_cam = b['d_cam'].data_ptr()
        if 'outlier_err' in b:
            ws.outlier_err, ws.outlier_scratch = b['outlier_err'].data_ptr(), b['outlier_scratch'].data_ptr()
        return ws

    def _select_order(self, view):
        """The current camera composites in the launch order view ``view`` left (_Camera.select_order)."""
        if self.tile_order_on and self.order_per_view:
            self._camera.select_order(view)

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    @staticmethod
    def uses_gs_loss(cfg):
        """``cfg['loss'] == 'gs'``: the iteration forms get_loss_gs (/root/reference/scripts/post_splatam_opt.py:111-147) instead of
        get_loss(mapping=True) -- of ``cfg`` it reads ``loss_weights`` (and ``lrs`` where a step is taken), nothing else."""
        loss = cfg.get('loss', 'splatam')
        if loss not in ('splatam', 'gs'):
            raise ValueError(f"cfg['loss'] must be 'splatam' or 'gs' (got {loss!r})")
        return loss == 'gs'

    @staticmethod
    def loss_config(cfg, tracking, do_ba=False, defer_finish=False, fused_composite=0):
        """The SplatLossConfig of ``cfg``; with ``cfg['loss'] == 'gs'`` a SplatLossConfigEx around it (mapping only)."""
        if FusedEngine.uses_gs_loss(cfg):
            if tracking or do_ba or defer_finish:
                raise ValueError("cfg['loss'] = 'gs' is a mapping loss without pose gradient: not with tracking, do_ba or tile rows")
            ex = _capi.SplatLossConfigEx()
            ex.loss_mode = _capi.SPLAT_LOSS_GS
            c = ex.base
            c.gaussians_grad, c.use_l1 = 1, 1
            c.sil_thres = float(cfg.get('sil_thres', 0.5))
            c.w_im, c.w_depth = float(cfg['loss_weights']['im']), float(cfg['loss_weights']['depth'])
            return ex
        c = _capi.SplatLossConfig()
        c.defer_finish = int(defer_finish)
        c.fused_composite = int(fused_composite)
        c.tracking = int(tracking)
        c.camera_grad = int(tracking or do_ba)
        c.gaussians_grad = int(not tracking)
        c.use_sil_for_loss, c.sil_thres = int(cfg['use_sil_for_loss']), float(cfg['sil_thres'])
        c.use_l1, c.ignore_outlier_depth_loss = int(cfg['use_l1']), int(cfg['ignore_outlier_depth_loss'])
        c.w_im, c.w_depth = float(cfg['loss_weights']['im']), float(cfg['loss_weights']['depth'])
        return c

    # ------------------------------------------------------------------ one iteration
    def loss_backward(self, curr_data, time_idx, cfg, tracking, map_grads=None, do_ba=False, pose_adam=None, map_adam=None,
                      tile_rows=None, keep_planes=None):
        """get_loss + backward.  Afterwards (stream order): ``self.grads`` (mapping) and
        ``self.buf['d_cam']`` = [dL/dq_raw(4), dL/dt_raw(3), loss].  ``pose_adam`` (a SplatPoseAdam): the pose's Adam step
        rides in the last kernel (splat_iter_tracking_step); ``map_adam`` (a SplatAdamMap): likewise the map's
        (splat_iter_mapping_step).  ``keep_planes`` (tracking): the rendered planes / gradient planes (``rendered()``,
        ``buf['dL_dout6']``) are wanted -- default: yes, unless the pose's Adam step rides along (the loop's own iterations); without
        them the tracking iteration's composites run as ONE kernel that keeps its planes in registers (SplatLossConfig.fused_composite)."""
        if map_grads is None:
            map_grads = not tracking
        self._check_cam(curr_data)
        cam = self._camera
        fr = self._frame(curr_data, time_idx)
        if keep_planes is None:
            keep_planes = pose_adam is None
        # (with the map's gradients the one-kernel form carries the backward composite's mapping form at four workgroups per CU: ahead
        #  where a tile's list is one or two batches -- B: +6.4 % --, behind where it is three -- B-loop: -1.2 %; profiles/r06_experiments.md 4)
        full_ok = self.track_fused_full and 0 < cam.max_list_hint <= 400
        one_kernel = (2 if keep_planes else 1) if (tracking and self.track_fused and (not map_grads or full_ok)) else 0
        lc = self.loss_config(cfg, tracking, do_ba, defer_finish=tile_rows is not None, fused_composite=one_kernel)
        cam._tile_rows = tile_rows          # a band: the iteration stops before its last kernel (finish_iteration completes it)
        cam._stats_partial = tile_rows is not None
        self._lc_keep = lc
        gs = isinstance(lc, _capi.SplatLossConfigEx)
        if gs and pose_adam is not None:
            raise ValueError("cfg['loss'] = 'gs' takes no pose step")
        if not gs and lc.ignore_outlier_depth_loss and 'outlier_err' not in cam.buf:
            cam.alloc_outlier_scratch()
        if self.tile_order_on and self.order_per_view:
            cam.select_order(int(time_idx))
        ws = self._workspace(map_grads, with_ssim=not tracking)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            if gs and map_adam is not None:
                _capi.check(self.L.splat_iter_mapping_step_ex(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws),
                                                              C.byref(map_adam), self._stream()), "splat_iter_mapping_step_ex")
            elif gs:
                _capi.check(self.L.splat_iter_loss_backward_ex(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws),
                                                               self._stream()), "splat_iter_loss_backward_ex")
            elif pose_adam is not None:
                _capi.check(self.L.splat_iter_tracking_step(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws),
                                                            C.byref(pose_adam), self._stream()), "splat_iter_tracking_step")
            elif map_adam is not None:
                _capi.check(self.L.splat_iter_mapping_step(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws),
                                                           C.byref(map_adam), self._stream()), "splat_iter_mapping_step")
            else:
                _capi.check(self.L.splat_iter_loss_backward(C.byref(cam.struct), C.byref(m), C.byref(fr), C.byref(lc), C.byref(ws),
                                                            self._stream()), "splat_iter_loss_backward")
        cam._tile_rows = None
        self._fr_keep = fr

    def finish_iteration(self, pose_adam=None):
        """The last kernel of an iteration that ran on a band of tile rows (``loss_backward(..., tile_rows=...)``), after the caller
        has summed ``self.buf['sums']`` over the ranks: pose gradient, loss value and -- with ``pose_adam`` -- the pose's Adam step
        and the best-candidate bookkeeping (splat_iter_finish)."""
        ws = self._workspace(False, with_ssim=False)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_finish(C.byref(self._camera.struct), C.byref(m), C.byref(self._fr_keep), C.byref(self._lc_keep), C.byref(ws),
                                                 C.byref(pose_adam) if pose_adam is not None else None, self._stream()), "splat_iter_finish")

    def tile_row_band(self, rank, world):
        """Rows [begin, end) of the 16-pixel tile grid that rank ``rank`` of ``world`` composites in tile-row-sharded tracking."""
        from .dist import tile_row_band
        return tile_row_band((self.H + 15) // 16, rank, world)

    def _adam_map_args(self, lrs, beta1=0.9, beta2=0.999, eps=1e-15, steps=None):
        """The next step of torch.optim.Adam(param_groups, lr=0.0, eps=1e-15) over the five Gaussian groups
        (/root/reference/scripts/splatam.py:160-166).  Bias corrections in double on the host, as torch forms them; ``steps``:
        the step count of each group AFTER this step (torch counts per parameter: a parameter the caller re-created restarts),
        default: the engine's own count for all five.  The step is gated on the iteration's capacity flag (SPLAT_REPORT_FLAG)."""
        if steps is None:
            self.map_step += 1
            steps = (self.map_step,) * 5
        o = _capi.SplatAdamMap()
        o.beta1, o.beta2, o.eps = beta1, beta2, eps
        o.one_minus_beta1, o.one_minus_beta2 = 1.0 - beta1, 1.0 - beta2        # (in double, as torch forms them)
        for k, name in enumerate(PARAM_ORDER):
            t = max(int(steps[k]), 1)
            o.bc2_sqrt[k] = math.sqrt(1.0 - beta2 ** t)
            o.step_size[k] = lrs[name] / (1.0 - beta1 ** t)
            o.grad[k] = self.grads[name].data_ptr()
            o.exp_avg[k] = self.exp_avg[name].data_ptr()
            o.exp_avg_sq[k] = self.exp_avg_sq[name].data_ptr()
        o.gate = self._camera.buf['d_cam'].data_ptr()
        return o

    def adam_map(self, lrs, beta1=0.9, beta2=0.999, eps=1e-15):
        """optimizer.step() of the mapping optimizer on ``self.grads`` (see _adam_map_args)."""
        o = self._adam_map_args(lrs, beta1, beta2, eps)
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_adam_map(C.byref(m), C.byref(o), self._stream()), "splat_iter_adam_map")

    def reset_map_optimizer(self):
        """The reference re-creates the optimizer for every frame's mapping phase (:821)."""
        for k in PARAM_ORDER:
            self.exp_avg[k].zero_()
            self.exp_avg_sq[k].zero_()
        self.map_step = 0

    def begin_tracking(self, time_idx):
        """Fresh Adam state and best-candidate bookkeeping for one frame (:680-684)."""
        st = self.map_buf['pose_state']
        st.zero_()
        st[14] = 1e20
        st[15:19] = self.params['cam_unnorm_rots'].detach()[0, :, time_idx]
        st[19:22] = self.params['cam_trans'].detach()[0, :, time_idx]
        self.pose_step = 0
        self.track_time_idx = int(time_idx)

    def adam_pose(self, lr_rot, lr_trans, beta1=0.9, beta2=0.999, eps=1e-8):
        self.pose_step += 1
        t = self.pose_step
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        m = self._map_struct()
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_iter_adam_pose(C.byref(m), self.track_time_idx, self._camera.buf['d_cam'].data_ptr(),
                                                    self.map_buf['pose_state'].data_ptr(), beta1, beta2, eps, math.sqrt(bc2),
                                                    lr_rot / bc1, lr_trans / bc1, self._stream()), "splat_iter_adam_pose")

    def end_tracking(self):
        """Copy the best candidate back (:741-744)."""
        st, t = self.map_buf['pose_state'], self.track_time_idx
        with torch.no_grad():
            self.params['cam_unnorm_rots'][0, :, t] = st[15:19]
            self.params['cam_trans'][0, :, t] = st[19:22]

    def _pose_adam_args(self, cfg):
        """The next step of the tracking optimizer (default betas / eps of torch.optim.Adam) as the C ABI takes it."""
        self.pose_step += 1
        t, beta1, beta2 = self.pose_step, 0.9, 0.999
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        pa = _capi.SplatPoseAdam()
        pa.state, pa.beta1, pa.beta2, pa.eps, pa.bc2_sqrt = self.map_buf['pose_state'].data_ptr(), beta1, beta2, 1e-8, math.sqrt(bc2)
        pa.step_size_rot, pa.step_size_trans = cfg['lrs']['cam_unnorm_rots'] / bc1, cfg['lrs']['cam_trans'] / bc1
        return pa

    def tracking_iteration(self, curr_data, cfg, shard=None, allreduce_sums=None):
        """Loop body of /root/reference/scripts/splatam.py:690-711 for frame ``begin_tracking`` named.

        ``shard = (rank, world)``: tile-row-sharded tracking over ``world`` processes holding the same map and pose -- this rank
        composites its band of tile rows only (forward, loss, backward: every term of the loss and of the pose gradient is a sum
        over pixels), ``allreduce_sums`` sums the 16 KB of partial sums over the ranks, and every rank takes the SAME Adam step on
        the pose (no broadcast needed).  Not with ``ignore_outlier_depth_loss`` (its median sees the whole render)."""
        pa = self._pose_adam_args(cfg)
        if shard is None or shard[1] <= 1:
            self.loss_backward(curr_data, self.track_time_idx, cfg, tracking=True, pose_adam=pa)
            return
        if cfg['ignore_outlier_depth_loss']:
            raise RuntimeError("tile-row-sharded tracking needs a pixel-local loss: not with ignore_outlier_depth_loss")
        self.loss_backward(curr_data, self.track_time_idx, cfg, tracking=True, tile_rows=self.tile_row_band(*shard), keep_planes=False)
        sums = self._camera.buf['sums']
        if self.fold_sums:
            # the 64 copies of the partial sums folded into the first (one tiny launch): the exchange carries 256 bytes, not 16 KB
            with torch.cuda.device(self.dev):
                _capi.check(self.L.splat_iter_fold_sums(sums.data_ptr(), self._stream()), "splat_iter_fold_sums")
            allreduce_sums(sums[:_capi.SPLAT_ITER_SUMS])
        else:
            allreduce_sums(sums)
        self.finish_iteration(pa)

    def mapping_iteration(self, iter_data, iter_time_idx, cfg, bucket_allreduce=None, keep_grads=None):
        """Loop body of /root/reference/scripts/splatam.py:828-869 (without pruning / densification).  Without a gradient
        exchange the whole iteration is one C call (the Adam step rides in the last kernel: splat_iter_mapping_step).
        ``keep_grads`` (default ``self.keep_map_grads``): also STORE the gradients the step was taken on (``self.grads``); the
        reference's loop discards them right after the step (optimizer.zero_grad(set_to_none=True), :860-861), and a loop that does
        the same saves 32 - 48 bytes of stores per Gaussian and iteration."""
        if bucket_allreduce is None and self.P <= self.fused_adam_max_rows:
            keep = self.keep_map_grads if keep_grads is None else keep_grads
            self.loss_backward(iter_data, iter_time_idx, cfg, tracking=False, map_adam=self._adam_map_args(cfg['lrs']),
                               map_grads=True if keep else "step only")
            return
        self.loss_backward(iter_data, iter_time_idx, cfg, tracking=False)
        if bucket_allreduce is not None:
            self.exchange_gradients(bucket_allreduce)      # one collective: 8 (isotropic) or 14 floats per Gaussian (+ the flag header)
        self.adam_map(cfg['lrs'])

    def mapping_batch(self, views, cfg, total_views=None, allreduce_sum=None):
        """One mapping step over SEVERAL keyframe views (the view-sharded form of the loop body: BASELINE config 3): the
        gradients of the map over ``views`` = [(iter_data, iter_time_idx), ...] are accumulated in the flat bucket, summed over
        the ranks by ``allreduce_sum`` (one collective on ``reduce_flat``), divided by ``total_views`` (views of ALL ranks) and
        applied by ONE Adam step -- what a single process gets by accumulating the same views."""
        acc = self._acc_flat()
        for i, (data, t) in enumerate(views):
            self.loss_backward(data, t, cfg, tracking=False)
            if i == 0:
                acc.copy_(self.grad_flat)
            else:
                acc.add_(self.grad_flat)
        red = acc[:self.reduce_flat.numel()]
        if allreduce_sum is not None:           # (the capacity flag of any rank's views travels in the header: exchange_gradients)
            self.exchange_gradients(allreduce_sum, self._acc_store[:_FLAG_SLOTS + self.reduce_flat.numel()])
        n = float(total_views if total_views is not None else len(views))
        if n != 1.0:
            red.mul_(1.0 / n)
        self.grad_flat.copy_(acc)
        self.adam_map(cfg['lrs'])

    def exchange_gradients(self, all_reduce, flat=None):
        """The gradient exchange of a multi-rank mapping step: ``all_reduce`` (sum or mean, in place) over the flat gradient bucket WITH
        this rank's capacity flag in its header.  Ranks render different views, so typically only some overflow their lists; the
        flag of ANY rank comes back non-zero on EVERY rank and is made this rank's sticky flag (SPLAT_REPORT_FLAG) before the Adam step
        that follows, so the replicas skip the same steps and stay bit-identical (the reduced gradient of such an iteration holds a
        truncated-list contribution: nobody may step on it).  ``flat``: another buffer laid out like ``_exchange_flat`` (mapping_batch's
        accumulator)."""
        flat = self._exchange_flat if flat is None else flat
        flag = self._camera.buf['d_cam'][_REPORT_FLAG:_REPORT_FLAG + 1]
        flat[0:1].copy_(flag)
        all_reduce(flat)
        torch.maximum(flag, (flat[0:1] != 0.0).to(flag.dtype), out=flag)

    def _acc_flat(self):
        a = getattr(self, "_acc_store", None)
        if a is None or a.numel() < _FLAG_SLOTS + self.grad_flat.numel():
            a = self._acc_store = torch.zeros(self._grad_store.numel(), dtype=torch.float32, device=self.dev)
        return a[_FLAG_SLOTS:_FLAG_SLOTS + self.grad_flat.numel()]

    # ------------------------------------------------------------------ read-backs (host sync)
    def loss(self):
        return float(self._camera.buf['d_cam'][_capi.SPLAT_REPORT_LOSS])

    def check_overflow(self, grow=True):
        """Lists are fixed-size; an iteration whose instances did not fit rendered truncated / empty lists and flagged
        it (stickily; from then on the device skips every Adam step: nothing moves on bad lists).  Call at frame end (two small
        D2H reads): returns True when iterations since the last call were flagged -- ``self.skipped_iterations`` says how many
        took no step.  Also learns the list statistics: from then on the per-tile lists are BUCKETED at 1.5x the longest
        list seen (the per-Gaussian kernel writes instances straight into their tile's bucket: no scan kernel, no
        scatter pass) and the long-list sort launch is skipped while lists stay short."""
        stat = self._camera.buf['status'].tolist()
        rep = self._camera.buf['d_cam'].cpu()
        return self._digest(stat, float(rep[_REPORT_FLAG]) != 0.0, int(rep.view(torch.int32)[_REPORT_SKIPPED]), grow)

    def settle(self, steps, ranks=None, grow=True):
        """End of a phase: ``check_overflow(grow)`` and, when iterations were flagged, the host-side step count they advanced
        (``steps``: "map" or "pose") taken back by as many, because the device took none of those steps.  Returns that number -- the
        iterations the caller runs again -- or 0.  ``ranks`` (``splatam_amd.dist``, or anything with its ``any_rank`` and ``max_int``):
        the flag of any rank and the largest count hold for every rank."""
        flagged = self.check_overflow(grow)
        if ranks is not None:
            flagged = ranks.any_rank(flagged, self.dev)
        if not flagged:
            return 0
        lost = max(self.skipped_iterations if ranks is None else ranks.max_int(self.skipped_iterations, self.dev), 1)
        self._take_back(steps, lost)
        return lost

    def _take_back(self, steps, n):
        """``n`` steps the device skipped never happened: the bias corrections of the "map" / "pose" optimizer are taken again."""
        name = {"map": "map_step", "pose": "pose_step"}[steps]
        setattr(self, name, max(getattr(self, name) - int(n), 0))

    def digest_report(self, report, grow=True):
        """check_overflow() from a HOST copy of an iteration's report (``buf['d_cam']``, SPLAT_ITER_DCAM floats: the status words
        the iteration left are at SPLAT_REPORT_STATUS) -- for callers that fetch the report asynchronously (splatam_amd.plugin): no
        blocking read here.  Only valid for reports of whole iterations (their last kernel writes the snapshot)."""
        ints = report.view(torch.int32)
        return self._digest(ints[_REPORT_STATUS:_REPORT_STATUS + 4].tolist(), float(report[_REPORT_FLAG]) != 0.0, int(ints[_REPORT_SKIPPED]), grow,
                            hysteresis=True)

    def _digest(self, stat, sticky, skipped, grow, hysteresis=False):
        cam, b = self._camera, self._camera.buf
        bad = sticky or stat[_STATUS_OVERFLOW] != 0 or stat[_STATUS_STALE_HINT] != 0 or (cam.tile_stride == 0 and stat[_STATUS_INSTANCES] > cam.capacity)
        self.skipped_iterations = 0
        if bad:
            self.skipped_iterations = max(int(skipped), 1)
            b['d_cam'][_REPORT_FLAG] = 0.0
            b['d_cam'][_REPORT_SKIPPED] = 0.0    # (an int32 counter: the bit pattern of 0.0 is 0)
            cam.reset_status()
            self.map_buf['accum'].zero_()
            b['sums'].zero_()
            cam.max_list_hint = 0
            if grow:
                cam.tile_stride = 0                 # (a bucket overflowed: back to exact lists, re-learn)
                if stat[_STATUS_INSTANCES] > cam.capacity:
                    self._alloc_lists(int(stat[_STATUS_INSTANCES] * 1.5) + 65536)
            return True
        if cam._stats_partial:                  # the last iteration composited a band of tile rows: its statistics are not the frame's
            return False
        longest = int(stat[_STATUS_LONGEST])
        cam.max_list_hint = longest             # short lists: sorted inside the composite, no sort launch
        cam.learnt_P = self.P
        cam.set_sub_bins(16 if longest > 2048 else 1)
        if grow and self.allow_buckets and longest > 0:
            stride = max(256, (int(longest * 1.5) + 63) // 64 * 64)
            # buckets cost 20 bytes per slot (keys, their merge partner, sorted ids): up to ~15 GB of the 288 GB for the clustered
            # stress scenes (337 M slots at 5 M Gaussians) -- one returning atomic per instance instead of count + scan + scatter
            # (reports digested every iteration: the stride only moves when the margin has become thin or the buckets far too wide --
            #  a stride that follows every fluctuation of the longest list would re-lay the buckets iteration by iteration)
            if hysteresis and cam.tile_stride > 0 and longest * 5 // 4 <= cam.tile_stride <= 2 * stride:
                stride = cam.tile_stride
            if stride != cam.tile_stride and stride * cam.num_tiles <= 768 * 1024 * 1024:
                if stride * cam.num_tiles > cam.capacity:
                    self._alloc_lists(stride * cam.num_tiles)
                cam.tile_stride = stride
        return False

    @property
    def seen(self):
        """variables['seen'] of the last iteration ([P], /root/reference/scripts/splatam.py:343)."""
        return self.map_buf['radii'][:self.P] > 0

    def rendered(self):
        """(im[3,H,W], depth[1,H,W], silhouette[H,W], depth_sq[1,H,W]) of the last iteration."""
        o = self._camera.buf['out6']
        return o[0:3], o[3:4], o[4], o[5:6]


def _of_current_camera(field, assignable=False):
    put = (lambda self, value: setattr(self._camera, field, value)) if assignable else None
    return property(lambda self: getattr(self._camera, field), put, doc=f"``{field}`` of the current camera")


# what callers read on the engine with "the current camera's" meaning (the engine's own hot paths read the _Camera itself); the list
# statistics can also be set: tests force stale ones
for _name in ("H", "W", "num_tiles", "num_groups", "capacity", "sub_bins", "_orders", "_natural_order", "_stats_partial", "tile_stride", "max_list_hint"):
    setattr(FusedEngine, _name, _of_current_camera(_name, assignable=_name in ("tile_stride", "max_list_hint")))
FusedEngine.cam_settings, FusedEngine._cam = _of_current_camera("settings"), _of_current_camera("struct")


# ---------------------------------------------------------------------- views (csrc/view.hip)
ViewImage = namedtuple("ViewImage", "rgb8 points colors truncated out6 key", defaults=(None,))
ViewImage.__doc__ = """What ``FusedEngine.render_view`` returns, all on the device and all the VIEW's (overwritten by its next call): ``rgb8``
[H, W, 3] uint8, ``points`` / ``colors`` [H W, 3] float32 (None unless asked for), ``truncated`` (int32 [1], != 0: the lists did not fit, the
picture is incomplete), ``out6`` [6, H, W] (r, g, b, depth, silhouette, depth^2 on a zero background; not written in ``centers`` mode),
``key`` (None unless ``overlay_planes``): the overlay's key plane, int64 [H, W]."""


def _intrinsics4(k):
    """(fx, fy, cx, cy) as host floats from a 3 x 3 / 4 x 4 matrix or a 4-tuple (a tensor on the device is read back: keep it on the host)."""
    if isinstance(k, (tuple, list)) and len(k) == 4 and not hasattr(k[0], "__len__"):
        return tuple(float(x) for x in k)
    if isinstance(k, torch.Tensor):
        k = k.detach().cpu()
    return float(k[0][0]), float(k[1][1]), float(k[0][2]), float(k[1][2])


def _device_mat4(t, name, dev, keep):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (4, 4)):
        got = f"{t.dtype}, {tuple(t.shape)}, {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} must be a float32 tensor of shape [4, 4] on {dev} (got {got})")
    if not t.is_contiguous():           # (a copy per call would be an allocation per call: the caller makes it once)
        raise RuntimeError(f"{name} must be contiguous (row-major 4 x 4): call .contiguous() once, not per view")
    keep.append(t)
    return t


class ViewCamera:
    """One camera that moves in place (``FusedEngine.view_camera``): a ``_Camera`` whose viewmatrix / projmatrix / campos are device
    buffers of its own that splat_view_camera rewrites, the ``w2c`` its frames point at, a one-frame identity pose (so that the
    composite's ``time_idx = 0`` applies no relative transform and the view matrix is the whole pose) and the outputs of
    splat_view_finish.  The Gaussian arrays it renders are the map's own."""

    def __init__(self, engine, width, height, capacity=None):
        from .rasterizer import GaussianRasterizationSettings
        if width <= 0 or height <= 0:
            raise ValueError(f"a view needs a positive size (got {width} x {height})")
        dev = engine.dev
        self.engine, self.W, self.H = engine, width, height
        z = dict(dtype=torch.float32, device=dev)
        self.identity = torch.eye(4, **z)
        self.mats = torch.eye(4, **z).repeat(3, 1, 1)              # w2c, viewmatrix, projmatrix: what splat_view_camera writes
        self.w2c, self.viewmatrix, self.projmatrix = self.mats[0], self.mats[1:2], self.mats[2:3]
        self.campos = torch.zeros(4, **z)[:3]
        self.pose_rot = torch.tensor([1.0, 0.0, 0.0, 0.0], **z).view(1, 4, 1)
        self.pose_trans = torch.zeros(1, 3, 1, **z)
        settings = GaussianRasterizationSettings(image_height=height, image_width=width, tanfovx=1.0, tanfovy=1.0,
                                                 bg=torch.zeros(3, **z), scale_modifier=1.0, viewmatrix=self.viewmatrix,
                                                 projmatrix=self.projmatrix, sh_degree=0, campos=self.campos, prefiltered=False)
        self.camera = _Camera(dev, settings, engine.Pcap, int(capacity) if capacity else 4 * engine.P + 65536, 0)
        assert self.camera.struct.viewmatrix == self.viewmatrix.data_ptr() and self.camera.struct.projmatrix == self.projmatrix.data_ptr()
        self.rgb8 = torch.zeros(height, width, 3, dtype=torch.uint8, device=dev)
        self.points = self.colors = self.keys = None
        self.truncated =torch.zeros(1, dtype=torch.int32, device=dev)
        from .view import jet_lut
        self._lut = torch.from_numpy(jet_lut()).to(dev).contiguous()     # depth mode's default table (768 bytes: made here, so that a later mode allocates nothing)
        self._offset = (C.c_double * 16)()
        self._replay_key, self._replay_rows, self._keep, self._rendered_P = None, {}, None, engine.P
        a = self.args = _capi.SplatViewArgs()
        a.width, a.height = width, height
        a.w2c, a.viewmatrix, a.projmatrix, a.campos = self.w2c.data_ptr(), self.viewmatrix.data_ptr(), self.projmatrix.data_ptr(), self.campos.data_ptr()

    def alloc_cloud(self):
        if self.points is None:
            self.points = torch.zeros(self.H * self.W, 3, dtype=torch.float32, device=self.engine.dev)
            self.colors = torch.zeros(self.H * self.W, 3, dtype=torch.float32, device=self.engine.dev)

    def default_lut(self):
        return self._lut

    def overlay_args(self):
        """The view as csrc/viewoverlay.hip draws through it; the key plane (8 bytes a pixel) is allocated at the first call."""
        if self.keys is None:
            self.keys = torch.full((self.H, self.W), -1, dtype=torch.int64, device=self.engine.dev)
            o = self._overlay = _capi.SplatViewOverlay()
            o.width, o.height, o.w2c, o.keys = self.W, self.H, self.w2c.data_ptr(), self.keys.data_ptr()
        return self._overlay

    def check_overflow(self, grow=True):
        """``FusedEngine.check_overflow`` for THIS camera (two small host reads): True when its renders since the last call ran on lists
        that did not fit -- the lists are grown, the statistics learnt, and the caller renders again.  Between iterations, like the
        render itself."""
        eng, current = self.engine, self.engine._camera
        eng._use(self.camera)
        try:
            skipped = eng.skipped_iterations
            flagged = eng.check_overflow(grow)
            if not flagged:
                self.camera.learnt_P = self._rendered_P   # (a replay renders a prefix of the rows: the statistics are that prefix's)
            eng.skipped_iterations = skipped            # (the loop's count of gated iterations is not the view's to change)
            return flagged
        finally:
            eng._use(current)


def view_finish(out6, mode="color", background=(0.0, 0.0, 0.0), depth_range=(0.0, 6.0), lut=None, rgb8=None, points=None, colors=None,
                intrinsics=None, w2c=None):
    """splat_view_finish on planes of the caller's (include/splat_hip.h): ``out6`` [>= 5, H, W] float32 on a CUDA/HIP device (r, g, b,
    depth, silhouette; a ground-truth frame is its image, its depth and a silhouette of ones) -> ``rgb8`` [H, W, 3] uint8 in ``mode``
    ("color" on ``background``, "depth": ``lut`` [256, 3] uint8 on the device over ``depth_range``, "sil"), ``points`` / ``colors`` [H W, 3]
    float32 (``points`` needs ``intrinsics`` on the host and ``w2c`` float32 [4, 4] on the device).  Outputs are contiguous tensors of
    the caller's with those element counts (views into larger buffers are fine); an output left None is not computed.  One launch on the
    current stream, nothing read back.  Returns ``(rgb8, points, colors)``."""
    if not (isinstance(out6, torch.Tensor) and out6.device.type == "cuda" and out6.dtype == torch.float32 and out6.dim() == 3
            and out6.shape[0] >= 5 and out6.is_contiguous()):
        raise RuntimeError("out6 must be a contiguous float32 tensor [>= 5, H, W] on a CUDA/HIP device; the HIP library has no CPU path")
    dev, H, W = out6.device, int(out6.shape[1]), int(out6.shape[2])
    modes = {"color": _capi.SPLAT_VIEW_COLOR, "depth": _capi.SPLAT_VIEW_DEPTH, "sil": _capi.SPLAT_VIEW_SILHOUETTE, "silhouette": _capi.SPLAT_VIEW_SILHOUETTE}
    if mode not in modes:
        raise ValueError(f"mode must be 'color', 'depth' or 'sil' (got {mode!r})")
    a = _capi.SplatViewArgs()
    a.width, a.height, a.out6, a.mode = W, H, out6.data_ptr(), modes[mode]
    a.bg[:] = [float(c) for c in background]
    a.vmin, a.vmax = float(depth_range[0]), float(depth_range[1])
    for name, t, dtype, n in (("rgb8", rgb8, torch.uint8, 3 * H * W), ("points", points, torch.float32, 3 * H * W), ("colors", colors, torch.float32, 3 * H * W)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.numel() == n and t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous {dtype} tensor of {n} elements on {dev}")
    if rgb8 is not None and modes[mode] == _capi.SPLAT_VIEW_DEPTH:
        if not (isinstance(lut, torch.Tensor) and lut.dtype == torch.uint8 and lut.device == dev and tuple(lut.shape) == (256, 3) and lut.is_contiguous()):
            raise RuntimeError(f"depth mode needs lut: a contiguous uint8 tensor of shape [256, 3] on {dev} (view.jet_lut() is the default table)")
        a.lut = lut.data_ptr()
    keep = []
    if points is not None:
        if intrinsics is None or w2c is None:
            raise ValueError("points need intrinsics and w2c")
        a.fx, a.fy, a.cx, a.cy = _intrinsics4(intrinsics)
        a.w2c = _device_mat4(w2c, "w2c", dev, keep).data_ptr()
    a.rgb8 = rgb8.data_ptr() if rgb8 is not None else None
    a.points = points.data_ptr() if points is not None else None
    a.colors = colors.data_ptr() if colors is not None else None
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_view_finish(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "splat_view_finish")
    return rgb8, points, colors


# ---------------------------------------------------------------------- evaluation metrics on planes (csrc/evalmetrics.hip)
_eval_bufs: dict = {}


def eval_workspace(dev, width, height, ms_ssim):
    """(SplatEvalWorkspace, its ``sums`` tensor) for a device and frame size, allocated on first use and kept (6.5 MB at 1200 x 680).
    The evaluation owns its scratch: an engine's ``buf['sums']`` / ``buf['ssim_maps']`` belong to its iterations.  ``sums`` is
    [SPLAT_ITER_SUM_COPIES + 1][SPLAT_EVAL_SUMS]: the copies (zero between calls) and, last, the totals of the latest frame."""
    key = (str(dev), int(width), int(height), bool(ms_ssim))
    if key not in _eval_bufs:
        lay = _capi.eval_workspace_layout(width, height, ms_ssim)
        pyramid = torch.empty(lay.bytes["pyramid"] // 4, dtype=torch.float32, device=dev) if ms_ssim else None
        sums = torch.zeros(lay.bytes["sums"] // 8, dtype=torch.float64, device=dev).view(-1, _capi.SPLAT_EVAL_SUMS)
        _eval_bufs[key] = (pyramid, sums)
    pyramid, sums = _eval_bufs[key]
    ews = _capi.SplatEvalWorkspace()
    ews.pyramid, ews.sums = (pyramid.data_ptr() if pyramid is not None else None), sums.data_ptr()
    return ews, sums


def _eval_config(sil_thres, sil_mask, ms_ssim, holes=False):
    c = _capi.SplatEvalConfig()
    c.sil_thres, c.sil_mask, c.ms_ssim, c.holes = float(sil_thres), int(bool(sil_mask)), int(bool(ms_ssim)), int(bool(holes))
    return c


def _check_eval_frame(curr_data, H, W, dev):
    for name, t, c in (("im", curr_data['im'], 3), ("depth", curr_data['depth'], 1)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (c, H, W)):
            raise RuntimeError(f"curr_data['{name}'] must be a float32 tensor of shape [{c}, {H}, {W}] on {dev}")


def _check_eval_row(out_row, dev):
    if not (isinstance(out_row, torch.Tensor) and out_row.dtype == torch.float64 and out_row.device == dev
            and out_row.is_contiguous() and out_row.numel() >= _capi.SPLAT_EVAL_ROW):
        raise RuntimeError(f"out_row must be a contiguous float64 tensor of {_capi.SPLAT_EVAL_ROW} elements on {dev}")


def evaluate_metrics(rgb, depth, sil, curr_data, out_row, sil_thres, sil_mask=False, ms_ssim=True, holes=False):
    """The metric kernels alone: ``rgb`` [3,H,W], ``depth`` [1,H,W] or [H,W], ``sil`` [H,W] (the two renders of the drop-in
    rasterizer, say) against ``curr_data['im']`` / ``['depth']``, all float32 on one CUDA/HIP device; the row
    (include/splat_hip.h SPLAT_EVAL_*; slot 5 is 0) goes to ``out_row`` (8 float64 on that device).  ``holes``: the same first-level
    kernel also counts the pixels with ``gt_depth > 0 and not sil > sil_thres`` (the holes of a novel view, eval_nvs()) into slot
    SPLAT_EVAL_HOLES, which is 0 otherwise; the other slots do not depend on it.  Enqueues on the current stream and reads nothing.  Returns the evaluation's sums buffer, whose last row holds the frame's totals once the kernels have
    run (level means = totals / window positions).  MS-SSIM needs min(H, W) > 160 (RuntimeError otherwise, before any launch)."""
    if not isinstance(rgb, torch.Tensor) or rgb.device.type != "cuda":
        raise RuntimeError("evaluate_metrics needs CUDA/HIP tensors; the HIP library has no CPU path")
    dev = rgb.device
    _check_eval_row(out_row, dev)
    H, W = int(rgb.shape[-2]), int(rgb.shape[-1])
    planes = []
    for name, t, n in (("rgb", rgb, 3), ("depth", depth, 1), ("sil", sil, 1), ("curr_data['im']", curr_data['im'], 3),
                       ("curr_data['depth']", curr_data['depth'], 1)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and t.numel() == n * H * W):
            got = f"{t.dtype}, {tuple(t.shape)}, {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise RuntimeError(f"{name} must be a float32 tensor of {n} x {H} x {W} elements on {dev} (got {got})")
        planes.append(t if t.is_contiguous() else t.contiguous())
    ews, sums = eval_workspace(dev, W, H, ms_ssim)
    cfg = _eval_config(sil_thres, sil_mask, ms_ssim, holes)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_eval_metrics(W, H, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
                                                   planes[3].data_ptr(), planes[4].data_ptr(), C.byref(cfg), C.byref(ews),
                                                   out_row.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "splat_eval_metrics")
    return sums


def evaluate_lpips(lpips, rgb, sil, curr_data, out_row, sil_thres, sil_mask=False):
    """LPIPS of an evaluated frame into slot SPLAT_EVAL_LPIPS of ``out_row`` (csrc/lpips.hip, splat_lpips_planes): ``lpips`` an
    ``lpips.Lpips`` on the planes' device, ``rgb`` [3,H,W] and ``sil`` [H,W] the render, ``curr_data['im']`` / ``['depth']`` the frame.
    The images are weighted as ``evaluate_metrics`` weighs them and clamped to 0..1, as the reference hands them to its network.  Call it
    AFTER the call that writes the row (the finish kernel of the metrics leaves 0 in the slot).  Enqueues only."""
    _check_eval_row(out_row, rgb.device)
    lpips.planes(rgb, sil, curr_data['im'], curr_data['depth'], sil_thres, sil_mask=sil_mask,
                 out=out_row[_capi.SPLAT_EVAL_LPIPS:_capi.SPLAT_EVAL_LPIPS + 1])
