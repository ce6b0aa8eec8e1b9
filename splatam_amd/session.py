"""SLAM on frames as they arrive: push a frame, get a pose.

``SlamSession`` is the frame loop of ``pipeline.rgbd_slam`` as an object -- its set-up (the first frame: camera, map, engine) and its
per-frame body (pose initialisation, tracking, densification, keyframe selection, mapping, keyframe list:
/root/reference/scripts/splatam.py:654-905) -- fed one frame at a time.  ``rgbd_slam`` is the driver over it for a finished
sequence; a sensor is another: /root/reference/scripts/iphone_demo.py:150-500 executes the same body while frames arrive from a
phone, each with raw RGB bytes and a float32 LiDAR depth image of a size of its own that are resized on the spot (:218-243).

=============================================  =============================================
here                                           reference
=============================================  =============================================
``SlamSession.add_frame``                      scripts/splatam.py:654-905 (one pass of the loop on a dataset item)
``SlamSession.add_raw_frame``                  scripts/iphone_demo.py:205-243 + the same body (:245-500)
``SlamSession.finish``                         scripts/splatam.py:973-986 / iphone_demo.py:502-520 (what is handed back)
=============================================  =============================================

A frame's path from sensor bytes to pose (``add_raw_frame`` on a HIP device): the caller's arrays are copied into one of two pinned
staging slots, uploaded on the current stream (an event after the upload guards the slot's next use), and ONE launch per resolution
(``fused.ingest_planes``, i.e. ``frames.ingest_planes``: csrc/frameprep.hip P3) writes the planes the loop works on -- full size, the tracking size where it has
one of its own, and on frames that add Gaussians the densification size -- each from the RAW frame, into buffers the session keeps.
Tracking then moves ``cam_unnorm_rots / cam_trans[..., time_idx]``; the returned ``w2c`` is built from them on the device.

The names the loop calls (``slam.initialize_camera_pose``, ``pipeline.keyframe_selection_overlap``, ...) are resolved in their
modules at call time: a wrapper installed there later (``plugin.install``, a recorder) is what runs.
"""
from __future__ import annotations

import json
import time

import numpy as np
import torch

from collections import namedtuple

from . import checkpoint, frames, pipeline, slam

ENGINES = ("fused", "dropin", "plugin", "plugin_map_edits")
HostView = namedtuple("HostView", "array event truncated")
HostView.__doc__ = """``SlamSession.render_view(to_host=True)``: ``array`` [H, W, 3] uint8, a numpy view of a pinned slot, and ``truncated`` (a
pinned int32 [1], != 0: the view's lists did not fit, the picture is incomplete -- ``view_check_overflow()``), both valid once
``event.synchronize()`` returns and until the call after next."""


class _StagingSlot:
    """Pinned host copies of one raw frame; ``busy``: the slot's one event, recorded after every upload that reads them."""

    def __init__(self):
        self.rgb, self.depth, self.busy, self.used = None, None, None, False


class SlamSession:
    """The SplaTAM frame loop fed one frame at a time.

    ``SlamSession(config, num_frames, engine="fused", gaussian_capacity=None, verbose=False)``: ``config`` as ``pipeline.rgbd_slam``
    takes it; ``num_frames`` is declared up front (``config['num_frames']`` in the reference's online demo): it sizes
    ``cam_unnorm_rots`` / ``cam_trans`` and drives the ``time_idx == num_frames - 2`` keyframe rule; one frame more raises.
    ``device``: where frames that arrive as host arrays are processed (default ``config['primary_device']``, else "cuda:0"); frames
    that are tensors on a device are processed there.  ``return_pose=False`` leaves ``w2c`` out of the result (the batch driver
    reads its poses from the parameters at the end).  ``reference_division``: how ``add_frame`` on the fused engine turns an item's
    0..255 colour into the loop's image on a HIP device.  False (default): one launch of ``fused.prepare_frame``, a correctly rounded
    division by 255 -- bit for bit what ``add_raw_frame`` writes for the same bytes.  True: torch's ``permute(2, 0, 1) / 255``,
    which on the device multiplies by the rounded reciprocal of 255 (different in the last bit for 126 of the 256 byte values), as
    the reference's own loop does on CUDA: what ``rgbd_slam`` has always computed, and keeps.

    The FIRST frame fixes the size, the intrinsics, the device and ``first_frame_w2c`` = ``inv(pose)`` -- the identity with
    ``pose=None`` (iphone_demo.py:231).  Intrinsics of later frames are ignored, as in the reference.  ``use_gt_poses`` needs a pose
    with every frame: a frame without one raises before anything is done with it.

    ``add_frame`` / ``add_raw_frame`` return ``{time_idx, w2c, tracking_iters, num_gaussians, keyframe, phase_ms}``: ``w2c`` the
    estimated world-to-camera [4, 4] on the device (nothing is read back for it).  ``finish()`` returns ``(params, variables,
    stats)`` as ``rgbd_slam`` does, with ``stats['frames_seen']``; before ``num_frames`` frames it cuts the two pose arrays to the
    frames seen.  A context manager; ``close()`` undoes ``plugin.install`` (engines "plugin", "plugin_map_edits").

    A keyframe is NOT stored for a frame whose ``pose`` holds inf or NaN (scripts/splatam.py:893-896, iphone_demo.py:468-469; TUM has
    such frames); every frame with ``pose=None`` is stored."""

    def __init__(self, config, num_frames, engine="fused", gaussian_capacity=None, verbose=False, device=None, return_pose=True,
                 reference_division=False):
        from . import dist as sdist
        if engine not in ENGINES:
            raise ValueError(engine)
        self.fused = engine == "fused"
        self.plugged = engine in ("plugin", "plugin_map_edits")
        if self.plugged and sdist.world_size() > 1:
            raise NotImplementedError(f"engine='{engine}' runs the reference's single-process loop")
        if int(num_frames) != num_frames or int(num_frames) < 1:
            raise ValueError(f"num_frames must be a positive integer, declared up front (got {num_frames!r})")
        self.config, self.num_frames, self.engine_name = config, int(num_frames), engine
        tcfg, mcfg = config['tracking'], config['mapping']
        if mcfg.get('use_gaussian_splatting_densification') and not self.fused:
            # the reference's own densify cannot run inside its SLAM loop either: it never extends variables['timestep'], and the
            # remove_points that follows indexes it with the longer mask (utils/slam_external.py:206-227, 139-162).  The fused engine
            # carries `timestep` along with the duplicated rows (FusedEngine.densify).
            raise NotImplementedError("gradient-based densification inside the frame loop needs engine='fused'")
        self.dist_kind = config.get('gaussian_distribution', 'isotropic')
        if self.dist_kind not in ("isotropic", "anisotropic"):
            raise ValueError(f"Unknown gaussian_distribution {self.dist_kind}")
        if self.fused and config['mean_sq_dist_method'] != "projective":
            raise ValueError(f"Unknown mean_sq_dist_method {config['mean_sq_dist_method']}")
        self.gaussian_capacity, self.verbose, self.return_pose = gaussian_capacity, verbose, return_pose
        self.reference_division = bool(reference_division)
        self.device = None if device is None else torch.device(device)
        self.frames_seen, self.engine, self.cam = 0, None, None
        self.params = self.variables = None
        self.keyframe_list, self.keyframe_time_indices = [], []
        self.stats = dict(tracking_iters=0, mapping_iters=0, tracking_s=0.0, mapping_s=0.0, mapping_loop_s=0.0, redone_iterations=0,
                          num_gaussians=[], phase_ms=[], frame_s=[], decisions=[])
        # the planes handed to the loop on the latest frame: {'full', 'tracking', 'densify'} -> (im, depth), None where the step ran on the
        # full frame (densification: also on frames that add nothing)
        self.last_frame = None
        self._installed, self._finished, self._t_frame = None, False, None
        self._phase, self._sync_prepare = None, False       # the phase timer, made with the first frame (its device)
        self._tracking_frames = self._densify_frames = None
        self._raw = None                    # the raw path's buffers and sizes, made on its first frame
        self._view = None                   # render_view's view camera and pinned slots, made on its first call
        # checkpoints: the writer thread, the pinned host copies and the keyframe planes already copied (all made by the first save_checkpoint)
        self._writer = self._host = None
        self._kf_host, self._raw_restored, self.last_checkpoint = [], False, None

    # ------------------------------------------------------------------ life cycle
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        """Undoes ``plugin.install`` (its counters go to ``stats['plugin']``) and waits for a checkpoint still being written; the session
        takes no more frames."""
        self._finished = True
        if self._installed is not None:
            from . import plugin
            self.stats['plugin'] = plugin.session_stats()
            self._installed.uninstall()
            self._installed = None
        self.join_checkpoint()                  # (a failed write raises here)

    def finish(self):
        """``(params, variables, stats)``; before ``num_frames`` frames the pose arrays are cut to ``stats['frames_seen']``."""
        if self.frames_seen == 0:
            raise RuntimeError("finish() before the first frame: there is no map")
        self.close()
        self.stats['keyframe_time_indices'] = self.keyframe_time_indices
        self.stats['frames_seen'] = n = self.frames_seen
        params = self.params
        if n < self.num_frames:
            params = dict(params)
            for k in ('cam_unnorm_rots', 'cam_trans'):
                params[k] = torch.nn.Parameter(params[k].detach()[..., :n].clone())
        return params, self.variables, self.stats

    # ------------------------------------------------------------------ checkpoints (splatam_amd/checkpoint.py)
    def _refuse_checkpoints(self, key):
        from . import dist as sdist
        if self.plugged:
            raise NotImplementedError(f"{key}: checkpoints are not supported with engine='{self.engine_name}' (use 'fused' or 'dropin')")
        if sdist.world_size() > 1:
            raise NotImplementedError(f"{key}: checkpoints are not supported in the multi-rank frame loop")

    def join_checkpoint(self):
        """Waits for the checkpoint being written, if any; a failed write raises here.  Returns the bytes written per file kind
        (``reference``, ``session``, ``keyframes``) of the latest checkpoint."""
        if self._writer is None:
            return {}
        self._writer.join()
        return dict(self._writer.bytes_written)

    def _host_copies(self, directory, key):
        self._refuse_checkpoints(key)
        if self.frames_seen == 0 or self.params is None:
            raise RuntimeError(f"{key}: a checkpoint before the first frame: there is no map")
        if self._writer is None:
            self._writer, self._host = checkpoint.Writer(), checkpoint.HostCopies(self.dev)
        self._writer.join()                     # (the pinned copies are the previous checkpoint's until its files are written)
        return {k: self._host.copy(k, self.params[k]) for k in checkpoint.MAP_KEYS}

    def save_reference_checkpoint(self, directory, time_idx=None):
        """The reference's checkpoint of the state after the latest frame (scripts/splatam.py:927-931): ``params<t>.npz`` with every
        entry of ``params`` and ``keyframe_time_indices<t>.npy``, written on the background thread.  Between frames."""
        t = self.frames_seen - 1 if time_idx is None else int(time_idx)
        host = self._host_copies(directory, "save_checkpoints")
        self._host.wait()
        indices = list(self.keyframe_time_indices)
        self._writer.submit([("reference", lambda: checkpoint.write_reference(directory, t, host, indices))])
        return checkpoint.reference_paths(directory, t)

    def load_reference_checkpoint(self, directory, time_idx, dataset, tracking_item=None, densify_item=None):
        """``load_checkpoint`` as the reference does it (scripts/splatam.py:604-640), before the first frame: the first frame's set-up
        runs on ``dataset[0]`` (camera, ``scene_radius``, first-frame point cloud; ``tracking_item`` / ``densify_item``: the first
        items of datasets at those sizes), then the parameters are replaced by the file's, ``max_2D_radius``,
        ``means2D_gradient_accum``, ``denom`` AND ``timestep`` become zeros of the loaded row count, the keyframe list is rebuilt for
        the listed indices BELOW ``time_idx`` (frames from ``dataset``, ``est_w2c`` from the loaded poses) while
        ``keyframe_time_indices`` keeps the file's list, and the next frame the session takes is ``time_idx`` itself: it is tracked
        and mapped a second time, and where it is a keyframe frame its index ends up in the list twice.  Random streams are left as
        they are."""
        self._refuse_checkpoints("load_checkpoint")
        if self.params is not None or self.frames_seen:
            raise RuntimeError("load_checkpoint: the session has taken frames already")
        time_idx = int(time_idx)
        if not 0 <= time_idx < self.num_frames:
            raise ValueError(f"checkpoint_time_idx = {time_idx} is outside the run's {self.num_frames} frames")
        loaded, indices = checkpoint.load_reference(directory, time_idx, "cpu")        # (a missing file is named before any work)
        missing = [k for k in checkpoint.MAP_KEYS if k not in loaded]
        if missing:
            raise ValueError(f"{checkpoint.reference_paths(directory, time_idx)[0]} has no entry {missing[0]!r}")
        color, depth, intrinsics, pose = dataset[0]
        self._first_item(color, depth, intrinsics, pose, *self._item_planes(color, depth), tracking_item, densify_item)
        if self.fused:
            self.engine.replace_map(loaded)
        else:
            for k in ('cam_unnorm_rots', 'cam_trans'):
                if tuple(loaded[k].shape) != tuple(self.params[k].shape):
                    raise ValueError(f"checkpoint entry '{k}' has shape {tuple(loaded[k].shape)}, the run was declared with "
                                     f"{tuple(self.params[k].shape)} (num_frames = {self.num_frames})")
            self.params = {k: v.detach().to(self.dev).requires_grad_(True) for k, v in loaded.items()}
            rows = self.params['means3D'].shape[0]
            for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep'):
                self.variables[k] = torch.zeros(rows, device=self.dev)
        with torch.no_grad():
            for t in range(time_idx):
                if t in indices:
                    color, depth = dataset[t][:2]
                    im, d = self._item_planes(color, depth)
                    self.keyframe_list.append({'id': t, 'est_w2c': pipeline._est_w2c(self.params, t), 'color': im, 'depth': d})
        self.keyframe_time_indices = list(indices)
        self.frames_seen, self._t_frame = time_idx, None
        return self

    def save_checkpoint(self, directory, keyframes=None):
        """An exact checkpoint of the session after its latest frame ``t``, between frames: the reference's pair (``params<t>.npz``,
        ``keyframe_time_indices<t>.npy``) plus ``session<t>.npz`` -- every entry of ``variables`` (``timestep`` too), ``frames_seen``,
        ``first_frame_w2c``, intrinsics, the frame size and the reduced sizes, every keyframe's ``est_w2c``, ``stats`` so far, the state
        of Python's, numpy's and torch's CPU random streams and of the device generator, and on the fused engine the list sizing
        of every camera (``FusedEngine.list_sizing``: it decides whether an iteration gets flagged, a flagged phase draws fresh
        random views for the iterations it runs again, so the random stream depends on it).  ``SlamSession.restore`` continues at
        ``t + 1`` as if the run had never stopped.  Arrays and JSON strings only; nothing is pickled.

        ``keyframes``: also write ``keyframes<t>.npz`` with every keyframe's colour and depth planes as float32, copied bit for bit:
        16 bytes per pixel and keyframe, 13 MB per keyframe at 1200 x 680.  Default: True for a session fed by ``add_raw_frame``
        (nothing to read them from again), False for an ``add_frame`` session (``restore`` reads them from a dataset).

        Device tensors are copied into pinned host buffers the session keeps (a keyframe's planes once: later checkpoints reuse the
        copy) with ONE synchronisation; the files are written by one background thread that the next ``save_checkpoint``,
        ``join_checkpoint``, ``finish()`` and ``close()`` join -- a failed write raises there.  Frames that do not checkpoint
        synchronise and allocate nothing for it.  Returns ``{time_idx, paths}``."""
        t0 = time.perf_counter()
        host = self._host_copies(directory, "save_checkpoint")
        t = self.frames_seen - 1
        if keyframes is None:
            keyframes = self._raw is not None or self._raw_restored
        H = self._host
        arrays = {f"var/{k}": H.copy(f"var/{k}", v) for k, v in self.variables.items() if isinstance(v, torch.Tensor) and k != 'means2D'}
        arrays['first_frame_w2c'] = H.copy('first_frame_w2c', self.first_frame_w2c)
        arrays['intrinsics'] = H.copy('intrinsics', self.intrinsics)
        kfs = self.keyframe_list
        if kfs:
            arrays['keyframe_est_w2c'] = H.copy('keyframe_est_w2c', torch.stack([kf['est_w2c'] for kf in kfs]))
        else:
            arrays['keyframe_est_w2c'] = np.zeros((0, 4, 4), dtype=np.float32)
        arrays['keyframe_ids'] = np.array([kf['id'] for kf in kfs], dtype=np.int64)
        arrays['keyframe_time_indices'] = np.array(self.keyframe_time_indices, dtype=np.int64)
        reduced = {}
        for which, fr in (('tracking', self._tracking_frames), ('densify', self._densify_frames)):
            reduced[which] = None if fr is None else dict(size=list(fr.size), from_items=bool(fr.from_items))
            if fr is not None:
                arrays[f"{which}_intrinsics"] = H.copy(f"{which}_intrinsics", fr.intrinsics)
        planes = None
        if keyframes:
            for i in range(len(self._kf_host), len(kfs)):       # (a stored keyframe never changes: each is copied once)
                self._kf_host.append((H.copy(None, kfs[i]['color'], keep=True), H.copy(None, kfs[i]['depth'], keep=True)))
            planes = dict(count=np.array(len(kfs), dtype=np.int64))
            for i, (c, d) in enumerate(self._kf_host[:len(kfs)]):
                planes[f"color{i}"], planes[f"depth{i}"] = c, d
        rng_arrays, rng_meta = checkpoint.capture_random(self.dev)
        arrays.update(rng_arrays)
        H.wait()                                # the checkpoint's one synchronisation
        cam = self.cam
        meta = dict(format=checkpoint.FORMAT, time_idx=t, frames_seen=self.frames_seen, num_frames=self.num_frames,
                    engine=self.engine_name, engine_family="fused" if self.fused else "statements", device=str(self.dev),
                    gaussian_distribution=self.dist_kind, frame_size=[int(cam.image_height), int(cam.image_width)], reduced=reduced,
                    reference_division=self.reference_division, raw=bool(self._raw is not None or self._raw_restored),
                    keyframes_stored=bool(keyframes), rng=rng_meta, stats=self.stats)
        if self.fused:
            eng = self.engine
            meta['fused'] = dict(list_sizing=eng.list_sizing(), gaussian_capacity=int(eng.Pcap), creation_order=bool(eng.creation_order))
        arrays['meta'] = np.array(json.dumps(meta))
        indices = list(self.keyframe_time_indices)
        jobs = [("reference", lambda: checkpoint.write_reference(directory, t, host, indices)),
                ("session", lambda: checkpoint._write_npz(checkpoint.session_path(directory, t), arrays))]
        if planes is not None:
            jobs.append(("keyframes", lambda: checkpoint._write_npz(checkpoint.keyframes_path(directory, t), planes)))
        self._writer.submit(jobs)
        paths = checkpoint.reference_paths(directory, t) + (checkpoint.session_path(directory, t),)
        if planes is not None:
            paths += (checkpoint.keyframes_path(directory, t),)
        self.last_checkpoint = dict(time_idx=t, paths=paths, host_ms=1e3 * (time.perf_counter() - t0))
        return self.last_checkpoint

    @classmethod
    def restore(cls, config, directory, time_idx, num_frames=None, dataset=None, engine="fused", gaussian_capacity=None, verbose=False,
                device=None, return_pose=True, reference_division=None):
        """The session ``save_checkpoint`` put down after frame ``time_idx``: its next frame is ``time_idx + 1``.

        Keyframe planes come from ``keyframes<t>.npz`` where the checkpoint has one, else from ``dataset`` (its full-size frames, through
        the path ``add_frame`` took -- ``reference_division`` is the checkpoint's; passing another value raises); with neither it
        raises.  A checkpoint whose ``frame_size``, ``tracking_size`` / ``densification_size``, ``gaussian_distribution`` or
        ``engine_family`` disagrees with ``config`` / ``engine`` is refused with a message that names the entry.  ``num_frames`` may be
        LARGER than the saved one -- the two pose arrays are extended with the rows ``initialize_params`` writes (identity quaternion,
        zero translation): a finished map is continued with more frames -- and not smaller.  The random streams are set from the
        checkpoint as the last act: the state of the calling process does not matter.  ``device``: default the checkpoint's."""
        arrays, meta = checkpoint.load_session(directory, time_idx)
        where = checkpoint.session_path(directory, time_idx)
        saved_frames = int(meta['num_frames'])
        num_frames = saved_frames if num_frames is None else int(num_frames)
        if num_frames < saved_frames:
            raise ValueError(f"{where}: num_frames = {num_frames} is smaller than the checkpoint's num_frames = {saved_frames}")
        if reference_division is not None and bool(reference_division) != bool(meta['reference_division']):
            raise ValueError(f"{where}: reference_division = {bool(meta['reference_division'])} in the checkpoint, {bool(reference_division)} asked for")
        self = cls(config, num_frames, engine=engine, gaussian_capacity=gaussian_capacity, verbose=verbose, device=device,
                   return_pose=return_pose, reference_division=bool(meta['reference_division']))
        self._refuse_checkpoints("restore")
        dev = torch.device(meta['device']) if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        family = "fused" if self.fused else "statements"
        if family != meta['engine_family']:
            raise ValueError(f"{where}: engine_family = {meta['engine_family']!r} (engine {meta['engine']!r}), engine={engine!r} asked for")
        if self.dist_kind != meta['gaussian_distribution']:
            raise ValueError(f"{where}: gaussian_distribution = {meta['gaussian_distribution']!r}, the config says {self.dist_kind!r}")
        data = config.get('data') or {}
        H, W = (int(x) for x in meta['frame_size'])
        if "desired_image_height" in data and (int(data["desired_image_height"]), int(data["desired_image_width"])) != (H, W):
            raise ValueError(f"{where}: frame_size = {(H, W)}, the config's desired_image_height / _width say "
                             f"{(int(data['desired_image_height']), int(data['desired_image_width']))}")
        for which, key in (('tracking', "tracking"), ('densify', "densification")):
            saved = meta['reduced'][which]
            if saved is not None and saved['from_items']:
                continue                        # (the size was a dataset's own: the items of the frames to come carry it)
            asked = (int(data[f"{key}_image_height"]), int(data[f"{key}_image_width"])) if f"{key}_image_height" in data else None
            asked = None if asked == (H, W) else asked
            have = None if saved is None else tuple(saved['size'])
            if asked != have:
                raise ValueError(f"{where}: {key}_size = {have}, the config's {key}_image_height / _width say {asked}")
        planes = checkpoint.load_keyframes(directory, time_idx)
        ids = [int(x) for x in arrays['keyframe_ids']]
        if planes is None and dataset is None and ids:
            raise ValueError(f"{checkpoint.keyframes_path(directory, time_idx)} does not exist and no dataset was passed: nothing to "
                             f"restore the planes of keyframes {ids} from")
        loaded, _ = checkpoint.load_reference(directory, time_idx, "cpu")
        on_dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)                   # noqa: E731
        with torch.no_grad():
            for k, first in (('cam_unnorm_rots', 1.0), ('cam_trans', 0.0)):
                if num_frames > saved_frames:
                    more = torch.zeros(1, loaded[k].shape[1], num_frames - saved_frames)
                    more[:, 0, :] = first
                    loaded[k] = torch.cat((loaded[k].detach(), more), dim=-1)
            params = {k: torch.nn.Parameter(loaded[k].detach().to(dev).contiguous().requires_grad_(True)) for k in checkpoint.MAP_KEYS}
        variables = {k[4:]: on_dev(v) for k, v in arrays.items() if k.startswith("var/")}
        intrinsics, first_frame_w2c = on_dev(arrays['intrinsics']), on_dev(arrays['first_frame_w2c']).float().contiguous()
        cam = slam.setup_camera(W, H, intrinsics.cpu().numpy(), first_frame_w2c.cpu().numpy(), device=dev)
        reduced = {}
        for which in ('tracking', 'densify'):
            saved = meta['reduced'][which]
            reduced[which] = None
            if saved is not None:
                fr = pipeline._ReducedFrames(None, saved['size'], (H, W), None, intrinsics=on_dev(arrays[f"{which}_intrinsics"]))
                fr.from_items = bool(saved['from_items'])
                fr.cam = slam.setup_camera(fr.size[1], fr.size[0], fr.intrinsics.cpu().numpy(), first_frame_w2c.cpu().numpy(), device=dev)
                reduced[which] = fr
        if self.fused:
            from .fused import FusedEngine
            sizing = meta['fused']
            cap = max(int(sizing['gaussian_capacity']), int(gaussian_capacity or 0))
            eng = FusedEngine(params, cam, gaussian_capacity=cap, variables=variables)
            eng.keep_map_grads = False
            for fr in (reduced['tracking'], reduced['densify']):        # (the order _start registers them in)
                if fr is not None:
                    eng.add_camera(fr.cam)
            eng.select_camera(cam)
            eng.set_list_sizing(sizing['list_sizing'])
            eng.creation_order = bool(sizing['creation_order'])
            self.engine = eng
        self.scene_radius = variables['scene_radius']
        self.params, self.variables, self.cam, self.dev = params, variables, cam, dev
        self.intrinsics, self.first_frame_w2c = intrinsics, first_frame_w2c
        self._tracking_frames, self._densify_frames, self._densify0 = reduced['tracking'], reduced['densify'], None
        self._phase = pipeline._PhaseTimer(dev)
        self._sync_prepare = reduced['tracking'] is not None or reduced['densify'] is not None
        self._raw_restored = bool(meta['raw'])
        est = on_dev(arrays['keyframe_est_w2c'])
        for i, t in enumerate(ids):
            if planes is not None:
                im, d = on_dev(planes[i][0]), on_dev(planes[i][1])
            else:
                color, depth = dataset[t][:2]
                if color.device != dev:
                    raise ValueError(f"the dataset's frames are on {color.device}, the checkpoint is restored on {dev}")
                im, d = self._item_planes(color, depth)
            if tuple(im.shape) != (3, H, W):
                raise ValueError(f"{where}: frame_size = {(H, W)}, keyframe {t} restored as {tuple(im.shape[1:])}")
            self.keyframe_list.append({'id': t, 'est_w2c': est[i].clone(), 'color': im, 'depth': d})
        self.keyframe_time_indices = [int(x) for x in arrays['keyframe_time_indices']]
        stats = meta['stats']
        for decided in stats.get('decisions', []):
            decided['prunes'] = [tuple(p) for p in decided['prunes']]
        self.stats = stats
        self.frames_seen = int(meta['frames_seen'])
        checkpoint.restore_random(arrays, meta['rng'], dev)
        return self

    def _check_raw_sizes(self):
        """A restored raw session's first raw frame: the sizes its buffers were just made for are the checkpoint's."""
        R = self._raw
        have = dict(full=(int(self.cam.image_height), int(self.cam.image_width)),
                    tracking=None if self._tracking_frames is None else tuple(self._tracking_frames.size),
                    densify=None if self._densify_frames is None else tuple(self._densify_frames.size))
        for which in ('full', 'tracking', 'densify'):
            if R[which] != have[which]:
                self._raw = None
                raise ValueError(f"the raw frame and config['data'] give a {which} size of {R[which]}, the restored session's is {have[which]}")

    def _densifies(self, time_idx):
        """Does frame ``time_idx`` read a densification frame (the first frame's point cloud, ``add_new_gaussians`` afterwards)?"""
        return time_idx == 0 or self._will_add(time_idx)

    def _will_add(self, time_idx):
        return time_idx > 0 and (time_idx + 1) % self.config['map_every'] == 0 and bool(self.config['mapping']['add_new_gaussians'])

    def _begin_frame(self):
        """The driver's hook: the moment the next frame starts to arrive.  From here its ``frame_s`` and its ``prepare_frames`` phase count
        (without the call they start with ``add_frame`` / ``add_raw_frame``)."""
        if self._t_frame is None:
            if self._phase is not None and self._sync_prepare:
                self._phase._sync()
            self._t_frame = time.perf_counter()

    def _admit(self, pose):
        if self._finished:
            raise RuntimeError("the session is finished")
        if self.frames_seen >= self.num_frames:
            raise RuntimeError(f"frame {self.frames_seen}: the session was declared with num_frames = {self.num_frames}")
        if pose is None and self.config['tracking']['use_gt_poses']:
            raise ValueError("config['tracking']['use_gt_poses'] needs a pose with every frame (got pose=None)")
        self._begin_frame()
        return self.frames_seen

    # ------------------------------------------------------------------ the two entries
    def add_frame(self, color, depth, intrinsics, pose=None, tracking_item=None, densify_item=None, _pose_finite=None):
        """One dataset item: ``color`` [H, W, 3] in 0..255, ``depth`` [H, W, 1], ``intrinsics`` [4, 4] (or [3, 3]), ``pose``
        camera-to-world [4, 4] or None, as ``dataset[i]`` hands them over.  ``tracking_item`` / ``densify_item``: this frame's item
        of a dataset at the tracking / densification size (``rgbd_slam(tracking_dataset=, densify_dataset=)``; the first frame decides
        whether there is one; ``densify_item`` is read on the first frame and on frames that add Gaussians).  Without them the
        sizes come from ``config['data']`` and the reduced frames are derived from the full one.  ``_pose_finite``: the driver's hook
        (``rgbd_slam`` answers the keyframe rule's question from the dataset's host copy of the poses, where it has one)."""
        time_idx = self._admit(pose)
        im, d = self._item_planes(color, depth)
        if self.params is None:
            self._first_item(color, depth, intrinsics, pose, im, d, tracking_item, densify_item)
        tf, df = self._tracking_frames, self._densify_frames
        curr = self._curr_data(time_idx, im, d)
        tracking_curr = curr if tf is None else tf.curr_data(time_idx, color, depth, self.first_frame_w2c, tracking_item)
        densify_curr = curr if (df is None or not self._will_add(time_idx)) else \
            df.curr_data(time_idx, color, depth, self.first_frame_w2c, densify_item)
        return self._step(time_idx, curr, tracking_curr, densify_curr, pose, owned=False, pose_finite=_pose_finite)

    def _item_planes(self, color, depth):
        """(im [3, H, W] in 0..1, depth [1, H, W]) of a dataset item's colour and depth: the path ``add_frame`` takes (a keyframe
        restored from a dataset goes through it again)."""
        if self.fused and color.device.type == "cuda" and not self.reference_division and color.dtype == depth.dtype == torch.float32:
            # one launch (csrc/frameprep.hip P1) and a correctly rounded division: the planes add_raw_frame writes for the same bytes
            from . import fused
            return fused.prepare_frame(color, depth)
        return (color.permute(2, 0, 1) / 255).contiguous(), depth.permute(2, 0, 1).contiguous()

    def _first_item(self, color, depth, intrinsics, pose, im, d, tracking_item, densify_item):
        """The set-up on the first dataset item (``im``, ``d``: its planes)."""
        full_size = (int(color.shape[0]), int(color.shape[1]))
        tracking = pipeline._reduced_frames("tracking", tracking_item, self.config, full_size, intrinsics)
        densify = pipeline._reduced_frames("densification", densify_item, self.config, full_size, intrinsics)
        densify0 = None
        if densify is not None:
            densify0 = densify.frame(0, color, depth, densify_item) + (densify.intrinsics,)
        self._start(color.device, im, d, intrinsics, pose, tracking, densify, densify0)

    def add_raw_frame(self, rgb_u8, depth_raw, intrinsics, pose=None, depth_scale=None):
        """What a sensor or a decoder delivers: ``rgb_u8`` [H, W, 3] uint8 and ``depth_raw`` [H', W'] at a size of its own -- float32
        metres with ``depth_scale=None``, or uint16 with the PNG-style divisor -- as numpy arrays, CPU tensors or tensors on the
        device.  ``intrinsics`` belong to the raw colour size and are scaled to ``config['data']['desired_image_height / _width']``
        (default: the raw size) with ``slam.scale_intrinsics``; where that size is raw / ``downscale_factor`` exactly this is the
        demo's division by ``downscale_factor`` (iphone_demo.py:228-230).

        Host data is copied into a pinned staging slot (two, used in turn, each guarded by an event recorded after its upload) and
        uploaded on the current stream: the caller may overwrite its arrays as soon as the call returns.  ``fused.ingest_planes``
        writes the full-size planes and, where ``config['data']`` names tracking / densification sizes of their own, those too
        (densification on frames that add Gaussians) -- each from the RAW frame, not from the resized one, as ``dataset.at_size`` and
        the demo (:235-243) do.  All buffers are the session's and are written again by the next frame (a stored keyframe keeps a copy
        of its planes): nothing else is allocated per frame after the first.  On ``device="cpu"`` ``datasets.ingest_planes_cpu`` runs.

        A known difference to the demo: it calls ``cv2.resize`` on the uint8 image, which rounds the result back to bytes with
        OpenCV's fixed-point weights; this path keeps the float32 blend, as the dataset loaders here and the reference's own dataset
        loaders (which resize float64 images) do.  OpenCV is not available where this is developed and tested: neither form is pinned
        against it."""
        time_idx = self._admit(pose)
        rgb, raw = self._as_tensor(rgb_u8, "rgb_u8", (torch.uint8,)), self._as_tensor(depth_raw, "depth_raw", (torch.uint16, torch.float32))
        if rgb.dim() != 3 or rgb.shape[2] != 3:
            raise ValueError(f"rgb_u8 must be [H, W, 3] (got {tuple(rgb.shape)})")
        if raw.dim() == 3 and raw.shape[2] == 1:
            raw = raw[:, :, 0]
        if raw.dim() != 2:
            raise ValueError(f"depth_raw must be [H, W] or [H, W, 1] (got {tuple(raw.shape)})")
        if raw.dtype == torch.float32:
            if depth_scale is not None and float(depth_scale) != 1.0:
                raise ValueError(f"float32 depth is in metres already: depth_scale must be None (got {depth_scale})")
            scale = None
        else:
            if depth_scale is None or not float(depth_scale) > 0.0:
                raise ValueError(f"uint16 depth needs its positive depth_scale (got {depth_scale})")
            scale = float(depth_scale)
        if self._raw is None:
            if time_idx != 0 and not self._raw_restored:
                raise RuntimeError("the session started with add_frame: its frames are dataset items")
            self._raw = self._raw_setup(rgb, raw, intrinsics)
            if self._raw_restored:
                self._check_raw_sizes()
        R = self._raw
        if (tuple(rgb.shape[:2]), tuple(raw.shape), raw.dtype) != R['shapes']:
            raise ValueError(f"frame {time_idx}: raw sizes {tuple(rgb.shape[:2])}, {tuple(raw.shape)} ({raw.dtype}) differ from the first frame's {R['shapes']}")
        dev = R['device']
        adds = self._densifies(time_idx)
        if dev.type == "cuda":
            rgb, raw = self._upload(rgb, raw)
            ingest = lambda which: frames.ingest_planes(rgb, raw, scale, R[which], out=R['planes'][which])        # noqa: E731
        else:
            ingest = lambda which: frames.ingest_planes_cpu(rgb, raw, scale, R[which])                              # noqa: E731
        planes = {'full': ingest('full')}
        for which in ('tracking', 'densify'):
            if R[which] is not None and (which == 'tracking' or adds):
                planes[which] = ingest(which)
        im, d = planes['full']
        if self.params is None:
            make = lambda which: None if R[which] is None else pipeline._ReducedFrames(        # noqa: E731
                None, R[which], R['full'], R['k_full'], intrinsics=R['k_' + which])
            tracking, densify = make('tracking'), make('densify')
            densify0 = None if densify is None else planes['densify'] + (densify.intrinsics,)
            self._start(dev, im, d, R['k_full'], None if pose is None else torch.as_tensor(pose, dtype=torch.float32), tracking, densify, densify0)
        curr = self._curr_data(time_idx, im, d)
        reduced = lambda frames, which: {'cam': frames.cam, 'im': planes[which][0], 'depth': planes[which][1], 'id': time_idx,     # noqa: E731
                                         'intrinsics': frames.intrinsics, 'w2c': self.first_frame_w2c}
        tracking_curr = curr if self._tracking_frames is None else reduced(self._tracking_frames, 'tracking')
        densify_curr = curr if (self._densify_frames is None or not self._will_add(time_idx)) else reduced(self._densify_frames, 'densify')
        if pose is not None:
            pose = torch.as_tensor(pose, dtype=torch.float32)
        return self._step(time_idx, curr, tracking_curr, densify_curr, pose, owned=dev.type == "cuda")

    # ------------------------------------------------------------------ a mesh of the map (csrc/tsdf.hip)
    def extract_mesh(self, frames=None, size=None, path=None, method="tetrahedra", views=None, views_mode="shaded", **kwargs):
        """A triangle mesh of the map as it is now: ``mesh.extract_mesh`` at the estimated poses of ``frames`` (time indices; default
        the keyframes so far), rendered at ``size`` = (height, width) (default the loop's) with the loop's intrinsics scaled to it.
        Further keywords (``voxel_size``, ``trunc``, ``bounds``, ``max_bytes``, ``sil_thres``, ``depth_max``, ``weight_max``,
        ``min_weight``, ``sparse``, ``clean``) go to ``mesh.extract_mesh``, as does ``method`` (``"tetrahedra"``, or ``"cubes"`` for
        marching cubes: about a third of the triangles; anything else is a ValueError); ``clean=True`` (or a dict of ``mesh_clean.clean_mesh``
        keywords) removes the mesh's small connected components.  ``simplify`` (a cell size in metres, or a dict of
        ``mesh_simplify.simplify_mesh`` keywords that names ``cell``) merges the vertices in each cell of a grid, after the cleaning.
        ``path``: also written there as a PLY.  ``views`` (a directory): pictures
        ``mesh_%04d.png`` of the mesh in ``views_mode`` at the estimated poses of ``frames``, numbered by time index
        (``mesh_view.render_trajectory``).  Returns the ``Mesh`` (on the device).
        Between frames and after ``finish()``; engine "fused" only.  The map, the optimiser state and the loop's cameras are left
        as they were."""
        from . import mesh as mesh_mod
        from .mesh_simplify import _simplified, simplify_options
        mesh_mod.check_method(method)
        simplify = simplify_options(kwargs.pop("simplify", None))
        if not self.fused:
            raise NotImplementedError("extract_mesh needs engine='fused'")
        if self.engine is None:
            raise RuntimeError("extract_mesh before the first frame: there is no map")
        H, W = (self.cam.image_height, self.cam.image_width) if size is None else (int(size[0]), int(size[1]))
        k = self.intrinsics.detach().cpu().double().numpy()
        k_view = (float(k[0][0]) * W / self.cam.image_width, float(k[1][1]) * H / self.cam.image_height,
                  float(k[0][2]) * W / self.cam.image_width, float(k[1][2]) * H / self.cam.image_height)
        if frames is None:
            frames = list(self.keyframe_time_indices) or list(range(self.frames_seen))
        with torch.no_grad():
            result = mesh_mod.extract_mesh(self.engine, frames, (W, H), k_view, first_w2c=self.first_frame_w2c.contiguous(), method=method, **kwargs)
            result = _simplified(result, simplify, self.engine.dev)
        if path is not None:
            from .export import save_mesh_ply
            save_mesh_ply(path, result.vertices.cpu().numpy(), result.faces.cpu().numpy(), result.colors.cpu().numpy())
        if views is not None:
            from . import mesh_view
            from .post_opt import estimated_w2c
            first = self.first_frame_w2c.detach().double().cpu().numpy().reshape(4, 4)
            frames = list(frames)
            numbers = [n if isinstance(fr, torch.Tensor) else int(fr) for n, fr in enumerate(frames)]          # (a w2c: its place in the list)
            poses = np.stack([fr.detach().double().cpu().numpy().reshape(4, 4) if isinstance(fr, torch.Tensor)
                              else estimated_w2c(self.engine.params, int(fr)).double().cpu().numpy() @ first for fr in frames])
            mesh_view.render_trajectory(result, poses, views, k_view, (W, H), device=self.engine.dev, numbers=numbers, mode=views_mode)
        return result

    # ------------------------------------------------------------------ a picture of the map (csrc/view.hip)
    def render_view(self, w2c=None, follow=False, time_idx=None, size=None, intrinsics=None, mode="color", background=(0.0, 0.0, 0.0),
                    to_host=False, cameras=False, frusta="current", **kwargs):
        """The map as it is now, as display bytes: ``FusedEngine.render_view`` on a view camera the session creates on first use
        (``size`` = (height, width), default the loop's; fixed by the first call).  The pose is one of: ``w2c`` (float32 [4, 4] on the
        device), ``follow=True`` -- the latest estimated pose seen from 0.5 m behind it, ``offset . first_frame_w2c . rel_w2c[latest]``
        with the reference's online viewer's offset --, or ``time_idx``, the estimated pose of that frame.  ``intrinsics`` default
        to the loop's, scaled to ``size``.  Further keywords (``depth_range``, ``lut``, ``max_timestep``, ``points``, ``offset``,
        ``near``, ``far``, ``point_size``, ``line_width``, ``occlude``, ``overlay_planes``; ``mode="centers"``) go to the engine's
        method; nothing is read on the host for the picture.

        ``cameras=True`` draws the session's own run so far into the picture (csrc/viewoverlay.hip): the estimated trajectory up to the
        latest frame and, with ``frusta="current"`` (the online viewer's picture), the latest camera's frustum -- ``"all"``: every
        camera's so far, ``None``: none.  The segments are rebuilt from the pose parameters on the loop's stream at every call (one
        small launch, no host read); the ``view.RunOverlay`` behind it is made at the first such call.

        Returns the engine's ``ViewImage`` (tensors on the device, overwritten by the next call).  ``to_host=True``: returns a
        ``HostView(array, event, truncated)`` instead -- ``rgb8`` and the truncation flag copied on the loop's stream into one of two
        pinned slots used in turn; ``array`` is that slot's numpy view [H, W, 3] uint8, valid once ``event.synchronize()`` returns and
        until the call after next.  The CALLER waits for the event; ``add_frame`` / ``add_raw_frame`` never do.  Between frames and
        after ``finish()``; engine "fused" only.

        The view's lists are sized for the map of the first call and are exact lists (scan, scatter and sort launches) until
        ``view_check_overflow()`` has digested a render: call it once the first picture has been read, and again whenever
        ``truncated`` comes back non-zero (the map outgrew the lists), then render again."""
        if not self.fused:
            raise NotImplementedError("render_view needs engine='fused'")
        if self.engine is None:
            raise RuntimeError("render_view before the first frame: there is no map")
        eng = self.engine
        V = self._view
        if V is None:
            H, W = (self.cam.image_height, self.cam.image_width) if size is None else (int(size[0]), int(size[1]))
            k = self.intrinsics.detach().cpu().double().numpy()
            k_view = (float(k[0][0]) * W / self.cam.image_width, float(k[1][1]) * H / self.cam.image_height,
                      float(k[0][2]) * W / self.cam.image_width, float(k[1][2]) * H / self.cam.image_height)
            from .view import follow_offset
            V = self._view = dict(view=eng.view_camera(W, H), k=k_view, slots=[None, None], events=[None, None], turn=0,
                                  follow=follow_offset())
        elif size is not None and (int(size[0]), int(size[1])) != (V['view'].H, V['view'].W):
            raise ValueError(f"the session's view is {V['view'].H} x {V['view'].W}: its size is fixed by the first render_view")
        if sum((w2c is not None, bool(follow), time_idx is not None)) != 1:
            raise ValueError("render_view takes one of w2c, follow=True, time_idx")
        if follow:
            time_idx = self.frames_seen - 1
            kwargs.setdefault('offset', V['follow'])
        pose = dict(w2c=w2c) if w2c is not None else dict(time_idx=time_idx, first_w2c=self.first_frame_w2c)
        if cameras:
            if 'overlay' not in V:
                from .view import RunOverlay
                V['first_w2c'] = self.first_frame_w2c.contiguous()
                V['overlay'] = RunOverlay(eng, eng.num_frames, first_w2c=V['first_w2c'], intrinsics=self.intrinsics.detach().cpu().double().numpy(),
                                          size=(self.cam.image_width, self.cam.image_height))
            latest = self.frames_seen - 1
            kwargs.update(overlay=V['overlay'].refresh(latest), overlay_upto=latest, frusta=frusta)
        with torch.no_grad():
            image = eng.render_view(V['view'], intrinsics=V['k'] if intrinsics is None else intrinsics, mode=mode,
                                    background=background, **pose, **kwargs)
        if not to_host:
            return image
        turn = V['turn']
        V['turn'] ^= 1
        if V['slots'][turn] is None:
            V['slots'][turn] = (torch.empty(tuple(image.rgb8.shape), dtype=torch.uint8, pin_memory=True),
                                torch.zeros(1, dtype=torch.int32, pin_memory=True))
            V['events'][turn] = torch.cuda.Event()
        pixels, flag = V['slots'][turn]
        pixels.copy_(image.rgb8, non_blocking=True)
        flag.copy_(image.truncated, non_blocking=True)
        V['events'][turn].record(torch.cuda.current_stream(self.dev))
        return HostView(pixels.numpy(), V['events'][turn], flag.numpy())

    def view_check_overflow(self):
        """The digest of the session's view camera (``ViewCamera.check_overflow``: two small host reads, between frames): True when its
        renders since the last call ran on lists that did not fit -- they have been grown; render again.  Otherwise the list
        statistics are learnt and later views take the bucketed lists (no scan, scatter and sort launches)."""
        if self._view is None:
            raise RuntimeError("view_check_overflow before the first render_view")
        return self._view['view'].check_overflow()

    # ------------------------------------------------------------------ the raw path's buffers
    @staticmethod
    def _as_tensor(x, name, dtypes):
        t = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
            got = t.dtype if isinstance(t, torch.Tensor) else type(x).__name__
            raise ValueError(f"{name} must be an array or tensor of {' or '.join(str(d).replace('torch.', '') for d in dtypes)} (got {got})")
        return t

    def _raw_setup(self, rgb, raw, intrinsics):
        """Sizes, scaled intrinsics and -- on a HIP device -- every buffer of the raw path, from its first frame."""
        data = self.config.get('data') or {}
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        if self.device is not None:
            dev = self.device
        elif rgb.device.type == "cuda":
            dev = rgb.device
        else:
            dev = torch.device(self.config.get('primary_device', "cuda:0"))
        for name, t in (("rgb_u8", rgb), ("depth_raw", raw)):
            if t.device.type != "cpu" and t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the session runs on {dev}")
        size = lambda which: (int(data[f"{which}_image_height"]), int(data[f"{which}_image_width"])) \
            if f"{which}_image_height" in data else None                                                        # noqa: E731
        full = size("desired") or (H, W)
        k = torch.as_tensor(intrinsics, dtype=torch.float32)
        scaled = lambda s: slam.scale_intrinsics(k, s[0] / H, s[1] / W).to(dev)                                   # noqa: E731
        R = dict(device=dev, shapes=((H, W), tuple(raw.shape), raw.dtype), full=full, k_full=scaled(full), planes={})
        for which, key in (('tracking', "tracking"), ('densify', "densification")):
            s = size(key)
            R[which] = None if (s is None or s == full) else s          # (equal sizes mean "not separate": scripts/splatam.py:498-517)
            R['k_' + which] = None if R[which] is None else scaled(R[which])
        if dev.type == "cuda":
            for which in ('full', 'tracking', 'densify'):
                if R[which] is not None:
                    h, w = R[which]
                    R['planes'][which] = (torch.empty(3, h, w, dtype=torch.float32, device=dev), torch.empty(1, h, w, dtype=torch.float32, device=dev))
            R['slots'], R['turn'] = (_StagingSlot(), _StagingSlot()), 0
            R['dev_rgb'] = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            R['dev_depth'] = torch.empty(tuple(raw.shape), dtype=raw.dtype, device=dev)
        return R

    def _upload(self, rgb, raw):
        """The raw frame on the device: arrays that are there already as they are, host arrays through this turn's pinned slot."""
        R = self._raw
        if rgb.device.type == "cuda" and raw.device.type == "cuda":
            return rgb, raw
        slot = R['slots'][R['turn']]
        R['turn'] ^= 1
        if slot.used:
            slot.busy.synchronize()                      # (the upload that last read this slot has finished)
        out = []
        for name, t, target in (("rgb", rgb, R['dev_rgb']), ("depth", raw, R['dev_depth'])):
            if t.device.type == "cuda":
                out.append(t)
                continue
            if getattr(slot, name) is None:
                setattr(slot, name, torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True))
            getattr(slot, name).copy_(t)
            target.copy_(getattr(slot, name), non_blocking=True)
            out.append(target)
        if slot.busy is None:
            slot.busy = torch.cuda.Event()               # (one event per slot, recorded again by every upload from it)
        slot.busy.record(torch.cuda.current_stream(R['device']))
        slot.used = True
        return out[0], out[1]

    # ------------------------------------------------------------------ set-up: the first frame (scripts/splatam.py:455-652)
    def _start(self, dev, im0, depth0, intr0, pose0, tracking_frames, densify_frames, densify0):
        from . import dist as sdist
        config, num_frames = self.config, self.num_frames
        if sdist.world_size() > 1 and (tracking_frames is not None or densify_frames is not None):
            raise NotImplementedError("tracking / densification at resolutions of their own is not supported in the multi-rank frame loop")
        if pose0 is None:
            pose0 = torch.eye(4)                        # (the live demo's first frame IS the world frame: iphone_demo.py:231)
        if self.fused:
            # first frame on the device: an empty capacity-managed map + one append of every valid-depth pixel
            # (splat_map_add_new_gaussians, SPLAT_ADD_VALID_DEPTH) = get_pointcloud + initialize_params of the reference
            from .fused import FusedEngine
            intrinsics = intr0[:3, :3]
            first_frame_w2c = torch.linalg.inv(pose0).to(dev).float().contiguous()
            H, W = im0.shape[1], im0.shape[2]
            cam = slam.setup_camera(W, H, intrinsics.cpu().numpy(), first_frame_w2c.detach().cpu().numpy(), device=dev)
            cols = 1 if self.dist_kind == "isotropic" else 3
            rots = torch.zeros(1, 4, num_frames, device=dev)
            rots[:, 0, :] = 1.0
            z = lambda *shape: torch.nn.Parameter(torch.zeros(*shape, device=dev))      # noqa: E731
            params = {'means3D': z(0, 3), 'rgb_colors': z(0, 3), 'unnorm_rotations': z(0, 4), 'logit_opacities': z(0, 1),
                      'log_scales': z(0, cols), 'cam_unnorm_rots': torch.nn.Parameter(rots), 'cam_trans': z(1, 3, num_frames)}
            variables = {k: torch.zeros(0, device=dev) for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep')}
            variables['scene_radius'] = torch.max(depth0 if densify0 is None else densify0[1]) / config['scene_radius_depth_ratio']
            cap = self.gaussian_capacity or int(H * W * 2.5) + 65536
            eng = FusedEngine(params, cam, gaussian_capacity=cap, variables=variables)
            eng.keep_map_grads = False      # (a mapping iteration's gradients are discarded after its step: /root/reference/scripts/splatam.py:860-861)
            self.engine = eng
        else:
            params, variables, intrinsics, first_frame_w2c, cam = pipeline.initialize_first_timestep(
                None, num_frames, config['scene_radius_depth_ratio'], config['mean_sq_dist_method'], self.dist_kind,
                device=dev, densify_frame=densify0, first=(None, None, intr0, pose0.to(dev)), planes=(im0, depth0))
            dev = params['means3D'].device
            first_frame_w2c = first_frame_w2c.to(dev).float().contiguous()
        # the cameras of the reduced resolutions: their own size and intrinsics at the FIRST frame's pose (scripts/splatam.py:191, 586)
        for frames in (tracking_frames, densify_frames):
            if frames is not None:
                frames.cam = slam.setup_camera(frames.size[1], frames.size[0], frames.intrinsics.cpu().numpy(),
                                               first_frame_w2c.detach().cpu().numpy(), device=dev)
                if self.fused:
                    self.engine.add_camera(frames.cam)           # one map, a camera per resolution
        if self.fused:
            if densify0 is None:
                self.engine.select_camera(cam)
                self.engine.add_valid_depth_points(im0, depth0, intrinsics, first_frame_w2c)
            else:
                self.engine.add_valid_depth_points(densify0[0], densify0[1], densify0[2], first_frame_w2c, cam=densify_frames.cam)
        self.scene_radius = variables['scene_radius']
        self.params, self.variables, self.cam, self.dev = params, variables, cam, dev
        self.intrinsics, self.first_frame_w2c = intrinsics, first_frame_w2c
        self._tracking_frames, self._densify_frames = tracking_frames, densify_frames
        self._densify0 = None if densify0 is None else (densify0[0], densify0[1])
        self._phase = pipeline._PhaseTimer(dev)
        self._sync_prepare = tracking_frames is not None or densify_frames is not None
        if self.plugged:
            from . import plugin
            self._installed = plugin.install(slam, map_edits=self.engine_name == "plugin_map_edits")
        self._t_frame = time.perf_counter()             # (the set-up is not part of the first frame's time)

    def _curr_data(self, time_idx, im, depth):
        return {'cam': self.cam, 'im': im, 'depth': depth, 'id': time_idx, 'intrinsics': self.intrinsics, 'w2c': self.first_frame_w2c}

    # ------------------------------------------------------------------ the loop body (scripts/splatam.py:654-905)
    @staticmethod
    def _pose_is_finite(pose, known=None):
        """No keyframe for a pose with inf or NaN.  ``known``: the driver's answer from a host copy of the poses; otherwise a pose on
        the host is looked at there, and only a pose on the device is read back (16 floats, on keyframe frames)."""
        if pose is None:
            return True
        if known is not None:
            return bool(known)
        return bool(torch.isfinite(pose).all())

    def _step(self, time_idx, curr_data, tracking_curr_data, densify_curr_data, gt_pose, owned, pose_finite=None):
        """One pass of the frame loop on prepared planes.  ``owned``: the planes are the session's buffers, written again by the next
        frame -- a keyframe keeps a copy."""
        from . import dist as sdist
        config, tcfg, mcfg = self.config, self.config['tracking'], self.config['mapping']
        params, variables, stats, phase, eng, dev = self.params, self.variables, self.stats, self._phase, self.engine, self.dev
        fused, keyframe_list = self.fused, self.keyframe_list
        color, depth = curr_data['im'], curr_data['depth']
        both = lambda data: None if data is curr_data else (data['im'], data['depth'])           # noqa: E731
        self.last_frame = {'full': (color, depth), 'tracking': both(tracking_curr_data),
                           'densify': self._densify0 if time_idx == 0 else both(densify_curr_data)}
        # (with one resolution the phase is the permute / 255 the loop always did: timed on the host, no synchronisation added)
        if self._sync_prepare:
            phase._sync()
        phase.frame["prepare_frames"] = 1e3 * (time.perf_counter() - self._t_frame)
        t_frame = self._t_frame
        # what the loop DECIDED on this frame, engine independent (host integers only; tests/loop_trace.py derives the same table
        # from a recording of the reference's own rgbd_slam)
        decided = dict(time_idx=time_idx, tracking_iters=0, rows_after_add=None, selected=None, views=[], prunes=[], rows_end=None,
                       keyframe=False)
        stats['decisions'].append(decided)
        if time_idx > 0:
            slam.initialize_camera_pose(params, time_idx, forward_prop=tcfg['forward_prop'])

        # ---------------- tracking (scripts/splatam.py:676-744)
        if fused and self._tracking_frames is not None and time_idx > 0 and not tcfg['use_gt_poses'] and not eng.lists_known(tracking_curr_data):
            # a tracking camera of its own whose list statistics are unknown (its first frame, or an edit dropped them): one probe
            # render sizes its lists, instead of a flagged first iteration and a phase run again
            with phase("relearn_lists"):
                eng.relearn_lists(tracking_curr_data, time_idx)
        with phase("tracking"):
            t0 = time.perf_counter()
            if time_idx > 0 and not tcfg['use_gt_poses']:
                if self.plugged:
                    n_track, variables = pipeline._track_frame_statements(params, variables, tracking_curr_data, time_idx, tcfg)
                    self.variables = variables
                else:
                    n_track = pipeline._track_frame(params, variables, tracking_curr_data, time_idx, tcfg, eng, stats)
                stats['tracking_iters'] += n_track
                decided['tracking_iters'] = n_track
                sdist.broadcast_pose(params, time_idx)              # replicas: one pose for the map edits that follow
            elif time_idx > 0:
                with torch.no_grad():
                    rel = torch.linalg.inv(gt_pose).to(dev)
                    params['cam_unnorm_rots'][..., time_idx] = pipeline._matrix_to_quaternion(rel[:3, :3])
                    params['cam_trans'][..., time_idx] = rel[:3, 3]
        stats['tracking_s'] += time.perf_counter() - t0

        # ---------------- densification + keyframe mapping (scripts/splatam.py:768-891)
        if time_idx == 0 or (time_idx + 1) % config['map_every'] == 0:
            t0 = time.perf_counter()
            if mcfg['add_new_gaussians'] and time_idx > 0:
                with phase("add_new_gaussians"):
                    if fused:
                        eng.add_new_gaussians(densify_curr_data, mcfg['sil_thres'], time_idx, config['mean_sq_dist_method'], self.dist_kind)
                    else:
                        params, variables = slam.add_new_gaussians(params, variables, densify_curr_data, mcfg['sil_thres'], time_idx,
                                                                   config['mean_sq_dist_method'], self.dist_kind)
                        self.params, self.variables = params, variables
                decided['rows_after_add'] = int(params['means3D'].shape[0])
                sdist.assert_replicated_count(int(params['means3D'].shape[0]), f"add_new_gaussians (frame {time_idx})", dev)
            with phase("keyframe_selection"), torch.no_grad():
                curr_w2c = pipeline._est_w2c(params, time_idx)
                selected = pipeline.keyframe_selection_overlap(depth, curr_w2c, self.intrinsics.to(dev), keyframe_list[:-1],
                                                               config['mapping_window_size'] - 2)
                if len(keyframe_list) > 0:
                    selected.append(len(keyframe_list) - 1)
                selected.append(-1)
                decided['selected'] = [int(x) for x in selected[:-1 - (1 if len(keyframe_list) > 0 else 0)]]
            if fused and not eng.lists_known(curr_data):
                with phase("relearn_lists"):
                    eng.relearn_lists(curr_data, time_idx)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            t_loop = time.perf_counter()                        # the reference's mapping timer starts here (scripts/splatam.py:825)
            t_prune0 = phase.frame.get("prune", 0.0)
            with phase("mapping_iterations"):
                pipeline._map_frame(params, variables, curr_data, time_idx, selected, keyframe_list, mcfg, eng,
                                    self.scene_radius if fused else None, stats, phase, decided)
            # (the prune phase is timed inside the loop: report the iterations without it)
            phase.frame["mapping_iterations"] -= phase.frame.get("prune", 0.0) - t_prune0
            stats['mapping_iters'] += mcfg['num_iters']
            stats['mapping_s'] += time.perf_counter() - t0
            stats['mapping_loop_s'] += time.perf_counter() - t_loop

        # ---------------- keyframe list (scripts/splatam.py:893-905): not for a frame whose ground-truth pose is inf / NaN
        w2c = None
        if time_idx == 0 or (time_idx + 1) % config['keyframe_every'] == 0 or time_idx == self.num_frames - 2:
            if self._pose_is_finite(gt_pose, pose_finite):
                with phase("keyframe_store"), torch.no_grad():
                    w2c = pipeline._est_w2c(params, time_idx)
                    kept = (color.clone(), depth.clone()) if owned else (color, depth)
                    keyframe_list.append({'id': time_idx, 'est_w2c': w2c, 'color': kept[0], 'depth': kept[1]})
                    self.keyframe_time_indices.append(time_idx)
                    decided['keyframe'] = True
        decided['rows_end'] = int(params['means3D'].shape[0])
        stats['num_gaussians'].append(int(params['means3D'].shape[0]))
        stats['phase_ms'].append(phase.next_frame())
        if self.return_pose:
            with torch.no_grad():                       # (a tensor of the caller's own: the keyframe list keeps its one)
                w2c = pipeline._est_w2c(params, time_idx) if w2c is None else w2c.clone()
        stats['frame_s'].append(time.perf_counter() - t_frame)
        self._t_frame = None
        self.frames_seen = time_idx + 1
        if self.verbose:
            print(f"frame {time_idx}: {stats['num_gaussians'][-1]} Gaussians, keyframes {self.keyframe_time_indices}", flush=True)
        return dict(time_idx=time_idx, w2c=w2c if self.return_pose else None, tracking_iters=decided['tracking_iters'],
                    num_gaussians=stats['num_gaussians'][-1], keyframe=decided['keyframe'], phase_ms=stats['phase_ms'][-1])
