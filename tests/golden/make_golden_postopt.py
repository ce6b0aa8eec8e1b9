"""Generates tests/golden/postopt_reference.npz by EXECUTING THE REFERENCE'S OWN refinement script --
/root/reference/scripts/post_splatam_opt.py, the file imported as it is: its ``get_loss_gs`` (:111-147), ``get_expon_lr_func``
(utils/gs_external.py:269-302) and its loop ``rgbd_slam`` (:160-385) with ``densify`` (utils/gs_external.py:191-257) -- on CPU in
this container, and recording what it computed.  tests/test_postopt_cpu.py (CPU, on the oracle) and tests/test_gpu_postopt.py (HIP)
hold ``splatam_amd.slam.get_loss_gs``, the learning-rate schedule and ``splatam_amd.post_opt.post_splatam_opt`` to this recording.

What is the reference's and what is not is what tests/golden/make_golden_loop.py says: the module and ``utils/*`` are the
reference's files; third-party imports that do not exist offline are empty stand-ins; ``.cuda()`` / ``device="cuda"`` go to the
CPU; ``diff_gaussian_rasterization`` is this repository's C ORACLE (oracle/c_ref.CRasterizer); ``get_dataset`` returns the recorded
synthetic frames, ``eval`` is a no-op, ``save_params`` hands the final dict to the recorder.  The configuration is the reference's
own configs/replica/post_splatam_opt.py with the sizes reduced -- every override is in ``LOOP_OVERRIDES``.

Run:  python tests/golden/make_golden_postopt.py      (needs /root/reference; not needed on the GPU box)
"""
import copy
import importlib.machinery
import importlib.util
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden_loop as MGL  # noqa: E402  (the device shim, the stand-in finder, the oracle renderer module)

MGL.STAND_INS = MGL.STAND_INS + ("matplotlib",)


def load_reference_script():
    """scripts/post_splatam_opt.py as a module object (its ``__main__`` block does not run)."""
    for name in list(sys.modules):
        if name.split(".")[0] in MGL.STAND_INS:
            del sys.modules[name]
    sys.meta_path.insert(0, MGL._StandInFinder())
    sys.modules["diff_gaussian_rasterization"] = MGL.oracle_renderer_module()
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_post_splatam_opt", os.path.join(REF, "scripts", "post_splatam_opt.py"))
    module = importlib.util.module_from_spec(spec)
    with open(os.devnull, "w") as null:
        out, sys.stdout = sys.stdout, null
        try:
            spec.loader.exec_module(module)
        finally:
            sys.stdout = out
    return module


# ---- the scene: a finished map of ~600 isotropic Gaussians, three frames at distinct, non-identity poses -------------------------
def make_scene(n, W, H, f, seed, frames=3):
    """(params of the finished run, list of (im [3,H,W], depth [1,H,W]) rendered on the oracle from poses perturbed against the map's)."""
    from oracle import c_ref
    from oracle import raster_ref as R
    from splatam_amd import slam
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    p = R.synthetic_cloud(n, W, H, f, f, cx, cy, seed=seed, anisotropic=False)
    g = torch.Generator().manual_seed(seed + 100)
    rots = torch.zeros(1, 4, frames)
    rots[:, 0, :] = 1.0
    rots += 0.02 * torch.randn(1, 4, frames, generator=g)
    trans = 0.03 * torch.randn(1, 3, frames, generator=g)
    params = dict(p)
    params['cam_unnorm_rots'], params['cam_trans'] = rots, trans
    cam = R.make_camera(W, H, f, f, cx, cy)
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    out = []
    try:
        with torch.no_grad():
            for t in range(frames):
                P2 = {k: v.clone() for k, v in params.items()}
                P2['cam_trans'][..., t] += torch.tensor([[0.01, -0.005, 0.005]])
                P2['rgb_colors'] = (P2['rgb_colors'] + 0.05 * torch.randn(P2['rgb_colors'].shape, generator=g)).clamp(0, 1)
                tg = slam.transform_to_frame(P2, t, False, False)
                im, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2rendervar(P2, tg))
                ds, _, _ = slam.Renderer(raster_settings=cam)(**slam.transformed_params2depthplussilhouette(P2, torch.eye(4), tg))
                depth = torch.where(ds[1:2] > 0.5, ds[0:1] / ds[1:2].clamp_min(1e-6), torch.zeros_like(ds[0:1]))
                out.append((im.clamp(0, 1).contiguous(), depth.contiguous()))
    finally:
        slam.Renderer = saved
    return params, out, (W, H, f, cx, cy)


def holed_depth(depth):
    """The frame of the loss fixtures: a block of zero depth over about a fifth of the image and ONE pixel of negative depth (on a
    pixel the map covers)."""
    d = depth.clone()
    H, W = d.shape[1:]
    d[:, : H // 2, : (2 * W) // 5] = 0.0              # 1/2 x 2/5 = a fifth
    ys, xs = torch.nonzero(d[0] > 0, as_tuple=True)
    i = len(ys) // 2
    d[0, ys[i], xs[i]] = -d[0, ys[i], xs[i]]
    return d, (int(ys[i]), int(xs[i]))


# ---- (1) get_loss_gs -----------------------------------------------------------------------------------------------------------------
def record_loss(S, out):
    from utils import recon_helpers as ref_recon          # the reference's setup_camera
    for name, (n, W, H, f, seed) in {"a": (700, 80, 56, 70.0, 2), "b": (500, 64, 48, 55.0, 5)}.items():
        params, frames, (W, H, f, cx, cy) = make_scene(n, W, H, f, seed)
        t = 1
        im, depth = frames[t]
        depth, neg = holed_depth(depth)
        k = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float32)
        q = torch.nn.functional.normalize(params['cam_unnorm_rots'][..., t])
        w2c = torch.eye(4)
        w2c[:3, :3] = S.build_rotation(q)
        w2c[:3, 3] = params['cam_trans'][..., t]
        cam = ref_recon.setup_camera(W, H, k, w2c.numpy())
        P = {kk: torch.nn.Parameter(v.clone()) for kk, v in params.items()}
        variables = {'max_2D_radius': torch.zeros(n), 'means2D_gradient_accum': torch.zeros(n), 'denom': torch.zeros(n)}
        curr = {'cam': cam, 'im': im, 'depth': depth, 'id': t, 'intrinsics': k, 'w2c': w2c}
        loss, variables, wl = S.get_loss_gs(P, curr, variables, dict(im=0.5, depth=1.0))
        loss.backward()
        for kk, v in params.items():
            out[f"loss/{name}/param/{kk}"] = v.numpy()
        out[f"loss/{name}/meta"] = np.array([n, W, H, f, cx, cy, t, neg[0], neg[1]], dtype=np.float64)
        out[f"loss/{name}/im"], out[f"loss/{name}/depth"], out[f"loss/{name}/w2c"] = im.numpy(), depth.numpy(), w2c.numpy()
        out[f"loss/{name}/loss"] = np.array([loss.item(), wl['im'].item(), wl['depth'].item()])
        for kk, v in P.items():
            out[f"loss/{name}/grad/{kk}"] = (torch.zeros_like(v) if v.grad is None else v.grad).numpy()
        out[f"loss/{name}/max_2D_radius"] = variables['max_2D_radius'].numpy()
        out[f"loss/{name}/means2D_grad"] = variables['means2D'].grad.numpy()
        frac = float((depth == 0).float().mean())
        print(f"[loss/{name}] loss {loss.item():.6f} im {wl['im'].item():.6f} depth {wl['depth'].item():.6f}; zero-depth pixels {100 * frac:.1f} %, "
              f"negative pixel {neg}, valid (!= 0) {int((depth != 0).sum())}, > 0 {int((depth > 0).sum())}")


# ---- (2) the learning-rate schedule ----------------------------------------------------------------------------------------------------
def record_lr(S, out):
    max_steps = 15000
    steps = np.array([1, 2, max_steps // 2, max_steps])
    out["lr/steps"], out["lr/args"] = steps, np.array([0.00032, 0.0000032, max_steps], dtype=np.float64)
    for mult in (0.01, 1.0):
        as_script = S.get_expon_lr_func(lr_init=0.00032, lr_final=0.0000032, lr_delay_mult=mult, max_steps=max_steps)       # (:284-287)
        delayed = S.get_expon_lr_func(lr_init=0.00032, lr_final=0.0000032, lr_delay_steps=100, lr_delay_mult=mult, max_steps=max_steps)
        out[f"lr/mult{mult}/script"] = np.array([as_script(int(s)) for s in steps], dtype=np.float64)
        out[f"lr/mult{mult}/delay100"] = np.array([delayed(int(s)) for s in steps], dtype=np.float64)
    out["lr/disabled"] = np.array([S.get_expon_lr_func(0.0, 0.0)(5), as_script(-1)], dtype=np.float64)


# ---- (3) the loop --------------------------------------------------------------------------------------------------------------------
LOOP_SCENE = dict(n=600, W=64, H=48, f=55.0, seed=9)
LOOP_OVERRIDES = dict(
    primary_device="cpu", use_wandb=False, report_iter_progress=False, workdir="unused", run_name="postopt", seed=0,
    data=dict(basedir="unused", sequence="synthetic", desired_image_height=48, desired_image_width=64, start=0, end=-1, stride=1,
              num_frames=3, eval_stride=1, eval_num_frames=3),
    train=dict(num_iters_mapping=40,
               densify_dict=dict(start_after=5, densify_every=10, remove_big_after=20, reset_opacities_every=20, stop_after=40)))


def loop_config(overrides):
    path = os.path.join(REF, "configs", "replica", "post_splatam_opt.py")
    cfg = copy.deepcopy(importlib.machinery.SourceFileLoader("ref_postopt_config", path).load_module().config)

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v
    merge(cfg, overrides)
    cfg['data'].pop('gradslam_data_cfg')
    cfg['data']['dataset_name'] = "synthetic"
    cfg.pop('viz', None)
    cfg.pop('wandb', None)
    return cfg


def record_loop(S, out):
    from loop_trace import RecordedRGBDSequence
    sc = LOOP_SCENE
    params, frames, (W, H, f, cx, cy) = make_scene(sc['n'], sc['W'], sc['H'], sc['f'], sc['seed'])
    n = sc['n']
    k4 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    color = np.stack([(im.permute(1, 2, 0) * 255.0).numpy() for im, _ in frames]).astype(np.float32)
    depth = np.stack([d.permute(1, 2, 0).numpy() for _, d in frames]).astype(np.float32)
    depth[:, : H // 2, : (2 * W) // 5] = 0.0                 # (the zero-depth block, in every frame)
    poses = np.stack([np.eye(4, dtype=np.float32)] * len(frames))
    for t in range(1, len(frames)):                          # camera-to-world of the map's own poses (only the evaluation reads them)
        q = torch.nn.functional.normalize(params['cam_unnorm_rots'][..., t])
        w2c = np.eye(4, dtype=np.float32)
        w2c[:3, :3] = S.build_rotation(q)[0].numpy()
        w2c[:3, 3] = params['cam_trans'][0, :, t].numpy()
        poses[t] = np.linalg.inv(w2c)
    fr = {"loop/frames/color": color, "loop/frames/depth": depth, "loop/frames/intrinsics": k4, "loop/frames/poses": poses}
    out.update(fr)
    dataset = RecordedRGBDSequence(fr, "loop")
    # the params.npz of the finished run, with the entries the script drops
    ckpt = {kk: v.numpy() for kk, v in params.items()}
    ckpt['timestep'] = (np.arange(n) % len(frames)).astype(np.float32)
    ckpt['intrinsics'], ckpt['w2c'] = k4[:3, :3], np.eye(4, dtype=np.float32)
    ckpt['org_width'], ckpt['org_height'] = np.array(W), np.array(H)
    ckpt['gt_w2c_all_frames'] = np.stack([np.linalg.inv(p) for p in poses])
    ckpt['keyframe_time_indices'] = np.array([0, 2])
    for kk, v in ckpt.items():
        out[f"loop/ckpt/{kk}"] = v
    tmp = tempfile.mkdtemp()
    ckpt_path = os.path.join(tmp, "params.npz")
    np.savez(ckpt_path, **ckpt)

    for run_name, dens in (("dens", True), ("plain", False)):
        over = copy.deepcopy(LOOP_OVERRIDES)
        over['workdir'] = tmp
        over['data']['param_ckpt_path'] = ckpt_path
        over['train']['use_gaussian_splatting_densification'] = dens
        cfg = loop_config(over)
        views, losses, rows, final = [], [], [], {}
        saved = {kk: getattr(S, kk) for kk in ("get_dataset", "eval", "save_params", "tqdm", "get_loss_gs", "densify")}
        orig_loss, orig_densify = S.get_loss_gs, S.densify

        def get_loss_gs(p, curr_data, variables, w):
            o = orig_loss(p, curr_data, variables, w)
            views.append(int(curr_data['id']))
            losses.append(float(o[0]))
            return o

        def densify(p, variables, optimizer, it, dd):
            before = int(p['means3D'].shape[0])
            o = orig_densify(p, variables, optimizer, it, dd)
            if it <= dd['stop_after'] and it >= dd['start_after'] and it % dd['densify_every'] == 0:
                rows.append((it, before, int(o[0]['means3D'].shape[0])))
            return o
        S.get_dataset = lambda **kw: dataset
        S.eval = lambda *a, **kw: None
        S.save_params = lambda p, output_dir: final.update(p)
        S.tqdm = lambda it=None, *a, **kw: mock.MagicMock() if it is None else MGL._Quiet(it)
        S.get_loss_gs, S.densify = get_loss_gs, densify
        try:
            S.seed_everything(seed=cfg['seed'])                 # scripts/post_splatam_opt.py:399
            S.rgbd_slam(copy.deepcopy(cfg))
        finally:
            for kk, v in saved.items():
                setattr(S, kk, v)
        cfg['workdir'], cfg['data']['param_ckpt_path'] = "unused", "unused"
        out[f"loop/{run_name}/config"] = np.array(json.dumps(cfg))
        out[f"loop/{run_name}/views"], out[f"loop/{run_name}/losses"] = np.array(views), np.array(losses, dtype=np.float64)
        out[f"loop/{run_name}/rows"] = np.array(rows, dtype=np.int64).reshape(-1, 3)
        for kk, v in final.items():
            out[f"loop/{run_name}/final/{kk}"] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        print(f"[loop/{run_name}] views {views}\n[loop/{run_name}] losses {np.round(losses, 5).tolist()}\n[loop/{run_name}] densifications {rows}; "
              f"{final['means3D'].shape[0]} Gaussians at the end; saved keys {sorted(final)}")


def main():
    MGL.install_device_shim()
    from oracle import c_ref
    c_ref.build()
    S = load_reference_script()
    print(f"reference module: {S.__file__}; get_loss_gs at line {S.get_loss_gs.__code__.co_firstlineno}; torch {torch.__version__}")
    out = {}
    record_loss(S, out)
    record_lr(S, out)
    record_loop(S, out)
    path = os.path.join(HERE, "postopt_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
