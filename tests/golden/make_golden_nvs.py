"""Generates tests/golden/nvs_reference.npz by EXECUTING THE REFERENCE'S OWN ``eval_nvs`` -- /root/reference/utils/eval_helpers.py:626-825,
the file imported as it is -- on CPU in this container, on the held-out split of tests/nvs_ref.py (13 items of 240 x 176: the first
training frame and twelve held-out frames at poses off the training trajectory; a hole in the map, a rectangle of invalid depth per
frame; an isotropic and an anisotropic map; both mask variants; eval_every 1 and 3; one case whose first pose is a general rigid
matrix).  Only numbers are recorded; the frames are regenerated from the seeds by the tests.

Recorded per case and scored frame: psnr / rmse / l1 as eval_nvs writes them into its eval_dir, the restated ms-ssim, the validity
flag of its valid_nvs_frames.npy, the held-out indices it scored (read off the names of the pictures it saves), the HOLE COUNT
-- eval_nvs forms it only inside its percentage; it is counted here by its expression ``(~(presence_sil_mask | ~valid_depth_mask)).sum()``
on the silhouette its own render call returned, and the generator asserts that the reference's flag follows from it -- and
``undecided``: the number of pixels with valid depth whose oracle silhouette lies within 1e-3 of sil_thres (ten times the project's
1e-4 plane tolerance): the pixels another renderer may decide the other way.

Stand-ins and device shim as tests/golden/make_golden_eval.py: ``diff_gaussian_rasterization`` is this repository's C oracle,
``ms_ssim`` the restatement of tests/eval_ref.py (recorded as ``ssim_restated_not_upstream``), the LPIPS network a function returning
NaN, cv2 a stand-in whose ``imwrite`` records the file names, the plots no-ops.

Asserted here, because the tests rely on it: every case scores at least two valid and two invalid frames, and every frame's
``|holes - 0.001 H W|`` exceeds its ``undecided`` count plus 8 pixels (no verdict hangs on a pixel a renderer could flip).

Run:  python tests/golden/make_golden_nvs.py      (needs /root/reference; not needed on the GPU box)
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden_loop as GL  # noqa: E402


def main():
    from oracle import c_ref
    from splatam_amd import slam
    from tests import eval_ref, nvs_ref
    GL.install_device_shim()
    GL.load_reference_module(GL.oracle_renderer_module())            # scripts/splatam.py imports utils/eval_helpers.py itself
    EH = sys.modules["utils.eval_helpers"]
    assert EH.__file__.startswith(GL.REF), EH.__file__
    EH.ms_ssim = lambda X, Y, data_range=1.0, size_average=True: eval_ref.ms_ssim_levels(X, Y)[2]
    EH.loss_fn_alex = lambda a, b: torch.tensor(float("nan"))
    EH.plot_rgbd_silhouette = lambda *a, **k: None
    EH.plt.savefig = lambda *a, **k: None
    EH.tqdm = lambda it, *a, **k: it
    written = []
    EH.cv2.imwrite = lambda path, *a, **k: written.append(path)

    renders = []
    oracle = EH.Renderer

    class Recording:
        """eval_nvs' Renderer: the oracle, with every output kept (per scored frame: depth + silhouette first, colour second)."""

        def __init__(self, raster_settings):
            self.inner = oracle(raster_settings=raster_settings)

        def __call__(self, **kw):
            out = self.inner(**kw)
            renders.append(out[0].detach().clone())
            return out
    EH.Renderer = Recording

    slam.Renderer = c_ref.CRasterizer                                # (the frames of tests/nvs_ref.py are made with the oracle too)
    s = nvs_ref.SCENE
    H, W = s['H'], s['W']
    limit = 0.001 * H * W
    out = {}
    for name in nvs_ref.CASES:
        dataset, params, (mapping_iters, add_new), every = nvs_ref.case(name, "cpu")
        written.clear()
        renders.clear()
        with tempfile.TemporaryDirectory() as d, torch.no_grad():
            EH.eval_nvs(dataset, params, len(dataset), d, sil_thres=nvs_ref.SIL_THRES, mapping_iters=mapping_iters, add_new_gaussians=add_new,
                        eval_every=every, save_frames=True)
            for file, k in (("psnr.txt", "psnr"), ("rmse.txt", "rmse"), ("l1.txt", "l1"), ("ssim.txt", "ssim_restated_not_upstream")):
                out[f"{name}/{k}"] = np.atleast_1d(np.loadtxt(os.path.join(d, file)))
            valid = np.load(os.path.join(d, "valid_nvs_frames.npy"))
            pictures = sorted(os.path.relpath(p, d) for p in written)
        frames = sorted(int(os.path.basename(p)[len("splatam_"):-len(".png")]) for p in pictures if p.startswith("rendered_rgb" + os.sep))
        assert len(frames) == len(valid) == len(out[f"{name}/psnr"]) and len(renders) == 2 * len(frames), (frames, len(valid), len(renders))
        holes, undecided = [], []
        for i, k in enumerate(frames):
            sil = renders[2 * i][1]
            depth_ok = dataset[k + 1][1][..., 0] > 0
            presence = sil > nvs_ref.SIL_THRES
            holes.append(int((~(presence | ~depth_ok)).sum()))
            undecided.append(int((depth_ok & ((sil - nvs_ref.SIL_THRES).abs() <= 1e-3)).sum()))
            # the reference's verdict, from ITS expression, follows from the count
            percent = torch.tensor(holes[-1]) / (H * W) * 100
            assert bool(percent > 0.1) == (not bool(valid[i])), (name, k, holes[-1], valid[i])
            assert abs(holes[-1] - limit) > undecided[-1] + 8, (name, k, holes[-1], undecided[-1])
        assert int(valid.sum()) >= 2 and int((~valid).sum()) >= 2, (name, valid.tolist())
        out[f"{name}/frames"], out[f"{name}/valid"] = np.array(frames), valid.astype(bool)
        out[f"{name}/holes"], out[f"{name}/undecided"] = np.array(holes), np.array(undecided)
        # the picture names the tests expect of the package (only numbers are recorded)
        assert pictures == sorted(os.path.join(folder, f"{prefix}_{k:04d}.png") for k in frames
                                  for folder, prefix in (("rendered_rgb", "splatam"), ("rendered_depth", "splatam"), ("rgb", "gt"), ("depth", "gt"))), pictures
        print(name, "frames", frames, "valid", valid.astype(int).tolist(), "holes", holes, "undecided", undecided, "psnr",
              np.round(out[f"{name}/psnr"], 3).tolist(), "l1", np.round(out[f"{name}/l1"], 5).tolist())
    path = os.path.join(HERE, "nvs_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
