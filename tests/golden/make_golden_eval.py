"""Generates tests/golden/eval_reference.npz by EXECUTING THE REFERENCE'S OWN ``eval`` -- /root/reference/utils/eval_helpers.py:408-623,
the file imported as it is -- on CPU in this container: on the synthetic sequence of tests/eval_ref.py (``golden_case``: 12 frames of
240 x 176, a rectangle of invalid depth, a hole in the map, perturbed final poses, one NaN ground-truth pose), with eval_every = 1 and
= 5, once per mask variant.  Recorded: the per-frame psnr / rmse / l1 it writes into its eval_dir, the frames it evaluated, the
value of its ``evaluate_ate`` (and the trajectories it was given), and ``align``'s outputs for three seeded trajectories.
Only numbers are recorded; the frames are regenerated from the seed by the tests.

What is the reference's and what is not (stand-ins and device shim as tests/golden/make_golden_loop.py):
  * ``diff_gaussian_rasterization`` is this repository's C oracle;
  * ``pytorch_msssim`` does not exist offline: ``ms_ssim`` is served by the restatement in tests/eval_ref.py.  Its per-frame values
    are recorded as ``ssim_restated_not_upstream`` -- they pin nothing of upstream's package;
  * the LPIPS network is replaced by a function returning NaN (not recorded); ``plot_rgbd_silhouette`` and ``plt.savefig`` are no-ops;
  * ``eval`` swallows every failure of the trajectory error and reports 100.0: the generator asserts that ``evaluate_ate`` ran.

Run:  python tests/golden/make_golden_eval.py      (needs /root/reference; not needed on the GPU box)
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
    from tests import eval_ref
    GL.install_device_shim()
    GL.load_reference_module(GL.oracle_renderer_module())            # scripts/splatam.py imports utils/eval_helpers.py itself
    EH = sys.modules["utils.eval_helpers"]
    assert EH.__file__.startswith(GL.REF), EH.__file__
    EH.ms_ssim = lambda X, Y, data_range=1.0, size_average=True: eval_ref.ms_ssim_levels(X, Y)[2]
    EH.loss_fn_alex = lambda a, b: torch.tensor(float("nan"))
    EH.plot_rgbd_silhouette = lambda *a, **k: None
    EH.plt.savefig = lambda *a, **k: None
    EH.tqdm = lambda it, *a, **k: it

    slam.Renderer = c_ref.CRasterizer
    dataset, params = eval_ref.golden_case("cpu")
    out = {}
    seen, ate = [], []
    orig_ttf, orig_ate = EH.transform_to_frame, EH.evaluate_ate

    def transform_to_frame(p, time_idx, **k):
        seen.append(int(time_idx))
        return orig_ttf(p, time_idx, **k)

    def evaluate_ate(gt, est):
        v = orig_ate(gt, est)
        ate.append((torch.stack(gt).numpy(), torch.stack(est).numpy(), float(v)))
        return v
    EH.transform_to_frame, EH.evaluate_ate = transform_to_frame, evaluate_ate
    for vname, (mapping_iters, add_new) in eval_ref.GOLDEN_VARIANTS.items():
        for every in eval_ref.GOLDEN_EVERY:
            seen.clear()
            ate.clear()
            with tempfile.TemporaryDirectory() as d, torch.no_grad():
                EH.eval(dataset, params, len(dataset), d, sil_thres=eval_ref.GOLDEN_SIL_THRES, mapping_iters=mapping_iters,
                        add_new_gaussians=add_new, eval_every=every)
                key = f"{vname}/every{every}"
                for name, k in (("psnr.txt", "psnr"), ("rmse.txt", "rmse"), ("l1.txt", "l1"), ("ssim.txt", "ssim_restated_not_upstream")):
                    out[f"{key}/{k}"] = np.atleast_1d(np.loadtxt(os.path.join(d, name)))
            assert len(ate) == 1, "evaluate_ate failed inside eval (it would have reported 100.0)"
            assert ate[0][2] != 100.0 and ate[0][2] > 1e-4
            out[f"{key}/frames"] = np.array(seen)
            out[f"{key}/ate"] = np.array(ate[0][2])
            out[f"{key}/ate_gt_w2c"], out[f"{key}/ate_est_w2c"] = ate[0][0], ate[0][1]
            assert len(seen) == len(out[f"{key}/psnr"])
            print(key, "frames", seen, "psnr", np.round(out[f"{key}/psnr"], 3).tolist(), "l1", np.round(out[f"{key}/l1"], 5).tolist(),
                  "ate", ate[0][2], "poses used", ate[0][0].shape[0])
    g = np.random.default_rng(99)
    for i, n in enumerate((5, 12, 40)):
        model = g.normal(size=(3, n))
        ang = 0.3 + 0.2 * i
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
        data = R @ model + g.normal(size=(3, 1)) + 0.02 * g.normal(size=(3, n))
        rot, trans, err = EH.align(np.asmatrix(model), np.asmatrix(data))
        out[f"align/{i}/model"], out[f"align/{i}/data"] = model, data
        out[f"align/{i}/rot"], out[f"align/{i}/trans"], out[f"align/{i}/trans_error"] = np.asarray(rot), np.asarray(trans), np.asarray(err)
    path = os.path.join(HERE, "eval_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
