"""What scoring a held-out view costs (``evaluation.evaluate_novel_views``; csrc/evalmetrics.hip with the hole count).  A synthetic
sequence at 1200 x 680 -- the first training frame and ``--frames`` held-out frames at poses off the training trajectory, rendered once
and kept on the device -- is scored by a map that lacks the Gaussians of one region:

  device        the HIP path (one ``evaluate_view`` per frame, one table read)
  device+save   the same with ``save_frames=True`` (four PNGs per frame, encoded by the saver's threads)
  mirror        the torch mirror on the drop-in rasterizer (two renders + torch metrics and one host copy per frame)

each ``--repeats`` times after one warm-up call; one JSON line per form with the wall milliseconds per held-out frame (from the call
to the table read, dataset access and list learning included, as ``eval_ms_per_frame`` reports them).  ``--markdown PATH`` also
writes the lines as a fenced block for profiles/novel_view.md.  These figures are reported, not gated.

    python scripts/novel_view_run.py [--frames 8] [--gaussians 300000] [--repeats 3] [--markdown PATH]
"""
import argparse
import json
import math
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, F = 1200, 680, 600.0


class HeldOut:
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, t):
        return self.items[t]


def build(n_gaussians, frames):
    """(dataset, params): item 0 at the identity, then ``frames`` views turned by up to 3 degrees about seeded axes and shifted by a
    few centimetres; the map is the scene without the Gaussians of x in (0.2, 0.7), y in (-0.1, 0.35)."""
    import numpy as np
    import torch
    from splatam_amd import pipeline
    ds = pipeline.SyntheticRGBDSequence(n_gaussians, W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, num_frames=frames + 1, seed=5)
    rng = np.random.default_rng(11)
    for t in range(1, frames + 1):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = math.radians(1.0 + 2.0 * rng.random())
        q = [math.cos(ang / 2)] + list(math.sin(ang / 2) * axis)
        ds._scene['cam_unnorm_rots'][0, :, t] = torch.tensor(q, dtype=torch.float32)
        ds._scene['cam_trans'][0, :, t] = torch.tensor(rng.uniform(-0.06, 0.06, size=3), dtype=torch.float32)
    items = [ds[t] for t in range(frames + 1)]
    m = ds._scene['means3D']
    keep = ~((m[:, 0] > 0.2) & (m[:, 0] < 0.7) & (m[:, 1] > -0.1) & (m[:, 1] < 0.35))
    params = {k: (v[keep] if v.shape[0] == m.shape[0] else v).clone().contiguous() for k, v in ds._scene.items()}
    return HeldOut(items), params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from splatam_amd import evaluation
    dataset, params = build(args.gaussians, args.frames)
    torch.cuda.synchronize()
    lines = []
    tmp = tempfile.mkdtemp(prefix="novel_view_run_")
    try:
        for form, kw in (("device", dict()), ("device+save", dict(save_frames=True, eval_dir=os.path.join(tmp, "eval_nvs"))),
                         ("mirror", dict(engine="mirror"))):
            ms = []
            for i in range(args.repeats + 1):
                out = evaluation.evaluate_novel_views(dataset, params, len(dataset), 0.5, 60, True, **kw)
                torch.cuda.synchronize()
                if i:                                   # (the first call loads kernels and allocates the evaluation's scratch)
                    ms.append(out['eval_ms_per_frame'])
            lines.append({"form": form, "size": [W, H], "gaussians": int(params['means3D'].shape[0]), "held_out_frames": len(out['frames']),
                          "ms_per_frame": [round(v, 2) for v in ms], "median_ms_per_frame": round(float(np.median(ms)), 2),
                          "valid_frames": int(out['valid_nvs_frames'].sum()), "repeated": len(out['repeated']),
                          "avg_psnr": round(out['avg_psnr'], 3), "holes": out['holes'].tolist()})
            print(json.dumps(lines[-1]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("```\n" + "\n".join(json.dumps(line) for line in lines) + "\n```\n")


if __name__ == "__main__":
    main()
