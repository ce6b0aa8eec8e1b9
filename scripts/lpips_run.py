#!/usr/bin/env python3
"""Measures LPIPS on the device (csrc/lpips.hip) with seeded stand-in weights (``lpips.random_weights``) and prints ONE JSON line.

  layers     each convolution alone on the chain's own activations at --width x --height: device-event time per launch after a
             warm-up, 2 M N K useful FLOP (M = output pixels of both images, N = output channels, K = Cin k k; the zero rows behind
             conv1's K = 363 are not counted), achieved TFLOP/s and its share of the 157 TFLOP/s f32-MFMA peak
  chain      the whole call (input stage, pools, convolutions, distances, finish) per pair of images
  evaluate   ``evaluation.evaluate`` of a synthetic sequence's own map with and without weights, alternating, ms per evaluated frame
  torch      (--torch) the same forward through ``torch.nn.functional.conv2d`` on the device (``slam.lpips``), if it runs there

Every timed block ends in a device synchronise or is bracketed by device events."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TFLOPS = 157.0


def image_pair(W, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(6.28 * (a * xx + b * yy)) for a, b in ((1.0, 2.0), (3.0, 0.5), (2.0, 2.5))])
    a = (base + 0.08 * torch.randn(base.shape, generator=g)).clamp(0, 1)
    b = (base + 0.1 * torch.cos(6.28 * (3 * xx - 2 * yy)) + 0.05 * torch.randn(base.shape, generator=g)).clamp(0, 1)
    return a.cuda().contiguous(), b.cuda().contiguous()


def events_ms(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / n


def layers(net, W, H, reps):
    from splatam_amd import lpips
    import torch.nn.functional as F
    a, b = image_pair(W, H)
    value = float(net(a, b).cpu())
    taps = [t.clone() for t in net.taps(W, H)]
    _, views = net.workspace(W, H)
    out = []
    for l, (cout, cin, k, _) in enumerate(lpips.CONV_SHAPES):
        stride, pad, pool = lpips.CONV_GEOMETRY[l]
        x = views["input"].view(2, 3, H, W).clone() if l == 0 else (F.max_pool2d(taps[l - 1], 3, 2) if pool else taps[l - 1]).contiguous()
        ms = events_ms(lambda: net.conv_layer(l, x), reps, 5)
        M, K = 2 * taps[l].shape[2] * taps[l].shape[3], cin * k * k
        flop = 2.0 * M * cout * K
        out.append({'layer': l + 1, 'M': M, 'N': cout, 'K': K, 'workgroups': -(-M // 64) * (cout // 64), 'ms': ms, 'gflop': flop / 1e9,
                    'tflops': flop / (ms * 1e-3) / 1e12, 'share_of_peak': flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS})
    chain_ms = events_ms(lambda: net(a, b), reps, 5)
    total = sum(r['gflop'] for r in out)
    return {'value': value, 'layers': out, 'conv_ms_sum': sum(r['ms'] for r in out), 'gflop_total': total, 'chain_ms': chain_ms,
            'chain_tflops': total / chain_ms}          # (GFLOP / ms = TFLOP/s)


def evaluate(weights, W, H, gaussians, frames, rounds):
    from splatam_amd import evaluation, pipeline
    f = 0.5 * W
    ds = pipeline.SyntheticRGBDSequence(gaussians, W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, num_frames=frames, seed=2, step_m=0.012,
                                        step_deg=0.4).preload()
    params = {k: v.clone().contiguous() for k, v in ds._scene.items()}
    args = (ds, params, len(ds), 0.5, 60, True)
    evaluation.evaluate(*args)                                  # warm-up of both forms
    last = evaluation.evaluate(*args, lpips_weights=weights)
    without, with_ = [], []
    for _ in range(rounds):
        without.append(evaluation.evaluate(*args)['eval_ms_per_frame'])
        last = evaluation.evaluate(*args, lpips_weights=weights)
        with_.append(last['eval_ms_per_frame'])
    return {'frames': frames, 'gaussians': gaussians, 'eval_ms_per_frame_without': without, 'eval_ms_per_frame_with': with_,
            'median_without': float(np.median(without)), 'median_with': float(np.median(with_)), 'avg_lpips': last['avg_lpips'],
            'avg_psnr': last['avg_psnr']}


def torch_form(weights, W, H, reps, value):
    from splatam_amd import slam
    a, b = image_pair(W, H)
    try:
        with torch.no_grad():
            t0 = time.perf_counter()
            v = float(slam.lpips(a, b, weights).cpu())
            first_s = time.perf_counter() - t0
            ms = events_ms(lambda: slam.lpips(a, b, weights), reps, 3)
        return {'runs': True, 'first_call_s': first_s, 'ms': ms, 'value': v, 'rel_diff_to_kernels': abs(v / value - 1) if value else None}
    except Exception as e:          # reported, not hidden: the JSON says that it did not run and why
        return {'runs': False, 'error': f"{type(e).__name__}: {e}"[:400]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gaussians", type=int, default=400000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--torch", action="store_true", help="also time the forward through torch.nn.functional.conv2d on the device")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_run.py measures on a GPU: none found")
    from splatam_amd import lpips
    weights = lpips.random_weights(0)
    net = lpips.Lpips(weights, "cuda")
    out = {'size': [a.width, a.height], 'peak_tflops': PEAK_TFLOPS}
    out.update(layers(net, a.width, a.height, a.reps))
    if not a.no_evaluate:
        out['evaluate'] = evaluate(weights, a.width, a.height, a.gaussians, a.frames, a.rounds)
    if a.torch:
        out['torch'] = torch_form(weights, a.width, a.height, max(3, a.reps // 3), out['value'])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
