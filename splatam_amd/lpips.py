"""LPIPS (AlexNet) from weights the USER supplies: what the reference's ``eval`` / ``eval_nvs`` get from torchmetrics'
``LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True)`` (utils/eval_helpers.py:484-485, 730-731), on the device
(csrc/lpips.hip: the five convolutions are one implicit GEMM on the exact-f32 MFMA) and without a host read.  This package carries no
weights and downloads nothing, ever: whoever runs the reference has the two files on disk (torchvision's AlexNet and the ``lpips``
package's linear layers, or torchmetrics' single file that holds both).

The definition (restated from the public implementation as recalled; agreement with torchmetrics on real weights has NOT
been checked in this repository -- ``python -m splatam_amd.lpips A.png B.png --weights W`` prints the number to compare):

  input     both images [3, H, W] in 0..1 (clamped); x <- 2x - 1; per channel (x - shift_c) / scale_c, shift (-0.030, -0.088, -0.188),
            scale (0.458, 0.448, 0.450)
  taps      f1 conv 3->64 11x11 stride 4 pad 2 + bias + ReLU; f2 maxpool 3x3 stride 2 (no padding, floor), conv 64->192 5x5 pad 2 + bias +
            ReLU; f3 maxpool, conv 192->384 3x3 pad 1 ...; f4 conv 384->256 3x3 pad 1 ...; f5 conv 256->256 3x3 pad 1 ...
  distance  per tap and pixel n = sqrt(sum_c f_c^2) + 1e-10, u = f / n for both images; d_l = mean over the tap's pixels of
            sum_c w_lc (u0_c - u1_c)^2; LPIPS = sum_l d_l.  31 x 31 is the smallest image for which every tap has an output.

CANONICAL ``.npz`` LAYOUT (``save_weights_npz`` / ``load_weights``), float32:
  ``conv1.weight`` [64, 3, 11, 11]   ``conv1.bias`` [64]      ``conv2.weight`` [192, 64, 5, 5]   ``conv2.bias`` [192]
  ``conv3.weight`` [384, 192, 3, 3]  ``conv3.bias`` [384]     ``conv4.weight`` [256, 384, 3, 3]  ``conv4.bias`` [256]
  ``conv5.weight`` [256, 256, 3, 3]  ``conv5.bias`` [256]     ``lin0`` [64]  ``lin1`` [192]  ``lin2`` [384]  ``lin3`` [256]  ``lin4`` [256]

``Lpips(weights, device)(im0, im1)`` is the device form; ``slam.lpips`` the torch form (the ``mirror`` engine, ``device="cpu"``)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import torch

CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
# per layer: stride, padding, a 3x3 stride-2 max-pool in front
CONV_GEOMETRY = ((4, 2, False), (1, 2, True), (1, 1, True), (1, 1, False), (1, 1, False))
LIN_CHANNELS = tuple(s[0] for s in CONV_SHAPES)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 31


class LpipsWeights:
    """The network: ``conv_weight[l]`` [Cout, Cin, k, k], ``conv_bias[l]`` [Cout], ``lin[l]`` [Cout] (>= 0 in a trained network), float32
    CPU tensors, checked on construction."""

    def __init__(self, conv_weight, conv_bias, lin):
        self.conv_weight = [torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous() for t in conv_weight]
        self.conv_bias = [torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous() for t in conv_bias]
        self.lin = [torch.as_tensor(t).detach().to("cpu", torch.float32).reshape(-1).contiguous() for t in lin]
        if not (len(self.conv_weight) == len(self.conv_bias) == len(self.lin) == 5):
            raise ValueError("LPIPS weights are five convolutions (weight, bias) and five linear layers")
        for l, shape in enumerate(CONV_SHAPES):
            if tuple(self.conv_weight[l].shape) != shape:
                raise ValueError(f"conv{l + 1}.weight has shape {tuple(self.conv_weight[l].shape)}, expected {shape}")
            if tuple(self.conv_bias[l].shape) != (shape[0],):
                raise ValueError(f"conv{l + 1}.bias has shape {tuple(self.conv_bias[l].shape)}, expected {(shape[0],)}")
            if tuple(self.lin[l].shape) != (shape[0],):
                raise ValueError(f"lin{l} has {self.lin[l].numel()} entries, expected {shape[0]}")

    def flat(self):
        """One float32 vector in the library's canonical order (include/splat_hip.h): weight, bias per layer; then lin0 .. lin4."""
        parts = []
        for w, b in zip(self.conv_weight, self.conv_bias):
            parts += [w.reshape(-1), b]
        return torch.cat(parts + self.lin)

    def named(self):
        out = {}
        for l in range(5):
            out[f"conv{l + 1}.weight"], out[f"conv{l + 1}.bias"] = self.conv_weight[l], self.conv_bias[l]
        for l in range(5):
            out[f"lin{l}"] = self.lin[l]
        return out


def save_weights_npz(weights, path):
    """Writes the canonical layout (module docstring)."""
    np.savez(path, **{k: v.numpy() for k, v in weights.named().items()})


def random_weights(seed=0):
    """A seeded stand-in network for tests and measurements: He-scaled convolutions, small biases, linear weights >= 0."""
    g = torch.Generator().manual_seed(int(seed))
    cw, cb, lin = [], [], []
    for shape in CONV_SHAPES:
        fan_in = shape[1] * shape[2] * shape[3]
        cw.append(torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5)
        cb.append(0.05 * torch.randn(shape[0], generator=g))
        lin.append(torch.rand(shape[0], generator=g))
    return LpipsWeights(cw, cb, lin)


def _load_npz(path):
    with np.load(path) as z:
        have = set(z.files)
        want = [f"conv{l + 1}.{p}" for l in range(5) for p in ("weight", "bias")] + [f"lin{l}" for l in range(5)]
        missing = [k for k in want if k not in have]
        if missing:
            raise ValueError(f"{path}: missing {', '.join(missing)} (the canonical layout: splatam_amd/lpips.py)")
        return LpipsWeights([z[f"conv{l + 1}.weight"] for l in range(5)], [z[f"conv{l + 1}.bias"] for l in range(5)],
                            [z[f"lin{l}"] for l in range(5)])


def _state_dict(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict")
    return {str(k): v for k, v in sd.items() if isinstance(v, torch.Tensor)}


def _distinct(cands):
    """Candidates [(key, tensor)] with equal tensors merged (torchmetrics stores each linear layer under two names): [(keys, tensor)]."""
    groups = []
    for k, t in cands:
        for keys, u in groups:
            if torch.equal(t, u):
                keys.append(k)
                break
        else:
            groups.append(([k], t))
    return groups


def _from_state_dicts(dicts, where):
    sd = {}
    for d in dicts:
        for k, v in d.items():
            if k in sd and not torch.equal(sd[k], v):
                raise ValueError(f"{where}: the key {k} is in both files with different contents")
            sd[k] = v
    cw, cb, lin = [], [], []
    for l, shape in enumerate(CONV_SHAPES):
        groups = _distinct([(k, t) for k, t in sd.items() if tuple(t.shape) == shape])
        if not groups:
            raise ValueError(f"{where}: conv{l + 1}.weight is missing (no tensor of shape {list(shape)})")
        if len(groups) > 1:
            raise ValueError(f"{where}: conv{l + 1}.weight is ambiguous: {', '.join(k for keys, _ in groups for k in keys)} all have shape {list(shape)}")
        keys, w = groups[0]
        bias = None
        for k in keys:
            bk = k[:-len("weight")] + "bias" if k.endswith("weight") else None
            if bk in sd:
                bias = sd[bk]
                break
        if bias is None:
            raise ValueError(f"{where}: conv{l + 1}.bias is missing (no 'bias' beside {keys[0]})")
        if tuple(bias.shape) != (shape[0],):
            raise ValueError(f"{where}: conv{l + 1}.bias has shape {list(bias.shape)}, expected {[shape[0]]}")
        cw.append(w)
        cb.append(bias)
    lins = {}
    for c in sorted(set(LIN_CHANNELS)):
        slots = [l for l, n in enumerate(LIN_CHANNELS) if n == c]
        groups = _distinct([(k, t) for k, t in sd.items() if tuple(t.shape) == (1, c, 1, 1)])
        names = ", ".join(f"lin{l}" for l in slots)
        if len(groups) < len(slots):
            raise ValueError(f"{where}: {names} missing ({len(groups)} tensor(s) of shape [1, {c}, 1, 1], expected {len(slots)})")
        if len(groups) > len(slots):
            raise ValueError(f"{where}: {names} ambiguous: {', '.join(k for keys, _ in groups for k in keys)} all have shape [1, {c}, 1, 1]")
        if len(slots) > 1:           # the two 256-wide layers: ordered by the integer in their key
            order = []
            for keys, t in groups:
                ints = [int(m) for m in re.findall(r"\d+", keys[0])]
                if not ints:
                    raise ValueError(f"{where}: {names} ambiguous: the key {keys[0]} holds no integer to order them by")
                order.append((ints[0], keys[0], t))
            if len({o[0] for o in order}) != len(order):
                raise ValueError(f"{where}: {names} ambiguous: {', '.join(o[1] for o in order)} carry the same integer")
            groups = [([o[1]], o[2]) for o in sorted(order, key=lambda o: o[0])]
        for l, (_, t) in zip(slots, groups):
            lins[l] = t.reshape(-1)
    for l in range(5):
        lin.append(lins[l])
    return LpipsWeights(cw, cb, lin)


def load_weights(path, lin_path=None):
    """``path``: a ``.npz`` in the canonical layout, or a torch state dict (read with ``weights_only=True``) that holds torchvision's
    AlexNet, the ``lpips`` package's linear layers, or both (as torchmetrics stores them); ``lin_path``: the second file when they are
    two.  Convolutions are identified by their shapes (all five differ), linear layers by shape [1, C, 1, 1], the two 256-wide ones
    ordered by the integer in their key.  Anything missing, ambiguous or of the wrong shape raises a ValueError that names it."""
    if isinstance(path, LpipsWeights):
        return path
    path = os.fspath(path)
    if path.endswith(".npz"):
        if lin_path is not None:
            raise ValueError("a canonical .npz holds all layers: lin_path does not apply")
        return _load_npz(path)
    dicts = [_state_dict(path)] + ([_state_dict(os.fspath(lin_path))] if lin_path is not None else [])
    return _from_state_dicts(dicts, path if lin_path is None else f"{path} + {os.fspath(lin_path)}")


def as_weights(weights):
    """None, an ``LpipsWeights``, or a path ``load_weights`` reads."""
    return None if weights is None else load_weights(weights)


def tap_shape(width, height, layer):
    """(C, H_l, W_l) of tap ``layer`` for an image of width x height."""
    from . import _capi
    L = _capi.lib()
    return LIN_CHANNELS[layer], int(L.splat_lpips_tap_size(int(height), layer)), int(L.splat_lpips_tap_size(int(width), layer))


class Lpips:
    """The device form.  The weights are uploaded and packed ONCE (``self.net``: the packed network every kernel reads); a workspace
    (activations of both images, the partial sums) is kept per image size.  ``Lpips(w)(im0, im1)`` returns a 0-dim float64 tensor on the device; nothing is read on the host."""

    def __init__(self, weights, device="cuda"):
        from . import _capi
        weights = load_weights(weights)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("Lpips runs on a HIP device; the torch form is splatam_amd.slam.lpips")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.dev, self.L = dev, _capi.lib()
        flat = weights.flat()
        assert flat.numel() == self.L.splat_lpips_weight_floats(), (flat.numel(), self.L.splat_lpips_weight_floats())
        self.net = torch.empty(self.L.splat_lpips_pack_floats(), dtype=torch.float32, device=dev)
        canonical = flat.to(dev)
        with torch.cuda.device(dev):
            _capi.check(self.L.splat_lpips_pack(canonical.data_ptr(), self.net.data_ptr(), self._stream()), "splat_lpips_pack")
        canonical.record_stream(torch.cuda.current_stream(dev))       # (dropped once the pack kernels have read it)
        self._ws = {}

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def workspace(self, width, height):
        """(SplatLpipsWorkspace, {array name: float32 / float64 view of the slab}) for an image size; allocated on first use."""
        from . import _capi
        key = (int(width), int(height))
        if key not in self._ws:
            if min(key) < MIN_SIZE:
                raise ValueError(f"LPIPS needs images of at least {MIN_SIZE} x {MIN_SIZE} pixels (got {key[0]} x {key[1]})")
            lay = _capi.lpips_workspace_layout(*key)
            slab = torch.empty(lay.total, dtype=torch.uint8, device=self.dev)
            ws = _capi.SplatLpipsWorkspace()
            with torch.cuda.device(self.dev):
                _capi.check(self.L.splat_lpips_workspace_bind(C.byref(ws), slab.data_ptr(), lay.arrays, lay.n, key[0], key[1]),
                            "splat_lpips_workspace_bind")
            views = {n: slab[lay.offset[n]:lay.offset[n] + lay.bytes[n]].view(torch.float64 if n == "partials" else torch.float32) for n in lay.names}
            self._ws[key] = (ws, views, slab)
        return self._ws[key][:2]

    def taps(self, width, height):
        """The five taps the latest call at this size left: [2, C_l, H_l, W_l] views of the workspace (image 0, image 1)."""
        _, views = self.workspace(width, height)
        return [views[f"tap{l}"].view(2, *tap_shape(width, height, l)) for l in range(5)]

    def _check(self, name, t, n, H, W):
        """``t`` is float32 on this device with shape [n, H, W] (a single plane may also be [H, W]); returned contiguous."""
        shapes = ((n, H, W), (H, W)) if n == 1 else ((n, H, W),)
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.dev and tuple(t.shape) in shapes):
            got = f"{t.dtype}, {tuple(t.shape)}, {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise RuntimeError(f"{name} must be a float32 tensor of shape [{n}, {H}, {W}] on {self.dev} (got {got})")
        return t if t.is_contiguous() else t.contiguous()

    def _out(self, out):
        if out is None:
            return torch.zeros((), dtype=torch.float64, device=self.dev)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == self.dev and out.numel() == 1):
            raise RuntimeError(f"out must be one float64 element on {self.dev}")
        return out

    def __call__(self, im0, im1, out=None):
        """LPIPS of two images [3, H, W] in 0..1 (values outside are clamped); ``out``: one float64 element to write to."""
        from . import _capi
        if not isinstance(im0, torch.Tensor) or im0.dim() != 3 or im0.shape[0] != 3:
            raise RuntimeError("im0 / im1 must be [3, H, W] tensors")
        H, W = int(im0.shape[-2]), int(im0.shape[-1])
        ws, _ = self.workspace(W, H)
        im0, im1, out = self._check("im0", im0, 3, H, W), self._check("im1", im1, 3, H, W), self._out(out)
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_lpips_images(W, H, im0.data_ptr(), im1.data_ptr(), self.net.data_ptr(), C.byref(ws), out.data_ptr(),
                                                  self._stream()), "splat_lpips_images")
        return out

    def planes(self, rgb, sil, gt_im, gt_depth, sil_thres, sil_mask=False, out=None):
        """LPIPS of an evaluated frame: ``weighted_im`` / ``weighted_gt_im`` formed from the planes as the metric kernels form them
        (``sil`` may be None without ``sil_mask``), clamped.  A frame whose every pixel is masked scores 0.0."""
        from . import _capi
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3 or rgb.shape[0] != 3:
            raise RuntimeError("rgb must be a [3, H, W] tensor")
        H, W = int(rgb.shape[-2]), int(rgb.shape[-1])
        ws, _ = self.workspace(W, H)
        rgb, gt_im, gt_depth = self._check("rgb", rgb, 3, H, W), self._check("gt_im", gt_im, 3, H, W), self._check("gt_depth", gt_depth, 1, H, W)
        if sil_mask or sil is not None:
            sil = self._check("sil", sil, 1, H, W)
        out = self._out(out)
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_lpips_planes(W, H, rgb.data_ptr(), sil.data_ptr() if sil is not None else None, gt_im.data_ptr(),
                                                  gt_depth.data_ptr(), float(sil_thres), int(bool(sil_mask)), self.net.data_ptr(),
                                                  C.byref(ws), out.data_ptr(), self._stream()), "splat_lpips_planes")
        return out

    def conv_layer(self, layer, x):
        """One layer alone (tests, measurements): convolution ``layer`` (0..4) + bias + ReLU of ``x`` [2, Cin, h, w], no pool."""
        from . import _capi
        cout, cin, k, _ = CONV_SHAPES[layer]
        stride, pad, _ = CONV_GEOMETRY[layer]
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[0] == 2 and x.shape[1] == cin):
            raise RuntimeError(f"x must be [2, {cin}, h, w]")
        h, w = int(x.shape[2]), int(x.shape[3])
        if not (x.dtype == torch.float32 and x.device == self.dev):
            raise RuntimeError(f"x must be float32 on {self.dev}")
        x = x.contiguous()
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        if ho < 1 or wo < 1:
            raise ValueError(f"layer {layer} has no output for an input of {w} x {h}")
        y = torch.empty(2, cout, ho, wo, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _capi.check(self.L.splat_lpips_conv(layer, w, h, x.data_ptr(), self.net.data_ptr(), y.data_ptr(), self._stream()),
                        "splat_lpips_conv")
        return y


def _read_image(path):
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m splatam_amd.lpips", description="LPIPS (AlexNet) of two pictures from user-supplied weights")
    ap.add_argument("image0")
    ap.add_argument("image1")
    ap.add_argument("--weights", required=True, help="canonical .npz or a torch state dict (torchvision AlexNet, lpips linear layers, or both)")
    ap.add_argument("--lin-weights", default=None, help="the second state dict when the linear layers are in a file of their own")
    ap.add_argument("--device", default="cuda", help="cuda (the HIP kernels) or cpu (the torch form)")
    args = ap.parse_args(argv)
    w = load_weights(args.weights, args.lin_weights)
    a, b = _read_image(args.image0), _read_image(args.image1)
    if a.shape != b.shape:
        raise SystemExit(f"the pictures differ in size: {tuple(a.shape[1:])} vs {tuple(b.shape[1:])}")
    if torch.device(args.device).type == "cuda":
        value = float(Lpips(w, args.device)(a.to(args.device), b.to(args.device)).cpu())
    else:
        from . import slam
        value = float(slam.lpips(a, b, w))
    print(f"LPIPS: {value:.6f}")
    return value


if __name__ == "__main__":
    main()
