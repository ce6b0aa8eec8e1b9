"""LPIPS without a GPU: splatam_amd/csrc/lpips_math.h compiled for the host (tests/lpips_math_shim.cpp), the torch form
``slam.lpips`` against the float64 numpy restatement (tests/lpips_ref.py), the weight loader, and ``evaluate`` with weights on the
torch mirror."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import eval_ref, lpips_ref
from tests.util import host_shim

I32P = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def shim():
    lib = host_shim("lpips_math_shim", "lpips_math.h", "eval_math.h")
    for name in ("lm_weight_offset", "lm_bias_offset", "lm_lin_offset", "lm_pack_offset", "lm_pack_bias_offset", "lm_pack_lin_offset"):
        getattr(lib, name).restype = C.c_longlong
        getattr(lib, name).argtypes = [C.c_int]
    lib.lm_weight_floats.restype = lib.lm_pack_floats.restype = C.c_longlong
    lib.lm_layer.argtypes = [C.c_int, I32P]
    lib.lm_k_map.argtypes = [C.c_int, C.c_int, I32P]
    lib.lm_input.restype = C.c_float
    lib.lm_input.argtypes = [C.c_float, C.c_int]
    lib.lm_input_masked.restype = C.c_float
    lib.lm_input_masked.argtypes = [C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
    return lib


@pytest.fixture(scope="module")
def weights():
    from splatam_amd import lpips
    return lpips.random_weights(3)


# ---------------------------------------------------------------------------------------------------------------- 1. lpips_math.h
def _layer(shim, l):
    out = (C.c_int * 6)()
    shim.lm_layer(l, out)
    return list(out)


def test_layer_table_matches_the_python_side(shim):
    from splatam_amd import lpips
    assert shim.lm_layers() == 5 and shim.lm_min_size() == lpips.MIN_SIZE == 31
    for l in range(5):
        cin, cout, k, stride, pad, pool = _layer(shim, l)
        assert (cout, cin, k, k) == lpips.CONV_SHAPES[l] and (stride, pad, bool(pool)) == lpips.CONV_GEOMETRY[l]
        assert shim.lm_layer_K(l) == cin * k * k and shim.lm_layer_Kpad(l) % 32 == 0 and 0 <= shim.lm_layer_Kpad(l) - cin * k * k < 32
    assert shim.lm_layer_K(0) == 363 and shim.lm_layer_Kpad(0) == 384


def test_stage_sizes_for_every_extent_31_to_80(shim):
    """Every stage's output size for ALL H, W in 31 .. 80 against the closed forms (conv: floor((n + 2p - k) / s) + 1, pool:
    floor((n - 3) / 2) + 1, partial rows: ceil(H_l W_l / 64)), and against the shapes torch's conv2d / max_pool2d give on the 50 pairs
    H = n, W = 111 - n, which put every n on both axes."""
    from splatam_amd import lpips, slam
    w = lpips.LpipsWeights([torch.zeros(s) for s in lpips.CONV_SHAPES], [torch.zeros(s[0]) for s in lpips.CONV_SHAPES],
                           [torch.zeros(s[0]) for s in lpips.CONV_SHAPES])
    def closed_form(n):
        sizes = []
        for l, ((_, _, k, _), (stride, pad, pool)) in enumerate(zip(lpips.CONV_SHAPES, lpips.CONV_GEOMETRY)):
            if pool:
                n = (n - 3) // 2 + 1
            n = (n + 2 * pad - k) // stride + 1
            sizes.append(n)
        return sizes
    for H in range(31, 81):
        hs = closed_form(H)
        for W in range(31, 81):
            ws = closed_form(W)
            for l in range(5):
                assert (shim.lm_tap_size(H, l), shim.lm_tap_size(W, l)) == (hs[l], ws[l]) and hs[l] >= 1 and ws[l] >= 1, (H, W, l)
                assert shim.lm_tap_rows(W, H, l) == -(-(hs[l] * ws[l]) // 64), (H, W, l)
    for n in range(31, 81):
        H, W = n, 111 - n
        taps = slam.lpips_taps(torch.zeros(1, 3, H, W), w)
        for l, f in enumerate(taps):
            assert (shim.lm_tap_size(H, l), shim.lm_tap_size(W, l)) == tuple(f.shape[2:]), (n, l)
            cin, cout, k, stride, pad, pool = _layer(shim, l)
            assert shim.lm_conv_out(shim.lm_layer_in(H, l), k, stride, pad) == f.shape[2]
            if pool:
                assert shim.lm_layer_in(H, l) == shim.lm_pool_out(shim.lm_tap_size(H, l - 1))
            assert shim.lm_tap_rows(W, H, l) == -(-(f.shape[2] * f.shape[3]) // 64)
    # 31 is the smallest extent with an output at every tap; 30 has none at the third
    assert [shim.lm_tap_size(31, l) for l in range(5)] == [7, 3, 1, 1, 1]
    assert shim.lm_tap_size(30, 2) == 0
    assert [shim.lm_tap_size(83, l) for l in range(5)] == [20, 9, 4, 4, 4] and [shim.lm_tap_size(61, l) for l in range(5)] == [14, 6, 2, 2, 2]
    assert [shim.lm_tap_size(1200, l) for l in range(5)] == [299, 149, 74, 74, 74] and [shim.lm_tap_size(680, l) for l in range(5)] == [169, 84, 41, 41, 41]


def test_k_map_is_the_weight_tensors_inner_order(shim):
    out = (C.c_int * 3)()
    for l in range(5):
        cin, _, k, _, _, _ = _layer(shim, l)
        for kk in range(cin * k * k):
            assert shim.lm_k_map(k, kk, out) == 1
            assert tuple(out) == tuple(int(v) for v in np.unravel_index(kk, (cin, k, k))), (l, kk)
    assert shim.lm_k_map(7, 0, out) == 0


def test_buffer_offsets(shim):
    from splatam_amd import lpips
    o = 0
    for l, s in enumerate(lpips.CONV_SHAPES):
        assert shim.lm_weight_offset(l) == o
        o += int(np.prod(s))
        assert shim.lm_bias_offset(l) == o
        o += s[0]
    for l, s in enumerate(lpips.CONV_SHAPES):
        assert shim.lm_lin_offset(l) == o
        o += s[0]
    assert shim.lm_weight_floats() == o == lpips.random_weights(0).flat().numel()
    p = 0
    for l, s in enumerate(lpips.CONV_SHAPES):
        assert shim.lm_pack_offset(l) == p
        p += shim.lm_layer_Kpad(l) * s[0]
    for name in ("lm_pack_bias_offset", "lm_pack_lin_offset"):          # the packed network: weights, then the biases, then the lin vectors
        for l, s in enumerate(lpips.CONV_SHAPES):
            assert getattr(shim, name)(l) == p
            p += s[0]
    assert shim.lm_pack_floats() == p


def test_input_transform_clamps_and_masks(shim):
    """Bit-equal to the float32 numpy expression; values outside 0..1 are clamped; a NaN stays; a masked pixel is the transform of 0."""
    shift, scale = np.float32(lpips_ref.SHIFT), np.float32(lpips_ref.SCALE)

    def want(v, ch):
        v = np.float32(min(max(v, 0.0), 1.0))
        return ((np.float32(2) * v - np.float32(1)) - shift[ch]) / scale[ch]
    rng = np.random.default_rng(0)
    for v in list(rng.uniform(0, 1, 50).astype(np.float32)) + [0.0, 1.0, -0.3, 1.7, -1e30, 1e30]:
        for ch in range(3):
            got = shim.lm_input(float(v), ch)
            assert np.float32(got) == want(float(v), ch), (v, ch)
            np.testing.assert_allclose(got, lpips_ref.transform(np.full((3, 1, 1), v))[ch, 0, 0], rtol=3e-7, atol=1e-7)
    assert shim.lm_input(-0.3, 1) == shim.lm_input(0.0, 1) and shim.lm_input(1.7, 2) == shim.lm_input(1.0, 2)
    assert np.isnan(shim.lm_input(float("nan"), 0))
    for ch in range(3):
        zero = shim.lm_input(0.0, ch)
        assert shim.lm_input_masked(0.6, ch, 0.0, 0.9, 0.5, 0) == zero                 # no depth
        assert shim.lm_input_masked(0.6, ch, 2.0, 0.4, 0.5, 1) == zero                 # depth, but no presence (sil_mask)
        assert shim.lm_input_masked(0.6, ch, 2.0, 0.4, 0.5, 0) == shim.lm_input(0.6, ch)
        assert shim.lm_input_masked(0.6, ch, 2.0, 0.9, 0.5, 1) == shim.lm_input(0.6, ch)
        assert shim.lm_input_masked(1.4, ch, 2.0, 0.9, 0.5, 1) == shim.lm_input(1.0, ch)


# ---------------------------------------------------------------------------------------------------------------- 2. the torch form
@pytest.mark.parametrize("W,H,seed", [(83, 61, 0), (31, 31, 1), (97, 45, 2)])
def test_slam_lpips_float64_matches_the_restatement(weights, W, H, seed):
    from splatam_amd import slam
    a, b = lpips_ref.image_pair(W, H, seed)
    want, taps, _, _ = lpips_ref.lpips(a, b, weights)
    got, got_taps = slam.lpips(torch.from_numpy(a).double(), torch.from_numpy(b).double(), weights, return_taps=True)
    assert want > 1e-3
    assert abs(float(got) - want) <= 1e-12 * want
    for f, g in zip(taps, got_taps):
        assert f.shape == tuple(g.shape)
        assert np.abs(g.numpy() - f).max() <= 1e-12 * np.abs(f).max()
    assert float(slam.lpips(torch.from_numpy(a), torch.from_numpy(a), weights)) == 0.0
    with pytest.raises(ValueError, match="31"):
        slam.lpips(torch.zeros(3, 30, 40), torch.zeros(3, 30, 40), weights)


def test_out_of_range_values_are_clamped(weights):
    from splatam_amd import slam
    a, b = lpips_ref.image_pair(40, 33, 5)
    a2 = a.copy()
    a2[a == 1.0] = 1.5
    a2[a == 0.0] = -0.5
    assert (a2 != a).any()
    assert float(slam.lpips(torch.from_numpy(a2), torch.from_numpy(b), weights)) == float(slam.lpips(torch.from_numpy(a), torch.from_numpy(b), weights))


# ---------------------------------------------------------------------------------------------------------------- 3. the loader
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.conv_weight + a.conv_bias + a.lin, b.conv_weight + b.conv_bias + b.lin))


def _torchvision_dict(w):
    idx = (0, 3, 6, 8, 10)
    d = {}
    for l, i in enumerate(idx):
        d[f"features.{i}.weight"], d[f"features.{i}.bias"] = w.conv_weight[l].clone(), w.conv_bias[l].clone()
    d["classifier.1.weight"], d["classifier.1.bias"] = torch.zeros(8, 16), torch.zeros(8)
    return d


def _lpips_dict(w):
    return {f"lin{l}.model.1.weight": w.lin[l].clone().view(1, -1, 1, 1) for l in range(5)}


def _combined_dict(w):
    idx = ((1, 0), (2, 3), (3, 6), (4, 8), (5, 10))
    d = {"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)}
    for l, (s, i) in enumerate(idx):
        d[f"net.slice{s}.{i}.weight"], d[f"net.slice{s}.{i}.bias"] = w.conv_weight[l].clone(), w.conv_bias[l].clone()
    for l in range(5):                                  # each linear layer under two names, as a module list beside attributes stores it
        d[f"lin{l}.model.1.weight"] = w.lin[l].clone().view(1, -1, 1, 1)
        d[f"lins.{l}.model.1.weight"] = w.lin[l].clone().view(1, -1, 1, 1)
    return d


def test_npz_round_trip_and_state_dict_forms(weights, tmp_path):
    from splatam_amd import lpips
    npz = str(tmp_path / "w.npz")
    lpips.save_weights_npz(weights, npz)
    with np.load(npz) as z:
        assert sorted(z.files) == sorted([f"conv{l}.{p}" for l in range(1, 6) for p in ("weight", "bias")] + [f"lin{l}" for l in range(5)])
        assert z["conv1.weight"].shape == (64, 3, 11, 11) and z["lin2"].shape == (384,) and z["conv3.bias"].dtype == np.float32
    assert _same(lpips.load_weights(npz), weights)
    assert lpips.load_weights(weights) is weights and lpips.as_weights(None) is None
    tv, ln, both = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth"), str(tmp_path / "both.pth")
    torch.save(_torchvision_dict(weights), tv)
    torch.save(_lpips_dict(weights), ln)
    torch.save(_combined_dict(weights), both)
    assert _same(lpips.load_weights(tv, ln), weights)
    assert _same(lpips.load_weights(ln, tv), weights)
    assert _same(lpips.load_weights(both), weights)
    # the 256-wide layers are ordered by the integer in their key, not by their position in the file
    d = _lpips_dict(weights)
    d = {k: d[k] for k in reversed(list(d))}
    d.update(_torchvision_dict(weights))
    torch.save(d, both)
    assert _same(lpips.load_weights(both), weights)
    assert not torch.equal(weights.lin[3], weights.lin[4])


def test_loader_refuses_by_name(weights, tmp_path):
    from splatam_amd import lpips
    path = str(tmp_path / "w.pth")

    def refused(d, match, second=None):
        torch.save(d, path)
        with pytest.raises(ValueError, match=match):
            lpips.load_weights(path, second)
    full = dict(_torchvision_dict(weights), **_lpips_dict(weights))
    d = dict(full)
    del d["features.6.weight"]
    refused(d, r"conv3\.weight is missing")
    d = dict(full)
    del d["features.8.bias"]
    refused(d, r"conv4\.bias is missing")
    d = dict(full)
    d["features.10.bias"] = torch.zeros(255)
    refused(d, r"conv5\.bias has shape \[255\]")
    d = dict(full)
    d["features.3.weight"] = torch.zeros(192, 64, 3, 3)                 # a wrong shape is no conv2 at all
    refused(d, r"conv2\.weight is missing")
    refused(_torchvision_dict(weights), r"lin0 missing")
    d = dict(full)
    d["extra.model.1.weight"] = torch.rand(1, 64, 1, 1)
    refused(d, r"lin0 ambiguous.*extra\.model\.1\.weight")
    d = dict(full)
    d["other.weight"] = torch.rand(256, 256, 3, 3)
    refused(d, r"conv5\.weight is ambiguous")
    d = {k: v for k, v in full.items() if not k.startswith(("lin3", "lin4"))}
    d["a.weight"], d["b.weight"] = weights.lin[3].view(1, -1, 1, 1), weights.lin[4].view(1, -1, 1, 1)
    refused(d, r"lin3, lin4 ambiguous.*no integer")
    d = {k: v for k, v in full.items() if not k.startswith("lin4")}
    refused(d, r"lin3, lin4 missing")
    npz = str(tmp_path / "w.npz")
    named = {k: v.numpy() for k, v in weights.named().items() if k != "lin2"}
    np.savez(npz, **named)
    with pytest.raises(ValueError, match="missing lin2"):
        lpips.load_weights(npz)
    named["lin2"] = np.zeros(383, dtype=np.float32)
    np.savez(npz, **named)
    with pytest.raises(ValueError, match="lin2 has 383 entries"):
        lpips.load_weights(npz)
    with pytest.raises(RuntimeError, match="HIP device"):
        lpips.Lpips(weights, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- 4. evaluate
def test_evaluate_with_weights_on_the_mirror(weights, tmp_path):
    """The existing synthetic sequence on the CPU (the torch mirror, the C oracle behind ``slam.Renderer``): one LPIPS per evaluated
    frame, its mean, lpips.txt -- and every other entry equal to the run without weights."""
    from oracle import c_ref
    from splatam_amd import evaluation, slam
    saved = slam.Renderer
    slam.Renderer = c_ref.CRasterizer
    try:
        dataset, params = eval_ref.golden_case("cpu")
        args = (dataset, params, len(dataset), eval_ref.GOLDEN_SIL_THRES, 0, False)
        plain = evaluation.evaluate(*args, eval_every=5, engine="mirror", eval_dir=str(tmp_path / "plain"))
        npz = str(tmp_path / "w.npz")
        from splatam_amd import lpips
        lpips.save_weights_npz(weights, npz)
        got = evaluation.evaluate(*args, eval_every=5, engine="mirror", eval_dir=str(tmp_path / "with"), lpips_weights=npz)
        # frame 0 by hand: the reference's expressions on its two renders
        color, depth, _, _ = evaluation._frame(dataset, 0)
        row = evaluation._mirror_row(params, {'cam': slam.setup_camera(color.shape[2], color.shape[1], dataset[0][2][:3, :3].numpy(),
                                                                       torch.linalg.inv(dataset[0][3]).numpy(), device="cpu"),
                                              'im': color, 'depth': depth, 'id': 0, 'w2c': torch.linalg.inv(dataset[0][3]).float()},
                                     0, eval_ref.GOLDEN_SIL_THRES, True, False, weights)
    finally:
        slam.Renderer = saved
    assert plain['lpips'] is None and 'avg_lpips' not in plain and not os.path.exists(tmp_path / "plain" / "lpips.txt")
    assert got['frames'] == [0, 4, 9] and got['lpips'].shape == (3,) and got['sil_mask']
    assert np.isfinite(got['lpips']).all() and (got['lpips'] > 0).all()
    assert got['avg_lpips'] == float(got['lpips'].mean())
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "with" / "lpips.txt"), got['lpips'])
    assert float(row[7]) == got['lpips'][0]
    for k in plain:
        if k in ('lpips', 'eval_s', 'eval_ms_per_frame'):
            continue
        if isinstance(plain[k], np.ndarray):
            np.testing.assert_array_equal(plain[k], got[k], err_msg=k)
        else:
            assert plain[k] == got[k], k
    assert set(got) - set(plain) == {'avg_lpips'}


def test_two_pictures_from_the_command_line_on_the_cpu(weights, tmp_path, capsys):
    from PIL import Image
    from splatam_amd import lpips
    a, b = lpips_ref.image_pair(64, 40, 3)
    paths, quantised = [], []
    for name, im in (("a.png", a), ("b.png", b)):
        paths.append(str(tmp_path / name))
        q = np.rint(im.transpose(1, 2, 0) * 255).astype(np.uint8)
        quantised.append(q.transpose(2, 0, 1).astype(np.float32) / 255.0)
        Image.fromarray(q).save(paths[-1])
    npz = str(tmp_path / "weights.npz")
    lpips.save_weights_npz(weights, npz)
    got = lpips.main(paths + ["--weights", npz, "--device", "cpu"])
    want = lpips_ref.lpips(quantised[0], quantised[1], weights)[0]
    assert abs(got - want) <= 1e-4 * want and f"LPIPS: {got:.6f}" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        lpips.main(paths[:1] + ["--weights", npz])
