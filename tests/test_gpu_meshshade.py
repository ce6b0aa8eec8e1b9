"""The mesh shade layer on the device (csrc/meshshade.hip through ``splatam_amd.mesh_view``), held bit for bit to the header on the host
(tests/meshshade_math_shim.cpp), which tests/test_meshshade_cpu.py holds to the float64 restatement:

  1. ``vertex_normals`` = the shim's bits on the grid cube, the sphere and the box; the same bits over two runs and a face permutation.
  2. ``splat_mesh_visibility``: the high words are ``mesh_render.render_depth``'s bits, the low words the shim's faces, on every case of
     ``meshrender_ref.render_cases`` (67 x 45 is an odd pixel count: the 16-byte clear of an 8-byte plane has a tail); two runs agree.
  3. ``MeshViewer.render`` = the shim byte for byte for every mode x smooth x samples 1, 2, 3 on the 67 x 45 cases and for ``shaded`` on the
     96 x 64 ones; ``planes=True`` gives the depth plane of ``render_depth``, the shim's faces and the shim's normals, bit for bit.
  4. Rejections return SPLAT_E_INVALID and launch nothing.
  5. An empty mesh is a picture of the background.
  6. A ``MeshViewer`` over a live engine's mesh leaves the engine untouched, and its second ``render`` allocates nothing.
  7. ``python -m splatam_amd.mesh_view`` writes the PNGs ``render`` returns; ``python -m splatam_amd.mesh --views`` writes its pictures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshrender_ref as R
import meshshade_ref as S
from test_meshshade_cpu import VARIANTS, jet, load_shim, normal_meshes, shim_normals, shim_shade, shim_visibility

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES = {0: "world", 1: "camera"}


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _device_mesh(v, f, colors=None):
    from splatam_amd.mesh import Mesh
    return Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda(),
                None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, np.float32)).cuda())


def _keys(t):
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- 1. normals
def test_vertex_normals_equal_the_header_and_do_not_depend_on_order(shim):
    from splatam_amd import mesh_view as MV
    for name, (v, f) in normal_meshes().items():
        want = shim_normals(shim, v, f)
        m = _device_mesh(v, f)
        got = MV.vertex_normals(m.vertices, m.faces)
        again = MV.vertex_normals(m.vertices, m.faces)
        perm = torch.from_numpy(np.random.default_rng(5).permutation(len(f))).cuda()
        shuffled = MV.vertex_normals(m.vertices, m.faces[perm].contiguous())
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), name
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(got.view(torch.int32), shuffled.view(torch.int32)), name
    assert MV.vertex_normals(m.vertices[:0], m.faces[:0]).shape == (0, 3)
    assert (MV.vertex_normals(m.vertices, m.faces[:0]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. visibility
@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_keys_equal_the_header_and_hold_the_depth_plane(shim, name):
    from splatam_amd import mesh_render as MR
    from splatam_amd import mesh_view as MV
    v, f, w2c, intr, size = R.render_cases()[name]
    viewer = MV.MeshViewer(_device_mesh(v, f), size, intr)
    viewer.render(w2c)
    keys = _keys(viewer.keys).copy()
    want = shim_visibility(shim, v, f, w2c, intr, size)
    depth = MR.render_depth(viewer.mesh.vertices, viewer.mesh.faces, w2c, intr, size).cpu().numpy()
    none = keys == np.uint64(0xffffffffffffffff)
    assert np.array_equal(np.where(none, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)), depth.view(np.uint32))
    assert np.array_equal(keys & np.uint64(0xffffffff), want & np.uint64(0xffffffff))
    assert np.array_equal(keys, want)
    viewer.render(w2c)
    assert np.array_equal(_keys(viewer.keys), keys)
    # at the default split only faces with a box beyond 16 pixels reach the wave's walk and its face index (the lane's own in the other)
    from splatam_amd import _capi
    L = _capi.lib()
    try:
        for split in (1, 1 << 30):                                       # every face by the wave; every face with a box by one lane
            assert L.splat_debug_option(5, split) in (0, 1)
            viewer.keys.fill_(0)
            viewer.render(w2c)
            assert np.array_equal(_keys(viewer.keys), want), split
    finally:
        L.splat_debug_option(5, 0)


# ---------------------------------------------------------------------------------------------------------------- 3. pictures
@pytest.mark.parametrize("name", sorted(R.render_cases()))
def test_render_equals_the_header_byte_for_byte(shim, name):
    from splatam_amd import mesh_view as MV
    v, f, w2c, intr, size = R.render_cases()[name]
    colours, lut = S.case_colors(name), jet()
    n32 = shim_normals(shim, v, f)
    small = name.endswith("67x45")
    for samples in ((1, 2, 3) if small else (1,)):
        viewer = MV.MeshViewer(_device_mesh(v, f, colours), size, intr, samples=samples)
        assert np.array_equal(viewer.normals.cpu().numpy().view(np.uint32), n32.view(np.uint32))
        keys = shim_visibility(shim, v, f, w2c, intr, size, samples)
        for mode, smooth, frame in (VARIANTS if small else [("shaded", True, 0)]):
            kw = dict(mode=mode, smooth=smooth, normal_frame=FRAMES[frame], background=S.BG, albedo=S.ALBEDO, ambient=S.AMBIENT, depth_range=S.DEPTH_RANGE)
            want = shim_shade(shim, v, f, colours, n32, w2c, intr, size, samples, keys, mode, smooth=smooth, normal_frame=frame, lut=lut,
                              planes=samples == 1)
            got = viewer.render(w2c, planes=samples == 1, **kw)
            if samples == 1:
                (got, planes), (want, wanted) = got, want
                assert np.array_equal(planes['face'].cpu().numpy(), wanted['face']), (mode, smooth)
                assert np.array_equal(planes['depth'].cpu().numpy().view(np.uint32), wanted['depth'].view(np.uint32)), (mode, smooth)
                assert np.array_equal(planes['normal'].cpu().numpy().view(np.uint32), wanted['normal'].view(np.uint32)), (mode, smooth)
            differ = int((got.cpu().numpy() != want).any(axis=2).sum())
            assert differ == 0, f"{name} x{samples} {mode} smooth={smooth} frame={frame}: {differ} pixels differ from the header"
        if samples == 1:
            from splatam_amd import mesh_render as MR
            depth = MR.render_depth(viewer.mesh.vertices, viewer.mesh.faces, w2c, intr, size)
            assert torch.equal(planes['depth'].view(torch.int32), depth.view(torch.int32))
    # a mesh without colours renders with the albedo, and the one-shot form is the viewer's
    plain = MV.render_mesh(_device_mesh(v, f), w2c, intr, size, mode="color", background=S.BG, albedo=S.ALBEDO)
    want = shim_shade(shim, v, f, None, n32, w2c, intr, size, 1, shim_visibility(shim, v, f, w2c, intr, size), "color")
    assert np.array_equal(plain.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- 4. rejections, 5. empty
def test_rejections_launch_nothing_and_an_empty_mesh_is_background():
    from splatam_amd import _capi
    from splatam_amd import mesh_view as MV
    v, f, w2c, intr, size = R.render_cases()["sphere-outside-67x45"]
    viewer = MV.MeshViewer(_device_mesh(v, f), size, intr)
    first = viewer.render(w2c).clone()
    keys = viewer.keys.clone()
    L, a, view = _capi.lib(), viewer.args, viewer.view
    m = viewer.mesh
    planes = torch.zeros(size[1], size[0], dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def shade(keys_ptr=viewer.keys.data_ptr(), depth=None):
        return L.splat_mesh_shade(m.vertices.data_ptr(), len(v), m.faces.data_ptr(), len(f), None, viewer.normals.data_ptr(), view, keys_ptr, a,
                                  viewer.rgb8.data_ptr(), depth, None, None, stream)

    viewer.rgb8.fill_(7)
    for samples in (0, 5):
        a.samples = samples
        assert shade() == 1
    a.samples = 1
    assert shade(keys_ptr=None) == 1
    two = MV.MeshViewer(m, (33, 22), (20.0, 20.0, 16.0, 11.0), samples=2)
    two.render(np.eye(4))
    two.rgb8.fill_(7)
    assert L.splat_mesh_shade(m.vertices.data_ptr(), len(v), m.faces.data_ptr(), len(f), None, two.normals.data_ptr(), two.view, two.keys.data_ptr(),
                              two.args, two.rgb8.data_ptr(), planes.data_ptr(), None, None, stream) == 1
    with pytest.raises(ValueError, match="samples = 1"):
        two.render(np.eye(4), planes=True)
    big = _capi.SplatMeshView()
    big.width, big.height, big.fx, big.fy, big.cx, big.cy, big.near_z, big.w2c = 1 << 15, 1 << 15, 1.0, 1.0, 0.0, 0.0, 0.01, viewer.pose.data_ptr()
    assert L.splat_mesh_visibility(m.vertices.data_ptr(), len(v), m.faces.data_ptr(), len(f), big, viewer.keys.data_ptr(), stream) == 1
    with pytest.raises(ValueError):
        MV.MeshViewer(m, (1 << 14, 1 << 14), intr, samples=2)
    torch.cuda.synchronize()
    assert (viewer.rgb8 == 7).all() and (two.rgb8 == 7).all() and torch.equal(viewer.keys, keys)       # nothing was launched
    assert torch.equal(viewer.render(w2c), first)
    # 5. an empty mesh: a picture of the background, planes of "none"
    empty = MV.MeshViewer(_device_mesh(v[:0], f[:0]), size, intr)
    image, p = empty.render(w2c, background=(1.0, 0.5, 0.25), planes=True)
    assert (image.cpu().numpy() == np.array([255, 128, 64], dtype=np.uint8)).all()
    assert (p['face'] == -1).all() and (p['depth'] == 0).all() and (p['normal'] == 0).all()
    no_faces = MV.MeshViewer(_device_mesh(v, f[:0]), size, intr, samples=3)
    assert (no_faces.render(w2c, mode="depth", background=(0.0, 0.0, 0.0)) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 6. hands off
def test_a_viewer_leaves_a_live_engine_untouched_and_allocates_once():
    from splatam_amd import mesh as M
    from splatam_amd import mesh_view as MV
    from splatam_amd.fused import PARAM_ORDER
    from test_gpu_meshscore import H, W, _engine
    eng, intr = _engine()
    main = eng._camera
    with torch.no_grad():
        mesh = M.extract_mesh(eng, [0, 1, 2], (W, H), intr, voxel_size=0.05, sil_thres=0.5, depth_max=6.0)
    torch.cuda.synchronize()
    assert mesh.faces.shape[0] > 500

    def snapshot():
        s = {f"param {n}": eng.params[n].detach().clone() for n in PARAM_ORDER + ("cam_unnorm_rots", "cam_trans")}
        s.update({f"exp_avg {n}": eng.exp_avg[n].clone() for n in PARAM_ORDER})
        s.update({f"exp_avg_sq {n}": eng.exp_avg_sq[n].clone() for n in PARAM_ORDER})
        s.update({f"variables {n}": eng.variables[n].clone() for n in ('max_2D_radius', 'timestep', 'means2D_gradient_accum', 'denom')})
        s.update({f"rendered {i}": t.clone() for i, t in enumerate(eng.rendered())})
        s.update({f"main {n}": main.buf[n].clone() for n in ('status', 'd_cam')})
        s.update({f"mesh {n}": getattr(mesh, n).clone() for n in ("vertices", "faces", "colors")})
        return s
    before = snapshot()
    views = np.stack([np.eye(4), R.rotated((0.05, 0.0, 0.02), 0.1, (0, 1, 0.2))])
    viewer = MV.MeshViewer(mesh, (W, H), intr, samples=2)
    first = viewer.render(views[0], mode="shaded-color").clone()
    viewer.render(views[1], mode="depth")
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    second = viewer.render(views[0], mode="shaded-color")
    viewer.render(torch.from_numpy(views[1]).float().cuda(), mode="normal", normal_frame="camera")
    assert torch.cuda.memory_allocated() == allocated
    third = viewer.render(views[0], mode="shaded-color")
    torch.cuda.synchronize()
    assert torch.equal(first, third) and second.data_ptr() == third.data_ptr()
    assert len(torch.unique(first.reshape(-1, 3), dim=0)) > 50                     # a picture, not a flat field
    after = snapshot()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for name, t in before.items():
        assert torch.equal(bits(t), bits(after[name])), name
    assert eng._camera is main


# ---------------------------------------------------------------------------------------------------------------- 7. commands
def test_the_command_writes_the_pictures_render_returns(tmp_path):
    from PIL import Image
    from splatam_amd import mesh_view as MV
    from splatam_amd.export import save_mesh_ply
    v, f = R.sphere()[:2]
    colours = S.vertex_colors(len(v), 11)
    ply = str(tmp_path / "mesh.ply")
    save_mesh_ply(ply, v, f, colours)
    w2c = R.ring_views(3, 2.0).astype(np.float64)
    np.savetxt(str(tmp_path / "traj.txt"), np.linalg.inv(w2c).reshape(3, 16))
    out = str(tmp_path / "pics")
    root = os.path.dirname(HERE)
    done = subprocess.run([sys.executable, "-m", "splatam_amd.mesh_view", ply, "--out", out, "--poses", str(tmp_path / "traj.txt"), "--size", "67x45",
                           "--intrinsics", "57", "57.7", "33.1", "22.1", "--mode", "shaded-color", "--samples", "2"],
                          cwd=root, env=dict(os.environ, PYTHONPATH=root), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    assert sorted(os.listdir(out)) == ["mesh_0000.png", "mesh_0001.png", "mesh_0002.png"]
    viewer = MV.MeshViewer(ply, (67, 45), (57.0, 57.7, 33.1, 22.1), samples=2)
    poses = MV.load_poses(str(tmp_path / "traj.txt"))
    for t in range(3):
        picture = np.array(Image.open(os.path.join(out, f"mesh_{t:04d}.png")))
        assert picture.shape == (45, 67, 3) and picture.dtype == np.uint8
        want = viewer.render(poses[t], mode="shaded-color").cpu().numpy()
        assert np.array_equal(picture, want)
        assert (want != 255).any(axis=2).sum() > 200                               # the sphere is in the picture


def test_the_mesh_tool_writes_views_of_its_mesh(tmp_path):
    from PIL import Image
    from splatam_amd import mesh as M
    from splatam_amd import pipeline
    from test_gpu_mesh import _sequence
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    params, variables, stats = pipeline.rgbd_slam(ds, cfg, engine="fused")
    out = {n: v for n, v in params.items()}
    out['timestep'] = variables['timestep']
    out['intrinsics'] = ds[0][2][:3, :3].cpu().numpy()
    out['w2c'] = torch.linalg.inv(ds[0][3]).cpu().numpy()
    out['org_width'], out['org_height'] = 72, 40
    out['keyframe_time_indices'] = np.array(stats['keyframe_time_indices'])
    path = pipeline.save_params(out, str(tmp_path / "run"))
    ply, plain, pics = str(tmp_path / "mesh.ply"), str(tmp_path / "plain.ply"), str(tmp_path / "pics")
    assert M.main([path, "--out", ply, "--voxel", "0.05", "--sil-thres", "0.5", "--every", "2", "--views", pics, "--views-mode", "normal"]) == 0
    assert M.main([path, "--out", plain, "--voxel", "0.05", "--sil-thres", "0.5", "--every", "2"]) == 0
    assert open(ply, "rb").read() == open(plain, "rb").read()                      # the option adds pictures and changes nothing else
    names = sorted(os.listdir(pics))
    assert names == [f"mesh_{t:04d}.png" for t in range(0, len(ds), 2)]
    for n in names:
        picture = np.array(Image.open(os.path.join(pics, n)))
        assert picture.shape == (40, 72, 3) and (picture != 255).any(axis=2).mean() > 0.2      # the mesh fills a good part of the view
    # the viewer's own command on the written PLY with the run's poses: the same pictures (normal mode reads no colours)
    from splatam_amd import mesh_view as MV
    again = str(tmp_path / "again")
    assert MV.main([ply, "--out", again, "--params", path, "--mode", "normal", "--every", "2"]) == 0
    for n in names:
        assert np.array_equal(np.array(Image.open(os.path.join(again, n))), np.array(Image.open(os.path.join(pics, n)))), n


def test_session_extract_mesh_writes_views(tmp_path):
    from PIL import Image
    from splatam_amd import mesh_view as MV
    from splatam_amd.post_opt import estimated_w2c
    from splatam_amd.session import SlamSession
    from test_gpu_mesh import _sequence
    ds, cfg = _sequence()
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(voxel_size=0.05, sil_thres=0.5)
    with SlamSession(cfg, len(ds)) as session:
        for t in range(len(ds)):
            session.add_frame(*ds[t])
        plain = session.extract_mesh(**kw)
        mesh = session.extract_mesh(views=str(tmp_path / "pics"), views_mode="shaded-color", **kw)
        for a, b in zip(mesh, plain):
            assert torch.equal(a, b)                                                # the option adds pictures and changes nothing else
        frames = list(session.keyframe_time_indices) or list(range(session.frames_seen))
        assert sorted(os.listdir(tmp_path / "pics")) == sorted(f"mesh_{int(t):04d}.png" for t in frames)
        k = session.intrinsics.detach().cpu().double().numpy()
        t = int(frames[-1])
        w2c = estimated_w2c(session.engine.params, t).double().cpu().numpy() @ session.first_frame_w2c.double().cpu().numpy()
        want = MV.render_mesh(mesh, w2c, (k[0][0], k[1][1], k[0][2], k[1][2]), (72, 40), mode="shaded-color")
        assert np.array_equal(np.array(Image.open(tmp_path / "pics" / f"mesh_{t:04d}.png")), want.cpu().numpy())
        session.finish()
