"""Map export next to ``params.npz`` ("the on-disk format ... and PLY export live next to it").

``save_ply`` writes what /root/reference/scripts/export_ply.py:20-42 writes -- a 3D-Gaussian-Splatting ``splat.ply`` with one float32
vertex element of 17 properties -- without the ``plyfile`` package (not installed here): the header is assembled by hand and the
table written in one piece.  Not on the hot path; kept because a user of the reference expects the file the viewers open."""
from __future__ import annotations

import numpy as np

PLY_ATTRS = ('x', 'y', 'z', 'nx', 'ny', 'nz', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity', 'scale_0', 'scale_1', 'scale_2',
             'rot_0', 'rot_1', 'rot_2', 'rot_3')
SH_C0 = 0.28209479177387814


def save_ply(path, means, scales, rotations, rgbs, opacities, normals=None):
    """Binary little-endian PLY, vertex properties ``PLY_ATTRS``: colours as the DC spherical-harmonic coefficient
    (rgb - 0.5) / C0, an isotropic [N, 1] scale column repeated to three, normals zero unless given; opacities stay logits and
    scales logs (the callers pass the raw parameters, as the reference does)."""
    means = np.asarray(means, dtype=np.float32)
    normals = np.zeros_like(means) if normals is None else np.asarray(normals, dtype=np.float32)
    scales = np.asarray(scales, dtype=np.float32)
    if scales.shape[1] == 1:
        scales = np.tile(scales, (1, 3))
    colors = (np.asarray(rgbs, dtype=np.float32) - 0.5) / SH_C0
    table = np.concatenate((means, normals, colors, np.asarray(opacities, dtype=np.float32).reshape(-1, 1), scales,
                            np.asarray(rotations, dtype=np.float32)), axis=1).astype('<f4')
    if table.shape[1] != len(PLY_ATTRS):
        raise ValueError(f"expected {len(PLY_ATTRS)} columns, got {table.shape[1]}")
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % table.shape[0]
    header += "".join(f"property float {a}\n" for a in PLY_ATTRS) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(table).tobytes())
    return path


def export_params_ply(params, path):
    """``params`` (the reference's dict, tensors or arrays: /root/reference/scripts/export_ply.py:63-73) -> ``path``."""
    def a(k):
        v = params[k]
        return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return save_ply(path, a('means3D'), a('log_scales'), a('unnorm_rotations'), a('rgb_colors'), a('logit_opacities'))


def save_mesh_ply(path, vertices, faces, colors=None):
    """A triangle mesh as binary little-endian PLY: ``vertices`` [V, 3] as float x, y, z, ``colors`` [V, 3] in 0..1 as uchar red, green,
    blue (rounded to nearest; left out when None), ``faces`` [F, 3] as ``list uchar int vertex_indices``.  What MeshLab, Open3D and
    trimesh open; written without the ``plyfile`` package, the tables in one piece each."""
    vertices = np.ascontiguousarray(np.asarray(vertices, dtype='<f4').reshape(-1, 3))
    faces = np.asarray(faces).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError("faces index vertices that do not exist")
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % vertices.shape[0]
    if colors is not None:
        colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if colors.shape[0] != vertices.shape[0]:
            raise ValueError(f"{colors.shape[0]} colours for {vertices.shape[0]} vertices")
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % faces.shape[0]
    vt = np.zeros(vertices.shape[0], dtype=fields)
    vt['x'], vt['y'], vt['z'] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    if colors is not None:
        bytes3 = np.rint(np.clip(np.nan_to_num(colors), 0.0, 1.0) * 255.0).astype(np.uint8)
        vt['red'], vt['green'], vt['blue'] = bytes3[:, 0], bytes3[:, 1], bytes3[:, 2]
    ft = np.zeros(faces.shape[0], dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    ft['n'], ft['v'] = 3, faces
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vt.tobytes())
        f.write(ft.tobytes())
    return path
