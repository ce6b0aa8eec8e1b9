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


def save_mesh_ply(path, vertices, faces, colors=None, normals=None):
    """A triangle mesh as binary little-endian PLY: ``vertices`` [V, 3] as float x, y, z, ``normals`` [V, 3] as float nx, ny, nz (left
    out when None: the file is then byte for byte what it was without the parameter), ``colors`` [V, 3] in 0..1 as uchar red, green,
    blue (rounded to nearest; left out when None), ``faces`` [F, 3] as ``list uchar int vertex_indices``.  What MeshLab, Open3D and
    trimesh open; written without the ``plyfile`` package, the tables in one piece each."""
    vertices = np.ascontiguousarray(np.asarray(vertices, dtype='<f4').reshape(-1, 3))
    faces = np.asarray(faces).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError("faces index vertices that do not exist")
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % vertices.shape[0]
    if normals is not None:
        normals = np.asarray(normals, dtype='<f4').reshape(-1, 3)
        if normals.shape[0] != vertices.shape[0]:
            raise ValueError(f"{normals.shape[0]} normals for {vertices.shape[0]} vertices")
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if colors.shape[0] != vertices.shape[0]:
            raise ValueError(f"{colors.shape[0]} colours for {vertices.shape[0]} vertices")
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % faces.shape[0]
    vt = np.zeros(vertices.shape[0], dtype=fields)
    vt['x'], vt['y'], vt['z'] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    if normals is not None:
        vt['nx'], vt['ny'], vt['nz'] = normals[:, 0], normals[:, 1], normals[:, 2]
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


PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
             'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _fan(counts, flat):
    """Triangles of polygons given as ``counts`` [F] and the concatenated ``flat`` indices: a fan from each polygon's first vertex."""
    counts = counts.astype(np.int64)
    if counts.size and (counts == counts[0]).all() and counts[0] >= 3:          # the usual file: all triangles, or all quads
        poly = flat.reshape(-1, int(counts[0]))
        return np.stack([poly[:, [0, k, k + 1]] for k in range(1, poly.shape[1] - 1)], axis=1).reshape(-1, 3)
    first = np.concatenate(([0], np.cumsum(counts)[:-1]))
    tris, owner = [np.zeros((0, 3), dtype=flat.dtype)], [np.zeros(0, dtype=np.int64)]
    for k in range(1, int(counts.max(initial=0)) - 1):                   # triangle k of every polygon that has one
        m = np.nonzero(counts > k + 1)[0]
        tris.append(np.stack((flat[first[m]], flat[first[m] + k], flat[first[m] + k + 1]), axis=1))
        owner.append(m)
    return np.concatenate(tris, axis=0)[np.argsort(np.concatenate(owner), kind="stable")]           # (polygon by polygon, in file order)


def load_mesh_ply(path):
    """``(vertices float32 [V, 3], faces int32 [F, 3], colors float32 [V, 3] in 0..1 or None)`` of an ASCII or binary little-endian PLY:
    any scalar vertex properties (x, y, z and, when all three are there, red, green, blue are used), a face list of any integer count
    and index type, polygons fan-triangulated from their first vertex (Replica's own meshes are quads).  Elements other than vertex and
    face may follow the two.  ValueError, naming the file, for a big-endian file, a file without faces and anything that is not such a
    PLY.  numpy only; reads back what ``save_mesh_ply`` writes."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            if w[1] == "list":
                elements[-1][2].append((w[4], PLY_TYPES.get(w[2]), PLY_TYPES.get(w[3])))
            else:
                elements[-1][2].append((w[2], PLY_TYPES.get(w[1]), None))
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: big-endian PLY files are not read; convert the file to binary_little_endian or ascii")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    names = [e[0] for e in elements]
    if names[:1] != ["vertex"]:
        raise ValueError(f"{path}: the first element of a mesh PLY must be vertex")
    if names[1:2] != ["face"] or elements[1][1] == 0:
        raise ValueError(f"{path}: the file has no faces (a point cloud cannot be scored as a mesh)")
    (_, V, vprops), (_, F, fprops) = elements[0], elements[1]
    if any(t is None or l is not None for _, t, l in vprops) or len(fprops) < 1 or fprops[0][2] is None or fprops[0][1] is None \
            or fprops[0][1][0] == 'f' or fprops[0][2][0] == 'f' or any(t is None for _, t, _ in fprops[1:]):
        raise ValueError(f"{path}: vertex properties must be scalars and the first face property an integer list")
    vnames = [n for n, _, _ in vprops]
    if not all(a in vnames for a in "xyz"):
        raise ValueError(f"{path}: the vertices have no x, y, z")
    body = data[nl + 1:]
    if fmt == "ascii":
        tokens = body.split()
        nv = V * len(vprops)
        table = np.array(tokens[:nv], dtype=np.float64).reshape(V, len(vprops))
        cols = {n: table[:, k] for k, n in enumerate(vnames)}
        rest, counts, flat, pos = tokens[nv:], np.zeros(F, dtype=np.int64), [], 0
        extra = len(fprops) - 1                                          # (scalar face properties after the list)
        if any(l is not None for _, _, l in fprops[1:]):
            raise ValueError(f"{path}: a second list property on the faces is not read")
        for m in range(F):
            c = int(rest[pos])
            counts[m] = c
            flat.extend(rest[pos + 1:pos + 1 + c])
            pos += 1 + c + extra
        flat = np.array(flat, dtype=np.int64)
    else:
        vdtype = np.dtype([(n, '<' + t) for n, t, _ in vprops])
        if len(body) < V * vdtype.itemsize:
            raise ValueError(f"{path}: the file ends inside the vertices")
        table = np.frombuffer(body, dtype=vdtype, count=V)
        cols = {n: table[n] for n in vnames}
        fb = body[V * vdtype.itemsize:]
        ct, it = np.dtype('<' + fprops[0][1]), np.dtype('<' + fprops[0][2])
        if len(fprops) != 1:
            raise ValueError(f"{path}: binary faces with properties besides the index list are not read")
        if len(fb) < ct.itemsize:
            raise ValueError(f"{path}: the file ends inside the faces")
        c0 = int(np.frombuffer(fb, dtype=ct, count=1)[0])
        rec = np.dtype([('n', ct), ('v', it, (c0,))])
        uniform = None
        if c0 >= 1 and len(fb) >= F * rec.itemsize:
            uniform = np.frombuffer(fb, dtype=rec, count=F)
            if not (uniform['n'] == c0).all():
                uniform = None
        if uniform is not None:
            counts, flat = np.full(F, c0, dtype=np.int64), uniform['v'].reshape(-1).astype(np.int64)
        else:                                                            # mixed polygons: one face at a time
            counts, flat, pos = np.zeros(F, dtype=np.int64), [], 0
            for m in range(F):
                if pos + ct.itemsize > len(fb):
                    raise ValueError(f"{path}: the file ends inside the faces")
                c = int(np.frombuffer(fb, dtype=ct, count=1, offset=pos)[0])
                pos += ct.itemsize
                if pos + c * it.itemsize > len(fb):
                    raise ValueError(f"{path}: the file ends inside the faces")
                flat.append(np.frombuffer(fb, dtype=it, count=c, offset=pos).astype(np.int64))
                counts[m] = c
                pos += c * it.itemsize
            flat = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int64)
    vertices = np.stack([np.asarray(cols[a], dtype=np.float32) for a in "xyz"], axis=1)
    colors = None
    if all(a in cols for a in ("red", "green", "blue")):
        scale = {n: (255.0 if t[0] in "iu" else 1.0) for n, t, _ in vprops}
        colors = np.stack([np.asarray(cols[a], dtype=np.float32) / np.float32(scale[a]) for a in ("red", "green", "blue")], axis=1)
    faces = _fan(counts, flat)
    if faces.shape[0] == 0:
        raise ValueError(f"{path}: the file has no faces (a point cloud cannot be scored as a mesh)")
    if faces.min() < 0 or faces.max() >= V:
        raise ValueError(f"{path}: faces index vertices that do not exist")
    return np.ascontiguousarray(vertices), np.ascontiguousarray(faces.astype(np.int32)), colors
