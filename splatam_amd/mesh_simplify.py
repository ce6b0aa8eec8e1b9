"""Simplify a mesh: vertex clustering with quadric placement, on the device.

A TSDF mesh carries its whole surface at the resolution of the voxels -- floors and walls are paid for at the same rate as chair legs --
and every layer downstream walks it.  This module makes it smaller without the mesh leaving the device (csrc/meshsimplify.hip, loop
bodies in csrc/meshsimplify_math.h): all vertices in one cell of a uniform grid of edge ``cell`` become one vertex, which sits where
the summed plane quadrics of the faces around the cell are smallest (P. Lindstrom, "Out-of-core simplification of large polygonal
models", SIGGRAPH 2000), so flat regions stay flat and edges and corners stay sharp; faces are renamed, faces that collapse go.

``cell_keys``      S0: per vertex the int64 key of its cell, -1 for a vertex that is not finite or lies beyond 2^20 cells of the origin.
``cluster_ids``    per vertex the rank of its key among the distinct keys (a stable sort, a flag, a prefix sum; no host read).
``cluster_sums``   S1 + S2: per cluster the count and 16 int64 words, by integer atomics only: the same bits on every run and order.
``simplify_mesh``  S3 (placement), S4 (faces), the optional removal of duplicate faces and the compaction (``mesh_render.cull_mesh``'s
                   conventions and its code), ONE host read.

The grid is anchored at the world origin, not at the mesh's box: a mesh and a piece of it cluster alike, and the output does not depend
on the order of vertices or faces -- the vertex and colour bytes are the same under any permutation of the input.

Not here: edge-collapse decimation to a target face count, normal-flip and fold-over tests, boundary and feature constraints, an
adaptive (octree) grid, pairing off opposite-wound twins, a CPU path, parity with Open3D's ``simplify_vertex_clustering``.
"""
from __future__ import annotations

import argparse
import math

import numpy as np
import torch

from . import _capi
from ._mesh_common import _device, _ptr, _stream, _tensor
from .mesh import Mesh

SUMS = _capi.SPLAT_MESH_SIMPLIFY_SUMS
AREA_QUANTUM = 2.0 ** -_capi.SPLAT_MESH_AREA_BITS
PLACEMENTS = {"mean": _capi.SPLAT_MESH_SIMPLIFY_MEAN, "quadric": _capi.SPLAT_MESH_SIMPLIFY_QUADRIC}
REPORT_KEYS = ("vertices", "faces", "vertices_kept", "faces_kept", "cells", "fallbacks", "rank1", "rank2", "rank3", "rms_plane_distance_m")


def _cell(cell):
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite, in metres (got {cell!r})")
    return cell


def _vertices(vertices):
    if isinstance(vertices, torch.Tensor) and vertices.device.type != "cuda":
        raise RuntimeError("vertices must be on a CUDA/HIP device; the HIP library has no CPU path")
    if not isinstance(vertices, torch.Tensor):
        raise RuntimeError("vertices must be a float32 tensor [V, 3] on the device")
    return _tensor(vertices, "vertices", torch.float32, ("V", 3), vertices.device).contiguous()


def cell_keys(vertices, cell):
    """S0: ``keys`` [V] int64 on the device of ``vertices`` [V, 3] float32: per axis ``i = floor(x / cell)`` in double,
    ``key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20)``; -1 for a vertex that is not finite or has ``|i| >= 2^20``.
    Enqueued on the current stream; nothing is read."""
    v, cell = _vertices(vertices), _cell(cell)
    V, dev = int(v.shape[0]), v.device
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_simplify_keys(_ptr(v, V), V, cell, _ptr(keys, V), _stream(dev)), "splat_mesh_simplify_keys")
    return keys


def cluster_ids(keys):
    """``cluster`` [V] int32: the rank of each key among the distinct keys >= 0 in ascending order, -1 for a key of -1.  Nothing is read."""
    keys = keys.reshape(-1)
    V = int(keys.shape[0])
    if V == 0:
        return torch.empty(0, dtype=torch.int32, device=keys.device)
    sorted_keys, order = torch.sort(keys, stable=True)
    first = torch.ones(V, dtype=torch.bool, device=keys.device)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    live = sorted_keys >= 0
    rank = torch.cumsum((first & live).to(torch.int32), 0, dtype=torch.int32) - 1
    cluster = torch.empty(V, dtype=torch.int32, device=keys.device)
    cluster[order] = torch.where(live, rank, torch.full_like(rank, -1))
    return cluster


def cluster_sums(mesh, cell, cluster=None, quadrics=True):
    """S1 + S2: a dict of device tensors indexed by CLUSTER, each of length V: ``count`` (int32), ``sums`` ([V, 16] int64: the sums of
    ``rint(p 2^32)`` [0:3] and ``rint(colour 2^32)`` [3:6], the quadric ``area {n n^T, d n, d^2}`` in quanta of 2^-40 m^2 [6:16]),
    ``cell_keys`` (int64, -1 beyond the last cluster), ``cluster`` (int32 [V], per VERTEX) and ``refused`` (int32 [1]: a face's area was
    beyond 2^22 m^2).  ``mesh``: a ``Mesh`` of device tensors; ``cluster``: what ``cluster_ids(cell_keys(...))`` gave, computed when
    None.  ``quadrics=False`` skips S2.  Enqueued; nothing is read."""
    cell = _cell(cell)
    v = _vertices(mesh[0])
    dev = v.device
    f = _tensor(mesh[1], "faces", torch.int32, ("F", 3), dev).contiguous()
    c = mesh[2] if len(mesh) > 2 else None
    V, F = int(v.shape[0]), int(f.shape[0])
    if c is not None:
        c = _tensor(c, "colors", torch.float32, (V, 3), dev).contiguous()
    keys = cell_keys(v, cell)
    cluster = (cluster_ids(keys) if cluster is None else _tensor(cluster, "cluster", torch.int32, (V,), dev)).contiguous()
    count = torch.zeros(V, dtype=torch.int32, device=dev)
    sums = torch.zeros(V, SUMS, dtype=torch.int64, device=dev)
    refused = torch.zeros(1, dtype=torch.int32, device=dev)
    # the key of each cluster's cell: every vertex of a cluster writes the same value
    per_cluster = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    per_cluster.scatter_(0, torch.where(cluster >= 0, cluster, torch.full_like(cluster, V)).long(), keys)
    L = _capi.lib()
    with torch.cuda.device(dev):
        _capi.check(L.splat_mesh_simplify_vertices(_ptr(v, V), None if c is None else _ptr(c, V), V, _ptr(cluster, V), cell, _ptr(count, V),
                                                   _ptr(sums, V), _stream(dev)), "splat_mesh_simplify_vertices")
        if quadrics:
            _capi.check(L.splat_mesh_simplify_quadrics(_ptr(v, V), V, _ptr(f, F), F, _ptr(cluster, V), cell, _ptr(sums, V), refused.data_ptr(),
                                                       _stream(dev)), "splat_mesh_simplify_quadrics")
    return {"count": count, "sums": sums, "cell_keys": per_cluster[:V].contiguous(), "cluster": cluster, "refused": refused, "keys": keys}


def place_clusters(acc, cell, placement="quadric", colors=False):
    """S3: a dict of device tensors by cluster from what ``cluster_sums`` gave: ``positions`` [V, 3] float32, ``colors`` ([V, 3] float32, or
    None), ``rank`` / ``fallback`` (int32) and ``value`` (float64, the quadric at the point).  Enqueued; nothing is read."""
    cell = _cell(cell)
    if placement not in PLACEMENTS:
        raise ValueError(f"placement is \"quadric\" or \"mean\" (got {placement!r})")
    count = acc["count"]
    V, dev = int(count.shape[0]), count.device
    positions = torch.empty(V, 3, dtype=torch.float32, device=dev)
    mean_colors = torch.empty(V, 3, dtype=torch.float32, device=dev) if colors else None
    rank, fallback = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    value = torch.empty(V, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_simplify_place(_ptr(count, V), _ptr(acc["sums"], V), _ptr(acc["cell_keys"], V), V, cell,
                                                          PLACEMENTS[placement], _ptr(positions, V), None if mean_colors is None else _ptr(mean_colors, V),
                                                          _ptr(rank, V), _ptr(fallback, V), _ptr(value, V), _stream(dev)),
                    "splat_mesh_simplify_place")
    return {"positions": positions, "colors": mean_colors, "rank": rank, "fallback": fallback, "value": value}


def cluster_faces(faces, cluster):
    """S4: ``triples`` [F, 3] int32: each face's clusters rotated so that the smallest comes first, (-1, -1, -1) for a face that goes."""
    V, F, dev = int(cluster.shape[0]), int(faces.shape[0]), cluster.device
    triples = torch.empty(F, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_simplify_faces(_ptr(faces, F), F, V, _ptr(cluster, V), _ptr(triples, F), _stream(dev)),
                    "splat_mesh_simplify_faces")
    return triples


def first_of_each_triple(triples, keep):
    """``keep`` without the faces whose rotated triple a kept face of LOWER index has too: two stable sorts (by the last two ids, then by
    the first), a flag where a triple differs from its predecessor, scattered back.  Nothing is read."""
    F = int(triples.shape[0])
    t = triples.long()
    low = torch.where(keep, (t[:, 1] << 31) | t[:, 2], torch.full((F,), -1, dtype=torch.int64, device=triples.device))
    order = torch.sort(low, stable=True).indices
    order = order[torch.sort(t[order, 0], stable=True).indices]         # equal triples are now neighbours, in input order
    s = t[order]
    first = torch.ones(F, dtype=torch.bool, device=triples.device)
    first[1:] = (s[1:] != s[:-1]).any(dim=1)
    out = torch.empty_like(keep)
    out[order] = first
    return out & keep


def _face_indices(triples, V):
    """``triples`` as the int64 indices ``_keep_faces`` wants.  A face that goes names (-1, -1, -1) and adds zeros there: its indices are
    spread over the vertices, because a million atomic adds of zero to ONE word take longer than everything else together."""
    F = int(triples.shape[0])
    spread = (torch.arange(F, dtype=torch.int64, device=triples.device) % max(V, 1))[:, None].expand(F, 3)
    return torch.where(triples >= 0, triples.long(), spread)


def _empty(m, V, F, report):
    v, f, c = m
    empty = Mesh(v[:0], f[:0], None if c is None else c[:0])
    return (empty, dict(zip(REPORT_KEYS, (V, F, 0, 0, 0, 0, 0, 0, 0, 0.0)))) if report else empty


def simplify_mesh(mesh, cell, placement="quadric", dedupe=True, transform=None, device="cuda:0", report=False):
    """``mesh`` (a ``Mesh`` tuple of device tensors or host arrays, or the path of a PLY) with all vertices of one cell of a uniform grid
    of edge ``cell`` (metres, anchored at the world origin) merged into one, as a ``Mesh`` on the device.

    ``placement="quadric"`` puts that vertex where the summed plane quadrics of the faces around the cell are smallest, within the cell
    (the mean where the quadric says nothing, or would leave the cell); ``"mean"`` takes the mean and skips the quadrics.  Colours are
    the cluster's mean.  A face survives when its three vertices fall into three different cells; it is renamed and rotated so that
    its smallest index comes first, the winding kept.  With ``dedupe``, of several faces with the same rotated triple only the one of
    lowest input index stays (opposite-wound twins are not paired off); ``dedupe=False`` keeps a closed mesh closed.  Surviving
    faces keep their order; vertices are numbered in ascending order of their cell's key (z, then y, then x) and those no surviving
    face names are dropped, as are faces that name a vertex that does not exist or is not finite.  Nothing surviving gives the EMPTY
    ``Mesh``.  ``transform`` (4 x 4) is applied to the vertices first.  The output does not depend on the order of the input's
    vertices or faces.

    ONE host read, of the surviving sizes; with ``report=True`` the result is (the ``Mesh``, a dict) and the same read also brings
    ``vertices`` / ``faces`` (of the input), ``vertices_kept`` / ``faces_kept``, ``cells`` (occupied), ``fallbacks`` (cells where the
    mean was taken for the quadric's point), ``rank1`` / ``rank2`` / ``rank3`` (cells placed on a plane, an edge, a corner) and
    ``rms_plane_distance_m``: ``cell sqrt(sum of the quadrics' values / sum of the areas)``, the area-weighted RMS distance of the new
    vertices from the planes they replace.  A finite vertex beyond 2^20 cells of the origin, or a face whose area is beyond the range
    of the integer sums, is refused (ValueError)."""
    dev = _device(device, "mesh simplification")
    cell = _cell(cell)
    if placement not in PLACEMENTS:
        raise ValueError(f"placement is \"quadric\" or \"mean\" (got {placement!r})")
    from .mesh_render import _keep_faces, to_device_mesh
    m = to_device_mesh(mesh, dev, transform)
    v, f, c = m
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0 or V == 0:
        return _empty(m, V, F, report)
    acc = cluster_sums(m, cell, quadrics=placement == "quadric")
    placed = place_clusters(acc, cell, placement, colors=c is not None)
    triples = cluster_faces(f, acc["cluster"])
    keep = triples[:, 0] >= 0
    if dedupe:
        keep = first_of_each_triple(triples, keep)
    occupied = acc["count"] > 0
    rank, sums = placed["rank"], acc["sums"]
    beyond = (torch.isfinite(v).all(dim=1) & (acc["keys"] < 0)).any()
    area = (sums[:, 6] + sums[:, 9] + sums[:, 11]).sum()                # (n is a unit vector: the trace of area n n^T is the area)
    extra = torch.stack((occupied.sum(), (placed["fallback"] > 0).sum(), (rank == 1).sum(), (rank == 2).sum(), (rank == 3).sum(), area,
                         placed["value"].sum().reshape(1).view(torch.int64)[0], beyond.to(torch.int64), acc["refused"][0].to(torch.int64)))
    out, got = _keep_faces(Mesh(placed["positions"], triples, placed["colors"]), _face_indices(triples, V), keep, extra)
    cells, fallbacks, rank1, rank2, rank3, area_q, value_bits, beyond, refused = (int(x) for x in got)
    if beyond:
        raise ValueError(f"simplify_mesh: a vertex lies beyond 2^20 cells of {cell} m from the origin")
    if refused:
        raise ValueError("simplify_mesh: a face's area is beyond 2^22 m^2, the range of the integer sums")
    if not report:
        return out
    value = float(np.array([value_bits], dtype=np.int64).view(np.float64)[0])
    rms = cell * math.sqrt(max(value, 0.0) / (area_q * AREA_QUANTUM)) if area_q > 0 else 0.0
    return out, dict(zip(REPORT_KEYS, (V, F, int(out.vertices.shape[0]), int(out.faces.shape[0]), cells, fallbacks, rank1, rank2, rank3, rms)))


def simplify_options(simplify):
    """The ``simplify_mesh`` keywords of a ``simplify=`` option: ``None`` / ``False`` -> None (off), a number -> ``{"cell": number}``,
    a dict (which must name ``cell``) -> a copy."""
    if simplify is None or simplify is False:
        return None
    if isinstance(simplify, dict):
        bad = set(simplify) - {"cell", "placement", "dedupe"}
        if bad:
            raise ValueError(f"simplify: unknown option(s) {sorted(bad)}")
        if "cell" not in simplify:
            raise ValueError("simplify: a dict must name the cell")
        options = dict(simplify)
    elif isinstance(simplify, (int, float)) and not isinstance(simplify, bool):
        options = {"cell": simplify}
    else:
        raise ValueError(f"simplify is None, a cell size in metres or a dict of simplify_mesh keywords (got {simplify!r})")
    options["cell"] = _cell(options["cell"])
    if options.get("placement", "quadric") not in PLACEMENTS:
        raise ValueError(f"simplify: placement is \"quadric\" or \"mean\" (got {options['placement']!r})")
    return options


def _simplified(mesh, simplify, device, simplification=None):
    """``mesh`` as ``simplify`` (what ``simplify_options`` returned) asks for it: as it is (None), or ``simplify_mesh`` of it with those
    keywords; ``simplification``, a dict, then receives the report."""
    if simplify is None:
        return mesh
    mesh, found = simplify_mesh(mesh, device=device, report=True, **simplify)
    if simplification is not None:
        simplification.update(found)
    return mesh


def format_simplification(r):
    share = lambda kept, of: 100.0 * kept / of if of else 0.0       # noqa: E731
    return (f"Simplification: {r['vertices_kept']} of {r['vertices']} vertices ({share(r['vertices_kept'], r['vertices']):.2f} %), "
            f"{r['faces_kept']} of {r['faces']} faces ({share(r['faces_kept'], r['faces']):.2f} %), {r['cells']} cells "
            f"(plane {r['rank1']}, edge {r['rank2']}, corner {r['rank3']}, mean {r['fallbacks']}), "
            f"RMS distance from the replaced planes {1000.0 * r['rms_plane_distance_m']:.4f} mm")


def _parser():
    parser = argparse.ArgumentParser(prog="python -m splatam_amd.mesh_simplify", description="Simplify a PLY mesh by quadric vertex clustering.")
    parser.add_argument("input", help="the mesh to simplify (PLY)")
    parser.add_argument("output", help="where the simplified mesh is written (PLY)")
    parser.add_argument("--cell", type=float, required=True, metavar="M", help="edge of the grid's cells, metres")
    parser.add_argument("--placement", choices=sorted(PLACEMENTS), default="quadric", help="where a cell's vertex sits (quadric)")
    parser.add_argument("--no-dedupe", action="store_true", help="keep faces that repeat another face's triple")
    parser.add_argument("--transform", default=None, metavar="FILE", help="a 4 x 4 matrix (text) applied to the vertices first")
    parser.add_argument("--device", default="cuda:0")
    return parser


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    if not (args.cell > 0 and math.isfinite(args.cell)):
        parser.error("--cell must be positive and finite")
    from .export import save_mesh_ply
    transform = None if args.transform is None else np.loadtxt(args.transform).reshape(4, 4)
    mesh, found = simplify_mesh(args.input, args.cell, placement=args.placement, dedupe=not args.no_dedupe, transform=transform,
                                device=args.device, report=True)
    save_mesh_ply(args.output, *mesh)
    print(format_simplification(found), flush=True)
    return found


if __name__ == "__main__":
    main()
