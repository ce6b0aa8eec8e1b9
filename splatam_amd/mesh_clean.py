"""Clean a mesh: remove its small connected components, on the device.

A TSDF fused from rendered depth carries floaters -- shells and crumbs of a few dozen triangles in free space, left by silhouette edges
and half-transparent Gaussians.  Every one of them is sampled by ``mesh_score.score_mesh`` and charged to accuracy, and pulls ICP
correspondences.  The evaluation scripts this kind of map is compared with remove every small component right after extraction; this
module does it without the mesh leaving the device (csrc/meshclean.hip, loop bodies in csrc/meshclean_math.h):

``label_components``  C1: per vertex the smallest vertex index of its component -- a concurrent union-find over the faces, canonical.
``component_stats``   C2: per component its vertices, faces, area and box, by integer atomics only: the same bits on every run.
``clean_mesh``        the filter and the compaction (``mesh_render.cull_mesh``'s conventions and its code), ONE host read.

Two vertices belong to one component when a chain of faces that share a vertex INDEX joins them -- what
``trimesh.graph.connected_components`` computes on a mesh's edges.  Coincident vertices with different indices do not connect: meshes
from ``extract()`` are welded, a loaded PLY is taken as it is.  A face with a repeated index links the vertices it names and has area 0;
a face that names a vertex that does not exist links nothing and is dropped; a vertex no face names is a component of its own, with 0
faces.

Not here: welding, hole filling, smoothing, face-adjacency (edge-sharing) connectivity, a CPU path.
"""
from __future__ import annotations

import torch

from . import _capi
from ._mesh_common import _device, _ptr, _stream, _tensor
from .mesh import Mesh

AREA_QUANTUM = 2.0 ** -_capi.SPLAT_MESH_AREA_BITS
REPORT_KEYS = ("components", "components_kept", "faces", "faces_removed", "area_m2", "area_removed_m2")


def _faces(faces, what="faces"):
    if not (isinstance(faces, torch.Tensor) and faces.device.type == "cuda" and faces.dtype == torch.int32 and faces.dim() == 2
            and faces.shape[1] == 3):
        if isinstance(faces, torch.Tensor) and faces.device.type != "cuda":
            raise RuntimeError(f"{what} must be on a CUDA/HIP device; the HIP library has no CPU path")
        raise RuntimeError(f"{what} must be an int32 tensor [F, 3] on the device")
    return faces.contiguous()


def label_components(num_vertices, faces):
    """C1: ``labels`` [num_vertices] int32 on the device of ``faces`` [F, 3] int32, ``labels[v]`` the smallest vertex index of ``v``'s
    component.  Enqueued on the current stream; nothing is read."""
    faces = _faces(faces)
    V, F = int(num_vertices), int(faces.shape[0])
    if V < 0:
        raise ValueError("num_vertices must not be negative")
    dev = faces.device
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_components(_ptr(faces, F), F, V, _ptr(labels, V), _stream(dev)),
                    "splat_mesh_components")
    return labels


def key_to_float(keys):
    """The float32 values of the order-preserving int32 keys of ``splat_mesh_component_stats``'s boxes (the map is its own inverse)."""
    return torch.where(keys >= 0, keys, keys ^ 0x7fffffff).view(torch.float32)


def component_stats(mesh, labels=None):
    """C2: a dict of device tensors indexed by ROOT LABEL, each of length V: ``num_vertices`` / ``num_faces`` (int32), ``area`` (float64,
    m^2: an exact integer sum of per-face quanta of 2^-40 m^2, converted; good for about 8.4e6 m^2 per component), ``lo`` / ``hi``
    ([V, 3] float32: the component's box), ``is_root`` (bool: ``labels[v] == v``) and ``area_quanta`` (int64, the sum itself).  Entries
    of indices that are no root are 0 (NaN in ``lo`` / ``hi``).  ``mesh``: a ``Mesh`` of device tensors; ``labels``: what
    ``label_components`` gave, computed when None.  Enqueued; nothing is read."""
    v, f = mesh[0], _faces(mesh[1])
    dev = f.device
    v = _tensor(v, "vertices", torch.float32, ("V", 3), dev).contiguous()
    V, F = int(v.shape[0]), int(f.shape[0])
    labels = (label_components(V, f) if labels is None else _tensor(labels, "labels", torch.int32, (V,), dev)).contiguous()
    num_v, num_f = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    area_q = torch.empty(V, dtype=torch.int64, device=dev)
    lo, hi = torch.empty(V, 3, dtype=torch.int32, device=dev), torch.empty(V, 3, dtype=torch.int32, device=dev)
    p = (lambda t: t.data_ptr()) if V else (lambda t: None)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().splat_mesh_component_stats(p(v), V, _ptr(f, F), F, p(labels), p(num_v), p(num_f), p(area_q),
                                                           p(lo), p(hi), _stream(dev)), "splat_mesh_component_stats")
    return {"num_vertices": num_v, "num_faces": num_f, "area": area_q.double() * AREA_QUANTUM, "lo": key_to_float(lo), "hi": key_to_float(hi),
            "is_root": labels == torch.arange(V, dtype=torch.int32, device=dev), "area_quanta": area_q}


def surviving_components(stats, min_vertices=200, min_faces=0, min_area=0.0, min_extent=0.0, keep_largest=None):
    """bool [V] by root label: the components with at least one face that pass every threshold of ``clean_mesh``.  Nothing is read."""
    nf = stats["num_faces"]
    d = stats["hi"].double() - stats["lo"].double()
    extent = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    keep = (stats["is_root"] & (nf > 0) & (stats["num_vertices"] >= int(min_vertices)) & (nf >= int(min_faces))
            & (stats["area"] >= float(min_area)) & (extent >= float(min_extent)))
    if keep_largest is not None:
        k = int(keep_largest)
        if k <= 0:
            raise ValueError("keep_largest must be positive")
        # the k survivors with the most faces, ties to the lower label: a stable descending sort keeps equal counts in label order
        order = torch.sort(torch.where(keep, nf, torch.full_like(nf, -1)), descending=True, stable=True).indices[:k]
        top = torch.zeros_like(keep)
        top[order] = True
        keep = keep & top
    return keep


def clean_mesh(mesh, min_vertices=200, min_faces=0, min_area=0.0, min_extent=0.0, keep_largest=None, transform=None, device="cuda:0",
               report=False):
    """``mesh`` (a ``Mesh`` tuple of device tensors or host arrays, or the path of a PLY) without its small connected components, as a
    ``Mesh`` on the device.  A component with at least one face survives when it has ``num_vertices >= min_vertices``,
    ``num_faces >= min_faces``, ``area >= min_area`` (m^2), a box whose diagonal is ``>= min_extent`` (m) and, with ``keep_largest=k``,
    is among the ``k`` such components with the most faces (ties go to the lower label).

    Surviving faces keep their order, the vertices they name are renumbered densely in their order and colours travel with them;
    vertices no surviving face names are dropped, and so are faces that name a vertex that does not exist.  Nothing surviving gives the
    EMPTY ``Mesh`` (0 vertices, 0 faces) -- ``mesh_render.cull_mesh``'s conventions.  ``transform`` (4 x 4) is applied to the vertices
    first.  ONE host read, of the surviving sizes; with ``report=True`` the result is (the ``Mesh``, a dict) and the same read also
    brings ``components`` (those with a face), ``components_kept``, ``faces`` / ``faces_removed`` and ``area_m2`` /
    ``area_removed_m2``.  A mesh with a vertex that is not finite, or a component whose area is beyond the range of the integer sum,
    is refused (ValueError).

    ``min_vertices`` = 200 is recalled from the evaluation scripts of the Point-SLAM family, which remove every component with fewer
    vertices right after extraction; those scripts are not part of this project, so no parity is claimed."""
    dev = _device(device, "mesh cleaning")
    if int(min_vertices) < 0 or int(min_faces) < 0 or not float(min_area) >= 0 or not float(min_extent) >= 0:
        raise ValueError("clean_mesh needs thresholds that are not negative")
    if keep_largest is not None and int(keep_largest) <= 0:
        raise ValueError("keep_largest must be positive")
    from .mesh_render import _keep_faces, to_device_mesh
    m = to_device_mesh(mesh, dev, transform)
    v, f, c = m
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0 or V == 0:
        empty = Mesh(v[:0], f[:0], None if c is None else c[:0])
        return (empty, dict(zip(REPORT_KEYS, (0, 0, F, F, 0.0, 0.0)))) if report else empty
    labels = label_components(V, f)
    stats = component_stats(m, labels)
    survive = surviving_components(stats, min_vertices, min_faces, min_area, min_extent, keep_largest)
    valid = ((f >= 0) & (f < V)).all(dim=1)
    idx = f.clamp(0, V - 1).long()
    keep = survive[labels[idx[:, 0]].long()] & valid
    with_face = stats["is_root"] & (stats["num_faces"] > 0)
    q = stats["area_quanta"]
    bad = (~torch.isfinite(v).all()) | (q < 0).any() | (q >= _capi.SPLAT_MESH_AREA_BAD).any()
    extra = torch.stack((with_face.sum(), survive.sum(), q.sum(), torch.where(survive, q, torch.zeros_like(q)).sum(), bad.to(torch.int64)))
    out, got = _keep_faces(m, idx, keep, extra)
    components, kept, total_q, kept_q, refused = (int(x) for x in got)
    if refused:
        raise ValueError("clean_mesh: the mesh has a vertex that is not finite, or a component's area is beyond 2^23 m^2")
    if not report:
        return out
    return out, dict(zip(REPORT_KEYS, (components, kept, F, F - int(out.faces.shape[0]), total_q * AREA_QUANTUM, (total_q - kept_q) * AREA_QUANTUM)))


def clean_options(clean):
    """The ``clean_mesh`` keywords of a ``clean=`` option: ``None`` / ``False`` -> None (off), ``True`` -> {} (the defaults), a dict -> a copy."""
    if clean is None or clean is False:
        return None
    if clean is True:
        return {}
    if isinstance(clean, dict):
        bad = set(clean) - {"min_vertices", "min_faces", "min_area", "min_extent", "keep_largest"}
        if bad:
            raise ValueError(f"clean: unknown option(s) {sorted(bad)}")
        return dict(clean)
    raise ValueError(f"clean is None, True or a dict of clean_mesh keywords (got {clean!r})")


def format_cleaning(r):
    share = 100.0 * r["area_removed_m2"] / r["area_m2"] if r["area_m2"] > 0 else 0.0
    return (f"Cleaning: kept {r['components_kept']} of {r['components']} components, removed {r['faces_removed']} of {r['faces']} faces, "
            f"{r['area_removed_m2']:.6f} m^2 ({share:.4f} % of the area)")
