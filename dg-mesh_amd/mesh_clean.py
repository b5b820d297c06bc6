"""Cleaning an extracted mesh on the device: connected components, per-component statistics, selection and order-preserving
compaction -- verts_on_largest_mesh of the reference (R/nvdiffrast_utils/dpsr_utils.py:345-368, igl on the host; R/ = dgmesh/) and
its pymeshlab meshing_remove_connected_component_by_* calls (R/scene/gaussian_model.py:633-650), as kernels of csrc/mesh_clean.hip
(DESIGN.md section 4.13).  igl, trimesh and pymeshlab are neither vendored nor dependencies.

Definitions (this project's; include/dgmesh_hip.h states them for the C ABI):
  * a face is valid iff its three indices are in [0, V) and pairwise different; two vertices are connected when a valid face uses
    both -- connectivity through shared VERTICES, which is igl's adjacency_matrix + connected_components, not trimesh's shared-edge
    split; a vertex no valid face uses is a component of its own;
  * a component's label is its smallest vertex index;
  * the criteria combine by AND; invalid faces are always dropped, and so is every vertex no surviving face uses;
  * surviving vertices and faces keep their order.
Everything is integers, comparisons and copies: the results are bit-reproducible.  fp32 vertices, int32 faces, CUDA/HIP tensors only
-- no CPU fallback.  Host synchronisations: 8 bytes in connected_components (the count of out-of-range faces, which raises), 8 bytes
in clean_mesh (the output sizes)."""
from dataclasses import dataclass

import torch

from . import _lib, mesh_args


@dataclass(frozen=True)
class CleanSpec:
    """The criteria of clean_mesh.  largest: keep only the component with the most valid faces (ties: the smaller label);
    min_faces: drop components with fewer valid faces; min_diameter_frac: drop components whose bounding-box diagonal is below this
    fraction of the whole mesh's (measured against the whole mesh also when `largest` is set)."""
    largest: bool = False
    min_faces: int = 0
    min_diameter_frac: float = 0.0

    def any(self):
        return bool(self.largest) or self.min_faces > 0 or self.min_diameter_frac > 0.0

    def describe(self):
        return f"largest_component {int(bool(self.largest))} min_component_faces {int(self.min_faces)} min_component_diameter {float(self.min_diameter_frac):g}"


def as_spec(clean):
    """None, a CleanSpec or a dict of its fields -> CleanSpec or None ("do nothing")."""
    return mesh_args.spec_of("mesh_clean", "clean", CleanSpec, clean)


def tile():
    """The integers per workgroup of the compaction's scans (dgm_mesh_clean_tile)."""
    return int(_lib.lib().dgm_mesh_clean_tile())


def connected_components(faces, num_verts):
    """labels (num_verts,) int32: the smallest vertex index of each vertex's component.  Faces with a repeated index connect nothing;
    a face with an index outside [0, num_verts) raises ValueError naming their count (the kernel range-checks before it indexes)."""
    faces = mesh_args.faces("mesh_clean.connected_components", faces, num_verts)
    V, F = int(num_verts), int(faces.shape[0])
    L = _lib.lib()
    dev = faces.device
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = _lib.scratch(L.dgm_mesh_cc_scratch_bytes(V, F), dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_mesh_cc_label(V, F, _lib.vp(faces), _lib.vp(scratch), _lib.vp(labels), _lib.vp(info), _lib.stream_ptr()))
        bad = int(info[0])  # host synchronisation
    if bad:
        raise ValueError(f"mesh_clean.connected_components: {bad} of {F} faces have an index outside [0, {V})")
    return labels


def _stats(verts, faces, labels):
    L = _lib.lib()
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
    comp_faces = torch.empty(V, dtype=torch.int32, device=dev)
    comp_verts = torch.empty(V, dtype=torch.int32, device=dev)
    comp_bbox = torch.empty((V, 6), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_mesh_cc_stats(V, F, _lib.vp(verts), _lib.vp(faces), _lib.vp(labels), _lib.vp(comp_faces), _lib.vp(comp_verts), _lib.vp(comp_bbox),
                                       _lib.stream_ptr()))
    return comp_faces, comp_verts, comp_bbox


def component_table(verts, faces, labels=None):
    """One row per component, ordered by label: {"label", "faces" (valid faces), "verts": (C,) int32, "bbox_min", "bbox_max":
    (C, 3) float32}, device tensors.  labels: connected_components' (computed when None)."""
    verts, faces = mesh_args.mesh("mesh_clean.component_table", verts, faces)
    V = int(verts.shape[0])
    labels = connected_components(faces, V) if labels is None else mesh_args.labels("mesh_clean.component_table", labels, V, faces.device)
    comp_faces, comp_verts, comp_bbox = _stats(verts, faces, labels)
    roots = torch.nonzero(comp_verts > 0).flatten()
    return {"label": roots.to(torch.int32), "faces": comp_faces[roots], "verts": comp_verts[roots],
            "bbox_min": comp_bbox[roots, :3].contiguous(), "bbox_max": comp_bbox[roots, 3:].contiguous()}


def keep_mask(verts, faces, labels=None, *, largest=False, min_faces=0, min_diameter_frac=0.0):
    """(F,) uint8, 1 for the faces clean_mesh keeps."""
    verts, faces = mesh_args.mesh("mesh_clean.keep_mask", verts, faces)
    if int(min_faces) < 0 or not float(min_diameter_frac) >= 0.0:
        raise ValueError(f"mesh_clean: need min_faces >= 0 and min_diameter_frac >= 0, got {min_faces} and {min_diameter_frac}")
    L = _lib.lib()
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
    labels = connected_components(faces, V) if labels is None else mesh_args.labels("mesh_clean.keep_mask", labels, V, dev)
    comp_faces, comp_verts, comp_bbox = _stats(verts, faces, labels)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    scratch = _lib.scratch(L.dgm_mesh_cc_select_scratch_bytes(), dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_mesh_cc_select(V, F, _lib.vp(faces), _lib.vp(labels), _lib.vp(comp_faces), _lib.vp(comp_verts), _lib.vp(comp_bbox),
                                        int(bool(largest)), int(min_faces), float(min_diameter_frac), _lib.vp(scratch), _lib.vp(keep),
                                        _lib.stream_ptr()))
    return keep


def compact(verts, faces, keep):
    """The faces with keep != 0 and the vertices they use, in their old order: (verts', faces' re-indexed, vert_index, face_index),
    the last two int32, the old index of each survivor.  One 8-byte read-back (the sizes)."""
    verts, faces = mesh_args.mesh("mesh_clean.compact", verts, faces)
    V, F, dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
    if not torch.is_tensor(keep) or keep.device != dev or keep.dtype not in (torch.uint8, torch.bool) or tuple(keep.shape) != (F,):
        raise ValueError(f"mesh_clean.compact: keep must be ({F},) uint8 or bool on {dev}")
    keep = keep.contiguous().view(torch.uint8)
    L = _lib.lib()
    scratch = _lib.scratch(L.dgm_mesh_compact_scratch_bytes(V, F), dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_mesh_compact_count(V, F, _lib.vp(faces), _lib.vp(keep), _lib.vp(scratch), _lib.vp(counts), _lib.stream_ptr()))
        Vn, Fn = counts.tolist()  # the one host synchronisation: the output sizes
        verts_out = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
        faces_out = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
        vert_index = torch.empty(Vn, dtype=torch.int32, device=dev)
        face_index = torch.empty(Fn, dtype=torch.int32, device=dev)
        _lib.check(L.dgm_mesh_compact_emit(V, F, _lib.vp(verts), _lib.vp(faces), _lib.vp(scratch), Vn, Fn, _lib.vp(verts_out), _lib.vp(faces_out),
                                           _lib.vp(vert_index), _lib.vp(face_index), _lib.stream_ptr()))
    return verts_out, faces_out, vert_index, face_index


def clean_mesh(verts, faces, *, largest=False, min_faces=0, min_diameter_frac=0.0, return_index=False):
    """The mesh without the components that fail a criterion (CleanSpec), without invalid faces and without unused vertices:
    (verts', faces') or, with return_index, (verts', faces', vert_index, face_index) -- the old index of every survivor, with which
    a caller gathers per-vertex attributes.  An empty result has (0, 3) tensors."""
    keep = keep_mask(verts, faces, largest=largest, min_faces=min_faces, min_diameter_frac=min_diameter_frac)
    out = compact(verts, faces, keep)
    return out if return_index else out[:2]


def verts_on_largest_mesh(verts, faces):
    """The reference's name (R/nvdiffrast_utils/dpsr_utils.py:345): clean_mesh(largest=True), device tensors."""
    return clean_mesh(verts, faces, largest=True)


def apply(clean, verts, faces, *attributes):
    """clean (as_spec) applied to a mesh and per-vertex attribute tensors: (verts', faces', *attributes gathered with vert_index);
    the inputs themselves when clean is None."""
    spec = as_spec(clean)
    if spec is None:
        return (verts, faces) + attributes
    v, f, vi, _ = clean_mesh(verts, faces, largest=spec.largest, min_faces=spec.min_faces, min_diameter_frac=spec.min_diameter_frac,
                             return_index=True)
    vi = vi.long()
    return (v, f) + tuple(None if a is None else a[vi] for a in attributes)
