"""Repairing an extracted mesh on the device: a consistent, outward orientation per body (orient_faces) and the filling of small
holes (fill_holes), together repair_mesh -- kernels of csrc/mesh_repair.hip on the edge table of mesh_topology (DESIGN.md section
4.20).  The reference ends its mesh clean-up with pymeshlab's meshing_close_holes(maxholesize=1000) and trimesh's fill_holes,
fix_inversion and fix_normals (R/scene/gaussian_model.py:652-691; R/ = dgmesh/); trimesh, Open3D and pymeshlab are neither vendored
nor dependencies.  mesh_inside (and with it volume_iou), the genus of mesh_topology and the face normals mesh_ray uses all want a
watertight, consistently oriented mesh; vertex clustering and iso-surfaces cut by the grid box do not give one.

Definitions (this project's; include/dgmesh_hip.h states them for the C ABI, tests/_repair_ref.py restates them in numpy):
  * faces are valid as in mesh_topology; invalid faces are passed through untouched and never flipped;
  * two valid faces are adjacent when they share an edge that exactly two valid faces traverse: with counts (1, 1) they agree, with
    (2, 0) or (0, 2) they disagree; boundary and non-manifold edges connect nothing (trimesh's face_adjacency).  Components are those
    of this adjacency, labelled by their smallest face;
  * a component that cannot be oriented (the Moebius strip) is left exactly as it is; an orientable one that is open (a half-edge of
    it is not on a connecting edge) takes the consistent orientation that flips fewer faces and, on a tie, keeps its smallest face; a
    closed one takes, with outward=True, the orientation whose signed volume is positive (an integer sum, see the header; a sum of 0
    falls back to the open rule), with outward=False the open rule.  A flipped face (a, b, c) becomes (a, c, b);
  * a boundary half-edge is the side a->b the single valid face of a boundary edge traverses, indexed by its edge's rank among the
    boundary edges of the edge table; a vertex is simple when exactly one leaves it and one arrives; next(a->b) leaves b when b is
    simple.  A hole is a closed cycle of next with n <= max_hole_edges half-edges, its leader the smallest of them.  n == 3: one face
    (b, a, c') from the leader; n >= 4: one new vertex at the centroid (the rim summed in fp64 in loop order from the leader's tail,
    divided once, rounded to fp32 once) and one face (b, a, centroid) per rim half-edge a->b.  The given vertices and faces come
    first, unchanged; new vertices follow in leader order, new faces in half-edge order.
Everything is decided by integers: the results are identical bit for bit from run to run and equal to the numpy restatement.  fp32
vertices, int32 faces, CUDA/HIP tensors only -- no CPU fallback.  Host read-backs: 32 bytes per edge table, 32 for the counts of
orient_faces, 32 for the output sizes of fill_holes (between its count and its emit call).
Not done here: non-manifold edges and vertices stay, T-vertices stay, nothing is remeshed and fills are not refined.

Command line: python -m dgmesh_amd.mesh_repair in.ply out.ply [--max_hole_edges N] [--no_orient] [--no_outward] reads and writes
ply_io's triangle-mesh PLY, keeps vertex colours (a new vertex takes the mean of its rim) and prints one JSON line of info."""
import argparse
import json
from dataclasses import dataclass

import torch

from . import _lib, mesh_args

ORIENT_FIELDS = ("components", "closed_components", "unorientable_components", "faces_flipped", "components_inverted", "outward_skipped")
FILL_FIELDS = ("boundary_edges", "holes_filled", "holes_too_long", "edges_on_open_chains", "verts_added", "faces_added")


@dataclass(frozen=True)
class RepairSpec:
    """The parameters of repair_mesh."""
    orient: bool = True
    outward: bool = True
    max_hole_edges: int = 1000

    def describe(self):
        return f"orient {bool(self.orient)} outward {bool(self.outward)} max_hole_edges {int(self.max_hole_edges)}"


def as_spec(repair):
    """None, a RepairSpec or a dict of its fields -> RepairSpec or None ("do nothing")."""
    return mesh_args.spec_of("mesh_repair", "repair", RepairSpec, repair)


def _max_hole_edges(n):
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) < 2 ** 31:
        raise ValueError(f"mesh_repair: max_hole_edges must be an integer in [0, 2^31), got {n}")
    return int(n)


def _table(name, verts, faces):
    from .mesh_topology import EdgeTable
    return EdgeTable(name, faces, int(verts.shape[0]))


def _orient(table, verts, faces, outward):
    L, V, F, dev = table.L, table.V, table.F, table.dev
    nbytes = L.dgm_mesh_orient_scratch_bytes(V, F)
    scratch = _lib.scratch(nbytes, dev)
    out = torch.empty_like(faces)
    flipped = torch.empty(F, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_mesh_orient(V, F, _lib.vp(verts), _lib.vp(faces), _lib.vp(table.scratch), _lib.vp(scratch), 1 if outward else 0, _lib.vp(out),
                                     _lib.vp(flipped), _lib.vp(info), _lib.stream_ptr()))
        counts = dict(zip(ORIENT_FIELDS, info.tolist()))  # a host synchronisation: the counts
    return out, flipped, counts


def _fill(table, verts, faces, flipped, max_hole_edges):
    """faces: what is copied in front of the new faces (the oriented ones in repair_mesh); table: that of the unflipped faces."""
    L, V, F, dev = table.L, table.V, table.F, table.dev
    B = table.info["boundary_edges"]
    scratch = _lib.scratch(L.dgm_mesh_fill_scratch_bytes(V, B), dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = _lib.stream_ptr()
        _lib.check(L.dgm_mesh_fill_count(V, F, B, _lib.vp(verts), _lib.vp(table.scratch), _lib.vp(flipped), max_hole_edges, _lib.vp(scratch),
                                         _lib.vp(info), st))
        counts = dict(zip(FILL_FIELDS, info.tolist()))  # the one host synchronisation: the output sizes
        nv, nf = counts["verts_added"], counts["faces_added"]
        if nf == 0:
            return verts, faces, counts
        verts_out = torch.empty((V + nv, 3), dtype=torch.float32, device=dev)
        faces_out = torch.empty((F + nf, 3), dtype=torch.int32, device=dev)
        _lib.check(L.dgm_mesh_fill_emit(V, F, B, _lib.vp(verts), _lib.vp(faces), _lib.vp(scratch), nv, nf, _lib.vp(verts_out), _lib.vp(faces_out), st))
    return verts_out, faces_out, counts


def orient_faces(verts, faces, *, outward=True):
    """(faces' (F, 3) int32, flipped (F,) bool, info): every orientable body wound consistently and, with outward=True, every closed
    one with its normals outwards -- trimesh's fix_normals (fix_winding plus fix_inversion) per body, by the module docstring's rules.
    Nested inner shells are turned outward too, as trimesh's multibody fix_inversion does: a cavity's shell then adds its volume where
    it should subtract it, so orient a mesh with cavities with outward=False and decide them yourself.  The inputs are not modified.
    info: {"components", "closed_components", "unorientable_components", "faces_flipped", "components_inverted": closed components that
    the volume rule turned against the orientation that keeps their smallest face, "outward_skipped": 1 when outward was asked for and
    the box of the used vertices is not finite or has no extent (the volume rule is then skipped for the whole mesh)}."""
    verts, faces = mesh_args.mesh("mesh_repair.orient_faces", verts, faces)
    faces_out, flipped, info = _orient(_table("orient_faces", verts, faces), verts, faces, bool(outward))
    return faces_out, flipped.bool(), info


def fill_holes(verts, faces, *, max_hole_edges=1000):
    """(verts' (V + verts_added, 3), faces' (F + faces_added, 3), info): every hole of at most max_hole_edges rim edges closed (1000 is
    the reference's maxholesize), by the module docstring's rules, on the mesh as given -- use it after orient_faces, because the loop
    around a misoriented rim breaks and is skipped.  A hole of more than three edges is closed by a fan around its centroid: exact on
    planar star-shaped rims, which is what an iso-surface cut by the grid box leaves; it is NOT a minimum-weight triangulation, and a
    strongly non-convex rim gives overlapping triangles.  Without a hole to fill the inputs themselves are returned.
    info: {"boundary_edges", "holes_filled", "holes_too_long": closed rims of more than max_hole_edges edges, "edges_on_open_chains":
    boundary edges on rims that pass a vertex where more than one rim meets, "verts_added", "faces_added"}."""
    n = _max_hole_edges(max_hole_edges)
    given = (verts, faces)
    verts, faces = mesh_args.mesh("mesh_repair.fill_holes", verts, faces)
    v, f, info = _fill(_table("fill_holes", verts, faces), verts, faces, None, n)
    return (given[0] if v is verts else v, given[1] if f is faces else f, info)


def repair_mesh(verts, faces, *, orient=True, outward=True, max_hole_edges=1000):
    """(verts', faces', info): orient_faces (with orient=True), then fill_holes, on ONE edge table: a boundary edge stays a boundary
    edge when its face is flipped, and its direction follows the flip.  info: the two infos merged (without orient, those of
    fill_holes alone)."""
    n = _max_hole_edges(max_hole_edges)
    given = (verts, faces)
    verts, faces = mesh_args.mesh("mesh_repair.repair_mesh", verts, faces)
    table = _table("repair_mesh", verts, faces)
    info, flipped, oriented = {}, None, faces
    if orient:
        oriented, flipped, info = _orient(table, verts, faces, bool(outward))
    v, f, fill_info = _fill(table, verts, oriented, flipped, n)
    info.update(fill_info)
    return (given[0] if v is verts else v, given[1] if f is faces else f, info)


def apply_with_info(repair, verts, faces, *attributes):
    """((verts', faces', *attributes'), info of repair_mesh or None): apply, below, with the counts."""
    spec = as_spec(repair)
    if spec is None:
        return (verts, faces) + attributes, None
    V = int(verts.shape[0])
    v, f, info = repair_mesh(verts, faces, orient=spec.orient, outward=spec.outward, max_hole_edges=spec.max_hole_edges)
    nv = int(v.shape[0]) - V
    if nv == 0:
        return (v, f) + attributes, info
    fan = f[int(faces.shape[0]):].long()
    fan = fan[fan[:, 2] >= V]  # (b, a, new vertex): one per rim half-edge a->b, so every rim vertex is the `a` of exactly one
    out = []
    for attr in attributes:
        if attr is None:
            out.append(None)
            continue
        rows = attr[fan[:, 1]].to(torch.float32 if not attr.is_floating_point() else attr.dtype)
        total = torch.zeros((nv,) + tuple(attr.shape[1:]), dtype=rows.dtype, device=attr.device).index_add_(0, fan[:, 2] - V, rows)
        n = torch.zeros(nv, dtype=rows.dtype, device=attr.device).index_add_(0, fan[:, 2] - V, torch.ones(len(fan), dtype=rows.dtype, device=attr.device))
        mean = total / n.reshape((nv,) + (1,) * (attr.dim() - 1))
        out.append(torch.cat([attr, mean.to(attr.dtype)]))
    return (v, f) + tuple(out), info


def apply(repair, verts, faces, *attributes):
    """repair (as_spec) applied to a mesh: (verts', faces', *attributes') -- every per-vertex attribute (V, ...) gets one row per new
    vertex, the mean of its rim's rows (torch ops over the fill faces); None stays None; the inputs themselves when repair is None."""
    return apply_with_info(repair, verts, faces, *attributes)[0]


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_repair",
                                 description="Repair a triangle-mesh PLY on the GPU: orient every body consistently and outwards, fill small holes.")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--max_hole_edges", type=int, default=1000, help="the longest rim that is filled (the reference's maxholesize)")
    ap.add_argument("--no_orient", action="store_true", help="fill holes only")
    ap.add_argument("--no_outward", action="store_true", help="wind every body consistently, but do not turn closed ones outwards")
    return ap


def spec_from_args(args):
    return RepairSpec(orient=not args.no_orient, outward=not args.no_outward, max_hole_edges=args.max_hole_edges)


def main(argv=None):
    from .ply_io import read_mesh_ply_on_device, write_mesh_ply
    args = build_parser().parse_args(argv)
    spec = spec_from_args(args)
    _max_hole_edges(spec.max_hole_edges)
    (v, f, c), info = apply_with_info(spec, *read_mesh_ply_on_device(args.input, torch.device("cuda")))
    write_mesh_ply(args.output, v, f, vertex_colors=c)
    print(json.dumps({"input": args.input, "output": args.output, "verts": int(v.shape[0]), "faces": int(f.shape[0]), **info}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
