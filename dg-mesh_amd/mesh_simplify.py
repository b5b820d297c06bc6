"""Simplifying an extracted mesh on the device: uniform-grid vertex clustering with quadric-error placement (Lindstrom 2000), as
kernels of csrc/mesh_simplify.hip.  With a tiny cell it is the rest of the reference's clean_mesh
(R/scene/gaussian_model.py:603-697; R/ = dgmesh/): pymeshlab's meshing_merge_close_vertices, meshing_remove_duplicate_faces and
meshing_remove_null_faces.  pymeshlab and trimesh are neither vendored nor dependencies.

Definitions (this project's; include/dgmesh_hip.h states them for the C ABI, tests/_simplify_ref.py restates them in numpy):
  * a face is valid iff its three indices are in [0, V) and pairwise different and its nine coordinates are finite; invalid faces
    are dropped (out-of-range indices are range-checked before any use);
  * the box is the per-axis min o and max hi over the vertices of the valid faces, floats ordered by their bits;
  * cells: n_k = max(1, ceil((hi_k - o_k) / h)), idx_k = min(n_k - 1, floor((x_k - o_k) / h)) in fp32 with correctly rounded subtract
    and divide; more than 2^20 cells along an axis is refused; the cell key is (idx_z n_y + idx_y) n_x + idx_x, 64-bit;
  * a cluster is the set of used vertices of one occupied cell, its representative its smallest old vertex index; new vertices are
    ordered by representative; vert_map (V,) int32 old -> new, -1 for a vertex no surviving face uses; vert_index new -> representative;
  * every valid face is remapped; it is null when two new indices coincide and a duplicate when a face with a smaller old index has
    the same unordered triple; both are dropped, survivors keep their order, face_index new -> old; a cluster left without a face is
    dropped.  Winding is kept as remapped: clustering can flip a triangle, which is not repaired;
  * placement, fp64 from the fp32 inputs: per cluster with cell centre c = o + (idx + 0.5) h, over the valid faces with at least one
    corner in it, each once, in ascending old face index: n = (p1 - p0) x (p2 - p0), d = -n . (p0 - c), g = (p0 + p1 + p2) / 3 - c;
    A = sum n n^T, b = sum n d, xh = (sum g) / |S|; mu = regularization * tr(A); mu == 0: x = xh, otherwise (A + mu I) x = mu xh - b;
    x is clamped per component to [-h, h]; the new vertex is fp32(c + x).  (The Tikhonov term stands for Lindstrom's singular-value
    truncation, the clamp for his outside-the-cell fallback: both are continuous.)
  * `grid` G means h = fp32(longest box side) / fp32(G) in fp32 (1 when that is not positive).
Every output is identical bit for bit from run to run: the per-cluster sums run over an inverted index in ascending face order and
no float is added by an atomic.  fp32 vertices, int32 faces, CUDA/HIP tensors only -- no CPU fallback.

Host read-backs of simplify_mesh: two with `cell` or `grid`, 24 bytes (the box) and 8 bytes (the output sizes); with `target_faces` the
box and 8 bytes per count-only pass of the bisection, 11 at the most (the pass that is kept is not repeated).

Command line: python -m dgmesh_amd.mesh_simplify in.ply out.ply (--cell H | --grid G | --target_faces N) [--regularization E]
reads and writes ply_io's triangle-mesh PLY and keeps vertex colours (a new vertex takes its representative's)."""
import argparse
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, mesh_args

MAX_DIM = 1 << 20
GRID_RANGE = (2, 1024)
MAX_COUNT_PASSES = 10


@dataclass(frozen=True)
class SimplifySpec:
    """The parameters of simplify_mesh: exactly one of cell (the cell size h), grid (cells along the longest box axis) and
    target_faces (bisection over grid for at most that many faces); regularization: the Tikhonov weight relative to tr(A)."""
    cell: float = None
    grid: int = None
    target_faces: int = None
    regularization: float = 1e-3

    def describe(self):
        return f"cell {self.cell} grid {self.grid} target_faces {self.target_faces} regularization {float(self.regularization):g}"


def as_spec(simplify):
    """None, a SimplifySpec or a dict of its fields -> SimplifySpec or None ("do nothing")."""
    return mesh_args.spec_of("mesh_simplify", "simplify", SimplifySpec, simplify)


def _choice(cell, grid, target_faces, regularization):
    given = [k for k, v in (("cell", cell), ("grid", grid), ("target_faces", target_faces)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"mesh_simplify: exactly one of cell, grid and target_faces must be given, got {', '.join(given) or 'none'}")
    if cell is not None and not (np.float32(cell) > 0 and np.isfinite(np.float32(cell))):
        raise ValueError(f"mesh_simplify: cell must be a finite fp32 size > 0, got {cell}")
    if grid is not None and (int(grid) != grid or not 1 <= int(grid) <= MAX_DIM):
        raise ValueError(f"mesh_simplify: grid must be an integer in [1, 2^20], got {grid}")
    if target_faces is not None and (int(target_faces) != target_faces or int(target_faces) < 1):
        raise ValueError(f"mesh_simplify: target_faces must be an integer >= 1, got {target_faces}")
    if not (float(regularization) >= 0.0 and np.isfinite(float(regularization))):
        raise ValueError(f"mesh_simplify: regularization must be finite and >= 0, got {regularization}")


def grid_cell(box, grid):
    """h of `grid` cells along the longest side of box = (o, hi): fp32(longest) / fp32(grid) in fp32; 1 when that is not positive."""
    o, hi = np.asarray(box[:3], np.float32), np.asarray(box[3:], np.float32)
    with np.errstate(all="ignore"):
        h = np.float32(np.max((hi - o).astype(np.float32)) / np.float32(grid))
    return h if h > 0 and np.isfinite(h) else np.float32(1.0)


def grid_dims(box, h):
    """(n_x, n_y, n_z) of the box at cell size h, in fp32; refuses more than 2^20 cells along an axis."""
    o, hi = np.asarray(box[:3], np.float32), np.asarray(box[3:], np.float32)
    with np.errstate(all="ignore"):
        q = np.ceil((hi - o).astype(np.float32) / np.float32(h))
    if not (q <= MAX_DIM).all():
        raise ValueError(f"mesh_simplify: a box of {(hi - o).tolist()} at cell size {float(h):g} needs {q.tolist()} cells per axis, "
                         f"over the limit of 2^20")
    return tuple(int(max(1, n)) for n in q)


class _State:
    """What one count pass leaves on the device and the placement continues from."""

    def __init__(self, L, V, F, dev, nbytes):
        self.scratch = _lib.scratch(nbytes, dev)
        self.cscratch = _lib.scratch(L.dgm_mesh_compact_scratch_bytes(V, F), dev)
        self.rep_faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        self.keep = torch.empty(F, dtype=torch.uint8, device=dev)
        self.h, self.dims, self.Vn, self.Fn = None, (1, 1, 1), 0, 0


class _Pass:
    """One mesh on the device: the box once, then count-only passes and at last the placement.  states = 2 for the bisection: a pass
    writes into the state that is not the best so far, so the pass that is kept needs no repetition."""

    def __init__(self, verts, faces, states=1):
        self.L = _lib.lib()
        self.verts, self.faces = verts, faces
        self.V, self.F, self.dev = int(verts.shape[0]), int(faces.shape[0]), faces.device
        L, V, F, dev = self.L, self.V, self.F, self.dev
        nbytes = L.dgm_mesh_simplify_scratch_bytes(V, F)
        if nbytes == 0:
            raise ValueError(f"mesh_simplify: a mesh of {V} vertices and {F} faces is over the supported 2^29 faces")
        self.states = [_State(L, V, F, dev, nbytes) for _ in range(states)]
        self.cur = self.best = self.states[0]
        self.counts = torch.empty(2, dtype=torch.int32, device=dev)
        box = torch.empty(6, dtype=torch.float32, device=dev)
        with _lib.device_guard(dev):
            for s in self.states:  # (every state's scratch gets the valid-face and used-vertex marks)
                _lib.check(L.dgm_mesh_simplify_box(V, F, _lib.vp(verts), _lib.vp(faces), _lib.vp(s.scratch), _lib.vp(box), _lib.stream_ptr()))
            self.box = box.cpu().numpy()  # host read-back: 24 bytes
        self.empty = not (self.box[0] <= self.box[3])
        self.count_passes = 0

    def _grid_args(self, s):
        return (float(self.box[0]), float(self.box[1]), float(self.box[2]), *s.dims, float(s.h))

    def count(self, h):
        """(V', F') at cell size h, without placement, into the current state.  One 8-byte read-back."""
        s = self.cur
        s.h = np.float32(h)
        if self.empty:
            return 0, 0
        s.dims = grid_dims(self.box, s.h)
        with _lib.device_guard(self.dev):
            _lib.check(self.L.dgm_mesh_simplify_count(self.V, self.F, _lib.vp(self.verts), _lib.vp(self.faces), *self._grid_args(s), _lib.vp(s.scratch),
                                                      _lib.vp(s.cscratch), _lib.vp(s.rep_faces), _lib.vp(s.keep), _lib.vp(self.counts), _lib.stream_ptr()))
            self.count_passes += 1
            s.Vn, s.Fn = self.counts.tolist()  # host read-back: the sizes
        return s.Vn, s.Fn

    def keep_current(self):
        """The current state becomes the best; the next pass writes into the other one."""
        self.best = self.cur
        if len(self.states) > 1:
            self.cur = self.states[1] if self.cur is self.states[0] else self.states[0]

    def emit(self, regularization):
        """From the best state: verts', faces', vert_index, face_index, vert_map."""
        V, F, dev, L, s = self.V, self.F, self.dev, self.L, self.best
        if self.empty:
            return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.full((V,), -1, dtype=torch.int32, device=dev))
        Vn, Fn = s.Vn, s.Fn
        placed = torch.empty((V, 3), dtype=torch.float32, device=dev)
        verts_out = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
        faces_out = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
        vert_index = torch.empty(Vn, dtype=torch.int32, device=dev)
        face_index = torch.empty(Fn, dtype=torch.int32, device=dev)
        vert_map = torch.empty(V, dtype=torch.int32, device=dev)
        with _lib.device_guard(dev):
            st = _lib.stream_ptr()
            _lib.check(L.dgm_mesh_simplify_place(V, F, _lib.vp(self.verts), _lib.vp(self.faces), _lib.vp(s.rep_faces), *self._grid_args(s),
                                                 float(regularization), _lib.vp(s.scratch), _lib.vp(placed), st))
            _lib.check(L.dgm_mesh_compact_emit(V, F, _lib.vp(placed), _lib.vp(s.rep_faces), _lib.vp(s.cscratch), Vn, Fn, _lib.vp(verts_out),
                                               _lib.vp(faces_out), _lib.vp(vert_index), _lib.vp(face_index), st))
            _lib.check(L.dgm_mesh_simplify_vert_map(V, F, Vn, _lib.vp(vert_index), _lib.vp(s.scratch), _lib.vp(vert_map), st))
        return verts_out, faces_out, vert_index, face_index, vert_map


def _bisect(count_at, target):
    """Bisection over grid in GRID_RANGE with at most MAX_COUNT_PASSES calls of count_at(grid) -> faces: the finest grid tried whose
    face count is <= target, and the grids tried."""
    lo, hi = GRID_RANGE
    best, tried = None, []
    while lo <= hi and len(tried) < MAX_COUNT_PASSES:
        mid = (lo + hi) // 2
        tried.append(mid)
        if count_at(mid) <= target:
            best, lo = mid, mid + 1
        else:
            hi = mid - 1
    return best, tried


def simplify_mesh(verts, faces, *, cell=None, grid=None, target_faces=None, regularization=1e-3, return_index=False, return_info=False):
    """The mesh decimated by quadric vertex clustering (module docstring): (verts', faces'), with return_index also vert_index (V',),
    face_index (F',) and vert_map (V,), all int32, and with return_info at the end a dict {"cell", "dims", "grid" (the grid chosen,
    None with `cell`), "grids_tried", "count_passes", "box"}.  Exactly one of cell (h), grid (cells along the longest box axis) and
    target_faces is given; target_faces bisects grid over [2, 1024] with at most 10 count-only passes and keeps the finest grid tried
    whose face count is <= the target (ValueError when even grid = 2 leaves more).  An empty result has (0, 3) tensors."""
    _choice(cell, grid, target_faces, regularization)
    verts, faces = mesh_args.mesh("mesh_simplify.simplify_mesh", verts, faces)
    p = _Pass(verts, faces, states=2 if target_faces is not None else 1)
    tried = []
    if target_faces is not None:
        def faces_at(g):
            fn = p.count(grid_cell(p.box, g))[1]
            if fn <= int(target_faces):
                p.keep_current()
            return fn

        grid, tried = _bisect(faces_at, int(target_faces))
        if grid is None:
            raise ValueError(f"mesh_simplify: target_faces = {target_faces} is not reached even at grid = {GRID_RANGE[0]} "
                             f"({p.cur.Fn} faces)")
    else:
        p.count(np.float32(cell) if cell is not None else grid_cell(p.box, int(grid)))
    out = p.emit(regularization)
    out = out if return_index else out[:2]
    if return_info:
        out = out + ({"cell": float(p.best.h), "dims": tuple(p.best.dims), "grid": None if grid is None else int(grid),
                      "grids_tried": tried, "count_passes": p.count_passes, "box": p.box.copy()},)
    return out


def apply(simplify, verts, faces, *attributes):
    """simplify (as_spec) applied to a mesh and per-vertex attribute tensors: (verts', faces', *attributes gathered at the
    representatives with vert_index); the inputs themselves when simplify is None."""
    spec = as_spec(simplify)
    if spec is None:
        return (verts, faces) + attributes
    v, f, vi, _, _ = simplify_mesh(verts, faces, cell=spec.cell, grid=spec.grid, target_faces=spec.target_faces,
                                   regularization=spec.regularization, return_index=True)
    vi = vi.long()
    return (v, f) + tuple(None if a is None else a[vi] for a in attributes)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_simplify",
                                 description="Decimate a triangle-mesh PLY by quadric vertex clustering on the GPU.")
    ap.add_argument("input")
    ap.add_argument("output")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--cell", type=float, default=None, help="cell size")
    how.add_argument("--grid", type=int, default=None, help="cells along the longest box axis")
    how.add_argument("--target_faces", type=int, default=None, help="at most this many faces (bisection over --grid)")
    ap.add_argument("--regularization", type=float, default=1e-3)
    return ap


def spec_from_args(args):
    return SimplifySpec(cell=args.cell, grid=args.grid, target_faces=args.target_faces, regularization=args.regularization)


def main(argv=None):
    from .ply_io import read_mesh_ply_on_device, write_mesh_ply
    args = build_parser().parse_args(argv)
    spec = spec_from_args(args)
    verts, faces, colors = read_mesh_ply_on_device(args.input, torch.device("cuda"))
    v, f, vi, _, _, info = simplify_mesh(verts, faces, cell=spec.cell, grid=spec.grid, target_faces=spec.target_faces,
                                         regularization=spec.regularization, return_index=True, return_info=True)
    write_mesh_ply(args.output, v, f, vertex_colors=None if colors is None else colors[vi.long()])
    print(f"mesh_simplify: V {len(verts)} F {len(faces)} -> V {v.shape[0]} F {f.shape[0]}  cell {info['cell']:g} dims {info['dims']}"
          + (f" grid {info['grid']}" if info["grid"] is not None else "") + f"  count passes {info['count_passes']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
