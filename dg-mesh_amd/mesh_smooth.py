"""Smoothing an extracted mesh on the device: Taubin's lambda | mu scheme ("A signal processing approach to fair surface design",
SIGGRAPH 1995) and plain Laplacian smoothing with uniform weights, on the sorted adjacency of mesh_topology, as the smoothing kernel
of csrc/mesh_edges.hip.  A mesh extracted from a grid carries grid-aligned staircase noise; vertex
clustering (mesh_simplify) keeps it.  Taubin's two steps per iteration -- lambda > 0 shrinks, mu < -lambda inflates -- remove the
high frequencies without the shrinkage of the Laplacian alone.  trimesh, Open3D and pymeshlab are neither vendored nor dependencies.

Definitions (this project's; include/dgmesh_hip.h states them for the C ABI, tests/_edges_ref.py restates them in numpy):
  * one step with factor f, for vertex i with neighbour set N (the distinct vertices that share a valid face's side with i):
    m = (the sum of the neighbours in fp64, from 0, in ascending neighbour order) / (double)|N|; out = (float)(x + f (m - x)) with
    x = (double)in[i]: one rounding to fp32 per step and coordinate;
  * a vertex with an empty N (no valid face uses it) and a vertex with a non-finite coordinate are copied unchanged.  A non-finite
    NEIGHBOUR is not left out of the sum: the vertices next to a NaN vertex become NaN in the first step (IEEE arithmetic) and are
    then copied themselves, so a NaN spreads by one ring of neighbours per step -- clean such a mesh first;
  * boundary "fixed": a vertex on a boundary edge (mesh_topology's vert_flag bit 1) is copied unchanged; "curve": for such a vertex N
    is restricted to the neighbours it is joined to by a boundary edge, so a rim is smoothed along itself; "free": no distinction;
  * method "taubin": per iteration a step with f = lam and a step with f = mu; "laplacian": a step with f = lam.
Faces are untouched, so per-vertex attributes need no remapping.  Every output is identical bit for bit from run to run and equal to
the numpy restatement.  fp32 vertices, int32 faces, CUDA/HIP tensors only -- no CPU fallback.  One 32-byte read-back per call (the
sizes of the edge table).

Command line: python -m dgmesh_amd.mesh_smooth in.ply out.ply [--iterations N] [--lam L] [--mu M] [--method taubin|laplacian]
[--boundary fixed|curve|free] reads and writes ply_io's triangle-mesh PLY and keeps vertex colours."""
import argparse
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, mesh_args

METHODS = ("taubin", "laplacian")
BOUNDARIES = ("fixed", "curve", "free")  # the int of the C ABI is the index


@dataclass(frozen=True)
class SmoothSpec:
    """The parameters of smooth_mesh."""
    iterations: int = 10
    lam: float = 0.5
    mu: float = -0.53
    method: str = "taubin"
    boundary: str = "fixed"

    def describe(self):
        return f"iterations {int(self.iterations)} lam {float(self.lam):g} mu {float(self.mu):g} method {self.method} boundary {self.boundary}"


def as_spec(smooth):
    """None, a SmoothSpec or a dict of its fields -> SmoothSpec or None ("do nothing")."""
    return mesh_args.spec_of("mesh_smooth", "smooth", SmoothSpec, smooth)


def _choice(iterations, lam, mu, method, boundary):
    if method not in METHODS:
        raise ValueError(f"mesh_smooth: method must be one of {', '.join(METHODS)}, got {method!r}")
    if boundary not in BOUNDARIES:
        raise ValueError(f"mesh_smooth: boundary must be one of {', '.join(BOUNDARIES)}, got {boundary!r}")
    if int(iterations) != iterations or int(iterations) < 0:
        raise ValueError(f"mesh_smooth: iterations must be an integer >= 0, got {iterations}")
    if not 0.0 < float(lam) <= 1.0:
        raise ValueError(f"mesh_smooth: lam must be in (0, 1], got {lam}")
    if method == "taubin" and not (float(mu) < -float(lam) and np.isfinite(float(mu))):
        raise ValueError(f"mesh_smooth: Taubin smoothing needs a finite mu < -lam = {-float(lam):g}, got mu = {mu}")


def step_factors(iterations, lam, mu, method):
    """The factor of every step, in order."""
    return [float(lam), float(mu)] * int(iterations) if method == "taubin" else [float(lam)] * int(iterations)


def smooth_mesh(verts, faces, *, iterations=10, lam=0.5, mu=-0.53, method="taubin", boundary="fixed"):
    """New vertices (V, 3) after `iterations` iterations of `method` (module docstring); the inputs are not modified and faces stay
    as they are.  iterations = 0 returns `verts` itself.  ValueError names iterations < 0, lam outside (0, 1] and, for Taubin,
    mu >= -lam."""
    _choice(iterations, lam, mu, method, boundary)
    given = verts
    verts, faces = mesh_args.mesh("mesh_smooth.smooth_mesh", verts, faces)
    factors = step_factors(iterations, lam, mu, method)
    V = int(verts.shape[0])
    if not factors or V == 0:
        return given
    from .mesh_topology import EdgeTable
    table = EdgeTable("smooth_mesh", faces, V)
    t = table.emit(edges=False, adjacency=True, kind=boundary == "curve")
    L, dev, A = table.L, table.dev, 2 * table.E
    src, dst = verts, torch.empty_like(verts)
    spare = torch.empty_like(verts) if len(factors) > 1 else None  # (the input is never written: the steps alternate between two others)
    with _lib.device_guard(dev):
        st = _lib.stream_ptr()
        for f in factors:
            _lib.check(L.dgm_mesh_smooth_step(V, A, _lib.vp(src), _lib.vp(table.adj_offset), _lib.vp(t["adj"]), _lib.vp(t["adj_kind"]), _lib.vp(table.vert_flag),
                                              f, BOUNDARIES.index(boundary), _lib.vp(dst), st))
            src, dst = dst, (spare if src is verts else src)
    return src


def apply(smooth, verts, faces, *attributes):
    """smooth (as_spec) applied to a mesh: (verts', faces, *attributes) -- smoothing moves vertices only, so faces and per-vertex
    attributes pass through; the inputs themselves when smooth is None."""
    spec = as_spec(smooth)
    if spec is None:
        return (verts, faces) + attributes
    v = smooth_mesh(verts, faces, iterations=spec.iterations, lam=spec.lam, mu=spec.mu, method=spec.method, boundary=spec.boundary)
    return (v, faces) + attributes


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_smooth",
                                 description="Smooth a triangle-mesh PLY on the GPU (Taubin lambda | mu or plain Laplacian).")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--method", choices=METHODS, default="taubin")
    ap.add_argument("--boundary", choices=BOUNDARIES, default="fixed")
    return ap


def spec_from_args(args):
    return SmoothSpec(iterations=args.iterations, lam=args.lam, mu=args.mu, method=args.method, boundary=args.boundary)


def main(argv=None):
    from .ply_io import read_mesh_ply_on_device, write_mesh_ply
    args = build_parser().parse_args(argv)
    spec = spec_from_args(args)
    _choice(spec.iterations, spec.lam, spec.mu, spec.method, spec.boundary)
    verts, faces, colors = read_mesh_ply_on_device(args.input, torch.device("cuda"))
    write_mesh_ply(args.output, apply(spec, verts, faces)[0], faces, vertex_colors=colors)
    print(f"mesh_smooth: V {len(verts)} F {len(faces)}  {spec.describe()}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
