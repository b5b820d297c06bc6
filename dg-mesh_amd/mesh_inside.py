"""Inside / outside queries on a triangle mesh on the device: the generalised winding number of query points and what rests on it --
point containment, a signed distance, occupancy voxelisation and the volumetric IoU of two meshes (csrc/mesh_inside.hip:
dgm_wind_number; include/dgmesh_hip.h states the definition and the summation order).  The reference scores
surfaces only (Chamfer distance and EMD, mesh_eval.py); it has nothing to port here.

  winding_number   w (N,): 1 inside a closed mesh wound outwards, 0 outside, -1 inside one wound inwards, a fraction near an open rim
  contains         w >= threshold (|w| with absolute=True)
  signed_distance  sqrt(d2) of correspondence.closest_on_mesh, negative where contains
  occupancy_grid   contains at the cell centres of a res^3 grid
  volume_iou       Monte-Carlo intersection over union of the volumes two meshes enclose, and the two volumes

The winding number is exact for watertight meshes and degrades gracefully on meshes with holes, on simplified meshes and on the
box-clipped rims of real captures, where ray parity fails.  Every value is bit-reproducible and does not depend on which other
queries it is asked with.  Cost: every query visits every face, N x F pairs.

float32 / int32 CUDA/HIP tensors only -- no CPU fallback; anything else raises.

  python -m dgmesh_amd.mesh_inside a.ply b.ply [--points N] [--seed S]
prints one JSON line: the volume IoU of the two mesh PLYs, the counts and the two volumes."""
import argparse
import json
import math

import torch

from . import _lib, mesh_args

SCRATCH_LIMIT = 64 << 20  # bytes of slice sums per launch; more queries are taken in batches (the result does not depend on them)
SLICE_FACES = 16384       # WN_SLICE of csrc/mesh_inside.hip


def batch_rows(F):
    """Queries per launch against F faces: the most whose slice sums stay below SCRATCH_LIMIT, a multiple of 256."""
    slices = max(1, -(-int(F) // SLICE_FACES))
    return max(256, (SCRATCH_LIMIT - 1) // (8 * slices) // 256 * 256)


def winding_number(points, verts, faces):
    """The generalised winding number w (N,) fp32 of points (N, 3) fp32 about the mesh (verts (V, 3) fp32, faces (F, 3) int32), by
    the definition and in the summation order of include/dgmesh_hip.h.  A face with an index outside [0, V), a non-finite corner or
    no volume against the query adds nothing; a query with a non-finite coordinate gets NaN; F = 0 or V = 0 gives 0.  N x F pairs;
    large N is taken in batches, which changes no bit."""
    v, f = mesh_args.mesh("mesh_inside.winding_number", verts, faces, ("points", points))
    p = points.detach().contiguous()
    N, V, F = p.shape[0], v.shape[0], f.shape[0]
    L = _lib.lib()
    w = torch.empty(N, dtype=torch.float32, device=p.device)
    step = batch_rows(F)
    with _lib.device_guard(p.device):
        for at in range(0, N, step):
            n = min(step, N - at)
            scratch = _lib.scratch(L.dgm_wind_scratch_bytes(n, F), p.device)
            _lib.check(L.dgm_wind_number(n, V, F, _lib.vp(p[at:at + n]), _lib.vp(v), _lib.vp(f), _lib.vp(scratch), _lib.vp(w[at:at + n]), _lib.stream_ptr()))
    return w


def _inside(w, threshold, absolute):
    return (w.abs() if absolute else w) >= threshold


def contains(points, verts, faces, threshold=0.5, absolute=False):
    """(N,) bool: winding_number >= threshold; absolute=True tests |w|, for a mesh wound inwards.  A NaN query is outside."""
    return _inside(winding_number(points, verts, faces), float(threshold), absolute)


def signed_distance(points, verts, faces, max_dist=math.inf, absolute=False):
    """(N,) fp32: the distance to the mesh, negative where contains(points, verts, faces, absolute=absolute).  The magnitude is
    sqrt(d2) of correspondence.closest_on_mesh(points, verts, faces, max_dist) -- the same kernel, the same bits --, so a query
    with no face within max_dist gets +inf outside and -inf inside."""
    from .correspondence import closest_on_mesh
    mesh_args.mesh("mesh_inside.signed_distance", verts, faces, ("points", points))
    dist = closest_on_mesh(points, verts, faces, max_dist)[1].sqrt()
    return torch.where(contains(points, verts, faces, absolute=absolute), -dist, dist)


def _box(name, verts, lo, hi):
    dev = verts.device
    if (lo is None) != (hi is None):
        raise ValueError(f"mesh_inside.{name}: give both lo and hi, or neither")
    if lo is None:
        if verts.shape[0] == 0:
            raise ValueError(f"mesh_inside.{name}: a mesh without vertices has no bounding box, give lo and hi")
        return verts.min(dim=0).values, verts.max(dim=0).values
    lo = torch.as_tensor(lo, dtype=torch.float32).to(dev).reshape(-1)
    hi = torch.as_tensor(hi, dtype=torch.float32).to(dev).reshape(-1)
    if lo.numel() != 3 or hi.numel() != 3:
        raise ValueError(f"mesh_inside.{name}: lo and hi must have three components")
    return lo, hi


def grid_centres(lo, hi, res):
    """The (res^3, 3) cell centres lo + (i + 0.5) (hi - lo) / res of the box, the x index slowest: row (i * res + j) * res + k is
    the cell (i, j, k) along (x, y, z)."""
    t = (torch.arange(res, dtype=torch.float32, device=lo.device) + 0.5) / res
    axes = [lo[a] + t * (hi[a] - lo[a]) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def occupancy_grid(verts, faces, res, lo=None, hi=None, absolute=False):
    """(res, res, res) bool, indexed [x, y, z]: contains() at the cell centres (grid_centres) of the box lo .. hi (three numbers or
    device tensors each); the default box is the bounding box of verts.  Cost: res^3 x F pairs -- every cell visits every face; a
    128^3 grid against 261 k faces is 5.5 10^11 pairs, about a second."""
    name = "occupancy_grid"
    v, f = mesh_args.mesh(f"mesh_inside.{name}", verts, faces)
    res = int(res)
    if res < 1:
        raise ValueError(f"mesh_inside.{name}: res must be >= 1, got {res}")
    lo, hi = _box(name, v, lo, hi)
    return contains(grid_centres(lo, hi, res), v, f, absolute=absolute).reshape(res, res, res)


def volume_iou(verts_a, faces_a, verts_b, faces_b, n_points=100000, generator=None, padding=0.0, absolute=True, return_points=False):
    """The volumetric intersection over union of meshes a and b by Monte-Carlo: n_points uniform samples (torch.rand of `generator`,
    a generator of the meshes' device; None: that device's default one) in the bounding box of both meshes' vertices, padded on
    every side by `padding` x its diagonal, each classified by contains(..., absolute=absolute) against either mesh.
    -> a dict of device scalars, nothing is read back: "iou" = n_inter / n_union (fp64; NaN when no sample is inside either),
    "n_a", "n_b", "n_inter", "n_union" (int64), "volume_a", "volume_b" (fp64: box volume x share of the samples); with
    return_points=True also "points" (n_points, 3)."""
    name = "volume_iou"
    va, fa = mesh_args.mesh(f"mesh_inside.{name}", verts_a, faces_a)
    vb, fb = mesh_args.mesh(f"mesh_inside.{name}", verts_b, faces_b)
    if va.device != vb.device:
        raise ValueError(f"mesh_inside.{name}: meshes on {va.device} and {vb.device}")
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError(f"mesh_inside.{name}: n_points must be >= 1, got {n_points}")
    if va.shape[0] + vb.shape[0] == 0:
        raise ValueError(f"mesh_inside.{name}: two meshes without vertices have no bounding box")
    dev = va.device
    both = torch.cat((va, vb))
    lo, hi = both.min(dim=0).values, both.max(dim=0).values
    pad = float(padding) * (hi - lo).norm()
    lo, hi = lo - pad, hi + pad
    points = (lo + torch.rand((n_points, 3), generator=generator, device=dev, dtype=torch.float32) * (hi - lo)).contiguous()
    in_a, in_b = contains(points, va, fa, absolute=absolute), contains(points, vb, fb, absolute=absolute)
    n_a, n_b, n_inter, n_union = in_a.sum(), in_b.sum(), (in_a & in_b).sum(), (in_a | in_b).sum()
    box = (hi - lo).double().prod()
    out = {"iou": n_inter.double() / n_union.double(), "n_a": n_a, "n_b": n_b, "n_inter": n_inter, "n_union": n_union,
           "volume_a": box * n_a.double() / n_points, "volume_b": box * n_b.double() / n_points}
    if return_points:
        out["points"] = points
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_inside",
                                 description="Print the volumetric IoU of two triangle-mesh PLY files as one JSON line.")
    ap.add_argument("mesh_a", help="triangle-mesh PLY file (ply_io's format)")
    ap.add_argument("mesh_b", help="triangle-mesh PLY file")
    ap.add_argument("--points", type=int, default=100000, metavar="N", help="uniform samples in the union bounding box")
    ap.add_argument("--seed", type=int, default=0, metavar="S", help="seed of the sampling generator")
    return ap


def main(argv=None):
    from .ply_io import read_mesh_ply
    args = build_parser().parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    meshes = []
    for path in (args.mesh_a, args.mesh_b):
        verts, faces = read_mesh_ply(path)[:2]
        meshes += [torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)]
    out = volume_iou(*meshes, n_points=args.points, generator=torch.Generator(device=dev).manual_seed(args.seed))
    keys = ("iou", "n_a", "n_b", "n_inter", "n_union", "volume_a", "volume_b")
    values = torch.stack([out[k].double() for k in keys]).tolist()  # the one read-back
    print(json.dumps({"mesh_a": args.mesh_a, "mesh_b": args.mesh_b, "points": args.points, "seed": args.seed,
                      **{k: (v if k in ("iou", "volume_a", "volume_b") else int(v)) for k, v in zip(keys, values)}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
