"""Timer of the closest point on a mesh (correspondence.closest_on_mesh, csrc/surface.hip; informational) at the mesh phase's size:
DiffMC of a smooth synthetic field on the 288^3 grid, the queries its own vertices displaced by up to 2 voxels.

    timeout 600 python tools/correspondence_bench.py [--res 288] [--iters 7] [--brute-queries 16384] [--torch-queries 2048]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream:
  * the bounded search at 4 voxels over every vertex, and its stages' share as faces tested per query (counted from the grid the way
    the kernel walks it: the references in the 27 buckets around each query, duplicates included);
  * the unbounded path (tiled brute force) at --brute-queries queries;
  * a chunked PyTorch brute force of the same formula on the same GPU at --torch-queries queries (the route without the kernel), whose
    distances must agree with the kernel's to rounding;
  * interpolate and palette over every vertex.
Algorithmic bytes: what the bounded call must read and write at least once (points, verts, faces, outputs).  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def smooth_field(res, dev):
    """Signed distance (negative inside) to a sphere whose radius undulates: one smooth closed surface of ~3e5 vertices at 288^3."""
    ax = (torch.arange(res, dtype=torch.float32, device=dev) + 0.5) / res * 2 - 1
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    return r - (0.62 + 0.08 * torch.sin(5 * x) * torch.cos(4 * y) + 0.06 * torch.sin(6 * z))


def torch_brute(p, verts, faces, chunk=128):
    """The same region test, dense over the faces, chunked over the queries: (face, d2)."""
    a, b, c = verts[faces[:, 0].long()][None], verts[faces[:, 1].long()][None], verts[faces[:, 2].long()][None]
    dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
    ab, ac = b - a, c - a
    out_f, out_d = [], []
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        ap, bp, cp = q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        zero, one = torch.zeros_like(v), torch.ones_like(v)
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = torch.where(m, 1 - wbc, v), torch.where(m, wbc, w)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = torch.where(m, zero, v), torch.where(m, d2 / (d2 - d6), w)
        m = (d6 >= 0) & (d5 <= d6)
        v, w = torch.where(m, zero, v), torch.where(m, one, w)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = torch.where(m, d1 / (d1 - d3), v), torch.where(m, zero, w)
        m = (d3 >= 0) & (d4 <= d3)
        v, w = torch.where(m, one, v), torch.where(m, zero, w)
        m = (d1 <= 0) & (d2 <= 0)
        v, w = torch.where(m, zero, v), torch.where(m, zero, w)
        e = q - ((a + ab * v[..., None]) + ac * w[..., None])
        dd = dot(e, e)
        dd = torch.where(torch.isnan(dd), torch.full_like(dd, float("inf")), dd)
        d, f = dd.min(1)
        out_f.append(f)
        out_d.append(d)
    return torch.cat(out_f), torch.cat(out_d)


def faces_tested(points, verts, faces, max_dist):
    """Mean number of (query, face) pair tests of the bounded search, from a torch rebuild of its grid: cell edge
    max(1.001 max_dist, 1.001 E), a face in every cell its box overlaps, the 27 cells around a query (hash collisions, which only
    add a few, are not modelled)."""
    a, b, c = verts[faces[:, 0].long()], verts[faces[:, 1].long()], verts[faces[:, 2].long()]
    lo, hi = torch.minimum(torch.minimum(a, b), c).double(), torch.maximum(torch.maximum(a, b), c).double()
    cell = max(1.001 * max_dist, 1.001 * float((hi - lo).max()))
    org = lo.min(0).values
    c0, c1 = torch.floor((lo - org) / cell).long(), torch.floor((hi - org) / cell).long()
    n = int(c1.max()) + 3
    grid = torch.zeros((n, n, n), dtype=torch.float64, device=verts.device)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                ok = (c0[:, 0] + dx <= c1[:, 0]) & (c0[:, 1] + dy <= c1[:, 1]) & (c0[:, 2] + dz <= c1[:, 2])
                idx = (c0[ok] + torch.tensor([dx, dy, dz], device=verts.device) + 1)
                grid.index_put_((idx[:, 0], idx[:, 1], idx[:, 2]), torch.ones(idx.shape[0], dtype=torch.float64, device=verts.device), accumulate=True)
    box = torch.nn.functional.avg_pool3d(grid[None, None], 3, stride=1, padding=1, divisor_override=1)[0, 0]
    q = (torch.floor((points.double() - org) / cell).long() + 1).clamp(0, n - 1)
    return float(box[q[:, 0], q[:, 1], q[:, 2]].mean()), float(grid.sum() / faces.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--brute-queries", type=int, default=16384)
    ap.add_argument("--torch-queries", type=int, default=2048)
    args = ap.parse_args()
    C = importlib.import_module("dg-mesh_amd.correspondence")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, faces = MC.marching_cubes(smooth_field(args.res, dev), isovalue=0.0, normalize=False)
        verts, faces = verts.contiguous(), faces.contiguous()
        V, F = verts.shape[0], faces.shape[0]
        voxel = 1.0  # (un-normalised DiffMC vertices are in voxel units)
        gen = torch.Generator(device=dev).manual_seed(0)
        step = torch.randn((V, 3), generator=gen, device=dev)
        step = step / step.norm(dim=1, keepdim=True) * (2.0 * voxel * torch.rand((V, 1), generator=gen, device=dev))
        points = (verts + step).contiguous()
        max_dist = 4.0 * voxel
        res = dict(res=args.res, V=V, F=F, queries=V, max_dist_voxels=4.0)
        res["scratch_bytes"] = int(importlib.import_module("dg-mesh_amd._lib").lib().dgm_surf_closest_scratch_bytes(V, F))
        res["bounded_ms"] = _median_ms(lambda: C.closest_on_mesh(points, verts, faces, max_dist), args.iters)
        face, d2, bary = C.closest_on_mesh(points, verts, faces, max_dist)
        res["found"] = int((face >= 0).sum())
        res["mean_dist_voxels"] = float(d2[face >= 0].double().sqrt().mean()) / voxel
        res["faces_tested_per_query"], res["refs_per_face"] = faces_tested(points, verts, faces, max_dist)
        res["bounded_pairs_per_s"] = res["faces_tested_per_query"] * V / (res["bounded_ms"] * 1e-3)
        res["algorithmic_bytes"] = V * 12 + V * 12 + F * 12 + V * (4 + 4 + 12)
        res["interpolate_ms"] = _median_ms(lambda: C.interpolate(verts, faces, face, bary), args.iters)
        res["palette_ms"] = _median_ms(lambda: C.palette(points, (0.0, 0.0, 0.0), float(args.res), "checker", 8), args.iters)
        nb = min(args.brute_queries, V)
        pb = points[:nb].contiguous()
        res["brute_queries"] = nb
        res["brute_ms"] = _median_ms(lambda: C.closest_on_mesh(pb, verts, faces), max(3, args.iters // 2))
        res["brute_pairs_per_s"] = nb * F / (res["brute_ms"] * 1e-3)
        fb, db, _ = C.closest_on_mesh(pb, verts, faces)
        res["brute_equals_bounded"] = bool(torch.equal(fb, face[:nb]) and torch.equal(db, d2[:nb]))  # (every query lies within 2 voxels)
        nt = min(args.torch_queries, V)
        pt = points[:nt].contiguous()
        res["torch_queries"] = nt
        res["torch_brute_ms"] = _median_ms(lambda: torch_brute(pt, verts, faces), 3)
        ft, dt = torch_brute(pt, verts, faces)
        res["torch_max_d2_difference"] = float((dt - d2[:nt]).abs().max())
        res["torch_ms_per_query_over_bounded"] = (res["torch_brute_ms"] / nt) / (res["bounded_ms"] / V)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
