"""Timer of the inside / outside queries (mesh_inside.winding_number, signed_distance, volume_iou; informational) on a mesh of the
mesh phase's size: DiffMC of the synthetic two-body field of tools/mesh_clean_bench.py on the 288^3 grid.

    timeout 600 python tools/mesh_inside_bench.py [--res 288] [--blobs 500] [--queries 100000] [--torch-queries 8192] [--iters 7]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation:
  winding_number   `queries` points uniform in the mesh's bounding box scaled by 1.1, with the pairs (queries x faces) per second;
                   the kernel launches alone through the C entry point on a scratch allocated before;
  signed_distance  the same points: closest_on_mesh (brute force, max_dist = inf) + winding_number; and with max_dist = 4 voxels;
  volume_iou       the mesh against itself moved by 5 voxels along x, `queries` samples: two winding numbers and the counts;
  torch            the same formula as PyTorch broadcasting on the same GPU, `torch-queries` points in chunks of 256 queries against
                   all faces (every intermediate is a 256 x F fp32 matrix), summed with .sum() in fp32; its pairs per second.
The torch sum does not add in the library's order: its largest difference from winding_number is reported, not asserted.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_clean_bench import _times, two_body_field  # noqa: E402

TORCH_CHUNK = 256


def torch_winding(points, verts, faces):
    """(1 / 4 pi) sum of 2 atan2(det, den) by broadcasting, TORCH_CHUNK queries at a time; valid finite faces assumed."""
    tri = verts[faces.long()]  # (F, 3, 3)
    out = []
    dot = lambda x, y: (x * y).sum(-1)
    for at in range(0, points.shape[0], TORCH_CHUNK):
        p = points[at:at + TORCH_CHUNK, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        det = dot(a, torch.linalg.cross(b, c))
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        omega = 2 * torch.atan2(det, den)
        out.append(torch.where(det != 0, omega, torch.zeros_like(omega)).sum(1) / (4 * torch.pi))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--torch-queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    M = importlib.import_module("dg-mesh_amd.mesh_inside")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    lib = importlib.import_module("dg-mesh_amd._lib")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        verts, faces = verts.contiguous(), faces.contiguous()
        V, F, N = verts.shape[0], faces.shape[0], args.queries
        res = dict(res=args.res, V=V, F=F, queries=N, pairs=N * F)
        lo, hi = verts.min(0).values, verts.max(0).values
        centre, half = (lo + hi) / 2, (hi - lo) / 2 * 1.1
        gen = torch.Generator(device=dev).manual_seed(0)
        points = (centre - half + torch.rand((N, 3), generator=gen, device=dev) * 2 * half).contiguous()
        voxel = 1.0  # (normalize=False: the mesh is in voxel units)

        w = M.winding_number(points, verts, faces)
        res["inside_share"] = float((w >= 0.5).float().mean())
        res["w_min"], res["w_max"] = float(w.min()), float(w.max())
        res["winding_ms"], res["winding_wall_ms"] = _times(lambda: M.winding_number(points, verts, faces), args.iters)
        res["winding_pairs_per_s"] = N * F / (res["winding_ms"] * 1e-3)
        L = lib.lib()
        scratch = torch.empty(int(L.dgm_wind_scratch_bytes(N, F)), dtype=torch.uint8, device=dev)
        out = torch.empty(N, dtype=torch.float32, device=dev)
        vp = M._lib.vp
        raw = lambda: lib.check(L.dgm_wind_number(N, V, F, vp(points), vp(verts), vp(faces), vp(scratch), vp(out), lib.stream_ptr()))
        res["dgm_wind_number_ms"], _ = _times(raw, args.iters)
        res["raw_equals_wrapper"] = bool(torch.equal(out, w))
        res["scratch_bytes"] = scratch.numel()

        res["signed_distance_ms"], res["signed_distance_wall_ms"] = _times(lambda: M.signed_distance(points, verts, faces), args.iters)
        near = lambda: M.signed_distance(points, verts, faces, max_dist=4 * voxel)
        res["signed_distance_4_voxels_ms"], _ = _times(near, args.iters)
        res["signed_distance_4_voxels_found"] = float(torch.isfinite(near()).float().mean())

        moved = (verts + torch.tensor([5 * voxel, 0.0, 0.0], device=dev)).contiguous()
        iou = lambda: M.volume_iou(verts, faces, moved, faces, n_points=N, generator=gen)
        res["volume_iou"] = float(iou()["iou"])
        res["volume_iou_ms"], res["volume_iou_wall_ms"] = _times(iou, args.iters)

        tq = min(args.torch_queries, N)
        by_torch = lambda: torch_winding(points[:tq], verts, faces)
        res["torch_queries"] = tq
        res["torch_max_abs_diff"] = float((by_torch() - w[:tq]).abs().max())
        res["torch_ms"], res["torch_wall_ms"] = _times(by_torch, args.iters)
        res["torch_pairs_per_s"] = tq * F / (res["torch_ms"] * 1e-3)
        res["winding_same_queries_ms"], _ = _times(lambda: M.winding_number(points[:tq].contiguous(), verts, faces), args.iters)
        res["torch_over_winding"] = res["torch_ms"] / res["winding_same_queries_ms"] if res["winding_same_queries_ms"] > 0 else None
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) and 1e-2 < abs(v) < 1e6 else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
