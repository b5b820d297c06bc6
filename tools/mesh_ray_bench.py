"""Timer of ray casting against a mesh (mesh_ray.RayMesh, ray_cast, occluded, mesh_texture.bake_ambient_occlusion; informational) on a
mesh of the mesh phase's size: DiffMC of the synthetic two-body field of tools/mesh_clean_bench.py on the 288^3 grid, scaled into
[-1, 1]^3.

    timeout 900 python tools/mesh_ray_bench.py [--res 288] [--blobs 500] [--side 800] [--grid 128] [--size 2048] [--samples 64]
                                               [--torch-rays 4096] [--iters 7] [--sweep 8,12,16,32,64,128]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream (and wall time with a synchronisation):
  build            RayMesh(verts, faces): the sort by Morton code and the chunk boxes;
  cast_accel       the side x side pixel-centre rays of synthetic.make_camera against the structure;
  cast_brute       the same rays by brute force, with the pairs (rays x faces) per second; the two answers are compared bit for bit;
  occluded_*       the same rays, any hit;
  sweep            the same camera against the mesh decimated by mesh_simplify at every grid of --sweep: brute force against build +
                   accelerated cast, which is what accel="auto" pays for one cast -- mesh_ray.AUTO_MIN_FACES follows from it;
  ao               bake_ambient_occlusion with `samples` rays per owned texel of the atlas of side `size` of the mesh decimated at
                   `grid` (the workload of tools/mesh_texture_bench.py), once after a warm-up of 1/16 of the samples;
  torch            Moeller-Trumbore by PyTorch broadcasting on the same GPU, `torch-rays` of the camera rays in chunks of 32 against
                   all faces (every intermediate is a 32 x F x 3 fp32 tensor); its pairs per second and its agreement on the face.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_clean_bench import _times, two_body_field  # noqa: E402

TORCH_CHUNK = 32


def torch_cast(origins, dirs, verts, faces):
    """The nearest hit by Moeller and Trumbore's test, broadcast: (face, t); valid finite faces assumed, no tie rule, no watertightness."""
    tri = verts[faces.long()]
    v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    face, best = [], []
    for at in range(0, origins.shape[0], TORCH_CHUNK):
        o, d = origins[at:at + TORCH_CHUNK, None, :], dirs[at:at + TORCH_CHUNK, None, :]
        p = torch.linalg.cross(d.expand(-1, e2.shape[1], -1), e2.expand(o.shape[0], -1, -1))
        det = (e1 * p).sum(-1)
        inv = 1.0 / det
        s = o - v0
        u = (s * p).sum(-1) * inv
        q = torch.linalg.cross(s, e1.expand(o.shape[0], -1, -1))
        v = (d * q).sum(-1) * inv
        t = (e2 * q).sum(-1) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
        t = torch.where(ok, t, torch.full_like(t, float("inf")))
        tb, fb = t.min(dim=1)
        face.append(torch.where(torch.isfinite(tb), fb, torch.full_like(fb, -1)))
        best.append(tb)
    return torch.cat(face), torch.cat(best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--torch-rays", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--sweep", default="8,12,16,32,64,128")
    args = ap.parse_args()
    pk = lambda name: importlib.import_module("dg-mesh_amd." + name)
    M, MT, MC, MS, SC, syn = (pk(n) for n in ("mesh_ray", "mesh_texture", "marching_cubes", "mesh_simplify", "scene", "synthetic"))
    dev = torch.device("cuda:0")
    with torch.no_grad():
        full_v, full_f = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        lo, hi = full_v.min(0).values, full_v.max(0).values
        scale = lambda v: ((v - (lo + hi) / 2) / (hi - lo).max() * 2.0).contiguous()  # into [-1, 1]^3: what the camera sees
        verts, faces = scale(full_v), full_f.contiguous()
        F = int(faces.shape[0])
        cam = SC.TorchCamera(syn.make_camera(args.side, args.side), dev)
        o, d = M.camera_rays(cam)
        N = int(o.shape[0])
        res = dict(res=args.res, V=int(verts.shape[0]), F=F, rays=N, pairs=N * F, auto_min_faces=M.AUTO_MIN_FACES)

        def measure(v, f, out, iters):
            """build, accelerated and brute-force cast and occluded of the camera rays against (v, f) into out."""
            out["build_ms"], out["build_wall_ms"] = _times(lambda: M.RayMesh(v, f), iters)
            mesh = M.RayMesh(v, f)
            a = M.ray_cast(o, d, v, f, accel=mesh)
            b = M.ray_cast(o, d, v, f, accel=None)
            out["accel_equals_brute"] = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(a, b))
            out["hit_share"] = float((a[0] >= 0).float().mean())
            out["cast_accel_ms"], out["cast_accel_wall_ms"] = _times(lambda: M.ray_cast(o, d, v, f, accel=mesh), iters)
            out["cast_brute_ms"], out["cast_brute_wall_ms"] = _times(lambda: M.ray_cast(o, d, v, f, accel=None), iters)
            out["brute_pairs_per_s"] = N * int(f.shape[0]) / (out["cast_brute_ms"] * 1e-3)
            out["occluded_accel_ms"], _ = _times(lambda: M.occluded(o, d, v, f, accel=mesh), iters)
            out["occluded_brute_ms"], _ = _times(lambda: M.occluded(o, d, v, f, accel=None), iters)
            out["brute_over_build_plus_accel"] = out["cast_brute_ms"] / (out["build_ms"] + out["cast_accel_ms"])
            return mesh, a

        mesh, answer = measure(verts, faces, res, args.iters)
        res["accel_bytes"] = int(mesh.accel.numel())

        sweep = []
        for grid in (int(g) for g in args.sweep.split(",") if g):
            sv, sf = MS.simplify_mesh(full_v.contiguous(), full_f.contiguous(), grid=grid)
            row = dict(grid=grid, F=int(sf.shape[0]))
            measure(scale(sv), sf.contiguous(), row, max(3, args.iters // 2))
            sweep.append({k: (round(x, 4) if isinstance(x, float) else x) for k, x in row.items()})
            if grid == args.grid:
                ao_v, ao_f = scale(sv), sf.contiguous()
        res["sweep"] = sweep
        if args.grid not in [r["grid"] for r in sweep]:
            sv, sf = MS.simplify_mesh(full_v.contiguous(), full_f.contiguous(), grid=args.grid)
            ao_v, ao_f = scale(sv), sf.contiguous()

        MT.bake_ambient_occlusion(ao_v, ao_f, size=args.size, samples=max(1, args.samples // 16))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ao = MT.bake_ambient_occlusion(ao_v, ao_f, size=args.size, samples=args.samples)[0]
        torch.cuda.synchronize()
        ao_wall_ms = (time.perf_counter() - t0) * 1e3
        owned = int((MT.atlas_interpolate(MT.build_atlas(int(ao_f.shape[0]), size=args.size), ao_v, ao_f)[1] >= 0).sum())
        res.update(ao_F=int(ao_f.shape[0]), ao_texels=owned, ao_rays=owned * args.samples, ao_wall_ms=ao_wall_ms,
                   ao_mean=float(ao.mean()), ao_min=float(ao.min()))
        res["ao_rays_per_s"] = res["ao_rays"] / (res["ao_wall_ms"] * 1e-3)

        tq = min(args.torch_rays, N)
        pick = torch.linspace(0, N - 1, tq, device=dev).long()  # spread over the image
        to, td = o[pick].contiguous(), d[pick].contiguous()
        by_torch = lambda: torch_cast(to, td, verts, faces)
        tf, tt = by_torch()
        mine_f, mine_t = answer[0][pick].long(), answer[1][pick]
        both = (tf >= 0) & (mine_f >= 0)
        res["torch_rays"] = tq
        res["torch_same_face_share"] = float((tf == mine_f).float().mean())
        res["torch_max_abs_t_diff"] = float((tt[both] - mine_t[both]).abs().max()) if bool(both.any()) else 0.0
        res["torch_ms"], res["torch_wall_ms"] = _times(by_torch, max(3, args.iters // 2))
        res["torch_pairs_per_s"] = tq * F / (res["torch_ms"] * 1e-3)
        res["cast_brute_same_rays_ms"], _ = _times(lambda: M.ray_cast(to, td, verts, faces, accel=None), args.iters)
        res["cast_accel_same_rays_ms"], _ = _times(lambda: M.ray_cast(to, td, verts, faces, accel=mesh), args.iters)
        res["torch_over_brute"] = res["torch_ms"] / res["cast_brute_same_rays_ms"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) and 1e-2 < abs(v) < 1e6 else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
