"""Timer of mesh repair (mesh_repair.orient_faces, fill_holes, repair_mesh; informational) on a mesh of the mesh phase's size: DiffMC
of the synthetic two-body field of tools/mesh_clean_bench.py on the 288^3 grid, damaged the way vertex clustering and a clipping
box damage a mesh: a random tenth of its faces flipped and the stars of a few thousand random vertices removed.

    timeout 900 python tools/mesh_repair_bench.py [--res 288] [--blobs 500] [--stars 3000] [--flip 0.1] [--iters 7] [--no-host]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation (every call
reads its counts back, so the wall time is what a caller sees):
  edge table    EdgeTable alone (the count call and its read-back), which every function below builds first;
  orient        orient_faces whole, and dgm_mesh_orient alone on a table built before;
  fill          fill_holes whole on the oriented mesh, and dgm_mesh_fill_count / dgm_mesh_fill_emit alone;
  repair        repair_mesh whole (one edge table for both parts), with the topology report before and after;
  host          the numpy restatement of the tests (tests/_repair_ref.py: Python loops over faces and edges, for orientation about
                what a host-side repair costs, not a tuned library) on the same mesh, and whether its output equals ours byte for
                byte.  It takes minutes at 288^3: --no-host leaves it out, a smaller --res keeps it short.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_clean_bench import _times, two_body_field  # noqa: E402


def damage(verts, faces, stars, flip, seed=0):
    """The faces around `stars` random vertices removed, then a fraction `flip` of the rest flipped."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    V = verts.shape[0]
    centres = torch.randperm(V, generator=g)[:stars].to(faces.device)
    gone = torch.zeros(V, dtype=torch.bool, device=faces.device)
    gone[centres] = True
    faces = faces[~gone[faces.long()].any(dim=1)]
    which = (torch.rand(faces.shape[0], generator=g) < flip).to(faces.device)
    faces = torch.where(which[:, None], faces[:, [0, 2, 1]], faces)
    return faces.contiguous(), int(which.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--stars", type=int, default=3000)
    ap.add_argument("--flip", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    T = importlib.import_module("dg-mesh_amd.mesh_topology")
    M = importlib.import_module("dg-mesh_amd.mesh_repair")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, clean_faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        verts = verts.contiguous()
        faces, n_flipped = damage(verts, clean_faces, args.stars, args.flip)
        V, F = verts.shape[0], faces.shape[0]
        res = dict(res=args.res, V=V, F_clean=int(clean_faces.shape[0]), F=F, stars=args.stars, faces_flipped_by_damage=n_flipped)
        res["before"] = {k: v for k, v in T.topology_report(verts, faces).items() if k != "edge_length"}

        table = T.EdgeTable("mesh_repair_bench", faces, V)
        res["edge_table_ms"], res["edge_table_wall_ms"] = _times(lambda: T.EdgeTable("mesh_repair_bench", faces, V), args.iters)
        L, vp, chk, st = table.L, T._lib.vp, T._lib.check, T._lib.stream_ptr

        oriented, flipped, info = M.orient_faces(verts, faces)
        res["orient_info"] = info
        res["orient_faces_ms"], res["orient_faces_wall_ms"] = _times(lambda: M.orient_faces(verts, faces), args.iters)
        scratch = T._lib.scratch(L.dgm_mesh_orient_scratch_bytes(V, F), dev)
        out, fl, buf = torch.empty_like(faces), torch.empty(F, dtype=torch.uint8, device=dev), torch.empty(8, dtype=torch.int32, device=dev)
        res["orient_alone_ms"], _ = _times(lambda: chk(L.dgm_mesh_orient(V, F, vp(verts), vp(faces), vp(table.scratch), vp(scratch), 1, vp(out),
                                                                           vp(fl), vp(buf), st())), args.iters)

        v2, f2, info = M.fill_holes(verts, oriented)
        res["fill_info"] = info
        res["fill_holes_ms"], res["fill_holes_wall_ms"] = _times(lambda: M.fill_holes(verts, oriented), args.iters)
        otable = T.EdgeTable("mesh_repair_bench", oriented, V)
        B, nv, nf = otable.info["boundary_edges"], info["verts_added"], info["faces_added"]
        fscratch = T._lib.scratch(L.dgm_mesh_fill_scratch_bytes(V, B), dev)
        vo, fo = torch.empty((V + nv, 3), dtype=torch.float32, device=dev), torch.empty((F + nf, 3), dtype=torch.int32, device=dev)
        res["fill_count_alone_ms"], _ = _times(lambda: chk(L.dgm_mesh_fill_count(V, F, B, vp(verts), vp(otable.scratch), None, 1000, vp(fscratch),
                                                                                   vp(buf), st())), args.iters)
        res["fill_emit_alone_ms"], _ = _times(lambda: chk(L.dgm_mesh_fill_emit(V, F, B, vp(verts), vp(oriented), vp(fscratch), nv, nf, vp(vo),
                                                                                 vp(fo), st())), args.iters)
        res["fill_alone_equals_whole"] = bool(torch.equal(vo, v2) and torch.equal(fo, f2))

        rv, rf, info = M.repair_mesh(verts, faces)
        res["repair_info"] = info
        res["repair_equals_orient_then_fill"] = bool(torch.equal(rv, v2) and torch.equal(rf, f2))
        res["repair_mesh_ms"], res["repair_mesh_wall_ms"] = _times(lambda: M.repair_mesh(verts, faces), args.iters)
        res["after"] = {k: v for k, v in T.topology_report(rv, rf).items() if k != "edge_length"}

        if not args.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _repair_ref as R
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hf, hinfo = R.repair(verts.cpu().numpy(), faces.cpu().numpy())
            back = torch.from_numpy(hv).to(dev), torch.from_numpy(hf).to(dev)
            torch.cuda.synchronize()
            res["host_route_wall_ms"] = (time.perf_counter() - t0) * 1e3
            res["host_route_over_repair_mesh"] = res["host_route_wall_ms"] / res["repair_mesh_wall_ms"]
            res["host_equals_ours"] = bool(torch.equal(back[0], rv) and torch.equal(back[1], rf) and hinfo == info)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
