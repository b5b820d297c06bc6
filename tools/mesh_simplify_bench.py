"""Timer of mesh simplification (mesh_simplify.simplify_mesh; informational) on a mesh of the mesh phase's size: DiffMC of the
synthetic two-body field of tools/mesh_clean_bench.py on the 288^3 grid.

    timeout 600 python tools/mesh_simplify_bench.py [--res 288] [--blobs 500] [--grid 64] [--iters 7] [--no-host]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation
(simplify_mesh reads the box and the sizes back, so the wall time is what a caller sees): the whole simplify_mesh(grid=G), and the C
entry points alone -- box (valid faces, used vertices, box), count (cell keys and cluster map, face remap with null and duplicate
flags, compaction count), place (instance index, quadric sums and solve), emit (compaction emit and vert_map).  A kernel trace splits
the entry points further.  For orientation the same mesh goes through tests/_simplify_ref.py on the host -- mesh to the host, numpy,
mesh back to the device -- timed with a wall clock; its integer outputs must equal the device's and the positions agree within 2 ulp
of the box's largest coordinate.  Also the lengths of the clusters' face lists: mean and max.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_clean_bench import _times, two_body_field  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    M = importlib.import_module("dg-mesh_amd.mesh_simplify")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        verts, faces = verts.contiguous(), faces.contiguous()
        V, F = verts.shape[0], faces.shape[0]
        res = dict(res=args.res, V=V, F=F, grid=args.grid)
        run = lambda: M.simplify_mesh(verts, faces, grid=args.grid, return_index=True, return_info=True)
        v1, f1, vi, fi, vm, info = run()
        res.update(V_out=v1.shape[0], F_out=f1.shape[0], cell=info["cell"], dims=list(info["dims"]))
        res["simplify_mesh_ms"], res["simplify_mesh_wall_ms"] = _times(run, args.iters)
        res["target_faces_20000_ms"], res["target_faces_20000_wall_ms"] = _times(
            lambda: M.simplify_mesh(verts, faces, target_faces=20000), args.iters)
        # the entry points alone, on one state
        p = M._Pass(verts, faces)
        h = M.grid_cell(p.box, args.grid)
        s, L, st = p.best, p.L, M._lib.stream_ptr
        box = torch.empty(6, dtype=torch.float32, device=dev)
        vp, chk = M._lib.vp, M._lib.check
        p.count(h)
        g = p._grid_args(s)
        placed = torch.empty((V, 3), dtype=torch.float32, device=dev)
        vo, fo = torch.empty((s.Vn, 3), dtype=torch.float32, device=dev), torch.empty((s.Fn, 3), dtype=torch.int32, device=dev)
        vio, fio = torch.empty(s.Vn, dtype=torch.int32, device=dev), torch.empty(s.Fn, dtype=torch.int32, device=dev)
        vmo = torch.empty(V, dtype=torch.int32, device=dev)
        stages = {
            "box": lambda: chk(L.dgm_mesh_simplify_box(V, F, vp(verts), vp(faces), vp(s.scratch), vp(box), st())),
            "count": lambda: chk(L.dgm_mesh_simplify_count(V, F, vp(verts), vp(faces), *g, vp(s.scratch), vp(s.cscratch), vp(s.rep_faces),
                                                           vp(s.keep), vp(p.counts), st())),
            "place": lambda: chk(L.dgm_mesh_simplify_place(V, F, vp(verts), vp(faces), vp(s.rep_faces), *g, 1e-3, vp(s.scratch), vp(placed),
                                                           st())),
            "emit": lambda: (chk(L.dgm_mesh_compact_emit(V, F, vp(placed), vp(s.rep_faces), vp(s.cscratch), s.Vn, s.Fn, vp(vo), vp(fo),
                                                         vp(vio), vp(fio), st())),
                             chk(L.dgm_mesh_simplify_vert_map(V, F, s.Vn, vp(vio), vp(s.scratch), vp(vmo), st()))),
        }
        for name, fn in stages.items():
            res[f"{name}_ms"], _ = _times(fn, args.iters)
        res["stages_equal_whole"] = bool(torch.equal(vo, v1) and torch.equal(fo, f1) and torch.equal(vmo, vm))
        if not args.no_host:
            import _simplify_ref as R
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = R.simplify(verts.cpu().numpy(), faces.cpu().numpy(), grid=args.grid)
            hv, hf = torch.from_numpy(ref["verts"]).to(dev), torch.from_numpy(ref["faces"]).to(dev)
            torch.cuda.synchronize()
            res["host_route_wall_ms"] = (time.perf_counter() - t0) * 1e3
            res["host_route_over_simplify_mesh"] = res["host_route_wall_ms"] / res["simplify_mesh_wall_ms"]
            res["integers_equal_host"] = bool(torch.equal(hf, f1) and np.array_equal(ref["vert_index"], vi.cpu().numpy())
                                              and np.array_equal(ref["face_index"], fi.cpu().numpy())
                                              and np.array_equal(ref["vert_map"], vm.cpu().numpy()))
            ulp = float(np.spacing(np.float32(np.abs(info["box"]).max())))
            res["verts_max_ulp_vs_host"] = float((hv.double() - v1.double()).abs().max()) / ulp if len(ref["verts"]) else 0.0
            res["list_len_mean"], res["list_len_max"] = float(ref["lists"].mean()), int(ref["lists"].max())
            res["list_len_median"] = float(np.median(ref["lists"]))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
