"""Timer of the edge table and of mesh smoothing (mesh_topology.EdgeTable, mesh_smooth.smooth_mesh; informational) on a mesh of the
mesh phase's size: DiffMC of the synthetic two-body field of tools/mesh_clean_bench.py on the 288^3 grid.

    timeout 600 python tools/mesh_smooth_bench.py [--res 288] [--blobs 500] [--iterations 10] [--iters 7] [--no-host]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation (the edge
table reads its sizes back, so the wall time is what a caller sees):
  edge table    EdgeTable + emit of every table, and the two C entry points alone (count: lists, ranking, degrees, scans; emit);
  smoothing     smooth_mesh(iterations Taubin iterations, boundary "fixed") whole -- edge table included -- and its 2 x iterations
                steps alone on a table built before, with the bytes a step moves (computed from V and E: every vertex reads its row,
                its two offsets and its flag and writes its row, 4 bytes per adjacency entry and a 12-byte row gathered per entry) and
                the rate that is of the steps' time;
  torch         the same steps as PyTorch ops on the same GPU from the same edges: two index_add_ into an fp64 (V, 3) sum, a divide
                by the degree, the update and a where() for the rim and the unused vertices;
  host          mesh to the host, numpy (np.unique for the edges, a sorted neighbour table, np.add.reduceat per step), vertices back.
The torch and numpy sums do not add in ascending neighbour order: their largest differences from smooth_mesh are reported, not
asserted.  Prints one JSON line."""
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


def step_bytes(V, E):
    """What one smoothing step reads and writes, before any cache: (everything, the gathered neighbour rows alone)."""
    gather = 12 * 2 * E
    return 12 * V + 4 * V + V + 4 * 2 * E + gather + 12 * V, gather


def torch_steps(verts, edges, vert_flag, factors):
    e0, e1 = edges[:, 0].long(), edges[:, 1].long()
    V = verts.shape[0]
    deg = torch.zeros(V, dtype=torch.float64, device=verts.device)
    one = torch.ones(e0.shape[0], dtype=torch.float64, device=verts.device)
    deg.index_add_(0, e0, one).index_add_(0, e1, one)
    move = ((deg > 0) & ((vert_flag & 2) == 0))[:, None]
    deg = deg.clamp(min=1.0)[:, None]
    x = verts
    for f in factors:
        xd = x.double()
        s = torch.zeros_like(xd).index_add_(0, e0, xd[e1]).index_add_(0, e1, xd[e0])
        x = torch.where(move, (xd + f * (s / deg - xd)).float(), x)
    return x


def numpy_route(verts, faces, factors):
    """numpy on the host, valid faces assumed (a marching-cubes mesh)."""
    f = faces.astype(np.int64)
    half = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    edges, mult = np.unique(half, axis=0, return_counts=True)
    V = len(verts)
    own = np.concatenate([edges[:, 0], edges[:, 1]])
    nbr = np.concatenate([edges[:, 1], edges[:, 0]])
    order = np.lexsort((nbr, own))
    own, nbr = own[order], nbr[order]
    deg = np.bincount(own, minlength=V)
    off = np.concatenate([[0], np.cumsum(deg)])
    rim = np.zeros(V, bool)
    rim[edges[mult == 1].reshape(-1)] = True
    move = (deg > 0) & ~rim
    start = np.minimum(off[:-1], max(len(nbr) - 1, 0))
    x = verts
    for fac in factors:
        xd = x.astype(np.float64)
        m = np.add.reduceat(xd[nbr], start, axis=0) / np.maximum(deg, 1)[:, None]
        x = np.where(move[:, None], (xd + fac * (m - xd)).astype(np.float32), x)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    T = importlib.import_module("dg-mesh_amd.mesh_topology")
    S = importlib.import_module("dg-mesh_amd.mesh_smooth")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        verts, faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        verts, faces = verts.contiguous(), faces.contiguous()
        V, F = verts.shape[0], faces.shape[0]
        res = dict(res=args.res, V=V, F=F, iterations=args.iterations)
        factors = S.step_factors(args.iterations, 0.5, -0.53, "taubin")

        def whole_table():
            table = T.EdgeTable("mesh_edges", faces, V)
            return table, table.emit(edges=True, faces=True, adjacency=True, kind=True)

        table, t = whole_table()
        E = table.E
        res.update(E=E, info=table.info)
        res["edge_table_ms"], res["edge_table_wall_ms"] = _times(whole_table, args.iters)
        L, vp, chk, st = table.L, T._lib.vp, T._lib.check, T._lib.stream_ptr
        info = torch.empty(8, dtype=torch.int32, device=dev)
        res["count_ms"], _ = _times(lambda: chk(L.dgm_mesh_edges_count(V, F, vp(faces), vp(table.scratch), vp(table.adj_offset),
                                                                         vp(table.vert_flag), vp(info), st())), args.iters)
        res["emit_ms"], _ = _times(lambda: chk(L.dgm_mesh_edges_emit(V, F, vp(table.scratch), E, vp(table.adj_offset), vp(t["adj"]),
                                                                       vp(t["adj_kind"]), vp(t["edges"]), vp(t["edge_faces"]),
                                                                       vp(t["edge_count"]), st())), args.iters)
        run = lambda: S.smooth_mesh(verts, faces, iterations=args.iterations)
        ours = run()
        res["smooth_mesh_ms"], res["smooth_mesh_wall_ms"] = _times(run, args.iters)
        a, b = torch.empty_like(verts), torch.empty_like(verts)

        def steps():
            src, dst = verts, a
            for f in factors:
                chk(L.dgm_mesh_smooth_step(V, 2 * E, vp(src), vp(table.adj_offset), vp(t["adj"]), vp(t["adj_kind"]), vp(table.vert_flag), f, 0,
                                           vp(dst), st()))
                src, dst = dst, (b if dst is a else a)
            return src

        res["steps_equal_whole"] = bool(torch.equal(steps(), ours))
        res["steps_ms"], _ = _times(steps, args.iters)
        res["step_ms"] = res["steps_ms"] / max(len(factors), 1)
        res["step_bytes"], res["step_gather_bytes"] = step_bytes(V, E)
        res["step_gb_per_s"] = res["step_bytes"] / (res["step_ms"] * 1e-3) / 1e9 if res["step_ms"] > 0 else None
        res["moved_max"] = float((ours - verts).abs().max())
        by_torch = lambda: torch_steps(verts, t["edges"], table.vert_flag, factors)
        res["torch_max_abs_diff"] = float((by_torch() - ours).abs().max())
        res["torch_steps_ms"], res["torch_steps_wall_ms"] = _times(by_torch, args.iters)
        res["torch_over_steps"] = res["torch_steps_ms"] / res["steps_ms"] if res["steps_ms"] > 0 else None
        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = torch.from_numpy(numpy_route(verts.cpu().numpy(), faces.cpu().numpy(), factors)).to(dev)
            torch.cuda.synchronize()
            res["host_route_wall_ms"] = (time.perf_counter() - t0) * 1e3
            res["host_route_over_smooth_mesh"] = res["host_route_wall_ms"] / res["smooth_mesh_wall_ms"]
            res["host_max_abs_diff"] = float((back - ours).abs().max())
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
