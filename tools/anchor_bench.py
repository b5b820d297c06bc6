"""Gaussian-mesh anchoring micro-benchmark (informational) on bench.py's mesh-phase scene (P = 100 k Gaussians, DPSR 288^3 ->
DiffMC, ~4.7 M faces).

    python tools/anchor_bench.py [--res 288] [--iters 10]

Reports the median device time (HIP events) of: face geometry; the nearest-face search (grid build + query) at the bounds of
search_radius 0.0005 and 0.0015 (the d-nerf configs; bound = gaussian_scale * radius, squared distances, as in the reference);
the classification; the unbounded search (P x P, the tiled brute force); the whole plan + apply (with the deformation MLP
calls); and a chunked fp32 brute-force nearest neighbour (torch, the same formula) on the same inputs for comparison.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/anchor_bench.py`.  Prints one JSON line."""
import argparse
import copy
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    fn()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def brute(q, t, max_d2, chunk=512):
    best = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    idx = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    for s in range(0, q.shape[0], chunk):
        qq = q[s:s + chunk]
        dx = t[None, :, 0] - qq[:, None, 0]
        dy = t[None, :, 1] - qq[:, None, 1]
        dz = t[None, :, 2] - qq[:, None, 2]
        m, j = ((dx * dx + dy * dy) + dz * dz).min(1)
        best[s:s + chunk], idx[s:s + chunk] = m, torch.where(m < max_d2, j, torch.full_like(j, -1))
    return idx, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--brute-queries", type=int, default=8192, help="queries of the brute-force comparison (scaled to P)")
    args = ap.parse_args()
    bench = importlib.import_module("bench")
    A = importlib.import_module("dg-mesh_amd.anchor")
    dev = torch.device("cuda:0")
    tr, _ = bench.build_scene(dev, 0, 1, "hip", phase="mesh", dpsr_res=args.res)
    ms, g = tr.mesh, tr.g
    t = tr.cameras[0].fid
    with torch.no_grad():
        verts, faces = ms.surface(g, ms.psr(g, None, None).contiguous())
        P = g._xyz.shape[0]
        x = (g.get_xyz + tr.deform.step(g.get_xyz, t.reshape(1, 1).expand(P, -1))[0]).contiguous()
    F = faces.shape[0]
    res = dict(res=args.res, P=P, V=verts.shape[0], F=F, scale=float(g.gaussian_scale.reshape(-1)[0]))
    res["face_geometry_ms"] = _ms(lambda: A.face_geometry(verts, faces), args.iters)
    cent, _ = A.face_geometry(verts, faces)
    for r in (0.0005, 0.0015):
        bound = float(torch.tensor(res["scale"], dtype=torch.float32) * r)
        idx, _ = A._nearest_raw(x, cent, bound)
        res[f"nn_ms_r{r}"] = _ms(lambda: A._nearest_raw(x, cent, bound), args.iters)
        res[f"valid_r{r}"] = int((idx >= 0).sum())
        nb = min(args.brute_queries, P)
        bi, _ = brute(x[:nb], cent, bound)
        assert torch.equal(bi.to(torch.int32), idx[:nb]), "grid NN != brute force"
        res[f"brute_ms_r{r}"] = _ms(lambda: brute(x[:nb], cent, bound), max(2, args.iters // 5)) * P / nb
        res[f"classify_ms_r{r}"] = _ms(lambda: A.classify(idx, F), args.iters)
    opt = tr.opt
    res["brute_scaled_from_queries"] = min(args.brute_queries, P)
    # the unbounded search (max_d2 = inf, the tiled brute force): all P Gaussians against P face centroids, the size of
    # normal_initialization's query (P Gaussians against P surface samples)
    sub = cent[torch.randperm(F, device=dev)[:P]].contiguous()
    res["nn_unbounded_PxP_ms"] = _ms(lambda: A._nearest_raw(x, sub, float("inf")), max(2, args.iters // 5))

    def plan_apply():
        gg = copy.copy(g)  # (a shallow copy: apply re-seats Parameters on the copy and its optimizer copy)
        gg.optimizer = torch.optim.Adam([dict(grp, params=list(grp["params"])) for grp in g.optimizer.param_groups], lr=0.0,
                                        eps=1e-15)
        plan = A.plan_anchor(gg, verts, faces, tr.deform, tr.deform_back, t, opt.anchor_search_radius, opt.anchor_topn,
                             opt.anchor_n_1_bs, opt.anchor_0_1_bs)
        plan["loss"].backward()
        return A.apply_anchor(gg, plan)

    res["plan_apply_ms"] = _ms(plan_apply, args.iters)
    res["plan_apply_info"] = plan_apply()
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
