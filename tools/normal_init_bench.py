"""Stage timer of entering the mesh phase (normal_init.normal_initialization; informational) on bench.py's mesh-phase scene
(P = 100 k Gaussians).

    python tools/normal_init_bench.py [--iters 5]

Reports the median device time (HIP events) of: the 50 deformation passes + bounding-box launches (update_scale_center); the opacity
field at 256^3; DiffMC of it; face areas + the fp64 scan; sampling P points; the nearest-sample search (P x P, unbounded); the whole
normal_initialization.  For orientation, the reference-shaped host path of the sampling stage (mesh to numpy, cumsum / searchsorted
on the CPU, samples back to the device) is timed on the same mesh with a wall clock.  The chain is also run once under
torch.cuda.set_sync_debug_mode("error") with DiffMC's {V, F} read-back -- its one host synchronisation -- exempted: any other
synchronising call raises.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def host_sampling(verts, faces, count, rng):
    """trimesh.sample.sample_surface's shape: mesh to the host, numpy cumsum / searchsorted, samples back to the device."""
    v, f = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy()
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    cum = np.cumsum(area)
    idx = np.searchsorted(cum, rng.random(count) * cum[-1])
    r = rng.random((count, 2, 1))
    fold = r.sum(1).reshape(-1) > 1.0
    r[fold] -= 1.0
    pts = ((tri[idx, 1:] - tri[idx, :1]) * np.abs(r)).sum(1) + tri[idx, 0]
    return torch.tensor(pts, dtype=torch.float32, device=verts.device), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    bench = importlib.import_module("bench")
    N = importlib.import_module("dg-mesh_amd.normal_init")
    A = importlib.import_module("dg-mesh_amd.anchor")
    M = importlib.import_module("dg-mesh_amd.mesh_utils")
    MC = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    tr, _ = bench.build_scene(dev, 0, 1, "hip", phase="mesh")
    g, deform = tr.g, tr.deform
    P = g._xyz.shape[0]
    opt = types.SimpleNamespace(init_density_threshold=0.05)
    gen = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        t = tr.cameras[0].fid.reshape(1, 1).expand(P, -1)
        d_xyz, d_rot, d_scl = deform.step(g.get_xyz.detach(), t)[:3]
        xyz = (g.get_xyz + d_xyz).detach().contiguous()
        field = lambda: M.get_opacity_field_from_gaussians(xyz, g.get_rotation + d_rot, g.get_scaling + d_scl, g.get_opacity, bbox_scale=2.0)
        occ = field()
        diffmc = MC.DiffMC()
        verts, faces = diffmc(-occ, isovalue=N.ISOVALUE)
        verts = (verts * 4.0 - 2.0).contiguous()
        F = faces.shape[0]
        res = dict(P=P, V=verts.shape[0], F=F)
        res["scale_center_50_frames_ms"] = _ms(lambda: N.update_scale_center(g, deform), args.iters)
        res["opacity_field_256_ms"] = _ms(field, args.iters)
        res["diffmc_ms"] = _ms(lambda: diffmc(-occ, isovalue=N.ISOVALUE), args.iters)
        res["areas_scan_ms"] = _ms(lambda: N.cumulative_areas(N.face_areas(verts, faces)), args.iters)
        u = torch.rand((P, 3), device=dev, generator=gen)
        res["sample_ms"] = _ms(lambda: N.sample_surface(verts, faces, P, draws=u, check=False), args.iters)
        samples, _ = N.sample_surface(verts, faces, P, draws=u, check=False)
        res["face_normals_ms"] = _ms(lambda: A.face_geometry(verts, faces), args.iters)
        res["nearest_sample_ms"] = _ms(lambda: A.nearest(xyz, samples), args.iters)
        chain = lambda: N.normal_initialization(g, deform, d_xyz, d_rot, d_scl, opt=opt, generator=gen, diffmc=diffmc)
        res["total_ms"] = _ms(chain, args.iters)
        # the reference-shaped host path of the sampling stage, wall clock (it synchronises by construction)
        rng = np.random.default_rng(0)
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_sampling(verts, faces, P, rng)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        res["host_path_sampling_wall_ms"] = sorted(times)[1]
        # host synchronisations: everything but DiffMC's {V, F} read-back must run under the "error" mode
        count_fn = MC._MarchingCubes.forward

        def exempt(ctx, *a):
            torch.cuda.set_sync_debug_mode("default")
            try:
                return count_fn(ctx, *a)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        MC._MarchingCubes.forward = staticmethod(exempt)
        torch.cuda.set_sync_debug_mode("error")
        try:
            chain()
            res["host_syncs_besides_diffmc"] = 0
        finally:
            torch.cuda.set_sync_debug_mode("default")
            MC._MarchingCubes.forward = staticmethod(count_fn)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
