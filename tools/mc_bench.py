"""Marching-cubes micro-benchmark (informational): DiffMC on the DPSR field of bench.py's synthetic mesh-phase scene.

    python tools/mc_bench.py [--res 288] [--iters 20] [--steps 5]

Reports the forward (count + emit, including the {V, F} read-back that sizes the outputs) and backward device times, V and F,
the bytes each pass must move at least and the fraction of the HBM rate (6.29 TB/s, the measured float4-copy rate of the MI355X)
they reach, and the wall time of one mesh-phase training step with mesh_source="probes" against one with "diffmc".
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
HBM = 6.29e12


def _ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def _step_ms(tr, it0, steps):
    for i in range(2):
        tr.step(it0 + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(it0 + 2 + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    bench = importlib.import_module("bench")
    T = importlib.import_module("dg-mesh_amd.trainer")
    M = importlib.import_module("dg-mesh_amd.marching_cubes")
    dev = torch.device("cuda:0")
    tr, _ = bench.build_scene(dev, 0, 1, "hip", phase="mesh", dpsr_res=args.res)
    ms, g = tr.mesh, tr.g
    with torch.no_grad():
        psr = ms.psr(g, None, None).contiguous()
    X, Y, Z = psr.shape
    N = X * Y * Z
    mc = M.DiffMC()
    grid = psr.detach().clone().requires_grad_(True)
    verts, faces = mc(grid)
    V, F = verts.shape[0], faces.shape[0]
    fwd = _ms(lambda: mc(grid), args.iters)
    w = torch.randn_like(verts)
    graphs = [mc(grid)[0] for _ in range(args.iters)]
    bwd = _ms(lambda: torch.autograd.grad(graphs.pop(), grid, w), args.iters)
    # least bytes: forward reads the grid once, writes and reads back the 40 B per 64 points of ballots / counts / offsets, reads
    # both grid values of every crossed edge and writes 12 B per vertex and per face; backward reads the ballots and offsets,
    # the dverts and the grid values at the surface, and writes the whole of dgrid
    fwd_bytes = 4 * N + 2 * 40 * N // 64 + 8 * V + 12 * V + 12 * F
    bwd_bytes = 40 * N // 64 + 4 * N + 12 * V + 8 * V
    probes_ms = _step_ms(tr, tr.opt.dpsr_iter + T.normal_deform_delay(tr.opt) + 1000, args.steps)
    # the same networks, DPSR and Gaussians drive both sources
    mesh = T.MeshPhase(*ms.networks(), dpsr=ms.dpsr, n_verts=ms.probes.shape[0], scale=float(g.gaussian_scale), device=dev,
                       mesh_source="diffmc")
    tr2 = T.Trainer(g, tr.deform, tr.deform_back, tr.cameras, background=tr.bg, is_blender=tr.is_blender, seed=0, mesh=mesh)
    diffmc_ms = _step_ms(tr2, tr.opt.dpsr_iter + T.normal_deform_delay(tr.opt) + 1000, args.steps)
    out = dict(res=[X, Y, Z], V=V, F=F, fwd_ms=round(fwd, 4), bwd_ms=round(bwd, 4), fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes,
               fwd_hbm_frac=round(fwd_bytes / (fwd * 1e-3) / HBM, 3), bwd_hbm_frac=round(bwd_bytes / (bwd * 1e-3) / HBM, 3),
               step_ms_probes=round(probes_ms, 3), step_ms_diffmc=round(diffmc_ms, 3), V_diffmc_last=int(mesh.last_mesh[0].shape[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
