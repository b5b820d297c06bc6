"""Mesh-rasterizer micro-benchmark (informational): rasterize / interpolate / antialias on the DiffMC mesh of bench.py's mesh-phase
scene (DPSR 288^3 -> DiffMC) at the workload's resolution (800 x 800).

    python tools/meshrast_bench.py [--res 288] [--iters 20]

Reports V, F, covered pixels, and the median device time (HIP events) of each stage's forward and backward: rasterize
(clear + triangle pass + large-triangle pass + resolve), interpolate (the 4-channel colour + ones of render_mask_and_mesh),
antialias (edge-topology hash + per-pixel gather) and the whole render_mask_and_mesh chain.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/meshrast_bench.py`.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    bench = importlib.import_module("bench")
    MR = importlib.import_module("dg-mesh_amd.mesh_raster")
    dev = torch.device("cuda:0")
    tr, (_, W, H) = bench.build_scene(dev, 0, 1, "hip", phase="mesh", dpsr_res=args.res)
    ms, g = tr.mesh, tr.g
    cam = tr.cameras[0]
    with torch.no_grad():
        verts, faces = ms.surface(g, ms.psr(g, None, None).contiguous())
    V, F = verts.shape[0], faces.shape[0]
    color = torch.rand((V, 3), device=dev)
    attr = torch.cat([color, torch.ones_like(color[:, :1])], 1).contiguous()
    pos = MR.clip_positions(cam, verts).detach().requires_grad_(True)
    rast, _ = MR.rasterize(None, pos, faces, (H, W))
    col, _ = MR.interpolate(attr, rast, faces)
    out = MR.antialias(col.detach(), rast.detach(), pos.detach(), faces)
    covered = int((rast[0, ..., 3] > 0).sum())
    res = dict(res=args.res, H=H, W=W, V=V, F=F, covered=covered)
    with torch.no_grad():
        res["rasterize_fwd_ms"] = _ms(lambda: MR.rasterize(None, pos, faces, (H, W)), args.iters)
        res["interpolate_fwd_ms"] = _ms(lambda: MR.interpolate(attr, rast, faces), args.iters)
        res["antialias_fwd_ms"] = _ms(lambda: MR.antialias(col, rast, pos, faces), args.iters)
    # backward passes alone: graphs built up front, one backward per timed call
    d4 = torch.randn((1, H, W, 4), device=dev)
    p = pos.detach().requires_grad_(True)
    graphs = [MR.rasterize(None, p, faces, (H, W))[0] for _ in range(args.iters + 1)]
    res["rasterize_bwd_ms"] = _ms(lambda: torch.autograd.grad(graphs.pop(), p, d4), args.iters)
    a = attr.detach().requires_grad_(True)
    graphs = [MR.interpolate(a, rast.detach(), faces)[0] for _ in range(args.iters + 1)]
    res["interpolate_bwd_ms"] = _ms(lambda: torch.autograd.grad(graphs.pop(), a, d4), args.iters)
    c = col.detach().requires_grad_(True)
    graphs = [MR.antialias(c, rast.detach(), p, faces) for _ in range(args.iters + 1)]
    res["antialias_bwd_ms"] = _ms(lambda: torch.autograd.grad(graphs.pop(), [c, p], d4), args.iters)
    vv = verts.detach().requires_grad_(True)
    cc = color.detach().requires_grad_(True)
    cam.gt_alpha_mask = torch.zeros((H, W, 1), device=dev)

    def chain():
        m, img = MR.render_mask_and_mesh(None, vv, faces, cc, cam)
        (m.sum() + img.sum()).backward()

    res["chain_fwd_bwd_ms"] = _ms(chain, args.iters)
    del out
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
