"""Times the approximate EMD (mesh_eval.emd_approx, csrc/emd.hip) on the GPU and prints one JSON line.

  python tools/emd_bench.py [--sizes 2048 8192] [--iters 50] [--warmup 10]

Per size n = m, B = 1, two seeded spheres (radius 1 against 1.05, shifted), one scratch buffer reused across calls:
  * `median_ms`, `min_ms`, `p90_ms`: HIP events around single calls;
  * `back_to_back_ms`: `iters` calls enqueued without a wait between them, per call;
  * `grid`: (row tiles, column parts, batch) of a sweep, `scratch_floats`;
  * `pairs_per_s`: 27 n m pair evaluations (nine levels, three sweeps) over the median.
No GPU: the script fails; it never falls back."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("dg-mesh_amd." + n)


def sphere(n, radius, shift, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randn((n, 3), device="cuda", generator=g)
    return (v / v.norm(dim=1, keepdim=True) * radius + torch.tensor([shift, 0.0, 0.0], device="cuda"))[None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "emd_bench needs a GPU"
    M, L = pkg("mesh_eval"), pkg("_lib").lib()
    tiles = M.emd_tiles()
    out = {"tiles": tiles, "sizes": {}}
    for n in args.sizes:
        a, b = sphere(n, 1.0, 0.0, 1), sphere(n, 1.05, 0.02, 2)
        need = int(L.dgm_emd_scratch_floats(1, n, n))
        scratch = torch.empty(need, device="cuda")
        for _ in range(args.warmup):
            cost = M.emd_approx(a, b, scratch=scratch)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cost = M.emd_approx(a, b, scratch=scratch)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            cost = M.emd_approx(a, b, scratch=scratch)
        e1.record()
        e1.synchronize()
        ms.sort()
        med = statistics.median(ms)
        out["sizes"][str(n)] = {
            "median_ms": med, "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "back_to_back_ms": e0.elapsed_time(e1) / args.iters,
            "grid": [-(-n // tiles["rows"]), M.emd_parts(n, n), 1], "scratch_floats": need,
            "pair_evals": 27 * n * n, "pairs_per_s": 27 * n * n / (med * 1e-3), "emd": float(cost[0]) / n}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
