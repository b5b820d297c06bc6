"""Times the test-view metrics (evaluate.image_metrics, csrc/metrics.hip) on the GPU and prints one JSON line.

  python tools/metrics_bench.py [--size 800] [--iters 200] [--views 8]

  * `hip_ms`: HIP-event median of one image_metrics call, B = 2 images against one target, 3 x size x size, five MS-SSIM levels
    (allocation of its workspace included, as a caller pays it);
  * `torch_ms`: the same four numbers formed with torch grouped convolutions in fp32 on the same GPU, for orientation only (it is
    not the reference's path, which runs rgb_ssim on the host);
  * `testing_ms_per_view`: evaluate.testing on a mesh-phase scene (20 000 Gaussians, DPSR at 128^3), Gaussian and mesh image per view.
No GPU: the script fails; it never falls back."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("dg-mesh_amd." + n)
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_metrics(images, gt):
    """(B, C, H, W) against (C, H, W): mse, psnr, rgb_ssim and ms_ssim with grouped convolutions (fp32)."""
    B, C = images.shape[:2]
    g = torch.exp(-((torch.arange(11, device=images.device) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    kh, kv = g.reshape(1, 1, 1, 11).repeat(C, 1, 1, 1), g.reshape(1, 1, 11, 1).repeat(C, 1, 1, 1)
    blur = lambda z: F.conv2d(F.conv2d(z, kh, groups=C), kv, groups=C)
    x, y = images, gt[None].expand_as(images)
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    terms, rgb = [], None
    for l in range(5):
        mu0, mu1 = blur(x), blur(y)
        s00, s11, s01 = blur(x * x) - mu0 * mu0, blur(y * y) - mu1 * mu1, blur(x * y) - mu0 * mu1
        cs = (2 * s01 + c2) / (s00 + s11 + c2)
        lum = (2 * mu0 * mu1 + c1) / (mu0 * mu0 + mu1 * mu1 + c1)
        if l == 0:
            k00, k11 = s00.clamp_min(0), s11.clamp_min(0)
            k01 = torch.sign(s01) * torch.minimum(torch.sqrt(k00 * k11), s01.abs())
            rgb = (lum * (2 * k01 + c2) / (k00 + k11 + c2)).mean(dim=(1, 2, 3))
        terms.append(torch.relu((cs if l < 4 else lum * cs).mean(dim=(2, 3))) ** WEIGHTS[l])
        if l < 4:
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    return mse, -10 * torch.log10(mse), rgb, torch.stack(terms).prod(0).mean(1)


def event_median(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU")
    E = pkg("evaluate")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    gt = torch.rand(3, a.size, a.size, generator=gen).to(dev)
    images = (gt[None] + 0.05 * torch.randn(2, 3, a.size, a.size, generator=gen).to(dev)).clamp(0, 1)
    hip = E.image_metrics(images, gt)
    ref = torch_metrics(images, gt)
    dev_diff = {k: float((hip[k] - r.double()).abs().max()) for k, r in zip(E.COLUMNS, ref)}
    hip_ms, hip_min = event_median(lambda: E.image_metrics(images, gt), a.iters)
    torch_ms, torch_min = event_median(lambda: torch_metrics(images, gt), a.iters)
    out = {"size": a.size, "B": 2, "levels": 5, "hip_ms": round(hip_ms, 4), "hip_min_ms": round(hip_min, 4),
           "torch_ms": round(torch_ms, 4), "torch_min_ms": round(torch_min, 4), "hip_vs_torch_fp32_abs_diff": dev_diff}
    if a.views > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_trainer_dp_gpu import make_mesh_trainer
        T, S = pkg("trainer"), pkg("scene")
        base = make_mesh_trainer(0, 1, res=128, P=20000, W=a.size, H=a.size, n_frames=a.views)
        mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=dev, mesh_source="diffmc")
        mesh.bind(base.g)
        run = lambda: E.testing(base.g, base.deform, base.deform_back, base.cameras, pipe=S.PipelineParams(), background=base.bg, mesh=mesh)
        run()
        res = [run() for _ in range(3)]
        out["testing_ms_per_view"] = round(1e3 * statistics.median(r["time_per_view"] for r in res), 3)
        out["testing_views"], out["testing_P"], out["testing_dpsr_res"] = a.views, 20000, 128
    print(json.dumps(out))


if __name__ == "__main__":
    main()
