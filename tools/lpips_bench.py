"""Times LPIPS (lpips.LPIPS, csrc/lpips.hip) on the GPU and prints one JSON line per network, then one for testing().

  python tools/lpips_bench.py [--size 800] [--iters 20] [--views 20] [--nets alex vgg]

  * `hip_ms`: HIP-event median of one LPIPS call, B = 2 images against one target, 3 x size x size, seeded full-width weights
    (allocation of its workspace included, as a caller pays it); `hip_tflops`: the convolutions' FLOPs (2 M K N per layer from the
    layer table, M = 3 images' output pixels) over that time -- a whole-call rate, pools, taps and launch gaps included;
  * `torch_ms`: the same network with the same weights as plain F.conv2d / F.max_pool2d in fp32 on the same GPU, the form the
    reference's own run takes; `torch_layers_ms`: its convolutions one by one, next to each layer's GFLOP;
  * `testing`: evaluate.testing on a mesh-phase scene (20 000 Gaussians, DPSR at 128^3), `--views` views, without and with both nets.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = lambda n: importlib.import_module("dg-mesh_amd." + n)


def event_median(fn, iters, warmup=3):
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


def layer_shapes(R, net, n, H, W):
    """[(name, (n, C_in, h, w) input, GFLOP)] per convolution."""
    out, cin, h, w = [], 3, H, W
    for cout, ks, stride, pad, pool, _ in R.NETS[net][0]:
        if pool:
            h, w = (h - pool) // 2 + 1, (w - pool) // 2 + 1
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        out.append((f"{cin}->{cout} k{ks} s{stride} {h}x{w}", (n, cin, h, w), 2.0 * n * ho * wo * ks * ks * cin * cout / 1e9))
        cin, h, w = cout, ho, wo
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--nets", nargs="+", default=["alex", "vgg"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs a GPU")
    import _lpips_ref as R
    LP, E = pkg("lpips"), pkg("evaluate")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    gt = torch.rand(3, a.size, a.size, generator=gen).to(dev)
    images = (gt[None] + 0.1 * torch.randn(2, 3, a.size, a.size, generator=gen).to(dev)).clamp(0, 1)
    models = {}
    for net in a.nets:
        sd = R.seeded_weights(net, 1)
        m = models[net] = LP.LPIPS(net, sd, dev)
        gsd = {k: v.to(dev) for k, v in sd.items()}
        shift, scale = (torch.tensor(v, device=dev).reshape(1, 3, 1, 1) for v in (R.SHIFT, R.SCALE))

        def torch_lpips():
            x = ((2 * torch.cat((images, gt[None])) - 1) - shift) / scale
            taps = R.features(net, gsd, x)
            return sum(R.tap_term(t[:-1], t[-1:], gsd[f"lin{k}.model.1.weight"].reshape(-1)) for k, t in enumerate(taps))

        with torch.no_grad():
            diff = float(((m(images, gt)["lpips"] - torch_lpips().double()).abs() / m(images, gt)["lpips"]).max())
            hip_ms, hip_min = event_median(lambda: m(images, gt), a.iters)
            print(f"[{net}] hip {hip_ms:.3f} ms", flush=True)
            torch_ms, torch_min = event_median(torch_lpips, a.iters)
            print(f"[{net}] torch {torch_ms:.3f} ms", flush=True)
            layers = layer_shapes(R, net, 3, a.size, a.size)
            per_layer = []
            for (name, shape, gflop), (cout, ks, stride, pad, _, _), n in zip(layers, R.NETS[net][0], R.NETS[net][1]):
                x = torch.randn(shape, device=dev)
                w, b = gsd[f"features.{n}.weight"], gsd[f"features.{n}.bias"]
                ms, _ = event_median(lambda: F.relu(F.conv2d(x, w, b, stride=stride, padding=pad)), a.iters)
                per_layer.append({"layer": name, "gflop": round(gflop, 2), "torch_ms": round(ms, 4)})
                del x
        gflop = sum(l[2] for l in layers)
        print(json.dumps({"net": net, "size": a.size, "B": 2, "gflop": round(gflop, 1), "hip_ms": round(hip_ms, 3),
                          "hip_min_ms": round(hip_min, 3), "hip_tflops": round(gflop / hip_ms, 2), "torch_ms": round(torch_ms, 3),
                          "torch_min_ms": round(torch_min, 3), "torch_tflops": round(gflop / torch_ms, 2),
                          "hip_vs_torch_fp32_rel_diff": diff, "torch_layers_ms": per_layer}), flush=True)
        torch.cuda.empty_cache()
    if a.views > 0:
        from test_trainer_dp_gpu import make_mesh_trainer
        T, S = pkg("trainer"), pkg("scene")
        base = make_mesh_trainer(0, 1, res=128, P=20000, W=a.size, H=a.size, n_frames=a.views)
        mesh = T.MeshPhase(*base.mesh.networks(), dpsr=base.mesh.dpsr, n_verts=4000, scale=1.0, device=dev, mesh_source="diffmc")
        mesh.bind(base.g)
        run = lambda lp: E.testing(base.g, base.deform, base.deform_back, base.cameras, pipe=S.PipelineParams(), background=base.bg,
                                   mesh=mesh, lpips=lp)
        out = {"testing_views": a.views, "size": a.size, "P": 20000, "dpsr_res": 128}
        for label, lp in (("without", None), ("with_" + "_".join(models), models)):
            run(lp)
            res = [run(lp) for _ in range(3)]
            out[f"ms_per_view_{label}"] = round(1e3 * statistics.median(r["time_per_view"] for r in res), 3)
            print(f"[testing] {label} done", flush=True)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
