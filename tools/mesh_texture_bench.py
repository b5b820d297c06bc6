"""Timer of the texture bake and of mesh_raster.texture (informational) on a mesh of the mesh phase's size: DiffMC of the synthetic
two-body field of tools/mesh_clean_bench.py on the 288^3 grid, decimated by mesh_simplify at grid 128.

    timeout 600 python tools/mesh_texture_bench.py [--res 288] [--blobs 500] [--grid 128] [--size 2048] [--side 800] [--iters 7]

Reports the median of `iters` runs after a warm-up, in HIP events on the stream and as wall time with a synchronisation:
  atlas            dgm_atlas_interpolate of the vertex positions into the size^2 atlas (the bake's kernel) with the bytes it must move
                   -- 16 bytes written per texel (three floats and the face id), the faces and vertices read once -- and bytes / s;
                   dgm_atlas_uv beside it;
  network          the appearance of evaluate.mesh_and_colors (deform_back.step + appearance.step, freshly initialised networks) on the
                   owned texels in chunks of 2^18: the bake's other part, timed separately; texels / s;
  bake             mesh_texture.bake end to end (kernel, ownership, chunked network, the scatter into the texture);
  texture          mesh_raster.texture of the baked (size, size, 3) texture at side x side samples, linear / clamp, forward and
                   backward: once at the uv of the mesh rasterized into a side x side view (a chart-coherent gather, what
                   render_mesh_textured does; the background pixels sit at uv = (0, 0) and get a zero output gradient, as there) and
                   once at uniformly random uv; the bytes counted are the uv read and the output written
                   (`stream`) and 4 texels per sample (`gather`, an upper bound on what must come from memory: neighbours share texels);
  grid_sample      torch.nn.functional.grid_sample (bilinear, border, align_corners=False) of the same texture in NCHW at the same uv
                   on the same GPU, forward and backward, and the largest difference of its output from texture()'s.
Rates are bytes over the HIP-event time; the chip's read rate for comparison is 6.3 TB/s for a copy (8 TB/s on the data sheet).
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_clean_bench import _times, two_body_field  # noqa: E402

COPY_RATE = 6.3e12  # bytes / s of a float4 copy on the chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=288)
    ap.add_argument("--blobs", type=int, default=500)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    pk = lambda name: importlib.import_module("dg-mesh_amd." + name)
    MT, MR, MC, MS, D, SC, syn = (pk(n) for n in ("mesh_texture", "mesh_raster", "marching_cubes", "mesh_simplify", "deform", "scene", "synthetic"))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with torch.no_grad():
        verts, faces = MC.marching_cubes(two_body_field(args.res, args.blobs, dev), isovalue=0.0, normalize=False)
        res = dict(res=args.res, V_full=int(verts.shape[0]), F_full=int(faces.shape[0]), grid=args.grid)
        verts, faces = MS.simplify_mesh(verts.contiguous(), faces.contiguous(), grid=args.grid)
        lo, hi = verts.min(0).values, verts.max(0).values
        verts = ((verts - (lo + hi) / 2) / (hi - lo).max() * 2.0).contiguous()  # into [-1, 1]^3: what the networks and the camera see
        faces = faces.contiguous()
        V, F = int(verts.shape[0]), int(faces.shape[0])
        atlas = MT.build_atlas(F, size=args.size)
        texels = atlas.size * atlas.size
        res.update(V=V, F=F, size=atlas.size, cell=atlas.cell, texels=texels)

        pos, face_id = MT.atlas_interpolate(atlas, verts, faces)
        owned = int((face_id >= 0).sum())
        res["owned_texels"], res["owned_share"] = owned, owned / texels
        res["atlas_ms"], res["atlas_wall_ms"] = _times(lambda: MT.atlas_interpolate(atlas, verts, faces), args.iters)
        res["atlas_bytes"] = texels * 16 + F * 12 + V * 12
        res["atlas_bytes_per_s"] = res["atlas_bytes"] / (res["atlas_ms"] * 1e-3)
        res["atlas_share_of_copy_rate"] = res["atlas_bytes_per_s"] / COPY_RATE
        res["atlas_uv_ms"], _ = _times(lambda: MT.atlas_uv(atlas, dev), args.iters)

        mesh = types.SimpleNamespace(appearance=D.AppearanceModel(is_blender=True, device=dev))
        deform_back = D.DeformModel(is_blender=True, device=dev)
        color_fn = MT.appearance_color_fn(mesh, deform_back, torch.tensor([0.25], device=dev))
        points = pos.reshape(-1, 3)[(face_id.reshape(-1) >= 0).nonzero().reshape(-1)]
        chunk = 1 << 18

        def network():
            for at in range(0, owned, chunk):
                color_fn(points[at:at + chunk])

        res["network_ms"], res["network_wall_ms"] = _times(network, max(3, args.iters // 2))
        res["network_texels_per_s"] = owned / (res["network_ms"] * 1e-3)
        res["bake_ms"], res["bake_wall_ms"] = _times(lambda: MT.bake(verts, faces, color_fn, size=args.size), max(3, args.iters // 2))
        tex, uv, _ = MT.bake(verts, faces, color_fn, size=args.size)

    # texture() at side x side samples
    side = args.side
    n = side * side
    cam = SC.TorchCamera(syn.make_camera(side, side, radius=3.2), dev)
    with torch.no_grad():
        rast, _ = MR.rasterize(None, MR.clip_positions(cam, verts), faces, (side, side))
        corner = torch.arange(3 * F, dtype=torch.int32, device=dev).reshape(F, 3)
        uv_mesh, _ = MR.interpolate(uv.reshape(3 * F, 2).contiguous(), rast, corner)
        res["covered_share"] = float((rast[..., 3] > 0).float().mean())
    uv_rand = torch.rand((1, side, side, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    tex4 = tex[None].contiguous()
    nchw = tex4.permute(0, 3, 1, 2).contiguous()
    res["side"], res["samples"] = side, n
    res["texture_stream_bytes"], res["texture_gather_bytes"] = n * (8 + 12), n * 4 * 12
    covered = (rast[..., 3:4] > 0).float()
    for name, q in (("mesh_uv", uv_mesh.contiguous()), ("random_uv", uv_rand)):
        g = torch.randn((1, side, side, 3), device=dev)
        if name == "mesh_uv":
            g = g * covered  # (as in render_mesh_textured: background pixels, all at uv = (0, 0), carry no gradient)
        with torch.no_grad():
            ours = MR.texture(tex4, q, boundary_mode="clamp")
            theirs = torch.nn.functional.grid_sample(nchw, 2 * q - 1, mode="bilinear", padding_mode="border", align_corners=False)
            res[f"{name}_max_abs_diff"] = float((ours - theirs.permute(0, 2, 3, 1)).abs().max())
            res[f"{name}_texture_ms"], res[f"{name}_texture_wall_ms"] = _times(lambda: MR.texture(tex4, q, boundary_mode="clamp"), args.iters)
            res[f"{name}_grid_sample_ms"], _ = _times(
                lambda: torch.nn.functional.grid_sample(nchw, 2 * q - 1, mode="bilinear", padding_mode="border", align_corners=False), args.iters)
        t = res[f"{name}_texture_ms"] * 1e-3
        res[f"{name}_stream_bytes_per_s"] = res["texture_stream_bytes"] / t
        res[f"{name}_stream_plus_gather_bytes_per_s"] = (res["texture_stream_bytes"] + res["texture_gather_bytes"]) / t
        res[f"{name}_grid_sample_over_texture"] = res[f"{name}_grid_sample_ms"] / res[f"{name}_texture_ms"]

        def ours_fb():
            a, b = tex4.detach().requires_grad_(True), q.detach().requires_grad_(True)
            torch.autograd.grad(MR.texture(a, b, boundary_mode="clamp"), [a, b], grad_outputs=g)

        def theirs_fb():
            a, b = nchw.detach().requires_grad_(True), q.detach().requires_grad_(True)
            out = torch.nn.functional.grid_sample(a, 2 * b - 1, mode="bilinear", padding_mode="border", align_corners=False)
            torch.autograd.grad(out, [a, b], grad_outputs=g.permute(0, 3, 1, 2))

        res[f"{name}_texture_fwd_bwd_ms"], _ = _times(ours_fb, args.iters)
        res[f"{name}_grid_sample_fwd_bwd_ms"], _ = _times(theirs_fb, args.iters)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) and 1e-2 < abs(v) < 1e6 else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
