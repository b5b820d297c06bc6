"""Evaluation of the test views on the device: testing() of the reference (R/train.py:559-761, R/ = dgmesh/) with its PSNR
(get_psnr, R/utils/image_utils.py:24-28), SSIM (rgb_ssim, R/utils/metric_utils.py:26-79, numpy + scipy on the host) and MS-SSIM
(pytorch_msssim.ms_ssim on fp64 copies) computed by the kernels of csrc/metrics.hip (dgm_image_metrics, include/dgmesh_hip.h).

pytorch_msssim is not vendored and not a dependency: the MS-SSIM here is this project's own statement of that package's defaults
(11-tap sigma-1.5 window without padding, five levels with weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333, 2x2 average pooling whose
odd sides are zero-padded on both ends, relu on each level's term, mean over channels); tests/_metrics_ref.py restates it in numpy.
LPIPS (the reference's LPIPS_A and LPIPS_V) is computed by the kernels of csrc/lpips.hip through lpips.LPIPS objects that the caller
builds from weight files of their own: the project ships none, and without them testing() reports the three metrics above.  The
Chamfer / EMD metrics of exported meshes against ground truth (the reference's mesh_evaluation.py) are in mesh_eval.py.

The reference copies four images to the host and makes six host round trips per view.  Here one dgm_image_metrics call per view
scores the Gaussian image and the mesh image against the target and writes a row of a device-side table that is read back once,
after the last view."""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib

COLUMNS = ("mse", "psnr", "ssim", "ms_ssim")
MS_SSIM_MIN_SIDE = 161  # (win - 1) * 2^4 < min(H, W)


def _metrics_into(images, gt, out, data_range, levels):
    """images (B, C, H, W), gt (C, H, W) fp32 contiguous on one device; out: (B, 4) float64 view that is written in place."""
    L = _lib.lib()
    B, C, H, W = images.shape
    ws = torch.empty(L.dgm_image_metrics_workspace_bytes(B, C, H, W, levels), dtype=torch.uint8, device=images.device)
    with _lib.device_guard(images.device):
        _lib.check(L.dgm_image_metrics(ctypes.c_void_p(images.data_ptr()), ctypes.c_void_p(gt.data_ptr()), B, C, H, W, float(data_range),
                                       levels, ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr()))


def _checked(images, gt, ms_ssim):
    if not (torch.is_tensor(images) and torch.is_tensor(gt) and images.is_cuda and gt.is_cuda):
        raise RuntimeError("image_metrics needs CUDA/HIP tensors (dg-mesh_amd has no CPU path for its kernels)")
    if images.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("image_metrics needs float32 tensors")
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or gt.dim() != 3 or images.shape[1:] != gt.shape or images.device != gt.device:
        raise ValueError(f"image_metrics: images {tuple(images.shape)} must be (C, H, W) or (B, C, H, W) matching gt {tuple(gt.shape)} "
                         "on the same device")
    H, W = gt.shape[1:]
    if min(H, W) < 11:
        raise ValueError(f"image_metrics: SSIM's 11-tap window needs min(H, W) >= 11, got {H}x{W}")
    if ms_ssim and min(H, W) < MS_SSIM_MIN_SIDE:
        raise ValueError(f"image_metrics: five-level MS-SSIM needs min(H, W) > 160, got {H}x{W}")
    return images.contiguous(), gt.contiguous()


def image_metrics(images, gt, data_range=1.0, ms_ssim=True):
    """MSE, PSNR = -10 log10(mse), SSIM (the rgb_ssim definition) and, when asked, five-level MS-SSIM of `images` ((C, H, W) or
    (B, C, H, W)) against ONE target `gt` (C, H, W): a dict of (B,) float64 device tensors `mse`, `psnr`, `ssim` (+ `ms_ssim`).
    fp32 CUDA/HIP inputs; all arithmetic is fp64 on the device, nothing is read back, and the results are bit-reproducible and
    independent of B.  ValueError: min(H, W) < 11, or <= 160 with ms_ssim."""
    images, gt = _checked(images, gt, ms_ssim)
    out = torch.empty((images.shape[0], 4), dtype=torch.float64, device=images.device)
    _metrics_into(images, gt, out, data_range, 5 if ms_ssim else 1)
    return {k: out[:, i] for i, k in enumerate(COLUMNS) if ms_ssim or k != "ms_ssim"}


def mesh_and_colors(mesh, gaussians, deform_back, d_xyz, d_normal, fid, who="testing"):
    """mesh_renderer of R/utils/renderer.py:124-230 up to its rendering: the DiffMC surface of the deformed Gaussians and the vertex
    colours (deform_back + appearance at the noise-free `fid`, a one-element tensor): (verts, faces, vtx_color).  Shared by
    testing() and the drivers of visualize.py."""
    verts, faces = mesh.surface(gaussians, mesh.psr(gaussians, d_xyz, d_normal))
    V = verts.shape[0]
    if V == 0:
        raise RuntimeError(f"{who}: the DPSR field has no surface at the density threshold (DiffMC returned no vertices)")
    t_v = fid.reshape(1, 1).expand(V, -1)
    back_v = deform_back.step(verts, t_v)[0]
    return verts, faces, mesh.appearance.step(verts + back_v, t_v)


def _mesh_view(mesh, gaussians, deform_back, d_xyz, d_normal, cam, white_background):
    """mesh_and_colors and the mesh image."""
    from .mesh_raster import render_mesh
    verts, faces, vtx_color = mesh_and_colors(mesh, gaussians, deform_back, d_xyz, d_normal, cam.fid)
    return render_mesh(None, verts, faces, vtx_color, cam, whitebackground=white_background), verts, faces, vtx_color


@torch.no_grad()
def testing(gaussians, deform, deform_back, cameras, *, pipe, background, mesh=None, deform_normal=None, is_6dof=False,
            white_background=True, out_dir=None, save_meshes=False, lpips=None, clean=None, simplify=None, smooth=None, repair=None,
            save_glb=False):
    """testing() of R/train.py:559-761 without the image files.  Per camera: deform.step at the camera's
    fid, scene.render clamped to [0, 1]; with `mesh` (a trainer.MeshPhase that has a DPSR module) also mesh.psr -> mesh.surface ->
    deform_back + mesh.appearance on the vertices -> mesh_raster.render_mesh (deform_normal: the network whose first output is added
    to the normals; None = mesh.deform_normal).  One image_metrics call per view scores both images against cam.original_image
    into a device-side (n_views, 2, 4) table -- [:, 0] the Gaussian image, [:, 1] the mesh image (NaN without `mesh`), columns
    mse, psnr, ssim, ms_ssim (NaN when min(H, W) <= 160) -- that is read back once, after the last view.  The only other host waits
    are DiffMC's 8-byte {V, F} read-back per view and the file writes.

    -> {"views": (n_views, 2, 4) float64 numpy array, "columns": COLUMNS, "gaussian": {column: mean}, "mesh": {column: mean} or
    None, "time_per_view": seconds, "fps": views per second}; the time is the wall time of the whole loop with one synchronisation
    at its end, metrics included (the reference times the two renders of each view on the host clock without synchronising).
    out_dir: writes test_results/test_result.txt, the reference's two lines (their LPIPS fields only with `lpips`), and with save_meshes
    test_results/dynamic_mesh/frame_{idx}.ply with vertex colours (ply_io.write_mesh_ply).  The four stages of
    mesh_post, each None or its spec (or a dict of its fields), change the WRITTEN mesh only, its colours following their vertices
    (mesh_post); the mesh image and its metrics are those of the full mesh -- clean: a mesh_clean.CleanSpec, first.  simplify: a
    mesh_simplify.SimplifySpec, after `clean`.  smooth: a mesh_smooth.SmoothSpec, after `clean` and BEFORE `simplify`.  repair: a
    mesh_repair.RepairSpec, LAST, after `simplify`.  save_glb: also writes the reference's test_results/dynamic_glb/frame_{idx}.glb (R/train.py:740), the same written mesh with its
    vertex colours as binary glTF (glb_io.write_mesh_glb); needs mesh and out_dir.

    lpips: None, or {"alex": lpips.LPIPS, "vgg": lpips.LPIPS} with either key optional.  Each network then scores both images of a
    view against the target in one call (the target's features are computed once) into a second device-side table that the same
    read-back brings over, and the result gains "lpips": {"views": (n_views, 2, n_nets) float64, "nets": the nets in the order
    alex, vgg, "gaussian": {net: mean}, "mesh": {net: mean} or None}; the two lines of test_result.txt gain ` LPIPS_A x.xxxx` /
    ` LPIPS_V x.xxxx` after MSSSIM (R/train.py:754-755) for the nets given.  "views" and "columns" are the same with and without."""
    from . import scene as S
    if mesh is not None and mesh.dpsr is None:
        raise RuntimeError("testing: mesh must be a MeshPhase with a DPSR module")
    if save_meshes and (mesh is None or out_dir is None):
        raise ValueError("testing: save_meshes needs mesh and out_dir")
    if save_glb and (mesh is None or out_dir is None):
        raise ValueError("testing: save_glb needs mesh and out_dir")
    cameras = list(cameras)
    if not cameras:
        raise ValueError("testing: no cameras")
    if deform_normal is None and mesh is not None:
        deform_normal = mesh.deform_normal
    dev = gaussians.get_xyz.device
    table = torch.full((len(cameras), 2, 4), float("nan"), dtype=torch.float64, device=dev)
    from . import lpips as LP
    unknown = sorted(set(lpips or {}) - set(LP.NETS))
    if unknown:
        raise ValueError(f"testing: unknown lpips net(s): {', '.join(unknown)}")
    nets = tuple(n for n in LP.NETS if n in (lpips or {}))
    # (view, net, image, the five tap terms and their sum): rows that dgm_lpips writes whole
    lp_table = torch.full((len(cameras), len(nets), 2, 6), float("nan"), dtype=torch.float64, device=dev) if nets else None
    saving_path = None if out_dir is None else os.path.join(out_dir, "test_results")
    if saving_path is not None:
        os.makedirs(saving_path, exist_ok=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for idx, cam in enumerate(cameras):
        xyz = gaussians.get_xyz.detach()
        time_input = cam.fid.reshape(1, 1).expand(xyz.shape[0], -1)
        d_xyz, d_rotation, d_scaling = deform.step(xyz, time_input)[:3]
        gs_image = S.render(cam, gaussians, pipe, background, d_xyz, d_rotation, d_scaling, is_6dof)["render"].clamp(0.0, 1.0)
        gt = cam.original_image
        if mesh is not None:
            d_normal = deform_normal.step(xyz, time_input)
            if isinstance(d_normal, (tuple, list)):
                d_normal = d_normal[0]
            mesh_image, verts, faces, vtx_color = _mesh_view(mesh, gaussians, deform_back, d_xyz, d_normal, cam, white_background)
            images = torch.stack((gs_image, mesh_image))
        else:
            images = gs_image[None]
        ms = min(gt.shape[1:]) >= MS_SSIM_MIN_SIDE
        images, gt = _checked(images, gt, ms)
        _metrics_into(images, gt, table[idx, :images.shape[0]], 1.0, 5 if ms else 1)
        for j, net in enumerate(nets):
            lpips[net]._into(*LP._checked(images, gt, net), lp_table[idx, j, :images.shape[0]])
        if save_meshes or save_glb:
            from . import mesh_post
            w_verts, w_faces, w_color = mesh_post.apply(verts, faces, vtx_color, clean=clean, smooth=smooth, simplify=simplify, repair=repair)
            if save_meshes:
                from .ply_io import write_mesh_ply
                write_mesh_ply(os.path.join(saving_path, "dynamic_mesh", f"frame_{idx}.ply"), w_verts, w_faces, vertex_colors=w_color)
            if save_glb:
                from .glb_io import write_mesh_glb
                write_mesh_glb(os.path.join(saving_path, "dynamic_glb", f"frame_{idx}.glb"), w_verts, w_faces, vertex_colors=w_color)
    torch.cuda.synchronize(dev)
    total = time.perf_counter() - t0
    both = table.flatten() if lp_table is None else torch.cat((table.flatten(), lp_table.flatten()))
    host = both.cpu().numpy()  # the one read-back
    views = host[:table.numel()].reshape(table.shape)
    mean = lambda row: {k: float(views[:, row, i].mean()) for i, k in enumerate(COLUMNS)}
    res = {"views": views, "columns": COLUMNS, "gaussian": mean(0), "mesh": mean(1) if mesh is not None else None,
           "time_per_view": total / len(cameras), "fps": len(cameras) / total}
    if nets:
        lp_views = np.ascontiguousarray(host[table.numel():].reshape(lp_table.shape)[..., 5].transpose(0, 2, 1))  # (view, image, net)
        lp_mean = lambda row: {net: float(lp_views[:, row, j].mean()) for j, net in enumerate(nets)}
        res["lpips"] = {"views": lp_views, "nets": nets, "gaussian": lp_mean(0), "mesh": lp_mean(1) if mesh is not None else None}
    lp_fields = lambda name: "".join(f" LPIPS_{net[0].upper()} {res['lpips'][name][net]:.4f}" for net in nets)
    if saving_path is not None:
        a = res["gaussian"]
        log = f"Gaussian image PSNR {a['psnr']:.4f} SSIM {a['ssim']:.4f} MSSSIM {a['ms_ssim']:.4f}{lp_fields('gaussian')} \n"
        if mesh is not None:
            m = res["mesh"]
            log += f"Mesh image PSNR {m['psnr']:.4f} SSIM {m['ssim']:.4f} MSSSIM {m['ms_ssim']:.4f}{lp_fields('mesh')} "
        log += f"total_time {res['time_per_view']:.4f} fps {res['fps']:.4f} \n"
        with open(os.path.join(saving_path, "test_result.txt"), "w") as fh:
            fh.write(log)
    return res
