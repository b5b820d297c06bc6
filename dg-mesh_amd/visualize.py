"""Rendering a trained checkpoint: the reference's render_test.py and render_trajectory.py (R/ = the reference's dgmesh/) and the
dynamic-mesh export at the end of training (R/train.py:389-423).  A frame puts panels side by side: the vertex-coloured mesh image
(mesh_raster.render_mesh), a shaded "shape" image of the bare mesh (mesh_shape_renderer, R/utils/renderer.py:236-319, a PyTorch3D
Phong pass there) and a point-cloud image of the deformed Gaussians (pointcloud_renderer, :322-374, a matplotlib scatter on the host
there).  The passes are HIP kernels of libdgmesh_hip (csrc/visualize.hip).  float32, CUDA/HIP tensors only -- no CPU fallback;
anything else raises.

Conventions chosen here (PyTorch3D and matplotlib are not vendored and were not available to compare against, so these are this
project's statement of what the reference's calls resolve to):
  * shape image: a deferred hard-Phong pass over the rasterizer's rast buffer, on render_mesh's pixel grid with no flips (the
    reference flips its PyTorch3D image to get there).  Per covered pixel the world position and the area-weighted vertex normal
    (vertex_normals) are interpolated with (u, v, 1 - u - v) and the normal renormalised; one directional light l;
    colour = clamp((ambient + diffuse * max(n.l, 0)) * base_color + specular * spec, 0, 1), spec = max(view.r, 0)^shininess where
    n.l > 0 (r = 2 (n.l) n - l, view = normalize(camera_center - p)), else 0.  Defaults: PyTorch3D's DirectionalLights defaults and
    the reference's Materials(specular_color=0.2, shininess=10): ambient 0.5, diffuse 0.3, specular 0.2 x 0.2 (light x material),
    shininess 10, base colour 1, white background.  The default light is the reference's headlight,
    normalize(camera_center - verts.mean(0)), computed on the device.
  * back faces are not lit (as PyTorch3D; the shader is one-sided).  DiffMC winds its faces so that (v1 - v0) x (v2 - v0) points from
    f < iso to f >= iso (marching_cubes.py), and MeshPhase.psr makes the field positive outside the object, so the meshes the drivers
    shade are wound outwards and need no flip (tests/test_visualize.py checks it on a sphere).  `flip_normals=True` negates the
    normals for a mesh wound the other way;
  * point cloud: every point with w > 0 and finite coordinates lands on pixel floor(s), s = ((x/w + 1) W/2, (y/w + 1) H/2) -- the
    rasterizer's mapping, so dots, mesh and Gaussians share pixels -- and covers the size x size square centred there (size odd,
    1..15), clipped to the image; the smallest z/w wins a pixel, ties to the lower point id.  Blue on white, as the reference draws;
  * frames: panels (3, H, W) or (H, W, 3) side by side, optionally averaged over 2x2 blocks as ((a + b) + (c + d)) * 0.25 (cv2.resize's
    INTER_LINEAR at exactly half size is that average), then clamp to [0, 1], x 255, truncated (the reference's astype(np.uint8));
    NaN writes 0;
  * reproducibility: splat_points and compose_frame are bit-identical run to run.  vertex_normals sums with fp32 atomics, so it, and
    the shape image through it, agree to rounding only.
The drivers keep every frame in one device-side uint8 tensor that is read back once, after the last frame; per frame the only host
wait is DiffMC's 8-byte {V, F} read.  Video encoding (gif / mp4) is not provided: there is no encoder to depend on.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib
from .mesh_raster import _check_rast, _need, _st, clip_positions, rasterize, render_mesh

MATERIAL = {"ambient": 0.5, "diffuse": 0.3, "specular": 0.2 * 0.2, "shininess": 10.0, "base_color": (1.0, 1.0, 1.0)}
MAX_PANELS = 4


def _check_mesh(name, verts, faces):
    _need(name, verts, "verts", torch.float32)
    _need(name, faces, "faces", torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"{name}: verts must be (V, 3), got {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"{name}: faces must be (F, 3), got {tuple(faces.shape)}")
    if faces.device != verts.device:
        raise RuntimeError(f"{name}: verts and faces must be on one device")


def _rgb(name, what, c):
    c = tuple(float(x) for x in c)
    if len(c) != 3:
        raise ValueError(f"{name}: {what} must have three components")
    return c


def vertex_normals(verts, faces):
    """Area-weighted unit vertex normals (V, 3): the unnormalised (v1 - v0) x (v2 - v0) of every face added to its three vertices,
    each vertex then normalised; accumulated length below 1e-6 (an unreferenced vertex, zero-area faces only) -> (0, 0, 0).  Faces
    with an index outside [0, V) are skipped, as the rasterizer skips them.  The sums are fp32 atomics: the result agrees to
    rounding, not bit for bit, run to run."""
    _check_mesh("vertex_normals", verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    normals = torch.empty_like(verts)
    with _lib.device_guard(verts.device):
        _lib.check(_lib.lib().dgm_vertex_normals(V, F, _lib.vp(verts), _lib.vp(faces), _lib.vp(normals), _st()))
    return normals


def mesh_shape_renderer(verts, faces, cam, *, light_dir=None, rast=None, background=(1.0, 1.0, 1.0), flip_normals=False, **material):
    """mesh_shape_renderer of R/utils/renderer.py:236-319: the shaded image (H, W, 3) of the bare mesh seen from `cam` (module
    docstring for the shading rule and its defaults).  verts (V, 3) world space, faces (F, 3) int32, cam: a TorchCamera.
    light_dir: the direction towards the light (3 numbers or a device tensor; normalised here); None = the reference's headlight,
    normalize(cam.camera_center - verts.mean(0)), computed on the device.  rast: the (1, H, W, 4) buffer of
    mesh_raster.rasterize(clip_positions(cam, verts), faces, (H, W)) when the caller already has it; None rasterizes here.
    flip_normals: negate the vertex normals (a mesh wound inwards; back faces are not lit).  material: ambient, diffuse, specular,
    shininess (numbers) and base_color (3 numbers), defaults MATERIAL."""
    name = "mesh_shape_renderer"
    _check_mesh(name, verts, faces)
    unknown = set(material) - set(MATERIAL)
    if unknown:
        raise TypeError(f"{name}: unknown material argument(s) {sorted(unknown)}; known: {sorted(MATERIAL)}")
    m = dict(MATERIAL, **material)
    H, W = int(cam.image_height), int(cam.image_width)
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if rast is None:
        rast, _ = rasterize(None, clip_positions(cam, verts), faces, (H, W))
    else:
        _check_rast(name, rast, dev)
        if tuple(rast.shape[1:3]) != (H, W):
            raise RuntimeError(f"{name}: rast {tuple(rast.shape)} does not match the camera's {(H, W)}")
    center = cam.camera_center.to(device=dev, dtype=torch.float32).reshape(3)
    if light_dir is None:
        light = center - verts.mean(0) if V > 0 else center
    else:
        light = torch.as_tensor(light_dir, dtype=torch.float32).to(dev).reshape(3)
    # one dgm_shade_params (include/dgmesh_hip.h) in device memory: the constants come from the host, the light and the camera
    # centre are written on the device
    bg, base = _rgb(name, "background", background), _rgb(name, "base_color", m["base_color"])
    params = torch.tensor([0.0, 0.0, 0.0, float(m["ambient"]), 0.0, 0.0, 0.0, float(m["diffuse"]), *bg, float(m["specular"]), *base,
                           float(m["shininess"]), -1.0 if flip_normals else 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    params[0:3] = light / light.norm()
    params[4:7] = center
    normals = vertex_normals(verts, faces)
    image = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().dgm_mesh_shade(V, F, H, W, _lib.vp(verts), _lib.vp(normals), _lib.vp(faces), _lib.vp(rast), _lib.vp(params), _lib.vp(image), _st()))
    return image


def splat_points(pos_clip, H, W, colors=None, color=(0.0, 0.0, 1.0), size=1, background=(1.0, 1.0, 1.0), return_ids=False):
    """The point-cloud image (H, W, 3) of clip-space points pos_clip (N, 4) or (1, N, 4) (module docstring for the rule).  colors:
    (N, 3) per-point colours, or None for the uniform `color`.  return_ids: also the (H, W) int64 image of the winning point ids,
    -1 on background.  Bit-identical run to run."""
    name = "splat_points"
    _need(name, pos_clip, "pos_clip", torch.float32)
    if pos_clip.dim() == 3 and pos_clip.shape[0] == 1:
        pos_clip = pos_clip[0]
    if pos_clip.dim() != 2 or pos_clip.shape[1] != 4:
        raise RuntimeError(f"{name}: pos_clip must be (N, 4) or (1, N, 4) clip-space positions, got {tuple(pos_clip.shape)}")
    H, W, size = int(H), int(W), int(size)
    if not (0 < H <= 16384 and 0 < W <= 16384):
        raise ValueError(f"{name}: resolution must be within [1, 16384]^2, got {(H, W)}")
    if size < 1 or size > 15 or size % 2 == 0:
        raise ValueError(f"{name}: size must be odd, 1 to 15, got {size}")
    N, dev = int(pos_clip.shape[0]), pos_clip.device
    if colors is not None:
        _need(name, colors, "colors", torch.float32)
        if tuple(colors.shape) != (N, 3) or colors.device != dev:
            raise RuntimeError(f"{name}: colors must be ({N}, 3) on the points' device, got {tuple(colors.shape)}")
    L = _lib.lib()
    bg6 = (ctypes.c_float * 6)(*_rgb(name, "background", background), *_rgb(name, "color", color))
    scratch = torch.empty(int(L.dgm_point_splat_scratch_bytes(H, W)), dtype=torch.uint8, device=dev)
    image = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_point_splat(N, H, W, _lib.vp(pos_clip), _lib.vp(colors), size, bg6, _lib.vp(scratch), _lib.vp(image), _st()))
    if not return_ids:
        return image
    keys = scratch[:H * W * 8].view(torch.int64).reshape(H, W)  # (ordered z/w bits) << 32 | id; all ones: empty
    return image, torch.where(keys == -1, keys, keys & 0xFFFFFFFF)


def pointcloud_renderer(points, cam, **kw):
    """pointcloud_renderer of R/utils/renderer.py:322-374: world-space points (N, 3) seen from `cam` as dots, (H, W, 3); kw: the
    keyword arguments of splat_points."""
    _need("pointcloud_renderer", points, "points", torch.float32)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"pointcloud_renderer: points must be (N, 3), got {tuple(points.shape)}")
    return splat_points(clip_positions(cam, points), int(cam.image_height), int(cam.image_width), **kw)


def _panel_layout(p, layout):
    """-> (H, W, hwc flag, tensor whose memory is read).  A (3, H, W) panel that is a permuted view of (H, W, 3) memory (render_mesh
    returns one) is read in place as (H, W, 3)."""
    if p.dim() != 3:
        raise ValueError(f"compose_frame: a panel must be (3, H, W) or (H, W, 3), got {tuple(p.shape)}")
    if layout is None:
        chw, hwc = p.shape[0] == 3, p.shape[2] == 3
        if not (chw or hwc):
            raise ValueError(f"compose_frame: a panel must be (3, H, W) or (H, W, 3), got {tuple(p.shape)}")
        layout = "hwc" if hwc else "chw"  # ((3, n, 3) reads as (H = 3, W = n, 3); pass layouts= to say otherwise)
    if layout not in ("chw", "hwc") or p.shape[0 if layout == "chw" else 2] != 3:
        raise ValueError(f"compose_frame: layout {layout!r} does not fit a panel of shape {tuple(p.shape)}")
    if layout == "hwc":
        return int(p.shape[0]), int(p.shape[1]), 1, p.contiguous()
    if not p.is_contiguous() and p.permute(1, 2, 0).is_contiguous():
        return int(p.shape[1]), int(p.shape[2]), 1, p.permute(1, 2, 0)
    return int(p.shape[1]), int(p.shape[2]), 0, p.contiguous()


def _need_contig_or_view(p):
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise RuntimeError("compose_frame: every panel must be a CUDA/HIP tensor (dg-mesh_amd has no CPU path)")
    if p.dtype != torch.float32:
        raise RuntimeError(f"compose_frame: every panel must be torch.float32, got {p.dtype}")


def compose_frame(panels, downsample=1, out=None, layouts=None):
    """Up to four fp32 panels of one size, each (3, H, W) or (H, W, 3), side by side as one uint8 frame (H/d, n W/d, 3) with
    d = downsample (1 or 2; module docstring for the arithmetic), in one launch.  out: a contiguous uint8 tensor of that shape to
    write into (the drivers pass a row of their frame buffer).  layouts: "chw" / "hwc" per panel when the shape is ambiguous.
    ValueError: no or more than four panels, panels of different sizes, d = 2 with an odd H or W."""
    panels = list(panels)
    if not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError(f"compose_frame: 1 to {MAX_PANELS} panels, got {len(panels)}")
    d = int(downsample)
    if d not in (1, 2):
        raise ValueError(f"compose_frame: downsample must be 1 or 2, got {downsample}")
    layouts = [None] * len(panels) if layouts is None else list(layouts)
    if len(layouts) != len(panels):
        raise ValueError("compose_frame: one layout per panel")
    for p in panels:
        _need_contig_or_view(p)
    info = [_panel_layout(p, lay) for p, lay in zip(panels, layouts)]
    H, W = info[0][:2]
    if any(i[:2] != (H, W) for i in info):
        raise ValueError(f"compose_frame: panels differ in size: {[i[:2] for i in info]}")
    if any(i[3].device != info[0][3].device for i in info):
        raise RuntimeError("compose_frame: panels must be on one device")
    if d == 2 and (H % 2 or W % 2):
        raise ValueError(f"compose_frame: downsample 2 needs even H and W, got {(H, W)}")
    dev = info[0][3].device
    shape = (H // d, len(panels) * (W // d), 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
              and out.device == dev):
        raise RuntimeError(f"compose_frame: out must be a contiguous uint8 tensor {shape} on the panels' device")
    ptrs = (ctypes.c_void_p * len(panels))(*[i[3].data_ptr() for i in info])
    lay = (ctypes.c_int * len(panels))(*[i[2] for i in info])
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().dgm_compose_frame(len(panels), ptrs, lay, H, W, d, _lib.vp(out), _st()))
    return out


# ---- cameras (host side, numpy) ------------------------------------------------------------------------------------------------------
def trajectory_poses(radius, elevation, total_frames, look_at=(0.0, 0.0, 0.0)):
    """get_camera_trajectory_pose / compute_pose_matrix of R/utils/camera_utils.py:121-148: (n, 4, 4) float64 OpenGL camera-to-world
    matrices, columns right, up, -forward, eye; eye_i = (r sin th, -r cos th, elevation), r = sqrt(radius^2 - elevation^2),
    th = 2 pi i / n; up is world z.  ValueError when radius <= |elevation| (the orbit has no radius)."""
    radius, elevation, n = float(radius), float(elevation), int(total_frames)
    if not radius > abs(elevation):
        raise ValueError(f"trajectory: radius {radius} must exceed |elevation| {abs(elevation)}")
    if n < 1:
        raise ValueError(f"trajectory: total_frames must be >= 1, got {total_frames}")
    target = np.asarray(look_at, np.float64).reshape(3)
    r = np.sqrt(radius ** 2 - elevation ** 2)
    poses = np.zeros((n, 4, 4), np.float64)
    for i in range(n):
        theta = 2 * np.pi * i / n
        eye = np.array([r * np.sin(theta), -r * np.cos(theta), elevation], np.float64)
        fwd = target - eye
        fwd = fwd / np.linalg.norm(fwd)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right = right / np.linalg.norm(right)
        up = np.cross(right, fwd)
        up = up / np.linalg.norm(up)
        poses[i, :3, 0], poses[i, :3, 1], poses[i, :3, 2], poses[i, :3, 3] = right, up, -fwd, eye
        poses[i, 3, 3] = 1.0
    return poses


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def camera_from_pose(c2w_gl, template_cam, fid=None):
    """A camera at the OpenGL camera-to-world pose `c2w_gl` (4, 4) (columns right, up, -forward, eye) with `template_cam`'s image
    size and projection: world_view_transform = W2C^T with the +x right, +y down, +z forward camera axes of this project,
    full_proj_transform = W2C^T P^T with P^T recovered from the template (inverse(world_view_transform) full_proj_transform, so a
    template built from an off-centre K keeps its principal point), camera_center = the eye.  fid: the camera's time (None: the
    template's).  A template with device tensors (scene.TorchCamera) gives a TorchCamera on its device -- without its images --,
    a numpy one (synthetic.Camera) a synthetic.Camera."""
    from .scene import TorchCamera
    from .synthetic import Camera
    c2w = np.array(c2w_gl, np.float64).reshape(4, 4)
    c2w[:3, 1:3] *= -1.0  # OpenGL (up, -forward) -> (down, forward)
    wvt = np.linalg.inv(c2w).T
    t_wvt, t_full = _host(template_cam.world_view_transform).astype(np.float64), _host(template_cam.full_proj_transform).astype(np.float64)
    proj_t = np.linalg.inv(t_wvt) @ t_full
    if fid is None:
        fid = float(_host(template_cam.fid).reshape(-1)[0])
    cam = Camera(int(template_cam.image_width), int(template_cam.image_height), float(template_cam.FoVx), float(template_cam.FoVy),
                 np.ascontiguousarray(wvt, np.float32), np.ascontiguousarray(wvt @ proj_t, np.float32),
                 np.ascontiguousarray(c2w[:3, 3], np.float32), float(fid))
    if isinstance(template_cam.world_view_transform, torch.Tensor):
        return TorchCamera(cam, template_cam.world_view_transform.device)
    return cam


def trajectory_cameras(radius, elevation, total_frames, template_cam, look_at=(0.0, 0.0, 0.0)):
    """The orbit of render_trajectory.py: camera i at trajectory_poses(...)[i] with the template's intrinsics and
    fid = i / total_frames."""
    poses = trajectory_poses(radius, elevation, total_frames, look_at)
    return [camera_from_pose(p, template_cam, fid=i / int(total_frames)) for i, p in enumerate(poses)]


# ---- drivers -----------------------------------------------------------------------------------------------------------------------
def _deformations(gaussians, deform, deform_normal, fid):
    xyz = gaussians.get_xyz.detach()
    time_input = fid.reshape(1, 1).expand(xyz.shape[0], -1)
    d_xyz = deform.step(xyz, time_input)[0]
    d_normal = deform_normal.step(xyz, time_input)
    if isinstance(d_normal, (tuple, list)):
        d_normal = d_normal[0]
    return xyz, d_xyz, d_normal


def _mesh_panels(who, gaussians, deform, deform_back, deform_normal, mesh, cam, white_background):
    """One frame's mesh work: the deformations at the camera's fid, the DiffMC mesh and its colours, ONE rasterize, the mesh image
    (3, H, W) and the shape image (H, W, 3) from that buffer; also the deformed Gaussian centres."""
    from .evaluate import mesh_and_colors
    xyz, d_xyz, d_normal = _deformations(gaussians, deform, deform_normal, cam.fid)
    verts, faces, vtx_color = mesh_and_colors(mesh, gaussians, deform_back, d_xyz, d_normal, cam.fid, who=who)
    verts, faces = verts.contiguous(), faces.contiguous()
    H, W = int(cam.image_height), int(cam.image_width)
    rast, _ = rasterize(None, clip_positions(cam, verts), faces, (H, W))
    mesh_image = render_mesh(None, verts, faces, vtx_color, cam, whitebackground=white_background, rast=rast)
    background = (1.0, 1.0, 1.0) if white_background else (0.0, 0.0, 0.0)
    shape_image = mesh_shape_renderer(verts, faces, cam, rast=rast, background=background)
    return mesh_image, shape_image, xyz + d_xyz


def _prepare(who, gaussians, mesh, deform_normal, cameras):
    if mesh is None or mesh.dpsr is None:
        raise RuntimeError(f"{who}: mesh must be a MeshPhase with a DPSR module")
    cameras = list(cameras)
    if not cameras:
        raise ValueError(f"{who}: no cameras")
    H, W = int(cameras[0].image_height), int(cameras[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cameras):
        raise ValueError(f"{who}: every camera must have the first one's image size {(H, W)}")
    return cameras, (mesh.deform_normal if deform_normal is None else deform_normal), H, W


def _finish(frames, dev, t0, out_dir):
    torch.cuda.synchronize(dev)
    total = time.perf_counter() - t0
    host = frames.cpu().numpy()  # the one read-back
    if out_dir is not None:
        from .png_io import write_png
        for idx, frame in enumerate(host):
            write_png(os.path.join(out_dir, "images", f"{idx:04d}.png"), frame)
    return {"frames": host, "time_per_frame": total / len(host), "fps": len(host) / total}


@torch.no_grad()
def render_test(gaussians, deform, deform_back, cameras, *, mesh, deform_normal=None, white_background=True, downsample=2,
                out_dir=None):
    """render_test.py:92-143 of the reference.  Per test camera: the deformations at its fid, mesh.psr -> mesh.surface, the vertex
    colours, one rasterize, the mesh image and the shape image, composed as [ground truth | mesh | shape] (cam.original_image is the
    ground truth) and halved by `downsample` = 2.  mesh: a trainer.MeshPhase with a DPSR module; deform_normal: None =
    mesh.deform_normal.  -> {"frames": (n, H/d, 3 W/d, 3) uint8 numpy array, "time_per_frame": seconds, "fps": frames per second}
    (wall time of the loop with one synchronisation at its end).  out_dir: also writes images/{idx:04d}.png (png_io.write_png)."""
    who = "render_test"
    cameras, deform_normal, H, W = _prepare(who, gaussians, mesh, deform_normal, cameras)
    if any(c.original_image is None for c in cameras):
        raise ValueError(f"{who}: every camera needs its original_image (the ground-truth panel)")
    d = int(downsample)
    if d not in (1, 2) or (d == 2 and (H % 2 or W % 2)):
        raise ValueError(f"{who}: downsample must be 1, or 2 with even H and W; got {downsample} at {(H, W)}")
    dev = gaussians.get_xyz.device
    frames = torch.empty((len(cameras), H // d, 3 * (W // d), 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for idx, cam in enumerate(cameras):
        mesh_image, shape_image, _ = _mesh_panels(who, gaussians, deform, deform_back, deform_normal, mesh, cam, white_background)
        compose_frame([cam.original_image, mesh_image, shape_image], d, out=frames[idx])
    return _finish(frames, dev, t0, out_dir)


@torch.no_grad()
def render_trajectory(gaussians, deform, deform_back, template_cam, *, mesh, deform_normal=None, white_background=True, radius=4.0,
                      elevation=1.0, total_frames=100, look_at=(0.0, 0.0, 0.0), point_size=1, out_dir=None):
    """render_trajectory.py:111-157 of the reference: an orbit of `total_frames` cameras (trajectory_cameras: the template's
    intrinsics, fid = i / total_frames), each frame [mesh | shape | point cloud of the deformed Gaussians] at full size.
    -> as render_test, frames (n, H, 3 W, 3)."""
    who = "render_trajectory"
    cameras = trajectory_cameras(radius, elevation, total_frames, template_cam, look_at)
    cameras, deform_normal, H, W = _prepare(who, gaussians, mesh, deform_normal, cameras)
    dev = gaussians.get_xyz.device
    frames = torch.empty((len(cameras), H, 3 * W, 3), dtype=torch.uint8, device=dev)
    background = (1.0, 1.0, 1.0) if white_background else (0.0, 0.0, 0.0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for idx, cam in enumerate(cameras):
        mesh_image, shape_image, points = _mesh_panels(who, gaussians, deform, deform_back, deform_normal, mesh, cam, white_background)
        cloud = pointcloud_renderer(points.contiguous(), cam, size=point_size, background=background)
        compose_frame([mesh_image, shape_image, cloud], 1, out=frames[idx])
    return _finish(frames, dev, t0, out_dir)


@torch.no_grad()
def export_dynamic_mesh(gaussians, deform, deform_back, mesh, out_dir, frames=200, deform_normal=None, clean=None, simplify=None, smooth=None,
                        repair=None, texture=None):
    """The dynamic-mesh sequence of R/train.py:389-423: dynamic_mesh/frame_{i}.ply under out_dir for t = i / frames, i < frames,
    with vertex colours (ply_io.write_mesh_ply).  Colours are written as clamp(c, 0, 1) * 255 truncated, as testing() writes them;
    the reference's astype(np.uint8) of the unscaled [0, 1] colours at this place is a bug (every channel becomes 0 or 1).
    The four stages of mesh_post, each None or its spec (or a dict of its fields), change each written mesh, its colours following
    their vertices (mesh_post) -- clean: a mesh_clean.CleanSpec, first.  simplify: a mesh_simplify.SimplifySpec, after `clean`.
    smooth: a mesh_smooth.SmoothSpec, after `clean` and BEFORE `simplify`.  repair: a mesh_repair.RepairSpec, LAST, after
    `simplify`.  texture: None, or a
    mesh_texture.TextureSpec (or a dict of its fields): every frame ALSO gets dynamic_mesh_textured/frame_{i}.obj (+ .mtl, .png) or
    .glb, the written mesh with a texture atlas baked after mesh_post from the appearance network itself (mesh_texture.bake with appearance_color_fn at the frame's time), not from the
    decimated vertex colours; with ao_samples > 0 the texture is multiplied by the baked ambient occlusion
    (mesh_texture.bake_ambient_occlusion); the PLY files are what they are without it.  -> the list of the PLY paths."""
    from . import mesh_post, mesh_texture
    from .evaluate import mesh_and_colors
    from .ply_io import write_mesh_ply
    who = "export_dynamic_mesh"
    if mesh is None or mesh.dpsr is None:
        raise RuntimeError(f"{who}: mesh must be a MeshPhase with a DPSR module")
    n = int(frames)
    if n < 1:
        raise ValueError(f"{who}: frames must be >= 1, got {frames}")
    if deform_normal is None:
        deform_normal = mesh.deform_normal
    tex_spec = mesh_texture.as_spec(texture)
    dev = gaussians.get_xyz.device
    paths = []
    for i in range(n):
        fid = torch.tensor([i / n], dtype=torch.float32, device=dev)
        _, d_xyz, d_normal = _deformations(gaussians, deform, deform_normal, fid)
        verts, faces, vtx_color = mesh_post.apply(*mesh_and_colors(mesh, gaussians, deform_back, d_xyz, d_normal, fid, who=who),
                                                  clean=clean, smooth=smooth, simplify=simplify, repair=repair)
        paths.append(os.path.join(out_dir, "dynamic_mesh", f"frame_{i}.ply"))
        write_mesh_ply(paths[-1], verts, faces, vertex_colors=vtx_color)
        if tex_spec is not None:
            tex, uv, _ = mesh_texture.bake(verts.contiguous(), faces.contiguous(), mesh_texture.appearance_color_fn(mesh, deform_back, fid),
                                           **tex_spec.atlas_args())
            tex = mesh_texture.apply_ambient_occlusion(tex, verts.contiguous(), faces.contiguous(), tex_spec, **tex_spec.atlas_args())
            mesh_texture.write_textured(os.path.join(out_dir, "dynamic_mesh_textured", f"frame_{i}"), tex_spec.format, verts, faces, uv, tex)
    return paths
