"""Mesh correspondence across time: which point of frame t's surface is which point of the reference frame's.  The reference's README
promises a "time-consistent mesh" and "the mesh vertice motion across time frames" and lists "Mesh correspondence visualization" as
an open item; there is nothing in it to port.  The link between frames runs through the canonical space: deform_back takes a point at
time t to canonical, deform takes a canonical point to any time.  A vertex of mesh(t_a) carried that way to t_b lands near
mesh(t_b), not on it; closest_on_mesh puts it on that surface as (face, barycentrics) -- the exact closest point on a triangle mesh
(csrc/surface.hip: dgm_surf_closest, dgm_surf_interp, dgm_corr_palette).

  closest_on_mesh / interpolate / palette   the three kernels
  to_canonical / advect / transport         the two networks, any object with .step(xyz, time_rows) whose first output is the offset
  correspond                                transport, closest_on_mesh, interpolate
  render_correspondence                     an orbit of frames [mesh image | correspondence-coloured mesh | tracked points]
  export_correspondence                     correspondence/frame_{i}.ply, tracks.npz, report.json

Colouring modes of the drivers: "canonical" colours a frame's vertices by the palette of their canonical positions; "reference"
carries every vertex to t_ref, snaps it onto mesh(t_ref) and colours it by the palette of that SURFACE POINT's canonical position, so
every frame wears the reference frame's texture and sliding shows; unmatched vertices take the lost colour (1, 0, 1).  Both drivers
return and write the per-frame table of the snap: n_queries, n_found, mean and max distance in world units and in voxels
(voxel = 2 gaussian_scale / grid_res) -- how far the transported surface of frame t lies from the reference surface.  sqrt(d2) is
summed in fp64 on the device and the table is read back once, after the last frame.

float32 CUDA/HIP tensors only -- no CPU fallback; anything else raises.
"""
import json
import math
import os
import time

import numpy as np
import torch

from . import _lib

MODES = ("reference", "canonical")
PALETTES = {"rgb": 0, "checker": 1}
LOST_COLOR = (1.0, 0.0, 1.0)
COLUMNS = ("n_queries", "n_found", "mean_dist", "max_dist", "mean_dist_voxels", "max_dist_voxels")


def _need(name, t, what, dtype, shape_tail=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"correspondence.{name}: {what} must be a CUDA/HIP tensor (dg-mesh_amd has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"correspondence.{name}: {what} must be {dtype}, got {t.dtype}")
    if shape_tail is not None and (t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail)):
        raise ValueError(f"correspondence.{name}: {what} must be (n, {', '.join(str(s) for s in shape_tail)}), got {tuple(t.shape)}")


def _same_device(name, first, *rest):
    for t in rest:
        if t.device != first.device:
            raise ValueError(f"correspondence.{name}: tensors on {first.device} and {t.device}")


def max_d2_of(max_dist):
    """The kernel's strict bound on the squared distance: fp32(max_dist * max_dist) (+inf for an unbounded search)."""
    max_dist = float(max_dist)
    if math.isnan(max_dist) or max_dist < 0:
        raise ValueError(f"correspondence: max_dist must be >= 0, got {max_dist}")
    return math.inf if math.isinf(max_dist) else float(np.float32(max_dist * max_dist))


def closest_on_mesh(points, verts, faces, max_dist=math.inf):
    """The closest point of the mesh (verts (V, 3) fp32, faces (F, 3) int32) to every row of points (N, 3) fp32:
    (face (N,) int32, d2 (N,) fp32 squared distance, bary (N, 3) fp32 = (1 - v - w, v, w)); only faces with d2 < fp32(max_dist^2)
    (strict) count, and a query without one gets face -1, d2 +inf, bary 0.  Exact in the sense of csrc/surface.hip's fp32 statement,
    ties to the smaller face index, bit-reproducible.  A finite max_dist searches a grid over the faces; inf is a brute force."""
    name = "closest_on_mesh"
    max_d2 = max_d2_of(max_dist)
    _need(name, points, "points", torch.float32, (3,))
    _need(name, verts, "verts", torch.float32, (3,))
    _need(name, faces, "faces", torch.int32, (3,))
    _same_device(name, points, verts, faces)
    p, v, f = points.detach().contiguous(), verts.detach().contiguous(), faces.contiguous()
    N, V, F = p.shape[0], v.shape[0], f.shape[0]
    dev = p.device
    L = _lib.lib()
    face = torch.empty(N, dtype=torch.int32, device=dev)
    d2 = torch.empty(N, dtype=torch.float32, device=dev)
    bary = torch.empty((N, 3), dtype=torch.float32, device=dev)
    scratch = None
    if not math.isinf(max_d2):
        scratch = _lib.scratch(L.dgm_surf_closest_scratch_bytes(N, F), dev)
    with _lib.device_guard(dev):
        _lib.check(L.dgm_surf_closest(N, V, F, _lib.vp(p), _lib.vp(v), _lib.vp(f), max_d2, _lib.vp(scratch), _lib.vp(face), _lib.vp(d2), _lib.vp(bary),
                                      _lib.stream_ptr()))
    return face, d2, bary


def interpolate(attr, faces, face, bary, fill=math.nan):
    """attr (V, C) or (V,) fp32 at the surface points (face (N,) int32, bary (N, 3) fp32) of the mesh with `faces`:
    (attr[i0] b0 + attr[i1] b1) + attr[i2] b2; a row with face < 0 is `fill`.  attr = verts gives the closest points themselves."""
    name = "interpolate"
    _need(name, attr, "attr", torch.float32)
    _need(name, faces, "faces", torch.int32, (3,))
    _need(name, face, "face", torch.int32, ())
    _need(name, bary, "bary", torch.float32, (3,))
    _same_device(name, attr, faces, face, bary)
    if attr.dim() not in (1, 2):
        raise ValueError(f"correspondence.{name}: attr must be (V,) or (V, C), got {tuple(attr.shape)}")
    if bary.shape[0] != face.shape[0]:
        raise ValueError(f"correspondence.{name}: {face.shape[0]} faces but {bary.shape[0]} barycentric rows")
    a = attr.detach().contiguous()
    V, C, N, F = a.shape[0], (a.shape[1] if a.dim() == 2 else 1), face.shape[0], faces.shape[0]
    if C < 1:
        raise ValueError(f"correspondence.{name}: attr needs at least one channel")
    out = torch.empty((N, C) if a.dim() == 2 else (N,), dtype=torch.float32, device=a.device)
    with _lib.device_guard(a.device):
        _lib.check(_lib.lib().dgm_surf_interp(N, V, F, C, _lib.vp(a), _lib.vp(faces.contiguous()), _lib.vp(face.contiguous()),
                                              _lib.vp(bary.detach().contiguous()), float(fill), _lib.vp(out), _lib.stream_ptr()))
    return out


def _palette_mode(name, mode, cells):
    if mode not in PALETTES:
        raise ValueError(f"correspondence.{name}: mode must be one of {sorted(PALETTES)}, got {mode!r}")
    cells = int(cells)
    if not 1 <= cells <= 4096:
        raise ValueError(f"correspondence.{name}: cells must be within [1, 4096], got {cells}")
    return PALETTES[mode], cells


def palette(xyz, center, scale, mode="rgb", cells=8):
    """The colour (N, 3) of canonical positions xyz (N, 3): u = clamp(((x - center) / scale) 0.5 + 0.5, 0, 1) per axis -- the unit
    cube of the DPSR grid when center / scale are the Gaussian model's --; "rgb": u; "checker": u, times 0.55 in every other cell of a
    cells^3 checkerboard.  A row with a NaN is the lost colour (1, 0, 1).  center: 3 numbers or a device tensor, scale: a number or a
    one-element device tensor (device tensors are read on the device)."""
    name = "palette"
    m, cells = _palette_mode(name, mode, cells)
    _need(name, xyz, "xyz", torch.float32, (3,))
    dev = xyz.device
    c = torch.as_tensor(center, dtype=torch.float32).to(dev).reshape(-1).contiguous()
    s = torch.as_tensor(scale, dtype=torch.float32).to(dev).reshape(-1).contiguous()
    if c.numel() != 3 or s.numel() != 1:
        raise ValueError(f"correspondence.{name}: center must have three components and scale one")
    x = xyz.detach().contiguous()
    out = torch.empty_like(x)
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().dgm_corr_palette(x.shape[0], _lib.vp(x), _lib.vp(c), _lib.vp(s), m, cells, _lib.vp(out), _lib.stream_ptr()))
    return out


# ---- the two networks ---------------------------------------------------------------------------------------------------------------
def _time_rows(t, N, dev):
    """(N, 1) as an expanded view of one element, so that the HIP MLP takes its one-row time branch."""
    return torch.as_tensor(t, dtype=torch.float32).to(dev).reshape(-1)[:1].reshape(1, 1).expand(N, -1)


def _offset(name, net, x, t):
    _need(name, x, "points", torch.float32, (3,))
    if x.shape[0] == 0:
        return x
    return x + net.step(x, _time_rows(t, x.shape[0], x.device))[0]


def to_canonical(points, t, deform_back):
    """points (N, 3) at time t -> their canonical positions: points + deform_back.step(points, t)[0]."""
    return _offset("to_canonical", deform_back, points, t)


def advect(canonical, t, deform):
    """canonical positions (N, 3) -> time t: canonical + deform.step(canonical, t)[0]."""
    return _offset("advect", deform, canonical, t)


def transport(points, t_from, t_to, deform, deform_back):
    """points (N, 3) of time t_from carried to time t_to through the canonical space."""
    return advect(to_canonical(points, t_from, deform_back), t_to, deform)


def correspond(points, t_from, verts_to, faces_to, t_to, deform, deform_back, max_dist=math.inf):
    """Where the points (N, 3) of time t_from are on the mesh of time t_to: {"position_free": the transported points, "face", "d2",
    "bary": closest_on_mesh of them, "position": that surface point (interpolate(verts_to, ...))}.  A query with no face within
    max_dist has face -1 and a NaN position."""
    free = transport(points, t_from, t_to, deform, deform_back).contiguous()
    face, d2, bary = closest_on_mesh(free, verts_to, faces_to, max_dist)
    return {"position_free": free, "face": face, "bary": bary, "d2": d2, "position": interpolate(verts_to, faces_to, face, bary)}


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
def _check_options(who, mode, palette_name, n_tracks, cells):
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {MODES}, got {mode!r}")
    _palette_mode(who, palette_name, cells)
    if int(n_tracks) < 1:
        raise ValueError(f"{who}: n_tracks must be >= 1, got {n_tracks}")


class _Tracker:
    """The state both drivers share: mesh(t_ref), the tracked points and their colours, the track tensor and the snap table."""

    def __init__(self, who, gaussians, deform, deform_back, mesh, deform_normal, n_frames, t_ref, mode, palette_name, max_dist, n_tracks,
                 seed, cells):
        from . import normal_init
        from .evaluate import mesh_and_colors
        from .visualize import _deformations
        self.who, self.g, self.deform, self.deform_back, self.mesh, self.deform_normal = who, gaussians, deform, deform_back, mesh, deform_normal
        self.mode, self.palette_name, self.cells = mode, palette_name, int(cells)
        dev = gaussians.get_xyz.device
        self.dev = dev
        self.t_ref = torch.tensor([float(t_ref)], dtype=torch.float32, device=dev)
        _, d_xyz, d_normal = _deformations(gaussians, deform, deform_normal, self.t_ref)
        psr = mesh.psr(gaussians, d_xyz, d_normal)
        self.grid_res = int(psr.shape[0])
        verts, faces = mesh.surface(gaussians, psr)
        if verts.shape[0] == 0:
            raise RuntimeError(f"{who}: the DPSR field has no surface at t_ref = {float(t_ref)} (DiffMC returned no vertices)")
        self.ref_verts, self.ref_faces = verts.contiguous(), faces.contiguous()
        # the one read before the loop: the search bound is an argument of the kernel
        self.voxel = 2.0 * float(torch.as_tensor(gaussians.gaussian_scale).reshape(-1)[0]) / self.grid_res
        self.max_dist = 4.0 * self.voxel if max_dist is None else float(max_dist)
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        self.track_ref, _ = normal_init.sample_surface(self.ref_verts, self.ref_faces, int(n_tracks), generator=gen)
        self.track_color = self.color_of(to_canonical(self.track_ref, self.t_ref, deform_back))
        self.tracks = torch.full((n_frames, int(n_tracks), 3), math.nan, dtype=torch.float32, device=dev)
        self.table = torch.zeros((n_frames, 4), dtype=torch.float64, device=dev)  # n_queries, n_found, sum, max
        self._mesh_and_colors, self._deformations = mesh_and_colors, _deformations

    def color_of(self, canonical):
        return palette(canonical, self.g.gaussian_center, self.g.gaussian_scale, self.palette_name, self.cells)

    def frame(self, idx, fid):
        """One frame at time fid (a one-element device tensor): (verts, faces, vtx_color, correspondence colours, tracked points)."""
        _, d_xyz, d_normal = self._deformations(self.g, self.deform, self.deform_normal, fid)
        verts, faces, vtx_color = self._mesh_and_colors(self.mesh, self.g, self.deform_back, d_xyz, d_normal, fid, who=self.who)
        verts, faces = verts.contiguous(), faces.contiguous()
        snap = correspond(verts, fid, self.ref_verts, self.ref_faces, self.t_ref, self.deform, self.deform_back, self.max_dist)
        found = snap["face"] >= 0
        dist = torch.where(found, snap["d2"].double().sqrt(), torch.zeros((), dtype=torch.float64, device=self.dev))
        row = self.table[idx]
        row[0] = verts.shape[0]
        row[1] = found.sum()
        row[2] = dist.sum()
        row[3] = dist.max()
        if self.mode == "reference":
            corr_color = self.color_of(to_canonical(snap["position"], self.t_ref, self.deform_back))
        else:
            corr_color = self.color_of(to_canonical(verts, fid, self.deform_back))
        self.tracks[idx] = correspond(self.track_ref, self.t_ref, verts, faces, fid, self.deform, self.deform_back, self.max_dist)["position"]
        return verts, faces, vtx_color, corr_color, self.tracks[idx]

    def report(self, times):
        """The snap table (its one read-back) as {"frames": [...], ...}."""
        tab = self.table.cpu().numpy()
        rows = []
        for t, (nq, nf, s, mx) in zip(times, tab):
            mean = s / nf if nf > 0 else math.nan
            mx = mx if nf > 0 else math.nan
            rows.append({"t": float(t), "n_queries": int(nq), "n_found": int(nf), "mean_dist": float(mean), "max_dist": float(mx),
                         "mean_dist_voxels": float(mean / self.voxel), "max_dist_voxels": float(mx / self.voxel)})
        return {"frames": rows, "columns": list(COLUMNS), "t_ref": float(self.t_ref[0]), "mode": self.mode, "palette": self.palette_name,
                "search_dist": self.max_dist, "voxel": self.voxel, "grid_res": self.grid_res, "n_tracks": int(self.tracks.shape[1]),
                "ref_verts": int(self.ref_verts.shape[0]), "ref_faces": int(self.ref_faces.shape[0])}


def _write_report(out_dir, report):
    path = os.path.join(out_dir, "correspondence", "report.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)
    return path


@torch.no_grad()
def render_correspondence(gaussians, deform, deform_back, template_cam, *, mesh, deform_normal=None, white_background=True, radius=4.0,
                          elevation=1.0, total_frames=100, look_at=(0.0, 0.0, 0.0), point_size=3, out_dir=None, t_ref=0.0,
                          mode="reference", palette="checker", max_dist=None, n_tracks=2048, seed=0, cells=8):
    """visualize.render_trajectory's orbit (the template's intrinsics, fid = i / total_frames) with the frames
    [mesh image | the mesh in its correspondence colours | the tracked points], full size.  The tracked points are n_tracks samples
    of mesh(t_ref) (normal_init.sample_surface, a device generator seeded with `seed`), carried to every frame and snapped onto its
    mesh, drawn as dots of `point_size` pixels in the palette colour of their canonical position.  max_dist: the search bound of
    every snap in world units, None = 4 voxels.  -> as render_trajectory ({"frames": (n, H, 3 W, 3) uint8, "time_per_frame",
    "fps"}) plus "report" (module docstring) and "tracks" (n, n_tracks, 3) float32 with NaN where a track found no surface.
    out_dir: also writes images/{idx:04d}.png and correspondence/report.json."""
    from . import visualize as VZ
    from .mesh_raster import clip_positions, rasterize, render_mesh
    who = "render_correspondence"
    _check_options(who, mode, palette, n_tracks, cells)
    cameras = VZ.trajectory_cameras(radius, elevation, total_frames, template_cam, look_at)
    cameras, deform_normal, H, W = VZ._prepare(who, gaussians, mesh, deform_normal, cameras)
    dev = gaussians.get_xyz.device
    tr = _Tracker(who, gaussians, deform, deform_back, mesh, deform_normal, len(cameras), t_ref, mode, palette, max_dist, n_tracks, seed, cells)
    frames = torch.empty((len(cameras), H, 3 * W, 3), dtype=torch.uint8, device=dev)
    background = (1.0, 1.0, 1.0) if white_background else (0.0, 0.0, 0.0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for idx, cam in enumerate(cameras):
        verts, faces, vtx_color, corr_color, points = tr.frame(idx, cam.fid)
        rast, _ = rasterize(None, clip_positions(cam, verts), faces, (H, W))
        mesh_image = render_mesh(None, verts, faces, vtx_color, cam, whitebackground=white_background, rast=rast)
        corr_image = render_mesh(None, verts, faces, corr_color, cam, whitebackground=white_background, rast=rast)
        dots = VZ.pointcloud_renderer(points.contiguous(), cam, colors=tr.track_color, size=point_size, background=background)
        VZ.compose_frame([mesh_image, corr_image, dots], 1, out=frames[idx])
    res = VZ._finish(frames, dev, t0, out_dir)
    res["report"] = tr.report([i / len(cameras) for i in range(len(cameras))])
    res["tracks"] = tr.tracks.cpu().numpy()
    if out_dir is not None:
        _write_report(out_dir, res["report"])
    return res


@torch.no_grad()
def export_correspondence(gaussians, deform, deform_back, mesh, out_dir, frames=200, deform_normal=None, clean=None, simplify=None,
                          smooth=None, repair=None, *, t_ref=0.0, mode="reference", palette="checker", max_dist=None, n_tracks=2048, seed=0, cells=8):
    """visualize.export_dynamic_mesh's sequence (t = i / frames) with the correspondence on it, under out_dir/correspondence:
    frame_{i}.ply -- the mesh of frame i in its correspondence colours (ply_io.write_mesh_ply) --, tracks.npz -- tracks
    (T, K, 3) float32 with NaN where unmatched, found (T, K) bool, times (T,) -- and report.json (module docstring).  The four stages of
    mesh_post, each None or its spec (or a dict of its fields), change the WRITTEN meshes only, the colours following their vertices
    (mesh_post); the snap and the tracks use the full meshes -- clean: a mesh_clean.CleanSpec, first.  simplify: a
    mesh_simplify.SimplifySpec, after `clean`.  smooth: a mesh_smooth.SmoothSpec, after `clean` and BEFORE `simplify`.  repair: a
    mesh_repair.RepairSpec, LAST, after `simplify`.
    ->{"paths": [...], "tracks_path", "report_path", "report", "tracks", "found", "times"}."""
    from . import mesh_post
    from .ply_io import write_mesh_ply
    who = "export_correspondence"
    _check_options(who, mode, palette, n_tracks, cells)
    if mesh is None or mesh.dpsr is None:
        raise RuntimeError(f"{who}: mesh must be a MeshPhase with a DPSR module")
    n = int(frames)
    if n < 1:
        raise ValueError(f"{who}: frames must be >= 1, got {frames}")
    if deform_normal is None:
        deform_normal = mesh.deform_normal
    dev = gaussians.get_xyz.device
    tr = _Tracker(who, gaussians, deform, deform_back, mesh, deform_normal, n, t_ref, mode, palette, max_dist, n_tracks, seed, cells)
    paths = []
    for i in range(n):
        fid = torch.tensor([i / n], dtype=torch.float32, device=dev)
        verts, faces, _, corr_color, _ = tr.frame(i, fid)
        verts, faces, corr_color = mesh_post.apply(verts, faces, corr_color, clean=clean, smooth=smooth, simplify=simplify, repair=repair)
        paths.append(os.path.join(out_dir, "correspondence", f"frame_{i}.ply"))
        write_mesh_ply(paths[-1], verts, faces, vertex_colors=corr_color)
    times = np.arange(n, dtype=np.float32) / np.float32(n)
    report = tr.report(times)
    tracks = tr.tracks.cpu().numpy()
    found = ~np.isnan(tracks).any(-1)
    tracks_path = os.path.join(out_dir, "correspondence", "tracks.npz")
    os.makedirs(os.path.dirname(tracks_path), exist_ok=True)
    np.savez(tracks_path, tracks=tracks, found=found, times=times)
    return {"paths": paths, "tracks_path": tracks_path, "report_path": _write_report(out_dir, report), "report": report,
            "tracks": tracks, "found": found, "times": times}
