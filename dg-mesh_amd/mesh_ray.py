"""Ray casting against a triangle mesh on the device: what a ray hits first, whether it hits anything, and what rests on that --
visibility between points, a depth map by rays, ambient occlusion at points, at vertices and (mesh_texture.bake_ambient_occlusion)
per texel (csrc/mesh_ray.hip: dgm_ray_build, dgm_ray_cast, dgm_ray_occluded; include/dgmesh_hip.h states the pair test and the
answer).  The reference has no counterpart: it renders by rasterisation only.

  RayMesh                   the acceleration structure of a mesh, built once and held
  ray_cast                  (face, t, bary) of the nearest hit per ray: face -1, t +inf, bary 0 for a miss
  occluded                  bool per ray: some face is hit with t_min <= t < t_max
  hit_points                origin + t dir (NaN for a miss)
  visible                   no face between a point and an eye
  camera_rays, depth_map    pixel-centre rays of a camera; view-space depth (H, W) by rays, +inf on the background, and the face ids
  ambient_occlusion         the share of unoccluded cosine-weighted hemisphere rays about a normal, in [0, 1]
  vertex_ambient_occlusion  the same at the vertices, with visualize.vertex_normals

The pair test is watertight: no ray slips between two faces that share an edge or a vertex.  The answer of a ray is the
lexicographic minimum of (t, face index) over the faces it hits, so every value is bit-reproducible, does not depend on which other
rays it is asked with, and is the same on both paths: brute force (accel=None, N x F pairs) and the structure (a RayMesh).
Directions are not normalised: t is in units of |dir|.

float32 / int32 CUDA/HIP tensors only -- no CPU fallback; anything else raises.

  python -m dgmesh_amd.mesh_ray mesh.ply --ao out.ply [--samples N] [--flip]
writes the mesh with its vertex ambient occlusion in the vertex colours: the file's colours multiplied by it, grey without any."""
import argparse
import math

import torch

from . import _lib, mesh_args

AUTO_MIN_FACES = 752       # accel="auto": the structure from this many faces on, the smallest mesh on which tools/mesh_ray_bench.py
                           # showed build + accelerated cast ahead of the brute force for one 800 x 800 cast
RAY_BATCH = 1 << 22        # rays per launch of ambient_occlusion (memory only: the result does not depend on it)


class RayMesh:
    """The acceleration structure of the mesh (verts (V, 3) fp32, faces (F, 3) int32), built once (dgm_ray_build) and held together
    with the mesh it was built from: the faces sorted by the Morton code of their centroid and one box per 256 of them.  Hand it to
    ray_cast, occluded, ... as `accel`; the answers are those of the brute force bit for bit."""

    def __init__(self, verts, faces):
        self.verts, self.faces = mesh_args.mesh("mesh_ray.RayMesh", verts, faces)
        V, F = self.verts.shape[0], self.faces.shape[0]
        L = _lib.lib()
        dev = self.verts.device
        self.accel = torch.empty(int(L.dgm_ray_accel_bytes(F)), dtype=torch.uint8, device=dev)
        with _lib.device_guard(dev):
            scratch = _lib.scratch(L.dgm_ray_build_scratch_bytes(F), dev)
            _lib.check(L.dgm_ray_build(V, F, _lib.vp(self.verts), _lib.vp(self.faces), _lib.vp(scratch), _lib.vp(self.accel), _lib.stream_ptr()))


def _resolve(name, verts, faces, accel):
    """-> verts, faces, the RayMesh to use or None (brute force)."""
    if isinstance(accel, RayMesh):
        if verts is not None and (tuple(verts.shape) != tuple(accel.verts.shape) or tuple(faces.shape) != tuple(accel.faces.shape)):
            raise ValueError(f"mesh_ray.{name}: the RayMesh was built for another mesh ({tuple(accel.verts.shape)}, {tuple(accel.faces.shape)})")
        return accel.verts, accel.faces, accel
    v, f = mesh_args.mesh(f"mesh_ray.{name}", verts, faces)
    if accel is None:
        return v, f, None
    if isinstance(accel, str) and accel == "auto":
        return v, f, (RayMesh(v, f) if f.shape[0] >= AUTO_MIN_FACES else None)
    raise TypeError(f"mesh_ray.{name}: accel must be a RayMesh, None or \"auto\", got {accel!r}")


def _accel_ptr(held):
    return _lib.vp(held.accel) if held is not None else None


def _rays(name, origins, dirs, v):
    who = f"mesh_ray.{name}"
    mesh_args.need(who, origins, "origins", torch.float32)
    mesh_args.need(who, dirs, "dirs", torch.float32)
    if origins.shape != dirs.shape:
        raise ValueError(f"{who}: origins {tuple(origins.shape)} and dirs {tuple(dirs.shape)} differ")
    mesh_args.one_device(who, ("verts", v), ("origins", origins), ("dirs", dirs))
    return origins.detach().contiguous(), dirs.detach().contiguous()


def ray_cast(origins, dirs, verts, faces, t_min=0.0, t_max=math.inf, accel="auto"):
    """The nearest hit of every ray origins + t dirs ((N, 3) fp32 each) on the mesh (verts (V, 3) fp32, faces (F, 3) int32) with
    t_min <= t < t_max: (face (N,) int32, t (N,) fp32, bary (N, 3) fp32), by the pair test and the tie rule of
    include/dgmesh_hip.h; a miss is (-1, +inf, 0).  A face with an index outside [0, V) or a non-finite corner is never hit; a ray
    with a non-finite component or a zero direction misses.  accel: a RayMesh (verts and faces may then be None), None (brute
    force, N x F pairs) or "auto" (a RayMesh built here from AUTO_MIN_FACES faces on); it changes no bit of the answer."""
    name = "ray_cast"
    v, f, acc = _resolve(name, verts, faces, accel)
    o, d = _rays(name, origins, dirs, v)
    N = o.shape[0]
    face = torch.empty(N, dtype=torch.int32, device=o.device)
    t = torch.empty(N, dtype=torch.float32, device=o.device)
    bary = torch.empty((N, 3), dtype=torch.float32, device=o.device)
    with _lib.device_guard(o.device):
        _lib.check(_lib.lib().dgm_ray_cast(N, v.shape[0], f.shape[0], _lib.vp(o), _lib.vp(d), float(t_min), float(t_max), _lib.vp(v), _lib.vp(f), _accel_ptr(acc),
                                           _lib.vp(face), _lib.vp(t), _lib.vp(bary), _lib.stream_ptr()))
    return face, t, bary


def occluded(origins, dirs, verts, faces, t_min=0.0, t_max=math.inf, accel="auto"):
    """(N,) bool: the ray hits some face with t_min <= t < t_max (= ray_cast(...)[0] >= 0; the ray stops at its first hit)."""
    name = "occluded"
    v, f, acc = _resolve(name, verts, faces, accel)
    o, d = _rays(name, origins, dirs, v)
    N = o.shape[0]
    hit = torch.empty(N, dtype=torch.uint8, device=o.device)
    with _lib.device_guard(o.device):
        _lib.check(_lib.lib().dgm_ray_occluded(N, v.shape[0], f.shape[0], _lib.vp(o), _lib.vp(d), float(t_min), float(t_max), _lib.vp(v), _lib.vp(f), _accel_ptr(acc),
                                               _lib.vp(hit), _lib.stream_ptr()))
    return hit != 0


def hit_points(origins, dirs, t):
    """origins + t dirs (N, 3); NaN where t is not finite (a miss)."""
    p = origins + t[:, None] * dirs
    return torch.where(torch.isfinite(t)[:, None], p, torch.full_like(p, math.nan))


def visible(points, eye, verts, faces, eps=1e-4, accel="auto"):
    """(N,) bool: no face is hit on the way from points (N, 3) to eye ((3,) or (N, 3)) with t in [eps, 1 - eps) along eye - point
    (eps keeps the surface a point lies on, and one the eye lies on, from hiding it)."""
    mesh_args.need("mesh_ray.visible", points, "points", torch.float32)
    eye = torch.as_tensor(eye, dtype=torch.float32).to(points.device)
    dirs = (eye.reshape(-1, 3) - points).contiguous()
    return ~occluded(points, dirs, verts, faces, float(eps), 1.0 - float(eps), accel)


def _cam_matrix(m, device):
    return torch.as_tensor(m).to(device=device, dtype=torch.float64).reshape(4, 4)


def camera_rays(camera, device=None):
    """The rays through the pixel centres of one of the project's cameras (image_width, image_height, world_view_transform,
    full_proj_transform, camera_center: scene.TorchCamera, synthetic.Camera): origins, dirs (H W, 3) fp32, pixel (px, py) at row
    py W + px, row 0 at NDC y = -1 as mesh_raster has it.  dirs have view-space depth 1, so the t of a hit is its view-space depth.
    Unprojected in fp64 through the inverse of full_proj_transform (an off-centre principal point is kept), on the device."""
    if device is None:
        m = camera.full_proj_transform
        device = m.device if isinstance(m, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mesh_ray.camera_rays needs a CUDA/HIP device (dg-mesh_amd has no CPU path)")
    H, W = int(camera.image_height), int(camera.image_width)
    full, wvt = _cam_matrix(camera.full_proj_transform, device), _cam_matrix(camera.world_view_transform, device)
    inv = torch.linalg.inv(full)
    x = (torch.arange(W, dtype=torch.float64, device=device) + 0.5) * (2.0 / W) - 1.0
    y = (torch.arange(H, dtype=torch.float64, device=device) + 0.5) * (2.0 / H) - 1.0
    yy, xx = torch.meshgrid(y, x, indexing="ij")
    ones = torch.ones_like(xx)
    unproject = lambda z: torch.stack([xx, yy, z * ones, ones], dim=-1).reshape(-1, 4) @ inv
    near, far = unproject(0.25), unproject(0.75)
    d = far[:, :3] / far[:, 3:] - near[:, :3] / near[:, 3:]
    d = d / (d @ wvt[:3, 2:3])  # view-space z of the direction -> 1
    center = torch.as_tensor(camera.camera_center).to(device=device, dtype=torch.float32).reshape(1, 3)
    return center.expand(H * W, 3).contiguous(), d.to(torch.float32).contiguous()


def depth_map(camera, verts, faces, accel="auto"):
    """(depth (H, W) fp32, face (H, W) int32): the view-space depth of the nearest face along the ray through every pixel centre
    (camera_rays), +inf and -1 on the background."""
    mesh_args.mesh("mesh_ray.depth_map", verts, faces)
    o, d = camera_rays(camera, verts.device)
    face, t, _ = ray_cast(o, d, verts, faces, 0.0, math.inf, accel)
    H, W = int(camera.image_height), int(camera.image_width)
    return t.reshape(H, W), face.reshape(H, W)


# ---- ambient occlusion ------------------------------------------------------------------------------------------------------------------
def _radical_inverse2(i):
    """The van der Corput sequence in base 2 of int64 i < 2^32, in [0, 1), fp64."""
    i = ((i & 0x55555555) << 1) | ((i >> 1) & 0x55555555)
    i = ((i & 0x33333333) << 2) | ((i >> 2) & 0x33333333)
    i = ((i & 0x0F0F0F0F) << 4) | ((i >> 4) & 0x0F0F0F0F)
    i = ((i & 0x00FF00FF) << 8) | ((i >> 8) & 0x00FF00FF)
    i = ((i & 0x0000FFFF) << 16) | ((i >> 16) & 0x0000FFFF)
    return i.double() / 4294967296.0


def _rotation(index, seed):
    """A number in [0, 1) per point from its int64 index and the seed: two rounds of a multiply-xorshift hash on 32 bits, fp64."""
    h = (index + int(seed) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    for mul in (0x85EBCA6B, 0xC2B2AE35):
        h = ((h ^ (h >> 16)) * mul) & 0xFFFFFFFF
    return (h ^ (h >> 15)).double() / 4294967296.0


def ao_directions(normals, samples, seed=0, start=0):
    """The `samples` directions (n, samples, 3) fp32 of ambient_occlusion about normals (n, 3), point k of this call counting as
    point start + k: the Hammersley set (u1, u2) = ((i + .5) / samples, radical inverse of i), cosine-weighted -- radius sqrt(u1),
    angle 2 pi (u2 + rotation(start + k, seed)), height sqrt(1 - u1) -- in the branchless orthonormal frame of Duff et al. (2017)
    about the normalised normal.  Formed in fp64 from the fp32 normals, rounded to fp32 once."""
    dev = normals.device
    n = torch.nn.functional.normalize(normals.double(), dim=1)
    i = torch.arange(int(samples), dtype=torch.int64, device=dev)
    u1 = (i.double() + 0.5) / int(samples)
    rot = _rotation(torch.arange(start, start + n.shape[0], dtype=torch.int64, device=dev), seed)
    phi = (2.0 * math.pi) * (_radical_inverse2(i)[None, :] + rot[:, None])
    r, h = torch.sqrt(u1)[None, :], torch.sqrt(1.0 - u1)[None, :]
    lx, ly = r * torch.cos(phi), r * torch.sin(phi)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sign = torch.where(nz >= 0, torch.ones_like(nz), -torch.ones_like(nz))
    a = -1.0 / (sign + nz)
    b = nx * ny * a
    tang = torch.stack([1.0 + sign * nx * nx * a, sign * b, -sign * nx], dim=1)
    bita = torch.stack([b, sign + ny * ny * a, -ny], dim=1)
    d = lx[..., None] * tang[:, None, :] + ly[..., None] * bita[:, None, :] + h[..., None] * n[:, None, :]
    return d.to(torch.float32)


def default_offset(verts):
    """1e-4 x the diagonal of the bounding box of the finite vertices, a 0-dim device tensor (0 for no vertex)."""
    if verts.shape[0] == 0:
        return torch.zeros((), dtype=torch.float32, device=verts.device)
    v = torch.where(torch.isfinite(verts), verts, torch.full_like(verts, math.nan))
    lo = torch.nan_to_num(v, nan=math.inf).min(dim=0).values
    hi = torch.nan_to_num(v, nan=-math.inf).max(dim=0).values
    return torch.nan_to_num((hi - lo).norm() * 1e-4, nan=0.0, posinf=0.0)


def ao_origins(points, normals, verts, offset=None):
    """The ray origins (n, 3) of ambient_occlusion: points + offset x the unit normal, in fp32; offset None: default_offset(verts)."""
    off = default_offset(verts) if offset is None else torch.as_tensor(offset, dtype=torch.float32).to(points.device)
    return points.detach() + off * torch.nn.functional.normalize(normals.detach(), dim=1)


def ambient_occlusion(points, normals, verts, faces, samples=64, max_dist=math.inf, offset=None, seed=0, accel="auto"):
    """(n,) fp32 in [0, 1]: the share of `samples` rays from points (n, 3) that hit no face within max_dist, over the cosine-weighted
    directions of ao_directions about normals (n, 3) -- 1 in the open, 0 where everything is covered.  The origins are lifted by
    `offset` along the unit normal (a number or a 0-dim device tensor; None: default_offset(verts)); directions are unit vectors,
    so max_dist is a distance.  A point whose normal is (0, 0, 0) gets 1.  Deterministic: the directions are a fixed low-discrepancy set, rotated per point by a hash of its
    index and `seed`, and the cast's answer is a set property.  Nothing is read back."""
    name = "ambient_occlusion"
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"mesh_ray.{name}: samples must be >= 1, got {samples}")
    v, f, held = _resolve(name, verts, faces, accel)
    mesh_args.mesh(f"mesh_ray.{name}", v, f, ("points", points), ("normals", normals))
    if points.shape != normals.shape:
        raise ValueError(f"mesh_ray.{name}: points {tuple(points.shape)} and normals {tuple(normals.shape)} differ")
    lifted = ao_origins(points, normals, v, offset)
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    step = max(1, RAY_BATCH // samples)
    for at in range(0, points.shape[0], step):
        d = ao_directions(normals[at:at + step].detach(), samples, seed, at)
        o = lifted[at:at + step, None, :].expand(-1, samples, -1)
        hit = occluded(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3), v, f, 0.0, max_dist, held)
        out[at:at + step] = 1.0 - hit.reshape(-1, samples).float().mean(dim=1)
    return torch.where(normals.detach().abs().sum(dim=1) > 0, out, torch.ones_like(out))  # (no normal, no hemisphere: 1)


def vertex_ambient_occlusion(verts, faces, samples=64, max_dist=math.inf, offset=None, seed=0, flip=False, accel="auto"):
    """ambient_occlusion at the vertices, (V,), about visualize.vertex_normals (area-weighted; fp32 atomics, equal to rounding run to
    run -- where a normal's z is rounding noise about 0 its sign, which picks the half of ao_directions' frame, can differ from run to
    run, and with it the rotation of that vertex's set); flip=True negates them, for a mesh wound inwards.  A vertex without a normal
    (unreferenced) gets 1."""
    from .visualize import vertex_normals
    v, f = mesh_args.mesh("mesh_ray.vertex_ambient_occlusion", verts, faces)
    normals = vertex_normals(v, f)
    if flip:
        normals = -normals
    return ambient_occlusion(v, normals, v, f, samples, max_dist, offset, seed, accel)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m dgmesh_amd.mesh_ray",
                                 description="Bake a triangle-mesh PLY's vertex ambient occlusion into its vertex colours on the GPU.")
    ap.add_argument("mesh", help="triangle-mesh PLY file (ply_io's format)")
    ap.add_argument("--ao", required=True, metavar="OUT", help="the PLY to write: the input's vertex colours times the ambient occlusion, grey without any")
    ap.add_argument("--samples", type=int, default=64, metavar="N", help="rays per vertex")
    ap.add_argument("--max-dist", type=float, default=math.inf, help="occluders farther than this do not count")
    ap.add_argument("--flip", action="store_true", help="the mesh is wound inwards")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def main(argv=None):
    from .ply_io import read_mesh_ply_on_device, write_mesh_ply
    args = build_parser().parse_args(argv)
    verts, faces, colors = read_mesh_ply_on_device(args.mesh, torch.device("cuda", torch.cuda.current_device()))
    ao = vertex_ambient_occlusion(verts, faces, samples=args.samples, max_dist=args.max_dist, seed=args.seed, flip=args.flip)
    base = colors if colors is not None else torch.ones_like(verts)  # (an ambient occlusion of 1 gives the file's byte back)
    write_mesh_ply(args.ao, verts, faces, vertex_colors=base * ao[:, None])
    print(f"mesh_ray: V {len(verts)} F {len(faces)}  samples {args.samples}  mean ambient occlusion {float(ao.mean()) if len(verts) else 1.0:.4f}  -> {args.ao}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
