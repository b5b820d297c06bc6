"""Entering the mesh co-training phase: update_scale_center and normal_initialization of GaussianModelDPSRDynamicAnchor
(R/scene/gaussian_model_dpsr_dynamic_anchor.py:93-120, 684-734, called from R/train.py:242-246 at iteration == dpsr_iter; R/ = the
reference's dgmesh/) on top of libdgmesh_hip (csrc/normal_init.hip).

The step measures the scene (bounding boxes of the deformed Gaussians over `total_frames` times -> gaussian_center / gaussian_scale),
extracts a first surface from the Gaussians' opacity field (mesh_utils.get_opacity_field_from_gaussians -> marching_cubes.DiffMC at
isovalue -0.01 of the negated field), samples as many surface points as there are Gaussians, gives every Gaussian the face normal of
its nearest sample (anchor.nearest with max_d2 = +inf, the exact first minimum of pytorch3d.knn_points(K=1)) and sets the density
threshold to opt.init_density_threshold.  The reference goes through trimesh / numpy / open3d on the host three times and takes 50
torch.max / torch.min pairs; here it is one device-side chain whose only host synchronisation is DiffMC's 8-byte {V, F} read-back.

Surface sampling (trimesh.sample.sample_surface: faces weighted by area, uniform inside each).  trimesh is not vendored and draws from
numpy's global stream, so the conventions are this project's (checked against a float64 restatement, tests/_ninit_ref.py):
  * draws: u = torch.rand((count, 3), generator=generator, device=...), fp32; u[:, 0] picks the face, u[:, 1:] the point;
  * area[f] = 0.5 |cross(v1 - v0, v2 - v0)|, fp32, no FMA; 0 for an index outside [0, V) and for a non-finite result;
  * cum = inclusive sum of the areas in fp64 over a fixed partition (bit-reproducible, non-decreasing exactly);
  * pick = double(u0) * cum[F - 1]; face = the smallest i with cum[i] >= pick (np.searchsorted(cum, pick, side="left")) among the faces
    with cum[i] > 0 -- a face of area 0 is never chosen, and the face found is never behind the last face of positive area;
  * trimesh's fold: if u1 + u2 > 1 both become 1 - u; point = v0 + (u1 (v1 - v0) + u2 (v2 - v0)), fp32.
Deviations from the reference: the sampling stream is this project's; zero-area / invalid faces are never
sampled; an empty surface raises instead of indexing an empty array (one without area raises one call later, AreaCheck); with several ranks rank 0's result is broadcast (trainer.py).
No CPU fallback: every function raises on CPU tensors.
"""
import os

import torch

from . import _lib
from . import anchor as _A


def _need_cuda(name, *ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"normal_init.{name} needs CUDA/HIP tensors (dg-mesh_amd has no CPU path)")


def bbox_scratch(device):
    """The (zeroed) scratch of bbox(); one buffer serves any number of calls on one stream."""
    return torch.zeros(int(_lib.lib().dgm_ninit_bbox_scratch_bytes()), dtype=torch.uint8, device=device)


def bbox(xyz, d_xyz=None, out=None, scratch=None):
    """(min x, min y, min z, max x, max y, max z) of the rows xyz + d_xyz (one fp32 addition, as the reference's points = xyz + d_xyz)
    in one launch; a NaN coordinate makes both extrema of its axis NaN, like torch.max / torch.min.  `out`: a (6,) fp32 row to write."""
    _need_cuda("bbox", xyz)
    x = xyz.detach().contiguous().float()
    d = None
    if d_xyz is not None:
        _need_cuda("bbox", d_xyz)
        d = d_xyz.detach().contiguous().float()
        if d.shape != x.shape:
            raise RuntimeError(f"normal_init.bbox: d_xyz {tuple(d.shape)} does not match xyz {tuple(x.shape)}")
    if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] == 0:
        raise RuntimeError(f"normal_init.bbox: xyz must be (P, 3) with P >= 1, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(6, dtype=torch.float32, device=x.device)
    if scratch is None:
        scratch = bbox_scratch(x.device)
    with _lib.device_guard(x.device):
        _lib.check(_lib.lib().dgm_ninit_bbox(x.shape[0], _lib.vp(x), _lib.vp(d), _lib.vp(scratch), _lib.vp(out), _lib.stream_ptr()))
    return out


def scale_center_from_table(table, gaussian_ratio):
    """(center (3,), scale (1,)) from the (frames, 6) table of boxes, on the device (R/...:104-117): centre = mean over frames of
    (max + min) / 2, scale = max over frames of the largest box edge * gaussian_ratio / 2."""
    mn, mx = table[:, :3], table[:, 3:]
    center = torch.mean((mx + mn) / 2.0, dim=0)
    ratio = torch.max(torch.max(mx - mn, dim=1).values, dim=0).values
    return center, (ratio * gaussian_ratio / 2.0).reshape(1)


@torch.no_grad()
def update_scale_center(g, deform, total_frames=50, gaussian_ratio=1.1, gaussian_center=(0.0, 0.0, 0.0), real=False):
    """update_scale_center (R/...:93-120): sets g.gaussian_center (3,) and g.gaussian_scale (1,), both device tensors; nothing is read
    back.  real=False: the boxes of xyz + d_xyz(t / total_frames), t = 0 .. total_frames - 1, one MLP pass and one launch per frame."""
    xyz = g.get_xyz.detach()
    _need_cuda("update_scale_center", xyz)
    dev = xyz.device
    if real:
        g.gaussian_scale = torch.full((1,), float(gaussian_ratio), dtype=torch.float32, device=dev) / 2.0
        c = torch.empty(3, dtype=torch.float32, device=dev)
        for k in range(3):
            c[k].fill_(float(gaussian_center[k]))
        g.gaussian_center = c
        return None
    N = xyz.shape[0]
    table = torch.empty((total_frames, 6), dtype=torch.float32, device=dev)
    scratch = bbox_scratch(dev)
    # (the reference's torch.ones(N, 1) * t / total_frames: the same fp32 product and quotient, formed on the device)
    times = torch.arange(total_frames, dtype=torch.float32, device=dev) / total_frames
    for t in range(total_frames):
        d_xyz = deform.step(xyz, times[t].reshape(1, 1).expand(N, -1))[0]
        bbox(xyz, d_xyz, out=table[t], scratch=scratch)
    g.gaussian_center, g.gaussian_scale = scale_center_from_table(table, gaussian_ratio)
    return table


def face_areas(verts, faces):
    """area (F,) fp32 = 0.5 |cross(v1 - v0, v2 - v0)|; 0 for a face with an index outside [0, V) or a non-finite result."""
    _need_cuda("face_areas", verts, faces)
    v = verts.detach().contiguous().float()
    f = faces.detach().contiguous().to(torch.int32)
    area = torch.empty(f.shape[0], dtype=torch.float32, device=v.device)
    with _lib.device_guard(v.device):
        _lib.check(_lib.lib().dgm_ninit_face_areas(v.shape[0], f.shape[0], _lib.vp(v), _lib.vp(f), _lib.vp(area), _lib.stream_ptr()))
    return area


def cumulative_areas(area):
    """Inclusive fp64 sums of `area` (F,) fp32 over the kernel's fixed partition: (F,) float64, non-decreasing, bit-reproducible."""
    _need_cuda("cumulative_areas", area)
    a = area.contiguous().float()
    F = a.shape[0]
    L = _lib.lib()
    cum = torch.empty(F, dtype=torch.float64, device=a.device)
    scratch = torch.empty(int(L.dgm_ninit_scan_scratch_bytes(F)), dtype=torch.uint8, device=a.device)
    with _lib.device_guard(a.device):
        _lib.check(L.dgm_ninit_area_scan(F, _lib.vp(a), _lib.vp(scratch), _lib.vp(cum), _lib.stream_ptr()))
    return cum


class AreaCheck:
    """The total sampled area on its way to the host without anyone waiting for it: an asynchronous 8-byte copy into pinned memory
    and an event.  Calling the object waits for the event (long past when the next iteration calls it) and raises if the area was
    not positive -- every face of the surface degenerate, so that every normal the chain wrote is zero."""

    def __init__(self, total, F):
        self.F = F
        self.host = torch.empty(1, dtype=torch.float64).pin_memory()
        self.host.copy_(total.reshape(1), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def __call__(self):
        self.event.synchronize()
        if not float(self.host[0]) > 0.0:
            raise RuntimeError(f"normal_init: the total area of the {self.F} faces of the sampled surface is 0: no point could be "
                               "sampled and every normal was set to zero")


def sample_surface(verts, faces, count, generator=None, draws=None, check=True):
    """trimesh.sample.sample_surface on the device: (points (count, 3) fp32, face_index (count,) int32), conventions in the module
    docstring.  `draws`: a (count, 3) fp32 tensor used instead of the generator (a test feeds recorded ones).  F == 0 raises; so does a
    total area of 0 when `check` (an 8-byte read-back); with check=False such a mesh gives face_index -1 and NaN points."""
    points, face_index, _ = _sample(verts, faces, count, generator, draws, check)
    return points, face_index


def _sample(verts, faces, count, generator, draws, check):
    """sample_surface plus the total area as a (1,) float64 device tensor."""
    _need_cuda("sample_surface", verts, faces)
    v = verts.detach().contiguous().float()
    f = faces.detach().contiguous().to(torch.int32)
    V, F = v.shape[0], f.shape[0]
    if F == 0:
        raise RuntimeError("normal_init.sample_surface: the mesh has no faces")
    cum = cumulative_areas(face_areas(v, f))
    if check and not float(cum[-1]) > 0.0:
        raise RuntimeError(f"normal_init.sample_surface: the total area of the {F} faces is 0")
    if draws is None:
        u = torch.rand((count, 3), generator=generator, device=v.device, dtype=torch.float32)
    else:
        _need_cuda("sample_surface", draws)
        u = draws.contiguous().float()
        if tuple(u.shape) != (count, 3):
            raise RuntimeError(f"normal_init.sample_surface: draws must be ({count}, 3), got {tuple(u.shape)}")
    points = torch.empty((count, 3), dtype=torch.float32, device=v.device)
    face_index = torch.empty(count, dtype=torch.int32, device=v.device)
    with _lib.device_guard(v.device):
        _lib.check(_lib.lib().dgm_ninit_sample(V, F, count, _lib.vp(v), _lib.vp(f), _lib.vp(cum), _lib.vp(u), _lib.vp(points), _lib.vp(face_index),
                                               _lib.stream_ptr()))
    return points, face_index, cum[-1:]


def normals_from_surface(xyz, verts, faces, count, generator=None, draws=None):
    """Steps 4-5 of normal_initialization: sample `count` surface points, give every row of xyz the unit face normal of its nearest
    sample (zero for a degenerate face or when nothing could be sampled).  Nothing is read back: the total area comes along as a
    device tensor for AreaCheck.  -> (normals (P, 3), samples, face_index, nearest (P,), total_area (1,) float64)."""
    samples, face_index, total = _sample(verts, faces, count, generator, draws, False)
    _, face_normals = _A.face_geometry(verts, faces)
    sample_normals = face_normals[face_index.long().clamp_min(0)]
    idx, _ = _A.nearest(xyz, samples)  # max_d2 = +inf: knn_points(K=1)
    normals = torch.where((idx >= 0)[:, None], sample_normals[idx.clamp_min(0)], torch.zeros_like(xyz))
    return normals, samples, face_index, idx, total


ISOVALUE = -0.01      # R/...:704
OCC_BBOX_SCALE = 2.0  # R/...:693


@torch.no_grad()
def normal_initialization(g, deform, d_xyz, d_rotation, d_scaling, *, opt, gaussian_ratio=1.1, gaussian_center=(0.0, 0.0, 0.0),
                          real=False, generator=None, out_dir=None, occ_resolution=256, diffmc=None, draws=None):
    """normal_initialization (R/...:684-734).  d_xyz / d_rotation / d_scaling: this iteration's deformation (tensors, or the float
    0.0 before warm_up).  Sets g.gaussian_center / gaussian_scale, g._normal.data (the Parameter object and its Adam state stay) and
    g.density_thres_param; `draws`: a (P, 3) table used instead of the generator (a test feeds the reference's); `out_dir`: also writes mesh_init.ply and pointcloud_init.ply there (None: nothing is copied to the host).
    Returns {"V", "F", "verts", "faces", "samples", "face_index", "nearest", "area_check"}; an empty surface raises RuntimeError.  A
    surface whose faces all have area 0 cannot be told without waiting for the device: `area_check` is an AreaCheck whose call raises
    in that case; call it once the step has been enqueued (the trainer does so at the start of the next iteration)."""
    from .marching_cubes import DiffMC
    from .mesh_utils import get_opacity_field_from_gaussians
    _need_cuda("normal_initialization", g.get_xyz)
    update_scale_center(g, deform, gaussian_ratio=gaussian_ratio, gaussian_center=gaussian_center, real=real)
    xyz = (g.get_xyz + d_xyz).detach()
    occ = get_opacity_field_from_gaussians(xyz, g.get_rotation + d_rotation, g.get_scaling + d_scaling, g.get_opacity,
                                           resolution=occ_resolution, bbox_scale=OCC_BBOX_SCALE)
    verts, faces = (diffmc or DiffMC(dtype=torch.float32))(-occ, deform=None, isovalue=ISOVALUE)
    if faces.shape[0] == 0:
        raise RuntimeError(f"normal_initialization: the negated opacity field has no surface at isovalue {ISOVALUE} "
                           f"(the field's maximum is {float(occ.max()):.6g}, it must exceed {-ISOVALUE}): no mesh to take normals from")
    verts = verts * 2.0 * OCC_BBOX_SCALE - OCC_BBOX_SCALE
    P = xyz.shape[0]
    normals, samples, face_index, idx, total = normals_from_surface(xyz, verts, faces, P, generator=generator, draws=draws)
    g._normal.data = normals
    g.density_thres_param.data.fill_(float(opt.init_density_threshold))
    if out_dir is not None:
        from .ply_io import write_mesh_ply, write_pointcloud_ply
        write_mesh_ply(os.path.join(out_dir, "mesh_init.ply"), verts, faces)
        write_pointcloud_ply(os.path.join(out_dir, "pointcloud_init.ply"), xyz, normals)
    return {"V": verts.shape[0], "F": faces.shape[0], "verts": verts, "faces": faces, "samples": samples, "face_index": face_index,
            "nearest": idx, "area_check": AreaCheck(total, faces.shape[0])}
