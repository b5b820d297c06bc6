"""Writes tests/golden/normal_init_small.npz: the REFERENCE's update_scale_center and normal_initialization executed from their
source text on the CPU.

Run from the repository root:  python tests/golden/make_normal_init_golden.py   (needs the reference tree at REF below).

GaussianModelDPSRDynamicAnchor.update_scale_center, normal_initialization and the properties get_xyz / get_rotation / get_scaling /
get_opacity (R/scene/gaussian_model_dpsr_dynamic_anchor.py:93-132, 684-734; R/ = dgmesh/) are compiled into a host class that owns the
parameter tensors; get_opacity_field_from_gaussians (R/utils/mesh_utils.py:7-76) and its helpers (R/utils/general_utils.py) are
executed from source too.  Edits to the source text: device 'cuda' -> 'cpu' (both quote styles) and .to("cuda") -> .to("cpu").
The one edit of a value: get_opacity_field_from_gaussians is called with resolution = RES instead of its default 256, so that the
fixture stays small.  Stubs for the packages the reference imports:
  * trimesh.Trimesh(vertices, faces): area_faces (fp64, 0.5 |cross|), face_normals (fp64 unit cross product, zero for a zero cross
    product), export = no-op;
  * trimesh.sample.sample_surface(mesh, count): trimesh's algorithm restated (np.cumsum of area_faces, np.searchsorted, the fold
    |u - 1| where u1 + u2 > 1, origin + sum of the two scaled edge vectors, all fp64) with its two np.random.random draws replaced by
    the columns of a recorded (count, 3) fp32 table u = torch.rand(..., generator=seeded): u[:, 0] picks the face, u[:, 1:] the point;
  * pytorch3d.ops.knn_points(K=1): the fp32 brute force of make_anchor_golden.py, d2 = (dx*dx + dy*dy) + dz*dz, first minimum;
  * open3d: no-op;  kiui.lo: no-op;  self.diffmc: tests/_mc_ref.marching_cubes (this project's marching-cubes conventions);
  * deform: tests/_anchor_ref.PolyField, a fixed analytic field with four outputs.
Scene: P Gaussians on a smooth closed blob.

The seed of the draws is the first one for which, on the golden mesh, (a) every pick lies farther than 2^-30 * total from every
cumulative boundary, for the fp64 areas and for the device's fp32 areas alike, and both give the same faces (the device sums fp32
areas, trimesh fp64 ones: with such a seed the two definitions agree on every draw); (b) no u1 + u2 lies within 1e-6 of 1 (the fold is
decided in fp32 on the device); (c) every Gaussian's nearest sample leads the second nearest by more than 5e-8 in d2 (the samples'
fp32 rounding moves d2 by ~1e-8).

flip_share_ref: the reference chain is re-run with occ perturbed by +- (2e-6 + 2e-5 |occ|) -- the tolerance of
tests/test_opacity_field.py::test_matches_reference_loop -- with a seeded random sign per voxel and with the opposite signs, same
draws; the larger share of Gaussians whose normal turns by more than 1 degree is stored.  It must be <= 0.02."""
import ast
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mc_ref  # noqa: E402
import _ninit_ref as NR  # noqa: E402
from _anchor_ref import PolyField  # noqa: E402
from make_anchor_golden import knn_points  # noqa: E402

REF = "/root/reference/dgmesh"
RES = 48
P = 3000
T0 = 0.3
WANT = {"update_scale_center", "normal_initialization", "get_xyz", "get_rotation", "get_scaling", "get_opacity"}
EDITS = (("device='cuda'", "device='cpu'"), ('device="cuda"', 'device="cpu"'), ('.to("cuda")', '.to("cpu")'))


class Trimesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
        tri = self.vertices[self.faces]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        self.area_faces = 0.5 * ln[:, 0]
        self.face_normals = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
        self.triangles = tri

    def export(self, path):
        pass


def functions(path, names, ns, subst=()):
    src = open(path).read()
    for a, b in subst:
        src = src.replace(a, b)
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), os.path.basename(path), "exec"), ns)


def host_class(state):
    """state: {"u": (count, 3) fp32 draws, "occ": None or the field to return instead of computing it, "rec": dict of records}."""
    src = open(os.path.join(REF, "scene/gaussian_model_dpsr_dynamic_anchor.py")).read()
    for a, b in EDITS:
        assert a in src, a
        src = src.replace(a, b)

    def sample_surface(mesh, count):
        u = state["u"].astype(np.float64)
        assert u.shape == (count, 3)
        weight_cum = np.cumsum(mesh.area_faces)
        face_pick = u[:, 0] * weight_cum[-1]
        face_index = np.searchsorted(weight_cum, face_pick)
        tri_origins = mesh.triangles[:, 0][face_index]
        tri_vectors = (mesh.triangles[:, 1:] - mesh.triangles[:, :1])[face_index]
        random_lengths = u[:, 1:].reshape(count, 2, 1).copy()
        test = random_lengths.sum(axis=1).reshape(-1) > 1.0
        random_lengths[test] -= 1.0
        random_lengths = np.abs(random_lengths)
        samples = (tri_vectors * random_lengths).sum(axis=1) + tri_origins
        state["rec"].update(samples=samples, face_index=face_index, fold_margin=np.abs(u[:, 1] + u[:, 2] - 1.0).min())
        return samples, face_index

    def knn(p1, p2, K=1):
        out = knn_points(p1, p2, K=K)
        state["rec"]["nearest"] = out[1].reshape(-1).numpy().copy()
        return out

    ons = {"torch": torch, "np": np, "kiui": types.SimpleNamespace(lo=lambda *a, **k: None)}
    functions(os.path.join(REF, "utils/general_utils.py"),
              {"strip_lowerdiag", "strip_symmetric", "build_rotation", "build_scaling_rotation", "build_covariance_from_scaling_rotation",
               "gaussian_3d_coeff"}, ons, EDITS[:2])
    functions(os.path.join(REF, "utils/mesh_utils.py"), {"get_opacity_field_from_gaussians"}, ons)

    def opacity_field(*a, **k):
        occ = ons["get_opacity_field_from_gaussians"](*a, resolution=RES, **k) if state["occ"] is None else state["occ"]
        state["rec"]["occ"] = occ.numpy().copy()
        return occ

    o3d = types.SimpleNamespace(geometry=types.SimpleNamespace(PointCloud=lambda: types.SimpleNamespace()),
                                utility=types.SimpleNamespace(Vector3dVector=lambda a: a),
                                io=types.SimpleNamespace(write_point_cloud=lambda *a, **k: None))
    ns = {"torch": torch, "nn": torch.nn, "np": np, "osp": os.path, "knn_points": knn, "o3d": o3d,
          "trimesh": types.SimpleNamespace(Trimesh=Trimesh, sample=types.SimpleNamespace(sample_surface=sample_surface)),
          "get_opacity_field_from_gaussians": opacity_field}
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "GaussianModelDPSRDynamicAnchor")
    body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert {n.name for n in body} == WANT
    host = ast.ClassDef(name="RefHost", bases=[], keywords=[], body=body, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module([host], [])), "gaussian_model_dpsr_dynamic_anchor.py", "exec"), ns)
    return ns["RefHost"]


def diffmc(grid, deform=None, isovalue=0.0):
    v, f, _ = _mc_ref.marching_cubes(grid.numpy(), iso=isovalue)
    state_rec["verts01"], state_rec["faces"] = v.copy(), f.copy()
    return torch.tensor(v), torch.tensor(f.astype(np.int64))


state_rec = {}


def make_scene():
    rng = np.random.RandomState(5)
    f32 = lambda a: np.asarray(a, np.float32)
    d = rng.randn(P, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a smooth closed blob: an ellipsoid with one low-frequency bump
    r = 0.75 * (1.0 + 0.15 * d[:, 0] * d[:, 1] + 0.1 * d[:, 2] ** 2)
    xyz = f32(d * r[:, None] * np.array([1.0, 0.85, 0.7]) + np.array([0.05, -0.03, 0.02]))
    raw = dict(xyz=xyz, rotation=f32(rng.randn(P, 4)), scaling=f32(np.log(rng.uniform(0.05, 0.09, (P, 3)))),
               opacity=f32(rng.uniform(0.0, 2.0, (P, 1))))
    deform = PolyField(*[f32(s * rng.randn(*shape)) for s, shape in ((0.01, (4, 3)), (0.002, (4,)), (0.002, (3,)), (0.002, (3,)))])
    return raw, deform


def new_host(state, raw):
    h = host_class(state)()
    for k in ("xyz", "rotation", "scaling", "opacity"):
        setattr(h, "_" + k, torch.nn.Parameter(torch.tensor(raw[k])))
    h._normal = torch.nn.Parameter(torch.zeros(P, 3))
    h.scaling_activation, h.opacity_activation, h.rotation_activation = torch.exp, torch.sigmoid, torch.nn.functional.normalize
    h.density_thres_param = torch.nn.Parameter(torch.tensor(0.0))
    h.diffmc = diffmc
    return h


def run(raw, deform, u, occ=None):
    state = {"u": u, "occ": occ, "rec": {}}
    h = new_host(state, raw)
    xyz = torch.tensor(raw["xyz"])
    d_xyz, d_rot, d_scl, _ = deform.step(xyz, T0)
    with tempfile.TemporaryDirectory() as tmp:
        h.normal_initialization(types.SimpleNamespace(data_type="DNeRF", model_path=tmp), types.SimpleNamespace(init_density_threshold=0.05),
                                types.SimpleNamespace(gaussian_ratio=1.1, gaussian_center=[0.0, 0.0, 0.0]), deform, d_xyz, d_rot, d_scl)
    rec = dict(state["rec"], **state_rec)
    rec.update(center=h.gaussian_center.numpy().copy(), scale=np.asarray(h.gaussian_scale.numpy()).reshape(-1).copy(),
               normals=h._normal.detach().numpy().copy(), threshold=h.density_thres_param.detach().numpy().reshape(-1).copy(),
               d_xyz=d_xyz.numpy().copy())
    return rec


def draws(seed):
    return torch.rand((P, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float32).numpy()


def seed_ok(seed, verts, faces, xyz_d):
    u = draws(seed)
    total = None
    picks = []
    for areas in (NR.face_areas(verts, faces), NR.face_areas32(verts, faces)):
        cum = np.cumsum(np.asarray(areas, np.float64))
        idx, margin = NR.pick_faces(cum, u[:, 0])
        total = cum[-1]
        if margin.min() <= 2.0 ** -30 * total:
            return False
        picks.append(idx)
    if not np.array_equal(picks[0], picks[1]) or np.abs(u[:, 1].astype(np.float64) + u[:, 2] - 1.0).min() < 1e-6:
        return False
    samples, _, _ = NR.sample_surface(verts, faces, u)
    _, gap = NR.nearest32(xyz_d, samples.astype(np.float32))
    return gap.min() > 5e-8


def main():
    raw, deform = make_scene()
    base = run(raw, deform, draws(0))  # (the mesh does not depend on the draws)
    verts = base["verts01"] * np.float32(4.0) - np.float32(2.0)
    xyz_d = raw["xyz"] + base["d_xyz"]
    seed = next(s for s in range(10000) if seed_ok(s, verts, base["faces"], xyz_d))
    u = draws(seed)
    gold = run(raw, deform, u)
    assert gold["fold_margin"] >= 1e-6
    occ = torch.tensor(gold["occ"])
    sign = torch.tensor(np.random.RandomState(99).choice([-1.0, 1.0], size=occ.shape).astype(np.float32))
    tol = 2e-6 + 2e-5 * occ.abs()
    shares = []
    for sgn in (1.0, -1.0):
        pert = run(raw, deform, u, occ=occ + sgn * sign * tol)
        cos = (pert["normals"].astype(np.float64) * gold["normals"].astype(np.float64)).sum(1)
        shares.append(float((cos < np.cos(np.deg2rad(1.0))).mean()))
    flip = max(shares)
    print("seed", seed, "V", len(verts), "F", len(gold["faces"]), "flip shares", shares, "occ max", float(occ.max()))
    assert flip <= 0.02, flip
    rec = dict(xyz=raw["xyz"], rotation=raw["rotation"], scaling=raw["scaling"], opacity=raw["opacity"], t0=np.float64(T0),
               res=np.int64(RES), seed=np.int64(seed), u=u, occ=gold["occ"].astype(np.float32), center=gold["center"], scale=gold["scale"],
               V=np.int64(len(verts)), F=np.int64(len(gold["faces"])), verts=verts.astype(np.float32), faces=gold["faces"].astype(np.int32),
               samples=gold["samples"], face_index=gold["face_index"].astype(np.int32), nearest=gold["nearest"].astype(np.int32),
               normals=gold["normals"], threshold=gold["threshold"], flip_share_ref=np.float64(flip),
               gaussian_ratio=np.float64(1.1))
    for i, c in enumerate(deform.consts()):
        rec[f"deform/{i}"] = c
    path = os.path.join(HERE, "normal_init_small.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
