"""Writes tests/golden/anchor_small.npz: the REFERENCE's Gaussian-mesh anchoring executed from its source text on the CPU.

Run from the repository root:  python tests/golden/make_anchor_golden.py   (needs the reference tree at REF below).

GaussianModelDPSRDynamicAnchor.prune_points, _prune_optimizer, cat_tensors_to_optimizer, densification_postfix,
average_and_prune, densify_from_face, anchor_mesh and get_xyz (R/scene/gaussian_model_dpsr_dynamic_anchor.py:130-132, 383-460,
599-677, 745-829) are compiled into a host class that owns the seven parameter tensors, a torch.optim.Adam with the reference's
group names and the densification statistics; inverse_sigmoid comes from R/utils/general_utils.py.  Edits to the source text:
device "cuda" -> "cpu", .cuda() dropped, torch.cuda.empty_cache() dropped, and the random draws (the two torch.randperm, the one
torch.randn of densify_from_face) routed through recorders, so a device implementation can be fed the same draws.
Stubs for the packages the reference imports:
  * pytorch3d.ops.knn_points(K=1): an fp32 brute force, d2 = (dx*dx + dy*dy) + dz*dz, first index of the minimum, d2 differentiable;
  * trimesh.Trimesh: triangles_center (fp64 mean of the three vertices), face_normals (fp64 unit cross product, zero for a zero
    cross product), edges_unique_length;
  * simple_knn distCUDA2: brute-force mean squared distance to the 3 nearest other points (fp32);
  * pytorch3d.transforms.axis_angle_to_quaternion: restated (real part first);
  * deform / deform_back: tests/_anchor_ref.PolyField, fixed analytic fields with four outputs.
Cases: 1-1, n-1 (faces with 2 and with >= 3 Gaussians), 0-1 faces, invalid Gaussians, degenerate faces, Adam state present."""
import ast
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _anchor_ref import PolyField  # noqa: E402

REF = "/root/reference/dgmesh"
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "normal")
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
            rotation="_rotation", normal="_normal")
WANT = {"prune_points", "_prune_optimizer", "cat_tensors_to_optimizer", "densification_postfix", "average_and_prune",
        "densify_from_face", "anchor_mesh", "get_xyz"}


def knn_points(p1, p2, K=1):
    assert K == 1 and p1.shape[0] == 1 and p2.shape[0] == 1
    q, t = p1[0].float(), p2[0].float()
    with torch.no_grad():
        dx = t[None, :, 0] - q[:, None, 0]
        dy = t[None, :, 1] - q[:, None, 1]
        dz = t[None, :, 2] - q[:, None, 2]
        _, j = ((dx * dx + dy * dy) + dz * dz).min(1)
    d = t[j] - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d2[None, :, None], j[None, :, None], None


class Trimesh:
    def __init__(self, vertices, faces):
        v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
        tri = v[f]
        self.triangles_center = tri.mean(axis=1)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        self.face_normals = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        e = np.unique(e, axis=0)
        self.edges_unique_length = np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1)


def distCUDA2(p):
    p = p.float()
    d = ((p[:, None, 0] - p[None, :, 0]) ** 2 + (p[:, None, 1] - p[None, :, 1]) ** 2) + (p[:, None, 2] - p[None, :, 2]) ** 2
    d.fill_diagonal_(float("inf"))
    k = min(3, p.shape[0] - 1)
    v = d.topk(k, dim=1, largest=False).values if k > 0 else d[:, :0]
    v = torch.cat([v, torch.full((p.shape[0], 3 - k), 3.4028234663852886e38)], 1)
    return v.mean(1)


def axis_angle_to_quaternion(axis_angle):
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half_angles = angles * 0.5
    small = angles.abs() < 1e-6
    s = torch.empty_like(angles)
    s[~small] = torch.sin(half_angles[~small]) / angles[~small]
    s[small] = 0.5 - (angles[small] * angles[small]) / 48
    return torch.cat([torch.cos(half_angles), axis_angle * s], dim=-1)


def host_class(draws):
    src = open(os.path.join(REF, "scene/gaussian_model_dpsr_dynamic_anchor.py")).read()
    for a, b in (("device='cuda'", "device='cpu'"), ('device="cuda"', 'device="cpu"'), ("torch.cuda.empty_cache()", "pass"),
                 (".float().cuda()", ".float()"), ("torch.randperm(", "_rec_randperm("),
                 ("torch.randn((new_normal.shape[0], 1)", "_rec_randn((new_normal.shape[0], 1)")):
        assert a in src, a
        src = src.replace(a, b)
    gen = torch.Generator().manual_seed(draws["seed"])

    def rec_randperm(n, device=None):
        p = torch.randperm(n, generator=gen)
        draws["perm"].append(p)
        return p

    def rec_randn(shape, device=None):
        r = torch.randn(shape, generator=gen)
        draws["randn"].append(r)
        return r

    ns = {"torch": torch, "nn": torch.nn, "np": np, "knn_points": knn_points, "trimesh": types.SimpleNamespace(Trimesh=Trimesh),
          "distCUDA2": distCUDA2, "p3d": types.SimpleNamespace(transforms=types.SimpleNamespace(axis_angle_to_quaternion=axis_angle_to_quaternion)),
          "_rec_randperm": rec_randperm, "_rec_randn": rec_randn}
    for node in ast.parse(open(os.path.join(REF, "utils/general_utils.py")).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "inverse_sigmoid":
            exec(compile(ast.Module([node], []), "general_utils.py", "exec"), ns)
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "GaussianModelDPSRDynamicAnchor")
    body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert {n.name for n in body} == WANT
    host = ast.ClassDef(name="RefHost", bases=[], keywords=[], body=body, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module([host], [])), "gaussian_model_dpsr_dynamic_anchor.py", "exec"), ns)
    return ns["RefHost"]


def make_case(seed, P, F, sh, scale):
    rng = np.random.RandomState(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    ctr = rng.rand(F, 3) * 2 - 1
    verts = f32((ctr[:, None, :] + 0.02 * rng.randn(F, 3, 3)).reshape(3 * F, 3))
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    faces[:4, 2] = faces[:4, 1]                                   # degenerate: two equal indices
    verts[3 * 4 + 1] = verts[3 * 4]                               # degenerate: three equal positions (face 4)
    verts[3 * 4 + 2] = verts[3 * 4]
    # Gaussians: clusters of 1..5 around the centroids of the first half of the faces, plus far-away (invalid) ones
    cent = verts[faces].astype(np.float64).mean(1)
    hosts = []
    for f in range(F // 2):
        hosts += [f] * int(rng.choice([1, 1, 2, 3, 5]))
    hosts = np.array(hosts)
    xyz = cent[hosts] + 0.002 * rng.randn(hosts.size, 3)
    xyz = np.concatenate([xyz, rng.rand(40, 3) * 4 + 3])      # invalid: far from every face
    perm = rng.permutation(xyz.shape[0])[:P]
    xyz = f32(xyz[perm])
    P = xyz.shape[0]
    K = (sh + 1) ** 2 - 1
    raw = dict(xyz=xyz, f_dc=f32(rng.randn(P, 1, 3)), f_rest=f32(0.1 * rng.randn(P, K, 3)), opacity=f32(rng.randn(P, 1)),
               scaling=f32(np.log(rng.uniform(0.002, 0.02, (P, 3)))), rotation=f32(rng.randn(P, 4)),
               normal=f32(rng.randn(P, 3)))
    deform = PolyField(*[f32(0.002 * rng.randn(*s)) for s in ((4, 3), (4,), (3,), (3,))])
    back = PolyField(*[f32(0.002 * rng.randn(*s)) for s in ((4, 3), (4,), (3,), (3,))])
    return raw, verts, faces, deform, back


def run_case(tag, seed, P, F, sh, scale, radius, t, topn, bs, increase_bs, rec):
    raw, verts, faces, deform, back = make_case(seed, P, F, sh, scale)
    draws = {"seed": seed, "perm": [], "randn": []}
    h = host_class(draws)()
    h.gaussian_param_list = list(NAMES)
    h.max_sh_degree = sh
    h.gaussian_scale = torch.tensor([scale], dtype=torch.float32)
    for k in NAMES:
        setattr(h, ATTR[k], torch.nn.Parameter(torch.tensor(raw[k]).requires_grad_(True)))
    h.optimizer = torch.optim.Adam([{"params": [getattr(h, ATTR[k])], "lr": 1e-3, "name": k} for k in NAMES], lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(seed + 1)
    for _ in range(2):  # non-trivial Adam moments
        for k in NAMES:
            getattr(h, ATTR[k]).grad = torch.randn(getattr(h, ATTR[k]).shape, generator=g)
        h.optimizer.step()
    Pn = h._xyz.shape[0]
    h.xyz_gradient_accum = torch.rand((Pn, 1), generator=g)
    h.denom = torch.ones((Pn, 1))
    h.max_radii2D = torch.rand(Pn, generator=g)
    grp = {x["name"]: x["params"][0] for x in h.optimizer.param_groups}
    for k in NAMES:
        st = h.optimizer.state[grp[k]]
        rec[f"{tag}/in/p/{k}"] = grp[k].detach().numpy().copy()
        rec[f"{tag}/in/m/{k}"] = st["exp_avg"].numpy().copy()
        rec[f"{tag}/in/v/{k}"] = st["exp_avg_sq"].numpy().copy()
    rec[f"{tag}/verts"], rec[f"{tag}/faces"] = verts, faces.astype(np.int32)
    for name, fld in (("deform", deform), ("back", back)):
        for i, c in enumerate(fld.consts()):
            rec[f"{tag}/{name}/{i}"] = c
    rec[f"{tag}/args"] = np.array([scale, radius, t, topn, bs, increase_bs, sh], np.float64)
    loss = h.anchor_mesh(torch.tensor(verts), torch.tensor(faces), deform, back, t, search_radius=radius, topn=topn, bs=bs,
                         increase_bs=increase_bs)
    assert len(draws["perm"]) == 2 and len(draws["randn"]) <= 1
    rec[f"{tag}/perm_n1"] = draws["perm"][0].numpy().astype(np.int32)
    rec[f"{tag}/perm_0_1"] = draws["perm"][1].numpy().astype(np.int32)
    rec[f"{tag}/angle"] = (draws["randn"][0] if draws["randn"] else torch.zeros(0, 1)).numpy()
    rec[f"{tag}/loss"] = np.float64(float(loss.detach()))
    grp = {x["name"]: x["params"][0] for x in h.optimizer.param_groups}
    for k in NAMES:
        assert grp[k] is getattr(h, ATTR[k])
        st = h.optimizer.state[grp[k]]
        rec[f"{tag}/out/p/{k}"] = grp[k].detach().numpy().copy()
        rec[f"{tag}/out/m/{k}"] = st["exp_avg"].numpy().copy()
        rec[f"{tag}/out/v/{k}"] = st["exp_avg_sq"].numpy().copy()
    rec[f"{tag}/out/accum"], rec[f"{tag}/out/denom"] = h.xyz_gradient_accum.numpy().copy(), h.denom.numpy().copy()
    rec[f"{tag}/out/max_radii"] = h.max_radii2D.numpy().copy()
    print(tag, "P", Pn, "->", h._xyz.shape[0], "loss", float(loss))


def main():
    rec = {}
    # (tag, seed, P, F, sh, gaussian_scale, search_radius, t, topn, bs, increase_bs)
    run_case("c0", 11, 900, 400, 1, 1.3, 0.0005, 0.25, 2, 40, 60, rec)
    run_case("c1", 12, 700, 300, 1, 1.0, 0.0015, 0.7, 2, 10_000, 10_000, rec)
    path = os.path.join(HERE, "anchor_small.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
