"""GPU tests of ray casting against a mesh (dg-mesh_amd/mesh_ray.py, csrc/mesh_ray.hip, mesh_texture.bake_ambient_occlusion) against the
numpy restatement of the definition (tests/_ray_ref.py).

Bits: face, t and bary of the device equal the fp32 restatement's on every ray, on both paths (brute force and the structure), alone,
in a batch and permuted.  Values: against the fp64 statement with tol = TOL_FACTOR x the largest deviation of the fp32 restatement
from the fp64 one on the same inputs (t, and the barycentrics on the fp32 statement's face) -- what the number format gives on the
case, not a chosen number; the device's own figures are printed.  No ray is excluded: a miss on one side with a hit on the other is
allowed only where the fp64 hit lies within tol of an edge or of a grazing face."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _edges_ref as E
import _inside_ref as IR
import _ray_ref as R
from conftest import pkg
from test_visualize import _record_psr, scene  # noqa: F401  (the tiny mesh-phase scene of the visualize tests, as a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0  # (tests/test_mesh_inside.py)
PATHS = ("brute", "accel")
INF = math.inf


def M():
    return pkg("mesh_ray")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the shared cases are read-only)


def accel_of(path, v, f):
    return None if path == "brute" else M().RayMesh(v, f)


def cast(o, d, v, f, accel, t_min=0.0, t_max=INF):
    face, t, bary = M().ray_cast(o, d, v, f, t_min, t_max, accel)
    assert face.dtype == torch.int32 and t.dtype == torch.float32 and bary.dtype == torch.float32
    assert face.shape == (o.shape[0],) and t.shape == (o.shape[0],) and bary.shape == (o.shape[0], 3) and face.device.type == "cuda"
    return face.cpu().numpy(), t.cpu().numpy(), bary.cpu().numpy()


def same_bits(got, ref, what):
    for name, a, b in zip(("face", "t", "bary"), got, ref):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1)) if len(a) else []
        assert len(bad) == 0, f"{what}: {name} differs on {len(bad)} of {len(a)} rays, the first ray {bad[0]}: {a[bad[0]]} against {b[bad[0]]}"


def f3(a):
    return np.asarray(a, np.float32).reshape(-1, 3)


# ---- 1: known answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_known_answers_on_one_triangle(path):
    v, f = dev(f3([[0, 0, 0], [1, 0, 0], [0, 1, 0]])), dev(np.array([[0, 1, 2]], np.int32))
    acc = accel_of(path, v, f)
    o = dev(f3([[0.25, 0.25, 2], [1.5, 0.25, 2], [0.25, 0.25, 2], [0.25, 0.25, 0], [-1, 0.25, 0]]))
    d = dev(f3([[0, 0, -1], [0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0]]))  # hit, beside, behind the origin, two rays in the plane
    face, t, bary = cast(o, d, v, f, acc)
    assert face.tolist() == [0, -1, -1, -1, -1]
    assert t[0] == 2 and bary[0].tolist() == [0.5, 0.25, 0.25]
    assert np.isposinf(t[1:]).all() and (bary[1:] == 0).all()
    assert M().occluded(o, d, v, f, accel=acc).tolist() == [True, False, False, False, False]
    assert cast(o[:1], d[:1] * 2, v, f, acc)[1][0] == 1  # t is in units of |d|
    # t_min is inclusive and t_max exclusive, with t landing exactly on each
    assert cast(o[:1], d[:1], v, f, acc, 2.0, 3.0)[0][0] == 0
    assert cast(o[:1], d[:1], v, f, acc, 1.0, 2.0)[0][0] == -1
    assert cast(o[:1], d[:1], v, f, acc, float(np.nextafter(np.float32(2), np.float32(3))), 9.0)[0][0] == -1
    assert M().occluded(o[:1], d[:1], v, f, 2.0, 3.0, acc).tolist() == [True] and M().occluded(o[:1], d[:1], v, f, 1.0, 2.0, acc).tolist() == [False]
    hp = M().hit_points(o, d, dev(t)).cpu().numpy()
    assert hp[0].tolist() == [0.25, 0.25, 0] and np.isnan(hp[1:]).all()


@pytest.mark.parametrize("path", PATHS)
def test_known_answers_on_a_cube(path):
    verts, faces = R.cube()
    v, f = dev(verts), dev(faces)
    acc = accel_of(path, v, f)
    # through a side's diagonal (faces 2k and 2k + 1 share it), through an edge of the cube, through a corner: the lowest index wins
    o = f3([[-1, 0.5, 0.5], [0.5, 0.5, 3], [-1, -1, 0.5], [-1, -1, -1]])
    d = f3([[1, 0, 0], [0, 0, -1], [1, 1, 0], [1, 1, 1]])
    face, t, bary = cast(dev(o), dev(d), v, f, acc)
    assert face.tolist() == [0, 10, 0, 0] and t.tolist() == [1, 2, 1, 1]
    assert np.abs(bary.sum(1) - 1).max() < 1e-6 and bary.min() >= 0
    for n in range(4):  # both (all) faces that meet at the hit point are hit on their own, with the same t
        alone = [k for k in range(12) if cast(dev(o[n:n + 1]), dev(d[n:n + 1]), v, f[k:k + 1].contiguous(), None)[1][0] == t[n]]
        assert len(alone) >= 2 and min(alone) == face[n], (n, alone)
    assert alone == [0, 1, 4, 5, 8, 9]  # the six faces at the corner (0, 0, 0)
    pts = dev(f3([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [2, 2, 2]]))
    assert M().visible(pts, dev(f3([[0.6, 0.4, 0.5], [0.5, 0.5, 2], [3, 3, 3]])), v, f, accel=acc).tolist() == [True, False, True]
    assert M().visible(pts, (0.5, 0.5, 2.0), v, f, accel=acc).tolist() == [False, False, True]


# ---- 2, 3: bitwise against the fp32 restatement, values against fp64 ----------------------------------------------------------------
def build(name):
    if name == "icosphere":
        return E.icosphere(3)
    if name == "torus":
        return R.torus()
    if name == "open":
        return IR.open_icosphere(2, 0.3)
    if name == "salted":
        return IR.salted_icosphere(2)[:2]
    if name == "soup":
        return R.soup(700, seed=5)
    raise KeyError(name)


CASES = ("icosphere", "torus", "open", "salted", "soup")
N_RAYS = 4000


@functools.lru_cache(maxsize=None)
def case(name):
    """The mesh, the rays and both numpy statements, computed once and shared (read-only)."""
    verts, faces = build(name)
    o, d = R.random_rays(N_RAYS, seed=len(name))
    ref32 = R.cast(o, d, verts, faces, dtype=np.float32)
    ref64 = R.cast(o, d, verts, faces, dtype=np.float64)
    for a in (verts, faces, o, d) + ref32 + ref64:
        a.setflags(write=False)
    return verts, faces, o, d, ref32, ref64


@functools.lru_cache(maxsize=None)
def bounded(name):
    verts, faces, o, d = case(name)[:4]
    return R.cast(o, d, verts, faces, 0.25, 1.5, np.float32)


def test_cases_are_what_they_claim():
    assert build("icosphere")[1].shape == (1280, 3) and build("torus")[1].shape == (576, 3) and build("open")[1].shape == (210, 3)
    verts, faces = build("soup")
    assert (faces < 0).any() and (faces >= len(verts)).any() and np.isnan(verts).any()
    verts, faces = build("salted")
    assert (faces < 0).any() and (faces >= len(verts)).any() and np.isnan(verts).any()
    o = case("icosphere")[2]
    r = np.linalg.norm(o, axis=1)
    assert (r < 0.9).sum() > 500 and (r > 1.1).sum() > 500  # origins inside and outside
    for name in CASES:
        hit = case(name)[5][0] >= 0
        assert 0.1 < hit.mean() < 1.0 or name == "icosphere", name


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", CASES)
def test_bits_equal_the_restatement(name, path):
    verts, faces, o, d, ref32, _ = case(name)
    v, f, od, dd = dev(verts), dev(faces), dev(o), dev(d)
    keep = [x.clone() for x in (v, f, od, dd)]
    acc = accel_of(path, v, f)
    got = cast(od, dd, v, f, acc)
    same_bits(got, ref32, f"{name} / {path}")
    assert np.array_equal(M().occluded(od, dd, v, f, accel=acc).cpu().numpy(), got[0] >= 0)
    # a bounded interval too: the structure culls by it
    same_bits(cast(od, dd, v, f, acc, 0.25, 1.5), bounded(name), f"{name} / {path} in [0.25, 1.5)")
    for a, b in zip((v, f, od, dd), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was written"


def deviation(verts, faces, o, d, ref32, ref64):
    """The largest deviation of the fp32 statement from the fp64 one on these inputs: t where both hit, and the barycentrics of the
    fp32 statement's face re-evaluated in fp64."""
    f32_, t32, b32 = ref32
    both = (f32_ >= 0) & (ref64[0] >= 0)
    hit = f32_ >= 0
    on = R.on_face(o[hit], d[hit], verts, faces, f32_[hit], np.float64)
    dev_t = np.abs(t32[both].astype(np.float64) - ref64[1][both]).max() if both.any() else 0.0
    dev_b = np.abs(b32[hit].astype(np.float64) - on["bary"]).max() if hit.any() else 0.0
    return float(max(dev_t, dev_b))


def check_against_fp64(what, verts, faces, o, d, got, ref32, ref64, t_min=0.0, t_max=INF):
    tol = TOL_FACTOR * deviation(verts, faces, o, d, ref32, ref64)
    face, t, bary = got
    f64_, t64, b64 = ref64
    hit = face >= 0
    on = R.on_face(o[hit], d[hit], verts, faces, face[hit], np.float64)
    worst_b = float(-on["bary"].min()) if hit.any() else 0.0
    both = hit & (f64_ >= 0)
    err_t = float(np.abs(t[both].astype(np.float64) - t64[both]).max()) if both.any() else 0.0
    print(f"{what}: tolerance {tol:.3e}; device: most negative fp64 barycentric on its face {max(worst_b, 0):.3e}, "
          f"max |t - t64| {err_t:.3e}; hits device {hit.sum()} fp64 {(f64_ >= 0).sum()}")
    assert tol > 0
    # the fp64 statement on the device's face is a hit
    assert (on["bary"] >= -tol).all() and (on["det"] != 0).all()
    assert ((on["t"] >= t_min - tol) & (on["t"] < t_max + tol)).all()
    assert np.abs(bary[hit].astype(np.float64) - on["bary"]).max() <= tol if hit.any() else True
    # the device's t is the fp64 nearest t
    assert err_t <= tol
    # a miss on one side, a hit on the other: only at an edge or on a grazing face
    lone64 = np.flatnonzero(~hit & (f64_ >= 0))
    if len(lone64):
        det = R.on_face(o[lone64], d[lone64], verts, faces, f64_[lone64], np.float64)["det"]
        assert ((b64[lone64].min(1) <= tol) | (np.abs(det) <= tol)).all()
    lone = np.flatnonzero(hit & (f64_ < 0))
    if len(lone):
        sub = R.on_face(o[lone], d[lone], verts, faces, face[lone], np.float64)
        assert ((sub["bary"].min(1) <= tol) | (np.abs(sub["det"]) <= tol)).all()
    print(f"{what}: {len(lone64)} rays hit only in fp64, {len(lone)} only on the device")


@pytest.mark.parametrize("name", CASES)
def test_values_against_fp64(name):
    verts, faces, o, d, ref32, ref64 = case(name)
    v, f = dev(verts), dev(faces)
    got = cast(dev(o), dev(d), v, f, M().RayMesh(v, f))
    check_against_fp64(name, verts, faces, o, d, got, ref32, ref64)


# ---- 4: watertightness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("subdivisions,origin", [(2, (0.1, -0.2, 0.05)), (2, (0.0, 0.0, 0.0)), (3, (0.1, -0.2, 0.05)), (3, (0.0, 0.0, 0.0))])
def test_watertight(subdivisions, origin, path):
    """tests/test_mesh_ray_host.py's check through the kernel: from inside a closed icosphere, random directions and a direction at
    every vertex and every edge midpoint.  Zero misses."""
    verts, faces = E.icosphere(subdivisions)
    o, d, n_random = R.watertight_rays(verts, faces, origin, 3000, seed=subdivisions)
    v, f = dev(verts), dev(faces)
    acc = accel_of(path, v, f)
    face, t, _ = cast(dev(o), dev(d), v, f, acc)
    print(f"icosphere({subdivisions}) from {origin} / {path}: {len(o)} rays, {(face < 0).sum()} misses")
    assert (face >= 0).all() and np.isfinite(t).all() and (t > 0).all()
    assert M().occluded(dev(o), dev(d), v, f, accel=acc).all()
    V = len(verts)
    assert (faces[face[n_random:n_random + V]] == np.arange(V)[:, None]).any(1).all()  # a face that meets the vertex aimed at


# ---- 5: the structure against the brute force -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere_prefix(F):
    verts, faces = E.icosphere(4 if F > 1280 else 3)
    return verts, np.ascontiguousarray(faces[:F])


@pytest.mark.parametrize("F", [1, 255, 256, 257, 511, 1280, 5120])  # ragged against the chunk of 256
def test_accel_equals_brute_force(F):
    verts, faces = sphere_prefix(F)
    assert len(faces) == F
    v, f = dev(verts), dev(faces)
    mesh = M().RayMesh(v, f)
    lib = pkg("_lib").lib()
    assert mesh.accel.numel() == lib.dgm_ray_accel_bytes(F) == -(-F // 256) * (256 * 48 + 32)
    for seed, (t_min, t_max) in enumerate([(0.0, INF), (0.3, 1.2), (0.0, 0.9)]):  # the structure built once, several batches
        o, d = R.random_rays(3000, seed=F + seed)
        if seed == 2:
            o = (o * 0).astype(np.float32)  # from the centre
        od, dd = dev(o), dev(d)
        brute = cast(od, dd, v, f, None, t_min, t_max)
        same_bits(cast(od, dd, v, f, mesh, t_min, t_max), brute, f"F {F}, batch {seed}")
        assert np.array_equal(M().occluded(od, dd, v, f, t_min, t_max, mesh).cpu().numpy(), brute[0] >= 0)
        assert np.array_equal(M().occluded(od, dd, v, f, t_min, t_max, None).cpu().numpy(), brute[0] >= 0)
        if F >= 1280:
            assert (brute[0] >= 0).sum() > 500
    same_bits(cast(od, dd, None, None, mesh, t_min, t_max), brute, "verts and faces from the RayMesh")


def test_accel_equals_brute_force_on_a_lattice():
    """Unit quads on the integer planes of [0, 6]^3 and axis-parallel rays from origins exactly on lattice planes and lines: the rays
    run inside faces, along edges, through vertices and along the faces of the chunk boxes, with direction components of exactly 0."""
    verts, faces = R.lattice(6)
    o, d = R.lattice_rays(6)
    assert len(faces) == 1512 and len(o) == 6 * 5 * 169 and (d == 0).sum() == 2 * len(d)
    v, f, od, dd = dev(verts), dev(faces), dev(o), dev(d)
    mesh = M().RayMesh(v, f)
    for t_min, t_max in [(0.0, INF), (1.0, 3.0), (0.5, 2.0)]:
        brute = cast(od, dd, v, f, None, t_min, t_max)
        same_bits(cast(od, dd, v, f, mesh, t_min, t_max), brute, f"lattice [{t_min}, {t_max})")
        assert np.array_equal(M().occluded(od, dd, v, f, t_min, t_max, mesh).cpu().numpy(), brute[0] >= 0)
    face, t, _ = brute
    same_bits(brute, R.cast(o, d, verts, faces, 0.5, 2.0, np.float32), "lattice against the restatement")
    full = cast(od, dd, v, f, mesh)
    assert (full[0] >= 0).sum() > 0.7 * len(o)  # (two of the ten families of rays point away from the lattice)


# ---- 6: batch and order independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_batch_and_order_independence(path):
    verts, faces, o, d, ref32, _ = case("torus")
    v, f = dev(verts), dev(faces)
    acc = accel_of(path, v, f)
    whole = cast(dev(o), dev(d), v, f, acc)
    same_bits(cast(dev(o), dev(d), v, f, acc), whole, "a second run")
    perm = np.random.default_rng(1).permutation(len(o))
    got = cast(dev(o[perm]), dev(d[perm]), v, f, acc)
    same_bits(got, tuple(a[perm] for a in whole), "a permuted batch")
    for n in (0, 255, 256, 1777):
        same_bits(cast(dev(o[n:n + 1]), dev(d[n:n + 1]), v, f, acc), tuple(a[n:n + 1] for a in whole), f"ray {n} alone")
    same_bits(cast(dev(o[300:1000]), dev(d[300:1000]), v, f, acc), tuple(a[300:1000] for a in whole), "a part")


# ---- 7: edge cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_edge_cases(path):
    verts, faces = E.icosphere(2)
    v, f = dev(verts), dev(faces)
    acc = accel_of(path, v, f)
    miss = lambda got, n: (got[0] == -1).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and len(got[0]) == n
    none = torch.zeros((0, 3), device=DEV)
    assert miss(cast(none, none, v, f, acc), 0) and M().occluded(none, none, v, f, accel=acc).shape == (0,)
    o, d = dev(f3([[0, 0, 0]] * 4)), dev(f3([[1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1]]))
    assert (cast(o, d, v, f, acc)[0] >= 0).all()
    no_f, no_v = torch.zeros((0, 3), dtype=torch.int32, device=DEV), torch.zeros((0, 3), device=DEV)
    for vv, ff in ((v, no_f), (no_v, f), (no_v, no_f)):  # F = 0, V = 0, both
        a = accel_of(path, vv, ff)
        assert miss(cast(o, d, vv, ff, a), 4) and not M().occluded(o, d, vv, ff, accel=a).any()
    bad_o = dev(f3([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]))
    bad_d = dev(f3([[1, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 1, 0], [0, -np.inf, 0], [0, 0, 1]]))
    got = cast(bad_o, bad_d, v, f, acc)
    assert miss(tuple(a[:5] for a in got), 5) and got[0][5] >= 0
    assert M().occluded(bad_o, bad_d, v, f, accel=acc).tolist() == [False] * 5 + [True]
    for t_min, t_max in ((1.0, 1.0), (2.0, 1.0), (math.nan, INF), (0.0, math.nan), (0.0, 0.0), (INF, INF)):  # t_max <= t_min, NaN bounds
        assert miss(cast(o, d, v, f, acc, t_min, t_max), 4) and not M().occluded(o, d, v, f, t_min, t_max, acc).any()
    # non-contiguous inputs
    wide_o, wide_d = torch.zeros((4, 6), device=DEV), torch.zeros((4, 6), device=DEV)
    wide_d[:, ::2] = d
    same_bits(cast(wide_o[:, ::2], wide_d[:, ::2], v, f, acc), cast(o, d, v, f, acc), "strided rays")
    wide_v = torch.zeros((len(verts), 5), device=DEV)
    wide_v[:, 1:4] = v
    same_bits(cast(o, d, wide_v[:, 1:4], f.t().contiguous().t(), None), cast(o, d, v, f, None), "strided mesh")
    # wrong dtype, device, shape, accel
    with pytest.raises(RuntimeError, match="origins must be torch.float32"):
        M().ray_cast(o.double(), d, v, f, accel=acc)
    with pytest.raises(RuntimeError, match="faces must be torch.int32"):
        M().ray_cast(o, d, v, f.long(), accel=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M().ray_cast(o.cpu(), d, v, f, accel=acc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M().occluded(o, d.cpu(), v, f, accel=acc)
    with pytest.raises(ValueError, match=r"must be \(n, 3\)"):
        M().ray_cast(o[:, :2], d, v, f, accel=acc)
    with pytest.raises(ValueError, match="differ"):
        M().ray_cast(o[:2], d, v, f, accel=acc)
    with pytest.raises(TypeError, match="accel must be"):
        M().ray_cast(o, d, v, f, accel="bvh")
    with pytest.raises(ValueError, match="another mesh"):
        M().ray_cast(o, d, v[:5], f, accel=M().RayMesh(v, f))


def test_auto_switches_at_the_threshold_and_changes_nothing(monkeypatch):
    verts, faces, o, d, ref32, _ = case("icosphere")
    v, f, od, dd = dev(verts), dev(faces), dev(o), dev(d)
    built = []

    class Counting(M().RayMesh):
        def __init__(self, *a):
            built.append(1)
            super().__init__(*a)

    monkeypatch.setattr(M(), "RayMesh", Counting)
    monkeypatch.setattr(M(), "AUTO_MIN_FACES", 1281)
    same_bits(cast(od, dd, v, f, "auto"), ref32, "auto below the threshold")
    assert not built
    monkeypatch.setattr(M(), "AUTO_MIN_FACES", 1280)
    same_bits(cast(od, dd, v, f, "auto"), ref32, "auto at the threshold")
    assert built == [1]


# ---- 8: the depth map against the mesh rasterizer -------------------------------------------------------------------------------------
def test_depth_map_against_the_rasterizer():
    syn, S, MR = pkg("synthetic"), pkg("scene"), pkg("mesh_raster")
    verts, faces = E.icosphere(3)
    H = W = 64
    cam = S.TorchCamera(syn.make_camera(W, H, azimuth=0.3, elevation=0.35, radius=3.2), DEV)
    v, f = dev(verts), dev(faces)
    depth, fid = M().depth_map(cam, v, f)
    assert depth.shape == (H, W) and fid.shape == (H, W) and depth.dtype == torch.float32 and fid.dtype == torch.int32
    o, d = M().camera_rays(cam)
    assert o.shape == (H * W, 3) and d.shape == (H * W, 3)
    view_z = (torch.cat([d, torch.zeros_like(d[:, :1])], dim=1) @ cam.world_view_transform)[:, 2]
    assert float((view_z - 1).abs().max()) < 1e-6  # t is the view-space depth
    same_bits(cast(o, d, v, f, None), (fid.reshape(-1).cpu().numpy(), depth.reshape(-1).cpu().numpy(), cast(o, d, v, f, None)[2]), "depth_map")
    # the rasterizer
    rast, _ = MR.rasterize(None, MR.clip_positions(cam, v), f, (H, W))
    rid = rast[0, ..., 3].round().int().cpu().numpy() - 1
    zv = (torch.cat([v, torch.ones_like(v[:, :1])], dim=1) @ cam.world_view_transform)[:, 2:3].contiguous()
    rdepth = MR.interpolate(zv, rast, f)[0][0, ..., 0].cpu().numpy()
    got_id, got_depth = fid.cpu().numpy(), depth.cpu().numpy()
    both = (rid >= 0) & (got_id >= 0)
    only = ((rid >= 0) ^ (got_id >= 0)).sum()
    assert both.sum() > 700 and np.isposinf(got_depth[got_id < 0]).all()
    # the fp64 statement at the pixel centres: which pixels have their centre on an edge
    o_h, d_h = o.cpu().numpy(), d.cpu().numpy()
    ref64 = R.cast(o_h, d_h, verts, faces, dtype=np.float64)
    ref32 = R.cast(o_h, d_h, verts, faces, dtype=np.float32)
    covered = ref64[0] >= 0
    on_edge = covered & (np.abs(ref64[2]).min(1) < 1e-4)
    print(f"depth_map: {both.sum()} pixels covered by both, {only} by one only; {on_edge.sum()} of {covered.sum()} centres within 1e-4 of an edge")
    assert on_edge.sum() <= 0.01 * covered.sum()  # the camera keeps the reference within the allowance
    differ = both & (rid != got_id)
    print(f"depth_map: {differ.sum()} pixels with another face than the rasterizer's")
    assert not (differ.reshape(-1) & ~on_edge).any()
    tol = TOL_FACTOR * deviation(verts, faces, o_h, d_h, ref32, ref64)
    err = np.abs(got_depth[both].astype(np.float64) - rdepth[both]).max()
    err64 = np.abs(got_depth.reshape(-1)[covered & (got_id.reshape(-1) >= 0)] - ref64[1][covered & (got_id.reshape(-1) >= 0)]).max()
    print(f"depth_map: max |depth - rasterizer's interpolated depth| {err:.3e}, |depth - fp64 t| {err64:.3e}, tolerance {tol:.3e}")
    assert err64 <= tol
    assert err <= tol


# ---- 9: ambient occlusion -------------------------------------------------------------------------------------------------------------
def quad(p0, e1, e2):
    p0, e1, e2 = (np.asarray(x, np.float64) for x in (p0, e1, e2))
    return f3([p0, p0 + e1, p0 + e1 + e2, p0 + e2]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def near_edge(o, d, verts, faces, tol, t_max):
    """Rays that the fp64 statement puts within tol of an edge of some face in range (or on a grazing face): their hit may flip."""
    corners, ok = R.face_corners(verts, faces)
    out = np.zeros(len(o), bool)
    for r0 in range(0, len(o), R.RAY_BLOCK):
        p = R.pair(o[r0:r0 + R.RAY_BLOCK], d[r0:r0 + R.RAY_BLOCK], corners[None], np.float64)
        with np.errstate(all="ignore"):
            b = np.stack([p[k] / p["det"] for k in ("U", "V", "W")], axis=-1)
            close = ok[None] & (p["t"] >= -tol) & (p["t"] < t_max + tol) & (b.min(-1) >= -tol) & ((b.min(-1) <= tol) | (np.abs(p["det"]) <= tol))
        out[r0:r0 + R.RAY_BLOCK] = close.any(1)
    return out


def ao_case(points, normals, verts, faces, samples, max_dist=INF, seed=0, accel=None):
    """ambient_occlusion on the device, and the count of the same rays by the fp64 statement; -> the device's values."""
    p, n, v, f = dev(f3(points)), dev(f3(normals)), dev(verts), dev(faces)
    ao = M().ambient_occlusion(p, n, v, f, samples, max_dist, None, seed, accel)
    assert ao.shape == (len(p),) and ao.dtype == torch.float32
    again = M().ambient_occlusion(p, n, v, f, samples, max_dist, None, seed, M().RayMesh(v, f))
    assert torch.equal(ao, again)  # deterministic, and the same on both paths
    o = M().ao_origins(p, n, v)[:, None, :].expand(-1, samples, -1).reshape(-1, 3).cpu().numpy()
    d = M().ao_directions(n, samples, seed).reshape(-1, 3).cpu().numpy()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (np.einsum("ij,ij->i", d.reshape(len(p), samples, 3).reshape(-1, 3), np.repeat(f3(normals), samples, 0)) >= -1e-6).all()
    ref32 = R.cast(o, d, verts, faces, 0.0, max_dist, np.float32)
    ref64 = R.cast(o, d, verts, faces, 0.0, max_dist, np.float64)
    tol = TOL_FACTOR * max(deviation(verts, faces, o, d, ref32, ref64), float(np.finfo(np.float32).eps))
    got = ao.cpu().numpy().astype(np.float64)
    count = 1.0 - (ref64[0] >= 0).reshape(len(p), samples).mean(1)
    shaky = near_edge(o, d, verts, faces, tol, max_dist).reshape(len(p), samples).sum(1)
    print(f"ambient occlusion: {len(p)} points x {samples} rays, {shaky.sum()} rays within {tol:.1e} of an edge; "
          f"max |device - fp64 count| {np.abs(got - count).max():.4f}")
    assert (np.abs(got - count) * samples <= shaky + 1e-9).all()
    assert (got >= 0).all() and (got <= 1).all()
    return got


def test_ambient_occlusion_known_values():
    # on top of a lone plane: nothing above
    plane = quad([-5, -5, 0], [10, 0, 0], [0, 10, 0])
    pts = [[0, 0, 0], [1.5, -2, 0], [-3, 3, 0]]
    assert (ao_case(pts, [[0, 0, 1]] * 3, *plane, 64) == 1).all()
    assert (ao_case(pts, [[0, 0, 2]] * 3, *plane, 16, max_dist=0.5) == 1).all()
    # the floor centre inside a closed box: everything is covered
    box = R.cube()
    assert (ao_case([[0.5, 0.5, 0]], [[0, 0, 1]], *box, 64) == 0).all()
    assert (ao_case([[0.5, 0.5, 0]], [[0, 0, 1]], *box, 64, max_dist=0.25) == 1).all()  # the lid and the walls are farther
    # at the foot of a tall wall on a floor: the wall covers the half of the hemisphere behind it, cosine-weighted 1/2
    floor = quad([-2000, -2000, 0], [4000, 0, 0], [0, 4000, 0])
    wall = quad([0, -2000, 0], [0, 4000, 0], [0, 0, 2000])
    verts, faces = IR.join(floor, wall)
    samples = 64
    foot = [[1e-3, y, 0] for y in (-3.0, 0.0, 0.7, 2.5, 11.0, -40.0)]
    got = ao_case(foot, [[0, 0, 1]] * len(foot), verts, faces, samples, seed=3)
    print(f"wall: ambient occlusion at the foot {got}")
    assert (np.abs(got - 0.5) <= 3 * math.sqrt(0.25 / samples)).all()
    got = ao_case(foot, [[0, 0, 1]] * len(foot), verts, faces, 256, seed=4)
    assert (np.abs(got - 0.5) <= 3 * math.sqrt(0.25 / 256)).all()
    # another seed is another rotation
    a = M().ao_directions(dev(f3([[0, 0, 1]] * 4)), 8, seed=0)
    b = M().ao_directions(dev(f3([[0, 0, 1]] * 4)), 8, seed=1)
    assert not torch.equal(a, b) and not torch.equal(a[0], a[1])
    assert torch.equal(M().ao_directions(dev(f3([[0, 0, 1]] * 4)), 8, seed=0, start=2)[:2], a[2:])  # a point's rotation follows its index


def test_vertex_ambient_occlusion_of_a_sphere():
    verts, faces = E.icosphere(2)
    v, f = dev(verts), dev(faces)
    ao = M().vertex_ambient_occlusion(v, f, samples=32)
    assert ao.shape == (len(verts),) and (ao == 1).all()
    rev = dev(IR.reversed_faces(faces))
    assert (M().vertex_ambient_occlusion(v, rev, samples=32, flip=True) == 1).all()
    inside = M().vertex_ambient_occlusion(v, rev, samples=32)  # the inward normals look into the closed ball
    assert (inside == 0).all()
    with pytest.raises(ValueError, match="samples must be >= 1"):
        M().vertex_ambient_occlusion(v, f, samples=0)


# ---- 10: the texture path ---------------------------------------------------------------------------------------------------------------
def colours_of(verts):
    return (0.5 + 0.5 * np.sin(verts.astype(np.float64) * [3.0, 5.0, 7.0])).astype(np.float32)


def files_of(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


@pytest.mark.parametrize("ext", ["obj", "glb"])
def test_texture_path(ext, tmp_path, capsys):
    MT, PLY = pkg("mesh_texture"), pkg("ply_io")
    verts, faces = R.torus()
    v, f = dev(verts), dev(faces)
    src = str(tmp_path / "in.ply")
    PLY.write_mesh_ply(src, verts, faces, vertex_colors=colours_of(verts))
    _, _, rgba = PLY.read_mesh_ply(src, return_colors=True)
    col = dev((rgba[:, :3].astype(np.float32) + np.float32(0.5)) / np.float32(255.0))
    # ao 0: the bytes of the path without it (bake_vertex_colors and write_textured, which this feature leaves alone)
    tex, uv, atlas = MT.bake_vertex_colors(v, f, col, cell=6)
    os.makedirs(tmp_path / "plain")
    MT.write_textured(str(tmp_path / "plain" / "torus"), ext, verts, faces, uv, tex)
    assert MT.main([src, str(tmp_path / "zero" / f"torus.{ext}"), "--cell", "6", "--ao", "0"]) == 0
    assert MT.main([src, str(tmp_path / "none" / f"torus.{ext}"), "--cell", "6"]) == 0
    plain = files_of(tmp_path / "plain")
    assert len(plain) == (3 if ext == "obj" else 1) and files_of(tmp_path / "zero") == plain and files_of(tmp_path / "none") == plain
    assert MT.apply_ambient_occlusion(tex, v, f, MT.TextureSpec(cell=6, format=ext), cell=6) is tex
    assert MT.TextureSpec(cell=6).describe() == "cell 6 format obj" and MT.TextureSpec(cell=6, ao_samples=16).describe() == "cell 6 format obj ao 16"
    # ao 16: colour x bake_ambient_occlusion
    ao, uv2, atlas2 = MT.bake_ambient_occlusion(v, f, cell=6, samples=16)
    assert ao.shape == (atlas.size, atlas.size, 1) and atlas2 == atlas and torch.equal(uv2, uv)
    assert float(ao.min()) >= 0 and float(ao.max()) == 1 and float(ao.min()) < 0.9  # the hole of the torus is shadowed
    assert torch.equal(MT.bake_ambient_occlusion(v, f, cell=6, samples=16, accel=None)[0], ao)
    spec = MT.as_spec({"cell": 6, "format": ext, "ao_samples": 16})
    shaded = MT.apply_ambient_occlusion(tex, v, f, spec, **spec.atlas_args())
    assert torch.equal(shaded, tex * ao)
    os.makedirs(tmp_path / "expected")
    MT.write_textured(str(tmp_path / "expected" / "torus"), ext, verts, faces, uv, tex * ao)
    capsys.readouterr()
    assert MT.main([src, str(tmp_path / "ao" / f"torus.{ext}"), "--cell", "6", "--ao", "16"]) == 0
    assert "F 576" in capsys.readouterr().out
    assert files_of(tmp_path / "ao") == files_of(tmp_path / "expected") and files_of(tmp_path / "ao") != plain
    # per texel: the owning face's normal and the interpolated position, the texel's rank among the owned ones as the point's index
    pos, face_id = MT.atlas_interpolate(atlas, v, f)
    owned = (face_id.reshape(-1) >= 0).nonzero().reshape(-1)
    corner = v[f[face_id.reshape(-1)[owned].long()].long()]
    normal = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    direct = M().ambient_occlusion(pos.reshape(-1, 3)[owned].contiguous(), normal, v, f, 16)
    assert torch.equal(ao.reshape(-1)[owned], direct) and (ao.reshape(-1)[face_id.reshape(-1) < 0] == 1).all()


def test_vertex_ao_command_line(tmp_path, capsys):
    PLY = pkg("ply_io")
    verts, faces = R.torus()
    # tilted: on the torus as built, the vertices of the two equators have a normal whose z is rounding noise of either sign (the vertex
    # normals sum with atomics), and the sign of z picks the half of the frame about the normal -- another rotation of the same set
    ca, sa, cb, sb = math.cos(0.37), math.sin(0.37), math.cos(0.51), math.sin(0.51)
    tilt = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    verts = (verts.astype(np.float64) @ tilt.T).astype(np.float32)
    plain, coloured = str(tmp_path / "plain.ply"), str(tmp_path / "coloured.ply")
    PLY.write_mesh_ply(plain, verts, faces)
    PLY.write_mesh_ply(coloured, verts, faces, vertex_colors=colours_of(verts))
    ao = M().vertex_ambient_occlusion(dev(verts), dev(faces), samples=16).cpu().numpy()
    assert ao.min() < 0.9 and ao.max() == 1
    assert M().main([plain, "--ao", str(tmp_path / "grey.ply"), "--samples", "16"]) == 0
    assert "V 288 F 576  samples 16" in capsys.readouterr().out
    v2, f2, grey = PLY.read_mesh_ply(str(tmp_path / "grey.ply"), return_colors=True)
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all() and (grey[:, 3] == 255).all()
    assert np.abs(grey[:, 0].astype(np.float64) - np.floor(np.clip(ao.astype(np.float64) * 255, 0, 255))).max() <= 1  # (vertex normals sum with atomics)
    assert M().main([coloured, "--ao", str(tmp_path / "shaded.ply"), "--samples", "16"]) == 0
    _, _, base = PLY.read_mesh_ply(coloured, return_colors=True)
    _, _, shaded = PLY.read_mesh_ply(str(tmp_path / "shaded.ply"), return_colors=True)
    assert (shaded[:, :3] <= base[:, :3]).all() and np.array_equal(shaded[ao == 1, :3], base[ao == 1, :3]) and (shaded[:, :3] < base[:, :3]).any()


def test_export_dynamic_mesh_with_ambient_occlusion(scene, tmp_path):  # noqa: F811
    """TextureSpec(ao_samples=N) multiplies every frame's baked texture by its ambient occlusion; ao_samples=0 writes the bytes of a
    spec without the field (on the same DPSR fields, as tests/test_mesh_texture.py replays them)."""
    V, O, MS, MT = pkg("visualize"), pkg("obj_io"), pkg("mesh_simplify"), pkg("mesh_texture")
    args = (scene["g"], scene["deform"], scene["deform_back"], scene["mesh"])
    m = scene["mesh"]
    fields, orig = _record_psr(m)
    try:
        V.export_dynamic_mesh(*args, str(tmp_path / "plain"), frames=1, simplify=MS.SimplifySpec(grid=12), texture={"cell": 6})
        for name, spec in (("zero", MT.TextureSpec(size=None, cell=6, ao_samples=0)), ("ao", {"cell": 6, "ao_samples": 8})):
            replay = iter(list(fields[:1]))
            m.psr = lambda *a, **k: next(replay)
            V.export_dynamic_mesh(*args, str(tmp_path / name), frames=1, simplify=MS.SimplifySpec(grid=12), texture=spec)
    finally:
        m.psr = orig
    plain = files_of(tmp_path / "plain" / "dynamic_mesh_textured")
    assert len(plain) == 3 and files_of(tmp_path / "zero" / "dynamic_mesh_textured") == plain
    v0, f0, uv0, tex0 = O.read_mesh_obj(str(tmp_path / "plain" / "dynamic_mesh_textured" / "frame_0.obj"))
    v1, f1, uv1, tex1 = O.read_mesh_obj(str(tmp_path / "ao" / "dynamic_mesh_textured" / "frame_0.obj"))
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1) and np.array_equal(uv0, uv1) and tex0.shape == tex1.shape
    ao = MT.bake_ambient_occlusion(dev(v0), dev(f0), cell=6, samples=8)[0].cpu().numpy().astype(np.float64)
    assert (tex1 <= tex0).all() and (tex1 < tex0).any()
    assert np.abs(tex1 - tex0 * ao).max() <= 1.0  # one step of the bytes: the file holds the colour's bytes, the product was taken before
