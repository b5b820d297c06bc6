"""CPU-side tests of ray casting against a mesh (dg-mesh_amd/mesh_ray.py, csrc/mesh_ray.hip): the numpy restatement of the GPU tests
(tests/_ray_ref.py) gives the known answers on hand-made meshes, obeys the never-hit rules and is watertight on icospheres; the C
ABI declares and exports the new entry points, its size functions are pure and monotone, and it refuses bad arguments before any
HIP call; the Python layer refuses host tensors and bad parameters; the command lines parse."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _edges_ref as E
import _ray_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ("dgm_ray_accel_bytes", "dgm_ray_build_scratch_bytes", "dgm_ray_build", "dgm_ray_cast", "dgm_ray_occluded")
BOTH = (np.float32, np.float64)
TRI = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))


def f32(a):
    return np.asarray(a, np.float32).reshape(-1, 3)


# ---- the restatement against known answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
def test_reference_one_triangle(dtype):
    verts, faces = TRI
    o = f32([[0.25, 0.25, 2], [1.5, 0.25, 2], [0.25, 0.25, 2], [0.25, 0.25, 0], [-1, 0.25, 0]])
    d = f32([[0, 0, -1], [0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0]])  # hit, beside, behind the origin, two rays in the plane
    face, t, bary = R.cast(o, d, verts, faces, dtype=dtype)
    assert t.dtype == dtype and bary.dtype == dtype and face.dtype == np.int32
    assert face.tolist() == [0, -1, -1, -1, -1]
    assert t[0] == 2 and (bary[0] == [0.5, 0.25, 0.25]).all()
    assert np.isinf(t[1:]).all() and (bary[1:] == 0).all()
    # a direction twice as long: t halves (t is in units of |d|)
    assert R.cast(o[:1], d[:1] * 2, verts, faces, dtype=dtype)[1][0] == 1
    # t_min is inclusive, t_max exclusive
    assert R.cast(o[:1], d[:1], verts, faces, 2.0, 3.0, dtype)[0][0] == 0
    assert R.cast(o[:1], d[:1], verts, faces, 1.0, 2.0, dtype)[0][0] == -1
    assert R.cast(o[:1], d[:1], verts, faces, 2.0, 2.0, dtype)[0][0] == -1
    assert R.cast(o[:1], d[:1], verts, faces, np.nextafter(np.float32(2), np.float32(3)), 9.0, dtype)[0][0] == -1


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_cube_shared_edges_and_corners(dtype):
    verts, faces = R.cube()
    # through a side's diagonal (faces 2k, 2k + 1 share it), through an edge of the cube, through a corner: the lowest index of those hit
    o = f32([[-1, 0.5, 0.5], [0.5, 0.5, 3], [-1, -1, 0.5], [-1, -1, -1]])
    d = f32([[1, 0, 0], [0, 0, -1], [1, 1, 0], [1, 1, 1]])
    face, t, _ = R.cast(o, d, verts, faces, dtype=dtype)
    assert face.tolist() == [0, 10, 0, 0] and t.tolist() == [1, 2, 1, 1]
    for n in range(4):  # every face that contains the hit point is accepted with the same t
        acc = [k for k in range(12) if R.cast(o[n:n + 1], d[n:n + 1], verts, faces[k:k + 1], dtype=dtype)[0][0] == 0
               and R.cast(o[n:n + 1], d[n:n + 1], verts, faces[k:k + 1], dtype=dtype)[1][0] == t[n]]
        assert len(acc) >= 2 and min(acc) == face[n], (n, acc)
    # from inside, every direction hits
    oi, di = np.full((500, 3), 0.5, np.float32), R.random_rays(500, 1)[1]
    assert (R.cast(oi, di, verts, faces, dtype=dtype)[0] >= 0).all()


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_never_hit_rules(dtype):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float32)
    o, d = f32([[0.2, 0.2, 1]]), f32([[0, 0, -1]])
    assert R.cast(o, d, verts, [[0, 1, 2]], dtype=dtype)[0][0] == 0
    for bad in ([[0, 1, 5]], [[-1, 1, 2]], [[0, 1, 3]], [[0, 4, 2]], [[0, 1, 1]], [[2, 2, 2]]):
        face, t, bary = R.cast(o, d, verts, bad, dtype=dtype)
        assert face[0] == -1 and np.isinf(t[0]) and (bary == 0).all(), bad
    # rays that test nothing
    bad_o = f32([[np.nan, 0.2, 1], [0.2, np.inf, 1], [0.2, 0.2, 1], [0.2, 0.2, 1], [0.2, 0.2, 1]])
    bad_d = f32([[0, 0, -1], [0, 0, -1], [0, 0, 0], [np.nan, 0, -1], [0, -np.inf, -1]])
    assert (R.cast(bad_o, bad_d, verts, [[0, 1, 2]], dtype=dtype)[0] == -1).all()
    # no faces, no vertices
    assert R.cast(o, d, verts, np.zeros((0, 3), np.int32), dtype=dtype)[0][0] == -1
    assert R.cast(o, d, np.zeros((0, 3), np.float32), [[0, 1, 2]], dtype=dtype)[0][0] == -1
    salted_v, salted_f, salt = __import__("_inside_ref").salted_icosphere(2)
    oo, dd = R.random_rays(300, 2)
    face = R.cast(oo, dd, salted_v, salted_f, dtype=dtype)[0]
    never = np.flatnonzero((salted_f[:, None, :] == salt[None, :5, :]).all(2).any(1))
    assert len(never) == 5 and not np.isin(face, never).any() and (face >= 0).any()


def test_reference_is_independent_of_the_batch_and_the_fallback_runs():
    verts, faces = E.icosphere(2)
    o, d = R.random_rays(600, 3)
    face, t, bary = R.cast(o, d, verts, faces)
    perm = np.random.default_rng(0).permutation(600)
    f2, t2, b2 = R.cast(o[perm], d[perm], verts, faces)
    assert (f2 == face[perm]).all() and (t2.view(np.uint32) == t[perm].view(np.uint32)).all() and (b2.view(np.uint32) == bary[perm].view(np.uint32)).all()
    f1, t1, _ = R.cast(o[7:8], d[7:8], verts, faces)
    assert f1[0] == face[7] and t1.view(np.uint32)[0] == t.view(np.uint32)[7]
    # a ray through a vertex of the lattice has exact zeros among its edge values: the fp64 fallback decides
    lv, lf = R.lattice(2)
    lo, ld = R.lattice_rays(2)
    p = R.pair(lo[:50], ld[:50], R.face_corners(lv, lf)[0][None], np.float32)
    assert ((p["U"] == 0) | (p["V"] == 0) | (p["W"] == 0)).any()


def watertight_case(subdivisions, origin):
    verts, faces = E.icosphere(subdivisions)
    return (verts, faces) + R.watertight_rays(verts, faces, origin, 3000, seed=subdivisions)


WATERTIGHT = [(2, (0.1, -0.2, 0.05)), (2, (0.0, 0.0, 0.0)), (3, (0.1, -0.2, 0.05)), (3, (0.0, 0.0, 0.0))]


@pytest.mark.parametrize("subdivisions,origin", WATERTIGHT)
def test_reference_is_watertight(subdivisions, origin):
    """From inside a closed icosphere no ray may miss: random directions, and a direction at every vertex and every edge midpoint,
    where a ray runs along shared edges.  Zero misses in fp32 and in fp64; on the random rays both choose the same face, on the
    aimed ones a face that meets the vertex or edge."""
    verts, faces, o, d, n_random = watertight_case(subdivisions, origin)
    assert len(faces) == (320 if subdivisions == 2 else 1280) and len(o) == n_random + len(verts) + len(faces) * 3 // 2
    f32_, t32, _ = R.cast(o, d, verts, faces, dtype=np.float32)
    f64_, t64, _ = R.cast(o, d, verts, faces, dtype=np.float64)
    print(f"icosphere({subdivisions}) from {origin}: {len(o)} rays, misses fp32 {(f32_ < 0).sum()} fp64 {(f64_ < 0).sum()}, "
          f"max relative |t32 - t64| {np.abs((t32 - t64) / t64).max():.2e}")
    assert (f32_ >= 0).all() and (f64_ >= 0).all()
    assert (f32_[:n_random] == f64_[:n_random]).all()
    assert np.abs((t32 - t64) / t64).max() < 1e-6
    # aimed rays: the chosen face contains the target vertex, or both ends of the target edge
    V = len(verts)
    aimed_v = f32_[n_random:n_random + V]
    assert (faces[aimed_v] == np.arange(V)[:, None]).any(1).all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    for name in NEW_SYMBOLS[:2]:
        assert re.search(rf"^size_t\s+{name}\s*\(", header, flags=re.M)
    assert L.ABI_VERSION == 5 and lib.dgm_abi_version() == 5
    assert "dgm_ray_*" in header[header.index("ABI history"):header.index("#define DGM_ABI_VERSION")]


def test_size_functions_are_pure_and_monotone():
    lib = pkg("_lib").lib()
    for size in (lib.dgm_ray_accel_bytes, lib.dgm_ray_build_scratch_bytes):
        assert size(-1) == 0 and size(-2 ** 31) == 0
        sizes = [size(F) for F in (0, 1, 255, 256, 257, 511, 512, 513, 5120, 261176, 10 ** 7, 2 ** 31 - 257)]
        assert sizes == [size(F) for F in (0, 1, 255, 256, 257, 511, 512, 513, 5120, 261176, 10 ** 7, 2 ** 31 - 257)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0
        assert size(2 ** 31 - 256) == 0  # an unsupported size
    accel = lib.dgm_ray_accel_bytes
    assert accel(0) == 0 and accel(1) == accel(256) == 256 * 48 + 32 and accel(257) == 2 * (256 * 48 + 32)
    assert accel(2 ** 31 - 257) == (2 ** 23 - 1) * (256 * 48 + 32)  # size_t arithmetic


def test_c_abi_argument_errors_without_gpu():
    lib = pkg("_lib").lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    err = lambda: lib.dgm_last_error()
    inf = math.inf
    cast = lambda N, V, F, o, d, v, f, acc, face, t, bary: lib.dgm_ray_cast(N, V, F, o, d, 0.0, inf, v, f, acc, face, t, bary, None)
    occ = lambda N, V, F, o, d, v, f, acc, hit: lib.dgm_ray_occluded(N, V, F, o, d, 0.0, inf, v, f, acc, hit, None)
    assert cast(-1, 1, 1, p, p, p, p, None, p, p, p) != 0 and b"ray_cast" in err() and b"N >= 0" in err()
    assert cast(1, -1, 1, p, p, p, p, None, p, p, p) != 0 and b"V >= 0" in err()
    assert cast(1, 1, -1, p, p, p, p, None, p, p, p) != 0 and b"F >= 0" in err()
    assert cast(1, 1, 2 ** 31 - 1, p, p, p, p, None, p, p, p) != 0 and b"too many faces" in err()
    assert cast(0, 4, 2, None, None, None, None, None, None, None, None) == 0  # nothing to do
    for args in ((None, p, p, p, None, p, p, p), (p, None, p, p, None, p, p, p), (p, p, None, p, None, p, p, p), (p, p, p, None, None, p, p, p),
                 (p, p, p, p, None, None, p, p), (p, p, p, p, None, p, None, p), (p, p, p, p, None, p, p, None)):
        assert cast(4, 3, 1, *args) != 0 and b"NULL pointer" in err()
    assert cast(4, 3, 1, p, p, p, p, odd, p, p, p) != 0 and b"16-byte aligned" in err()
    assert occ(-1, 1, 1, p, p, p, p, None, p) != 0 and b"ray_occluded" in err() and b"N >= 0" in err()
    assert occ(4, 3, 1, p, p, p, p, None, None) != 0 and b"NULL pointer" in err()
    assert occ(4, 3, 1, p, p, p, p, odd, p) != 0 and b"16-byte aligned" in err()
    assert occ(0, 3, 1, None, None, None, None, None, None) == 0
    build = lambda V, F, v, f, scratch, acc: lib.dgm_ray_build(V, F, v, f, scratch, acc, None)
    assert build(-1, 1, p, p, p, p) != 0 and b"V >= 0" in err()
    assert build(1, -1, p, p, p, p) != 0 and b"F >= 0" in err()
    assert build(1, 2 ** 31 - 1, p, p, p, p) != 0 and b"too many faces" in err()
    assert build(3, 0, None, None, None, None) == 0  # nothing to do
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert build(3, 1, *args) != 0 and b"NULL pointer" in err()
    assert build(3, 1, p, p, p, odd) != 0 and b"16-byte aligned" in err()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_host_tensors_and_bad_parameters():
    M = pkg("mesh_ray")
    o, verts, faces = torch.zeros(5, 3), torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    for call in (lambda: M.ray_cast(o, o, verts, faces), lambda: M.ray_cast(o, o, verts, faces, accel=None), lambda: M.occluded(o, o, verts, faces),
                 lambda: M.RayMesh(verts, faces), lambda: M.visible(o, (0, 0, 1), verts, faces), lambda: M.ambient_occlusion(o, o, verts, faces),
                 lambda: M.vertex_ambient_occlusion(verts, faces), lambda: pkg("mesh_texture").bake_ambient_occlusion(verts, faces, size=64)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    sig = inspect.signature
    assert [(k, v.default) for k, v in sig(M.ray_cast).parameters.items()][4:] == [("t_min", 0.0), ("t_max", math.inf), ("accel", "auto")]
    assert [(k, v.default) for k, v in sig(M.occluded).parameters.items()][4:] == [("t_min", 0.0), ("t_max", math.inf), ("accel", "auto")]
    assert [(k, v.default) for k, v in sig(M.ambient_occlusion).parameters.items()][4:] == [
        ("samples", 64), ("max_dist", math.inf), ("offset", None), ("seed", 0), ("accel", "auto")]
    assert [(k, v.default) for k, v in sig(M.vertex_ambient_occlusion).parameters.items()][2:] == [
        ("samples", 64), ("max_dist", math.inf), ("offset", None), ("seed", 0), ("flip", False), ("accel", "auto")]
    assert "N x F" in " ".join(M.__doc__.split())
    T = pkg("mesh_texture")
    assert T.TextureSpec().ao_samples == 0 and T.as_spec({"ao_samples": 16}).ao_samples == 16
    with pytest.raises(ValueError, match="ao_samples"):
        T.as_spec({"ao_samples": -1})


def test_command_lines_parse():
    M, T = pkg("mesh_ray"), pkg("mesh_texture")
    ap = M.build_parser()
    a = ap.parse_args(["mesh.ply", "--ao", "out.ply"])
    assert (a.mesh, a.ao, a.samples, a.flip, a.seed) == ("mesh.ply", "out.ply", 64, False, 0) and a.max_dist == math.inf
    a = ap.parse_args(["mesh.ply", "--ao", "out.ply", "--samples", "16", "--flip"])
    assert (a.samples, a.flip) == (16, True)
    for bad in ([], ["mesh.ply"], ["mesh.ply", "--ao"], ["mesh.ply", "--ao", "out.ply", "--samples", "many"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    ap = T.build_parser()
    assert ap.parse_args(["in.ply", "out.obj", "--size", "256"]).ao == 0
    assert ap.parse_args(["in.ply", "out.glb", "--cell", "8", "--ao", "16"]).ao == 16
