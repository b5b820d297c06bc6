"""CPU-side tests of the inside / outside queries (dg-mesh_amd/mesh_inside.py, csrc/mesh_inside.hip, mesh_eval.evaluation_iou): the
numpy reference of the GPU tests (tests/_inside_ref.py) gives the known winding numbers on hand-made meshes and obeys the
zero-contribution rules; the C ABI declares and exports the new entry points and refuses bad arguments before any HIP call; the
Python layer refuses host tensors and bad parameters; the command lines parse."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _edges_ref as E
import _inside_ref as R
import _surface_ref as S
from conftest import ROOT, pkg

NEW_SYMBOLS = ("dgm_wind_scratch_bytes", "dgm_wind_number")
BOTH = (np.float32, np.float64)


def w_of(points, verts, faces, dtype):
    return R.winding(np.asarray(points, np.float32).reshape(-1, 3), verts, faces, dtype)


# ---- the reference against known answers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
def test_reference_sphere(dtype):
    verts, faces = E.icosphere(2)
    assert faces.shape == (320, 3) and E.enclosed_volume(verts, faces) > 0  # wound outwards
    tol = 1e-5 if dtype is np.float32 else 1e-12
    w = w_of([[0, 0, 0], [3, 0, 0], [0.3, -0.2, 0.5], [0, -2.1, 2.1]], verts, faces, dtype)
    assert w.dtype == dtype and np.abs(w - [1, 0, 1, 0]).max() < tol
    w = w_of([[0, 0, 0], [3, 0, 0]], verts, R.reversed_faces(faces), dtype)
    assert np.abs(w - [-1, 0]).max() < tol


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_nested_spheres(dtype):
    verts, faces = E.icosphere(2)
    tol = 1e-5 if dtype is np.float32 else 1e-12
    queries = [[0, 0, 0], [0.7, 0, 0], [0, 0, 1.5]]  # the centre, between the shells (the inner one has radius 0.5), outside
    both = R.join((verts, faces), (verts * np.float32(0.5), faces))
    assert np.abs(w_of(queries, *both, dtype) - [2, 1, 0]).max() < tol
    inner_reversed = R.join((verts, faces), (verts * np.float32(0.5), R.reversed_faces(faces)))
    assert np.abs(w_of(queries, *inner_reversed, dtype) - [0, 1, 0]).max() < tol
    disjoint = R.join((verts, faces), (verts + np.float32([3, 0, 0]), faces))
    assert np.abs(w_of([[0, 0, 0], [3, 0, 0], [1.5, 0, 0]], *disjoint, dtype) - [1, 1, 0]).max() < tol


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_large_triangle_seen_from_close_above(dtype):
    """A point just above the middle of a triangle sees it as half of the sphere: w -> 0.5 from below."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 3 ** 0.5 / 2, 0]], np.float32)  # edge 1, counter-clockwise seen from +z
    faces = np.array([[0, 1, 2]], np.int32)
    centroid = verts.astype(np.float64).mean(0)
    w = w_of([centroid + [0, 0, -1e-3], centroid + [0, 0, 1e-3]], verts, faces, dtype)
    assert 0.45 < w[0] < 0.5 and -0.5 < w[1] < -0.45  # the normal (0, 0, 1) points at the second query: it is outside
    far = w_of([centroid + [0, 0, -100.0]], verts, faces, dtype)
    assert 0 < far[0] < 1e-5


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_open_mesh_degrades_gracefully(dtype):
    verts, faces = R.open_icosphere()
    assert len(faces) == 210
    w = w_of([[0, 0, -0.5], [0, 0, -3], [0, 0, 0.9]], verts, faces, dtype)
    assert 0.5 < w[0] < 1 and abs(w[1]) < 0.1 and w[2] < 0.5  # deep in the bowl, far below it, above the rim's plane


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_marching_cubes_sphere(dtype):
    """What DiffMC produces: watertight, wound outwards, with tiny faces and slivers where the isosurface grazes lattice nodes."""
    verts, faces = S.mc_sphere(1e-3)
    rep = E.report(verts, faces)
    assert rep["watertight"] and rep["genus"] == 0 and E.enclosed_volume(verts, faces) > 0
    centre = verts.astype(np.float64).mean(0)
    queries = R.box_queries(verts, 200, 3)
    w = w_of(np.concatenate([[centre], queries]), verts, faces, dtype)
    assert np.abs(w - np.round(w)).max() < (1e-5 if dtype is np.float32 else 1e-12) and w[0].round() == 1
    radius = np.linalg.norm(verts.astype(np.float64) - centre, axis=1)
    r = np.linalg.norm(queries.astype(np.float64) - centre, axis=1)
    assert (w[1:][r < radius.min() * 0.95].round() == 1).all() and (w[1:][r > radius.max()].round() == 0).all()
    assert (r < radius.min() * 0.95).sum() > 20 and (r > radius.max()).sum() > 20


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_zero_contribution_rules(dtype):
    verts, faces = E.icosphere(2)
    queries = R.box_queries(verts, 50, 0)
    clean = w_of(queries, verts, faces, dtype)
    salted_v, salted_f, salt = R.salted_icosphere(2)
    assert len(salted_f) == len(faces) + len(salt) == 328
    salted = w_of(queries, salted_v, salted_f, dtype)
    # a bad index and a NaN corner add exactly 0; a zero-area face with distinct corner values has a det of rounding noise
    assert np.abs(salted - clean).max() < (1e-5 if dtype is np.float32 else 1e-12)
    assert (w_of(queries, salted_v, salt[:5], dtype) == 0).all()
    assert np.abs(w_of(queries, salted_v, salt[5:], dtype)).max() < (1e-7 if dtype is np.float32 else 1e-15)
    # one face at a time
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float32)
    above = [[0.2, 0.2, -0.5]]
    assert w_of(above, tri, [[0, 1, 2]], dtype)[0] > 0.01
    for bad in ([[0, 1, 5]], [[-1, 1, 2]], [[0, 1, 3]], [[0, 4, 2]], [[0, 1, 1]], [[2, 2, 2]]):  # (b = c and a = b = c: b x c is exactly 0)
        assert w_of(above, tri, bad, dtype)[0] == 0, bad
    in_plane = [[0.2, 0.2, 0], [5, 5, 0], [-1, 0.5, 0], [0, 0, 0], [0.5, 0, 0]]  # inside, outside, beside, on a corner, on an edge
    assert (w_of(in_plane, tri, [[0, 1, 2]], dtype) == 0).all()
    # no faces, no vertices
    assert (w_of(above, tri, np.zeros((0, 3), np.int32), dtype) == 0).all()
    assert (w_of(above, np.zeros((0, 3), np.float32), [[0, 1, 2]], dtype) == 0).all()


@pytest.mark.parametrize("dtype", BOTH)
def test_reference_nan_query(dtype):
    verts, faces = E.icosphere(1)
    w = w_of([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], verts, faces, dtype)
    assert abs(w[0] - 1) < 1e-5 and np.isnan(w[1:]).all()
    assert np.isnan(w_of([[np.nan, 0, 0]], verts, np.zeros((0, 3), np.int32), dtype)).all()


def test_reference_summation_order():
    """The fp32 statement crosses a chunk and a slice boundary; asking a query alone changes no bit; the fp64 statement is the same
    sum up to fp64 rounding whatever the order."""
    verts, faces = E.torus(97, 89)
    assert faces.shape[0] == 17266 == 67 * 256 + 114 and faces.shape[0] > R.CHUNK * R.SLICE_CHUNKS
    queries = R.box_queries(verts, 6, 1)
    w32, w64 = w_of(queries, verts, faces, np.float32), w_of(queries, verts, faces, np.float64)
    assert (w_of(queries[3:4], verts, faces, np.float32).view(np.uint32) == w32[3:4].view(np.uint32)).all()
    assert np.abs(w32 - w64).max() < 1e-4 and np.abs(w64 - np.round(w64)).max() < 1e-9
    shuffled = faces[np.random.default_rng(0).permutation(len(faces))]
    assert np.abs(w_of(queries, verts, shuffled, np.float64) - w64).max() < 1e-12


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"^size_t\s+dgm_wind_scratch_bytes\s*\(", header, flags=re.M)
    assert L.ABI_VERSION == 5 and lib.dgm_abi_version() == 5


def test_c_abi_argument_errors_without_gpu():
    lib = pkg("_lib").lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    err = lambda: lib.dgm_last_error()
    size = lib.dgm_wind_scratch_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(0, 5) == 0 and size(5, 0) == 0
    assert size(1, 1) == 8 and size(1000, 16384) == 8000 and size(1000, 16385) == 16000 and size(3, 17266) == 48
    assert size(1 << 20, 2 ** 31 - 1) == (1 << 20) * 131072 * 8  # size_t arithmetic
    wind = lambda N, V, F, pts, verts, faces, scratch, w: lib.dgm_wind_number(N, V, F, pts, verts, faces, scratch, w, None)
    assert wind(-1, 1, 1, p, p, p, p, p) != 0 and b"N >= 0" in err()
    assert wind(1, -1, 1, p, p, p, p, p) != 0 and b"V >= 0" in err()
    assert wind(1, 1, -1, p, p, p, p, p) != 0 and b"F >= 0" in err()
    assert wind(1, 1, 2 ** 31 - 1, p, p, p, p, p) != 0 and b"too many faces" in err()
    assert wind(0, 4, 2, None, None, None, None, None) == 0  # nothing to do
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, p, None)):
        assert wind(4, 3, 1, *args) != 0 and b"NULL pointer" in err()
    assert wind(4, 3, 16385, p, p, p, None, p) != 0 and b"NULL scratch" in err()
    assert wind(4, 3, 16385, p, p, p, odd, p) != 0 and b"8-byte aligned" in err()
    assert wind(2 ** 31 - 1, 3, 2 ** 31 - 300, p, p, p, p, p) != 0 and b"split N" in err()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_host_tensors_and_bad_parameters():
    M = pkg("mesh_inside")
    pts, verts, faces = torch.zeros(5, 3), torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    for call in (lambda: M.winding_number(pts, verts, faces), lambda: M.contains(pts, verts, faces),
                 lambda: M.contains(pts, verts, faces, threshold=0.3, absolute=True), lambda: M.signed_distance(pts, verts, faces),
                 lambda: M.signed_distance(pts, verts, faces, max_dist=0.5, absolute=True), lambda: M.occupancy_grid(verts, faces, 4),
                 lambda: M.occupancy_grid(verts, faces, 4, lo=(0, 0, 0), hi=(1, 1, 1)), lambda: M.volume_iou(verts, faces, verts, faces),
                 lambda: M.volume_iou(verts, faces, verts, faces, n_points=10, return_points=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    sig = inspect.signature
    assert [(k, v.default) for k, v in sig(M.contains).parameters.items()][3:] == [("threshold", 0.5), ("absolute", False)]
    assert [(k, v.default) for k, v in sig(M.signed_distance).parameters.items()][3:] == [("max_dist", float("inf")), ("absolute", False)]
    assert [(k, v.default) for k, v in sig(M.occupancy_grid).parameters.items()][2:] == [("res", inspect.Parameter.empty), ("lo", None), ("hi", None),
                                                                                           ("absolute", False)]
    assert [(k, v.default) for k, v in sig(M.volume_iou).parameters.items()][4:] == [("n_points", 100000), ("generator", None), ("padding", 0.0),
                                                                                       ("absolute", True), ("return_points", False)]
    ev = sig(pkg("mesh_eval").evaluation_iou).parameters
    assert [(k, v.default) for k, v in ev.items()][3:] == [("n_points", 100000), ("seed", 0), ("clean", None)]
    assert list(sig(pkg("mesh_eval").evaluation).parameters) == ["gt_mesh_path", "eval_mesh_path", "eval_model_type", "emd_sample", "seed", "clean"]
    assert "N x F" in " ".join(M.__doc__.split()) and "pairs" in M.occupancy_grid.__doc__  # the cost is stated where it is paid


def test_batches_keep_the_scratch_below_the_limit():
    M = pkg("mesh_inside")
    lib = pkg("_lib").lib()
    for F in (0, 1, 16384, 16385, 261000, 5_000_000):
        rows = M.batch_rows(F)
        assert rows % 256 == 0 and rows >= 256
        assert lib.dgm_wind_scratch_bytes(rows, F) < M.SCRATCH_LIMIT <= lib.dgm_wind_scratch_bytes(rows + 256, max(F, 1))
    assert M.SLICE_FACES == R.CHUNK * R.SLICE_CHUNKS


def test_evaluation_iou_refuses_before_the_device_is_touched(tmp_path):
    ME = pkg("mesh_eval")
    with pytest.raises(ValueError, match="not supported"):
        ME.evaluation_iou(str(tmp_path), str(tmp_path), "nerfies")
    with pytest.raises(ValueError, match=r"mesh_eval.evaluation_iou: no \*.obj"):
        ME.evaluation_iou(str(tmp_path), str(tmp_path), "dgmesh")
    (tmp_path / "a.obj").write_text("v 0 0 0\n")
    with pytest.raises(ValueError, match="1 ground-truth meshes"):
        ME.evaluation_iou(str(tmp_path), str(tmp_path), "dgmesh")


def test_command_lines_parse():
    M, ME = pkg("mesh_inside"), pkg("mesh_eval")
    ap = M.build_parser()
    a = ap.parse_args(["a.ply", "b.ply"])
    assert (a.mesh_a, a.mesh_b, a.points, a.seed) == ("a.ply", "b.ply", 100000, 0)
    a = ap.parse_args(["a.ply", "b.ply", "--points", "5000", "--seed", "7"])
    assert (a.points, a.seed) == (5000, 7)
    for bad in ([], ["a.ply"], ["a.ply", "b.ply", "c.ply"], ["a.ply", "b.ply", "--points", "many"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    ap = ME.build_parser()
    base = ["--path", "scene", "--eval_type", "dgmesh"]
    assert ap.parse_args(base).iou is None
    assert ap.parse_args(base + ["--iou"]).iou == 100000
    assert ap.parse_args(base + ["--iou", "4096"]).iou == 4096
    assert ap.parse_args(["--iou", "--path", "scene", "--eval_type", "dgmesh"]).iou == 100000
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--iou", "x"])
    text = " ".join(ap.format_help().split())
    assert "--iou [N]" in text and "volumetric IoU" in text and "100000" in text
