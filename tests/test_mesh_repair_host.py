"""CPU-side tests of mesh repair (dg-mesh_amd/mesh_repair.py, csrc/mesh_repair.hip): the numpy reference of the GPU tests
(tests/_repair_ref.py) keeps its own invariants on hand-made meshes; the C ABI declares and exports the new entry points and refuses
bad arguments before any HIP call; the Python layer refuses host tensors and bad parameters; the four entry points have the opt-in
keyword; the command line parses."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _edges_ref as E
import _repair_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ("dgm_mesh_orient_scratch_bytes", "dgm_mesh_orient", "dgm_mesh_fill_scratch_bytes", "dgm_mesh_fill_count", "dgm_mesh_fill_emit")


# ---- the reference's own invariants ------------------------------------------------------------------------------------------------
def test_reference_repairs_a_punctured_sphere():
    verts, faces = R.icosphere_without_stars()
    assert not E.report(verts, faces)["watertight"]
    which = np.random.default_rng(1).random(len(faces)) < 1 / 3
    v, f, info = R.repair(verts, R.flip_some(faces, which))
    rep = E.report(v, f)
    assert rep["watertight"] and rep["genus"] == 0 and E.enclosed_volume(v, f) > 0
    assert (info["holes_filled"], info["verts_added"], info["faces_added"], info["boundary_edges"]) == (3, 3, 17, 17)
    assert info["faces_flipped"] == int(which.sum()) and info["unorientable_components"] == 0
    # the fill alone puts back what was cut out, up to the fan's centre
    v2, f2, _ = R.fill(verts, faces)
    assert (v2[:len(verts)].view(np.uint32) == verts.view(np.uint32)).all() and (f2[:len(faces)] == faces).all()
    assert np.allclose(np.linalg.norm(v2[len(verts):], axis=1), 1.0, atol=0.1)  # the centroid of a small ring on the unit sphere


def test_reference_triangular_holes_and_touching_holes():
    verts, faces = R.icosphere_without_faces()
    v, f, info = R.fill(verts, faces)
    assert (info["holes_filled"], info["verts_added"], info["faces_added"], info["boundary_edges"]) == (3, 0, 3, 9)
    assert E.report(v, f)["watertight"] and len(v) == len(verts)
    verts, faces = R.touching_holes()
    v, f, info = R.fill(verts, faces)
    assert (info["boundary_edges"], info["edges_on_open_chains"], info["holes_filled"], info["faces_added"]) == (6, 6, 0, 0)
    assert (f == faces).all()


def test_reference_orientation_rules():
    verts, faces = E.icosphere(2)
    out, flipped, info = R.orient(verts, R.flip_some(faces, np.ones(len(faces), bool)))
    assert (out == faces).all() and flipped.all() and info["components_inverted"] == 1 and info["closed_components"] == 1
    out, flipped, info = R.orient(verts, R.flip_some(faces, np.ones(len(faces), bool)), outward=False)
    assert not flipped.any() and info["components_inverted"] == 0 and info["outward_skipped"] == 0
    verts, faces = R.moebius()
    out, flipped, info = R.orient(verts, faces)
    assert (out == faces).all() and not flipped.any()
    assert (info["components"], info["unorientable_components"], info["closed_components"]) == (1, 1, 0)
    assert E.report(verts, faces)["boundary_edges"] == 2 * 20 and E.report(verts, faces)["misoriented_edges"] == 1
    verts, faces = E.same_winding_pair()
    assert R.orient(verts, faces)[1].tolist() == [False, True]  # the tie keeps face 0
    verts, faces = R.isolated_triangles(5)
    v, f, info = R.repair(verts, faces)
    assert (f[5:] == faces[:, [1, 0, 2]]).all() and E.report(v, f)["watertight"] and info["components"] == 5


def test_reference_limit_and_wheel():
    verts, faces = E.wheel(12)
    assert R.fill(verts, faces, 11)[2]["holes_too_long"] == 1 and R.fill(verts, faces, 11)[2]["faces_added"] == 0
    v, f, info = R.fill(verts, faces, 12)
    assert (info["holes_filled"], info["verts_added"], info["faces_added"]) == (1, 1, 12) and E.report(v, f)["watertight"]
    ring = verts[1:].astype(np.float64)
    s = np.zeros(3)
    for p in ring:  # the leader is the half-edge of the edge (1, 2), whose tail is vertex 1: loop order is 1, 2, ..., 12
        s = s + p
    assert (v[-1].view(np.uint32) == (s / 12.0).astype(np.float32).view(np.uint32)).all()


def test_volume_sum_fits_int64_at_the_stated_bound():
    assert (6 << 30) * (1 << 28) < 2 ** 61 < 2 ** 63
    rng = np.random.default_rng(0)
    verts = (rng.uniform(-1, 1, (200, 3)) * [1e3, 1.0, 1e-3] + [5e5, -7.0, 0.0]).astype(np.float32)
    faces = rng.integers(0, 200, (500, 3)).astype(np.int32)
    ok = E.valid_faces(faces, 200)
    lo, shift = R.box_of_used(verts, faces, ok)
    x = verts.astype(np.float64)
    terms = [R.volume_term(x[a] - lo, x[b] - lo, x[c] - lo, shift) for a, b, c in faces[ok]]
    assert max(abs(t) for t in terms) <= 6 << 30 and any(terms)
    swapped = [R.volume_term(x[a] - lo, x[c] - lo, x[b] - lo, shift) for a, b, c in faces[ok]]
    assert swapped == [-t for t in terms]  # turning a face negates its term exactly: the sum's sign is the orientation's
    for side, e in ((1.0, 0), (1.5, 1), (2.0, 1), (0.75, 0), (0.5, -1), (3e-5, -15)):
        box = R.box_of_used(np.array([[0, 0, 0], [side, 0, 0], [0, side / 2, 0]], np.float32), np.array([[0, 1, 2]]), np.array([True]))
        assert box[1] == 30 - 3 * e, side
    assert R.box_of_used(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), np.array([True])) is None  # no extent
    assert R.box_of_used(np.array([[0, 0, 0], [np.inf, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]), np.array([True])) is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name


def test_c_abi_argument_errors_without_gpu():
    lib = pkg("_lib").lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast((ctypes.c_int * 64)(), ctypes.c_void_p)
    err = lambda: lib.dgm_last_error()
    big = (1 << 28) + 1
    assert lib.dgm_mesh_orient_scratch_bytes(-1, 0) == 0 and lib.dgm_mesh_orient_scratch_bytes(0, -1) == 0
    assert lib.dgm_mesh_orient_scratch_bytes(4, big) == 0  # unsupported
    assert lib.dgm_mesh_orient_scratch_bytes(1000, 2000) >= 2000 * 37 and lib.dgm_mesh_orient_scratch_bytes(0, 0) > 0
    assert lib.dgm_mesh_fill_scratch_bytes(-1, 0) == 0 and lib.dgm_mesh_fill_scratch_bytes(0, -1) == 0
    assert lib.dgm_mesh_fill_scratch_bytes(1000, 300) >= 1000 * 20 + 300 * 52 and lib.dgm_mesh_fill_scratch_bytes(0, 0) > 0
    orient = lambda V, F, verts, faces, es, s, out, fl, info: lib.dgm_mesh_orient(V, F, verts, faces, es, s, 1, out, fl, info, None)
    assert orient(-1, 0, p, p, p, p, q, p, p) != 0 and b"V >= 0" in err()
    assert orient(4, -1, p, p, p, p, q, p, p) != 0 and b"F >= 0" in err()
    assert orient(4, big, p, p, p, p, q, p, p) != 0 and b"over the supported" in err()
    for args in ((None, p, p, p, q, p, p), (p, None, p, p, q, p, p), (p, p, None, p, q, p, p), (p, p, p, None, q, p, p), (p, p, p, p, None, p, p),
                 (p, p, p, p, q, None, p), (p, p, p, p, q, p, None)):
        assert orient(4, 2, *args) != 0 and b"NULL" in err()
    assert orient(4, 2, p, p, p, p, p, p, p) != 0 and b"must not be faces" in err()
    count = lambda V, F, B, verts, es, m, s, info: lib.dgm_mesh_fill_count(V, F, B, verts, es, None, m, s, info, None)
    assert count(-1, 0, 0, p, p, 10, p, p) != 0 and b"V >= 0" in err()
    assert count(4, 2, -1, p, p, 10, p, p) != 0 and b"B <= 3 F" in err()
    assert count(4, 2, 7, p, p, 10, p, p) != 0 and b"B <= 3 F" in err()
    assert count(4, 2, 3, p, p, -1, p, p) != 0 and b"max_hole_edges" in err()
    for args in ((None, p, 10, p, p), (p, None, 10, p, p), (p, p, 10, None, p), (p, p, 10, p, None)):
        assert count(4, 2, 3, *args) != 0 and b"NULL" in err()
    emit = lambda V, F, B, verts, faces, s, nv, nf, vo, fo: lib.dgm_mesh_fill_emit(V, F, B, verts, faces, s, nv, nf, vo, fo, None)
    assert emit(4, -1, 0, p, p, p, 0, 0, q, q) != 0 and b"F >= 0" in err()
    assert emit(4, 2, 7, p, p, p, 0, 0, q, q) != 0 and b"B <= 3 F" in err()
    assert emit(4, 2, 3, p, p, p, 4, 0, q, q) != 0 and b"nv <= B" in err()
    assert emit(4, 2, 3, p, p, p, 0, -1, q, q) != 0 and b"nf <= B" in err()
    assert emit((1 << 31) - 2, 2, 3, p, p, p, 3, 3, q, q) != 0 and b"int32 range" in err()
    for args in ((None, p, p, 1, 3, q, q), (p, None, p, 1, 3, q, q), (p, p, None, 1, 3, q, q), (p, p, p, 1, 3, None, q), (p, p, p, 1, 3, q, None)):
        assert emit(4, 2, 3, *args) != 0 and b"NULL" in err()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_host_tensors():
    M = pkg("mesh_repair")
    verts, faces = torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    for call in (lambda: M.orient_faces(verts, faces), lambda: M.orient_faces(verts, faces, outward=False), lambda: M.fill_holes(verts, faces),
                 lambda: M.fill_holes(verts, faces, max_hole_edges=5), lambda: M.repair_mesh(verts, faces),
                 lambda: M.repair_mesh(verts, faces, orient=False), lambda: M.apply({"max_hole_edges": 3}, verts, faces),
                 lambda: M.apply(M.RepairSpec(outward=False), verts, faces, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for bad in (-1, 2.5, 2 ** 31, True):
        with pytest.raises(ValueError, match="max_hole_edges"):
            M.fill_holes(verts, faces, max_hole_edges=bad)
        with pytest.raises(ValueError, match="max_hole_edges"):
            M.repair_mesh(verts, faces, max_hole_edges=bad)
    for fn, names, defaults in ((M.orient_faces, ("outward",), [True]), (M.fill_holes, ("max_hole_edges",), [1000]),
                                (M.repair_mesh, ("orient", "outward", "max_hole_edges"), [True, True, 1000])):
        sig = inspect.signature(fn).parameters
        assert list(sig) == ["verts", "faces", *names] and [sig[k].default for k in names] == defaults
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names)
    assert M.ORIENT_FIELDS == R.ORIENT_FIELDS and M.FILL_FIELDS == R.FILL_FIELDS
    for fn, words in ((M.orient_faces, ("inner shells",)), (M.fill_holes, ("centroid", "NOT a minimum-weight triangulation"))):
        assert all(w in " ".join(fn.__doc__.split()) for w in words)  # stated where the function is


def test_repair_spec():
    M = pkg("mesh_repair")
    verts, faces = torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    assert M.as_spec(None) is None and M.as_spec({"max_hole_edges": 30, "outward": False}) == M.RepairSpec(outward=False, max_hole_edges=30)
    d = M.RepairSpec()
    assert (d.orient, d.outward, d.max_hole_edges) == (True, True, 1000) and M.as_spec(d) is d
    assert "max_hole_edges 1000" in d.describe()
    with pytest.raises(TypeError):
        M.as_spec("fill")
    with pytest.raises(TypeError):
        M.as_spec({"holes": 3})
    with pytest.raises(Exception):  # frozen
        M.RepairSpec().orient = False
    assert M.apply(None, verts, faces, None) == (verts, faces, None)  # "do nothing" hands the inputs back


def test_entry_points_have_the_opt_in_keyword():
    for fn in (pkg("visualize").export_dynamic_mesh, pkg("evaluate").testing, pkg("trainer").MeshPhase.extract_mesh,
               pkg("correspondence").export_correspondence):
        params = inspect.signature(fn).parameters
        assert params["repair"].default is None
        names = list(params)
        assert names.index("repair") == names.index("smooth") + 1
        doc = " ".join(fn.__doc__.split())
        assert "repair:" in doc and "LAST, after `simplify`" in doc  # the order is stated where the keyword is
    assert "repair" not in inspect.signature(pkg("trainer").Trainer.__init__).parameters  # never inside the training step


def test_command_line_parses():
    M = pkg("mesh_repair")
    ap = M.build_parser()
    a = ap.parse_args(["in.ply", "out.ply"])
    assert (a.input, a.output) == ("in.ply", "out.ply") and M.spec_from_args(a) == M.RepairSpec()
    a = ap.parse_args(["a", "b", "--max_hole_edges", "30", "--no_orient", "--no_outward"])
    assert M.spec_from_args(a) == M.RepairSpec(orient=False, outward=False, max_hole_edges=30)
    for bad in (["a"], ["a", "b", "--max_hole_edges", "x"], ["a", "b", "--outward"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
