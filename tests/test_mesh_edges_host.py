"""CPU-side tests of the edge table and of mesh smoothing (dg-mesh_amd/mesh_topology.py, mesh_smooth.py, csrc/mesh_edges.hip): the
numpy reference of the GPU tests (tests/_edges_ref.py) gives the known answers on hand-made meshes and Taubin smoothing does on a
noisy sphere what it is chosen for; the C ABI declares and exports the new entry points and refuses bad arguments before any HIP
call; the Python layer refuses host tensors and bad parameters; the four entry points have the opt-in keyword; the command lines
parse."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _edges_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ("dgm_mesh_edges_scratch_bytes", "dgm_mesh_edges_count", "dgm_mesh_edges_emit", "dgm_mesh_smooth_step")


# ---- the reference on meshes with known answers ----------------------------------------------------------------------------------------
def test_reference_tetrahedron():
    verts, faces = R.tetrahedron()
    t = R.edge_table(faces, 4)
    assert t["edges"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert (t["edge_count"] == 1).all() and (t["kind"] == R.KIND_REGULAR).all()
    assert t["edge_faces"].tolist()[0] == [0, 1]  # 0->1 in face (0, 1, 2), 1->0 in face (0, 3, 1)
    assert t["adj_offset"].tolist() == [0, 3, 6, 9, 12] and t["adj"].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert (t["vert_flag"] == 1).all()
    rep = R.report(verts, faces)
    assert (rep["edges"], rep["euler"], rep["watertight"], rep["genus"], rep["components"]) == (6, 2, True, 0, 1)


def test_reference_icosphere_and_torus():
    verts, faces = R.icosphere(3)
    assert verts.shape == (642, 3) and faces.shape == (1280, 3)
    rep = R.report(verts, faces)
    assert (rep["edges"], rep["euler"], rep["watertight"], rep["genus"]) == (1920, 2, True, 0)
    assert R.enclosed_volume(verts, faces) > 0  # wound outwards
    verts, faces = R.torus()
    rep = R.report(verts, faces)
    assert rep["watertight"] and rep["euler"] == 0 and rep["genus"] == 1 and rep["components"] == 1


@pytest.mark.parametrize("n,m", [(2, 2), (3, 5), (6, 4)])
def test_reference_grid_patch_has_a_rim(n, m):
    verts, faces = R.grid_patch(n, m)
    t = R.edge_table(faces, n * m)
    rep = R.report(verts, faces)
    assert rep["boundary_edges"] == 2 * (n - 1) + 2 * (m - 1) and not rep["watertight"] and rep["genus"] is None
    assert rep["nonmanifold_edges"] == 0 and rep["misoriented_edges"] == 0 and rep["euler"] == 1
    assert (((t["vert_flag"] & 2) != 0) == R.grid_rim(n, m)).all()
    assert (t["edge_faces"][t["kind"] == R.KIND_BOUNDARY] == -1).sum() == rep["boundary_edges"]  # one side of each is empty


def test_reference_bad_edges():
    verts, faces = R.fan()
    t = R.edge_table(faces, len(verts))
    rep = R.report(verts, faces)
    assert (rep["nonmanifold_edges"], rep["misoriented_edges"], rep["boundary_edges"]) == (1, 0, 6) and not rep["watertight"]
    assert t["edge_count"][0].tolist() == [3, 0] and t["edge_faces"][0].tolist() == [0, -1]
    assert t["vert_flag"].tolist() == [7, 7, 3, 3, 3]
    verts, faces = R.same_winding_pair()
    t = R.edge_table(faces, len(verts))
    rep = R.report(verts, faces)
    assert (rep["nonmanifold_edges"], rep["misoriented_edges"], rep["boundary_edges"]) == (0, 1, 4)
    assert t["edge_count"][0].tolist() == [2, 0] and t["edge_faces"][0].tolist() == [0, -1] and t["kind"][0] == R.KIND_MISORIENTED
    verts, faces = R.bow_tie()
    rep = R.report(verts, faces)
    assert (rep["edges"], rep["boundary_edges"], rep["components"], rep["euler"]) == (6, 6, 1, 1)
    verts, faces = R.wheel(600)
    t = R.edge_table(faces, len(verts))
    assert t["adj_offset"][1] == 600 and t["info"]["edges"] == 1200 and t["info"]["boundary_edges"] == 600


def test_reference_salted_mesh():
    verts, faces, sets = R.salted()
    V = len(verts)
    ok = R.valid_faces(faces, V)
    assert (~ok).sum() == 6 and ok.sum() == 80
    t = R.edge_table(faces, V)
    assert (t["vert_flag"][sets["unused"]] == 0).all() and (np.diff(t["adj_offset"])[sets["unused"]] == 0).all()
    rep = R.report(verts, faces)
    assert (rep["verts"], rep["verts_used"], rep["faces"], rep["faces_valid"], rep["edges"]) == (47, 42, 86, 80, 120)
    assert rep["watertight"] and rep["genus"] == 0 and rep["components"] == 1
    soup_v, soup_f = R.random_soup()
    t = R.edge_table(soup_f, len(soup_v))
    assert t["info"]["nonmanifold_edges"] > 0 and np.diff(t["adj_offset"]).max() > 20
    assert (t["edges"][:, 0] < t["edges"][:, 1]).all() and t["info"]["faces_valid"] < len(soup_f)  # (some triples repeat a corner)


def test_reference_smoothing_is_what_taubin_is_chosen_for():
    """The icosphere of subdivision 3 with its vertices scaled radially by 1 + 0.02 N(0, 1), lam = 0.5, mu = -0.53, 10 iterations: the
    radius' standard deviation is 0.0200 before, 0.0081 after Taubin and 0.0049 after the plain Laplacian; the enclosed volume is
    +0.8 % of the clean sphere's after Taubin and -16 % after the Laplacian, which is why Taubin is the default."""
    clean, faces = R.icosphere(3)
    noisy, _ = R.noisy_icosphere(3, 0.02, 0)
    radius_std = lambda v: float(np.linalg.norm(v.astype(np.float64), axis=1).std())
    vol = R.enclosed_volume(clean, faces)
    taubin = R.smooth(noisy, faces, 10, 0.5, -0.53, "taubin", "fixed")
    laplace = R.smooth(noisy, faces, 10, 0.5, -0.53, "laplacian", "fixed")
    print(f"std of the radius: {radius_std(noisy):.4f} -> Taubin {radius_std(taubin):.4f}, Laplacian {radius_std(laplace):.4f}; volume vs. "
          f"clean: Taubin {R.enclosed_volume(taubin, faces) / vol:.4f}, Laplacian {R.enclosed_volume(laplace, faces) / vol:.4f}")
    assert radius_std(taubin) <= 0.5 * radius_std(noisy)
    assert abs(R.enclosed_volume(taubin, faces) / vol - 1.0) <= 0.02
    assert R.enclosed_volume(laplace, faces) < 0.9 * vol


def test_reference_smoothing_rules():
    verts, faces = R.grid_patch(5, 6, seed=2)
    rim = R.grid_rim(5, 6)
    fixed = R.smooth(verts, faces, 3, boundary="fixed")
    curve = R.smooth(verts, faces, 3, boundary="curve")
    free = R.smooth(verts, faces, 3, method="laplacian", boundary="free")
    assert (fixed[rim].view(np.uint32) == verts[rim].view(np.uint32)).all() and (fixed[~rim] != verts[~rim]).any()
    assert (curve[rim, 2] == 0).all() and (curve[rim, :2] != verts[rim, :2]).any()  # the rim moves, inside its plane
    assert (free[rim, 2] != 0).any()
    assert R.smooth(verts, faces, 0) is not verts and (R.smooth(verts, faces, 0) == verts).all()
    # one step by hand: vertex 7 of the 5 x 6 patch has the neighbours 1, 6, 8, 13, 14 and, across its two diagonals, 0
    t = R.edge_table(faces, 30)
    nb = t["adj"][t["adj_offset"][7]:t["adj_offset"][8]].tolist()
    assert nb == [0, 1, 6, 8, 13, 14]
    x = verts.astype(np.float64)
    s = np.zeros(3)
    for k in nb:
        s = s + x[k]
    expect = (x[7] + 0.5 * (s / 6.0 - x[7])).astype(np.float32)
    assert (R.smooth_step(verts, t, 0.5, "free")[7].view(np.uint32) == expect.view(np.uint32)).all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert L.ABI_VERSION == 5 and lib.dgm_abi_version() == 5


def test_c_abi_argument_errors_without_gpu():
    lib = pkg("_lib").lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.dgm_last_error()
    assert lib.dgm_mesh_edges_scratch_bytes(-1, 0) == 0 and lib.dgm_mesh_edges_scratch_bytes(0, -1) == 0
    assert lib.dgm_mesh_edges_scratch_bytes(4, (1 << 28) + 1) == 0  # unsupported
    assert lib.dgm_mesh_edges_scratch_bytes(1000, 2000) >= 4 * 1000 * 6 + 2000 * (48 + 48 + 24)
    assert lib.dgm_mesh_edges_scratch_bytes(0, 0) > 0
    assert lib.dgm_mesh_edges_count(-1, 0, p, p, p, p, p, None) != 0 and b"V >= 0" in err()
    assert lib.dgm_mesh_edges_count(4, -1, p, p, p, p, p, None) != 0 and b"F >= 0" in err()
    assert lib.dgm_mesh_edges_count(4, (1 << 28) + 1, p, p, p, p, p, None) != 0 and b"over the supported" in err()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.dgm_mesh_edges_count(4, 1, *args, None) != 0 and b"NULL" in err()
    assert lib.dgm_mesh_edges_emit(-1, 0, p, 0, p, p, p, p, p, p, None) != 0 and b"V >= 0" in err()
    assert lib.dgm_mesh_edges_emit(4, 2, p, -1, p, p, p, p, p, p, None) != 0 and b"E <= 3 F" in err()
    assert lib.dgm_mesh_edges_emit(4, 2, p, 7, p, p, p, p, p, p, None) != 0 and b"E <= 3 F" in err()
    assert lib.dgm_mesh_edges_emit(4, 2, None, 3, p, p, p, p, p, p, None) != 0 and b"NULL" in err()
    assert lib.dgm_mesh_edges_emit(4, 2, p, 3, None, p, p, p, p, p, None) != 0 and b"NULL" in err()
    assert lib.dgm_mesh_edges_emit(4, 2, p, 0, p, None, None, None, None, None, None) == 0  # nothing to emit
    assert lib.dgm_mesh_edges_emit(0, 0, p, 0, p, None, None, None, None, None, None) == 0
    step = lambda V, A, vin, off, adj, kind, flag, f, b, out: lib.dgm_mesh_smooth_step(V, A, vin, off, adj, kind, flag, f, b, out, None)
    assert step(-1, 0, p, p, p, p, p, 0.5, 0, p) != 0 and b"V >= 0" in err()
    assert step(4, -1, p, p, p, p, p, 0.5, 0, p) != 0 and b"A >= 0" in err()
    for b in (-1, 3):
        assert step(4, 6, p, p, p, p, p, 0.5, b, p) != 0 and b"boundary" in err()
    for f in (float("nan"), float("inf")):
        assert step(4, 6, p, p, p, p, p, f, 0, p) != 0 and b"finite factor" in err()
    q = ctypes.cast((ctypes.c_int * 64)(), ctypes.c_void_p)
    for args in ((None, p, p, p, p, 0.5, 1, q), (p, None, p, p, p, 0.5, 1, q), (p, p, None, p, p, 0.5, 1, q), (p, p, p, None, p, 0.5, 1, q),
                 (p, p, p, p, None, 0.5, 1, q), (p, p, p, p, p, 0.5, 1, None)):
        assert step(4, 6, *args) != 0 and b"NULL" in err()
    assert step(4, 6, p, p, p, p, p, 0.5, 0, p) != 0 and b"must not be verts_in" in err()
    assert step(0, 0, None, None, None, None, None, 0.5, 0, None) == 0  # nothing to do


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_host_tensors():
    T, S = pkg("mesh_topology"), pkg("mesh_smooth")
    verts, faces = torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    for call in (lambda: T.mesh_edges(faces, 4), lambda: T.mesh_edges(faces, 4, return_faces=True, return_adjacency=True),
                 lambda: T.vertex_flags(faces, 4), lambda: T.topology_report(verts, faces), lambda: S.smooth_mesh(verts, faces),
                 lambda: S.smooth_mesh(verts, faces, iterations=0), lambda: S.apply({"iterations": 2}, verts, faces),
                 lambda: S.apply(S.SmoothSpec(method="laplacian"), verts, faces, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    sig = inspect.signature(T.mesh_edges).parameters
    assert list(sig) == ["faces", "num_verts", "return_faces", "return_adjacency"]
    assert sig["return_faces"].default is False and sig["return_adjacency"].default is False


def test_smooth_spec_and_validation():
    S = pkg("mesh_smooth")
    verts, faces = torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    assert S.as_spec(None) is None and S.as_spec({"iterations": 3, "boundary": "curve"}) == S.SmoothSpec(iterations=3, boundary="curve")
    d = S.SmoothSpec()
    assert (d.iterations, d.lam, d.mu, d.method, d.boundary) == (10, 0.5, -0.53, "taubin", "fixed")
    assert S.as_spec(d) is d
    with pytest.raises(TypeError):
        S.as_spec("taubin")
    with pytest.raises(Exception):  # frozen
        S.SmoothSpec().lam = 0.3
    assert S.apply(None, verts, faces, None) == (verts, faces, None)  # "do nothing" hands the inputs back
    sig = inspect.signature(S.smooth_mesh).parameters
    names = ("iterations", "lam", "mu", "method", "boundary")
    assert [sig[k].default for k in names] == [10, 0.5, -0.53, "taubin", "fixed"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names)
    # every refusal names its parameter, before the tensors are looked at
    for kw, word in (({"iterations": -1}, "iterations"), ({"iterations": 2.5}, "iterations"), ({"lam": 0.0}, "lam"), ({"lam": 1.5}, "lam"),
                     ({"lam": -0.5}, "lam"), ({"lam": float("nan")}, "lam"), ({"mu": -0.5}, "mu"), ({"mu": 0.3}, "mu"),
                     ({"lam": 0.6, "mu": -0.53}, "mu"), ({"mu": float("-inf")}, "mu"), ({"method": "cotan"}, "method"),
                     ({"boundary": "pinned"}, "boundary")):
        with pytest.raises(ValueError, match=word):
            S.smooth_mesh(verts, faces, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):  # the Laplacian does not look at mu; lam = 1 is allowed
        S.smooth_mesh(verts, faces, method="laplacian", mu=5.0, lam=1.0)
    assert S.step_factors(2, 0.5, -0.53, "taubin") == [0.5, -0.53, 0.5, -0.53] and S.step_factors(3, 0.4, -0.53, "laplacian") == [0.4] * 3
    assert S.BOUNDARIES == R.BOUNDARIES


def test_entry_points_have_the_opt_in_keyword():
    for fn in (pkg("visualize").export_dynamic_mesh, pkg("evaluate").testing, pkg("trainer").MeshPhase.extract_mesh,
               pkg("correspondence").export_correspondence):
        params = inspect.signature(fn).parameters
        assert params["smooth"].default is None
        names = list(params)
        assert names.index("smooth") == names.index("simplify") + 1 == names.index("clean") + 2
        assert "BEFORE `simplify`" in " ".join(fn.__doc__.split())  # the order is stated where the keyword is
    assert "smooth" not in inspect.signature(pkg("trainer").Trainer.__init__).parameters  # never inside the training step


def test_command_lines_parse():
    S, T = pkg("mesh_smooth"), pkg("mesh_topology")
    ap = S.build_parser()
    a = ap.parse_args(["in.ply", "out.ply"])
    assert (a.input, a.output) == ("in.ply", "out.ply") and S.spec_from_args(a) == S.SmoothSpec()
    a = ap.parse_args(["a", "b", "--iterations", "3", "--lam", "0.4", "--mu", "-0.45", "--method", "laplacian", "--boundary", "curve"])
    assert S.spec_from_args(a) == S.SmoothSpec(iterations=3, lam=0.4, mu=-0.45, method="laplacian", boundary="curve")
    for bad in (["a"], ["a", "b", "--method", "cotan"], ["a", "b", "--boundary", "pinned"], ["a", "b", "--iterations", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    assert T.build_parser().parse_args(["a.ply", "b.ply"]).meshes == ["a.ply", "b.ply"]
    with pytest.raises(SystemExit):
        T.build_parser().parse_args([])
