"""CPU-side tests of the mesh cleaning layer (dg-mesh_amd/mesh_clean.py, csrc/mesh_clean.hip): the numpy reference of the GPU tests
labels as scipy does, the C ABI declares and exports the new entry points and refuses bad arguments before any HIP call, the Python
layer refuses host tensors, and the evaluation's command line knows the three component flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _meshclean_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ("dgm_mesh_clean_tile", "dgm_mesh_cc_scratch_bytes", "dgm_mesh_cc_label", "dgm_mesh_cc_stats",
               "dgm_mesh_cc_select_scratch_bytes", "dgm_mesh_cc_select", "dgm_mesh_compact_scratch_bytes", "dgm_mesh_compact_count",
               "dgm_mesh_compact_emit")


@pytest.mark.parametrize("V,F,seed", [(1, 0, 0), (7, 3, 1), (200, 60, 2), (200, 400, 3), (1000, 350, 4), (50, 500, 5)])
def test_reference_labels_equal_scipy(V, F, seed):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.RandomState(seed)
    faces = rng.randint(0, V, (F, 3)).astype(np.int32)  # an index soup: repeated indices and duplicated faces occur
    ok = R.valid_faces(faces, V)
    e = np.concatenate([faces[ok][:, [0, 1]], faces[ok][:, [1, 2]], faces[ok][:, [2, 0]]]).astype(np.int64)
    adj = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    _, comp = connected_components(adj, directed=False)
    first = np.full(comp.max() + 1, V, np.int64)
    np.minimum.at(first, comp, np.arange(V))
    assert np.array_equal(R.labels(faces, V), first[comp].astype(np.int32))


def test_reference_compaction_and_selection_by_hand():
    # two triangles sharing vertex 2 (one component, label 0), a far triangle (label 5), vertex 8 unused, one degenerate face
    verts = np.arange(27, dtype=np.float32).reshape(9, 3)
    faces = np.array([[2, 1, 0], [2, 3, 4], [5, 6, 7], [3, 3, 4]], np.int32)
    lab = R.labels(faces, 9)
    assert lab.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 8]
    t = R.table(verts, faces, lab)
    assert t["label"].tolist() == [0, 5, 8] and t["faces"].tolist() == [2, 1, 0] and t["verts"].tolist() == [5, 3, 1]
    assert t["bbox_min"][1].tolist() == [15.0, 16.0, 17.0] and t["bbox_max"][1].tolist() == [21.0, 22.0, 23.0]
    assert R.keep_mask(verts, faces, lab).tolist() == [1, 1, 1, 0]
    assert R.keep_mask(verts, faces, lab, largest=True).tolist() == [1, 1, 0, 0]
    assert R.keep_mask(verts, faces, lab, min_faces=2).tolist() == [1, 1, 0, 0]
    v, f, vi, fi = R.clean(verts, faces, min_faces=1, largest=False)
    assert vi.tolist() == list(range(8)) and fi.tolist() == [0, 1, 2] and np.array_equal(v, verts[:8])
    v, f, vi, fi = R.compact(verts, faces, [0, 0, 1, 0])
    assert vi.tolist() == [5, 6, 7] and f.tolist() == [[0, 1, 2]] and fi.tolist() == [2]


def test_symbols_are_declared_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "dgmesh_hip.h")).read()
    declared = set(re.findall(r"\b(dgm_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.dgm_mesh_clean_tile() > 0 and lib.dgm_mesh_clean_tile() % 64 == 0


def test_c_abi_argument_errors_without_gpu():
    lib = pkg("_lib").lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dgm_mesh_cc_scratch_bytes(-1, 0) == 0 and lib.dgm_mesh_cc_scratch_bytes(0, -1) == 0
    assert lib.dgm_mesh_cc_scratch_bytes(1000, 10) >= 4000
    assert lib.dgm_mesh_compact_scratch_bytes(-1, 0) == 0 and lib.dgm_mesh_compact_scratch_bytes(1000, 2000) >= 4 * (2 * 1000 + 2000)
    assert lib.dgm_mesh_cc_select_scratch_bytes() >= 32
    assert lib.dgm_mesh_cc_label(-1, 0, None, p, p, p, None) != 0 and b"V >= 0" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_label(4, 1, None, p, p, p, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_label(4, 1, p, None, p, p, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_stats(4, -1, p, p, p, p, p, p, None) != 0 and b"F >= 0" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_stats(4, 1, None, p, p, p, p, p, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_stats(0, 0, None, None, None, None, None, None, None) == 0  # nothing to do
    assert lib.dgm_mesh_cc_select(4, 1, p, p, p, p, p, 0, -1, 0.0, p, p, None) != 0 and b"min_faces" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_select(4, 1, p, p, p, p, p, 0, 0, float("nan"), p, p, None) != 0 and b"min_diameter_frac" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_select(4, 1, p, p, p, p, p, 0, 0, 0.0, p, None, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mesh_cc_select(4, 0, None, None, None, None, None, 1, 0, 0.0, None, None, None) == 0  # F == 0: nothing to do
    assert lib.dgm_mesh_compact_count(4, -2, p, p, p, p, None) != 0 and b"F >= 0" in lib.dgm_last_error()
    assert lib.dgm_mesh_compact_count(4, 1, p, None, p, p, None) != 0 and b"NULL" in lib.dgm_last_error()
    assert lib.dgm_mesh_compact_emit(4, 1, p, p, p, 5, 1, p, p, p, p, None) != 0 and b"Vn <= V" in lib.dgm_last_error()
    assert lib.dgm_mesh_compact_emit(4, 1, p, p, p, 3, 1, None, p, p, p, None) != 0 and b"NULL" in lib.dgm_last_error()


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    M = pkg("mesh_clean")
    verts, faces = torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32)
    for call in (lambda: M.connected_components(faces, 4), lambda: M.component_table(verts, faces), lambda: M.clean_mesh(verts, faces),
                 lambda: M.verts_on_largest_mesh(verts, faces), lambda: M.clean_mesh(verts, faces, largest=True, return_index=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert M.as_spec(None) is None and M.as_spec({"largest": True}) == M.CleanSpec(largest=True)
    assert not M.CleanSpec().any() and M.CleanSpec(min_faces=3).any() and M.CleanSpec(min_diameter_frac=0.1).any()
    with pytest.raises(TypeError):
        M.as_spec("largest")
    # the opt-in switches exist and default to "do nothing"
    import inspect
    for fn in (pkg("visualize").export_dynamic_mesh, pkg("evaluate").testing, pkg("trainer").MeshPhase.extract_mesh,
               pkg("mesh_eval").evaluation):
        assert inspect.signature(fn).parameters["clean"].default is None


def test_cli_parses_the_component_flags():
    E, M = pkg("mesh_eval"), pkg("mesh_clean")
    ap = E.build_parser()
    args = ap.parse_args(["--path", "x", "--eval_type", "dgmesh"])
    assert (args.largest_component, args.min_component_faces, args.min_component_diameter) == (False, 0, 0.0)
    assert E.clean_from_args(args) is None
    args = ap.parse_args(["--path", "x", "--eval_type", "dgmesh", "--largest_component", "--min_component_faces", "25",
                          "--min_component_diameter", "0.05"])
    assert E.clean_from_args(args) == M.CleanSpec(largest=True, min_faces=25, min_diameter_frac=0.05)
    assert E.clean_from_args(ap.parse_args(["--path", "x", "--eval_type", "dgmesh", "--min_component_faces", "2"])) == M.CleanSpec(min_faces=2)
    with pytest.raises(ValueError):
        E.clean_from_args(ap.parse_args(["--path", "x", "--eval_type", "dgmesh", "--min_component_faces", "-2"]))
